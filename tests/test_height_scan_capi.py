"""t1env_height_scan (the height scan and the critic-history assembly as one launch after the step), the parts that
need no GPU: the header declares it, the library exports it and the ctypes mirror lists it, argument errors are
reported before any device work, and the env accepts fp16 histories together with the scan."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd import build as b
    b.build()
    return _lib.load()


def test_height_scan_is_declared_exported_and_checks_its_arguments(lib):
    from ti5_isaacgym_amd import _lib
    src = open(os.path.join(REPO, "include", "t1env.h")).read()
    assert ("int t1env_height_scan(t1env* env, int32_t obs_slot, const float* points, int32_t npts, float scale, "
            "float* measured, const void* prev, void* out, void* stream);") in " ".join(src.split())
    assert "t1env_height_scan" in _lib.EXPORTS and hasattr(lib, "t1env_height_scan")
    assert len(lib.t1env_height_scan.argtypes) == 9
    rc = lib.t1env_height_scan(None, 0, None, 187, 5.0, None, None, None, None)
    assert rc == -1   # T1ENV_E_ARG
    assert b"t1env_height_scan" in lib.t1env_last_error()
    # timer id 4 is the scan's (the header's timer list)
    assert re.search(r"4 the height scan \(t1env_height_scan\)", src)


def test_env_accepts_fp16_histories_with_the_scan():
    """state_dtype = 'fp16' with measure_heights = True is no longer refused: construction gets as far as the device
    check (the env runs on the HIP device only)."""
    import ti5_isaacgym_amd as t

    def hook(cfg):
        cfg.env.state_dtype = "fp16"
        cfg.terrain.measure_heights = True
    with pytest.raises(RuntimeError, match="HIP device only") as e:
        t.make_t1_env(num_envs=4, mesh_type="plane", device="cpu", cfg_hook=hook)
    assert not isinstance(e.value, NotImplementedError)
