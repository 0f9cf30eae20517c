"""The depth camera's sensor model on the host: the numpy reference tests/depth_model_ref.py against the statistics the
header promises, the ring's arithmetic, and the model's surface (C ABI, config, play's arguments).  Seeds and frames
are fixed, so every draw here is deterministic."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import depth_model_ref as M  # noqa: E402

# the figure of profiles/depth_model_parity.json that tests/test_gpu_depth_model.py builds its tolerance on
RECORDED_F32_VS_F64 = 1.4914181178937724e-07


def _frame(**kw):
    clean = M.clean_images(64, 48)
    return clean, M.measure(clean, M.params(**kw), frame=0)


def test_noise_has_zero_mean_and_unit_variance():
    _, r = _frame(**M.NOISY)
    g = r["g"].astype(np.float64).ravel()
    n = g.size
    assert n == 5 * 48 * 64
    assert abs(g.mean()) < 5.0 / np.sqrt(n)
    assert abs(g.var() - 1.0) < 0.05
    assert np.abs(g).max() <= 131070 * np.sqrt(3.0) / 65536 + 1e-6   # the tails are cut at 3.464


def test_noise_is_the_integer_sum_times_one_constant():
    """g is exact up to its one multiply: the float32 and float64 evaluations differ by one rounding of that product"""
    clean = M.clean_images(64, 48)
    a = M.measure(clean, M.params(**M.NOISY), 0, np.float32)["g"]
    b = M.measure(clean, M.params(**M.NOISY), 0, np.float64)["g"]
    assert a.dtype == np.float32 and b.dtype == np.float64
    assert np.abs(a - b).max() <= 4 * 2.0 ** -23   # |g| < 4; relative 2^-24 each for the constant and the product


def test_dropout_count_is_binomial():
    clean, r = _frame(p_drop=0.1)
    in_range = ~r["beyond"]
    n = int(in_range.sum())
    k = int(r["drop"].sum())
    assert n > 14000 and abs(k - 0.1 * n) < 5.0 * np.sqrt(n * 0.1 * 0.9)
    assert not (r["drop"] & r["beyond"]).any() and not r["edge"].any()
    assert (r["image"][r["drop"]] == np.float32(-1.0)).all()
    keep = ~r["none"]
    assert np.array_equal(r["image"][keep], clean[keep])   # no sigma: a measured pixel is the clean one


def test_step_image_drops_only_far_side_pixels():
    clean, r = _frame(p_edge=1.0)
    w, h = 64, 48
    want2 = np.zeros((h, w), bool)
    want2[:, w // 2] = True            # env 2: the first column of the far half
    want4 = np.zeros((h, w), bool)
    want4[h // 2, :] = True            # env 4: the first row of the far half
    assert np.array_equal(r["edge"][2], want2) and np.array_equal(r["edge"][4], want4)
    assert not r["edge"][[0, 1, 3]].any()   # ramps, and the far patch (nothing in range comes first) have no shadow
    _, half = _frame(p_edge=0.5)
    assert not (half["edge"] & ~r["edge"]).any()
    k = int(half["edge"].sum())
    n = int(r["edge"].sum())
    assert n == h + w and abs(k - 0.5 * n) < 5.0 * np.sqrt(n * 0.25)


def test_far_pixels_are_fill_and_nothing_else_at_zero_parameters():
    clean, r = _frame()
    assert np.array_equal(r["none"], clean >= np.float32(M.FAR)) and r["none"].sum() > 100
    assert np.array_equal(r["image"], np.where(r["none"], np.float32(-1.0), clean))


def test_noise_grows_with_depth_squared():
    clean = np.stack([np.full((48, 64), 0.5, np.float32), np.full((48, 64), 2.0, np.float32)])
    r = M.measure(clean, M.params(sigma2=0.01), 0, np.float64)
    err = r["image"] - clean
    assert abs(err[0].std() / (0.01 * 0.25) - 1.0) < 0.05 and abs(err[1].std() / (0.01 * 4.0) - 1.0) < 0.05


def test_draws_depend_on_seed_frame_and_env_base():
    clean = M.clean_images(17, 5)
    base = M.measure(clean, M.params(**M.NOISY), 0)["image"]
    assert np.array_equal(base, M.measure(clean, M.params(**M.NOISY), 0)["image"])
    for other in (M.measure(clean, M.params(**M.NOISY), 1), M.measure(clean, M.params(seed=5, **M.NOISY), 0),
                  M.measure(clean, M.params(env_base=1, **M.NOISY), 0)):
        assert not np.array_equal(base, other["image"])
    shifted = M.measure(clean[2:5], M.params(env_base=2, **M.NOISY), 0)["image"]
    assert np.array_equal(shifted, base[2:5])


def test_recorded_float32_difference_covers_the_reference():
    """The GPU test's tolerance is 8 x this figure.  It is the reference's own error, and is recomputed here."""
    assert M.f32_vs_f64() <= RECORDED_F32_VS_F64
    import json
    with open(os.path.join(REPO, "profiles", "depth_model_parity.json")) as f:
        prof = json.load(f)
    assert prof["reference_fp32_vs_fp64"]["max_abs_m"] == RECORDED_F32_VS_F64


@pytest.mark.parametrize("K", [1, 3, 4])
def test_ring_serves_frame_t_minus_lag_and_refills_on_fresh(K):
    n = 4
    lag = np.array([0, 1, 2, 9])
    d = np.clip(lag, 0, K - 1)
    ring = M.Ring(K)
    frames = [np.full((n, 2, 3), 10.0 * t, np.float32) + np.arange(n, dtype=np.float32).reshape(n, 1, 1)
              for t in range(7)]
    born = np.zeros(n, dtype=int)   # the frame at which an env's history began
    for t, fr in enumerate(frames):
        fresh = np.ones(n, np.uint8) if t == 0 else np.array([0, 0, 1, 0], np.uint8) if t == 4 else None
        if fresh is not None:
            born[fresh != 0] = t
        out = ring.push(fr, t, lag, fresh)
        for e in range(n):
            assert np.array_equal(out[e], frames[max(t - d[e], born[e])][e]), (K, t, e)
    assert not (ring.slots == -77.0).any()


def test_c_abi_is_declared_and_exported():
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd import build as b
    src = " ".join(open(os.path.join(REPO, "include", "t1render.h")).read().split())
    assert ("int t1render_depth_model(const t1render_depth_noise* m, const void* clean, int32_t num_envs, int32_t width, "
            "int32_t height, int32_t flags") in src
    for field in ("uint32_t seed;", "int32_t env_base;", "float near, far;", "float sigma0, sigma2;", "float p_drop;",
                  "float p_edge, edge_abs, edge_rel;", "float fill;", "} t1render_depth_noise;"):
        assert field in src, field
    assert "MUST MAKE EVERY ENV FRESH ON THE FIRST CALL" in src
    assert ("t1render_depth_model.hip", "-O3") in b.UNITS
    assert _lib.RENDER_DEPTH_MODEL_EXPORTS == ["t1render_depth_model"] and _lib.RENDER_DEPTH_MAXRING == 16
    assert _lib.C.sizeof(_lib.RenderDepthNoise) == 44
    b.build()
    lib = _lib.load()
    assert len(lib.t1render_depth_model.argtypes) == 13
    # argument errors are reported before any device work
    assert lib.t1render_depth_model(None, None, 1, 4, 4, 0, 0, None, 1, None, None, None, None) == -1
    assert b"t1render_depth_model" in lib.t1env_last_error()


def test_seed_salt_keeps_the_draws_apart_from_the_steps():
    from ti5_isaacgym_amd.utils import render
    assert render.SEED_SALT == M.SEED_SALT != 0
    n = render.DepthNoise(sigma2=0.01, p_drop=0.5)
    packed = n.pack(seed=5, env_base=3, near=0.1, far=3.0)
    assert packed.seed == 5 ^ M.SEED_SALT and packed.env_base == 3
    assert packed.fill == np.float32(3.0) and packed.edge_abs == np.float32(0.05)   # fill None means far
    assert render.DepthNoise(fill=-1.0).pack(0, 0, 0.1, 3.0).fill == -1.0


def test_default_config_has_the_model_switched_off():
    from ti5_isaacgym_amd import task_registry
    cfg, _ = task_registry.get_cfgs("t1_dh_stand")
    dc = cfg.env.depth_camera
    assert dc.enable is False and dc.noise.enable is False and list(dc.latency_frames) == [0, 0]
    nz = dc.noise
    assert (nz.sigma0, nz.sigma2, nz.p_drop, nz.p_edge, nz.edge_abs, nz.edge_rel, nz.fill) == \
        (0.0, 0.0, 0.0, 0.0, 0.05, 0.05, None)


def test_play_refuses_depth_noise_without_depth():
    from ti5_isaacgym_amd.scripts import play
    base = ["--checkpoint", "none.pt"]
    a = play.parse(base + ["--depth", "d"])
    assert a.depth_noise is False and a.depth_latency == [0, 0]
    a = play.parse(base + ["--depth", "d", "--depth_noise", "--depth_latency", "1", "3"])
    assert a.depth_noise is True and a.depth_latency == [1, 3]
    for bad in (["--depth_noise"], ["--depth_latency", "0", "1"], ["--depth", "d", "--depth_latency", "2", "1"],
                ["--depth", "d", "--depth_latency", "-1", "1"], ["--depth", "d", "--depth_latency", "0", "16"]):
        with pytest.raises(ValueError):
            play.parse(base + bad)
