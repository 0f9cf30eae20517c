"""The fp16-observation entry points of include/t1policy.h (t1policy_conv1d_forward_packed_h, t1policy_heads_forward_h):
exported, bound by _lib, and their argument checks -- every refusal here is decided on the host before any device
call, so none of this needs a GPU (the pointers are never dereferenced).  The kernels themselves:
tests/test_gpu_policy_fp16_obs.py."""
import ctypes

import pytest

# the heads' compiled layer shapes, (out, in) per layer (t1policy.h: conv2 as (16, 32 * 4))
DIMS = [16, 128, 128, 96, 64, 128, 256, 235, 128, 256, 64, 128, 3, 64, 512, 302, 256, 512, 128, 256, 12, 128, 768, 219,
        256, 768, 128, 256, 1, 128]
P = 64   # a non-null, 16-byte-aligned stand-in for a device pointer


@pytest.fixture(scope="module")
def lib():
    from ti5_isaacgym_amd import _lib
    return _lib.load()


def test_fp16_entries_are_exported_and_bound(lib):
    from ti5_isaacgym_amd import _lib
    for name in ("t1policy_conv1d_forward_packed_h", "t1policy_heads_forward_h"):
        assert name in _lib.POLICY_EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert len(lib.t1policy_conv1d_forward_packed_h.argtypes) == 11
    assert len(lib.t1policy_heads_forward_h.argtypes) == 16


def _conv(lib, x=P, frag=P, bias=P, y=P, batch=8, shape=(66, 47, 32, 6, 3)):
    return lib.t1policy_conv1d_forward_packed_h(x, frag, bias, y, batch, *shape, None)


def test_conv_h_argument_checks(lib):
    for null in ("x", "frag", "bias", "y"):
        assert _conv(lib, **{null: None}) == -1, null
    assert _conv(lib, batch=-1) == -1
    assert _conv(lib, batch=0) == 0
    assert _conv(lib, shape=(66, 47, 32, 5, 3)) == 1     # no compiled instance
    assert _conv(lib, shape=(64, 47, 32, 6, 3)) == 1
    # x is read as dwords: a base off a 4-byte boundary is refused (an fp16 tensor viewed from an odd element)
    assert _conv(lib, x=ctypes.c_void_p(6)) == -1
    assert _conv(lib, x=ctypes.c_void_p(66)) == -1
    assert _conv(lib, frag=ctypes.c_void_p(72)) == -1    # the fragments are read as 16-byte vectors
    # 32-bit byte offsets: batch * 66 * 47 * 2 < 2^31
    assert _conv(lib, batch=2 ** 31 // (66 * 47 * 2) + 1) == -1


def _heads(lib, batch=8, dims=DIMS, obs_cols=66 * 47, critic_cols=219, **ptrs):
    params = (ctypes.c_uint64 * 31)(*([P] * 31))
    d = None if dims is None else (ctypes.c_int * 30)(*dims)
    a = dict(params=params, dims=d, frag=P, y1=P, obs=P, critic_obs=P, eps=P, mean=P, actions=P, sigma=P, logp=P,
             value=P)
    a.update(ptrs)
    return lib.t1policy_heads_forward_h(a["params"], a["dims"], a["frag"], a["y1"], a["obs"], obs_cols,
                                        a["critic_obs"], critic_cols, a["eps"], a["mean"], a["actions"], a["sigma"],
                                        a["logp"], a["value"], batch, None)


def test_heads_h_argument_checks(lib):
    for null in ("params", "dims", "frag", "y1", "obs", "critic_obs", "eps", "mean", "actions", "sigma", "logp",
                 "value"):
        assert _heads(lib, **{null: None}) == -1, null
    assert _heads(lib, batch=-1) == -1
    assert _heads(lib, batch=0) == 0
    assert _heads(lib, dims=DIMS[:-1] + [64]) == 1        # another model
    assert _heads(lib, obs_cols=234) == 1 and _heads(lib, critic_cols=218) == 1
    assert _heads(lib, frag=ctypes.c_void_p(72)) == -1
    # fp16 rows are read by 16-bit loads: any even address is taken, an odd one cannot hold halves
    assert _heads(lib, obs=ctypes.c_void_p(65)) == -1 and _heads(lib, critic_obs=ctypes.c_void_p(65)) == -1
    null_param = (ctypes.c_uint64 * 31)(*([P] * 30 + [0]))
    assert _heads(lib, params=null_param) == -1
