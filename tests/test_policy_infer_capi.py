"""The one-role inference entry points of include/t1policy.h (t1policy_actor_forward[_h], t1policy_critic_forward[_h]):
exported, bound by _lib, named in POLICY_EXPORTS, and their argument checks -- every refusal is decided on the host
before any device call, so none of this needs a GPU (the pointers are never dereferenced).  The kernels themselves:
tests/test_gpu_policy_infer.py."""
import ctypes

import pytest

# the heads' compiled layer shapes, (out, in) per layer (t1policy.h: conv2 as (16, 32 * 4))
DIMS = [16, 128, 128, 96, 64, 128, 256, 235, 128, 256, 64, 128, 3, 64, 512, 302, 256, 512, 128, 256, 12, 128, 768, 219,
        256, 768, 128, 256, 1, 128]
P = 64   # a non-null, 16-byte-aligned stand-in for a device pointer
ENTRIES = ("t1policy_actor_forward", "t1policy_actor_forward_h", "t1policy_critic_forward",
           "t1policy_critic_forward_h")


@pytest.fixture(scope="module")
def lib():
    from ti5_isaacgym_amd import _lib
    return _lib.load()


def test_inference_entries_are_exported_and_bound(lib):
    from ti5_isaacgym_amd import _lib
    for name in ENTRIES:
        assert name in _lib.POLICY_EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert len(lib.t1policy_actor_forward.argtypes) == len(lib.t1policy_actor_forward_h.argtypes) == 10
    assert len(lib.t1policy_critic_forward.argtypes) == len(lib.t1policy_critic_forward_h.argtypes) == 8


def test_fragment_buffer_is_unchanged(lib):
    # 1,768 step-tiles of hi + lo fragments and 90 bias tiles: the buffer t1policy_heads_pack fills for every entry
    assert lib.t1policy_heads_frag_bytes() == 1768 * 2 * 64 * 16 + 90 * 4 * 64 * 16


def _actor(lib, entry, batch=8, dims=DIMS, obs_cols=66 * 47, **ptrs):
    a = dict(params=(ctypes.c_uint64 * 31)(*([P] * 31)), dims=None if dims is None else (ctypes.c_int * 30)(*dims),
             frag=P, y1=P, obs=P, mean=P, est_vel=P)
    a.update(ptrs)
    return getattr(lib, entry)(a["params"], a["dims"], a["frag"], a["y1"], a["obs"], obs_cols, a["mean"],
                               a["est_vel"], batch, None)


def _critic(lib, entry, batch=8, dims=DIMS, critic_cols=219, **ptrs):
    a = dict(params=(ctypes.c_uint64 * 31)(*([P] * 31)), dims=None if dims is None else (ctypes.c_int * 30)(*dims),
             frag=P, critic_obs=P, value=P)
    a.update(ptrs)
    return getattr(lib, entry)(a["params"], a["dims"], a["frag"], a["critic_obs"], critic_cols, a["value"], batch, None)


@pytest.mark.parametrize("entry", ["t1policy_actor_forward", "t1policy_actor_forward_h"])
def test_actor_argument_checks(lib, entry, monkeypatch):
    monkeypatch.delenv("T1POLICY_INFER_TILE", raising=False)
    for null in ("params", "dims", "frag", "y1", "obs", "mean", "est_vel"):
        assert _actor(lib, entry, **{null: None}) == -1, null
    assert _actor(lib, entry, batch=-1) == -1
    assert _actor(lib, entry, batch=0) == 0
    assert _actor(lib, entry, dims=DIMS[:-1] + [64]) == 1        # another model
    assert _actor(lib, entry, obs_cols=234) == 1                 # no room for the 235-column short history
    assert _actor(lib, entry, frag=ctypes.c_void_p(72)) == -1    # the fragments are read as 16-byte vectors
    null_param = (ctypes.c_uint64 * 31)(*([P] * 30 + [0]))
    assert _actor(lib, entry, params=null_param) == -1
    if entry.endswith("_h"):   # fp16 rows are read by 16-bit loads: an odd address cannot hold halves
        assert _actor(lib, entry, obs=ctypes.c_void_p(65)) == -1


@pytest.mark.parametrize("entry", ["t1policy_critic_forward", "t1policy_critic_forward_h"])
def test_critic_argument_checks(lib, entry, monkeypatch):
    monkeypatch.delenv("T1POLICY_INFER_TILE", raising=False)
    for null in ("params", "dims", "frag", "critic_obs", "value"):
        assert _critic(lib, entry, **{null: None}) == -1, null
    assert _critic(lib, entry, batch=-1) == -1
    assert _critic(lib, entry, batch=0) == 0
    assert _critic(lib, entry, dims=[16, 127] + DIMS[2:]) == 1
    assert _critic(lib, entry, critic_cols=218) == 1 and _critic(lib, entry, critic_cols=220) == 1
    assert _critic(lib, entry, frag=ctypes.c_void_p(72)) == -1
    null_param = (ctypes.c_uint64 * 31)(*([0] + [P] * 30))
    assert _critic(lib, entry, params=null_param) == -1
    if entry.endswith("_h"):
        assert _critic(lib, entry, critic_obs=ctypes.c_void_p(65)) == -1
