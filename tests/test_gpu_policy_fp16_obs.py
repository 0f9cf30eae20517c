"""The rollout's policy forward on fp16 observation histories read in place (cfg.env.state_dtype = "fp16", BASELINE
config 5): k_conv1d_pair_h (t1policy_conv1d_forward_packed_h), k_heads64<fp16> (t1policy_heads_forward_h),
dh_policy.conv1d_direct / heads_forward on fp16 tensors and DHPPO._act_body / act without the fp32 copy.  Needs the
MI355X.

Every input is rounded to fp16 first and every reference is computed from the widened values, so input rounding is
part of no error.  An fp16 value is its own hi part with a zero lo part: the conv keeps the fp32 kernel's bound against
fp64 (tests/test_gpu_policy_conv.py: 1e-5 (1 + |y|)), and the heads stage exactly the fragments the fp32 kernel makes
of the widened inputs, so their outputs are bit-identical to it given the same conv output."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=2e-5, atol=2e-5)     # tests/test_gpu_policy_heads.py's bounds
NAMES = ("mean", "actions", "sigma", "logp", "value")
_MODELS = {}


def _model(scale=1.0):
    """(host copy, device copy) of the t1 policy, default init x scale (test_gpu_policy_heads._model); shared."""
    if scale not in _MODELS:
        from ti5_isaacgym_amd import task_registry
        from ti5_isaacgym_amd.algo.dh_policy import ActorCriticDH
        from ti5_isaacgym_amd.utils.helpers import class_to_dict
        _, tc = task_registry.get_cfgs("t1_dh_stand")
        torch.manual_seed(0)
        ac = ActorCriticDH(235, 47, 219, 12, **class_to_dict(tc)["policy"])
        with torch.no_grad():
            for p in ac.parameters():
                p.mul_(scale)
            ac.std.copy_(torch.linspace(0.2, 1.3, 12))
        _MODELS[scale] = (ac, copy.deepcopy(ac).to(DEV))
    return _MODELS[scale]


def _inputs(n, seed):
    """fp16 obs (n, 3102), critic obs (n, 219) and fp32 eps (n, 12) on the host: randn x 2, obs clamped to +-18."""
    g = torch.Generator().manual_seed(seed)
    obs = (torch.randn(n, 66 * 47, generator=g) * 2.0).clamp(-18, 18).half()
    cobs = (torch.randn(n, 219, generator=g) * 2.0).half()
    eps = torch.randn(n, 12, generator=g)
    return obs, cobs, eps


def _ref64(ac, obs, cobs, eps):
    """The fp64 forward of the widened inputs: mean, actions, sigma, logp, value."""
    from torch.distributions import Normal
    a64 = copy.deepcopy(ac).cpu().double()
    with torch.no_grad():
        o, c, e = obs.double(), cobs.double(), eps.double()
        mean = a64.actor(a64.actor_input(o))
        value = a64.critic(c)
        std = a64.std.expand_as(mean)
        act = mean + std * e
        logp = Normal(mean, std).log_prob(act).sum(-1)
    return mean, act, std, logp, value


def _assert_heads_close(out, ref):
    """out, ref: (mean, actions, sigma, logp, value); test_gpu_policy_heads.py's bounds."""
    mean, act, sigma, logp, value = [t.detach().cpu().double() for t in out]
    rm, ra, rs, rl, rv = [t.detach().cpu().double() for t in ref]
    torch.testing.assert_close(mean, rm, **TOL)
    torch.testing.assert_close(value.reshape(rv.shape), rv, **TOL)
    torch.testing.assert_close(act, ra, **TOL)
    torch.testing.assert_close(sigma, rs.expand_as(sigma), rtol=0, atol=0)
    torch.testing.assert_close(logp, rl, rtol=2e-5, atol=1e-4)


def _conv(scale=1.0, seed=0):
    torch.manual_seed(seed)
    conv = nn.Conv1d(66, 32, kernel_size=6, stride=3)
    with torch.no_grad():
        for p in conv.parameters():
            p.mul_(scale)
    return conv.to(DEV)


def _conv_err(y, x16, conv):
    """max |y - fp64 conv of the widened x| / (1 + |fp64 conv|), channels-last."""
    with torch.no_grad():
        ref = nn.functional.conv1d(x16.double(), conv.weight.double(), conv.bias.double(), stride=3).transpose(1, 2)
    assert y.shape == ref.shape and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    return float(((y.double() - ref).abs() / (1 + ref.abs())).max())


# ---- 1. the conv against fp64
# 1, 2: fewer samples than workgroups could take, every prefetch clamped to the run's last sample; 33, 777: ragged runs;
# 3073 = 3 * (256 CUs * 4 pairs) + 1: the grid is min(batch, 4 pairs per CU), so this is the smallest batch at which a
# workgroup's run reaches a third sample -- the first one loaded into a refilled register buffer and staged into an
# LDS buffer that was read before
@pytest.mark.parametrize("batch", [1, 2, 33, 777, 3073])
def test_conv_fp16_matches_fp64(batch):
    from ti5_isaacgym_amd.algo.dh_policy import conv1d_direct
    conv = _conv()
    g = torch.Generator().manual_seed(batch)
    x = (torch.randn(batch, 66, 47, generator=g) * 2.0).clamp(-18, 18).half().to(DEV)
    y = conv1d_direct(x, conv)
    torch.cuda.synchronize()
    assert y is not None, "no fp16 instance of the history conv"
    err = _conv_err(y, x, conv)
    print(f"batch {batch}: max err / (1 + |y|) = {err:.3e}")
    assert err < 1e-5


def test_conv_fp16_at_the_env_clip_value():
    """+-100.0, the env's observation clip value, with weights x 1.5: one +100 and one -100 at a random place of every
    sample, the way a clip shows up (a saturated entry here and there).  Denser would test the bound, not the kernel:
    every fp32 sum of these 396 products, in any order, carries ~2^-24 sqrt(396) of its partial sums, and at 1 % of the
    inputs on +-100 the partial sums are large enough that the sequential fp32 sum (tools/conv_emulate.py) already
    sits at 1.3e-5 (1 + |y|) where y cancels; with two per sample it sits at 4.4e-6."""
    from ti5_isaacgym_amd.algo.dh_policy import conv1d_direct
    conv = _conv(scale=1.5, seed=1)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(777, 66 * 47, generator=g) * 2.0).clamp(-18, 18)
    pos = torch.randint(0, 66 * 47, (777, 2), generator=g)
    x[torch.arange(777), pos[:, 0]] = 100.0
    x[torch.arange(777), pos[:, 1]] = -100.0
    x = x.view(777, 66, 47).half().to(DEV)
    assert int((x == 100).sum()) >= 700 and int((x == -100).sum()) >= 700
    y = conv1d_direct(x, conv)
    torch.cuda.synchronize()
    err = _conv_err(y, x, conv)
    print(f"+-100 inputs: max err / (1 + |y|) = {err:.3e}")
    assert err < 1e-5


# ---- 2. alignment
def test_conv_fp16_odd_sample_parity_and_refused_base():
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.algo.dh_policy import conv1d_direct, packed_conv_weights
    conv = _conv(seed=2)
    g = torch.Generator().manual_seed(34)
    buf = (torch.randn(34, 66, 47, generator=g) * 2.0).clamp(-18, 18).half().to(DEV)
    x = buf[1:]   # one 6204-byte sample in: every sample's 8- / 4-byte alignment is the other one
    assert buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 12 and x.is_contiguous()
    y = conv1d_direct(x, conv)
    torch.cuda.synchronize()
    err = _conv_err(y, x, conv)
    print(f"base = 12 mod 16: max err / (1 + |y|) = {err:.3e}")
    assert err < 1e-5
    # a base on a 2-byte boundary only: refused by the C entry (-1) and by conv1d_direct (None), nothing launched
    flat = torch.zeros(2 * 66 * 47 + 1, dtype=torch.float16, device=DEV)
    x2 = flat[1:].view(2, 66, 47)
    assert x2.data_ptr() % 4 == 2
    lib = _lib.load()
    sp = torch.cuda.current_stream().cuda_stream
    frag = packed_conv_weights(conv, sp)
    y2 = torch.empty(2, 14, 32, device=DEV)
    assert lib.t1policy_conv1d_forward_packed_h(x2.data_ptr(), frag.data_ptr(), conv.bias.data_ptr(), y2.data_ptr(), 2,
                                                66, 47, 32, 6, 3, sp) == -1
    assert conv1d_direct(x2, conv) is None


# ---- 3. the heads: bit-identical to the fp32 entry on the widened inputs
# 33: one full 32-env tile and one env; 3000: test_gpu_policy_heads.py's ragged batch; at 96 critic_obs is base[1:], so
# its row 0 starts 438 B into the buffer (2-byte aligned only) and the even rows are the odd-aligned ones
@pytest.mark.parametrize("n,shifted", [(33, False), (96, True), (3000, False)])
def test_heads_fp16_equal_fp32_heads_on_widened_inputs(n, shifted):
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.algo.dh_policy import conv1d_direct, packed_heads_weights
    _, acd = _model(1.5)
    obs, cobs, eps = [t.to(DEV) for t in _inputs(n, 300 + n)]
    if shifted:
        base = torch.zeros(n + 1, 219, dtype=torch.float16, device=DEV)
        base[1:] = cobs
        cobs = base[1:]
        assert cobs.data_ptr() % 4 == 2 and cobs.is_contiguous()
    lib = _lib.load()
    sp = torch.cuda.current_stream().cuda_stream
    with torch.inference_mode():
        y1 = conv1d_direct(obs.view(n, 66, 47), acd.long_history[0])
        frag, ptrs, dims = packed_heads_weights(acd, sp)
        obs32, cobs32 = obs.float(), cobs.float().contiguous()

        def run(entry, o, c):
            outs = [torch.full(s, float("nan"), device=DEV) for s in ((n, 12), (n, 12), (n, 12), (n,), (n, 1))]
            rc = entry(ptrs, dims, frag.data_ptr(), y1.data_ptr(), o.data_ptr(), 66 * 47, c.data_ptr(), 219,
                       eps.data_ptr(), *[t.data_ptr() for t in outs], n, sp)
            assert rc == 0, rc
            return outs
        o16 = run(lib.t1policy_heads_forward_h, obs, cobs)
        o32 = run(lib.t1policy_heads_forward, obs32, cobs32)
        torch.cuda.synchronize()
    for name, a, b in zip(NAMES, o16, o32):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), (name, (a - b).abs().max().item())


# ---- 4. end to end against fp64
@pytest.mark.parametrize("n,scale", [(33, 1.0), (1000, 1.5), (3000, 1.0)])
def test_heads_forward_fp16_matches_fp64(n, scale):
    from ti5_isaacgym_amd.algo.dh_policy import heads_forward
    ac, acd = _model(scale)
    obs, cobs, eps = _inputs(n, n)
    with torch.inference_mode():
        out = heads_forward(acd, obs.to(DEV), cobs.to(DEV), eps.to(DEV))
        assert out is not None, "the fused heads have no fp16 instance for the t1 policy"
        m32 = acd.actor(acd.actor_input(obs.float().to(DEV))).cpu().double()   # torch's fp32 layers, widened inputs
        v32 = acd.critic(cobs.float().to(DEV)).cpu().double()
        # mixed dtypes have no instance
        assert heads_forward(acd, obs.to(DEV), cobs.float().to(DEV), eps.to(DEV)) is None
        assert heads_forward(acd, obs.float().to(DEV), cobs.to(DEV), eps.to(DEV)) is None
    ref = _ref64(ac, obs.float(), cobs.float(), eps)
    _assert_heads_close(out, ref)
    mean, value = out[0].cpu().double(), out[4].cpu().double()
    em, ev = (mean - ref[0]).abs().max(), (value - ref[4]).abs().max()
    print(f"n {n} x{scale}: mean err {em:.3e} (torch fp32 {(m32 - ref[0]).abs().max():.3e}), "
          f"value err {ev:.3e} (torch fp32 {(v32 - ref[4]).abs().max():.3e})")
    assert em <= 4 * (m32 - ref[0]).abs().max() + 1e-6
    assert ev <= 4 * (v32 - ref[4]).abs().max() + 1e-6


# ---- 5. NaN
def test_heads_fp16_propagate_nan_to_its_env_only():
    from ti5_isaacgym_amd.algo.dh_policy import heads_forward
    _, acd = _model(1.0)
    n = 96
    obs, cobs, eps = [t.to(DEV) for t in _inputs(n, 7)]
    with torch.inference_mode():
        clean = [t.clone() for t in heads_forward(acd, obs, cobs, eps)]
        obs_n, cobs_n = obs.clone(), cobs.clone()
        obs_n[5, -3] = float("nan")     # the short history: the estimator and the actor
        cobs_n[40, 7] = float("nan")    # the critic
        mean, act, sigma, logp, value = heads_forward(acd, obs_n, cobs_n, eps)
        torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in clean)
    assert torch.isnan(mean[5]).all() and torch.isnan(act[5]).all() and torch.isnan(logp[5])
    assert torch.isnan(value[40]).all()
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[5] = False
    for t, c in ((mean, clean[0]), (act, clean[1]), (logp, clean[3])):
        assert torch.equal(t[keep], c[keep])
    assert torch.equal(sigma, clean[2])
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[40] = False
    assert torch.equal(value[keep], clean[4][keep])


def _alg(scale=1.0):
    from ti5_isaacgym_amd import task_registry
    from ti5_isaacgym_amd.algo.dh_update import DHPPO
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    ac, _ = _model(scale)
    return DHPPO(copy.deepcopy(ac), device=DEV, **class_to_dict(tc)["algorithm"])


def _body(alg, obs, cobs, eps):
    """_act_body's outputs in this file's order: mean, actions, sigma, logp, value."""
    actions, value, logp, mean, sigma = alg._act_body(obs, cobs, eps)
    return mean, actions, sigma, logp, value


# ---- 6. _act_body makes no fp32 copy
def test_act_body_fp16_makes_no_fp32_copy():
    """The widened copy of 4096 histories alone is 50.8 MB; the fp16 path allocates the conv output (7.3 MB) and the
    outputs.  Bound: half of that copy."""
    n = 4096
    alg = _alg()
    obs, cobs, eps = [t.to(DEV) for t in _inputs(n, 6)]
    with torch.inference_mode():
        for _ in range(2):
            alg._act_body(obs, cobs, eps)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        out = _body(alg, obs, cobs, eps)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - start
        print(f"_act_body on fp16 histories at {n} envs: peak - start = {extra / 1e6:.1f} MB")
        assert extra < n * 66 * 47 * 2, extra
        wide = _body(alg, obs.float(), cobs.float(), eps)
    _assert_heads_close(out, wide)


# ---- 7. the graph and the fall-throughs
def test_graphed_act_fp16_replays_the_eager_body():
    n = 1000
    alg = _alg()
    obs, cobs, _ = [t.to(DEV) for t in _inputs(n, 70)]
    with torch.inference_mode():
        alg.act(obs, cobs)
        alg.act(obs, cobs)
        key = (obs.data_ptr(), cobs.data_ptr(), tuple(obs.shape), tuple(cobs.shape))
        assert alg.graph_act and list(alg._act_graphs) == [key]
        _, outs, eps = alg._act_graphs[key]
        assert alg.transition.actions is outs[0]
        eager = alg._act_body(obs, cobs, eps.clone())
        torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b), (a - b).abs().max().item()


def test_act_body_fp16_falls_through_to_the_cast(monkeypatch):
    """fp16 obs one element into its buffer (a base off a 4-byte boundary, which the fp16 conv cannot read:
    conv1d_direct refuses): the fp16 call is refused and the cast path answers;
    FUSED_ACT off: torch's layers on the cast, and the fused path is not tried."""
    from ti5_isaacgym_amd.algo import dh_update
    from ti5_isaacgym_amd.algo.dh_policy import heads_forward
    n = 1000
    alg = _alg()
    ac, _ = _model()
    obs, cobs, eps = _inputs(n, 71)
    ref = _ref64(ac, obs.float(), cobs.float(), eps)
    obs, cobs, eps = obs.to(DEV), cobs.to(DEV), eps.to(DEV)
    buf = torch.zeros(n * 66 * 47 + 1, dtype=torch.float16, device=DEV)
    buf[1:] = obs.reshape(-1)
    odd = buf[1:].view(n, 66 * 47)
    assert odd.data_ptr() % 4 == 2 and odd.is_contiguous() and torch.equal(odd, obs)
    with torch.inference_mode():
        assert heads_forward(alg.actor_critic, odd, cobs, eps) is None
        assert heads_forward(alg.actor_critic, odd.float(), cobs.float(), eps) is not None
        _assert_heads_close(_body(alg, odd, cobs, eps), ref)
        monkeypatch.setattr(dh_update, "FUSED_ACT", False)
        monkeypatch.setattr(dh_update, "heads_forward", lambda *a: pytest.fail("the fused path ran with FUSED_ACT off"))
        _assert_heads_close(_body(alg, obs, cobs, eps), ref)


# ---- 8. from the env
def test_act_on_the_fp16_envs_buffers():
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        cfg.env.state_dtype = "fp16"
    env = make_t1_env(num_envs=64, mesh_type="plane", seed=4, device=DEV, cfg_hook=hook)
    alg = _alg()
    obs, priv = env.reset()
    seen = set()
    with torch.inference_mode():
        for step in range(3):
            assert obs.dtype == torch.float16 and priv.dtype == torch.float16
            actions = alg.act(obs, priv)
            key = (obs.data_ptr(), priv.data_ptr(), tuple(obs.shape), tuple(priv.shape))
            seen.add(key)
            assert key in alg._act_graphs, "act() on the env's fp16 buffers did not run as a graph"
            eps = alg._act_graphs[key][2].clone()
            wide = _body(alg, obs.float(), priv.float(), eps)
            got = (alg.transition.action_mean, actions, alg.transition.action_sigma, alg.transition.actions_log_prob,
                   alg.transition.values)
            _assert_heads_close(got, wide)
            obs, priv, _, _, _ = env.step(actions.clone())
    assert set(alg._act_graphs) == seen and 1 <= len(seen) <= 2
