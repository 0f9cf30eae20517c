"""The one-role launches of the fused heads kernel (t1policy_actor_forward[_h], t1policy_critic_forward[_h],
ti5_isaacgym_amd/csrc/t1policy_heads.hip) and what runs on them: ActorCriticDH.act_inference /
act_inference_with_velocity, DHOnPolicyRunner.get_inference_policy(graphed=...) / get_inference_critic, and
scripts/play.py.  Needs the MI355X.

Batches 1, 33, 65 and 777: a single env, one env past a 32-env tile, one past a 64-env tile, and a ragged tail in both
tilings (777 = 24 x 32 + 9 = 12 x 64 + 9).  The model and inputs are tests/test_gpu_policy_heads.py's (restated here):
_model(scale=1.5), randn * 2 clamped to +-18.

Tolerances: TOL is that file's (split fp16 operands on the matrix cores with fp32 accumulation, ~2^-22 of each product);
the 4 x (torch fp32's error) + 1e-6 bound is the one it holds the mean to."""
import copy
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = dict(rtol=2e-5, atol=2e-5)
DEV = torch.device("cuda:0")
BATCHES = (1, 33, 65, 777)
TILES = ("32", "64")
GUARD = 64          # rows allocated past the batch
SENTINEL = -7.5


def _model(seed=0, scale=1.0):
    from ti5_isaacgym_amd import task_registry
    from ti5_isaacgym_amd.algo.dh_policy import ActorCriticDH
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(seed)
    ac = ActorCriticDH(235, 47, 219, 12, **class_to_dict(tc)["policy"])
    with torch.no_grad():
        for p in ac.parameters():   # trained-policy-like magnitudes on top of the default init
            p.mul_(scale)
        ac.std.copy_(torch.linspace(0.2, 1.3, 12))
    return ac


@functools.lru_cache(maxsize=None)
def _models():
    """(the host model, its copy on the device): built once, never changed by a test."""
    ac = _model(scale=1.5)
    return ac, copy.deepcopy(ac).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _inputs(n):
    g = torch.Generator().manual_seed(4000 + n)
    obs = (torch.randn(n, 66 * 47, generator=g) * 2.0).clamp(-18, 18)
    cobs = torch.randn(n, 219, generator=g) * 2.0
    eps = torch.randn(n, 12, generator=g)
    return obs, cobs, eps


@functools.lru_cache(maxsize=None)
def _ref64(n):
    """The fp64 forward of the model on _inputs(n), and torch's fp32 layers on the device: (mean, est, value) each."""
    ac, acd = _models()
    obs, cobs, _ = _inputs(n)
    a64 = copy.deepcopy(ac).double()
    with torch.no_grad():
        o, c = obs.double(), cobs.double()
        ref = (a64.actor(a64.actor_input(o)), a64.state_estimator(o[:, -235:]), a64.critic(c))
    with torch.inference_mode():
        od, cd = obs.to(DEV), cobs.to(DEV)
        t32 = (acd.actor(acd.actor_input(od)), acd.state_estimator(od[:, -235:]), acd.critic(cd))
    return ref, tuple(t.cpu().double() for t in t32)


def _raw(acd, n, obs_ptr=None, obs_cols=66 * 47, cobs_ptr=None, y1=None, half=False, obs=None, cobs=None):
    """The C entries on raw pointers, the outputs allocated with GUARD sentinel rows past the batch: returns the whole
    (n + GUARD)-row mean, est and value buffers.  obs / cobs: device tensors (obs also feeds the first conv unless y1
    is given); obs_ptr / cobs_ptr override the addresses the entries read."""
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.algo.dh_policy import conv1d_direct, packed_heads_weights
    lib = _lib.load()
    sp = torch.cuda.current_stream().cuda_stream
    with torch.inference_mode():
        frag, ptrs, dims = packed_heads_weights(acd, sp)
        mean = torch.full((n + GUARD, 12), SENTINEL, device=DEV)
        est = torch.full((n + GUARD, 3), SENTINEL, device=DEV)
        value = torch.full((n + GUARD, 1), SENTINEL, device=DEV)
        if obs is not None or obs_ptr is not None:
            if y1 is None:
                y1 = conv1d_direct(obs.view(n, 66, 47), acd.long_history[0])
            fn = lib.t1policy_actor_forward_h if half else lib.t1policy_actor_forward
            rc = fn(ptrs, dims, frag.data_ptr(), y1.data_ptr(), obs_ptr or obs.data_ptr(), obs_cols, mean.data_ptr(),
                    est.data_ptr(), n, sp)
            assert rc == 0, rc
        if cobs is not None or cobs_ptr is not None:
            fn = lib.t1policy_critic_forward_h if half else lib.t1policy_critic_forward
            rc = fn(ptrs, dims, frag.data_ptr(), cobs_ptr or cobs.data_ptr(), 219, value.data_ptr(), n, sp)
            assert rc == 0, rc
        torch.cuda.synchronize()
    return mean, est, value


# ---- 1. bit-identity with act()'s kernel, and of the two tilings
@pytest.mark.parametrize("n", BATCHES)
def test_one_role_launches_equal_the_act_kernel(n, monkeypatch):
    from ti5_isaacgym_amd.algo.dh_policy import actor_forward, critic_forward, heads_forward
    _, acd = _models()
    obs, cobs, eps = [t.to(DEV) for t in _inputs(n)]
    got = {}
    with torch.inference_mode():
        mean, _, _, _, value = [t.clone() for t in heads_forward(acd, obs, cobs, eps)]
        for tile in TILES:
            monkeypatch.setenv("T1POLICY_INFER_TILE", tile)
            m, e = actor_forward(acd, obs)
            v = critic_forward(acd, cobs)
            assert m.shape == (n, 12) and e.shape == (n, 3) and v.shape == (n, 1)
            assert torch.equal(m, mean), (tile, (m - mean).abs().max().item())
            assert torch.equal(v, value), (tile, (v - value).abs().max().item())
            got[tile] = (m.clone(), e.clone(), v.clone())
    for name, a, b in zip(("mean", "est_vel", "value"), got["32"], got["64"]):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())


# ---- 2. against fp64
@pytest.mark.parametrize("n", BATCHES)
def test_one_role_launches_match_fp64(n, monkeypatch):
    from ti5_isaacgym_amd.algo.dh_policy import actor_forward, critic_forward
    monkeypatch.delenv("T1POLICY_INFER_TILE", raising=False)
    _, acd = _models()
    obs, cobs, _ = [t.to(DEV) for t in _inputs(n)]
    ref, t32 = _ref64(n)
    with torch.inference_mode():
        mean, est = actor_forward(acd, obs)
        value = critic_forward(acd, cobs)
    for name, got, r, t in zip(("mean", "est_vel", "value"), (mean, est, value), ref, t32):
        got = got.cpu().double()
        err, err32 = (got - r).abs().max().item(), (t - r).abs().max().item()
        print(f"n={n} {name}: max |fused - fp64| = {err:.3e}, max |torch fp32 - fp64| = {err32:.3e}")
        torch.testing.assert_close(t, r, **TOL)
        torch.testing.assert_close(got, r, **TOL)
        assert err <= 4 * err32 + 1e-6, name


# ---- 3. fp16 observations read in place
@pytest.mark.parametrize("n", BATCHES)
def test_fp16_entries_equal_fp32_entries_on_widened_inputs(n, monkeypatch):
    """The _h entries on obs.half() against the fp32 entries on obs.half().float(), given the same first-conv output
    (the conv's own fp16 instance differs from its fp32 one in summation order: tests/test_gpu_policy_fp16_obs.py).
    critic_obs rows are 219 halves, so every other row starts on an odd half; the actor entry is also run on a column
    slice of a wider fp16 buffer (3103 halves per row: every other row starts on an odd half)."""
    from ti5_isaacgym_amd.algo.dh_policy import conv1d_direct
    _, acd = _models()
    obs, cobs, _ = _inputs(n)
    obs16, cobs16 = obs.half().to(DEV), cobs.half().to(DEV)
    obs32, cobs32 = obs16.float(), cobs16.float()
    wide = torch.zeros(n, 66 * 47 + 1, dtype=torch.float16, device=DEV)
    wide[:, 1:] = obs16
    with torch.inference_mode():
        y1 = conv1d_direct(obs16.view(n, 66, 47), acd.long_history[0])
    for tile in TILES:
        monkeypatch.setenv("T1POLICY_INFER_TILE", tile)
        o16 = _raw(acd, n, obs=obs16, cobs=cobs16, y1=y1, half=True)
        o32 = _raw(acd, n, obs=obs32, cobs=cobs32, y1=y1)
        ow = _raw(acd, n, obs_ptr=wide.data_ptr(), obs_cols=66 * 47 + 1, y1=y1, half=True)
        for name, a, b in zip(("mean", "est_vel", "value"), o16, o32):
            assert bool(torch.isfinite(a[:n]).all()), (tile, name)
            assert torch.equal(a, b), (tile, name, (a - b).abs().max().item())
        for name, a, b in zip(("mean", "est_vel"), ow, o16):
            assert torch.equal(a, b), (tile, "wide " + name, (a - b).abs().max().item())


# ---- 4. a NaN stays in its env
@pytest.mark.parametrize("n", BATCHES)
def test_nan_reaches_its_env_only(n, monkeypatch):
    from ti5_isaacgym_amd.algo.dh_policy import actor_forward, critic_forward
    _, acd = _models()
    obs, cobs, _ = [t.to(DEV) for t in _inputs(n)]
    bad = n // 2
    obs_n, cobs_n = obs.clone(), cobs.clone()
    obs_n[bad, -3] = float("nan")     # the short history: the estimator and the actor
    cobs_n[bad, 7] = float("nan")
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[bad] = False
    for tile in TILES:
        monkeypatch.setenv("T1POLICY_INFER_TILE", tile)
        with torch.inference_mode():
            clean = (*actor_forward(acd, obs), critic_forward(acd, cobs))
            dirty = (*actor_forward(acd, obs_n), critic_forward(acd, cobs_n))
        for name, c, d in zip(("mean", "est_vel", "value"), clean, dirty):
            assert bool(torch.isfinite(c).all()), (tile, name)
            assert bool(torch.isnan(d[bad]).all()), (tile, name)
            assert torch.equal(d[keep], c[keep]), (tile, name)


# ---- 5. nothing is written past the batch
@pytest.mark.parametrize("n", BATCHES)
def test_rows_past_the_batch_are_untouched(n, monkeypatch):
    _, acd = _models()
    obs, cobs, _ = [t.to(DEV) for t in _inputs(n)]
    for tile in TILES:
        monkeypatch.setenv("T1POLICY_INFER_TILE", tile)
        for half in (False, True):
            o, c = (obs.half(), cobs.half()) if half else (obs, cobs)
            for name, t in zip(("mean", "est_vel", "value"), _raw(acd, n, obs=o, cobs=c, half=half)):
                assert bool((t[n:] == SENTINEL).all()), (tile, half, name)
                assert bool(torch.isfinite(t[:n]).all()) and not bool((t[:n] == SENTINEL).all()), (tile, half, name)


# ---- 6. which path act_inference takes
def _count(monkeypatch, name):
    from ti5_isaacgym_amd import _lib
    lib = _lib.load()
    real, calls = getattr(lib, name), []
    monkeypatch.setattr(lib, name, lambda *a: (calls.append(1), real(*a))[1])
    return calls


def test_act_inference_routing(monkeypatch):
    from ti5_isaacgym_amd.algo.dh_policy import ActorCriticDH, actor_forward
    monkeypatch.delenv("T1_FUSED_INFERENCE", raising=False)
    monkeypatch.delenv("T1POLICY_INFER_TILE", raising=False)
    acd = _model(seed=5, scale=1.5).to(DEV).eval()
    obs = _inputs(65)[0].to(DEV)
    calls = _count(monkeypatch, "t1policy_actor_forward")
    with torch.no_grad():
        want = actor_forward(acd, obs)[0].clone()
        assert len(calls) == 1
        got = acd.act_inference(obs)
        assert len(calls) == 2 and torch.equal(got, want) and not got.requires_grad
    with torch.inference_mode():
        assert torch.equal(acd.act_inference(obs), want) and len(calls) == 3
    # autograd on: torch's layers, a graph behind the result
    g = acd.act_inference(obs)
    assert len(calls) == 3 and g.requires_grad
    torch.testing.assert_close(g.detach(), want, **TOL)
    # the A/B switch
    monkeypatch.setenv("T1_FUSED_INFERENCE", "0")
    with torch.no_grad():
        t = acd.act_inference(obs)
    assert len(calls) == 3
    torch.testing.assert_close(t, want, **TOL)
    monkeypatch.delenv("T1_FUSED_INFERENCE")
    # a model the kernels have no instance of: torch's layers
    other = ActorCriticDH(235, 47, 219, 12, actor_hidden_dims=[256, 256, 128], critic_hidden_dims=[768, 256, 128],
                          state_estimator_hidden_dims=[256, 128, 64], kernel_size=[6, 4], filter_size=[32, 16],
                          stride_size=[3, 2], lh_output_dim=64).to(DEV).eval()
    with torch.no_grad():
        assert actor_forward(other, obs) is None
        o = other.act_inference(obs)
        assert len(calls) == 3 and o.shape == (65, 12)
        torch.testing.assert_close(o, other.actor(other.actor_input(obs)), rtol=0, atol=0)
    # an in-place parameter change shows in the next call
    with torch.no_grad():
        for p in acd.actor.parameters():
            p.add_(0.01)
        moved = acd.act_inference(obs)
        assert len(calls) == 4 and not torch.allclose(moved, want)
        torch.testing.assert_close(moved, acd.actor(acd.actor_input(obs)), **TOL)


def test_act_inference_with_velocity_is_the_exported_module(monkeypatch):
    from ti5_isaacgym_amd.scripts.export_policy import ExportedDH
    monkeypatch.delenv("T1_FUSED_INFERENCE", raising=False)
    ac, acd = _models()
    obs = _inputs(33)[0]
    calls = _count(monkeypatch, "t1policy_actor_forward")
    exported = torch.jit.script(ExportedDH(ac))
    with torch.no_grad():
        want_mean, want_vel = exported(obs)
        mean, vel = acd.act_inference_with_velocity(obs.to(DEV))
        assert len(calls) == 1
        cpu_mean, cpu_vel = ac.act_inference_with_velocity(obs)      # the host: torch's layers
    assert len(calls) == 1
    torch.testing.assert_close(mean.cpu(), want_mean, **TOL)
    torch.testing.assert_close(vel.cpu(), want_vel, **TOL)
    torch.testing.assert_close(cpu_mean, want_mean, **TOL)
    torch.testing.assert_close(cpu_vel, want_vel, **TOL)
    g_mean, g_vel = acd.act_inference_with_velocity(obs.to(DEV))      # autograd on: torch's layers
    assert len(calls) == 1 and g_mean.requires_grad and g_vel.requires_grad
    torch.testing.assert_close(g_mean.detach().cpu(), want_mean, **TOL)


def test_inference_critic_routing(monkeypatch):
    from ti5_isaacgym_amd.algo.dh_policy import critic_forward
    monkeypatch.delenv("T1_FUSED_INFERENCE", raising=False)
    runner = _runner()
    ac = runner.alg.actor_critic
    critic = runner.get_inference_critic()
    cobs = _inputs(65)[1].to(DEV)
    calls = _count(monkeypatch, "t1policy_critic_forward")
    with torch.no_grad():
        v = critic(cobs)
        assert len(calls) == 1 and torch.equal(v, critic_forward(ac, cobs))
        torch.testing.assert_close(v, ac.evaluate(cobs), **TOL)
        assert len(calls) == 2     # (critic_forward above; evaluate is torch's layers)
    g = critic(cobs)
    assert len(calls) == 2 and g.requires_grad


# ---- 7. the graphed policy
@functools.lru_cache(maxsize=None)
def _runner():
    """A fresh runner over a 64-env fp32 plane env (shared: tests change its weights only in place, by design)."""
    from ti5_isaacgym_amd import DHOnPolicyRunner, make_t1_env, task_registry
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    env = make_t1_env(num_envs=64, mesh_type="plane", seed=4, device=str(DEV))
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(0)
    return DHOnPolicyRunner(env, class_to_dict(tc), None, device=str(DEV))


def test_graphed_inference_replays_the_eager_call(monkeypatch):
    monkeypatch.delenv("T1_FUSED_INFERENCE", raising=False)
    monkeypatch.delenv("T1POLICY_INFER_TILE", raising=False)
    runner = _runner()
    env, ac = runner.env, runner.alg.actor_critic
    policy = runner.get_inference_policy(device=env.device, graphed=True)
    eager = runner.get_inference_policy(device=env.device)
    obs = env.get_observations()
    seen = set()
    with torch.inference_mode():
        for _ in range(4):
            got = policy(obs).clone()
            assert got.shape == (64, 12) and torch.equal(got, eager(obs))
            seen.add((obs.data_ptr(), tuple(obs.shape), obs.dtype))
            obs = env.step(got)[0]
        assert len(seen) == 2 and set(policy.graphs) == seen      # the env's ping-pong pair: one graph each
        before = policy(obs).clone()
        with torch.no_grad():
            for p in ac.actor.parameters():   # what an optimizer step does
                p.add_(0.01)
        after = policy(obs).clone()
        assert not torch.allclose(before, after) and torch.equal(after, eager(obs))
        assert set(policy.graphs) == seen
        with torch.no_grad():
            for p in ac.actor.parameters():
                p.sub_(0.01)


# ---- 8. an fp16 env
def test_inference_policy_on_an_fp16_env():
    """act_inference on the fp16 histories of an env with cfg.env.state_dtype = "fp16" (torch's layers raise on them):
    the fp32 entry on the widened buffer, given the same first-conv output, bit for bit."""
    from ti5_isaacgym_amd import DHOnPolicyRunner, make_t1_env, task_registry
    from ti5_isaacgym_amd.algo.dh_policy import conv1d_direct
    from ti5_isaacgym_amd.utils.helpers import class_to_dict

    def hook(cfg):
        cfg.env.state_dtype = "fp16"
    env = make_t1_env(num_envs=64, mesh_type="plane", seed=4, device=str(DEV), cfg_hook=hook)
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(0)
    runner = DHOnPolicyRunner(env, class_to_dict(tc), None, device=str(DEV))
    policy = runner.get_inference_policy(device=env.device)
    obs = env.get_observations()
    assert obs.dtype == torch.float16
    with torch.inference_mode():
        out = policy(obs)
        y1 = conv1d_direct(obs.view(64, 66, 47), runner.alg.actor_critic.long_history[0])
    assert out.shape == (64, 12) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    wide = _raw(runner.alg.actor_critic, 64, obs=obs.float(), y1=y1)[0][:64]
    assert torch.equal(out, wide), (out - wide).abs().max().item()


# ---- 9. play
def test_play_logs_states_and_rewards(tmp_path):
    from ti5_isaacgym_amd.scripts import play
    ckpt = str(tmp_path / "model_0.pt")
    _runner().save(ckpt)
    out = tmp_path / "play"
    summary = play.main(["--checkpoint", ckpt, "--num_envs", "9", "--steps", "30", "--command", "0.5", "0", "0",
                         "--mesh_type", "plane", "--out", str(out)])
    states = np.load(out / "states.npz")
    assert set(states.files) == set(play.STATE_KEYS)
    for k in play.SCALARS:
        assert states[k].shape == (30,) and np.isfinite(states[k]).all(), k
    for k in play.PER_JOINT:
        assert states[k].shape == (30, 12) and np.isfinite(states[k]).all(), k
    assert (states["command_x"] == 0.5).all() and (states["command_y"] == 0).all() and (states["command_yaw"] == 0).all()
    assert states["base_height"].min() > 0.0
    with open(out / "summary.json") as f:
        loaded = json.load(f)
    assert loaded == json.loads(json.dumps(summary))
    assert loaded["steps"] == 30 and loaded["num_envs"] == 9 and loaded["command"] == [0.5, 0.0, 0.0]
    assert isinstance(loaded["episodes"], int) and loaded["episodes"] >= 0
    assert any(k.startswith("rew_") for k in loaded["mean_episode"])
    for v in loaded["mean_episode"].values():
        assert (v is None) == (loaded["episodes"] == 0)
