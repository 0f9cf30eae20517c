"""t1env_height_scan on the MI355X: the height scan and the critic-history assembly as ONE launch after the (fused)
step, for fp32 and fp16 histories (terrain.measure_heights = True; inactive in DHT1StandCfg).

  * against the reference's own outputs (tests/golden/heights16.npz): the kernel called directly on buffers filled
    from the fixture;
  * T1DHStandEnv.step() (t1env_step, then the scan) against the explicit split sequence through the C ABI
    (height_scan_util.split_scan_step), which samples root_states between the phases as the reference does;
  * fp16 histories: the fp32 result rounded once, element for element;
  * reset_idx between steps, reset(), and the runner over the 780-wide fp16 critic observation.

Env counts: 5 (less than one 8-env tile) and 97 (odd: fp16 rows 8-byte aligned only, and a ragged last tile of one env).
The terrain is parity_driver.make_env_for's small trimesh (6 x 4 sub-terrains, border 5).
"""
import numpy as np
import pytest
import torch

from golden_util import assert_close, load
from height_scan_util import make_scan_env, split_scan_step, sync_state

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NPRIV, NPTS, CH = 73, 187, 3
W = NPRIV + NPTS


def _scan(env, slot, prev, out, measured):
    from ti5_isaacgym_amd import _lib
    _lib.check(env._lib.t1env_height_scan(env._handle, slot, env._height_pts.data_ptr(), env.num_height_points,
                                          float(env.obs_scales.height_measurements), measured.data_ptr(),
                                          prev.data_ptr(), out.data_ptr(), env._stream()), "t1env_height_scan")


def test_scan_kernel_matches_the_reference_fixture():
    """heights16: 7 recorded steps of the reference's env with the scan on.  An env reset in step t has its recorded
    root after the reset while the scan sampled the one before, so those env-steps are left out of the measured /
    newest-frame comparisons (and only of those): resets per step [1, 1, 7, 0, 4, 0, 0], 13 of 112."""
    from parity_driver import make_env_for
    fx = load("heights16")
    env = make_env_for(fx, DEV)
    n = env.num_envs
    root, reset = fx["step_root_states"], fx["step_reset"]
    priv = fx["step_priv"].reshape(-1, n, CH, W)
    assert priv.shape[0] == 7 and n == 16
    masked = 0
    for t in range(7):
        slot = t & 1
        pose = torch.from_numpy(root[t][:, :7]).to(DEV)
        env.rigid_state[:, 0, :7] = pose
        env.root_states[:, :7] = pose
        env.reset_buf.copy_(torch.from_numpy(reset[t]).to(DEV))
        env._priv[slot].copy_(torch.from_numpy(np.ascontiguousarray(priv[t][:, :, :NPRIV]).reshape(n, CH * NPRIV)).to(DEV))
        prev = torch.from_numpy(priv[t - 1].reshape(n, CH * W)).to(DEV) if t else torch.zeros(n, CH * W, device=DEV)
        out = torch.full((n, CH * W), float("nan"), device=DEV)
        measured = torch.full((n, NPTS), float("nan"), device=DEV)
        _scan(env, slot, prev, out, measured)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(n, CH, W)
        ctx = f" [heights16 step {t}]"
        np.testing.assert_array_equal(got[:, :, :NPRIV], priv[t][:, :, :NPRIV], err_msg="73-wide columns" + ctx)
        np.testing.assert_array_equal(got[:, :2, NPRIV:], priv[t][:, :2, NPRIV:], err_msg="heights frames 0-1" + ctx)
        if reset[t].any():
            assert not got[reset[t], :2, NPRIV:].any()
        keep = ~reset[t]
        masked += int(reset[t].sum())
        np.testing.assert_array_equal(measured.cpu().numpy()[keep], fx["step_measured_heights"][t][keep],
                                      err_msg="measured_heights" + ctx)
        assert_close("priv_heights_scan", got[keep, 2, NPRIV:], priv[t][keep, 2, NPRIV:], ctx=ctx)
    assert masked == 13


def _force_timeouts(env):
    n = env.num_envs
    env.episode_length_buf[::5] = int(env.max_episode_length) - 1 - torch.arange(0, n, 5, device=DEV) % 4


def _pair_fp32(n):
    a, b = make_scan_env(n), make_scan_env(n)
    for e in (a, b):
        e.reset()
        _force_timeouts(e)
    return a, b


def _compare_step_to_split(a, b, t):
    """a: the split sequence's env, b: step()'s.  test_gpu_fused.py's equality: resets exact, float buffers to 1e-5
    relative / 1e-6 absolute (the fused and the split step kernel are two instantiations of the dynamics); the scan's
    samples are int16 x vertical_scale, so they are compared exactly."""
    where = f"step {t}"
    assert torch.equal(a.reset_buf, b.reset_buf), f"{where}: reset_buf differs"
    assert b.privileged_obs_buf.shape == (a.num_envs, CH * W)
    pose_differs = int((a.rigid_state[:, 0, :7] != b.rigid_state[:, 0, :7]).any(1).sum())
    assert torch.equal(a.measured_heights, b.measured_heights), \
        f"{where}: measured_heights differs ({pose_differs} envs with a different pre-reset pose)"
    for f in ("privileged_obs_buf", "obs_buf", "rew_buf"):
        torch.testing.assert_close(getattr(b, f), getattr(a, f), rtol=1e-5, atol=1e-6,
                                   msg=lambda m, f=f: f"{where}: {f}: {m}")
    # what the assembly only copies is bit for bit the split sequence's
    pa, pb = a.privileged_obs_buf.view(-1, CH, W), b.privileged_obs_buf.view(-1, CH, W)
    assert torch.equal(pa[:, :2, NPRIV:], pb[:, :2, NPRIV:]), f"{where}: heights frames 0-1"
    assert torch.equal(pb[:, :, :NPRIV], b._priv[b._slot ^ 1].view(-1, CH, NPRIV)), f"{where}: 73-wide columns"


@pytest.mark.parametrize("n", [5, 97])
def test_step_equals_the_split_sequence(n):
    a, b = _pair_fp32(n)
    g = torch.Generator(device=DEV).manual_seed(2)
    b.set_timing(True)
    resets = 0
    for t in range(12):
        act = 0.3 * torch.randn(n, 12, device=DEV, generator=g)
        sync_state(b, a)
        split_scan_step(a, act)
        b.step(act)
        _compare_step_to_split(a, b, t)
        resets += int(b.reset_buf.sum())
    assert resets > 0 and b.measured_heights.std() > 0
    tm = b.get_timing()
    b.set_timing(False)
    # one launch for the step (no split post-physics kernels) and one for the scan
    assert tm["k_post_a"]["launches"] == 0 and tm["k_post_b"]["launches"] == 0
    assert tm["k_height_scan"]["launches"] == 12


@pytest.mark.parametrize("n", [5, 97])
def test_command_curriculum_step_equals_the_split_sequence(n):
    a, b = _pair_fp32(n)
    for e in (a, b):
        e.common_step_counter = int(e.max_episode_length) - 2
    g = torch.Generator(device=DEV).manual_seed(4)
    b.set_timing(True)
    for t in range(3):
        act = 0.3 * torch.randn(n, 12, device=DEV, generator=g)
        sync_state(b, a)
        split_scan_step(a, act)
        b.step(act)
        _compare_step_to_split(a, b, t)
        assert a.command_ranges["lin_vel_x"] == b.command_ranges["lin_vel_x"]
    tm = b.get_timing()
    b.set_timing(False)
    # the middle step is the curriculum's: its two halves ran split, the other two fused; the scan followed each
    assert tm["k_post_a"]["launches"] == 1 and tm["k_post_b"]["launches"] == 1
    assert tm["k_height_scan"]["launches"] == 3


@pytest.mark.parametrize("n", [5, 97])
def test_fp16_scan_equals_the_fp32_scan_rounded(n, monkeypatch):
    monkeypatch.setenv("T1ENV_DYN_KERNEL", "6")   # one step kernel for both dtypes (as tests/test_gpu_fp16.py)
    e32, e16 = make_scan_env(n, "fp32"), make_scan_env(n, "fp16")
    for e in (e32, e16):
        e.reset()
        _force_timeouts(e)
    g = torch.Generator(device=DEV).manual_seed(2)
    resets = 0
    for t in range(12):
        act = 0.3 * torch.randn(n, 12, device=DEV, generator=g)
        _, p32, _, d32, _ = e32.step(act)
        _, p16, _, d16, _ = e16.step(act)
        assert p16.dtype == torch.float16 and p16.shape == (n, CH * W) and p32.dtype == torch.float32
        assert torch.equal(p16.view(torch.int16), p32.half().view(torch.int16)), f"step {t}: critic history"
        assert e16.measured_heights.dtype == torch.float32
        assert torch.equal(e16.measured_heights, e32.measured_heights), f"step {t}: measured_heights"
        assert torch.equal(d16, d32)
        resets += int(d32.sum())
    assert resets > 0 and e32.measured_heights.std() > 0
    assert p16.view(n, CH, W)[:, :, NPRIV:].float().abs().max() > 0


def test_fp16_resets_between_steps():
    n = 5
    env = make_scan_env(n, "fp16")
    obs, priv = env.reset()
    assert priv.dtype == torch.float16 and priv.shape == (n, CH * W)
    assert not priv.view(n, CH, W)[:, :2, NPRIV:].any()   # reset() cleared the heights history
    g = torch.Generator(device=DEV).manual_seed(6)
    for _ in range(3):
        env.step(0.3 * torch.randn(n, 12, device=DEV, generator=g))
    before = env.privileged_obs_buf.clone()
    assert before.view(n, CH, W)[:, :2, NPRIV:].any()
    env.reset_idx([1, 3])
    after = env.privileged_obs_buf
    assert not after[[1, 3]].any()
    assert torch.equal(after[[0, 2, 4]], before[[0, 2, 4]])
    env.step(0.3 * torch.randn(n, 12, device=DEV, generator=g))
    ext = env.privileged_obs_buf.view(n, CH, W)
    assert not ext[[1, 3], :2, NPRIV:].any()
    assert torch.isfinite(ext[:, 2, NPRIV:].float()).all()
    keep = [i for i in (0, 2, 4) if not bool(env.reset_buf[i])]   # the other rows shifted
    assert torch.equal(ext[keep, :2, NPRIV:], before.view(n, CH, W)[keep, 1:, NPRIV:])
    obs, priv = env.reset()
    assert priv.dtype == torch.float16 and priv.shape == (n, CH * W)
    assert not priv.view(n, CH, W)[:, :2, NPRIV:].any()


def test_injected_physics_with_fp16_and_the_scan_is_refused():
    from ti5_isaacgym_amd import _lib
    env = make_scan_env(4, "fp16")
    with pytest.raises(NotImplementedError, match="injected physics with fp16"):
        env.step(torch.zeros(4, 12, device=DEV), _injected=_lib.Injected())


def test_runner_over_the_fp16_scan():
    """dtype and width plumbing: the 780-wide fp16 critic observation through DHOnPolicyRunner.learn(1)"""
    from ti5_isaacgym_amd import task_registry
    from ti5_isaacgym_amd.algo import DHOnPolicyRunner
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    n = 64
    env = make_scan_env(n, "fp16", seed=5)
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    cfg = class_to_dict(tc)
    cfg["runner"]["num_steps_per_env"] = 4
    cfg["algorithm"]["num_mini_batches"] = 2
    cfg["algorithm"]["num_learning_epochs"] = 1
    # the state estimator's target in the 780-wide critic observation (t1_dh_stand_config.py:460-466)
    e = env.cfg.env
    cfg["algorithm"]["lin_vel_idx"] = (e.single_num_privileged_obs + NPTS) * (e.c_frame_stack - 1) + e.single_linvel_index
    torch.manual_seed(0)
    runner = DHOnPolicyRunner(env, cfg, None, device=DEV)
    first = next(m for m in runner.alg.actor_critic.critic.modules() if isinstance(m, torch.nn.Linear))
    assert first.in_features == CH * W == 780
    losses = []
    update = runner.alg.update
    runner.alg.update = lambda: losses.append(update()) or losses[-1]
    runner.learn(1)
    assert len(losses) == 1 and len(losses[0]) == 3
    assert all(np.isfinite(float(x)) for x in losses[0])
    assert env.privileged_obs_buf.dtype == torch.float16 and env.privileged_obs_buf.shape == (n, 780)
    for p in runner.alg.actor_critic.parameters():
        assert torch.isfinite(p).all()
