"""The four reward terms DHT1StandCfg leaves at scale 0 (dof_vel_limits, feet_stumble, stand_sysmetry, termination) on
the GPU: the injected step against the reference's own run (tests/golden/rewards28_16.npz), the fused epilogues against
the split kernels with the terms on, and a zero scale against a cfg that never heard of them, bit for bit."""
import numpy as np
import pytest
import torch

import rewards28_util as R28
from golden_util import assert_close, assert_close_nan, load
from test_gpu_fused import CLOSE, EXACT, _sync

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _snapshot(env):
    ex = env.extras.get("episode", {})
    n = env.num_envs
    return dict(
        obs=env.obs_buf[:, -47:].cpu().numpy(), priv=env.privileged_obs_buf.cpu().numpy(), rew=env.rew_buf.cpu().numpy(),
        reset=env.reset_buf.cpu().numpy(), time_out=env.time_out_buf.cpu().numpy(),
        episode_length_buf=env.episode_length_buf.cpu().numpy(), gait_time=env.gait_time.cpu().numpy(),
        commands=env.commands.cpu().numpy(), feet_air_time=env.feet_air_time.cpu().numpy(),
        feet_height=env.feet_height.cpu().numpy(),
        episode_sums=np.stack([env.episode_sums[k].cpu().numpy() if k in env.episode_sums
                               else np.full(n, np.nan, np.float32) for k in R28.REWARD_NAMES]),
        extras_episode=np.array([float(ex["rew_" + k]) if "rew_" + k in ex else np.nan for k in R28.REWARD_NAMES],
                                np.float32))


def test_injected_step_matches_the_reference_with_the_four_terms_on():
    from ti5_isaacgym_amd import make_t1_env
    fx = load("rewards28_16")
    settings = R28.settings_of(fx)
    env = make_t1_env(num_envs=int(fx["num_envs"]), mesh_type="plane", seed=int(fx["seed"]), device=DEV,
                      cfg_hook=lambda cfg: R28.cfg_hook(cfg, settings))
    assert env._episode_sums.shape == (28, env.num_envs) and sorted(env.episode_sums) == R28.REWARD_NAMES
    np.testing.assert_array_equal(env.dof_vel_limits.cpu().numpy(), fx["init_dof_vel_limits"])
    inj = R28.Injector(env, int(fx["synth_seed"]))
    env.reset_idx_all()
    env.step(torch.zeros(env.num_envs, 12, device=env.device), _injected=inj.next())
    outs = [_snapshot(env)]
    env.episode_length_buf = torch.from_numpy(fx["override_episode_length_buf"])
    for t in range(fx["actions"].shape[0]):
        env.step(torch.from_numpy(fx["actions"][t]).to(env.device), _injected=inj.next())
        outs.append(_snapshot(env))
    for t, s in enumerate(outs):
        ctx = f" [rewards28_16 step {t}]"
        for k in ("reset", "time_out", "episode_length_buf", "gait_time"):
            np.testing.assert_array_equal(s[k], fx["step_" + k][t], err_msg=k + ctx)
        for k in ("rew", "obs", "priv", "commands", "feet_air_time", "feet_height"):
            assert_close(k, s[k], fx["step_" + k][t], ctx=ctx)
        assert_close_nan("episode_sums", s["episode_sums"], fx["step_episode_sums"][t], ctx=ctx)
        if t > 0:
            assert_close_nan("extras_episode", s["extras_episode"], fx["step_extras_episode"][t], ctx=ctx)
    # the model's limits are untouched by the reward's override of joints 4 and 9
    np.testing.assert_array_equal(env.dof_vel_limits.cpu().numpy(), fx["init_dof_vel_limits"])


# ---- fused == split, 97 envs (one full k_dyn4 workgroup + a ragged one; three k_dyn5 / k_dyn6 workgroups + one lane)
N_FS = 97
LYING = [5, 40, 96]   # envs put down on the base box: base contact -> termination (no time-out) in the next step
# the base pitched -90 deg so that the base box's front edge is the robot's lowest part (the legs point backwards, 3 cm
# higher), 6 mm into the plane: ~1 kN on the base, nothing on the feet (checked with the CPU build of the dynamics)
LYING_QUAT, LYING_BOX_EDGE, LYING_DEPTH = (0.0, -0.70710678, 0.0, 0.70710678), 0.006, 0.006


def _terms_on(cfg):
    """the fixture's scenario, but the dof_vel_limits penalty starting at ~0.2 rad/s: a robot driven by random actions
    from its start pose does not reach the fixture's 1.7 rad/s within a dozen steps"""
    R28.cfg_hook(cfg, dict(R28.SETTINGS, soft_dof_vel_limit=0.02))


STANDING = list(range(10, 20))   # envs given a zero command: they stand from the first step on (stand_sysmetry)


def _env(hook, fused):
    from ti5_isaacgym_amd import make_t1_env
    env = make_t1_env(num_envs=N_FS, mesh_type="plane", seed=11, device=DEV, cfg_hook=hook)
    env.set_fused(fused)
    env.reset()
    env.episode_length_buf[::7] = int(env.max_episode_length) - 2 - torch.arange(0, N_FS, 7, device=DEV) % 6
    return env


def _lay_down(env, ids):
    r = env.root_states
    r[ids, 2] = env.env_origins[ids, 2] - LYING_BOX_EDGE - LYING_DEPTH
    r[ids, 3:7] = torch.tensor(LYING_QUAT, device=DEV)
    r[ids, 7:13] = 0.0
    env.dof_state.view(env.num_envs, 12, 2)[ids, :, 1] = 0.0
    env.contact_vimp[ids] = 0.0


def test_fused_step_equals_split_sequence_with_the_four_terms_on(dyn_kernel):
    fused, split = _env(_terms_on, True), _env(_terms_on, False)
    split.commands[STANDING, :3] = 0.0
    assert "rew_termination" in (fused.extras["episode"].keys() & split.extras["episode"].keys())
    g = torch.Generator(device=DEV).manual_seed(1)
    terminated = timed_out = 0
    stood = torch.zeros(N_FS, dtype=torch.bool, device=DEV)   # envs whose command was ever within the stand threshold
    thr = split.cfg.commands.stand_com_threshold
    LAY_AT = 3   # not the first step: every env has stepped, and none of LYING is near its time-out (ids % 7 != 0)
    for t in range(12):
        a = torch.randn(N_FS, 12, device=DEV, generator=g)
        if t == LAY_AT:
            _lay_down(split, LYING)
        _sync(fused, split)
        stood |= split.commands[:, :3].norm(dim=1) <= thr
        fused.step(a)
        split.step(a)
        stood |= split.commands[:, :3].norm(dim=1) <= thr
        for f in EXACT:
            assert torch.equal(getattr(fused, f), getattr(split, f)), f"step {t}: {f} differs"
        for f in CLOSE:
            torch.testing.assert_close(getattr(fused, f), getattr(split, f), rtol=1e-5, atol=1e-6,
                                       msg=lambda m, f=f, t=t: f"step {t}: {f}: {m}")
        r = split.reset_buf.bool()
        for env in (fused, split):
            assert not env.obs_buf[r, :-47].any() and not env.privileged_obs_buf[r, :-73].any()
        ef, es = fused.extras["episode"], split.extras["episode"]
        assert ef.keys() == es.keys()
        for k in ef:
            torch.testing.assert_close(torch.as_tensor(ef[k]), torch.as_tensor(es[k]), rtol=1e-5, atol=1e-7)
        term = fused.reset_buf.bool() & ~fused.time_out_buf.bool()
        terminated += int(term.sum())
        timed_out += int(fused.time_out_buf.sum())
        if t == LAY_AT:
            assert term[LYING].all(), "the envs laid on the base box did not terminate"
            assert (fused.rew_buf[term] < 0).any()   # termination is added after the only_positive_rewards clip
            for env in (fused, split):
                assert float(env.extras["episode"]["rew_termination"]) < 0
    assert terminated >= len(LYING) and timed_out > 0
    # the other rows moved too (termination's is zeroed by the reset it comes with: the extras above; a stumble needs a
    # foot pushed sideways, which the injected-physics test provides)
    for k in ("dof_vel_limits", "stand_sysmetry"):
        for env in (fused, split):
            assert (env.episode_sums[k] != 0).any(), k
    assert stood[STANDING].all() and not stood.all()
    assert not fused.episode_sums["stand_sysmetry"][~stood].any(), "stand_sysmetry paid to an env that never stood"


def test_zero_scales_are_bit_identical_to_a_cfg_without_the_terms(dyn_kernel):
    """A term with a zero scale contributes +0.0f and evaluates nothing: with the four scales at 0 (and no
    soft_dof_vel_limit) the fused run equals, bit for bit, the run of an env whose cfg does not define them."""
    def zeros(cfg):
        for k in R28.NEW_TERMS:
            setattr(cfg.rewards.scales, k, 0.0)
    with_zeros, without = _env(zeros, True), _env(None, True)
    assert sorted(with_zeros.episode_sums) == sorted(without.episode_sums) and len(without.episode_sums) == 24
    assert with_zeros.extras["episode"].keys() == without.extras["episode"].keys()
    g = torch.Generator(device=DEV).manual_seed(2)
    for t in range(8):
        a = torch.randn(N_FS, 12, device=DEV, generator=g)
        with_zeros.step(a)
        without.step(a)
        for k, x in with_zeros._keepalive.items():   # every buffer of the C ABI, as bytes (the extras ring starts as NaN)
            assert torch.equal(x.view(torch.uint8), without._keepalive[k].view(torch.uint8)), f"step {t}: {k} differs"
        assert torch.equal(with_zeros.obs_buf, without.obs_buf)
        assert torch.equal(with_zeros.privileged_obs_buf, without.privileged_obs_buf)
    rows = [R28.REWARD_NAMES.index(k) for k in R28.NEW_TERMS]
    assert not with_zeros._episode_sums[rows].any()


def test_reset_idx_reports_and_zeroes_all_28_rows():
    """t1env_reset_idx between steps: extras["episode"] holds the means of all 28 rows over the masked envs (the rows
    behind the new indices moved: torques .. vel_mismatch_exp are now rows 24-27), and the masked envs' rows are zeroed."""
    env = _env(_terms_on, True)
    env.commands[STANDING, :3] = 0.0
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(4):
        env.step(torch.randn(N_FS, 12, device=DEV, generator=g))
    ids = [1, 12, 13, 50, 96]
    sums = env._episode_sums[:, ids].clone()
    for k in ("dof_vel_limits", "stand_sysmetry", "vel_mismatch_exp"):
        assert (sums[R28.REWARD_NAMES.index(k)] != 0).any(), k
    others = [i for i in range(N_FS) if i not in ids]
    kept = env._episode_sums[:, others].clone()
    env.reset_idx(ids)
    ep = env.extras["episode"]
    assert sorted(k for k in ep if k.startswith("rew_")) == sorted("rew_" + k for k in R28.REWARD_NAMES)
    for i, k in enumerate(R28.REWARD_NAMES):
        want = sums[i].double().mean() / env.max_episode_length_s
        torch.testing.assert_close(ep["rew_" + k].double().cpu(), want.cpu(), rtol=1e-5, atol=1e-7, msg=k)
    assert not env._episode_sums[:, ids].any()
    assert torch.equal(env._episode_sums[:, others], kept)
