"""k_dyn6's core wave moves its rows between LDS and registers without changing a bit -- needs the MI355X.

The core wave (W0) reads the other roles' terms, its own joint subspaces and its own state out of LDS rows after S2,
writes the next state there before S1, and keeps its copy of that state in registers across S1.  A row read that was
hoisted across a barrier, or consumed before its writer (or before the read itself has landed), does not fail the
same way twice: what it picks up depends on how the eight waves of the workgroup happen to run.  So the test steps two
envs made from one seed through the same seeded actions for 8 policy steps and requires what the step writes to be
BIT-identical between the two runs: root_states, dof_state, contact_vimp, obs_buf, privileged_obs_buf, rew_buf,
reset_buf.  Episodes last four policy steps and start staggered, so envs reset at different steps and the state the
core wave holds is replaced under it.  (A read that is wrong in the same way every time is what the one-step
kernel-agreement, fp64 dynamics, fused-versus-split and log-identity tests catch.)

Env counts 1 (a single lane), 33 (a ragged second workgroup whose inactive lanes read rows nobody wrote) and 97; the
plane, and the trimesh of tests/test_gpu_dynamics.py; decimation 10, and 4 with the lag rings off (they are defined for
ten substeps).  Every output is finite and at least one env reset.
"""
import pytest
import torch

from test_gpu_dynamics import _terrain_hook

pytestmark = pytest.mark.gpu

FIELDS = ("root_states", "dof_state", "contact_vimp", "obs_buf", "privileged_obs_buf", "rew_buf", "reset_buf")
STEPS = 8


def _make(n, mesh, decimation):
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        if mesh != "plane":
            _terrain_hook(cfg)
        cfg.control.decimation = decimation
        cfg.env.episode_length_s = 3.5 * decimation * cfg.sim.dt  # four policy steps
        if decimation != 10:  # the sensor / actuator lag rings are defined for ten substeps
            dr = cfg.domain_rand
            dr.add_lag = dr.add_dof_lag = dr.add_imu_lag = False
    env = make_t1_env(num_envs=n, mesh_type=mesh, seed=6, device="cuda:0", cfg_hook=hook)
    assert int(env.max_episode_length) == 4
    env.reset()
    env.episode_length_buf[:] = torch.arange(n, device="cuda:0", dtype=env.episode_length_buf.dtype) % 3
    return env


@pytest.mark.parametrize("decimation", [10, 4])
@pytest.mark.parametrize("mesh", ["plane", "trimesh"])
@pytest.mark.parametrize("n", [1, 33, 97])
def test_two_runs_agree_bit_for_bit(n, mesh, decimation, monkeypatch):
    monkeypatch.setenv("T1ENV_DYN_KERNEL", "6")
    envs = [_make(n, mesh, decimation) for _ in range(2)]
    g = torch.Generator(device="cuda:0").manual_seed(9)
    resets = 0
    for t in range(STEPS):
        a = 0.3 * torch.randn(n, 12, device="cuda:0", generator=g)
        for e in envs:
            e.step(a)
        torch.cuda.synchronize()
        for f in FIELDS:
            x, y = getattr(envs[0], f), getattr(envs[1], f)
            assert x.shape == y.shape and x.dtype == y.dtype, f
            if x.is_floating_point():
                assert torch.isfinite(x).all() and torch.isfinite(y).all(), f"step {t}: {f} is not finite"
            assert torch.equal(x, y), (f"step {t}: {f} differs between two runs of the same step in "
                                       f"{int((x != y).sum())} of {x.numel()} elements")
        resets += int(envs[0].reset_buf.sum())
    assert resets > 0, "no env reset"
