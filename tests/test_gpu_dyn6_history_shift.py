"""k_dyn6's history shift and prologue staging across the action ring's slots -- needs the MI355X.

The fused step shifts the observation history (66 frames of 47) and the critic history (3 frames of 73) by one frame
inside k_dyn6: six of its waves move a slice of the workgroup's rows per substep through registers, and the epilogue
writes the newest frame and zeroes the older frames of an env that resets.  The shift copies, so after every step

  * an env that did not reset has obs_buf[:, :-47] equal to the previous step's obs_buf[:, 47:] bit for bit (fp32
    and fp16 histories alike: halves are moved, not converted), and the critic buffer likewise by 73;
  * an env that reset has zeros in those older columns;
  * every output is finite.

Sizes 1, 33 and 65 (one lane of one workgroup, one env over a workgroup, one over two: the ragged last workgroup and
the whole-chunk store's workgroup-boundary rule), decimation 10 (one slice per substep held in registers) and 4 (slices
larger than the hold: the "rest" chunks), six steps, which pass every residue of the 4-slot action ring that W4's
prologue stages, with episodes cut short so that envs reset at different steps.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

NOBS, NPRIV = 47, 73


def _make(n, dtype, decimation):
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        cfg.env.state_dtype = dtype
        cfg.control.decimation = decimation
        cfg.env.episode_length_s = 3.5 * decimation * cfg.sim.dt  # four policy steps
        if decimation != 10:  # the sensor / actuator lag rings are defined for ten substeps
            dr = cfg.domain_rand
            dr.add_lag = dr.add_dof_lag = dr.add_imu_lag = False
    return make_t1_env(num_envs=n, mesh_type="plane", seed=6, device="cuda:0", cfg_hook=hook)


@pytest.mark.parametrize("decimation", [10, 4])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("n", [1, 33, 65])
def test_shift_moves_older_frames_and_reset_zeroes_them(n, dtype, decimation, monkeypatch):
    monkeypatch.setenv("T1ENV_DYN_KERNEL", "6")
    env = _make(n, dtype, decimation)
    assert int(env.max_episode_length) == 4
    obs, priv = env.reset()
    assert obs.shape[1] % NOBS == 0 and priv.shape[1] % NPRIV == 0
    env.episode_length_buf[:] = torch.arange(n, device="cuda:0", dtype=env.episode_length_buf.dtype) % 3
    g = torch.Generator(device="cuda:0").manual_seed(9)
    prev_obs, prev_priv = env.obs_buf.clone(), env.privileged_obs_buf.clone()
    resets = kept = 0
    for t in range(6):
        a = 0.3 * torch.randn(n, 12, device="cuda:0", generator=g)
        obs, priv, rew, done, _ = env.step(a)
        done = done.bool()
        keep = ~done
        for name, buf, prev, f in (("obs", obs, prev_obs, NOBS), ("priv", priv, prev_priv, NPRIV)):
            assert torch.isfinite(buf).all(), f"{name} step {t}"
            torch.testing.assert_close(buf[keep][:, :-f], prev[keep][:, f:], atol=0, rtol=0,
                                       msg=lambda m, name=name: f"{name} step {t}: {m}")
            assert (buf[done][:, :-f] == 0).all(), f"{name} step {t}: a reset env's older frames"
        assert torch.isfinite(rew).all() and torch.isfinite(env.root_states).all() and torch.isfinite(env.dof_state).all()
        resets += int(done.sum())
        kept += int(keep.sum())
        prev_obs, prev_priv = obs.clone(), priv.clone()
    assert resets > 0 and kept > 0
