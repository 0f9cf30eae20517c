"""The history shift of every step path that is not k_dyn6's own -- needs the MI355X.

Every env step shifts the observation history (66 frames of 47) and the critic history (3 frames of 73) by one frame.
Outside k_dyn5's and k_dyn6's in-workgroup shifts the copy is one kernel body, launched beside the step kernel or alone
in stream order, so an error in it would be common to the fused and the split step and pass their comparison.  This file
pins the copy itself, as test_gpu_dyn6_history_shift.py does for k_dyn6.  After every step, for both histories,

  * an env that did not reset has buf[:, :-F] equal to the previous step's buf[:, F:] bit for bit (fp32 and fp16
    histories alike: halves are moved, not converted);
  * an env that reset has zeros in those older columns;
  * every output is finite.

Paths: the fused step and the split step (set_fused(False)) under every step kernel of the dyn_kernel fixture, the
injected-physics step (the stand-alone shift after k_physics_injected), and phase B without a phase A
(t1env_step_reset_and_observe alone, which runs the stand-alone shift first and resets again the envs the previous
step reset).

Sizes 1, 9 and 65: less than one 8-row shift unit, a unit plus one row, and a 64-env k_dyn4 workgroup plus one env (two
32-env workgroups plus one lane) -- the smallest sizes with a partial unit, the buffer-end element path and a ragged
last workgroup.  Decimation 10, six steps, with episodes cut short so that envs reset at different steps.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NOBS, NPRIV = 47, 73
SIZES = [1, 9, 65]
DTYPES = ["fp32", "fp16"]
STEPS = 6


def _make(n, dtype):
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        cfg.env.state_dtype = dtype
        cfg.control.decimation = 10
        cfg.env.episode_length_s = 3.5 * 10 * cfg.sim.dt  # four policy steps

    env = make_t1_env(num_envs=n, mesh_type="plane", seed=6, device="cuda:0", cfg_hook=hook)
    assert int(env.max_episode_length) == 4
    return env


def _start(env):
    n = env.num_envs
    obs, priv = env.reset()
    assert obs.shape[1] == NOBS * 66 and priv.shape[1] == NPRIV * 3
    env.episode_length_buf[:] = torch.arange(n, device="cuda:0", dtype=env.episode_length_buf.dtype) % 3
    return env.obs_buf.clone(), env.privileged_obs_buf.clone()


def _assert_shifted(env, prev_obs, prev_priv, done, t):
    """The shift property of the current buffers against the previous step's; returns (resets, kept)."""
    keep = ~done
    for name, buf, prev, f in (("obs", env.obs_buf, prev_obs, NOBS), ("priv", env.privileged_obs_buf, prev_priv, NPRIV)):
        assert torch.isfinite(buf).all(), f"{name} step {t}"
        torch.testing.assert_close(buf[keep][:, :-f], prev[keep][:, f:], atol=0, rtol=0,
                                   msg=lambda m, name=name: f"{name} step {t}: {m}")
        assert (buf[done][:, :-f] == 0).all(), f"{name} step {t}: a reset env's older frames"
    return int(done.sum()), int(keep.sum())


def _run_steps(env, injector=None):
    n = env.num_envs
    prev_obs, prev_priv = _start(env)
    g = torch.Generator(device="cuda:0").manual_seed(9)
    resets = kept = 0
    for t in range(STEPS):
        a = 0.3 * torch.randn(n, 12, device="cuda:0", generator=g)
        if injector is None:
            _, _, rew, done, _ = env.step(a)
        else:
            _, _, rew, done, _ = env.step(a, _injected=injector.next())
        r, k = _assert_shifted(env, prev_obs, prev_priv, done.bool(), t)
        assert torch.isfinite(rew).all() and torch.isfinite(env.root_states).all() and torch.isfinite(env.dof_state).all()
        resets += r
        kept += k
        prev_obs, prev_priv = env.obs_buf.clone(), env.privileged_obs_buf.clone()
    assert resets > 0 and kept > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_fused_step_shift(n, dtype, dyn_kernel):
    _run_steps(_make(n, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_split_step_shift(n, dtype, dyn_kernel):
    env = _make(n, dtype)
    env.set_fused(False)
    _run_steps(env)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_injected_step_shift(n, dtype):
    from parity_driver import Injector
    env = _make(n, dtype)
    _run_steps(env, Injector(env, 11))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_phase_b_alone_shift(n, dtype):
    """t1env_step_reset_and_observe without a preceding phase A: it shifts in stream order, then k_post_b resets again
    the envs of reset_buf (the previous step's).  Only the shift property is checked: the newest frame of such a call
    has no reference.  An ordinary step between the calls moves the resets on."""
    from ti5_isaacgym_amd import _lib
    env = _make(n, dtype)
    _start(env)
    g = torch.Generator(device="cuda:0").manual_seed(9)
    resets = kept = 0
    for t in range(STEPS):
        env.step(0.3 * torch.randn(n, 12, device="cuda:0", generator=g))
        prev_obs, prev_priv = env.obs_buf.clone(), env.privileged_obs_buf.clone()
        a = env._args(env.common_step_counter)
        _lib.check(env._lib.t1env_step_reset_and_observe(env._handle, ctypes.byref(a), env._stream()),
                   "t1env_step_reset_and_observe")
        env._slot ^= 1
        r, k = _assert_shifted(env, prev_obs, prev_priv, env.reset_buf.bool(), t)
        resets += r
        kept += k
    assert resets > 0 and kept > 0
