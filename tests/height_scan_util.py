"""Helpers of the height-scan tests and of tools/height_scan_timing.py.

split_scan_step drives one env step with the explicit split sequence through the C ABI,
    t1env_step_physics_and_rewards -> t1env_measure_heights -> t1env_step_reset_and_observe -> t1env_critic_heights
(with the command curriculum's host read between the phases on its steps): the reference's own order, with the scan
sampling root_states before the reset.  T1DHStandEnv.step() runs t1env_step and then t1env_height_scan instead; the two
must give the same buffers.  fp32 histories only (t1env_critic_heights refuses fp16)."""
import torch


def small_trimesh(cfg):
    """the small trimesh terrain of parity_driver.make_env_for, with the scan on"""
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 6, 4, 5
    cfg.terrain.measure_heights = True


def make_scan_env(n, dtype="fp32", seed=3, mesh="trimesh", small=True, device="cuda:0"):
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        cfg.terrain.measure_heights = True
        if small:
            small_trimesh(cfg)
        cfg.env.state_dtype = dtype
    return make_t1_env(num_envs=n, mesh_type=mesh, seed=seed, device=device, cfg_hook=hook)


def split_scan_step(env, actions):
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.envs.t1_env import EXTRAS_RING, REWARD_NAMES
    assert env.measure_heights and env.obs_dtype == torch.float32
    assert actions.dtype == torch.float32 and actions.is_contiguous() and actions.device == env.device
    lib, h, s = env._lib, env._handle, env._stream()
    ext_call, ext_first, push_call = env._schedule()
    a = env._args(env.common_step_counter, ext_call, ext_first, push_call)
    ctr_post = env.common_step_counter + 1
    npts, pts, meas = env.num_height_points, env._height_pts.data_ptr(), env.measured_heights.data_ptr()
    _lib.check(lib.t1env_step_physics_and_rewards(h, actions.data_ptr(), _lib.C.byref(a), s), "physics")
    _lib.check(lib.t1env_measure_heights(h, pts, npts, meas, s), "t1env_measure_heights")
    if env.cfg.commands.curriculum and ctr_post % env.max_episode_length == 0:
        acc = env._ep_accum.cpu()
        env._command_curriculum(float(acc[REWARD_NAMES.index("tracking_lin_vel")]), float(acc[_lib.ACC_COUNT]))
        a = env._args(env.common_step_counter, ext_call, ext_first, push_call)
    _lib.check(lib.t1env_step_reset_and_observe(h, _lib.C.byref(a), s), "t1env_step_reset_and_observe")
    _lib.check(lib.t1env_critic_heights(h, env._slot, npts, float(env.obs_scales.height_measurements), meas,
                                        env._priv_ext[env._slot ^ 1].data_ptr(), env._priv_ext[env._slot].data_ptr(), s),
               "t1env_critic_heights")
    env.common_step_counter += 1
    env._slot ^= 1
    env._fill_extras(env.common_step_counter % EXTRAS_RING)
    return env.obs_buf, env.privileged_obs_buf, env.rew_buf, env.reset_buf, env.extras


def sync_state(dst, src):
    """src's whole state into dst (test_gpu_fused._sync, plus the scan's buffers): every step of the two starts from
    identical buffers, so an ulp between two instantiations of the dynamics cannot grow into different trajectories"""
    for k, t in src._keepalive.items():
        dst._keepalive[k].copy_(t)
    for k in range(2):
        dst._obs[k].copy_(src._obs[k])
        dst._priv[k].copy_(src._priv[k])
        dst._priv_ext[k].copy_(src._priv_ext[k])
    dst.measured_heights.copy_(src.measured_heights)
    dst.command_ranges["lin_vel_x"][:] = src.command_ranges["lin_vel_x"]
