"""The reset work on the fused step's tail -- needs the MI355X.

In the fused step an env that resets has its new state written by the state wave's reset_idx in two parts (the terrain
curriculum, which settles the terrain-level sum, then the rest), and the older frames of its two history rows zeroed 16
bytes per store.  In k_dyn6 the waves that have left the epilogue zero those rows and the env's lag rings, and the state
wave signals the level sum through a flag and runs the rest of the reset behind it.  The split kernel sequence keeps the
one-lane reset_env as one piece and the element-wise zeroing, and is the reference here, as in test_gpu_fused.py: a fused
and a split env with the same seed, the split env's whole state copied into the fused one before every step.

Resets are forced: the chosen envs' episode step is set to the episode length, so they time out on the next step.  Both
histories are filled with non-zero values before that step, so a zero in them afterwards was stored by it.  Checked on
every step: test_gpu_fused.py's exact and close lists on every row; the rows of reset envs exactly equal in everything
reset_idx writes from draws and constants; reset rows of both histories all zero but for the newest frame, which equals
the split env's (the wide zero stores end where it begins); every other row the previous history shifted by one frame,
bit for bit; extras["episode"] as the split env's, and the previous ring slot's values on a step without a reset.

Env counts 1 (63 shadow lanes), 33 (a second workgroup with one live env), 64 and 97 (a ragged last workgroup); the
plane, and trimesh at 97, where the curriculum moves origins; fp32 histories, and fp16 at 33 and 97 (rows 4-byte
aligned only); every dynamics kernel (k_dyn5 and k_dyn4 take the shared wide zeroing through their own structure).
"""
import pytest
import torch

from test_gpu_fused import CLOSE, EXACT, _sync

pytestmark = pytest.mark.gpu

NOBS, NPRIV = 47, 73
# everything reset_env writes from draws and constants (attribute names of the env; dof_state is (N * 12, 2))
RESET_EXACT = ["contact_vimp", "dof_state", "motor_offsets", "randomized_p_gains", "randomized_d_gains",
               "randomized_joint_coulomb", "randomized_joint_viscous", "joint_armatures", "_act_hist", "_dof_hist",
               "_imu_hist", "lag_timestep", "dof_lag_timestep", "imu_lag_timestep", "actions", "episode_length_buf",
               "phase_length_buf", "gait_start", "gait_time", "base_lin_vel", "base_ang_vel", "projected_gravity",
               "base_euler_xyz", "terrain_levels", "env_origins", "commands", "root_states"]

RESET_SETS = {
    "none": lambda n: [],
    "all": lambda n: list(range(n)),
    "corners": lambda n: sorted({i for i in (0, 31, 32, n - 1) if i < n}),
    "adjacent": lambda n: [i for i in (5, 6, 7) if i < n],
    "single": lambda n: [min(16, n - 1)],
}

CONFIGS = [(1, "plane", "fp32"), (33, "plane", "fp32"), (64, "plane", "fp32"), (97, "plane", "fp32"),
           (97, "trimesh", "fp32"), (33, "plane", "fp16"), (97, "plane", "fp16")]


def _env(n, mesh, dtype, fused):
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        cfg.env.state_dtype = dtype
    env = make_t1_env(num_envs=n, mesh_type=mesh, seed=11, device="cuda:0", cfg_hook=hook)
    env.set_fused(fused)
    env.reset()
    return env


def _bits_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize("which", sorted(RESET_SETS))
@pytest.mark.parametrize("n,mesh,dtype", CONFIGS, ids=[f"{n}_{m}_{d}" for n, m, d in CONFIGS])
def test_forced_resets_equal_the_split_sequence(n, mesh, dtype, which, dyn_kernel):
    fused, split = _env(n, mesh, dtype, True), _env(n, mesh, dtype, False)
    forced = torch.tensor(RESET_SETS[which](n), dtype=torch.long, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(3)
    ring = split._extras_ring.shape[0]
    for t in range(3):
        if t == 1:  # the forced step: non-zero histories, the chosen envs at their last episode step
            for k in range(2):
                split._obs[k].uniform_(0.5, 1.0, generator=g)
                split._priv[k].uniform_(0.5, 1.0, generator=g)
            split.episode_length_buf[forced] = int(split.max_episode_length)
        a = 0.3 * torch.randn(n, 12, device="cuda:0", generator=g)
        _sync(fused, split)
        prev_obs, prev_priv = split.obs_buf.clone(), split.privileged_obs_buf.clone()
        fused.step(a)
        split.step(a)
        where = f"step {t}"
        r = split.reset_buf.bool()
        if t == 1:
            for env in (fused, split):  # the case cannot pass without having reset
                assert bool((env.reset_buf[forced] == 1).all()), f"{where}: a forced env did not reset"
        if which == "none" or t == 0:
            assert not bool(r.any()) and not bool(fused.reset_buf.any()), f"{where}: an unforced reset"
        for f in EXACT:
            assert torch.equal(getattr(fused, f), getattr(split, f)), f"{where}: {f} differs"
        for f in CLOSE:
            torch.testing.assert_close(getattr(fused, f), getattr(split, f), rtol=1e-5, atol=1e-6,
                                       msg=lambda m, f=f: f"{where}: {f}: {m}")
        for f in RESET_EXACT:  # the rows of reset envs: exactly the split sequence's
            x, y = getattr(fused, f).reshape(n, -1), getattr(split, f).reshape(n, -1)
            assert torch.equal(x[r], y[r]), f"{where}: {f} differs on a reset row"
        for name, fr, prev in (("obs", NOBS, prev_obs), ("priv", NPRIV, prev_priv)):
            fb = fused.obs_buf if name == "obs" else fused.privileged_obs_buf
            sb = split.obs_buf if name == "obs" else split.privileged_obs_buf
            for env_name, buf in (("fused", fb), ("split", sb)):
                assert not bool(buf[r][:, :-fr].any()), f"{where}: {env_name} {name}: a reset row's older frames"
                assert torch.equal(buf[~r][:, :-fr], prev[~r][:, fr:]), f"{where}: {env_name} {name}: the shifted rows"
            assert torch.equal(fb[r][:, -fr:], sb[r][:, -fr:]), f"{where}: {name}: a reset row's newest frame"
            if t == 1 and bool(r.any()):
                assert bool(fb[r][:, -fr:].any()), f"{where}: {name}: a reset row's newest frame is empty"
        ef, es = fused.extras["episode"], split.extras["episode"]
        assert set(ef) == set(es)
        for k in ef:
            torch.testing.assert_close(torch.as_tensor(ef[k]), torch.as_tensor(es[k]), rtol=1e-5, atol=1e-7,
                                       msg=lambda m, k=k: f"{where}: extras {k}: {m}")
        if not bool(r.any()):  # a step without a reset keeps the previous ring slot's values
            slot = fused.common_step_counter % ring
            for env in (fused, split):
                assert _bits_equal(env._extras_ring[slot], env._extras_ring[(slot - 1) % ring]), \
                    f"{where}: extras of a step without resets"
