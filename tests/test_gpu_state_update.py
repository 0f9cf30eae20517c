"""The substep's state update in the step kernels (k_dyn6 / k_dyn5 / k_dyn4) -- needs the MI355X.

The independent references return a velocity change; integrate_base (position from the new base-origin velocity,
first-order normalised quaternion from the new angular velocity) and integrate_leg (q += dt qd_new, the joint speed
clamped to vel_limit[6 leg + k]) were held only to the same header compiled in fp64, and k_dyn6 runs its own pinned
variants of both.  Inputs, restatement and bounds: tests/state_update_util.py; the host builds' twin:
tests/test_state_update.py.

State update along the log: 33 envs (one full k_dyn6 workgroup plus one env) on the plane near the origin, pushes off,
a third each standing in contact, airborne tumbling and lying on the base box; one env step with the substep log, rows
s - 1 -> s (row -1: the state set before the step).  Bound per field and env row: 4 x the numpy fp32 restatement's
largest gap from the fp64 one over the test's rows + one fp32 ulp of the field's magnitude.

Joint speed clamp: 33 airborne envs, self-collision and the action lag off, every joint at 0.97-1.0 of its velocity
limit with the action driving the PD torque into its limit outward; substep 0 against clip(qd0 + dt a_ref, +-vl) with
a_ref from oracle/dynamics_ref.py Robot.accel on the logged torque: fp32(vl_j) bit for bit beyond the limit, dt 2e-4
(1 + |a_ref|max) inside.

The MI355X's figures per kernel: profiles/state_update_gpu_tests.log.
"""
import numpy as np
import pytest
import torch

import state_update_util as su

pytestmark = pytest.mark.gpu


def _set_state(env, root, dof):
    n = root.shape[0]
    env.root_states.copy_(torch.from_numpy(root.astype(np.float32)))
    env.dof_state.copy_(torch.from_numpy(dof.reshape(n * 12, 2).astype(np.float32)))
    env.contact_vimp.zero_()
    env.applied_force.zero_()


def _log(env):
    lg = {k: v.cpu().numpy().astype(np.float64) for k, v in env.substep_log.items()}
    env.set_substep_log(False)
    return lg


def test_state_update_along_the_substep_log(dyn_solver):
    from ti5_isaacgym_amd import make_t1_env
    from ti5_isaacgym_amd.utils.urdf import load_model

    def hook(cfg):
        cfg.domain_rand.push_robots = False
        cfg.env.env_spacing = 0.05   # origins within 0.3 m of zero: an fp32 ulp of position stays small

    tab = load_model()
    root, dof, kinds = su.log_case(tab)
    env = make_t1_env(num_envs=su.N, mesh_type="plane", seed=13, device="cuda:0", cfg_hook=hook)
    env.set_substep_log(True)
    env.reset()
    _set_state(env, root, dof)
    cd = env.com_displacements.cpu().numpy().astype(np.float64)   # read before the step: a reset redraws it
    rng = np.random.default_rng(7)
    env.step(torch.from_numpy(rng.normal(0, 0.5, (su.N, 12)).astype(np.float32)).to("cuda:0"))
    lg = _log(env)
    assert lg["root"].shape[0] == 10
    rows = [(root, dof)] + [(lg["root"][k], lg["dof"][k]) for k in range(10)]
    com = np.asarray(tab["com"], float)[0] + cd
    vel_limit = [env._model.vel_limit[j] for j in range(12)]
    assert np.array_equal(np.float32(vel_limit), np.asarray(tab["limits"], np.float32)[:, 3])
    yard, worst, fails = su.walk_rows(rows, com, vel_limit, dt=float(env.sim_params.dt))
    print(su.report_line(dyn_solver, yard, worst))
    assert not fails, "\n".join(fails[:8])
    assert np.abs(rows[10][0][:, 0:3] - rows[0][0][:, 0:3]).max() > 1e-2
    assert np.abs(rows[10][0][:, 3:7] - rows[0][0][:, 3:7]).max() > 1e-2


def test_joint_speed_clamp(dyn_solver):
    from ti5_isaacgym_amd import make_t1_env
    from ti5_isaacgym_amd.utils.urdf import load_model

    def hook(cfg):
        cfg.domain_rand.push_robots = False
        cfg.asset.self_collisions = 1      # Isaac Gym's filter: 1 = disabled
        cfg.domain_rand.add_lag = False    # substep 0 sees this step's action

    tab = load_model()
    root, dof, sign = su.clamp_case(tab)
    env = make_t1_env(num_envs=su.N, mesh_type="plane", seed=11, device="cuda:0", cfg_hook=hook)
    env.set_substep_log(True)
    env.reset()
    root[:, 0:2] = env.env_origins[:, 0:2].cpu().numpy().astype(np.float64)
    _set_state(env, root, dof)
    par = {"bm": env.body_mass.cpu().numpy().reshape(su.N).astype(np.float64),
           "ls": env.link_mass_scale.cpu().numpy().astype(np.float64),
           "cd": env.com_displacements.cpu().numpy().astype(np.float64),
           "arm": env.joint_armatures.cpu().numpy().astype(np.float64)}
    # 40 x action_scale 0.5 = 20 rad beyond the pose: the PD torque saturates at its limit, outward
    env.step(torch.from_numpy((40.0 * sign).astype(np.float32)).to("cuda:0"))
    lg = _log(env)
    su.check_clamp(tab, root, dof, lg["dof"][0, :, :, 1], lg["torque"][0], par,
                   [env._model.vel_limit[j] for j in range(12)], dt=float(env.sim_params.dt), label=dyn_solver)
