"""The step kernels (k_dyn6 / k_dyn5 / k_dyn4) against the robot description itself -- needs the MI355X.

tests/test_gpu_dynamics_kane.py holds a kernel substep to Kane's equations on the collapsed tables, which the kernel
reads too.  Here the reference is tests/urdf_links.py on the description fixture (tests/golden/t1_robot/urdf/t1.urdf):
all 24 links as rigid bodies of their own, never load_model().  That closes the chain description -> compile_model ->
ctypes model -> make_dyn_model -> kernel end to end; tests/test_model_tables.py holds the tables to the same reference on
the host.

The Kane test's set-up at 16 envs: airborne at 5 m, self-collision off, one env step with the substep log, substep 0; the
velocity change / dt recovered exactly as there.  The mass, COM and link-mass randomisations are off (they are defined
on the collapsed bodies), the armature's stays on.  Bound: 2e-4 (1 + |ref|max) per env, the project's Kane bound.

An env built with urdf_path = the fixture must produce byte-identical outputs to the env built from the committed JSON,
over 3 steps at 33 envs.
"""
import copy

import numpy as np
import pytest
import torch

import golden_util
import state_update_util as su
import urdf_links
from oracle.dynamics_ref import quat_to_R

pytestmark = pytest.mark.gpu

N = 16
_REF = {}   # raw-tree accelerations by the bits of their inputs: shared where the kernels log the same torques


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _hook(cfg):
    cfg.domain_rand.push_robots = False
    cfg.asset.self_collisions = 1   # Isaac Gym's filter: 1 = disabled (Kane's equations have no contact terms)
    golden_util.apply_overrides(cfg, su.DR_MASS_OFF)


def test_one_substep_matches_the_uncollapsed_description(dyn_solver):
    from ti5_isaacgym_amd import make_t1_env
    from ti5_isaacgym_amd.utils.urdf import DOF_NAMES

    tree = urdf_links.LinkTree(urdf_links.FIXTURE, DOF_NAMES)
    base_mass, com_base = tree.rigid_group(tree.root)
    env = make_t1_env(num_envs=N, mesh_type="plane", seed=11, device="cuda:0", cfg_hook=_hook)
    env.set_substep_log(True)
    env.reset()
    # the randomisations that are defined on the collapsed bodies are off
    assert np.array_equal(env.body_mass.cpu().numpy().reshape(N), np.full(N, np.float32(base_mass)))
    assert (env.link_mass_scale.cpu().numpy() == 1).all() and (env.com_displacements.cpu().numpy() == 0).all()
    arm = env.joint_armatures.cpu().numpy().astype(np.float64)
    assert len(np.unique(arm)) > 1, "armature randomisation is off"

    rng = np.random.default_rng(7)
    lim = np.array([[tree.joints[n]["limit"][k] for k in ("lower", "upper", "effort", "velocity")] for n in DOF_NAMES])
    lo = np.maximum(np.array([-0.5, -0.17, -0.78, 0.01, -1.9, -2.9] * 2), lim[:, 0] + 0.05)
    hi = np.minimum(np.array([0.5, 0.17, 0.78, 2.0, 1.9, 2.9] * 2), lim[:, 1] - 0.05)
    q0 = np.clip(su.Q_NOMINAL + rng.uniform(-0.15, 0.15, (N, 12)), lo, hi)
    qd0 = np.clip(rng.normal(0, 1.5, (N, 12)), -0.3 * lim[:, 3], 0.3 * lim[:, 3])
    quat = rng.normal(size=(N, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    root = np.zeros((N, 13), np.float32)
    root[:, 0:2] = env.env_origins[:, 0:2].cpu().numpy()
    root[:, 2] = 5.0
    root[:, 3:7] = quat
    root[:, 7:10] = rng.normal(0, 0.5, (N, 3))   # COM velocity (the root-state convention)
    root[:, 10:13] = rng.normal(0, 0.8, (N, 3))
    env.root_states.copy_(torch.from_numpy(root))
    env.dof_state.copy_(torch.from_numpy(np.stack([q0, qd0], -1).reshape(N * 12, 2).astype(np.float32)))
    env.applied_force.zero_()
    env.step(torch.from_numpy(rng.normal(0, 0.5, (N, 12)).astype(np.float32)).to("cuda:0"))
    lg = {k: v.cpu().numpy().astype(np.float64) for k, v in env.substep_log.items()}
    env.set_substep_log(False)

    dt = float(env.sim_params.dt)
    r0 = root.astype(np.float64)
    q0, qd0 = q0.astype(np.float32).astype(np.float64), qd0.astype(np.float32).astype(np.float64)
    worst = 0.0
    for n in range(N):
        R0, w0 = quat_to_R(r0[n, 3:7]), r0[n, 10:13]
        vo0 = r0[n, 7:10] - np.cross(w0, R0 @ com_base)
        tau = lg["torque"][0, n]
        key = (r0[n].tobytes(), q0[n].tobytes(), qd0[n].tobytes(), tau.tobytes(), arm[n].tobytes())
        if key not in _REF:
            _REF[key] = tree.accel(r0[n, 0:3], r0[n, 3:7], w0, vo0, q0[n], qd0[n], tau, arm[n])[0]
        ref_sp = _REF[key].copy()
        ref_sp[3:6] -= np.cross(w0, vo0)   # classical -> spatial acceleration of the base origin
        # the kernel's velocity change over substep 0 (vb = vO_new + dt w_new x vO_new, reported at the COM)
        r1 = lg["root"][0, n]
        R1, w1 = quat_to_R(r1[3:7] / np.linalg.norm(r1[3:7])), r1[10:13]
        vb1 = r1[7:10] - np.cross(w1, R1 @ com_base)
        vo1 = np.linalg.solve(np.eye(3) + dt * _skew(w1), vb1)
        du = np.concatenate([w1 - w0, vo1 - vo0, lg["dof"][0, n, :, 1] - qd0[n]]) / dt
        err = np.abs(du - ref_sp).max()
        scale = np.abs(ref_sp).max() + 1.0
        worst = max(worst, err / scale)
        assert err <= 2e-4 * scale, f"env {n}: |gpu - raw tree| {err:.3g} (scale {scale:.3g})\n{du}\n{ref_sp}"
    print(f"[{dyn_solver}] worst |gpu - raw 24-link tree| / (1 + |ref|max) over {N} envs: {worst:.2e}")


def _make(num_envs, seed, urdf_path):
    """make_t1_env with the model from a URDF"""
    from ti5_isaacgym_amd import T1DHStandEnv, set_seed, task_registry
    cfg, _ = task_registry.get_cfgs("t1_dh_stand")
    cfg = copy.deepcopy(cfg)
    cfg.env.num_envs, cfg.seed, cfg.terrain.mesh_type = num_envs, seed, "plane"
    set_seed(seed)
    return T1DHStandEnv(cfg, sim_device="cuda:0", urdf_path=urdf_path)


def test_env_from_the_description_equals_env_from_the_tables(dyn_solver):
    n = 33
    outs = []
    for path in (None, urdf_links.FIXTURE):
        env = _make(n, 9, path)
        model = bytes(env._model)
        env.reset()
        g = torch.Generator().manual_seed(3)
        rec = []
        for _ in range(3):
            obs, priv, rew, reset, _ = env.step(torch.randn(n, 12, generator=g).to("cuda:0"))
            rec.append([t.cpu().numpy().tobytes() for t in (obs, priv, rew, reset, env.root_states, env.dof_state,
                                                             env.rigid_state, env.contact_forces, env.torques)])
        outs.append((model, rec))
        del env
    assert outs[0][0] == outs[1][0], "the model struct differs"
    names = ("obs", "priv", "rew", "reset", "root_states", "dof_state", "rigid_state", "contact_forces", "torques")
    for s in range(3):
        for name, a, b in zip(names, outs[0][1][s], outs[1][1][s]):
            assert a == b, f"step {s}: {name} differs"
