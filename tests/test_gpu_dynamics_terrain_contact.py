"""The GPU solver (k_dyn6 / k_dyn5 / k_dyn4, fp32) in contact with a SLOPED HEIGHT FIELD against an independent
formulation that works on the triangle mesh -- needs the MI355X.

tests/test_gpu_dynamics_contact.py checks one substep of the step kernels in contact on the plane, where every normal
is (0, 0, 1); tests/test_gpu_dynamics.py[trimesh] compares the kernels with the same header built for the host.  Here
the kernels run one substep on the synthetic field of tests/terrain_contact_scenarios.py (a rough tilted region and a
0.25 m step; 16 envs each of the kinds slope, impact, edge, base) and are compared with oracle/dynamics_ref.py
ContactRobot on a MeshTerrain (explicit triangles, barycentric containment and interpolation, normals from the edges),
as tests/test_dynamics_terrain_contact.py does for the host builds.  On the device this also covers what no host build
runs: the packed two-points-per-instruction contact math with a different normal per point, and the coarse height
bound (k_hmax and the bound test ahead of every body's contact): in the `edge` kind a foot touches the plateau while
its frame origin, less its contact radius, is above the terrain under the origin, so a bound one cell short would drop
the foot's whole contact.

The field is installed through t1env_set_terrain on the env's handle (which rebuilds the coarse bound); the terrain
struct is passed by value to every launch.  Robots stand at absolute field coordinates.  Each env is compared with its
own randomized masses, COM, armature, friction and restitution; the kernel's velocity change over substep 0 is
recovered from the substep log as in tests/test_gpu_dynamics_contact.py.

Bound: |du_gpu - du_ref| <= 1e-4 (1 + |du_ref|_max) per env (tests/test_gpu_dynamics_contact.py's).  The host fp32
builds of the header reach 1.5e-6 .. 1.4e-5 on the same states (tests/test_dynamics_terrain_contact.py prints them).
The worst values measured on the MI355X and the contact counts are in profiles/terrain_contact_gpu_tests.log.
"""
import numpy as np
import pytest
import torch

import terrain_contact_scenarios as tcs
from oracle.dynamics_ref import ContactRobot, quat_to_R

pytestmark = pytest.mark.gpu

BOUND = 1e-4
_REF = {}   # the reference's du per env, shared by the kernels where their inputs (state, parameters, torques) agree


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _hook(cfg):
    cfg.domain_rand.push_robots = False
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 6, 4, 5


def test_one_substep_on_sloped_terrain_matches_mesh_reference(dyn_solver):
    from ti5_isaacgym_amd import _lib, make_t1_env
    from ti5_isaacgym_amd.envs.t1_env import SOLVER
    from ti5_isaacgym_amd.utils.urdf import load_model

    n = tcs.PER * len(tcs.KINDS)
    tab = load_model()
    field = tcs.make_field()
    terrain = tcs.mesh_terrain(field)
    env = make_t1_env(num_envs=n, mesh_type="trimesh", seed=13, device="cuda:0", cfg_hook=_hook)
    env.set_substep_log(True)
    env.reset()
    # the synthetic field in place of the env's own, through the call the env itself installs its terrain with
    torch.cuda.synchronize()
    env.height_samples = torch.from_numpy(field).to("cuda:0").contiguous()   # kept alive on the env
    _lib.check(env._lib.t1env_set_terrain(env._handle, env.height_samples.data_ptr(), field.shape[0], field.shape[1],
                                          tcs.HS, tcs.VS, tcs.BORDER, 2), "t1env_set_terrain")
    m = env._model
    roots, dofs, vimps, facts = [], [], [], []
    for kind in tcs.KINDS:
        root, dof, vimp, f = tcs.scenario(kind, tab, terrain)
        tcs.check_kind(kind, f, vimp, float(m.bounce_threshold))
        roots.append(root)
        dofs.append(dof)
        vimps.append(vimp)
        facts += f
    r0, d0, vimp = np.concatenate(roots), np.concatenate(dofs), np.concatenate(vimps)
    env.root_states.copy_(torch.from_numpy(r0.astype(np.float32)))
    env.dof_state.copy_(torch.from_numpy(d0.reshape(n * 12, 2).astype(np.float32)))
    env.contact_vimp.copy_(torch.from_numpy(vimp))
    env.applied_force.zero_()
    # each env's randomized parameters, read BEFORE the step: a robot lying on its base box terminates, and the reset at
    # the end of the step redraws them
    base_mass = env.body_mass.cpu().numpy().reshape(n).astype(np.float64)
    link_scale = env.link_mass_scale.cpu().numpy().astype(np.float64)
    com_disp = env.com_displacements.cpu().numpy().astype(np.float64)
    arm = env.joint_armatures.cpu().numpy().astype(np.float64)
    fr = env.env_frictions.cpu().numpy().reshape(n).astype(np.float64)
    rst = env.restitution_coeffs.cpu().numpy().reshape(n).astype(np.float64)
    rng = np.random.default_rng(7)
    env.step(torch.from_numpy(rng.normal(0, 0.5, (n, 12)).astype(np.float32)).to("cuda:0"))
    lg = {k: v.cpu().numpy().astype(np.float64) for k, v in env.substep_log.items()}
    env.set_substep_log(False)

    dt = float(env.sim_params.dt)
    solver = dict(SOLVER, bounce_threshold=float(m.bounce_threshold))
    lim = np.array([[m.q_lower[j], m.q_upper[j]] for j in range(12)], float)
    mass0 = np.asarray(tab["mass"], float)
    com_base = np.asarray(tab["com"], float)[0]
    worst, failures = {}, []
    for i in range(n):
        kind = tcs.KINDS[i // tcs.PER]
        R0, w0 = quat_to_R(r0[i, 3:7]), r0[i, 10:13]
        vo0 = r0[i, 7:10] - np.cross(w0, R0 @ (com_base + com_disp[i]))
        key = (i, base_mass[i], link_scale[i].tobytes(), com_disp[i].tobytes(), arm[i].tobytes(), fr[i], rst[i],
               lg["torque"][0, i].tobytes())
        if key not in _REF:
            mass = mass0.copy()
            mass[0] = base_mass[i]
            mass[1:] = mass0[1:] * link_scale[i]
            isc = np.concatenate([[base_mass[i] / mass0[0]], link_scale[i]])
            rob = ContactRobot(tab, mass, isc, com_disp[i], arm[i], solver=solver, limits=lim, terrain=terrain)
            mu_g = 0.5 * (fr[i] + float(m.ground_friction))
            e_g = 0.5 * (rst[i] + float(m.ground_restitution))
            _REF[key], _ = rob.step(r0[i, 0:3], r0[i, 3:7], w0, vo0, d0[i, :, 0], d0[i, :, 1], lg["torque"][0, i], dt,
                                    mu_g, e_g, fr[i], rst[i], vimp=vimp[i].astype(np.float64))
        ref = _REF[key]
        r1 = lg["root"][0, i]
        R1, w1 = quat_to_R(r1[3:7] / np.linalg.norm(r1[3:7])), r1[10:13]
        vb1 = r1[7:10] - np.cross(w1, R1 @ (com_base + com_disp[i]))
        vo1 = np.linalg.solve(np.eye(3) + dt * _skew(w1), vb1)
        du = np.concatenate([w1 - w0, vo1 - vo0, lg["dof"][0, i, :, 1] - d0[i, :, 1]])
        err = np.abs(du - ref).max() / (np.abs(ref).max() + 1.0)
        worst[kind] = max(worst.get(kind, 0.0), err)
        if err > BOUND:
            failures.append(f"{kind} env {i} ({facts[i]['contacts']} contacts on bodies {facts[i]['bodies']}): "
                            f"|gpu - ref| / (1 + |ref|max) {err:.3g}\n{du}\n{ref}")
    count = lambda key, pred=bool: {k: sum(pred(f[key]) for f in facts[j * tcs.PER:(j + 1) * tcs.PER])  # noqa: E731
                                    for j, k in enumerate(tcs.KINDS)}
    print(f"[{dyn_solver}] worst |gpu - ref| / (1 + |ref|max):", {k: f"{v:.2e}" for k, v in worst.items()},
          "contacts:", count("contacts", int), "base-box contacts:", count("base_contacts", int)["base"],
          "edge envs meeting the cull condition:", count("cull_condition")["edge"])
    assert not failures, "\n".join(failures)
