"""The step kernels' end-of-step report (rigid_state, contact_forces; k_dyn6 / k_dyn5 / k_dyn4, fp32) against an
independent restatement of its definition -- needs the MI355X.

After the last substep every env step writes rigid_state (13 bodies x position, quaternion, COM velocity, angular
velocity) and contact_forces (13 x net contact force); post-physics reads them for the feet contact mask, the
base-contact termination and seven reward terms, and the product parity test hands them to the oracle as inputs.  The
three kernels spread the report differently over their waves (k_dyn6: roles W2-W6 with LDS hand-offs; k_dyn5 / k_dyn4:
leg wave and helper), none of which a host build runs.  Here each kernel takes one env step from the 64 states of
tests/report_scenarios.py -- the plane (stance / self / limits / impact) and the synthetic height field installed
through t1env_set_terrain (slope / impact / edge / base), 16 envs per kind, pushes off -- and both buffers, poisoned
with NaN before the step, are compared whole with oracle/dynamics_ref.py ContactRobot.report (DESIGN.md §4 "The report",
as tests/test_dynamics_report.py does for the host builds) at the kernel's own end-of-step state: the substep log's
last row, with each env's randomized COM displacement, friction and restitution read before the step.

End-of-step episodes: env.contact_vimp after the step for envs that did not reset; envs that did (the `base` kind
terminates on its own contact, and the reset zeroes the episodes) get theirs from ContactRobot.episodes_after carried
through the step's ten substep start states (the state set, then log rows 0..8).  The same reconstruction must equal
env.contact_vimp on the envs that did not reset (rtol 1e-4 / atol 1e-6): the episode carry across substeps, which no
other GPU test pins.

Bound per env and field group: |gpu - ref|_max <= 10 x the host fp32 build's worst distance from the same reference at
the end-of-step states of its own ten substeps + one fp32 ulp of the env's largest reference magnitude in the group
(10 x: tests/test_gpu_kernel_agreement.py's margin).  Host fp32 figures (tests/report_scenarios.py YARDSTICK, measured
by tests/test_dynamics_report.py::test_host_fp32_yardstick):
             position [m]  quaternion  COM velocity [m/s]  angular velocity [rad/s]  force [N]
    plane    1.5e-7        2.8e-7      2.2e-6              3.8e-6                    0.37
    field    1.4e-7        3.2e-7      1.3e-6              3.0e-6                    0.047
so the bounds are 1.5e-6 m, 2.8e-6, 2.2e-5 m/s, 3.8e-5 rad/s, 3.7 N on the plane and 1.4e-6 m, 3.2e-6, 1.3e-5 m/s,
3.0e-5 rad/s, 0.47 N on the field (plus the ulp floor).  The forces set the scale: k = 1e5 N/m turns 1e-6 m of a
foot's height into 0.1 N, and the plane's `self` kind carries capsule overlaps of centimetres (forces of several kN).

Guard: the force law jumps by d |v_n| where a point's depth crosses zero and at capsule distance r_a + r_b, so a body
row with a candidate within report_scenarios.GUARD of such a surface at the end-of-step state (fp32 rounding of the
coordinates, derived there) is left out of the FORCE comparison, at most 5% of the (env, body) rows that have contact
candidates; rigid rows are never left out.  The episode comparison leaves out a slot whose body comes that close in
any of the ten start states.

The MI355X's worst values per kernel, kind and group: profiles/report_gpu_tests.log.
"""
import numpy as np
import pytest
import torch

import report_scenarios as rs
import terrain_contact_scenarios as tcs

pytestmark = pytest.mark.gpu

SLOT_BODY = (4, 6, 10, 12, 0, 0)
POINT_BODIES = (0, 4, 6, 10, 12)
_REF = {}    # reference reports by the bits of (state, episodes, parameters): shared where kernels agree bit for bit


def check_report(name, case, ref, states, reset, vimp_end, rigid, contact, label=""):
    """the comparison, on host arrays: states = the eleven (root (n, 13), dof (n, 12, 2)) of the step -- the state set,
    then the ten substep ends; reset (n) bool; vimp_end (n, 6), rigid (n, 13, 13), contact (n, 13, 3) as read back"""
    n = rigid.shape[0]
    guard, yard = rs.GUARD[name], rs.YARDSTICK[name]
    assert np.isfinite(rigid).all() and np.isfinite(contact).all(), "a report row was not written (NaN poison left)"
    nopts = [b for b in range(13) if b not in POINT_BODIES]
    assert not contact[:, nopts].any(), "a body without contact points reports a force"
    assert np.abs(np.linalg.norm(rigid[:, :, 3:7], axis=2) - 1.0).max() <= 1e-6
    worst, fails, left, carry_checked = {}, [], 0, 0
    in_contact = dict.fromkeys(case["kinds"], 0)
    feet, base = [], []
    for i in range(n):
        kind = case["kinds"][i // rs.PER]
        # the episodes carried through the ten substeps, and the guard of that comparison
        ep, near_ep = case["vimp"][i].astype(np.float64), np.zeros(6, bool)
        for root, dof in states[:10]:
            sd = ref.switch_distance(i, root[i], dof[i])
            near_ep |= np.array([sd[b] < guard for b in SLOT_BODY])
            ep = ref.episodes_after(i, root[i], dof[i], ep)
        if reset[i]:
            vimp = ep
        else:
            vimp = vimp_end[i]
            ok = ~near_ep
            carry_checked += int(ok.sum())
            if not np.allclose(vimp[ok], ep[ok], rtol=1e-4, atol=1e-6):
                fails.append(f"{kind} env {i}: episodes {vimp} carried by the reference as {ep} (guarded {near_ep})")
        root, dof = states[10]
        key = (name, i, root[i].tobytes(), dof[i].tobytes(), vimp.tobytes(), ref.par["cd"][i].tobytes(),
               ref.par["fr"][i].tobytes(), ref.par["rst"][i].tobytes())
        if key not in _REF:
            _REF[key] = ref.report(i, root[i], dof[i], vimp) + (ref.switch_distance(i, root[i], dof[i]) < guard,)
        ref_rigid, ref_contact, near = _REF[key]
        in_contact[kind] += int(np.abs(ref_contact).max() > 0)
        feet += [ref_contact[b] for b in (6, 12)]
        base.append(ref_contact[0])
        left += int(near[list(POINT_BODIES)].sum())
        e = rs.group_errors(rigid[i], contact[i], ref_rigid, ref_contact)
        for g in rs.GROUP_NAMES:
            err = float(np.where(near, 0.0, e[g][0]).max()) if g == "force" else float(e[g][0])
            bound = 10 * yard[g] + rs.ULP * e[g][1]
            worst[(kind, g)] = max(worst.get((kind, g), 0.0), err)
            if err > bound:
                fails.append(f"{kind} env {i} {g}: |gpu - ref| {err:.3g} > {bound:.3g} (|ref|max {e[g][1]:.3g})"
                             + (f"\n{contact[i]}\n{ref_contact}" if g == "force" else ""))
    for kind in case["kinds"]:
        print(f"[{label}] {name} {kind}: worst |gpu - ref|",
              {g: f"{worst[(kind, g)]:.2e}" for g in rs.GROUP_NAMES}, "envs in contact", in_contact[kind])
    print(f"[{label}] {name}: force rows left out {left} of {len(POINT_BODIES) * n}; envs reset {int(reset.sum())}; "
          f"episode slots compared {carry_checked}")
    assert not fails, "\n".join(fails[:8])
    assert left <= rs.GUARD_CAP * len(POINT_BODIES) * n, f"{left} force rows within the guard distance"
    assert all(v > 0 for v in in_contact.values()), f"a kind without contact after the step: {in_contact}"
    assert carry_checked >= 6 * n // 2, "too few episode slots compared"
    feet, base = np.array(feet), np.array(base)
    assert (feet[:, 2] > 5.0).any(), "no foot row above the 5 N contact threshold"
    if name == "plane":
        assert ((np.abs(feet).max(axis=1) > 0) & (feet[:, 2] < 5.0)).any(), "no nonzero foot row below 5 N"
    else:
        assert (np.linalg.norm(base, axis=1) > 1.0).any(), "no base row above the 1 N termination threshold"


def _hook_field(cfg):
    cfg.domain_rand.push_robots = False
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 6, 4, 5


def _hook_plane(cfg):
    cfg.domain_rand.push_robots = False


@pytest.mark.parametrize("name", ["plane", "field"])
def test_end_of_step_report_matches_definition(dyn_solver, name):
    from ti5_isaacgym_amd import _lib, make_t1_env
    from ti5_isaacgym_amd.envs.t1_env import SOLVER
    from ti5_isaacgym_amd.utils.urdf import load_model

    tab = load_model()
    case = rs.plane_case(tab) if name == "plane" else rs.field_case(tab)
    n = case["root"].shape[0]
    env = make_t1_env(num_envs=n, mesh_type="plane" if name == "plane" else "trimesh", seed=13, device="cuda:0",
                      cfg_hook=_hook_plane if name == "plane" else _hook_field)
    env.set_substep_log(True)
    env.reset()
    if name == "field":   # the synthetic field in place of the env's own, as tests/test_gpu_dynamics_terrain_contact.py
        torch.cuda.synchronize()
        env.height_samples = torch.from_numpy(case["field"]).to("cuda:0").contiguous()   # kept alive on the env
        _lib.check(env._lib.t1env_set_terrain(env._handle, env.height_samples.data_ptr(), case["field"].shape[0],
                                              case["field"].shape[1], tcs.HS, tcs.VS, tcs.BORDER, 2), "t1env_set_terrain")
    env.root_states.copy_(torch.from_numpy(case["root"].astype(np.float32)))
    env.dof_state.copy_(torch.from_numpy(case["dof"].reshape(n * 12, 2).astype(np.float32)))
    env.contact_vimp.copy_(torch.from_numpy(case["vimp"]))
    env.applied_force.zero_()
    env.rigid_state.fill_(float("nan"))
    env.contact_forces.fill_(float("nan"))
    # the randomized parameters, read BEFORE the step: the reset at its end redraws them
    par = {"cd": env.com_displacements.cpu().numpy(), "fr": env.env_frictions.cpu().numpy().reshape(n),
           "rst": env.restitution_coeffs.cpu().numpy().reshape(n)}
    rng = np.random.default_rng(7)
    env.step(torch.from_numpy(rng.normal(0, 0.5, (n, 12)).astype(np.float32)).to("cuda:0"))
    lg = {k: v.cpu().numpy().astype(np.float64) for k, v in env.substep_log.items()}
    env.set_substep_log(False)
    reset = env.reset_buf.cpu().numpy().astype(bool).reshape(n)
    vimp_end = env.contact_vimp.cpu().numpy().astype(np.float64)
    rigid = env.rigid_state.cpu().numpy().astype(np.float64)
    contact = env.contact_forces.cpu().numpy().astype(np.float64)
    assert lg["root"].shape[0] == 10

    ref = rs.Reference(tab, env._model, SOLVER, par, case["terrain"])
    states = [(case["root"], case["dof"])] + [(lg["root"][k], lg["dof"][k]) for k in range(10)]
    check_report(name, case, ref, states, reset, vimp_end, rigid, contact, label=dyn_solver)
