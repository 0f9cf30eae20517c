"""The end-of-step report (rigid_state 13 x 13, contact_forces 13 x 3) of the product header against an independent
restatement of its definition (DESIGN.md §4 "The report") -- host builds, no GPU.

Post-physics reads these two buffers for the feet contact mask (f_z > 5 N), the base-contact termination (|f| > 1 N),
feet_contact_forces, foot_slip, feet_clearance, feet_distance, knee_distance, feet_rotation and collision; the product
parity test hands them to the oracle as inputs, and the solver tests check the velocity change, not the report.  Here
t1dyn_substeps(nsub = 0) writes the report of a given state, and oracle/dynamics_ref.py ContactRobot.report restates
it in fp64 from plain forward kinematics, central-difference velocities, the explicit triangle mesh (or the plane),
its own capsule closest-point search and the force law per point, on the 64 + 64 states of tests/report_scenarios.py
(plane: stance / self / limits / impact; the synthetic field: slope / impact / edge / base), each env with its own
masses, COM displacement, friction and restitution.

Bound (fp64 builds, flags 1 and 3, both mesh types): |out - ref|_max <= 1e-5 (1 + |ref|_max) per env and field group
(position, quaternion up to sign, COM velocity, angular velocity, force); the reference's velocities are central
differences with step 1e-6, and the host writes its fp64 result to fp32 buffers (6e-8 relative).  No group needed a
looser bound.  Reported quaternions are unit to 1e-6.  Control: against a reference blind to the field the force rows
must miss by >= 100 x the bound.

The reference alone must show (test_inputs_cover_the_law): points approaching, separating below an active restitution
target, and separating on the spring alone; sliding and sticking points; self-contact forces on a shank and on a foot
from cross-leg and within-leg pairs; a base-box force with two different episodes on its halves; feet f_z on both
sides of 5 N and base |f| on both sides of 1 N.  A point whose force is clamped at zero is not among them: the law
has none.  f_n = k pen - [v_n < v_tgt] d (v_n - v_tgt) with pen > 0 is at least k pen
whenever the damper acts (v_n - v_tgt < 0 there) and k pen otherwise, so the max(., 0) never binds on a point in
contact; the test asserts that instead (the unclamped f_n of every point is positive).

The host fp32 builds' (flags 0, 2) distance from the reference is printed per case and group, on these states and on
the states ten substeps later: the yardstick of tests/test_gpu_dynamics_report.py (tests/report_scenarios.py YARDSTICK
records the end-of-step figures; the measurement must stay within twice of them).
test_episodes_carry_through_ten_substeps follows the restitution episodes of the fp64 compositions through ten
substeps against ContactRobot.episodes_after (the GPU test does the same for the kernels).
Both mutants of the header -- the foot's target taken from the shank's episode, the self-contact forces dropped -- fail
this file: profiles/report_mutants.log.
"""
import numpy as np
import pytest

import report_scenarios as rs
from test_dynamics_contact import make_setup

BOUND = 1e-5
_CACHE = {}


@pytest.fixture(scope="module")
def setup():
    return make_setup()


def case(setup, name):
    """the case's inputs, per-env parameters, the reference's report (with per-point detail) and the blind one"""
    if name not in _CACHE:
        from ti5_isaacgym_amd.envs.t1_env import SOLVER
        dyn, m, tab = setup
        c = rs.plane_case(tab) if name == "plane" else rs.field_case(tab)
        par = rs.host_params(m, c)
        ref = rs.Reference(tab, m, SOLVER, par, c["terrain"])
        n = c["root"].shape[0]
        det = [[] for _ in range(n)]
        rep = [ref.report(i, c["root"][i], c["dof"][i], c["vimp"][i], detail=det[i]) for i in range(n)]
        c.update(par=par, ref=ref, rigid=np.array([r[0] for r in rep]), contact=np.array([r[1] for r in rep]),
                 detail=det)
        if name == "field":
            c["blind"] = np.array([ref.report(i, c["root"][i], c["dof"][i], c["vimp"][i], blind=True)[1]
                                   for i in range(n)])
        _CACHE[name] = c
    return _CACHE[name]


def errors(c, out, rigid=None, contact=None):
    """per env {group: |out - ref|_max / (1 + |ref|_max)} against the case's reference"""
    rigid, contact = c["rigid"] if rigid is None else rigid, c["contact"] if contact is None else contact
    res = []
    for i in range(rigid.shape[0]):
        e = rs.group_errors(out["rigid"][i], out["contact"][i], rigid[i], contact[i])
        res.append({g: float(np.max(v[0])) / (1.0 + v[1]) for g, v in e.items()})
    return res


@pytest.mark.parametrize("flags", [1, 3], ids=["assembled", "split"])
@pytest.mark.parametrize("name,mesh", [("plane", 0), ("field", 1), ("field", 2)],
                         ids=["plane", "field-heightfield", "field-trimesh"])
def test_report_matches_definition(setup, name, flags, mesh):
    c = case(setup, name)
    out = rs.host_report(setup, c, c["par"], flags, mesh=mesh)
    assert np.isfinite(out["rigid"]).all() and np.isfinite(out["contact"]).all(), "a row was not written"
    assert np.abs(np.linalg.norm(out["rigid"][:, :, 3:7], axis=2) - 1.0).max() <= 1e-6
    # the eight bodies without contact points (13 less the base box, the shanks and the feet): exactly zero (the
    # buffers were poisoned with NaN)
    nopts = [b for b in range(13) if setup[2]["contact_count"][b] == 0]
    assert len(nopts) == 8 and not out["contact"][:, nopts].any()
    err = errors(c, out)
    worst, fails = {}, []
    for i, e in enumerate(err):
        kind = c["kinds"][i // rs.PER]
        for g, v in e.items():
            worst[(kind, g)] = max(worst.get((kind, g), 0.0), v)
            if v > BOUND:
                fails.append(f"{kind} env {i} {g}: |out - ref| / (1 + |ref|max) {v:.3g}\n{out['contact'][i]}\n{c['contact'][i]}")
    print(name, {f"{k[0]}.{k[1]}": f"{v:.1e}" for k, v in worst.items()})
    assert not fails, "\n".join(fails[:8])
    if name == "field":
        blind = errors(c, out, contact=c["blind"])
        for j, kind in enumerate(c["kinds"]):
            miss = max(e["force"] for e in blind[j * rs.PER:(j + 1) * rs.PER])
            assert miss >= 100 * BOUND, f"{kind}: a reference blind to the field is only {miss:.3g} away"


def test_inputs_cover_the_law(setup):
    """what the states exercise, from the reference alone"""
    dyn, m, tab = setup
    thr = float(m.bounce_threshold)
    pts, rows = [], []
    for name in ("plane", "field"):
        c = case(setup, name)
        for i, det in enumerate(c["detail"]):
            kind = c["kinds"][i // rs.PER]
            pts += [dict(d, env=(name, i), kind=kind) for d in det]
            rows.append((name, kind, i, c["contact"][i], c["vimp"][i]))
        for j, kind in enumerate(c["kinds"]):
            assert all(len(d) > 0 for d in c["detail"][j * rs.PER:(j + 1) * rs.PER]), f"{name} {kind}: an env without contact"
    terr = [p for p in pts if p["other"] is None]
    assert any(p["vn"] < 0 for p in terr), "no approaching point"
    assert any(p["vtg"] > 0 and 0 <= p["vn"] < p["vtg"] for p in terr), "no point separating below an active target"
    assert any(p["vn"] >= p["vtg"] and p["vn"] > 0 for p in terr), "no point separating on the spring alone"
    assert any(p["vtg"] > 0 and p["vn"] >= p["vtg"] for p in terr), "no point separating faster than an active target"
    assert min(p["raw"] for p in pts) > 0, "the law's clamp binds after all (see the module docstring)"
    vs = 0.01
    assert any(p["vt"] > vs for p in pts) and any(p["vt"] < vs for p in terr), "sliding and sticking points"
    selfp = [p for p in pts if p["other"] is not None]
    for body in (4, 10, 6, 12):
        assert any(p["body"] == body and np.abs(p["force"]).max() > 1.0 for p in selfp), f"no self-contact force on {body}"
    pairs = {frozenset((p["body"], p["other"])) for p in selfp}
    assert pairs & {frozenset(x) for x in ((4, 10), (4, 12), (6, 10), (6, 12))}, "no cross-leg pair"
    assert frozenset((4, 6)) in pairs and frozenset((10, 12)) in pairs, "a within-leg shank-foot pair is missing"
    # Newton's third law per self-contact pair: the two sides are evaluated separately
    for a in selfp:
        b = [p for p in selfp if p["env"] == a["env"] and p["body"] == a["other"] and p["other"] == a["body"]]
        assert len(b) == 1
        tol = BOUND * (1.0 + np.abs(a["force"]).max())
        assert np.abs(a["force"] + b[0]["force"]).max() <= tol, (a, b[0])
    # the base box with different episodes on its halves (one target above the threshold at least)
    assert any(np.abs(f[0]).max() > 1.0 and v[4] != v[5] and max(v[4], v[5]) > thr for _, _, _, f, v in rows), \
        "no base-box force with two different episodes"
    feet = np.array([f[b, 2] for _, _, _, f, _ in rows for b in (6, 12)])
    assert (feet > 5.0).any() and ((feet > 0.0) & (feet < 5.0)).any(), "feet f_z on one side of 5 N only"
    base = np.array([np.linalg.norm(f[0]) for _, _, _, f, _ in rows])
    assert (base > 1.0).any() and ((base > 0.0) & (base < 1.0)).any(), "base |f| on one side of 1 N only"
    print("points", len(pts), "self", len(selfp), "feet rows below 5 N", int(((feet > 0) & (feet < 5)).sum()),
          "base rows below 1 N", int(((base > 0) & (base < 1)).sum()))


def test_self_pair_forces_balance_in_the_product(setup):
    """the product evaluates each side of a self-contact pair on its own: summed over an airborne robot's shanks and
    feet (the plane's `self` kind: no terrain contact) the reported forces cancel within the bound"""
    c = case(setup, "plane")
    out = rs.host_report(setup, c, c["par"], 1)
    sl = slice(rs.PER, 2 * rs.PER)
    assert all(d["other"] is not None for det in c["detail"][sl] for d in det), "the self kind touches the plane"
    f = out["contact"][sl]
    assert np.abs(f).max() > 100.0
    assert (np.abs(f.sum(axis=1)).max(axis=1) <= BOUND * (1.0 + np.abs(f).max(axis=(1, 2)))).all()


@pytest.mark.parametrize("name,flags", [("plane", 1), ("field", 1), ("field", 3), ("field", 5), ("field", 9)])
def test_episodes_carry_through_ten_substeps(setup, name, flags):
    """the restitution episodes of the fp64 compositions (assembled, split, k_dyn5's and k_dyn6's roles) after each of
    ten substeps against ContactRobot.episodes_after at the same start state: open, keep, close.  The du tests compare
    the episodes after one substep of their own states; over ten, feet rebound, and a body whose points in contact
    all leave faster than 1 m/s must keep its episode (the header's "no contact" start value of the fastest approach
    is -1: compared with -v_n instead of max(-v_n, 0) it closed such an episode a substep early)"""
    c = case(setup, name)
    n = c["root"].shape[0]
    tau = np.random.default_rng(11).normal(0, 20, (n, 12))
    cur, fast = dict(c), 0
    for k in range(10):
        out = rs.host_report(setup, cur, c["par"], flags, nsub=1, tau=tau)
        for i in range(n):
            det = []
            ep = c["ref"].episodes_after(i, cur["root"][i], cur["dof"][i], cur["vimp"][i].astype(np.float64), detail=det)
            np.testing.assert_allclose(out["vimp"][i], ep, rtol=1e-5, atol=1e-6, err_msg=f"substep {k} env {i}")
            for slot in range(6):
                vn = [v for s_, v in det if s_ == slot]
                fast += bool(vn) and min(vn) > 1.0 and cur["vimp"][i][slot] > 0
        cur = dict(c, root=out["root"], dof=out["dof"], vimp=out["vimp"].astype(np.float32))
    if name == "field":
        assert fast > 0, "no open episode whose points all leave faster than 1 m/s"


def absolute_errors(c, ref, out, guard):
    """per group the worst absolute |out - ref| over the envs at the states `out` holds; force rows within the guard
    distance of a switching surface are left out: (worst per group, rows left out, rows of bodies with candidates)"""
    worst = dict.fromkeys(rs.GROUP_NAMES, 0.0)
    left, total = 0, 0
    for i in range(out["root"].shape[0]):
        rigid, contact = ref.report(i, out["root"][i], out["dof"][i], out["vimp"][i])
        e = rs.group_errors(out["rigid"][i], out["contact"][i], rigid, contact)
        near = ref.switch_distance(i, out["root"][i], out["dof"][i]) < guard
        left, total = left + int(near[[0, 4, 6, 10, 12]].sum()), total + 5
        for g in rs.GROUP_NAMES[:4]:
            worst[g] = max(worst[g], float(e[g][0]))
        worst["force"] = max(worst["force"], float(np.where(near, 0.0, e["force"][0]).max()))
    return worst, left, total


@pytest.mark.parametrize("name", ["plane", "field"])
def test_host_fp32_yardstick(setup, name, capsys):
    """the host fp32 builds (flags 0, 2) against the reference, absolute worst per group: on the given states (nsub 0)
    and at the end-of-step states of their own ten substeps -- the figures the GPU test's bound is 10 x of -- and the
    share of force rows within the guard distance after those ten substeps"""
    c = case(setup, name)
    tau = np.random.default_rng(11).normal(0, 20, (c["root"].shape[0], 12))
    lines = []
    for nsub in (0, 10):
        worst = dict.fromkeys(rs.GROUP_NAMES, 0.0)
        for flags in (0, 2):
            out = rs.host_report(setup, c, c["par"], flags, nsub=nsub, tau=tau)
            w, left, total = absolute_errors(c, c["ref"], out, rs.GUARD[name])
            worst = {g: max(worst[g], w[g]) for g in worst}
            assert left <= rs.GUARD_CAP * total, f"{name}: {left} of {total} force rows within the guard distance"
        lines.append(f"host fp32 report, {name}, after {nsub} substeps: worst |out - ref| "
                     + str({g: f"{v:.2e}" for g, v in worst.items()}) + f"; guarded rows {left} of {total}")
        for g, v in worst.items() if nsub else ():
            # (within 2 x: another compiler's contraction and summation order move an fp32 worst case)
            assert v <= 2 * rs.YARDSTICK[name][g], f"{name} {g}: host fp32 {v:.3g} is beyond twice the recorded yardstick"
    with capsys.disabled():
        print("\n" + "\n".join(lines))
