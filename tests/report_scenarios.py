"""Inputs and the comparison shared by the tests of the end-of-step report (rigid_state, contact_forces):
tests/test_dynamics_report.py (host builds) and tests/test_gpu_dynamics_report.py (the step kernels).

Two cases of 64 envs, 16 per kind:
  plane  stance, self, limits, impact  (tests/test_dynamics_contact.py scenario() and _place_on_ground)
  field  slope, impact, edge, base     (tests/terrain_contact_scenarios.py on its synthetic height field)
The du tests keep their own inputs; these are drawn with seeds of their own and a few envs per kind are varied so that
every branch of the report's force law occurs (the tests assert that on the reference):
  plane stance 12-15  velocities scaled to mm/s: sticking friction (|v_t| < v_s); env 15 touches 30 um deep: a foot row
                      below the 5 N contact threshold
  plane self 12-15    an ankle pitched until the foot's capsule enters its own leg's shank capsule (the within-leg pair)
  plane impact 8-15   rebounding: moving up slowly with episodes open above the bounce threshold (separating below an
                      active restitution target) and a high restitution draw
  field slope 15      at rest, 30 um deep
  field base 8-15     the base box's two halves carry different episodes; env 15 at rest, 6 um deep (|f| < 1 N)
All states are fp32-exact.
"""
import ctypes as C

import numpy as np

import terrain_contact_scenarios as tcs
from oracle.dynamics_ref import ContactRobot, MeshTerrain, quat_to_R
from test_dynamics_contact import _place_on_ground, scenario as plane_scenario

PLANE_KINDS = ("stance", "self", "limits", "impact")
PER = 16
GROUPS = {"pos": slice(0, 3), "quat": slice(3, 7), "vel": slice(7, 10), "ang": slice(10, 13)}
GROUP_NAMES = ("pos", "quat", "vel", "ang", "force")
ULP = 2.0 ** -23
# The force law jumps by d |v_n| (1500 N per m/s) where a terrain point's depth h - z crosses zero, and at capsule
# distance r_a + r_b.  A body row is left out of the FORCE comparison when one of its candidates is within GUARD of that
# surface, GUARD from fp32 rounding of the coordinates involved: a point's world position is the base position (|z| ~
# 1 m, ulp 2^-23 = 1.2e-7 m) plus a chain of six rotations and offsets, each rounding at the same scale -- 4 ulp at 1 m.
# On the field the height under the point moves with its x and y (up to 4 m: ulp 2^-22, again 4 of them) times the
# slope, at most 2.5 on the step's ramp (0.25 m over one 0.1 m cell).
GUARD = {"plane": 4 * ULP, "field": 4 * ULP + 2.5 * 4 * 2 * ULP}
# The host fp32 builds' worst absolute distance from the reference per group (m, 1, m/s, rad/s, N) at the end-of-step
# states of their own ten substeps from the cases' states, as tests/test_dynamics_report.py::test_host_fp32_yardstick
# measures it (1.42e-7, 2.70e-7, 2.14e-6, 3.72e-6, 0.368 on the plane; 1.37e-7, 3.19e-7, 1.25e-6, 2.97e-6, 0.0465 on the
# field; rounded up here).  The GPU test allows 10 x this plus one fp32 ulp of the env's largest magnitude in the group.
YARDSTICK = {"plane": {"pos": 1.5e-7, "quat": 2.8e-7, "vel": 2.2e-6, "ang": 3.8e-6, "force": 0.37},
             "field": {"pos": 1.4e-7, "quat": 3.2e-7, "vel": 1.3e-6, "ang": 3.0e-6, "force": 0.047}}
GUARD_CAP = 0.05    # of the (env, body) rows of bodies that have contact candidates (5 per env)


def _fp32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def plane_case(tab):
    rob = ContactRobot(tab, solver={})
    roots, dofs, vimps, bouncy = [], [], [], []
    for j, kind in enumerate(PLANE_KINDS):
        rng = np.random.default_rng(40 + j)
        root, dof = plane_scenario(kind, PER, rng, tab)
        vimp = np.zeros((PER, 6), np.float32)
        b = np.zeros(PER, bool)
        if kind == "stance":
            root[12:, 7:13] *= 0.02
            dof[12:, :, 1] *= 0.02
        if kind == "self":
            dof[12:14, 4, 0] = -rng.uniform(1.2, 1.5, 2)
            dof[14:16, 10, 0] = -rng.uniform(1.2, 1.5, 2)
        if kind == "impact":
            root[:8, 9] = -rng.uniform(0.8, 1.5, 8)
            root[8:, 9] = rng.uniform(0.02, 0.15, 8)
            vimp = np.where(rng.uniform(size=(PER, 6)) < 0.6, rng.uniform(0.6, 2.0, (PER, 6)), 0.0).astype(np.float32)
            vimp[8:] = rng.uniform(1.0, 2.0, (8, 6))
            b[8:] = True
        root, dof = _fp32(root), _fp32(dof)
        _place_on_ground(rob, root, dof, rng, depth=(0.001, 0.004) if kind != "self" else (-0.05, -0.02))
        if kind == "stance":
            _place_on_ground(rob, root[15:], dof[15:], rng, depth=(3e-5, 3e-5))
        roots.append(_fp32(root))
        dofs.append(dof)
        vimps.append(vimp)
        bouncy.append(b)
    return {"name": "plane", "kinds": PLANE_KINDS, "root": np.concatenate(roots), "dof": np.concatenate(dofs),
            "vimp": np.concatenate(vimps), "bouncy": np.concatenate(bouncy), "terrain": None, "field": None}


def field_case(tab):
    field = tcs.make_field()
    # the mesh at the scales the Terrain struct holds: fp32 vertical scale and border, and the horizontal scale as its
    # fp32 reciprocal (1 / fp32(0.1) rounds to 10).  On a row of a few N the bound is below what the fp64 0.005 against
    # the fp32 one moves a height of 300 raw units by (3e-8 m, 3e-3 N through k).
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    terrain = MeshTerrain(field, 1.0 / float(np.float32(1.0) / np.float32(tcs.HS)), f32(tcs.VS), f32(tcs.BORDER))
    rob = ContactRobot(tab, solver={}, terrain=terrain)
    roots, dofs, vimps, bouncy, facts = [], [], [], [], []
    for j, kind in enumerate(tcs.KINDS):
        root, dof, vimp, f = tcs.scenario(kind, tab, tcs.mesh_terrain(field))
        tcs.check_kind(kind, f, vimp)
        rng = np.random.default_rng(60 + j)
        b = np.zeros(PER, bool)
        if kind == "slope":
            root[15, 7:13] *= 0.002
            dof[15, :, 1] *= 0.002
            root, dof = _fp32(root), _fp32(dof)
            tcs._settle(rob, root[15], dof[15], 3e-5)
        if kind == "base":
            vimp = vimp.copy()
            vimp[8:, 4] = rng.uniform(0.6, 2.0, 8)
            vimp[8:, 5] = np.where(np.arange(8) % 2 == 0, 0.0, rng.uniform(0.6, 2.0, 8))
            b[8:] = True
            root[15, 7:13] *= 0.002
            dof[15, :, 1] *= 0.002
            root, dof = _fp32(root), _fp32(dof)
            vimp[15] = 0.0
            tcs._settle(rob, root[15], dof[15], 6e-6)
        roots.append(root)
        dofs.append(dof)
        vimps.append(vimp.astype(np.float32))
        bouncy.append(b)
        facts += f
    return {"name": "field", "kinds": tcs.KINDS, "root": np.concatenate(roots), "dof": np.concatenate(dofs),
            "vimp": np.concatenate(vimps), "bouncy": np.concatenate(bouncy), "terrain": terrain, "field": field}


def host_params(m, case, seed=5):
    """per-env masses, COM displacement, friction and restitution for the host builds (the GPU test reads the env's)"""
    n = case["root"].shape[0]
    rng = np.random.default_rng(seed)
    par = {"bm": (m.mass[0] + rng.uniform(-1.0, 1.0, n)).astype(np.float32),
           "ls": rng.uniform(0.9, 1.1, (n, 12)).astype(np.float32),
           "cd": rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32),
           "arm": np.full((n, 12), 0.1, np.float32),
           "fr": rng.uniform(0.2, 1.3, n).astype(np.float32),
           "rst": rng.uniform(0.0, 0.4, n).astype(np.float32)}
    par["rst"][case["bouncy"]] = rng.uniform(0.3, 0.4, int(case["bouncy"].sum())).astype(np.float32)
    return par


def host_report(setup, case, par, flags, mesh=2, nsub=0, tau=None, dt=0.001):
    """t1dyn_substeps on the case's states: {root, dof, vimp after nsub substeps (fp32-exact), rigid, contact}; the
    report buffers are poisoned with NaN before the call (nsub = 0: the report of the state as given)"""
    dyn, m, _ = setup
    n = case["root"].shape[0]
    fp = C.POINTER(C.c_float)
    r = np.ascontiguousarray(case["root"], np.float32).copy()
    d = np.ascontiguousarray(case["dof"].reshape(n, 24), np.float32).copy()
    vi = np.ascontiguousarray(case["vimp"], np.float32).copy()
    t = np.ascontiguousarray(np.zeros((n, 12)) if tau is None else tau, np.float32)
    rigid = np.full((n, 13, 13), np.nan, np.float32)
    contact = np.full((n, 13, 3), np.nan, np.float32)
    if case["field"] is None:
        hf, hs, vs, border, mesh = np.zeros((2, 2), np.int16), 0.1, 0.005, 0.0, 0
    else:
        hf, hs, vs, border = np.ascontiguousarray(case["field"], np.int16), tcs.HS, tcs.VS, tcs.BORDER
    rc = dyn.t1dyn_substeps(C.byref(m), n, flags, r.ctypes.data_as(fp), d.ctypes.data_as(fp), t.ctypes.data_as(fp),
                            par["bm"].ctypes.data_as(fp), par["ls"].ctypes.data_as(fp), par["cd"].ctypes.data_as(fp),
                            par["arm"].ctypes.data_as(fp), par["fr"].ctypes.data_as(fp), par["rst"].ctypes.data_as(fp),
                            vi.ctypes.data_as(fp), None, C.c_float(dt), nsub, hf.ctypes.data_as(C.POINTER(C.c_int16)),
                            hf.shape[0], hf.shape[1], C.c_float(hs), C.c_float(vs), C.c_float(border), mesh,
                            rigid.ctypes.data_as(fp), contact.ctypes.data_as(fp))
    assert rc == 0
    return {"root": r.astype(np.float64), "dof": d.astype(np.float64).reshape(n, 12, 2), "vimp": vi.astype(np.float64),
            "rigid": rigid.astype(np.float64), "contact": contact.astype(np.float64)}


class Reference:
    """ContactRobot.report per env from Gym-layout rows (root with the base's COM velocity, dof (12, 2)), each env
    with its own COM displacement, friction and restitution"""

    def __init__(self, tab, m, solver, par, terrain):
        # the model as the builds hold it: its struct keeps the link geometry in fp32 (a foot point's height moves by
        # ~1e-8 m against the fp64 table, 1e-3 N through k -- as much as the whole bound on a 5 N row)
        tab = dict(tab, **{k: np.asarray(tab[k], np.float32).astype(np.float64).tolist()
                           for k in ("joint_offset", "joint_axis", "com", "contact_point")})
        self.tab, self.par, self.terrain = tab, {k: np.asarray(v, np.float64) for k, v in par.items()}, terrain
        self.solver = dict(solver, bounce_threshold=float(m.bounce_threshold))
        self.gf, self.gr = float(m.ground_friction), float(m.ground_restitution)
        self.com0 = np.asarray(tab["com"], float)[0]

    def robot(self, i, blind=False):
        return ContactRobot(self.tab, com_disp=self.par["cd"][i], solver=self.solver,
                            terrain=None if blind else self.terrain)

    def _state(self, i, root, dof):
        quat = root[3:7]   # as given (fp32 rows are unit to 6e-8), like the du tests
        w = root[10:13]
        vo = root[7:10] - np.cross(w, quat_to_R(quat) @ (self.com0 + self.par["cd"][i]))
        return root[0:3], quat, w, vo, dof[:, 0], dof[:, 1]

    def report(self, i, root, dof, vimp, detail=None, blind=False):
        fr, rst = self.par["fr"][i], self.par["rst"][i]
        return self.robot(i, blind).report(*self._state(i, root, dof), vimp, 0.5 * (fr + self.gf),
                                           0.5 * (rst + self.gr), fr, detail=detail)

    def episodes_after(self, i, root, dof, vimp, detail=None):
        return self.robot(i).episodes_after(*self._state(i, root, dof), vimp, detail=detail)

    def switch_distance(self, i, root, dof):
        p, quat, _, _, q, _ = self._state(i, root, dof)
        return self.robot(i).switch_distance(p, quat, q)


def group_errors(rigid, contact, ref_rigid, ref_contact):
    """{group: (|out - ref|_max, |ref|_max)} of one env; quaternions compared up to sign; the force group per body row
    (13,) so that rows can be left out"""
    out = {}
    for g, sl in GROUPS.items():
        a, b = rigid[:, sl], ref_rigid[:, sl]
        if g == "quat":
            a = a * np.where((a * b).sum(1, keepdims=True) < 0, -1.0, 1.0)
        out[g] = (np.abs(a - b).max(), np.abs(b).max())
    out["force"] = (np.abs(contact - ref_contact).max(axis=1), np.abs(ref_contact).max())
    return out
