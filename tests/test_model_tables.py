"""The committed model tables (ti5_isaacgym_amd/resources/t1_model.json) against the robot description itself -- no GPU.

The kernels (build_model, t1_model_conv.h) and every fp64 reference of oracle/dynamics_ref.py read the same tables, the
description's 24 links collapsed to 13 bodies by utils/urdf.py, so a wrong collapse moves both sides of every physics
test together.  Here the description is a fixture (tests/golden/t1_robot: t1.urdf and the two foot meshes it reads) and

  a. compile_model(fixture) reproduces the committed JSON (a stale or hand-edited table fails);
  b. tests/urdf_links.py -- an independent reader that keeps all 24 links as rigid bodies of their own -- gives the same
     mass matrix and accelerations as oracle/dynamics_ref.py Robot on the tables, at 16 random states:
       |M_links - M_tables| <= 1e-8 max|M|,  |a_links - a_tables| <= 1e-5 (1 + max|a_tables|)
     (the two finite-difference formulations agree to 9.2e-11 and 4.5e-8; 1e-5 is test_dynamics_contact.py's bound for
     fp64 against fp64);
  c. limits and joint axes per DOF name, read by the new reader;
  d. the contact and self-collision geometry recomputed with plain loops;
  e. the model constants oracle/t1_oracle.py states a second time;
  f. four one-line mutants of the collapse each miss a bound of b by >= 100 x (profiles/model_tables_mutants.txt).
"""
import json
import os
import struct
import types

import numpy as np
import pytest

import urdf_links
from oracle.dynamics_ref import Robot

N_STATES = 16
M_BOUND, A_BOUND = 1e-8, 1e-5


@pytest.fixture(scope="module")
def tab():
    from ti5_isaacgym_amd.utils.urdf import RESOURCE
    with open(RESOURCE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tree(tab):
    return urdf_links.LinkTree(urdf_links.FIXTURE, tab["dof_names"])


@pytest.fixture(scope="module")
def link_side(tab, tree):
    """the 16 states of b and the raw tree's (a, M) at each, computed once"""
    rng = np.random.default_rng(1)
    lim = np.asarray(tab["limits"])
    states = []
    for _ in range(N_STATES):
        quat = rng.standard_normal(4)
        quat /= np.linalg.norm(quat)
        s = dict(p=rng.standard_normal(3), quat=quat, q=np.clip(rng.uniform(-0.5, 0.5, 12), lim[:, 0], lim[:, 1]),
                 qd=np.clip(rng.normal(0, 1.5, 12), -0.3 * lim[:, 3], 0.3 * lim[:, 3]), w=rng.normal(0, 0.8, 3),
                 v=rng.normal(0, 0.5, 3), tau=rng.normal(0, 20, 12), arm=rng.uniform(0.01, 0.05, 12))
        states.append(s)
    out = [tree.accel(s["p"], s["quat"], s["w"], s["v"], s["q"], s["qd"], s["tau"], s["arm"]) for s in states]
    return states, out


def tables_against_links(tab, link_side):
    """(worst |M_links - M_tables| / max|M|, worst |a_links - a_tables| / (1 + max|a_tables|)) over the states"""
    states, links = link_side
    wm = wa = 0.0
    for s, (a1, M1) in zip(states, links):
        a0, M0 = Robot(tab, armature=s["arm"]).accel(s["p"], s["quat"], s["w"], s["v"], s["q"], s["qd"], s["tau"])
        wm = max(wm, np.abs(M1 - M0).max() / np.abs(M0).max())
        wa = max(wa, np.abs(a1 - a0).max() / (1.0 + np.abs(a0).max()))
    return wm, wa


# ---- a ------------------------------------------------------------------------------------------------------------
def _same(path, got, want):
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), f"{path}: keys {sorted(got)} vs {sorted(want)}"
        for k in want:
            _same(f"{path}.{k}", got[k], want[k])
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), f"{path}: length"
        for i, (g, w) in enumerate(zip(got, want)):
            _same(f"{path}[{i}]", g, w)
    elif isinstance(want, float):
        assert isinstance(got, (int, float)) and abs(got - want) <= 1e-12 * abs(want), f"{path}: {got!r} vs {want!r}"
    else:
        assert type(got) is type(want) and got == want, f"{path}: {got!r} vs {want!r}"


def test_compiled_fixture_equals_committed_tables(tab):
    from ti5_isaacgym_amd.utils.urdf import compile_model
    got = json.loads(json.dumps(compile_model(urdf_links.FIXTURE)))   # through JSON, like the committed file
    _same("t1_model", got, tab)


# ---- b ------------------------------------------------------------------------------------------------------------
def test_raw_link_tree_matches_collapsed_tables(tab, tree, link_side):
    kinds = [j["type"] for j in tree.joints.values()]
    assert (len(tree.links), kinds.count("fixed"), kinds.count("revolute")) == (24, 11, 12)
    wm, wa = tables_against_links(tab, link_side)
    print(f"raw tree against tables over {N_STATES} states: M {wm:.2e} (bound {M_BOUND:g}), a {wa:.2e} (bound {A_BOUND:g})")
    assert wm <= M_BOUND, wm
    assert wa <= A_BOUND, wa
    total = float(tree.masses().sum())
    assert abs(total - 55.746) <= 1e-9 and abs(sum(tab["mass"]) - total) <= 1e-12 * total, (total, sum(tab["mass"]))


# ---- c ------------------------------------------------------------------------------------------------------------
def _body_link(tree, link):
    """the link whose body a link belongs to after the collapse: up through fixed joints"""
    up = {j["child"]: j for j in tree.joints.values()}
    while link in up and up[link]["type"] == "fixed":
        link = up[link]["parent"]
    return link


def test_limits_axes_and_topology(tab, tree):
    names = tab["body_names"]
    assert len(tab["dof_names"]) == 12 and len(names) == 13 and names[0] == tree.root
    for k, jn in enumerate(tab["dof_names"]):
        j = tree.joints[jn]
        assert j["type"] == "revolute", jn
        lim = j["limit"]
        assert tab["limits"][k] == [lim["lower"], lim["upper"], lim["effort"], lim["velocity"]], jn
        b = names.index(j["child"])
        assert b == k + 1, f"{jn}: DOF {k} moves body {b}"   # the kernels index joint k's body as k + 1
        assert tab["joint_axis"][b] == list(j["axis"]) and abs(np.linalg.norm(j["axis"]) - 1.0) < 1e-12, jn
        assert np.array_equal(j["R"], np.eye(3)), f"{jn} carries an rpy the tables cannot hold"
        assert tab["parent"][b] == names.index(_body_link(tree, j["parent"])), jn
        assert j["parent"] in names, f"{jn} hangs off a merged link: joint_offset would need that link's transform"
        assert tab["joint_offset"][b] == list(j["xyz"]), jn
    assert tab["parent"][0] == -1
    # every link belongs to exactly one of the 13 bodies
    assert sorted({_body_link(tree, ln) for ln in tree.links}) == sorted(names)


# ---- d ------------------------------------------------------------------------------------------------------------
def _stl_vertices(path):
    """the vertices of a binary STL, triangle by triangle"""
    with open(path, "rb") as f:
        b = f.read()
    n = struct.unpack_from("<I", b, 80)[0]
    assert len(b) == 84 + 50 * n, "not a binary STL"
    out = []
    for t in range(n):
        vals = struct.unpack_from("<12f", b, 84 + 50 * t)
        for k in range(3):
            out.append([float(vals[3 + 3 * k]), float(vals[4 + 3 * k]), float(vals[5 + 3 * k])])
    return out


def _collisions(tree, tab):
    """{body index: [(kind, data, xyz, R)]} with the collision origin in the body's frame (all joints at zero)"""
    fr = tree.frames(np.zeros(3), np.eye(3), np.zeros(12))
    out = {}
    for ln, el in tree.elements.items():
        body = _body_link(tree, ln)
        (pb, Rb), (pl, Rl) = fr[body], fr[ln]
        for col in el.findall("collision"):
            cx, cR = urdf_links.origin(col)
            g = col.find("geometry")[0]
            xyz, R = Rb.T @ (pl + Rl @ cx - pb), Rb.T @ Rl @ cR
            if g.tag == "box":
                item = ("box", urdf_links.floats(g.get("size")), xyz, R)
            else:
                assert g.tag == "mesh", g.tag
                path = os.path.normpath(os.path.join(os.path.dirname(tree.path), g.get("filename")))
                item = ("mesh", _stl_vertices(path), xyz, R)
            out.setdefault(tab["body_names"].index(body), []).append(item)
    return out


def _rows(a):
    return sorted(tuple(float(x) for x in r) for r in a)


def test_contact_and_self_collision_geometry(tab, tree):
    from ti5_isaacgym_amd.utils.urdf import FOOT_POINT_DIRS, SELF_BODIES, self_capsules
    cols = _collisions(tree, tab)
    feet = [i for i, n in enumerate(tab["body_names"]) if n.endswith("6_link")]
    shanks = [i for i, n in enumerate(tab["body_names"]) if n.endswith("4_link")]
    assert sorted(cols) == sorted([0] + feet + shanks) and all(len(v) == 1 for v in cols.values())
    assert list(SELF_BODIES) == sorted(feet + shanks)
    pts = tab["contact_point"]
    nxt = 0
    for b in range(13):
        if b not in cols:
            assert tab["contact_count"][b] == 0 and tab["contact_start"][b] == 0, b
            continue
        assert tab["contact_count"][b] == 8 and tab["contact_start"][b] == nxt, b
        assert tab["contact_body"][nxt:nxt + 8] == [b] * 8
        got = pts[nxt:nxt + 8]
        nxt += 8
        kind, data, xyz, R = cols[b][0]
        if kind == "box":
            want = []
            for sx in (-1, 1):
                for sy in (-1, 1):
                    for sz in (-1, 1):
                        want.append(xyz + R @ (np.array([sx, sy, sz]) * data / 2))
            np.testing.assert_allclose(_rows(got), _rows(want), rtol=0, atol=1e-15, err_msg=f"box corners of body {b}")
            if b == 0:   # the base box is pitched by 0.115 rad about y
                assert abs(np.arctan2(R[0, 2], R[0, 0]) - 0.115) < 1e-12 and abs(R[1, 1] - 1.0) < 1e-15
            else:
                assert np.array_equal(R, np.eye(3))
                np.testing.assert_allclose(tab["self_box"][list(SELF_BODIES).index(b)], list(xyz) + list(data / 2),
                                           rtol=0, atol=1e-15)
        else:
            verts = [xyz + R @ np.array(v) for v in data]
            for d, g in zip(FOOT_POINT_DIRS, got):
                best, arg = -np.inf, None
                for v in verts:
                    s = v[0] * d[0] + v[1] * d[1] + v[2] * d[2]
                    if s > best:
                        best, arg = s, v
                assert np.abs(np.array(g) - arg).max() <= 1e-15, f"foot {b} direction {d}: {g} vs {arg}"
            box = tab["self_box"][list(SELF_BODIES).index(b)]
            for v in verts:
                for k in range(3):
                    assert abs(v[k] - box[k]) <= box[3 + k] + 1e-12, f"foot {b}: vertex {v} outside its self_box"
    assert nxt == len(pts) == len(tab["contact_body"]) == 40
    for cap, box in zip(self_capsules(tab), tab["self_box"]):
        a, e, r = cap[0:3], cap[3:6], cap[6]
        assert r > 0
        for end in (a, e):
            for k in range(3):
                assert abs(end[k] - box[k]) + r <= box[3 + k] + 1e-12, f"capsule {cap} leaves its box {box}"


# ---- e ------------------------------------------------------------------------------------------------------------
def test_oracle_constants_equal_tables(tab):
    from oracle import t1_oracle as o
    lim = np.asarray(tab["limits"])
    assert np.array_equal(o.EFFORT, lim[:, 2].astype(np.float32))
    assert np.array_equal(o.TORQUE_LIMITS, (lim[:, 2].astype(np.float32) * np.float32(0.85)).astype(np.float32))
    assert abs(o.BASE_MASS - tab["mass"][0]) <= 1e-12 * tab["mass"][0], (o.BASE_MASS, tab["mass"][0])
    names = tab["body_names"]
    assert o.NUM_BODIES == len(names) and o.NUM_ACTIONS == len(tab["dof_names"])
    assert o.BASE == names.index("base_link")
    assert list(o.FEET) == [i for i, n in enumerate(names) if "6_link" in n]    # legged_robot.py's name matches
    assert list(o.KNEES) == [i for i, n in enumerate(names) if "4_link" in n]


# ---- f ------------------------------------------------------------------------------------------------------------
def _lightest_fixed_leaf(tree):
    leaves = [j["child"] for j in tree.joints.values() if j["type"] == "fixed" and j["child"] not in tree.children]
    return min(leaves, key=lambda n: tree.links[n][0])


MUTANTS = {
    "inertial rotation transposed": ("pieces.append((m, c, Rb @ Il @ Rb.T))", "pieces.append((m, c, Rb.T @ Il @ Rb))"),
    "fixed joint's Rj dropped": ("item = (child, p + R @ xyz, R @ Rj)", "item = (child, p + R @ xyz, R)"),
    "parallel-axis term dropped": ("Ic += Ii + m * (np.dot(d, d) * np.eye(3) - np.outer(d, d))", "Ic += Ii"),
    "one fixed descendant skipped": ('if j.get("type") != "fixed":',
                                     'if j.get("type") != "fixed" or j.find("child").get("link") == "{leaf}":'),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_collapse_mutant_misses_the_raw_tree(name, tab, tree, link_side):
    import ti5_isaacgym_amd.utils.urdf as real
    old, new = MUTANTS[name]
    leaf = _lightest_fixed_leaf(tree)
    with open(real.__file__) as f:
        src = f.read()
    assert src.count(old) == 1, f"{name}: the line to mutate is not in utils/urdf.py"
    mod = types.ModuleType("urdf_mutant")
    mod.__file__ = real.__file__
    exec(compile(src.replace(old, new.replace("{leaf}", leaf)), "urdf_mutant.py", "exec"), mod.__dict__)
    mut = json.loads(json.dumps(mod.compile_model(urdf_links.FIXTURE)))
    wm, wa = tables_against_links(mut, link_side)
    print(f"mutant '{name}'" + (f" ({leaf}, {tree.links[leaf][0]} kg)" if "skipped" in name else "")
          + f": M {wm:.2e} = {wm / M_BOUND:.3g} x its bound, a {wa:.2e} = {wa / A_BOUND:.3g} x its bound")
    assert max(wm / M_BOUND, wa / A_BOUND) >= 100.0
