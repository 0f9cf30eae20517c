"""utils/urdf.visual_meshes on a robot description whose every mesh file exists: the fixture URDF, the two real ankle
STLs and 12-triangle boxes under the other 22 names (tests/render_scenes_mesh.synth_robot).  The arm chain is recomputed
here from the XML, in float64 and with this file's own rpy code."""
import os
import shutil
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_scenes_mesh as SM  # noqa: E402
from ti5_isaacgym_amd.utils import urdf as U  # noqa: E402


def _rot(rpy):
    """URDF fixed-axis roll, pitch, yaw: R = Rz(yaw) Ry(pitch) Rx(roll), written out element by element."""
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], dtype=np.float64)


def _pose(el):
    o = el.find("origin")
    xyz = np.array((o.get("xyz") if o is not None and o.get("xyz") else "0 0 0").split(), dtype=np.float64)
    rpy = (o.get("rpy") if o is not None and o.get("rpy") else "0 0 0").split()
    return xyz, _rot(rpy)


@pytest.fixture(scope="module")
def robot(tmp_path_factory):
    return SM.synth_robot(str(tmp_path_factory.mktemp("robot")))


def test_twenty_four_links_on_thirteen_bodies(robot):
    m = U.visual_meshes(robot)
    assert len(m["links"]) == 24 and len(set(m["links"])) == 24 and m["skipped"] == []
    assert sorted(set(m["body"].tolist())) == list(range(13))
    assert m["tri"].dtype == np.float32 and m["body"].dtype == np.int32 and m["link"].dtype == np.int32
    T = len(m["tri"])
    assert m["tri"].shape == (T, 3, 3) and m["body"].shape == (T,) and m["link"].shape == (T,)
    assert T == 22 * 12 + len(SM.ankle("L")) + len(SM.ankle("R"))
    # the base group: pelvis, three waist links, eight arm links
    base = {m["links"][k] for k in set(m["link"][m["body"] == 0].tolist())}
    assert len(base) == 12 and "base_link" in base and "L_ELBOW_P_S" in base and "WAIST_Y_S" in base
    for b in range(1, 13):
        assert {m["links"][k] for k in set(m["link"][m["body"] == b].tolist())} == {U.BODY_NAMES[b]}


def test_a_leg_links_vertices_are_the_files_own(robot):
    m = U.visual_meshes(robot)
    for side, b in (("L", 6), ("R", 12)):
        assert np.array_equal(m["tri"][m["body"] == b], SM.ankle(side))
    knee = U.load_stl(os.path.join(os.path.dirname(robot), "..", "meshes", "L_KNEE_P_S.STL")).reshape(-1, 3, 3)
    assert np.array_equal(m["tri"][m["body"] == 4], knee.astype(np.float32))


def test_the_elbow_goes_through_four_fixed_joints(robot):
    root = ET.parse(robot).getroot()
    joints = {j.get("name"): j for j in root.findall("joint")}
    chain = ["L_SHOULDER_P", "L_SHOULDER_R", "L_SHOULDER_Y", "L_ELBOW_P"]
    assert joints[chain[-1]].find("child").get("link") == "L_ELBOW_P_S"
    for a, b in zip(chain, chain[1:]):
        assert joints[a].find("child").get("link") == joints[b].find("parent").get("link")
    # up to the base: the chain hangs on the waist, which hangs on base_link through three more fixed joints
    up, link = [], joints[chain[0]].find("parent").get("link")
    while link != "base_link":
        j = next(j for j in joints.values() if j.find("child").get("link") == link)
        assert j.get("type") == "fixed"
        up.append(j.get("name"))
        link = j.find("parent").get("link")
    p, R = np.zeros(3), np.eye(3)
    for name in up[::-1] + chain:
        assert joints[name].get("type") == "fixed"
        xyz, Rj = _pose(joints[name])
        p, R = p + R @ xyz, R @ Rj
    vis = next(l for l in root.findall("link") if l.get("name") == "L_ELBOW_P_S").find("visual")
    vx, vR = _pose(vis)
    v = U.load_stl(os.path.join(os.path.dirname(robot), "..", "meshes", "L_ELBOW_P_S.STL")).astype(np.float64)
    want = ((v @ vR.T + vx) @ R.T + p).reshape(-1, 3, 3)
    m = U.visual_meshes(robot)
    got = m["tri"][m["link"] == m["links"].index("L_ELBOW_P_S")]
    assert got.shape == want.shape == (12, 3, 3) and (m["body"][m["link"] == m["links"].index("L_ELBOW_P_S")] == 0).all()
    assert np.abs(got - want).max() <= 1e-6
    assert np.linalg.norm(p) > 0.3   # the chain is not the identity: the elbow is well away from the pelvis


def test_missing_files_scale_and_non_mesh_visuals(robot, tmp_path):
    dst = str(tmp_path / "copy")
    shutil.copytree(os.path.dirname(os.path.dirname(robot)), dst)
    urdf = os.path.join(dst, "urdf", "t1.urdf")
    os.remove(os.path.join(dst, "meshes", "WAIST_Y_S.STL"))
    with pytest.raises(FileNotFoundError, match="WAIST_Y_S.STL"):
        U.visual_meshes(urdf)
    m = U.visual_meshes(urdf, missing_ok=True)
    assert len(m["links"]) == 23 and "WAIST_Y_S" not in m["links"]
    assert len(m["skipped"]) == 1 and m["skipped"][0].endswith("WAIST_Y_S.STL")
    # ASCII STL, and a scale attribute
    tri = SM.box_tris((-0.1, -0.2, -0.3), (0.1, 0.2, 0.3))
    with open(os.path.join(dst, "meshes", "WAIST_Y_S.STL"), "w") as f:
        f.write("solid box\n")
        for t in tri:
            f.write("facet normal 0 0 0\n outer loop\n" + "".join("  vertex %r %r %r\n" % tuple(float(x) for x in v) for v in t) +
                    " endloop\nendfacet\n")
        f.write("endsolid box\n")
    text = open(urdf).read()
    assert text.count('filename="../meshes/L_KNEE_P_S.STL" />') == 1
    open(urdf, "w").write(text.replace('filename="../meshes/L_KNEE_P_S.STL" />',
                                       'filename="../meshes/L_KNEE_P_S.STL" scale="2 3 0.5" />'))
    m = U.visual_meshes(urdf)
    assert len(m["links"]) == 24 and (m["link"] == m["links"].index("WAIST_Y_S")).sum() == 12
    knee = U.load_stl(os.path.join(dst, "meshes", "L_KNEE_P_S.STL")).reshape(-1, 3, 3)
    assert np.array_equal(m["tri"][m["body"] == 4], (knee * (2, 3, 0.5)).astype(np.float32))
    # a visual that is not a mesh
    text = open(urdf).read()
    a = text.index("<mesh", text.index('name="base_link"'))
    b = text.index("/>", a) + 2
    open(urdf, "w").write(text[:a] + '<box size="0.1 0.1 0.1" />' + text[b:])
    with pytest.raises(ValueError, match="base_link"):
        U.visual_meshes(urdf)


def test_articulation_is_what_it_was():
    """visual_meshes shares the collapse with Articulation: the compiled model of the fixture is still the committed one."""
    import json
    got = U.compile_model(os.path.join(SM.ROBOT, "urdf", "t1.urdf"))
    with open(U.RESOURCE) as f:
        want = json.load(f)
    for k in ("mass", "com", "inertia", "joint_offset", "contact_point", "self_box"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
