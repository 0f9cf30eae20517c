"""The robot-mesh camera's host side, no device needed: the C ABI (declared, exported, bound, a C header), the refusals
that come before any device work, play's --render_urdf, the Renderer's and RobotMesh's surface, and scene 1 of
tests/render_scenes_mesh.py under the fp64 reference (the ambiguity cap, and that the scene shows what it is for)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import render_ref_mesh as RM  # noqa: E402
import render_scenes_mesh as SM  # noqa: E402
from ti5_isaacgym_amd import _lib  # noqa: E402

NEW = ["t1render_mesh_create", "t1render_mesh_destroy", "t1render_mesh_info", "t1render_mesh_workspace_bytes",
       "t1render_mesh_scene"]


def _lib_built():
    from ti5_isaacgym_amd import build as b
    b.build()
    return _lib.load()


def test_c_abi_is_declared_exported_and_bound():
    from ti5_isaacgym_amd import build as b
    src = " ".join(open(os.path.join(REPO, "include", "t1render.h")).read().split())
    for decl in ("typedef struct t1render_mesh t1render_mesh;",
                 "int t1render_mesh_create(const float* tri, const int32_t* body, const uint32_t* rgb, int32_t ntri, "
                 "t1render_mesh** out);",
                 "int t1render_mesh_destroy(t1render_mesh* m);",
                 "int t1render_mesh_info(const t1render_mesh* m, int32_t* ntri, int32_t* nnodes, int32_t* max_depth, "
                 "float* radius /*[13]*/);",
                 "#define T1RENDER_MESH_BRUTE 8 ",
                 "long long t1render_mesh_workspace_bytes(int32_t num_envs, int32_t ncams);",
                 "int t1render_mesh_scene(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_mesh* mesh, "
                 "const t1render_style* style, int32_t flags, int32_t width, int32_t height, uint32_t* rgba, float* depth, "
                 "int32_t* ids, int32_t* envs, int32_t* tris, void* workspace, long long workspace_bytes, void* stream);"):
        assert decl in src, decl
    assert _lib.RENDER_MESH_EXPORTS == NEW and _lib.RENDER_MESH_BRUTE == 8
    assert not set(NEW) & set(_lib.EXPORTS + _lib.POLICY_EXPORTS + _lib.RENDER_EXPORTS + _lib.RENDER_SCENE_EXPORTS)
    assert ("t1render_mesh.hip", "-O3") in b.UNITS
    lib = _lib_built()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    vp, i32, C = _lib.C.c_void_p, _lib.C.c_int32, _lib.C
    P = C.POINTER
    assert lib.t1render_mesh_scene.argtypes == [vp, P(_lib.RenderCamera), i32, vp, P(_lib.RenderStyle), i32, i32, i32,
                                                vp, vp, vp, vp, vp, vp, C.c_longlong, vp]
    assert lib.t1render_mesh_create.argtypes == [P(C.c_float), P(i32), P(C.c_uint32), i32, P(vp)]
    assert lib.t1render_mesh_workspace_bytes.restype == C.c_longlong and lib.t1render_mesh_scene.restype == C.c_int
    assert lib.t1render_mesh_info.argtypes == [vp, P(i32), P(i32), P(i32), P(C.c_float)]
    assert lib.t1render_mesh_destroy.argtypes == [vp]


def test_the_header_is_c(tmp_path):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc")
    assert cc, "no host C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "t1render.h"\nint use(t1render_mesh* m) { return t1render_mesh_destroy(m) + T1RENDER_MESH_BRUTE; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", "-o",
                    str(tmp_path / "use.o"), str(src)], check=True)


def test_workspace_query_is_the_scenes():
    lib = _lib_built()
    for bad in ((-1, 1), (5, 0), (5, 17)):
        assert lib.t1render_mesh_workspace_bytes(*bad) == -1
    for n in (0, 1, 64, 65, 1000, 4096, (1 << 31) - 1):
        for c in (1, 2, 16):
            assert lib.t1render_mesh_workspace_bytes(n, c) == lib.t1render_scene_workspace_bytes(n, c)


def _create(lib, tri, body, rgb, ntri=None, out=True):
    tri = np.ascontiguousarray(tri, np.float32)
    body, rgb = np.ascontiguousarray(body, np.int32), np.ascontiguousarray(rgb, np.uint32)
    h = _lib.C.c_void_p()
    f = lambda a, t: a.ctypes.data_as(_lib.C.POINTER(t)) if a is not None else None
    rc = lib.t1render_mesh_create(f(tri, _lib.C.c_float), f(body, _lib.C.c_int32), f(rgb, _lib.C.c_uint32),
                                  len(tri) if ntri is None else ntri, _lib.C.byref(h) if out else None)
    return rc, h


def test_create_refuses_before_any_device_work():
    lib = _lib_built()
    tri = SM.box_tris((-1, -1, -1), (1, 1, 1))
    body, rgb = np.zeros(12, np.int32), np.zeros(12, np.uint32)
    bad = {}
    for v in (np.nan, np.inf):
        t = tri.copy()
        t[7, 1, 2] = v
        bad["vertex %r" % v] = (t, body, rgb, None, True)
    for b in (13, -1):
        bb = body.copy()
        bb[11] = b
        bad["body %d" % b] = (tri, bb, rgb, None, True)
    bad["ntri -1"] = (tri, body, rgb, -1, True)
    bad["ntri 2^20 + 1"] = (tri, body, rgb, (1 << 20) + 1, True)
    bad["null out"] = (tri, body, rgb, None, False)
    for name, a in bad.items():
        rc, h = _create(lib, *a)
        assert rc == -1 and not h.value, name
        assert b"t1render_mesh_create" in lib.t1env_last_error(), name
    h = _lib.C.c_void_p()
    f32p, i32p, u32p = (_lib.C.POINTER(t) for t in (_lib.C.c_float, _lib.C.c_int32, _lib.C.c_uint32))
    for k in range(3):
        args = [tri.ctypes.data_as(f32p), body.ctypes.data_as(i32p), rgb.ctypes.data_as(u32p)]
        args[k] = None
        assert lib.t1render_mesh_create(*args, 12, _lib.C.byref(h)) == -1 and not h.value
    # the other entry points: a null or unknown handle
    assert lib.t1render_mesh_destroy(None) == 0
    assert lib.t1render_mesh_info(None, None, None, None, None) == -1
    junk = (_lib.C.c_char * 256)()
    assert lib.t1render_mesh_info(_lib.C.addressof(junk), None, None, None, None) == -1
    assert lib.t1render_mesh_destroy(_lib.C.addressof(junk)) == -1
    assert lib.t1render_mesh_scene(None, None, 1, None, None, 0, 4, 4, None, None, None, None, None, None, 0, None) == -1
    assert b"t1render_mesh_scene" in lib.t1env_last_error()


def test_play_parses_render_urdf(tmp_path):
    from ti5_isaacgym_amd.scripts import play
    assert play.parse(["--checkpoint", "none.pt"]).render_urdf is None
    urdf = SM.synth_robot(str(tmp_path / "robot"))
    a = play.parse(["--checkpoint", "none.pt", "--render", "d", "--render_urdf", urdf, "--render_scene", "all",
                    "--render_terrain_shadow"])
    assert a.render_urdf == urdf and a.render_scene == "all" and a.render_terrain_shadow
    with pytest.raises(ValueError, match="--render"):
        play.parse(["--checkpoint", "none.pt", "--render_urdf", urdf])
    with pytest.raises(FileNotFoundError, match="nowhere.urdf"):
        play.parse(["--checkpoint", "none.pt", "--render", "d", "--render_urdf", str(tmp_path / "nowhere.urdf")])


def test_renderer_and_robot_mesh_surface():
    import inspect
    from ti5_isaacgym_amd.utils import render as R
    p = inspect.signature(R.Renderer.__init__).parameters
    assert p["mesh"].default is None and list(p)[-1] == "mesh"
    assert list(inspect.signature(R.RobotMesh.__init__).parameters) == ["self", "tri", "body", "rgb"]
    q = inspect.signature(R.RobotMesh.from_urdf).parameters
    assert list(q) == ["path", "missing_ok"] and q["missing_ok"].default is False
    for name in ("close", "__del__", "info"):
        assert callable(getattr(R.RobotMesh, name))
    with pytest.raises(ValueError):
        R.RobotMesh(np.zeros((3, 3)), np.zeros(1), np.zeros(1))


def test_scene_1_shows_what_it_is_for():
    s, ref = SM.scene1(), SM.reference1()
    m = s["mesh"]
    assert [int((m["body"] == b).sum()) for b in (0, 1, 2, 3, 4, 5, 6, 7)] == [80, 1, 4, 5, 9, 0, 2, 1]
    assert 1900 < (m["body"] == 12).sum() < 2100
    assert ref["ambiguous"].mean() <= SM.AMBIGUOUS_CAP
    seen = set(ref["ids"][~ref["ambiguous"]].tolist())
    assert seen == {-1, 0, 1, 2, 3, 4, 5, 7, 13}            # sky, terrain, every body that has area; not body 5, not 7
    assert not (ref["tris"] == s["zero"]).any()              # the zero-area triangle in front of everything
    quad = np.isin(ref["tris"], s["quad"])
    assert quad.sum() > 30
    # the quad is seen from behind: its winding's normal points away from the eye, the shading normal towards it
    v = m["tri"][s["quad"][0]].astype(np.float64)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    eye = np.array(s["cam"]["eye"]) - s["rigid"][0, 6, 0:3]
    assert n @ eye < 0 and (ref["nl"][quad] > 0).all()
    assert (~ref["lit"] & ~ref["ambiguous"]).sum() > 10      # and something casts a shadow
    assert len(set(ref["tris"][ref["ids"] == 13].tolist())) > 20


def test_the_crowd_pins_the_mesh_radii_in_the_culling_bound():
    """By construction: in the fp64 reference ARM shows in the picture by its arm box alone, and t1render_scene's own
    bound of it (the sphere around its primitives, swept along the shadow segment) lies wholly outside every tile it
    shows in, so a cull that took a robot's extent from the primitives would drop it there."""
    from ti5_isaacgym_amd.utils import render as R
    w, h = SM.CROWD_SIZE
    ref = RM.render(dict(rigid=SM.crowd_poses(), terrain=None), SM.crowd_camera(), w, h, SM.crowd_mesh(), SM.style(),
                    np.float64, True, False)
    arm = np.argwhere(ref["envs"] == SM.ARM)
    assert len(arm) >= 4 and not (ref["envs"] == SM.CASTER).any()
    assert ((ref["tris"][ref["envs"] == SM.ARM] >= SM.ARM_BOX[0]) & (ref["tris"][ref["envs"] == SM.ARM] < SM.ARM_BOX[1])).all()
    tiles = {(int(j) // 16, int(i) // 16) for i, j in arm}
    assert SM.primitives_cull_arm(tiles)
    assert SM.primitives_cull_arm([(tx, ty) for tx in range(3) for ty in range(2)])   # and from every other tile
    # the recomputation is no rubber stamp: a robot in the picture is kept by its own tile
    c, r = SM.primitive_sphere(R.robot_primitives(), SM.crowd_poses()[0])
    o, d = RM.RR.camera_rays(SM.crowd_camera(), SM.crowd_poses()[0, 0, 0:3], w, h, np.float64)
    px = int(np.argmax(d @ ((c - o) / np.linalg.norm(c - o))))   # the pixel that looks at its centre
    assert not SM.capsule_outside(*SM.tile_planes(SM.crowd_camera(), w, h, (px % w) // 16, (px // w) // 16), c, c, r)
    assert np.linalg.norm(c - SM.crowd_poses()[0, 0, 0:3]) < 1.0 and 0.3 < r < 1.5


def test_reference_agrees_with_a_direct_moeller_trumbore():
    """The reference's three-matrix-product form against the textbook loop, on random rays and triangles."""
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (40, 3, 3))
    W = (v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    o = np.array([0.1, -0.2, 3.0])
    d = RM.RR._unit(rng.uniform(-0.4, 0.4, (200, 3)) - np.array([0, 0, 1.0]))
    t, k = RM.cast_from_point(W, o, d, 0.05, np.float64)
    for r in range(len(d)):
        th = RM.RR._tri_hits(o, d[r:r + 1], *[x for x in (v[:, 0], v[:, 1], v[:, 2])], np.float64)[0]
        th = np.where((th > 0.05) & (th <= 200.0), th, np.inf)
        assert (np.isinf(t[r]) and np.isinf(th.min())) or (k[r] == th.argmin() and abs(t[r] - th.min()) < 1e-12)
    assert np.isfinite(t).sum() > 50
    L = RM.RR._unit(np.array([0.2, 0.1, 1.0]))
    so = rng.uniform(-1, 1, (150, 3)) - np.array([0, 0, 2.0])
    t2, k2 = RM.cast_along(W, so, L, 0.0, np.float64)
    for r in range(len(so)):
        th = RM.RR._tri_hits(so[r], L[None, :], v[:, 0], v[:, 1], v[:, 2], np.float64)[0]
        th = np.where((th > 0) & (th <= 200.0), th, np.inf)
        assert (np.isinf(t2[r]) and np.isinf(th.min())) or (k2[r] == th.argmin() and abs(t2[r] - th.min()) < 1e-12)
    assert np.isfinite(t2).sum() > 30
