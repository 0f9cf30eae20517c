"""t1render_scene's parts that need no GPU: the conditions the scenes of tests/render_scenes_multi.py must meet for
tests/test_gpu_render_scene.py to compare anything (asserted on the fp64 reference alone: if one fails, change the
scene, not the bound), tests/render_ref_scene.py against closed forms, the C ABI's declaration, export list and ctypes
signatures, the workspace query, and play's two switches."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import render_ref_scene as RS  # noqa: E402
import render_scenes_multi as M  # noqa: E402
from ti5_isaacgym_amd import _lib  # noqa: E402

OTHERS, SHADOW, BRUTE = _lib.RENDER_SCENE_OTHERS, _lib.RENDER_SCENE_TERRAIN_SHADOW, _lib.RENDER_SCENE_BRUTE
AMBIGUOUS_CAP = 0.01


# ---- scene conditions
@pytest.mark.parametrize("cam", [0, 1], ids=["A", "B"])
def test_trimesh_scene_has_neighbours_and_both_kinds_of_shadow(cam):
    ref = M.reference_of(cam, "both")
    ok = ~ref["ambiguous"]
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP, ref["ambiguous"].mean()
    own = M.cameras()[cam]["env"]
    other = ok & (ref["envs"] >= 0) & (ref["envs"] != own)
    assert other.sum() >= 100 and len(set(ref["envs"][ok & (ref["envs"] >= 0)].tolist())) >= 5
    hit = ok & (ref["ids"] >= 0)
    assert (hit & ref["by_terrain"] & ~ref["by_robot"]).sum() >= 200
    assert (hit & ref["by_robot"] & ~ref["by_terrain"]).sum() >= 50
    assert (hit & ref["by_robot"] & ~ref["by_own"]).sum() >= 100
    assert np.isfinite(ref["depth"]).any() and ref["depth"][np.isfinite(ref["depth"])].max() > 8.0


def test_scene_poses_stand_where_the_recipe_puts_them():
    rs = M.poses()
    assert rs.shape == (8, 13, 13) and np.allclose(np.linalg.norm(rs[:, :, 3:7], axis=-1), 1.0, atol=1e-6)
    np.testing.assert_allclose(rs[:, 0, 0:2], M.BASES, atol=1e-5)
    assert np.abs(rs[:, 1:, 0:2] - rs[:, :1, 0:2]).max() <= 0.5 + 1e-5
    cams = M.cameras()
    assert [c["env"] for c in cams] == [0, 3] and all(c["vfov"] == 0.8 and not c["follow"] for c in cams)


def _crowd_scene(drop=None):
    rows = [n for n in M.crowd_subset() if n != drop]
    return dict(rigid=M.crowd_poses()[rows], terrain=None), rows


def test_crowd_subset_shows_the_tie_and_the_unseen_caster():
    """What the culling test compares with the reference on nine envs: the twins' pixels (the lower env's), and a robot
    that camera 0 does not see but whose shadow it does."""
    from ti5_isaacgym_amd.utils import render as R
    scene, rows = _crowd_scene()
    lo, hi, caster = rows.index(M.TWIN_LO), rows.index(M.TWIN_HI), rows.index(M.CASTER)
    assert lo < hi and np.array_equal(scene["rigid"][lo], scene["rigid"][hi])
    w, h = M.CROWD_SIZE
    cam = dict(M.crowd_cameras()[0], env=0)
    ref = RS.reference(scene, cam, w, h, R.robot_primitives(), R.STYLE, True, False)
    ok = ~ref["ambiguous"]
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP
    assert (ok & (ref["envs"] == lo)).sum() >= 20 and not (ref["envs"] == hi).any()
    assert not (ref["envs"] == caster).any()
    without, _ = _crowd_scene(drop=M.CASTER)
    bare = RS.render(without, cam, w, h, R.robot_primitives(), R.STYLE, np.float64, True, False)
    # shadowed only because the caster is in the scene; each such pixel is an exact lit decision, ten tell its presence
    assert (ok & ~ref["lit"] & bare["lit"]).sum() >= 10


def test_crowd_has_what_the_culling_test_names():
    rs, cams = M.crowd_poses(), M.crowd_cameras()
    assert rs.shape == (1000, 13, 13)
    d = np.linalg.norm(rs[:300, 0, 0:2] - M.CROWD_CENTRE, axis=1)
    assert d.max() <= 3.0 and 300 > 8   # more than one LDS batch of 8 envs
    eye = np.array(cams[0]["eye"])
    assert abs(np.linalg.norm(eye - [*M.CROWD_CENTRE, 0.6]) - 8.0) < 0.2
    assert np.array_equal(rs[M.AT_EYE, 0, 0:3], np.float32(eye))
    assert np.abs(rs[M.FAR, 0, 0:2]).min() >= 9.9e3
    view = np.array(cams[0]["target"]) - eye
    assert (rs[M.BEHIND, 0, 0:3] - eye) @ view < 0
    assert cams[1]["up"] == (1.0, 0.0, 0.0) and cams[1]["eye"][2] == 30.0


# ---- closed forms for the helper
IDENT = np.zeros((13, 13), np.float32)
IDENT[:, 6] = 1.0
STYLE = dict(light=(0.0, 0.6, 0.8), ambient=0.25, terrain_rgb=((1.0, 0.5, 0.25), (0.2, 0.4, 0.6)),
             sky_rgb=((0.1, 0.2, 0.3), (0.5, 0.7, 0.9)))
SPHERE = [dict(body=0, kind=1, a=(0, 0, 0), b=(0, 0, 0), r=0.3, rgb=0x0000FF)]


def _spheres(xs):
    rigid = np.stack([IDENT.copy() for _ in xs])
    for n, x in enumerate(xs):
        rigid[n, :, 0:3] = (x, 0.0, 5.0)
    return dict(rigid=rigid, terrain=None)


def test_reference_nearer_of_two_envs_on_one_ray():
    cam = dict(env=0, follow=False, eye=(6.0, 0.0, 5.0), target=(0.0, 0.0, 5.0), up=(0, 0, 1), vfov=0.05)
    out = RS.render(_spheres([0.0, 2.0]), cam, 3, 3, SPHERE, STYLE)
    r = np.float64(np.float32(0.3))
    assert out["envs"][1, 1] == 1 and out["ids"][1, 1] == 1 and abs(out["depth"][1, 1] - (4.0 - r)) < 1e-12
    # the camera's own robot only: the farther sphere
    own = RS.render(_spheres([0.0, 2.0]), cam, 3, 3, SPHERE, STYLE, others=False)
    assert own["envs"][1, 1] == 0 and abs(own["depth"][1, 1] - (6.0 - r)) < 1e-12
    # sky and terrain carry no env
    up = dict(cam, target=(6.0, 0.0, 9.0), up=(1, 0, 0))
    assert (RS.render(_spheres([0.0, 2.0]), up, 3, 3, SPHERE, STYLE)["envs"] == -1).all()


def test_reference_identical_spheres_show_the_lower_env():
    xs = [100.0, 200.0, 0.0, 300.0, 400.0, 0.0]   # envs 2 and 5 coincide
    cam = dict(env=0, follow=False, eye=(6.0, 0.0, 5.0), target=(0.0, 0.0, 5.0), up=(0, 0, 1), vfov=0.05)
    out = RS.render(_spheres(xs), cam, 3, 3, SPHERE, STYLE)
    assert (out["ids"] == 1).all() and (out["envs"] == 2).all()


def test_reference_wall_shadow_reaches_h_over_tan_e():
    """A one-cell-wide wall of height H (rows 8 and 9 of a 1 m grid raised to 1 m; its faces slope over one cell) under
    a light of elevation e = 30 degrees from +x: a ground point is shadowed out to (H - z0) / tan e behind the wall's
    top edge x = 8, z0 = 1e-3 being the shadow ray's start above the ground.  (A start within 0.05 m of the face's foot
    is shadowed as well: its ray enters the wall unseen and meets the top from below, and the field is two-sided.)"""
    h = np.zeros((13, 4), np.int16)
    h[8:10, :] = 200
    T = dict(h=h, hscale=1.0, vscale=0.005, border=0.0)
    e = np.deg2rad(30.0)
    L = np.array([np.cos(e), 0.0, np.sin(e)])
    tip = 8.0 - (1.0 - 1e-3) / np.tan(e)
    xs = np.array([tip - 1e-6, tip + 1e-6, 0.5 * (tip + 7.0), 6.99, 3.0])
    so = np.stack([xs, np.full_like(xs, 1.5), np.full_like(xs, 1e-3)], 1)
    got = RS.terrain_shadow(T, so, L, np.ones(len(xs), bool), np.float64)
    assert got.tolist() == [False, True, True, True, False]
    assert not RS.terrain_shadow(T, so, L, np.zeros(len(xs), bool), np.float64).any()
    # and through render(): a camera straight above the tip sees the shadow's edge between its two middle columns
    rigid = IDENT.copy()[None]
    rigid[:, :, 0:3] = (100.0, 100.0, 50.0)
    tipg = 8.0 - 1.0 / np.tan(e)   # the rendered ground's own start is z0 = 1e-3 n above z = 0
    cam = dict(env=0, follow=False, eye=(tipg, 1.5, 4.0), target=(tipg, 1.5, 0.0), up=(0, 1, 0), vfov=0.1)
    style = dict(STYLE, light=tuple(L))
    out = RS.render(dict(rigid=rigid, terrain=T), cam, 4, 1, [], style)
    assert (out["ids"] == 0).all()
    # the view is -z and up is +y, so the columns run along +x: towards the wall
    assert out["lit"][0].tolist() == [True, True, False, False] and out["by_terrain"][0].tolist() == [False, False, True, True]
    assert RS.render(dict(rigid=rigid, terrain=T), cam, 4, 1, [], style, shadow=False)["lit"].all()


# ---- host-side code
def test_c_abi_is_declared_exported_and_bound():
    from ti5_isaacgym_amd import build as b
    src = " ".join(open(os.path.join(REPO, "include", "t1render.h")).read().split())
    assert "long long t1render_scene_workspace_bytes(int32_t num_envs, int32_t ncams);" in src
    assert ("int t1render_scene(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_prim* prims, "
            "int32_t nprims, const t1render_style* style, int32_t flags, int32_t width, int32_t height, uint32_t* rgba, "
            "float* depth, int32_t* ids, int32_t* envs, void* workspace, long long workspace_bytes, void* stream);") in src
    for name, value in (("OTHERS", 1), ("TERRAIN_SHADOW", 2), ("BRUTE", 4)):
        assert "#define T1RENDER_SCENE_%s %d " % (name, value) in src
    assert (OTHERS, SHADOW, BRUTE) == (1, 2, 4)
    assert _lib.RENDER_SCENE_EXPORTS == ["t1render_scene_workspace_bytes", "t1render_scene"]
    assert _lib.RENDER_EXPORTS == ["t1render_frame"]
    assert not set(_lib.RENDER_SCENE_EXPORTS) & set(_lib.EXPORTS + _lib.POLICY_EXPORTS + _lib.RENDER_EXPORTS)
    assert ("t1render_scene.hip", "-O3") in b.UNITS and ("t1render.hip", "-O3") in b.UNITS
    b.build()
    lib = _lib.load()
    vp, i32 = _lib.C.c_void_p, _lib.C.c_int32
    P = _lib.C.POINTER
    assert lib.t1render_scene.argtypes == [vp, P(_lib.RenderCamera), i32, P(_lib.RenderPrim), i32, P(_lib.RenderStyle),
                                           i32, i32, i32, vp, vp, vp, vp, vp, _lib.C.c_longlong, vp]
    assert lib.t1render_scene.restype == _lib.C.c_int
    assert lib.t1render_scene_workspace_bytes.argtypes == [i32, i32]
    assert lib.t1render_scene_workspace_bytes.restype == _lib.C.c_longlong
    # argument errors are reported before any device work
    assert lib.t1render_scene(None, None, 1, None, 0, None, 0, 4, 4, None, None, None, None, None, 0, None) == -1
    assert b"t1render_scene" in lib.t1env_last_error()


def test_workspace_query():
    from ti5_isaacgym_amd import build as b
    b.build()
    q = _lib.load().t1render_scene_workspace_bytes
    for bad in ((-1, 1), (5, 0), (5, -1), (5, 17), (-1, 0)):
        assert q(*bad) == -1, bad
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4096, 32768, 1 << 20]
    for c in range(1, 17):
        row = [q(n, c) for n in sizes]
        assert all(a <= b_ for a, b_ in zip(row, row[1:])) and all(v >= 16 * n and v % 16 == 0 for v, n in zip(row, sizes))
        if c > 1:
            assert all(q(n, c) >= q(n, c - 1) for n in sizes)
    assert q((1 << 31) - 1, 16) > (1 << 35)   # no 32-bit arithmetic in the size


def test_play_parses_the_scene_switches():
    from ti5_isaacgym_amd.scripts import play
    a = play.parse(["--checkpoint", "none.pt"])
    assert a.render_scene == "own" and a.render_terrain_shadow is False
    a = play.parse(["--checkpoint", "none.pt", "--render", "d", "--render_scene", "all", "--render_terrain_shadow"])
    assert a.render_scene == "all" and a.render_terrain_shadow is True
    assert play.parse(["--checkpoint", "none.pt", "--render_scene", "own"]).render_scene == "own"
    with pytest.raises(SystemExit):
        play.parse(["--checkpoint", "none.pt", "--render_scene", "some"])


def test_renderer_takes_the_two_switches():
    import inspect
    from ti5_isaacgym_amd.utils import render as R
    p = inspect.signature(R.Renderer.__init__).parameters
    assert list(p)[:7] == ["self", "env", "width", "height", "cameras", "prims", "style"]
    assert p["others"].default is False and p["terrain_shadow"].default is False
