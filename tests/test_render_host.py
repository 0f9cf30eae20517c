"""The headless camera's parts that need no GPU: the primitive table of the committed model, write_png, the numpy
reference (tests/render_ref.py) against closed forms, the ambiguity cap on every scene tests/test_gpu_render.py compares
on the trimesh (tests/render_scenes.py), the C ABI's declaration, and play's frame-buffer refusal."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import render_ref  # noqa: E402
import render_scenes  # noqa: E402

AMBIGUOUS_CAP = 0.01   # at most 1% of a scene's pixels may be ambiguous: a condition on the scenes, not a measurement


def _R():
    from ti5_isaacgym_amd.utils import render
    return render


def test_primitive_table_of_the_committed_model():
    from ti5_isaacgym_amd.utils.urdf import SELF_BODIES, load_model
    R, tab = _R(), load_model()
    prims = R.robot_primitives(tab)
    assert len(prims) == 15 <= 32
    boxes = [p for p in prims if p["kind"] == R.BOX]
    caps = [p for p in prims if p["kind"] == R.CAPSULE]
    assert [p["body"] for p in boxes] == [0] + SELF_BODIES
    pts = np.array([p for p, b in zip(tab["contact_point"], tab["contact_body"]) if b == 0])
    np.testing.assert_allclose(np.array(boxes[0]["a"]) - boxes[0]["b"], pts.min(0), atol=1e-12)
    np.testing.assert_allclose(np.array(boxes[0]["a"]) + boxes[0]["b"], pts.max(0), atol=1e-12)
    for p, box in zip(boxes[1:], tab["self_box"]):
        assert list(p["a"]) + list(p["b"]) == list(box)
    assert len(caps) == 10
    ends = {(p["body"], tuple(p["b"])) for p in caps}
    for c, b in enumerate(tab["parent"]):
        if b >= 1:
            assert (b, tuple(tab["joint_offset"][c])) in ends
    assert all(p["a"] == (0.0, 0.0, 0.0) and p["r"] == R.LIMB_RADIUS == 0.04 for p in caps)
    groups = {p["rgb"] for p in prims}
    assert groups == {R.COLOR_BASE, R.COLOR_LEFT, R.COLOR_RIGHT, R.COLOR_FEET} and len(groups) == 4
    assert {p["rgb"] for p in prims if p["body"] in (6, 12)} == {R.COLOR_FEET}
    assert abs(np.linalg.norm(R.STYLE["light"]) - 1.0) < 1e-12


@pytest.mark.parametrize("shape", [(1, 1), (3, 17), (36, 64)])
@pytest.mark.parametrize("channels", [3, 4])
def test_write_png_round_trips_through_pillow(tmp_path, shape, channels):
    from PIL import Image
    a = np.random.default_rng(shape[1] * 10 + channels).integers(0, 256, shape + (channels,), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    _R().write_png(path, a)
    with Image.open(path) as im:
        assert im.size == (shape[1], shape[0]) and im.mode == ("RGB" if channels == 3 else "RGBA")
        np.testing.assert_array_equal(np.asarray(im), a)
    with pytest.raises(ValueError):
        _R().write_png(path, a.astype(np.float32))


IDENT = np.zeros((13, 13), np.float32)
IDENT[:, 6] = 1.0
STYLE = dict(light=(0.0, 0.6, 0.8), ambient=0.25, terrain_rgb=((1.0, 0.5, 0.25), (0.2, 0.4, 0.6)),
             sky_rgb=((0.1, 0.2, 0.3), (0.5, 0.7, 0.9)))


def _rays(cam, W, H):
    o, d = render_ref.camera_rays(cam, np.zeros(3), W, H, np.float64)
    return o, d.reshape(H, W, 3)


def test_reference_sphere_closed_form():
    rigid = IDENT.copy()
    rigid[3, 0:3] = (0.5, -0.25, 1.0)
    r = np.float64(np.float32(0.3))
    prims = [dict(body=3, kind=1, a=(0, 0, 0), b=(0, 0, 0), r=0.3, rgb=0x0000FF)]
    cam = dict(env=0, follow=False, eye=(5.5, -0.25, 1.0), target=(0.5, -0.25, 1.0), up=(0, 0, 1), vfov=0.2)
    out = render_ref.render(dict(rigid=rigid, terrain=None), cam, 5, 5, prims, STYLE)
    o, d = _rays(cam, 5, 5)
    c = np.array([0.5, -0.25, 1.0])
    perp = np.linalg.norm(np.cross(c - o, d), axis=-1)   # the centre's distance from each ray
    along = (d * (c - o)).sum(-1)
    hit = perp < r
    assert hit[2, 2] and not hit[0, 0]
    np.testing.assert_array_equal(out["ids"] == 4, hit)
    np.testing.assert_allclose(out["depth"][hit], (along - np.sqrt(r * r - perp ** 2, where=hit, out=perp * 0))[hit],
                               rtol=0, atol=1e-12)
    assert abs(out["depth"][2, 2] - (5.0 - r)) < 1e-12
    # the centre pixel's normal is +x: n.L = 0, so only the ambient term of a red sphere is left
    np.testing.assert_array_equal(out["rgb"][2, 2], [int(np.floor(np.float32(0.25) * 255 + 0.5)), 0, 0])
    assert out["lit"].all()


def test_reference_capsule_side_on_closed_form():
    prims = [dict(body=0, kind=1, a=(0, -1, 0), b=(0, 1, 0), r=0.2, rgb=0x00FF00)]
    rigid = IDENT.copy()
    rigid[0, 0:3] = (0, 0, 1)
    cam = dict(env=0, follow=False, eye=(4, 0, 1), target=(0, 0, 1), up=(0, 0, 1), vfov=0.2)
    W, H = 9, 5
    out = render_ref.render(dict(rigid=rigid, terrain=None), cam, W, H, prims, STYLE)
    o, d = _rays(cam, W, H)
    r = np.float64(np.float32(0.2))
    # the cylinder about the line x = 0, z = 1: in the x-z plane a circle of radius r around the origin
    A = d[..., 0] ** 2 + d[..., 2] ** 2
    B = 4.0 * d[..., 0]
    disc = B * B - A * (16.0 - r * r)
    with np.errstate(invalid="ignore"):
        t = (-B - np.sqrt(disc)) / A
    y = t * d[..., 1]
    side = (disc >= 0) & (np.abs(y) < 1.0)   # these pixels see the cylinder's side (the image stays inside |y| < 1)
    assert side.sum() >= 9 and (np.abs(4.0 * d[..., 1] / -d[..., 0]) < 0.9).all()
    np.testing.assert_array_equal(out["ids"] == 1, side)
    np.testing.assert_allclose(out["depth"][side], t[side], rtol=0, atol=1e-12)
    assert abs(out["depth"][2, 4] - (4.0 - r)) < 1e-12
    n = (o + t[..., None] * d) * [1, 0, 1] - [0, 0, 1]
    nl = np.maximum((n / r) @ np.float64(np.float32(STYLE["light"])), 0)
    np.testing.assert_allclose(out["nl"][side], nl[side], atol=1e-7)   # the light is a unit vector only to fp32


def test_reference_plane_closed_form():
    cam = dict(env=0, follow=False, eye=(0.3, 0.2, 2.0), target=(3.3, 0.2, 0.0), up=(0, 0, 1), vfov=0.8)
    W, H = 7, 5
    rigid = IDENT.copy()
    rigid[:, 0:3] = (100.0, 100.0, 50.0)   # the robot far out of view
    out = render_ref.render(dict(rigid=rigid, terrain=None), cam, W, H, _R().robot_primitives(), STYLE)
    o, d = _rays(cam, W, H)
    t = -o[2] / d[..., 2]
    assert (d[..., 2] < 0).all() and (out["ids"] == 0).all() and out["lit"].all()
    np.testing.assert_allclose(out["depth"], t, rtol=0, atol=1e-12)
    p = o + t[..., None] * d
    par = (np.floor(p[..., 0]).astype(int) + np.floor(p[..., 1]).astype(int)) & 1
    assert par.min() == 0 and par.max() == 1
    base = np.float64(np.float32(STYLE["terrain_rgb"]))[par]
    amb = np.float64(np.float32(0.25))
    val = (amb + (1 - amb) * np.float64(np.float32(0.8))) * base
    np.testing.assert_array_equal(out["rgb"], np.floor(val * 255 + 0.5).astype(np.uint8))
    # looking up: the sky's gradient on the ray's z
    up = dict(cam, target=(3.3, 0.2, 4.0))
    sky = render_ref.render(dict(rigid=rigid, terrain=None), up, 3, 3, [], STYLE)
    _, du = _rays(up, 3, 3)
    s0, s1 = np.float64(np.float32(STYLE["sky_rgb"]))
    assert (sky["ids"] == -1).all() and np.isinf(sky["depth"]).all()
    np.testing.assert_array_equal(sky["rgb"], np.floor((s0 + (0.5 * (du[..., 2:3] + 1)) * (s1 - s0)) * 255 + 0.5)
                                  .astype(np.uint8))


def test_reference_tilted_triangle_closed_form():
    # one cell: z = u - v on the triangle u >= v ((0,0)-(1,0)-(1,1)), z = 0 on the other
    T = dict(h=np.array([[0, 0], [200, 0]], np.int16), hscale=1.0, vscale=0.005, border=0.0)
    scene = dict(rigid=IDENT.copy(), terrain=T)
    scene["rigid"][:, 0:3] = (100.0, 100.0, 50.0)
    for (x, y), depth, tri, n in (((0.7, 0.2), 2.5, 0, np.array([-1.0, 1.0, 1.0]) / np.sqrt(3.0)),
                                  ((0.2, 0.7), 3.0, 1, np.array([0.0, 0.0, 1.0]))):
        cam = dict(env=0, follow=False, eye=(x, y, 3.0), target=(x, y, 0.0), up=(1, 0, 0), vfov=0.1)
        out = render_ref.render(scene, cam, 1, 1, [], STYLE)
        assert out["ids"][0, 0] == 0 and out["tri"][0, 0] == tri
        assert abs(out["depth"][0, 0] - depth) < 1e-6   # eye and target are fp32 values
        assert abs(out["nl"][0, 0] - max(n @ np.float64(np.float32(STYLE["light"])), 0)) < 1e-7
    # beside the footprint there is no terrain: the sky, also when looking down
    cam = dict(env=0, follow=False, eye=(1.5, 0.5, 3.0), target=(1.5, 0.5, 0.0), up=(1, 0, 0), vfov=0.1)
    assert render_ref.render(scene, cam, 1, 1, [], STYLE)["ids"][0, 0] == -1


@pytest.mark.parametrize("name", [c[0] for c in render_scenes.trimesh_cases()])
def test_ambiguity_cap_holds_on_every_trimesh_scene(name):
    ref = render_scenes.reference_of(name)
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP, (name, ref["ambiguous"].mean())
    if name in ("B0", "B1", "B2", "Bdown"):   # the comparison has terrain, robot and shadow pixels to compare
        ok = ~ref["ambiguous"]
        assert (ref["ids"][ok] == 0).sum() > 100 and (ref["ids"][ok] > 0).sum() > 50 and (~ref["lit"][ok]).sum() > 10
    if name == "C":   # the footprint's edge: sky above the terrain's last cells
        assert (ref["ids"] == -1).sum() > 100 and (ref["ids"] == 0).sum() > 100


def test_scenes_cover_the_field_and_the_straight_down_ray():
    T, rs = render_scenes.trimesh_terrain(), render_scenes.trimesh_poses()
    assert T["h"].shape == (580, 420) and np.unique(T["h"]).size > 50
    assert rs.shape == (5, 13, 13) and np.allclose(np.linalg.norm(rs[:, :, 3:7], axis=-1), 1.0, atol=1e-6)
    cam = render_scenes.down_camera()
    _, d = _rays(cam, 33, 33)
    assert d[16, 16, 0] == 0.0 and d[16, 16, 1] == 0.0 and d[16, 16, 2] == -1.0
    assert {c["env"] for c in render_scenes.trimesh_cameras()} == {0, 1, 4}


def test_c_abi_is_declared_and_exported():
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd import build as b
    src = " ".join(open(os.path.join(REPO, "include", "t1render.h")).read().split())
    assert ("int t1render_frame(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_prim* prims, "
            "int32_t nprims, const t1render_style* style, int32_t width, int32_t height, uint32_t* rgba, float* depth, "
            "int32_t* ids, void* stream);") in src
    assert "#define T1RENDER_MAXCAM 16" in src and "#define T1RENDER_MAXPRIM 32" in src
    assert ("t1render.hip", "-O3") in b.UNITS
    assert _lib.RENDER_EXPORTS == ["t1render_frame"] and "t1render_frame" not in _lib.EXPORTS
    assert (_lib.C.sizeof(_lib.RenderCamera), _lib.C.sizeof(_lib.RenderPrim), _lib.C.sizeof(_lib.RenderStyle)) == \
        (48, 40, 64)
    b.build()
    lib = _lib.load()
    assert len(lib.t1render_frame.argtypes) == 12
    # argument errors are reported before any device work
    assert lib.t1render_frame(None, None, 1, None, 0, None, 4, 4, None, None, None, None) == -1
    assert b"t1render_frame" in lib.t1env_last_error()


def test_play_refuses_a_frame_buffer_over_8_gib():
    from ti5_isaacgym_amd.scripts import play
    with pytest.raises(ValueError, match=r"50000 frames of 1920 x 1080") as e:
        play.parse(["--checkpoint", "none.pt", "--render", "frames", "--steps", "100000", "--render_size", "1920", "1080"])
    assert "8 GiB" in str(e.value)
    a = play.parse(["--checkpoint", "none.pt", "--render", "frames", "--steps", "200"])
    assert (a.render_every, a.render_size, a.render_follow) == (2, [640, 360], [3.0, 0.0, 1.0])
    assert play.num_frames(200, 2) == 100 and play.num_frames(6, 2) == 3 and play.num_frames(7, 3) == 2
    assert play.parse(["--checkpoint", "none.pt", "--steps", "100000000"]).render is None   # no --render: no check
