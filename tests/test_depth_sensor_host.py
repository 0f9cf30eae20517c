"""The depth camera sensor's parts that need no GPU: the numpy reference (tests/depth_ref.py) against closed forms, the
conditions on the scenes tests/test_gpu_depth_sensor.py compares (tests/depth_scenes.py: the ambiguity cap over each
launch, the pixel counts), the C ABI's declaration, and play's --depth arguments."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import depth_ref  # noqa: E402
import depth_scenes as S  # noqa: E402

AMBIGUOUS_CAP = 0.01   # at most 1% of a launch's pixels may be ambiguous: a condition on the scenes, not a measurement

IDENT = np.zeros((13, 13), np.float32)
IDENT[:, 6] = 1.0
FAR_AWAY = (100.0, 100.0, 50.0)


def _R():
    from ti5_isaacgym_amd.utils import render
    return render


def _sensor(**kw):
    return dict(dict(body=0, pos=(0.0, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0), vfov=0.4, near=0.1, far=3.0), **kw)


def _scene(base=(0.0, 0.0, 1.0), quat=(0.0, 0.0, 0.0, 1.0), terrain=None):
    rigid = IDENT.copy()
    rigid[1:, 0:3] = FAR_AWAY
    rigid[0, 0:3], rigid[0, 3:7] = base, quat
    return dict(rigid=rigid, terrain=terrain)


def test_reference_sphere_straight_ahead_at_a_known_planar_depth():
    """A sphere of radius 0.3 centred 2 m ahead of a camera that looks along +x: the centre pixel reads 1.7, and every
    pixel that sees it reads the x coordinate of its hit point, which is not the distance along its ray."""
    sc = _scene()
    sc["rigid"][3, 0:3] = (2.0, 0.0, 1.0)
    r = np.float64(np.float32(0.3))
    prims = [dict(body=3, kind=1, a=(0, 0, 0), b=(0, 0, 0), r=0.3, rgb=0)]
    W = H = 7
    out = depth_ref.render(sc, _sensor(far=2.5), W, H, prims)
    th = np.tan(np.float64(np.float32(0.4)) / 2)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    x, y = (2 * (jj + 0.5) / W - 1) * th * W / H, (1 - 2 * (ii + 0.5) / H) * th
    d = np.stack([np.ones_like(x), -x, y], -1)   # f = +x, r = -l = -y, u = +z
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    c = np.array([2.0, 0.0, 0.0])   # the sphere's centre seen from the eye
    b = d @ c
    disc = b * b - (c @ c - r * r)
    hit = disc >= 0
    assert hit[3, 3] and not hit[0, 0]
    np.testing.assert_array_equal(out["ids"] == 4, hit)
    t = b - np.sqrt(np.where(hit, disc, 0))
    np.testing.assert_allclose(out["depth"][hit], (t * d[..., 0])[hit], rtol=0, atol=1e-12)
    assert abs(out["depth"][3, 3] - (2.0 - r)) < 1e-12
    # where nothing is hit (the plane z = 0 lies beyond far = 2.5 along these rays) the value is exactly far
    assert (out["ids"][~hit] == -1).all() and (out["depth"][~hit] == np.float64(np.float32(2.5))).all()
    assert out["depth"][1, 3] > out["depth"][3, 3] and (t * d[..., 0])[1, 3] < t[1, 3]   # planar, not radial


def test_reference_plane_under_a_pitched_camera_is_planar_depth():
    """The camera 1 m above the plane, the base yawed and the mount pitched down by p: on the centre column a ray a
    further angle a below the axis meets the ground at t = 1 / sin(p + a) and reads z = t cos(a)."""
    from depth_scenes import rpy_quat
    p = 0.6
    W, H = 5, 9
    vf = 0.5
    out = depth_ref.render(_scene(quat=tuple(rpy_quat(0.0, 0.0, 1.1))),
                           _sensor(pos=(0.0, 0.0, 0.0), quat=tuple(rpy_quat(0.0, p, 0.0)), vfov=vf, far=10.0), W, H, [])
    th = np.tan(np.float64(np.float32(vf)) / 2)
    y = (1 - 2 * (np.arange(H) + 0.5) / H) * th
    a = -np.arctan(y)   # the angle below the axis of the centre column's rays
    np.testing.assert_allclose(out["depth"][:, 2], np.cos(a) / np.sin(p + a), rtol=0, atol=1e-6)   # the quats are float32
    assert (out["ids"] == 0).all()
    # z is constant along an image row on a plane only when the camera does not roll: the row's planar depth is one value
    np.testing.assert_allclose(out["depth"], np.broadcast_to(out["depth"][:, 2:3], (H, W)), rtol=0, atol=1e-6)


def test_reference_capsule_that_straddles_the_near_plane_is_not_seen():
    """A capsule along the view axis from 0.08 to 1 m ahead, radius 0.05: the rays enter it 0.03 m ahead, before
    near = 0.1, so they see the wall behind it; shortened to start at 0.3 m it is seen at 0.25."""
    sc = _scene()
    sc["rigid"][5, 0:3] = (2.0, 0.0, 1.0)
    wall = dict(body=5, kind=0, a=(0, 0, 0), b=(0.1, 2.0, 2.0), r=0.0, rgb=0)   # its face at x = 1.9
    cap = dict(body=0, kind=1, a=(0.08, 0, 0), b=(1.0, 0, 0), r=0.05, rgb=0)
    out = depth_ref.render(sc, _sensor(vfov=0.05), 3, 3, [cap, wall])
    assert (out["ids"] == 6).all() and np.allclose(out["depth"], 1.9, atol=1e-6)
    assert (out["side"] == depth_ref.BEFORE).all()
    out = depth_ref.render(sc, _sensor(vfov=0.05), 3, 3, [dict(cap, a=(0.3, 0, 0)), wall])
    assert out["ids"][1, 1] == 1 and abs(out["depth"][1, 1] - 0.25) < 1e-6
    # a primitive that contains the eye is not seen either
    out = depth_ref.render(sc, _sensor(vfov=0.05), 3, 3, [dict(body=0, kind=0, a=(0, 0, 0), b=(0.5, 0.5, 0.5), r=0.0, rgb=0), wall])
    assert (out["ids"] == 6).all()


def test_reference_hit_just_past_far_gives_far():
    sc = _scene()
    sc["rigid"][5, 0:3] = (2.0, 0.0, 1.0)
    wall = dict(body=5, kind=0, a=(0, 0, 0), b=(0.1, 2.0, 2.0), r=0.0, rgb=0)   # planar depth 1.9 on every ray
    far32 = np.float64(np.float32(1.8999))
    out = depth_ref.render(sc, _sensor(far=1.8999), 5, 5, [wall])
    assert (out["ids"] == -1).all() and (out["depth"] == far32).all() and (out["side"] == depth_ref.BEYOND).all()
    out = depth_ref.render(sc, _sensor(far=1.9001), 5, 5, [wall])
    assert (out["ids"] == 6).all() and np.allclose(out["depth"], 1.9, atol=1e-6) and (out["side"] == depth_ref.INSIDE).all()
    # the height field: a flat one-cell field 1 m below the eye, seen straight down from body axes turned by the mount
    T = dict(h=np.zeros((2, 2), np.int16), hscale=1.0, vscale=0.005, border=0.0)
    from depth_scenes import rpy_quat
    down = tuple(rpy_quat(0.0, np.pi / 2, 0.0))
    sc = _scene(base=(0.5, 0.5, 1.0), terrain=T)
    assert depth_ref.render(sc, _sensor(quat=down, vfov=0.05, far=0.9999), 1, 1, [])["depth"][0, 0] == np.float64(np.float32(0.9999))
    out = depth_ref.render(sc, _sensor(quat=down, vfov=0.05, far=1.0001), 1, 1, [])
    assert out["ids"][0, 0] == 0 and abs(out["depth"][0, 0] - 1.0) < 1e-6
    # beside the footprint there is no terrain
    sc = _scene(base=(1.5, 0.5, 1.0), terrain=T)
    assert depth_ref.render(sc, _sensor(quat=down, vfov=0.05), 1, 1, [])["ids"][0, 0] == -1
    # a surface in front of near is not seen, and nothing else is there
    sc = _scene(base=(0.5, 0.5, 0.08), terrain=T)
    out = depth_ref.render(sc, _sensor(quat=down, vfov=0.05), 1, 1, [])
    assert out["ids"][0, 0] == -1 and out["depth"][0, 0] == 3.0 and out["side"][0, 0] == depth_ref.BEFORE


def test_float32_reference_stays_close_to_float64():
    ref = S.reference_of(1)
    f32 = depth_ref.render(S.scene(1), S.sensor(), S.WIDTH, S.HEIGHT, _R().robot_primitives(), np.float32)
    m = ~ref["ambiguous"] & (ref["ids"] >= 0) & (f32["ids"] == ref["ids"])
    assert m.sum() > 200 and np.abs(f32["depth"][m] - ref["depth"][m]).max() < 1e-3
    assert f32["depth"].dtype == np.float32


def test_conditions_on_the_trimesh_launch():
    """What the five-env launch of the GPU test compares: at most 1% ambiguous pixels over the launch, and among the
    others more than 100 terrain, 30 own-robot and 30 far pixels; env 2 looks out over the field's edge, env 4 stands on
    the stairs."""
    refs = [S.reference_of(n) for n in range(S.NUM_ENVS)]
    amb = np.stack([r["ambiguous"] for r in refs])
    ids = np.stack([r["ids"] for r in refs])
    assert amb.shape == (5, 13, 21) and amb.mean() <= AMBIGUOUS_CAP, amb.mean()
    ok = ~amb
    assert (ids[ok] == 0).sum() > 100 and (ids[ok] > 0).sum() > 30 and (ids[ok] < 0).sum() > 30
    # env 2: the rays that reach the ground's level beyond x = -5 find no terrain
    T, rs = S.trimesh_terrain(), S.trimesh_poses()
    assert rs[2, 0, 0] - (-T["border"]) < 1.5 and (refs[2]["side"] == depth_ref.NONE).sum() > 30
    assert (refs[2]["ids"] == 0).sum() > 30
    # env 4: the terrain around it has steps (flat treads at several levels)
    i, j = (int((S.BASES[4][k] + T["border"]) / T["hscale"]) for k in range(2))
    patch = T["h"][i - 15:i + 15, j - 15:j + 15]
    levels = np.unique(patch)
    assert 3 <= levels.size <= 12 and (np.diff(levels) >= 8).all()
    # the poses: yaw anywhere, roll and pitch within 0.5 rad, the base 0.6 to 1.2 m above the local ground
    for n in range(S.NUM_ENVS):
        x, y, z, w = rs[n, 0, 3:7].astype(np.float64)
        roll = np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
        pitch = np.arcsin(2 * (w * y - z * x))
        assert abs(roll) <= 0.5 and abs(pitch) <= 0.5
        assert 0.6 <= rs[n, 0, 2] - S._ground(T, *S.BASES[n]) <= 1.2
    assert np.allclose(np.linalg.norm(rs[:, :, 3:7], axis=-1), 1.0, atol=1e-6)
    assert (S.WIDTH % 16, S.HEIGHT % 4, S.SENSOR["far"]) == (5, 1, 3.0)
    assert S.SENSOR["pos"][0] > 0 and S.MOUNT_RPY[1] > 0   # forward of the base's origin, pitched down


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s[:2])
def test_ambiguity_cap_holds_at_every_size(size):
    ref = S.reference_of(0, size)
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP and (ref["ids"] >= 0).any()


@pytest.mark.parametrize("which,size", S.COUNTS, ids=lambda v: str(v).replace(" ", ""))
def test_ambiguity_cap_holds_over_every_count_launch(which, size):
    refs = [S.reference_of(k, size) for k in which]
    assert np.mean([r["ambiguous"].mean() for r in refs]) <= AMBIGUOUS_CAP
    assert sum((r["ids"] >= 0).sum() for r in refs) > 0


def test_other_mount_changes_the_picture():
    ref = depth_ref.reference(S.scene(3), S.sensor(), S.WIDTH, S.HEIGHT, _R().robot_primitives(), mount=S.OTHER_MOUNT)
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP
    assert np.abs(ref["depth"] - S.reference_of(3)["depth"]).max() > 0.05
    assert abs(np.linalg.norm(S.OTHER_MOUNT[3:7]) - 1.0) < 1e-6


def test_c_abi_is_declared_and_exported():
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd import build as b
    src = " ".join(open(os.path.join(REPO, "include", "t1render.h")).read().split())
    assert ("typedef struct t1render_sensor { int32_t body; float pos[3], quat[4], vfov, near, far; } "
            "t1render_sensor;") in src
    assert "#define T1RENDER_DEPTH_F16 1" in src
    assert ("int t1render_depth(t1env* env, const t1render_sensor* sensor, const float* mounts, const t1render_prim* "
            "prims, int32_t nprims, int32_t width, int32_t height, int32_t flags, void* depth, int8_t* ids, "
            "void* stream);") in src
    for words in ("eye = p_b + R_b pos", "PLANAR depth z = t (d.f)", "exactly far", "near <= z <= far"):
        assert words in src, words
    assert ("t1render_depth.hip", "-O3") in b.UNITS
    assert _lib.RENDER_DEPTH_EXPORTS == ["t1render_depth"] and _lib.RENDER_DEPTH_F16 == 1
    assert not set(_lib.RENDER_DEPTH_EXPORTS) & set(_lib.EXPORTS + _lib.POLICY_EXPORTS + _lib.RENDER_EXPORTS +
                                                    _lib.RENDER_SCENE_EXPORTS + _lib.RENDER_MESH_EXPORTS)
    assert _lib.C.sizeof(_lib.RenderSensor) == 44
    b.build()
    lib = _lib.load()
    assert len(lib.t1render_depth.argtypes) == 11
    # argument errors are reported before any device work
    assert lib.t1render_depth(None, None, None, None, 0, 4, 4, 0, None, None, None) == -1
    assert b"t1render_depth" in lib.t1env_last_error()


def test_default_config_has_the_sensor_switched_off():
    from ti5_isaacgym_amd import task_registry
    cfg, _ = task_registry.get_cfgs("t1_dh_stand")
    dc = cfg.env.depth_camera
    assert dc.enable is False and dc.update_interval == 1 and (dc.width, dc.height, dc.far) == (64, 48, 3.0)
    assert dc.dtype == "fp32" and len(dc.pos) == 3 and len(dc.rpy) == 3


def test_rpy_quat_is_the_urdf_convention():
    R = _R()
    np.testing.assert_allclose(R.rpy_quat(0.3, -0.2, 1.1), S.rpy_quat(0.3, -0.2, 1.1), atol=1e-15)
    # a positive pitch turns +x towards -z: the camera looks down
    fwd = depth_ref.quat_rot(R.rpy_quat(0.0, 0.5, 0.0), np.float64)[:, 0]
    np.testing.assert_allclose(fwd, [np.cos(0.5), 0.0, -np.sin(0.5)], atol=1e-15)


def test_play_refuses_bad_depth_arguments_and_keeps_its_defaults():
    from ti5_isaacgym_amd.scripts import play
    base = ["--checkpoint", "none.pt", "--depth", "d"]
    a = play.parse(base)
    assert (a.depth, a.depth_size, a.depth_every, a.depth_range) == ("d", [64, 48], 2, [0.1, 3.0])
    assert a.depth_mount == [0.1, 0.0, 0.1, 0.0, 0.6, 0.0] and (a.render, a.render_every) == (None, 2)
    for bad in (["--depth_every", "0"], ["--depth_size", "0", "4"], ["--depth_size", "4", "-1"],
                ["--depth_range", "0", "3"], ["--depth_range", "2", "1"], ["--depth_range", "0.1", "300"]):
        with pytest.raises(ValueError, match="--depth"):
            play.parse(base + bad)
    with pytest.raises(ValueError, match="8 GiB"):
        play.parse(base + ["--steps", "100000000", "--depth_size", "640", "480"])
    assert play.parse(["--checkpoint", "none.pt", "--depth_every", "0"]).depth is None   # no --depth: no check
