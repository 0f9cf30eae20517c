"""The headless camera on the MI355X (csrc/t1render.hip through utils/render.py) against the numpy fp64 ray caster
tests/render_ref.py, on the scenes of tests/render_scenes.py.

Compared on the non-ambiguous pixels (render_ref.reference: the fp64 rays through the pixel's centre and 1e-3 pixel
beside it agree on id, lit flag and terrain triangle; at most 1% of a scene may be ambiguous): ids exactly, the lit
decision, colour within 1 LSB, depth within DEPTH_ATOL and DEPTH_RTOL.

The depth tolerance is measured (tools/render_parity.py, profiles/render_parity.json): render_ref in float32 against
float64 on the trimesh scenes differs by at most 2.03e-4 m and 8.68e-5 relative (the capsules' quadratic cancels: its
constant term is |o - a|^2 - r^2 with |o - a| ~ 3 m and r = 0.04 m); the kernel is allowed 8 x that, because it
contracts to fma and orders its sums differently from numpy.  Its own worst errors are in the same file."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_ref  # noqa: E402
import render_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
DEPTH_ATOL, DEPTH_RTOL = FACTOR * 2.03e-4, FACTOR * 8.68e-5   # profiles/render_parity.json: fp32_vs_fp64 x factor
AMBIGUOUS_CAP = 0.01
E_ARG = -1


def _R():
    from ti5_isaacgym_amd.utils import render
    return render


def _camera(c):
    return _R().Camera(c["env"], c["eye"], c["target"], c["up"], c["vfov"], c["follow"])


def _plane_env(n=2, seed=11):
    from ti5_isaacgym_amd import make_t1_env
    return make_t1_env(num_envs=n, mesh_type="plane", seed=seed, device=DEV)


@pytest.fixture(scope="module")
def tri_env():
    """The 6 x 4 trimesh env of render_scenes with the synthetic poses written straight into rigid_state."""
    from ti5_isaacgym_amd import make_t1_env
    env = make_t1_env(num_envs=S.NUM_ENVS, mesh_type="trimesh", seed=S.SEED, device=DEV, cfg_hook=S.terrain_hook)
    T = S.trimesh_terrain()
    assert np.array_equal(env.height_samples.cpu().numpy(), T["h"])
    tc = env.cfg.terrain
    assert (tc.horizontal_scale, tc.vertical_scale, float(tc.border_size)) == (T["hscale"], T["vscale"], T["border"])
    env.rigid_state.copy_(torch.from_numpy(np.array(S.trimesh_poses())))
    return env


def _render(env, cams, w, h):
    r = _R().Renderer(env, w, h, [_camera(c) for c in cams])
    rgba = r.render()
    torch.cuda.synchronize()
    assert rgba.shape == (len(cams), h, w, 4) and rgba.dtype == torch.uint8 and rgba.data_ptr() == r.rgba.data_ptr()
    return rgba.cpu().numpy(), r.depth.cpu().numpy(), r.ids.cpu().numpy()


def _check(ref, rgba, depth, ids):
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP
    return render_ref.compare(ref, rgba, depth, ids, DEPTH_ATOL, DEPTH_RTOL)


# ---- A. plane
@pytest.mark.parametrize("steps", [0, 1])
def test_plane_follow_camera_matches_the_reference(steps):
    """2 envs after reset() (and after one more step, when rigid_state holds a pose the physics made), a follow camera
    on env 1, 50 x 37: no multiple of the tile in either axis."""
    env = _plane_env()
    env.reset()
    for _ in range(steps):
        env.step(torch.zeros(2, 12, device=DEV))
    w, h = S.PLANE_SIZE
    rgba, depth, ids = _render(env, [S.PLANE_CAMERA], w, h)
    rigid = env.rigid_state.cpu().numpy()
    R = _R()
    ref = render_ref.reference(dict(rigid=rigid[1], terrain=None), S.PLANE_CAMERA, w, h, R.robot_primitives(), R.STYLE)
    _check(ref, rgba[0], depth[0], ids[0])
    assert (ids[0] == 0).any() and (ids[0] == -1).any()
    if steps:
        assert (ids[0] > 0).sum() > 20   # the robot stands in the picture


# ---- B. trimesh
def test_trimesh_three_cameras_in_one_call(tri_env):
    cams = S.trimesh_cameras()
    rgba, depth, ids = _render(tri_env, cams, 48, 32)
    for k in range(3):
        _check(S.reference_of("B%d" % k), rgba[k], depth[k], ids[k])
    assert len({rgba[k].tobytes() for k in range(3)}) == 3


def test_trimesh_straight_down_camera(tri_env):
    """up = (1, 0, 0); the centre ray has zero x and y components, its row and column one zero component each."""
    rgba, depth, ids = _render(tri_env, [S.down_camera()], 33, 33)
    ref = S.reference_of("Bdown")
    _check(ref, rgba[0], depth[0], ids[0])
    assert not ref["ambiguous"][16, 16] and ids[0, 16, 16] == ref["ids"][16, 16] and np.isfinite(depth[0, 16, 16])


# ---- C. footprint edge
def test_rays_that_leave_the_footprint_show_the_sky(tri_env):
    rgba, depth, ids = _render(tri_env, [S.edge_camera()], 40, 24)
    _check(S.reference_of("C"), rgba[0], depth[0], ids[0])
    assert (ids[0] == -1).sum() > 100 and (ids[0] == 0).sum() > 100


# ---- D. image sizes
@pytest.mark.parametrize("size", S.SIZES_D, ids=lambda s: "%dx%d" % s[:2])
def test_image_sizes(tri_env, size):
    w, h, vfov = size
    rgba, depth, ids = _render(tri_env, [dict(S.trimesh_cameras()[0], vfov=vfov)], w, h)
    _check(S.reference_of("D%dx%d" % (w, h)), rgba[0], depth[0], ids[0])


# ---- E. optional outputs
def _frame(env, cams, prims, style, w, h, rgba, depth, ids, ncams=None, nprims=None):
    from ti5_isaacgym_amd import _lib
    R = _R()
    cc = (_lib.RenderCamera * max(len(cams), 1))(*[_camera(c).pack() for c in cams])
    return env._lib.t1render_frame(env._handle, cc, len(cams) if ncams is None else ncams, R.pack_prims(prims),
                                   len(prims) if nprims is None else nprims, _lib.C.byref(R.pack_style(style)), w, h,
                                   rgba.data_ptr() if rgba is not None else None,
                                   depth.data_ptr() if depth is not None else None,
                                   ids.data_ptr() if ids is not None else None,
                                   torch.cuda.current_stream().cuda_stream)


def test_depth_and_ids_are_optional(tri_env):
    R = _R()
    cams = S.trimesh_cameras()
    full, _, _ = _render(tri_env, cams, 48, 32)
    only = torch.zeros(3, 32, 48, 4, dtype=torch.uint8, device=DEV)
    assert _frame(tri_env, cams, R.robot_primitives(), R.STYLE, 48, 32, only, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(only.cpu().numpy(), full)


# ---- F. isolation
def test_render_is_repeatable_and_touches_no_env_state():
    env, twin = _plane_env(4, seed=21), _plane_env(4, seed=21)
    for e in (env, twin):
        e.reset()
        e.step(torch.zeros(4, 12, device=DEV))
    r = _R().Renderer(env, 50, 37, [_R().Camera.follow(0), _R().Camera.follow(3)])
    names = ("rigid_state", "root_states")
    before = [getattr(env, k).clone() for k in names] + [o.clone() for o in env._obs]
    one = r.render().clone()
    d1, i1 = r.depth.clone(), r.ids.clone()
    two = r.render()
    torch.cuda.synchronize()
    assert torch.equal(one, two) and torch.equal(d1, r.depth) and torch.equal(i1, r.ids)
    after = [getattr(env, k) for k in names] + list(env._obs)
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # a step after a render is, bit for bit, the twin's step that never rendered
    g = torch.Generator().manual_seed(5)
    act = torch.randn(4, 12, generator=g).to(DEV)
    out_a, out_b = env.step(act), twin.step(act)
    torch.cuda.synchronize()
    for a, b in zip(out_a[:4], out_b[:4]):
        assert torch.equal(a, b)
    for k in names + ("dof_state", "contact_forces", "torques"):
        assert torch.equal(getattr(env, k), getattr(twin, k)), k


# ---- G. follow mode
def test_follow_camera_equals_the_fixed_camera_at_base_plus_offset():
    env = _plane_env(3, seed=31)
    env.reset()
    g = torch.Generator().manual_seed(6)
    for _ in range(5):
        env.step(torch.randn(3, 12, generator=g).to(DEV))
    R = _R()
    offset, look = (2.5, -1.0, 0.8), (0.0, 0.0, 0.5)
    follow, _, _ = _render(env, [dict(env=2, follow=True, eye=offset, target=look, up=(0, 0, 1), vfov=0.9)], 50, 37)
    base = env.rigid_state[2, 0, 0:3].cpu().numpy()   # the one read
    assert np.abs(base[:2]).max() > 0 and base[2] > 0.3
    eye = (np.float32(offset) + base).tolist()         # the device's own fp32 additions
    tgt = (np.float32(look) + base).tolist()
    fixed, _, _ = _render(env, [dict(env=2, follow=False, eye=eye, target=tgt, up=(0, 0, 1), vfov=0.9)], 50, 37)
    assert np.array_equal(follow, fixed)
    assert (follow[0, ..., :3].reshape(-1, 3) != follow[0, 0, 0, :3]).any()


# ---- H. argument errors
def test_argument_errors_leave_the_outputs_untouched():
    """Every T1ENV_E_ARG case of include/t1render.h.  (T1ENV_E_STATE, a height-field handle without samples, cannot be
    reached through the ABI: t1env_set_terrain refuses such a field, as for t1env_measure_heights.)"""
    env = _plane_env(2)
    env.reset()
    R = _R()
    prims, style = R.robot_primitives(), R.STYLE
    cam = dict(env=0, follow=False, eye=(3, 0, 1), target=(0, 0, 0.5), up=(0, 0, 1), vfov=0.9)
    rgba = torch.full((1, 8, 8, 4), 77, dtype=torch.uint8, device=DEV)
    depth = torch.full((1, 8, 8), -3.0, device=DEV)
    ids = torch.full((1, 8, 8), 99, dtype=torch.int32, device=DEV)
    lib, h = env._lib, env._handle

    def call(cams=(cam,), prims=prims, w=8, h_=8, **kw):
        return _frame(env, list(cams), prims, style, w, h_, rgba, depth, ids, **kw)
    bad = {
        "ncams 0": lambda: call(ncams=0), "ncams 17": lambda: call(ncams=17),
        "nprims -1": lambda: call(nprims=-1), "nprims 33": lambda: call(nprims=33),
        "width 0": lambda: call(w=0), "height 0": lambda: call(h_=0),
        "camera env -1": lambda: call(cams=[dict(cam, env=-1)]), "camera env N": lambda: call(cams=[dict(cam, env=2)]),
        "body -1": lambda: call(prims=[dict(prims[0], body=-1)]), "body 13": lambda: call(prims=[dict(prims[0], body=13)]),
        "kind 2": lambda: call(prims=[dict(prims[0], kind=2)]), "kind -1": lambda: call(prims=[dict(prims[0], kind=-1)]),
        "up parallel, fixed": lambda: call(cams=[dict(cam, eye=(1, 2, 5), target=(1, 2, 0))]),
        "up parallel, follow": lambda: call(cams=[dict(cam, follow=True, eye=(0, 0, 4), target=(0, 0, 0))]),
        "up zero": lambda: call(cams=[dict(cam, up=(0, 0, 0))]),
    }
    from ti5_isaacgym_amd import _lib
    cc = (_lib.RenderCamera * 1)(_camera(cam).pack())
    pp, st = R.pack_prims(prims), _lib.C.byref(R.pack_style(style))
    args = [h, cc, 1, pp, len(prims), st, 8, 8, rgba.data_ptr(), depth.data_ptr(), ids.data_ptr(), None]
    for k, name in ((0, "env"), (1, "cams"), (3, "prims"), (5, "style"), (8, "rgba")):
        bad["null " + name] = lambda k=k: lib.t1render_frame(*[None if i == k else a for i, a in enumerate(args)])
    for name, f in bad.items():
        assert f() == E_ARG, name
        assert b"t1render_frame" in lib.t1env_last_error(), name
    torch.cuda.synchronize()
    assert (rgba == 77).all() and (depth == -3.0).all() and (ids == 99).all()
    assert call() == 0   # and the good call writes all three
    torch.cuda.synchronize()
    assert (rgba[..., 3] == 255).all() and (depth > 0).all() and (ids < 99).all()


# ---- I. play --render
def test_play_render_end_to_end(tmp_path):
    from PIL import Image
    from ti5_isaacgym_amd import DHOnPolicyRunner, make_t1_env, task_registry
    from ti5_isaacgym_amd.scripts import play
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    env = make_t1_env(num_envs=64, mesh_type="plane", seed=4, device=DEV)
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(0)
    ckpt = str(tmp_path / "model_0.pt")
    DHOnPolicyRunner(env, class_to_dict(tc), None, device=DEV).save(ckpt)
    common = ["--checkpoint", ckpt, "--num_envs", "4", "--steps", "6", "--mesh_type", "plane"]
    frames = tmp_path / "frames"
    summary = play.main(common + ["--out", str(tmp_path / "a"), "--render", str(frames), "--render_every", "2",
                                  "--render_size", "64", "36"])
    assert summary["frames"] == 3
    assert sorted(os.listdir(frames)) == ["frame_%06d.png" % k for k in range(3)]
    R = _R()
    robot = {((c >> 0) & 255, (c >> 8) & 255, (c >> 16) & 255) for c in (R.COLOR_BASE, R.COLOR_LEFT, R.COLOR_RIGHT,
                                                                          R.COLOR_FEET)}
    for k in range(3):
        with Image.open(frames / ("frame_%06d.png" % k)) as im:
            assert im.size == (64, 36) and im.mode == "RGBA"
            px = np.asarray(im)[..., :3].reshape(-1, 3).astype(np.float64)
        sky = (px[:, 2] > px[:, 0] + 20) & (px[:, 2] >= 200)                 # the sky's blue gradient
        grey = (np.abs(px - px.mean(1, keepdims=True)).max(1) < 12)         # the checker's two greys, lit or shaded
        hue = px / np.maximum(px.max(1, keepdims=True), 1)                  # shading scales a colour, the hue stays
        body = np.zeros(len(px), bool)
        for c in robot:
            body |= (np.abs(hue - np.array(c) / max(c)).max(1) < 0.04) & (px.max(1) > 40) & ~grey
        assert sky.sum() > 50 and grey.sum() > 200 and body.sum() > 20, (k, sky.sum(), grey.sum(), body.sum())
    with open(tmp_path / "a" / "summary.json") as f:
        assert json.load(f)["frames"] == 3
    plain = play.main(common + ["--out", str(tmp_path / "b")])
    assert "frames" not in plain
    with open(tmp_path / "b" / "summary.json") as f:
        assert "frames" not in json.load(f)
    assert not [p for p in os.listdir(tmp_path / "b") if p.endswith(".png")] and sorted(os.listdir(tmp_path)) == \
        ["a", "b", "frames", "model_0.pt"]
