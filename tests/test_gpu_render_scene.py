"""t1render_scene on the MI355X (csrc/t1render_scene.hip through utils/render.py and the C ABI) against t1render_frame
(flags = 0: equal bits), against the numpy fp64 reference tests/render_ref_scene.py on the scenes of
tests/render_scenes_multi.py, and against itself without culling (T1RENDER_SCENE_BRUTE: equal bits).

Compared with the reference on the non-ambiguous pixels (the fp64 rays through a pixel's centre and 1e-3 pixel beside
it agree on id, env, lit flag and terrain triangle; at most 1% of a scene may be ambiguous): ids and envs exactly, the
lit decision, colour within 1 LSB, depth within DEPTH_ATOL and DEPTH_RTOL.

The depth tolerance is measured on these scenes (tools/render_scene_parity.py, profiles/render_scene_parity.json):
hits lie up to 11 m out, where the capsules' quadratic cancels harder than at the 3 m of tests/test_gpu_render.py.
render_ref_scene in float32 against float64 on cameras A and B differs by at most 2.24e-4 m and 5.19e-5 relative; the
kernel is allowed 8 x that, the factor of tests/test_gpu_render.py and for its reason: it contracts to fma and orders
its sums differently from numpy.  The kernel's own worst errors are in the same file.  Thirteen pixels are left out of
that measurement (never out of this comparison): there the float32 reference drops a primitive's true entry, its
on-surface test of 3e-5 m being tighter than float32 places a point 5 m out, and reports a root 3 to 10 cm behind it;
taking 8 x 0.10 m from them would check nothing."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_ref_scene as RS  # noqa: E402
import render_scenes as S  # noqa: E402
import render_scenes_multi as M  # noqa: E402
from ti5_isaacgym_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
FP32_ABS, FP32_REL = 2.24e-4, 5.19e-5   # profiles/render_scene_parity.json: fp32_vs_fp64
DEPTH_ATOL, DEPTH_RTOL = FACTOR * FP32_ABS, FACTOR * FP32_REL
AMBIGUOUS_CAP = 0.01
E_ARG = -1
OTHERS, SHADOW, BRUTE = _lib.RENDER_SCENE_OTHERS, _lib.RENDER_SCENE_TERRAIN_SHADOW, _lib.RENDER_SCENE_BRUTE
FLAGS = {"others": OTHERS, "shadow": SHADOW, "both": OTHERS | SHADOW}


def _R():
    from ti5_isaacgym_amd.utils import render
    return render


def _camera(c):
    return _R().Camera(c["env"], c["eye"], c["target"], c["up"], c["vfov"], c["follow"])


def _env(n, mesh="plane", seed=11, hook=None):
    from ti5_isaacgym_amd import make_t1_env
    return make_t1_env(num_envs=n, mesh_type=mesh, seed=seed, device=DEV, cfg_hook=hook)


def _tri_env(n, poses):
    env = _env(n, "trimesh", S.SEED, S.terrain_hook)
    assert np.array_equal(env.height_samples.cpu().numpy(), S.trimesh_terrain()["h"])
    env.rigid_state.copy_(torch.from_numpy(np.array(poses)))
    return env


@pytest.fixture(scope="module")
def tri5():
    """tests/test_gpu_render.py's env: the five poses of render_scenes."""
    return _tri_env(S.NUM_ENVS, S.trimesh_poses())


@pytest.fixture(scope="module")
def tri8():
    return _tri_env(M.NUM_ENVS, M.poses())


def _workspace(env, ncams):
    size = env._lib.t1render_scene_workspace_bytes(int(env.num_envs), ncams)
    assert size >= 16
    return torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)   # its content before the call does not matter


def _scene(env, cams, w, h, flags, style=None, workspace="auto"):
    """One t1render_scene call through the C ABI: rgba, depth, ids, envs as numpy arrays."""
    R = _R()
    n = len(cams)
    cc = (_lib.RenderCamera * n)(*[_camera(c).pack() for c in cams])
    prims = R.robot_primitives()
    rgba = torch.zeros(n, h, w, 4, dtype=torch.uint8, device=DEV)
    depth = torch.zeros(n, h, w, device=DEV)
    ids = torch.full((n, h, w), 77, dtype=torch.int32, device=DEV)
    envs = torch.full((n, h, w), 77, dtype=torch.int32, device=DEV)
    ws = _workspace(env, n) if workspace == "auto" else workspace
    rc = env._lib.t1render_scene(env._handle, cc, n, R.pack_prims(prims), len(prims),
                                 _lib.C.byref(R.pack_style(style or R.STYLE)), flags, w, h, rgba.data_ptr(),
                                 depth.data_ptr(), ids.data_ptr(), envs.data_ptr(),
                                 ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, env._lib.t1env_last_error()
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy(), envs.cpu().numpy()


def _frame(env, cams, w, h):
    r = _R().Renderer(env, w, h, [_camera(c) for c in cams])
    rgba = r.render()
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), r.depth.cpu().numpy(), r.ids.cpu().numpy()


def _equal_planes(a, b):
    for name, x, y in zip(("rgba", "depth", "ids", "envs"), a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name


def _check(ref, out, k=0):
    rgba, depth, ids, envs = out
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP
    worst = RS.compare(ref, rgba[k], depth[k], ids[k], envs[k], DEPTH_ATOL, DEPTH_RTOL)
    print("depth worst abs %.3e rel %.3e (allowed %.3e, %.3e)" % (worst + (DEPTH_ATOL, DEPTH_RTOL)))
    return worst


# ---- 1. flags = 0 is t1render_frame
def _same_as_frame(env, cams, w, h):
    want = _frame(env, cams, w, h)
    got = _scene(env, cams, w, h, 0, workspace=None)
    for name, x, y in zip(("rgba", "depth", "ids"), want, got):
        assert x.tobytes() == y.tobytes(), name
    for k, c in enumerate(cams):
        assert np.array_equal(got[3][k], np.where(got[2][k] > 0, c["env"], -1))
    assert (got[2] > 0).any() and (got[2] == 0).any()


def test_no_flags_equals_render_frame_on_the_trimesh(tri5):
    _same_as_frame(tri5, S.trimesh_cameras(), 48, 32)


def test_no_flags_equals_render_frame_on_the_plane():
    env = _env(2)
    env.reset()
    env.step(torch.zeros(2, 12, device=DEV))
    _same_as_frame(env, [S.PLANE_CAMERA], *S.PLANE_SIZE)


# ---- 2. against the reference
@pytest.mark.parametrize("case", ["others", "shadow", "both"])
def test_trimesh_scene_matches_the_reference(tri8, case):
    """Cameras A and B in one call; the Renderer's own call gives the same bits as the raw one."""
    w, h = M.SIZE
    out = _scene(tri8, M.cameras(), w, h, FLAGS[case], style=M.style())
    for k in range(2):
        ref = M.reference_of(k, case)
        _check(ref, out, k)
        if case != "shadow":
            seen = set(out[3][k][~ref["ambiguous"]].tolist()) - {-1}
            assert len(seen) >= 5 and seen - {M.cameras()[k]["env"]}
        else:
            assert set(out[3][k].ravel().tolist()) <= {-1, M.cameras()[k]["env"]}
    r = _R().Renderer(tri8, w, h, [_camera(c) for c in M.cameras()], style=M.style(), others=case != "shadow",
                      terrain_shadow=case != "others")
    rgba = r.render()
    torch.cuda.synchronize()
    _equal_planes(out, (rgba.cpu().numpy(), r.depth.cpu().numpy(), r.ids.cpu().numpy(), r.envs.cpu().numpy()))


# ---- 3. a real plane
COINCIDE = 1e-5   # [m]: ten ulp of a coordinate of 8 m in rigid_state's float32


def test_plane_grid_of_nine_matches_the_reference():
    """Nine robots the physics posed.  Their limbs share joint spheres: the capsule of a link ends where its child's
    begins, posed once through each body, so the two entries differ by the rounding of rigid_state alone (1e-8 to 1e-7 m
    in fp64 here) and no float32 ray caster can tell which is nearer.  Where the fp64 ray enters primitives of another
    id or env within COINCIDE of its nearest entry, the kernel may show any of them, at the reference's depth; such
    pixels count towards the 1 % cap, and everywhere else the comparison is the usual one."""
    env = _env(9, seed=17)
    env.reset()
    env.step(torch.zeros(9, 12, device=DEV))
    rigid = env.rigid_state.cpu().numpy()
    base = rigid[:, 0, 0:3].astype(np.float64)
    corner, mid = base[:, 0:2].min(0), base[:, 0:2].mean(0)
    away = (corner - mid) / np.linalg.norm(corner - mid)
    eye = np.float32([*(corner + 2.5 * away), 3.0]).tolist()   # above and outside a corner of the grid, looking across
    cam = dict(env=0, follow=False, eye=tuple(eye), target=(float(mid[0]), float(mid[1]), 0.5), up=(0.0, 0.0, 1.0),
               vfov=0.9)
    out = _scene(env, [cam], 64, 48, OTHERS | SHADOW)
    R = _R()
    scene = dict(rigid=rigid, terrain=None)
    ref = RS.reference(scene, cam, 64, 48, R.robot_primitives(), R.STYLE)
    mask, sets = RS.coincident(scene, cam, 64, 48, R.robot_primitives(), COINCIDE)
    print("ambiguous %d, coincident %d pixels" % (ref["ambiguous"].sum(), mask.sum()))
    for (i, j), allowed in sets.items():
        if ref["ids"][i, j] > 0 and not ref["ambiguous"][i, j]:
            assert (int(out[2][0, i, j]), int(out[3][0, i, j])) in allowed, (i, j, allowed)
            assert abs(out[1][0, i, j] - ref["depth"][i, j]) <= DEPTH_ATOL
    ref["ambiguous"] = ref["ambiguous"] | mask
    _check(ref, out)
    assert len(set(out[3][0].ravel().tolist()) - {-1}) >= 3
    assert (~ref["lit"] & ~ref["ambiguous"]).sum() > 20 and not ref["by_terrain"].any()   # the plane casts nothing


# ---- 4. culling is invisible
def test_culling_equals_brute_force_in_a_crowd():
    """1000 envs on the plane (render_scenes_multi.crowd_poses), a camera 8 m from the cluster and one 30 m above it."""
    env = _env(M.CROWD_ENVS)
    env.rigid_state.copy_(torch.from_numpy(np.array(M.crowd_poses())))
    w, h = M.CROWD_SIZE
    cams = M.crowd_cameras()
    culled = _scene(env, cams, w, h, OTHERS)
    brute = _scene(env, cams, w, h, OTHERS | BRUTE, workspace=None)
    _equal_planes(culled, brute)
    seen = set(culled[3].ravel().tolist())
    assert len(seen & set(range(300))) > 3 * 8        # the pixels alone show more robots than three batches hold
    assert M.TWIN_LO in seen and M.TWIN_HI not in seen   # identical rows: the lower env
    assert M.FAR not in seen and M.BEHIND not in set(culled[3][0].ravel().tolist())
    assert M.CASTER not in set(culled[3][0].ravel().tolist())


@pytest.mark.parametrize("shadow", [0, SHADOW], ids=["plain", "terrain_shadow"])
def test_culling_equals_brute_force_on_the_trimesh(shadow):
    """The eight poses of test 2 tiled to 200 envs: every robot has 24 exact copies, so every primitive pixel is a tie."""
    env = _tri_env(200, np.tile(M.poses(), (25, 1, 1)))
    w, h = M.SIZE
    culled = _scene(env, M.cameras(), w, h, OTHERS | shadow, style=M.style())
    brute = _scene(env, M.cameras(), w, h, OTHERS | BRUTE | shadow, style=M.style(), workspace=None)
    _equal_planes(culled, brute)
    assert set(culled[3].ravel().tolist()) <= set(range(-1, 8)) and len(set(culled[3].ravel().tolist())) >= 6


def test_tie_and_unseen_caster_match_the_reference():
    """Nine envs of the crowd: the twins (identical rows) and the robot that camera 0 sees only by its shadow."""
    rows = M.crowd_subset()
    env = _env(len(rows))
    env.rigid_state.copy_(torch.from_numpy(np.array(M.crowd_poses()[rows])))
    w, h = M.CROWD_SIZE
    cam = dict(M.crowd_cameras()[0], env=0)
    out = _scene(env, [cam], w, h, OTHERS)
    R = _R()
    ref = RS.reference(dict(rigid=M.crowd_poses()[rows], terrain=None), cam, w, h, R.robot_primitives(), R.STYLE, True, False)
    _check(ref, out)
    lo, hi, caster = rows.index(M.TWIN_LO), rows.index(M.TWIN_HI), rows.index(M.CASTER)
    assert (out[3][0] == lo).sum() >= 20 and not (out[3][0] == hi).any() and not (out[3][0] == caster).any()
    _equal_planes(out, _scene(env, [cam], w, h, OTHERS | BRUTE, workspace=None))


# ---- 5. isolation
def test_scene_render_is_repeatable_and_touches_no_env_state():
    env, twin = _env(4, seed=21), _env(4, seed=21)
    for e in (env, twin):
        e.reset()
        e.step(torch.zeros(4, 12, device=DEV))
    R = _R()
    r = R.Renderer(env, 50, 37, [R.Camera.follow(0), R.Camera.follow(3)], others=True, terrain_shadow=True)
    names = ("rigid_state", "root_states")
    before = [getattr(env, k).clone() for k in names] + [o.clone() for o in env._obs]
    one = r.render().clone()
    d1, i1, e1 = r.depth.clone(), r.ids.clone(), r.envs.clone()
    two = r.render()
    torch.cuda.synchronize()
    assert torch.equal(one, two) and torch.equal(d1, r.depth) and torch.equal(i1, r.ids) and torch.equal(e1, r.envs)
    assert (r.envs >= 0).any()
    after = [getattr(env, k) for k in names] + list(env._obs)
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    g = torch.Generator().manual_seed(5)
    act = torch.randn(4, 12, generator=g).to(DEV)
    out_a, out_b = env.step(act), twin.step(act)
    torch.cuda.synchronize()
    for a, b in zip(out_a[:4], out_b[:4]):
        assert torch.equal(a, b)
    for k in names + ("dof_state", "contact_forces", "torques"):
        assert torch.equal(getattr(env, k), getattr(twin, k)), k


# ---- 6. errors
def test_argument_errors_leave_outputs_and_workspace_untouched():
    env = _env(2)
    env.reset()
    R = _R()
    prims, style = R.robot_primitives(), R.STYLE
    cam = dict(env=0, follow=False, eye=(3, 0, 1), target=(0, 0, 0.5), up=(0, 0, 1), vfov=0.9)
    rgba = torch.full((1, 8, 8, 4), 77, dtype=torch.uint8, device=DEV)
    depth = torch.full((1, 8, 8), -3.0, device=DEV)
    ids = torch.full((1, 8, 8), 99, dtype=torch.int32, device=DEV)
    envs = torch.full((1, 8, 8), 99, dtype=torch.int32, device=DEV)
    lib, h = env._lib, env._handle
    need = lib.t1render_scene_workspace_bytes(2, 1)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0

    def call(cams=(cam,), prims=prims, style=style, flags=OTHERS, w=8, h_=8, ncams=None, nprims=None, wptr=ws.data_ptr(),
             wbytes=need):
        cc = (_lib.RenderCamera * max(len(cams), 1))(*[_camera(c).pack() for c in cams])
        return lib.t1render_scene(h, cc, len(cams) if ncams is None else ncams, R.pack_prims(prims),
                                  len(prims) if nprims is None else nprims, _lib.C.byref(R.pack_style(style)), flags, w, h_,
                                  rgba.data_ptr(), depth.data_ptr(), ids.data_ptr(), envs.data_ptr(), wptr, wbytes,
                                  torch.cuda.current_stream().cuda_stream)
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
        "vfov 0": lambda: call(cams=[dict(cam, vfov=0.0)]), "vfov pi": lambda: call(cams=[dict(cam, vfov=3.1416)]),
        "light zero": lambda: call(style=dict(style, light=(0, 0, 0))),
        "flag 8": lambda: call(flags=8), "flag -1": lambda: call(flags=-1), "flag 1 | 16": lambda: call(flags=17),
        "others, no workspace": lambda: call(wptr=None, wbytes=0),
        "others | shadow, no workspace": lambda: call(flags=OTHERS | SHADOW, wptr=None, wbytes=need),
        "workspace one byte short": lambda: call(wbytes=need - 1),
        "workspace of zero bytes": lambda: call(wbytes=0),
        "workspace off a 16-byte boundary": lambda: call(wptr=ws.data_ptr() + 4, wbytes=need),
        "workspace off by 8": lambda: call(wptr=ws.data_ptr() + 8, wbytes=need),
    }
    cc = (_lib.RenderCamera * 1)(_camera(cam).pack())
    args = [h, cc, 1, R.pack_prims(prims), len(prims), _lib.C.byref(R.pack_style(style)), OTHERS, 8, 8, rgba.data_ptr(),
            depth.data_ptr(), ids.data_ptr(), envs.data_ptr(), ws.data_ptr(), need, None]
    for k, name in ((0, "env"), (1, "cams"), (3, "prims"), (5, "style"), (9, "rgba")):
        bad["null " + name] = lambda k=k: lib.t1render_scene(*[None if i == k else a for i, a in enumerate(args)])
    for name, f in bad.items():
        assert f() == E_ARG, name
        assert b"t1render_scene" in lib.t1env_last_error(), name
    torch.cuda.synchronize()
    assert (rgba == 77).all() and (depth == -3.0).all() and (ids == 99).all() and (envs == 99).all()
    assert (ws == 0x5A).all()
    assert call() == 0   # and the good call writes all four planes
    torch.cuda.synchronize()
    assert (rgba[..., 3] == 255).all() and (depth > 0).all() and (ids < 99).all() and (envs < 99).all()
    assert (ws[need:] == 0x5A).all() and not (ws[:need] == 0x5A).all()   # nothing past the queried size
    # the workspace may be absent where it is not needed
    assert call(flags=0, wptr=None, wbytes=0) == 0 and call(flags=SHADOW, wptr=None, wbytes=0) == 0
    assert call(flags=OTHERS | BRUTE, wptr=None, wbytes=0) == 0
    torch.cuda.synchronize()


# ---- 7. play --render_scene
def _robot_pixels(path):
    from PIL import Image
    R = _R()
    robot = {((c >> 0) & 255, (c >> 8) & 255, (c >> 16) & 255) for c in (R.COLOR_BASE, R.COLOR_LEFT, R.COLOR_RIGHT,
                                                                          R.COLOR_FEET)}
    with Image.open(path) as im:
        assert im.size == (64, 36) and im.mode == "RGBA"
        px = np.asarray(im)[..., :3].reshape(-1, 3).astype(np.float64)
    grey = (np.abs(px - px.mean(1, keepdims=True)).max(1) < 12)         # the checker's two greys, lit or shaded
    hue = px / np.maximum(px.max(1, keepdims=True), 1)                  # shading scales a colour, the hue stays
    body = np.zeros(len(px), bool)
    for c in robot:
        body |= (np.abs(hue - np.array(c) / max(c)).max(1) < 0.04) & (px.max(1) > 40) & ~grey
    return int(body.sum())


def test_play_render_scene_all(tmp_path):
    from ti5_isaacgym_amd import DHOnPolicyRunner, make_t1_env, task_registry
    from ti5_isaacgym_amd.scripts import play
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    env = make_t1_env(num_envs=64, mesh_type="plane", seed=4, device=DEV)
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(0)
    ckpt = str(tmp_path / "model_0.pt")
    DHOnPolicyRunner(env, class_to_dict(tc), None, device=DEV).save(ckpt)
    # from 5 m out and 3 m up along the grid's diagonal the followed robot's neighbours stand in the picture
    common = ["--checkpoint", ckpt, "--num_envs", "9", "--steps", "6", "--mesh_type", "plane", "--robot_index", "4",
              "--render_every", "2", "--render_size", "64", "36", "--render_follow", "3.5", "3.5", "3.0"]
    runs = {}
    for name, extra in (("default", []), ("own", ["--render_scene", "own"]), ("all", ["--render_scene", "all"])):
        frames = tmp_path / name
        summary = play.main(common + ["--out", str(tmp_path / ("out_" + name)), "--render", str(frames)] + extra)
        assert summary["frames"] == 3 and sorted(os.listdir(frames)) == ["frame_%06d.png" % k for k in range(3)]
        runs[name] = [open(frames / ("frame_%06d.png" % k), "rb").read() for k in range(3)]
        with open(tmp_path / ("out_" + name) / "summary.json") as f:
            assert json.load(f)["frames"] == 3
    assert runs["own"] == runs["default"]
    for k in range(3):
        assert runs["all"][k] != runs["own"][k]
        own, everyone = (_robot_pixels(tmp_path / n / ("frame_%06d.png" % k)) for n in ("own", "all"))
        assert own > 5 and everyone > own, (k, own, everyone)
