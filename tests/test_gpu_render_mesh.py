"""t1render_mesh_scene on the MI355X (csrc/t1render_mesh.hip through utils/render.py and the C ABI): against the numpy
fp64 reference tests/render_ref_mesh.py, which tests every ray against every triangle, on the scenes of
tests/render_scenes_mesh.py; against itself without the hierarchy (T1RENDER_MESH_BRUTE) and without env culling
(T1RENDER_SCENE_BRUTE): equal bits; against t1render_frame with nothing to draw; and through play --render_urdf.

Compared with the reference on the non-ambiguous pixels (the fp64 rays through a pixel's centre and 1e-3 pixel beside it
agree on id, env, triangle, lit flag and terrain triangle; at most 1 % of a scene may be ambiguous): ids, envs and tris
exactly, the lit decision, colour within 1 LSB, depth within DEPTH_ATOL and DEPTH_RTOL.

The depth tolerance is measured on these scenes (tools/render_parity.py --mesh, profiles/render_mesh_parity.json):
render_ref_mesh in float32 against float64 differs by at most FP32_ABS and FP32_REL; the kernel is allowed 8 x that, the
factor of tests/test_gpu_render.py and for its reason: it contracts to fma and orders its sums differently from numpy.
The kernel's own worst errors are in the same file."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_ref_mesh as RM  # noqa: E402
import render_scenes as S  # noqa: E402
import render_scenes_mesh as SM  # noqa: E402
import render_scenes_multi as M  # noqa: E402
from ti5_isaacgym_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
FP32_ABS, FP32_REL = 9.16e-5, 2.69e-5   # profiles/render_mesh_parity.json: fp32_vs_fp64
DEPTH_ATOL, DEPTH_RTOL = FACTOR * FP32_ABS, FACTOR * FP32_REL
E_ARG = -1
OTHERS, SHADOW, BRUTE = _lib.RENDER_SCENE_OTHERS, _lib.RENDER_SCENE_TERRAIN_SHADOW, _lib.RENDER_SCENE_BRUTE
MESH_BRUTE = _lib.RENDER_MESH_BRUTE
PLANES = ("rgba", "depth", "ids", "envs", "tris")


def _R():
    from ti5_isaacgym_amd.utils import render
    return render


def _camera(c):
    return _R().Camera(c["env"], c["eye"], c["target"], c["up"], c["vfov"], c["follow"])


def _env(n, mesh="plane", seed=11, hook=None):
    from ti5_isaacgym_amd import make_t1_env
    return make_t1_env(num_envs=n, mesh_type=mesh, seed=seed, device=DEV, cfg_hook=hook)


def _posed(poses, terrain=False):
    poses = np.array(poses)
    env = _env(len(poses), "trimesh", S.SEED, S.terrain_hook) if terrain else _env(len(poses))
    if terrain:
        assert np.array_equal(env.height_samples.cpu().numpy(), S.trimesh_terrain()["h"])
    env.rigid_state.copy_(torch.from_numpy(poses))
    return env


def _mesh(m):
    return _R().RobotMesh(m["tri"], m["body"], m["rgb"])


def _workspace(env, ncams):
    size = env._lib.t1render_mesh_workspace_bytes(int(env.num_envs), ncams)
    assert size >= 16
    return torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)   # its content before the call does not matter


def _scene(env, cams, w, h, mesh, flags, style=None, workspace="auto"):
    """One t1render_mesh_scene call through the C ABI: rgba, depth, ids, envs, tris as numpy arrays."""
    R = _R()
    n = len(cams)
    cc = (_lib.RenderCamera * n)(*[_camera(c).pack() for c in cams])
    rgba = torch.zeros(n, h, w, 4, dtype=torch.uint8, device=DEV)
    depth = torch.zeros(n, h, w, device=DEV)
    ids, envs, tris = (torch.full((n, h, w), 77, dtype=torch.int32, device=DEV) for _ in range(3))
    ws = _workspace(env, n) if workspace == "auto" else workspace
    rc = env._lib.t1render_mesh_scene(env._handle, cc, n, mesh._handle, _lib.C.byref(R.pack_style(style or R.STYLE)),
                                      flags, w, h, rgba.data_ptr(), depth.data_ptr(), ids.data_ptr(), envs.data_ptr(),
                                      tris.data_ptr(), ws.data_ptr() if ws is not None else None,
                                      ws.numel() if ws is not None else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, env._lib.t1env_last_error()
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (rgba, depth, ids, envs, tris))


def _equal_planes(a, b):
    for name, x, y in zip(PLANES, a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name


def _check(ref, out, k=0):
    assert ref["ambiguous"].mean() <= SM.AMBIGUOUS_CAP
    rgba, depth, ids, envs, tris = out
    worst = RM.compare(ref, rgba[k], depth[k], ids[k], envs[k], tris[k], DEPTH_ATOL, DEPTH_RTOL)
    print("ambiguous %.4f, depth worst abs %.3e rel %.3e (allowed %.3e, %.3e)" %
          ((ref["ambiguous"].mean(),) + worst + (DEPTH_ATOL, DEPTH_RTOL)))
    return worst


def _all_four(env, cams, w, h, mesh, flags, style=None):
    """The five planes across {0, MESH_BRUTE} x {0, SCENE_BRUTE}: equal to the bit.  Returns the plain call's."""
    base = _scene(env, cams, w, h, mesh, flags, style)
    for extra in (MESH_BRUTE, BRUTE, MESH_BRUTE | BRUTE):
        _equal_planes(base, _scene(env, cams, w, h, mesh, flags | extra, style, workspace=None if extra & BRUTE else "auto"))
    return base


@pytest.fixture(scope="module")
def one():
    s = SM.scene1()
    return _posed(s["rigid"]), _mesh(s["mesh"])


@pytest.fixture(scope="module")
def pit():
    return _posed(M.poses(), terrain=True), _mesh(SM.mesh3())


# ---- 1. the plane, one env, synthetic meshes
def test_scene_1_matches_the_reference(one):
    env, mesh = one
    s, ref = SM.scene1(), SM.reference1()
    info = mesh.info()
    assert info["ntri"] == len(s["mesh"]["tri"]) and info["max_depth"] <= 9 and info["radius"][5] == 0
    assert (info["radius"][[0, 1, 2, 3, 4, 6, 7, 12]] > 0).all()
    w, h = SM.SIZE1
    out = _scene(env, [s["cam"]], w, h, mesh, 0, workspace=None)
    _check(ref, out)
    rgba, depth, ids, envs, tris = out
    assert set(ids[0][~ref["ambiguous"]].tolist()) == {-1, 0, 1, 2, 3, 4, 5, 7, 13}   # every leaf-size edge is in view
    assert not (tris == s["zero"]).any() and not (ids == 8).any()                     # the zero-area triangle
    quad = np.isin(tris[0], s["quad"])
    assert quad.sum() > 30 and (ids[0][quad] == 7).all()                              # seen from its back side
    assert np.array_equal(envs[0], np.where(ids[0] > 0, 0, -1)) and np.array_equal(tris[0] >= 0, ids[0] > 0)
    # the Renderer's own call gives the same bits
    r = _R().Renderer(env, w, h, [_camera(s["cam"])], mesh=mesh)
    got = r.render()
    torch.cuda.synchronize()
    _equal_planes(out, tuple(x.cpu().numpy() for x in (got, r.depth, r.ids, r.envs, r.tris)))


# ---- 2. ties
def test_ties_go_to_the_lower_env_and_the_lower_triangle():
    s = SM.scene1()
    m = s["mesh"]
    # every triangle twice: the copies are coincident, the lower index must show
    twice = dict(tri=np.concatenate([m["tri"], m["tri"]]), body=np.concatenate([m["body"], m["body"]]),
                 rgb=np.concatenate([m["rgb"], m["rgb"] ^ 0xFFFFFF]))
    env, mesh = _posed(np.repeat(s["rigid"], 2, 0)), _mesh(twice)   # and two envs with identical rows
    w, h = SM.SIZE1
    cam = dict(s["cam"], env=1)
    out = _all_four(env, [cam], w, h, mesh, OTHERS)
    rgba, depth, ids, envs, tris = out
    robot = ids[0] > 0
    assert robot.sum() > 150 and (envs[0][robot] == 0).all() and (envs[0][~robot] == -1).all()
    assert (tris[0][robot] < len(m["tri"])).all()
    # and it is, to the bit, the picture of the single mesh in a single env
    env1, mesh1 = _posed(s["rigid"]), _mesh(m)
    single = _scene(env1, [s["cam"]], w, h, mesh1, 0, workspace=None)
    for name, x, y in zip(PLANES, out, single):
        assert x.tobytes() == y.tobytes(), name
    mesh.close()
    mesh1.close()


# ---- 3. the stair pit
def test_stair_pit_matches_the_reference(pit):
    env, mesh = pit
    w, h = SM.SIZE3
    out = _scene(env, SM.cameras3(), w, h, mesh, OTHERS | SHADOW, style=M.style())
    ref = SM.reference3(0)
    _check(ref, out)
    ok = ~ref["ambiguous"]
    assert len(set(out[3][0][ok].tolist()) - {-1}) >= 4 and set(out[2][0][ok].tolist()) >= set(range(0, 14))
    assert (ref["by_terrain"] & ok).sum() > 50 and (ref["by_robot"] & ok).sum() > 50
    r = _R().Renderer(env, w, h, [_camera(c) for c in SM.cameras3()], style=M.style(), others=True, terrain_shadow=True,
                      mesh=mesh)
    got = r.render()
    torch.cuda.synchronize()
    _equal_planes(out, tuple(x.cpu().numpy() for x in (got, r.depth, r.ids, r.envs, r.tris)))


# ---- 4. the hierarchy and the culling are invisible
def test_brute_equality_on_scene_1(one):
    env, mesh = one
    for flags in (0, OTHERS):
        _all_four(env, [SM.scene1()["cam"]], *SM.SIZE1, mesh, flags)


def test_brute_equality_in_the_stair_pit(pit):
    env, mesh = pit
    for flags in (OTHERS | SHADOW, SHADOW):
        _all_four(env, SM.cameras3() + [M.cameras()[1]], *SM.SIZE3, mesh, flags, style=M.style())


def test_brute_equality_in_a_crowd():
    """200 envs on the plane.  ARM stands outside the view, and so does every primitive the product would draw for it:
    only its arm-like box, part of the base's mesh, reaches into the picture.  CASTER is seen by its shadow alone.
    A culling sphere taken from the primitives instead of the mesh drops ARM from the very tiles its arm shows in
    (render_scenes_mesh.primitives_cull_arm recomputes t1render_scene's bound and tile test for them), and the culled
    picture then differs from the brute one."""
    env, mesh = _posed(SM.crowd_poses()), _mesh(SM.crowd_mesh())
    w, h = SM.CROWD_SIZE
    out = _all_four(env, [SM.crowd_camera()], w, h, mesh, OTHERS)
    envs, tris = out[3][0], out[4][0]
    seen = set(envs.ravel().tolist())
    assert len(seen & set(range(150))) > 3 * 8           # more robots in the picture than three batches hold
    assert SM.ARM in seen and SM.CASTER not in seen
    arm = np.argwhere(envs == SM.ARM)
    assert len(arm) >= 4 and ((tris[envs == SM.ARM] >= SM.ARM_BOX[0]) & (tris[envs == SM.ARM] < SM.ARM_BOX[1])).all()
    assert SM.primitives_cull_arm({(int(j) // 16, int(i) // 16) for i, j in arm})
    assert mesh.info()["radius"][0] > 1.9                # while the mesh's own radius covers the arm
    # the primitives' extent of ARM (what t1render_scene's bound covers) lies wholly outside the camera's view
    R = _R()
    prims_only = R.Renderer(env, w, h, [_camera(SM.crowd_camera())], others=True)
    prims_only.render()
    torch.cuda.synchronize()
    assert not (prims_only.envs == SM.ARM).any()
    # CASTER's shadow is in the picture: without it more ground is lit
    poses = np.array(SM.crowd_poses())
    poses[SM.CASTER, :, 0:2] += 500.0
    env2 = _posed(poses)
    away = _scene(env2, [SM.crowd_camera()], w, h, mesh, OTHERS)
    darker = (out[0][0][..., :3].astype(int).sum(-1) < away[0][0][..., :3].astype(int).sum(-1)) & (out[2][0] == 0)
    assert darker.sum() >= 2 and np.array_equal(out[2], away[2])
    mesh.close()


# ---- 5. nothing to draw
@pytest.mark.parametrize("terrain", [False, True], ids=["plane", "trimesh"])
def test_empty_mesh_equals_render_frame_without_primitives(terrain):
    R = _R()
    env = _posed(S.trimesh_poses(), terrain=True) if terrain else _posed(SM.scene1()["rigid"])
    cams = S.trimesh_cameras()[:2] if terrain else [SM.scene1()["cam"]]
    w, h = (48, 32) if terrain else SM.SIZE1
    empty = R.RobotMesh(np.zeros((0, 3, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint32))
    assert empty.info()["ntri"] == 0 and empty.info()["nnodes"] == 0 and (empty.info()["radius"] == 0).all()
    got = _scene(env, cams, w, h, empty, 0, workspace=None)
    r = R.Renderer(env, w, h, [_camera(c) for c in cams], prims=[])
    rgba = r.render()
    torch.cuda.synchronize()
    for name, x, y in zip(PLANES[:3], got, (rgba.cpu().numpy(), r.depth.cpu().numpy(), r.ids.cpu().numpy())):
        assert x.tobytes() == y.tobytes(), name
    assert (got[3] == -1).all() and (got[4] == -1).all() and (got[2] <= 0).all() and (got[2] == 0).any()
    _equal_planes(got, _scene(env, cams, w, h, empty, OTHERS))   # and with OTHERS there is still nothing
    empty.close()


# ---- 6. repeatability and isolation
def test_mesh_render_is_repeatable_and_touches_no_env_state():
    env, twin = _env(4, seed=21), _env(4, seed=21)
    for e in (env, twin):
        e.reset()
        e.step(torch.zeros(4, 12, device=DEV))
    R = _R()
    mesh = _mesh(SM.crowd_mesh())
    r = R.Renderer(env, 50, 37, [R.Camera.follow(0), R.Camera.follow(3)], others=True, terrain_shadow=True, mesh=mesh)
    names = ("rigid_state", "root_states")
    before = [getattr(env, k).clone() for k in names] + [o.clone() for o in env._obs]
    one = r.render().clone()
    kept = [x.clone() for x in (r.depth, r.ids, r.envs, r.tris)]
    two = r.render()
    torch.cuda.synchronize()
    assert torch.equal(one, two) and all(torch.equal(a, b) for a, b in zip(kept, (r.depth, r.ids, r.envs, r.tris)))
    assert (r.envs >= 0).any() and (r.tris >= 0).any()
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
    mesh.close()


# ---- 7. errors
def test_argument_errors_leave_outputs_and_workspace_untouched():
    env = _env(2)
    env.reset()
    R = _R()
    style = R.STYLE
    mesh = _mesh(SM.crowd_mesh())
    gone = _mesh(SM.crowd_mesh())
    gone_handle = gone._handle.value
    gone.close()
    cam = dict(env=0, follow=False, eye=(3, 0, 1), target=(0, 0, 0.5), up=(0, 0, 1), vfov=0.9)
    rgba = torch.full((1, 8, 8, 4), 77, dtype=torch.uint8, device=DEV)
    depth = torch.full((1, 8, 8), -3.0, device=DEV)
    ids, envs, tris = (torch.full((1, 8, 8), 99, dtype=torch.int32, device=DEV) for _ in range(3))
    lib, h = env._lib, env._handle
    need = lib.t1render_mesh_workspace_bytes(2, 1)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0

    def call(cams=(cam,), mesh_=mesh._handle, style=style, flags=OTHERS, w=8, h_=8, ncams=None, wptr=ws.data_ptr(),
             wbytes=need):
        cc = (_lib.RenderCamera * max(len(cams), 1))(*[_camera(c).pack() for c in cams])
        return lib.t1render_mesh_scene(h, cc, len(cams) if ncams is None else ncams, mesh_,
                                       _lib.C.byref(R.pack_style(style)), flags, w, h_, rgba.data_ptr(), depth.data_ptr(),
                                       ids.data_ptr(), envs.data_ptr(), tris.data_ptr(), wptr, wbytes,
                                       torch.cuda.current_stream().cuda_stream)
    bad = {
        "null mesh": lambda: call(mesh_=None), "destroyed mesh": lambda: call(mesh_=gone_handle),
        "ncams 0": lambda: call(ncams=0), "ncams 17": lambda: call(ncams=17),
        "width 0": lambda: call(w=0), "height 0": lambda: call(h_=0),
        "camera env -1": lambda: call(cams=[dict(cam, env=-1)]), "camera env N": lambda: call(cams=[dict(cam, env=2)]),
        "up parallel": lambda: call(cams=[dict(cam, eye=(1, 2, 5), target=(1, 2, 0))]),
        "up zero": lambda: call(cams=[dict(cam, up=(0, 0, 0))]),
        "vfov 0": lambda: call(cams=[dict(cam, vfov=0.0)]), "vfov pi": lambda: call(cams=[dict(cam, vfov=3.1416)]),
        "light zero": lambda: call(style=dict(style, light=(0, 0, 0))),
        "flag 16": lambda: call(flags=16), "flag -1": lambda: call(flags=-1), "flag 1 | 32": lambda: call(flags=33),
        "others, no workspace": lambda: call(wptr=None, wbytes=0),
        "others | mesh brute, no workspace": lambda: call(flags=OTHERS | MESH_BRUTE, wptr=None, wbytes=need),
        "workspace one byte short": lambda: call(wbytes=need - 1),
        "workspace of zero bytes": lambda: call(wbytes=0),
        "workspace off a 16-byte boundary": lambda: call(wptr=ws.data_ptr() + 4, wbytes=need),
        "workspace off by 8": lambda: call(wptr=ws.data_ptr() + 8, wbytes=need),
    }
    cc = (_lib.RenderCamera * 1)(_camera(cam).pack())
    args = [h, cc, 1, mesh._handle, _lib.C.byref(R.pack_style(style)), OTHERS, 8, 8, rgba.data_ptr(), depth.data_ptr(),
            ids.data_ptr(), envs.data_ptr(), tris.data_ptr(), ws.data_ptr(), need, None]
    for k, name in ((0, "env"), (1, "cams"), (4, "style"), (8, "rgba")):
        bad["null " + name] = lambda k=k: lib.t1render_mesh_scene(*[None if i == k else a for i, a in enumerate(args)])
    for name, f in bad.items():
        assert f() == E_ARG, name
        assert b"t1render_mesh_scene" in lib.t1env_last_error(), name
    torch.cuda.synchronize()
    assert (rgba == 77).all() and (depth == -3.0).all() and all((p == 99).all() for p in (ids, envs, tris))
    assert (ws == 0x5A).all()
    assert lib.t1render_mesh_info(gone_handle, None, None, None, None) == E_ARG
    assert lib.t1render_mesh_destroy(gone_handle) == E_ARG
    assert call() == 0   # and the good call writes all five planes
    torch.cuda.synchronize()
    assert (rgba[..., 3] == 255).all() and (depth > 0).all() and all((p < 99).all() for p in (ids, envs, tris))
    assert (ws[need:] == 0x5A).all() and not (ws[:need] == 0x5A).all()   # nothing past the queried size
    # the workspace may be absent where it is not needed, and depth, ids, envs, tris may each be absent
    for flags in (0, SHADOW, OTHERS | BRUTE, MESH_BRUTE, OTHERS | BRUTE | MESH_BRUTE):
        assert call(flags=flags, wptr=None, wbytes=0) == 0, flags
    for k in (9, 10, 11, 12):
        assert lib.t1render_mesh_scene(*[None if i == k else a for i, a in enumerate(args)]) == 0
    torch.cuda.synchronize()
    # create's refusals
    tri, body, rgb = (np.array(SM.crowd_mesh()[k]) for k in ("tri", "body", "rgb"))
    nan = tri.copy()
    nan[5, 1, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        R.RobotMesh(nan, body, rgb)
    b13 = body.copy()
    b13[3] = 13
    with pytest.raises(RuntimeError, match="body"):
        R.RobotMesh(tri, b13, rgb)
    mesh.close()


# ---- 8. play --render_urdf
def test_play_render_urdf(tmp_path):
    from PIL import Image
    from ti5_isaacgym_amd import DHOnPolicyRunner, make_t1_env, task_registry
    from ti5_isaacgym_amd.scripts import play
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    urdf = SM.synth_robot(str(tmp_path / "robot"))
    env = make_t1_env(num_envs=64, mesh_type="plane", seed=4, device=DEV)
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(0)
    ckpt = str(tmp_path / "model_0.pt")
    DHOnPolicyRunner(env, class_to_dict(tc), None, device=DEV).save(ckpt)
    common = ["--checkpoint", ckpt, "--num_envs", "9", "--steps", "4", "--mesh_type", "plane", "--robot_index", "4",
              "--render_every", "2", "--render_size", "64", "36", "--render_follow", "3.5", "3.5", "3.0", "--render_scene",
              "all"]
    runs = {}
    for name, extra in (("prims", []), ("mesh", ["--render_urdf", urdf])):
        frames = tmp_path / name
        summary = play.main(common + ["--out", str(tmp_path / ("out_" + name)), "--render", str(frames)] + extra)
        assert summary["frames"] == 2 and sorted(os.listdir(frames)) == ["frame_%06d.png" % k for k in range(2)]
        with open(tmp_path / ("out_" + name) / "summary.json") as f:
            assert json.load(f)["frames"] == 2
        runs[name] = []
        for k in range(2):
            with Image.open(frames / ("frame_%06d.png" % k)) as im:
                assert im.size == (64, 36) and im.mode == "RGBA"
                runs[name].append(np.asarray(im).copy())
    assert summary["robot_pixels"] > 5          # some pixels carry ids > 0
    for k in range(2):
        assert not np.array_equal(runs["mesh"][k], runs["prims"][k])
    with pytest.raises(FileNotFoundError):
        play.main(common + ["--out", str(tmp_path / "o"), "--render", str(tmp_path / "f"), "--render_urdf",
                            str(tmp_path / "no.urdf")])
