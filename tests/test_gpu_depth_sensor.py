"""The depth camera sensor on the MI355X (csrc/t1render_depth.hip through utils/render.DepthSensor) against the numpy
fp64 reference tests/depth_ref.py, on the scenes of tests/depth_scenes.py and on poses the physics made.

Compared on the non-ambiguous pixels (depth_ref.reference: the fp64 rays through the pixel's centre and 1e-3 pixel beside
it agree on the id, the terrain triangle and the side of near and far; at most 1% of a launch may be ambiguous): ids
exactly, pixels without a hit exactly far, a hit's depth within DEPTH_ATOL and DEPTH_RTOL.  Where two surfaces with
different ids tie within 1e-5 m along the ray -- consecutive limb capsules share their joint sphere, and float places
its centre through two different sums -- either id is accepted and the depth is compared all the same (depth_ref.TIE).

The depth tolerance is measured (tools/depth_parity.py, profiles/depth_sensor_parity.json): depth_ref in float32 against
float64 on the five trimesh envs and on plane poses after reset() and five random-action steps differs by at most
2.45e-5 m and 4.40e-5 relative; the kernel is allowed 8 x that, the factor tests/test_gpu_render.py uses and justifies
(it contracts to fma and orders its sums differently from numpy).  Its own worst errors, 9.5e-6 m and 1.8e-5, are in the
same file."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import depth_ref  # noqa: E402
import depth_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
DEPTH_ATOL, DEPTH_RTOL = FACTOR * 2.45e-5, FACTOR * 4.40e-5   # profiles/depth_sensor_parity.json: fp32_vs_fp64 x factor
AMBIGUOUS_CAP = 0.01
E_ARG = -1
W, H = S.WIDTH, S.HEIGHT


def _R():
    from ti5_isaacgym_amd.utils import render
    return render


def _plane_env(n=3, seed=31):
    from ti5_isaacgym_amd import make_t1_env
    return make_t1_env(num_envs=n, mesh_type="plane", seed=seed, device=DEV)


def _stepped(n=3, seed=31, steps=5):
    env = _plane_env(n, seed)
    env.reset()
    g = torch.Generator().manual_seed(6)
    for _ in range(steps):
        env.step(torch.randn(n, 12, generator=g).to(DEV))
    return env


@pytest.fixture(scope="module")
def tri_env():
    """The 6 x 4 trimesh env of depth_scenes with the synthetic poses written straight into rigid_state."""
    from ti5_isaacgym_amd import make_t1_env
    env = make_t1_env(num_envs=S.NUM_ENVS, mesh_type="trimesh", seed=S.SEED, device=DEV, cfg_hook=S.terrain_hook)
    assert np.array_equal(env.height_samples.cpu().numpy(), S.trimesh_terrain()["h"])
    env.rigid_state.copy_(torch.from_numpy(np.array(S.trimesh_poses())))
    return env


def _sensor(env, sensor, w=W, h=H, **kw):
    kw.setdefault("ids", True)
    return _R().DepthSensor(env, w, h, sensor["pos"], quat=sensor["quat"], body=sensor["body"], vfov=sensor["vfov"],
                            near=sensor["near"], far=sensor["far"], **kw)


def _images(s):
    depth = s.render()
    torch.cuda.synchronize()
    n = s.env.num_envs
    assert depth.data_ptr() == s.depth.data_ptr() and depth.shape == (n, s.height, s.width)
    return depth.float().cpu().numpy(), None if s.ids is None else s.ids.cpu().numpy().astype(np.int64)


def _check_launch(refs, depth, ids, far):
    """every env of a launch against its reference; the ambiguity cap holds over the launch"""
    assert np.mean([r["ambiguous"].mean() for r in refs]) <= AMBIGUOUS_CAP
    assert (depth >= np.float32(0.1)).all() and (depth <= np.float32(far)).all()
    worst = [depth_ref.compare(r, depth[n], ids[n], far, DEPTH_ATOL, DEPTH_RTOL) for n, r in enumerate(refs)]
    return max(w[0] for w in worst), max(w[1] for w in worst)


def _plane_refs(env, sensor, w=W, h=H, mounts=None):
    rigid = env.rigid_state.cpu().numpy()
    prims = _R().robot_primitives()
    return [depth_ref.reference(dict(rigid=rigid[n], terrain=None), sensor, w, h, prims,
                                mount=None if mounts is None else mounts[n]) for n in range(env.num_envs)]


# ---- 1. trimesh
def test_trimesh_five_envs_in_one_launch(tri_env):
    depth, ids = _images(_sensor(tri_env, S.sensor()))
    refs = [S.reference_of(n) for n in range(S.NUM_ENVS)]
    _check_launch(refs, depth, ids, S.SENSOR["far"])
    assert (ids == 0).sum() > 100 and (ids > 0).sum() > 30 and (depth == np.float32(3.0)).sum() > 30
    assert len({depth[n].tobytes() for n in range(S.NUM_ENVS)}) == S.NUM_ENVS


# ---- 2. plane, poses the physics made
@pytest.mark.parametrize("steps", [0, 5])
def test_plane_poses_the_physics_made(steps):
    """3 envs after reset() and after 5 random-action steps, the camera inside the base's box looking down and back
    under it: the robot's own legs are in the picture, the box that holds the camera is not."""
    env = _stepped(steps=steps)
    sensor = S.plane_sensor()
    depth, ids = _images(_sensor(env, sensor))
    _check_launch(_plane_refs(env, sensor), depth, ids, sensor["far"])
    assert (ids > 0).sum() > 20 and (ids == 0).sum() > 100 and not (ids == 1).any()


# ---- 3. fp16
@pytest.mark.parametrize("size", [(21, 13), (17, 1)], ids=lambda s: "%dx%d" % s)
def test_fp16_is_the_fp32_image_rounded_once(size):
    """odd widths: the rows' 4-byte alignment alternates, so both the packed pair stores and the single ones run"""
    env = _stepped()
    sensor = S.plane_sensor()
    w, h = size
    full = _sensor(env, sensor, w, h)
    half = _sensor(env, sensor, w, h, dtype=torch.float16)
    half.depth.fill_(-1.0)
    a, b = full.render(), half.render()
    torch.cuda.synchronize()
    assert b.dtype == torch.float16 and a.dtype == torch.float32
    assert torch.equal(a.half().view(torch.int16), b.view(torch.int16))
    assert torch.equal(full.ids, half.ids) and a.unique().numel() > 3


# ---- 4. sizes and counts
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s[:2])
def test_image_sizes(tri_env, size):
    w, h, vfov = size
    s = _sensor(tri_env, S.sensor(vfov=vfov), w, h)
    depth, ids = _images(s)
    ref = S.reference_of(0, size)
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP
    depth_ref.compare(ref, depth[0], ids[0], S.SENSOR["far"], DEPTH_ATOL, DEPTH_RTOL)


@pytest.mark.parametrize("which,size", S.COUNTS, ids=lambda v: str(v).replace(" ", ""))
def test_env_counts_that_do_not_fill_the_workgroups(which, size):
    """depth_scenes.COUNTS: env counts that are no multiple of the envs a workgroup holds, a single env, and images whose
    blocks straddle workgroups; each env has one of the trimesh scenes' five poses."""
    n, which = len(which), list(which)
    from ti5_isaacgym_amd import make_t1_env
    env = make_t1_env(num_envs=n, mesh_type="trimesh", seed=S.SEED, device=DEV, cfg_hook=S.terrain_hook)
    assert np.array_equal(env.height_samples.cpu().numpy(), S.trimesh_terrain()["h"])
    env.rigid_state.copy_(torch.from_numpy(np.array(S.trimesh_poses())[which]))
    w, h, vfov = size
    s = _sensor(env, S.sensor(vfov=vfov), w, h)
    s.depth.fill_(-7.0)
    depth, ids = _images(s)
    _check_launch([S.reference_of(k, size) for k in which], depth, ids, S.SENSOR["far"])


# ---- 5. mounts
def test_mounts_replace_the_mount_env_by_env(tri_env):
    sensor = S.sensor()
    plain = _sensor(tri_env, sensor)
    base, base_ids = _images(plain)
    q = [float(np.float32(v)) for v in sensor["quat"]]   # the call's own normalisation: double, summed in order
    qq = 0.0
    for v in q:
        qq += v * v
    row = np.float32(list(sensor["pos"]) + [v / math.sqrt(qq) for v in q])
    mounts = torch.from_numpy(np.tile(row, (S.NUM_ENVS, 1))).to(DEV)
    same, same_ids = _images(_sensor(tri_env, sensor, mounts=mounts))
    assert np.array_equal(base.view(np.int32), same.view(np.int32)) and np.array_equal(base_ids, same_ids)
    mounts[3] = torch.from_numpy(S.OTHER_MOUNT).to(DEV)
    other, other_ids = _images(_sensor(tri_env, sensor, mounts=mounts))
    keep = [0, 1, 2, 4]
    assert np.array_equal(base[keep].view(np.int32), other[keep].view(np.int32))
    assert np.array_equal(base_ids[keep], other_ids[keep]) and not np.array_equal(base[3], other[3])
    ref = depth_ref.reference(S.scene(3), sensor, W, H, _R().robot_primitives(), mount=S.OTHER_MOUNT)
    assert ref["ambiguous"].mean() <= AMBIGUOUS_CAP
    depth_ref.compare(ref, other[3], other_ids[3], sensor["far"], DEPTH_ATOL, DEPTH_RTOL)


# ---- 6. optional ids
def test_ids_are_optional(tri_env):
    with_ids, _ = _images(_sensor(tri_env, S.sensor()))
    s = _sensor(tri_env, S.sensor(), ids=False)
    assert s.ids is None
    without, _ = _images(s)
    assert np.array_equal(with_ids.view(np.int32), without.view(np.int32))


# ---- 7. isolation
def test_render_is_repeatable_and_touches_no_env_state():
    env, twin = _plane_env(4, seed=21), _plane_env(4, seed=21)
    for e in (env, twin):
        e.reset()
        e.step(torch.zeros(4, 12, device=DEV))
    s = _sensor(env, S.plane_sensor())
    names = ("rigid_state", "root_states")
    before = [getattr(env, k).clone() for k in names] + [o.clone() for o in env._obs]
    one = s.render().clone()
    i1 = s.ids.clone()
    two = s.render()
    torch.cuda.synchronize()
    assert torch.equal(one, two) and torch.equal(i1, s.ids)
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


# ---- 8. graph
def test_captured_render_replays_on_a_later_state():
    env = _stepped(steps=2)
    s = _sensor(env, S.plane_sensor())
    s.render()   # warm: the code object is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.render()
    first = s.depth.clone()
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        env.step(torch.randn(3, 12, generator=g).to(DEV))
    s.depth.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed, replayed_ids = s.depth.clone(), s.ids.clone()
    eager = _sensor(env, S.plane_sensor())
    eager.render()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager.depth) and torch.equal(replayed_ids, eager.ids)
    assert not torch.equal(replayed, first)


# ---- 9. argument errors
def test_argument_errors_leave_the_outputs_untouched():
    """Every T1ENV_E_ARG case of include/t1render.h's t1render_depth.  (T1ENV_E_STATE, a height-field handle without
    samples, cannot be reached through the ABI: t1env_set_terrain refuses such a field.)"""
    from ti5_isaacgym_amd import _lib
    env = _plane_env(2)
    env.reset()
    R = _R()
    prims = R.robot_primitives()
    good = S.plane_sensor()
    depth = torch.full((2, 8, 8), -3.0, device=DEV)
    ids = torch.full((2, 8, 8), 99, dtype=torch.int8, device=DEV)
    lib, h = env._lib, env._handle
    stream = torch.cuda.current_stream().cuda_stream

    def pack(s):
        return _lib.RenderSensor(int(s["body"]), (_lib.f32 * 3)(*s["pos"]), (_lib.f32 * 4)(*s["quat"]), s["vfov"],
                                 s["near"], s["far"])

    def call(sensor=good, prims=prims, w=8, h_=8, flags=0, nprims=None, null=()):
        args = [h, _lib.C.byref(pack(sensor)), None, R.pack_prims(prims), len(prims) if nprims is None else nprims,
                w, h_, flags, depth.data_ptr(), ids.data_ptr(), stream]
        return lib.t1render_depth(*[None if i in null else a for i, a in enumerate(args)])
    nan, inf = float("nan"), float("inf")
    bad = {
        "null env": lambda: call(null=(0,)), "null sensor": lambda: call(null=(1,)), "null depth": lambda: call(null=(8,)),
        "nprims -1": lambda: call(nprims=-1), "nprims 33": lambda: call(nprims=33),
        "null prims": lambda: call(null=(3,)),
        "sensor body -1": lambda: call(dict(good, body=-1)), "sensor body 13": lambda: call(dict(good, body=13)),
        "body -1": lambda: call(prims=[dict(prims[0], body=-1)]), "body 13": lambda: call(prims=[dict(prims[0], body=13)]),
        "kind 2": lambda: call(prims=[dict(prims[0], kind=2)]), "kind -1": lambda: call(prims=[dict(prims[0], kind=-1)]),
        "width 0": lambda: call(w=0), "height 0": lambda: call(h_=0),
        "2^31 pixels": lambda: call(w=32768, h_=32768),
        "flag 2": lambda: call(flags=2), "flag 1 | 4": lambda: call(flags=5),
        "vfov 0": lambda: call(dict(good, vfov=0.0)), "vfov pi": lambda: call(dict(good, vfov=3.1415927)),
        "vfov nan": lambda: call(dict(good, vfov=nan)),
        "near 0": lambda: call(dict(good, near=0.0)), "near == far": lambda: call(dict(good, near=3.0)),
        "near > far": lambda: call(dict(good, near=4.0)), "far 201": lambda: call(dict(good, far=201.0)),
        "near nan": lambda: call(dict(good, near=nan)), "far nan": lambda: call(dict(good, far=nan)),
        "quat zero": lambda: call(dict(good, quat=(0.0, 0.0, 0.0, 0.0))),
        "quat nan": lambda: call(dict(good, quat=(0.0, nan, 0.0, 1.0))),
        "quat inf": lambda: call(dict(good, quat=(inf, 0.0, 0.0, 1.0))),
        "pos nan": lambda: call(dict(good, pos=(0.0, 0.0, nan))), "pos inf": lambda: call(dict(good, pos=(inf, 0.0, 0.0))),
    }
    for name, f in bad.items():
        assert f() == E_ARG, name
        assert b"t1render_depth" in lib.t1env_last_error(), name
    torch.cuda.synchronize()
    assert (depth == -3.0).all() and (ids == 99).all()
    assert call(nprims=0, null=(3,)) == 0   # null prims are legal without primitives
    assert call() == 0                      # and the good call writes both
    torch.cuda.synchronize()
    assert (depth >= 0.1).all() and (depth <= 3.0).all() and (ids < 99).all()


# ---- 10. env
def _depth_hook(cfg):
    dc = cfg.env.depth_camera
    dc.enable, dc.update_interval, dc.width, dc.height = True, 2, 16, 12
    dc.pos, dc.rpy, dc.vfov = list(S.PLANE_SENSOR["pos"]), list(S.PLANE_RPY), S.PLANE_SENSOR["vfov"]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_env_returns_the_image_as_extras_depth(dtype):
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        _depth_hook(cfg)
        cfg.env.depth_camera.dtype = dtype
    env = make_t1_env(num_envs=4, mesh_type="plane", seed=8, device=DEV, cfg_hook=hook)
    want = torch.float16 if dtype == "fp16" else torch.float32
    alone = _sensor(env, S.plane_sensor(), 16, 12, dtype=want, ids=False)

    def fresh():
        out = alone.render().clone()
        torch.cuda.synchronize()
        return out
    env.reset()
    img = env.extras["depth"]
    assert img.shape == (4, 12, 16) and img.dtype == want and img.data_ptr() == env.depth_sensor.depth.data_ptr()
    assert torch.equal(img, fresh())   # reset() leaves a current image, on or off the interval
    g = torch.Generator().manual_seed(3)
    last = img.clone()
    for _ in range(4):
        extras = env.step(torch.randn(4, 12, generator=g).to(DEV))[4]
        torch.cuda.synchronize()
        assert extras["depth"] is img
        if env.common_step_counter % 2 == 0:
            assert torch.equal(img, fresh()) and not torch.equal(img, last)
        else:
            assert torch.equal(img.view(torch.uint8), last.view(torch.uint8))
        last = img.clone()


def test_env_without_the_sensor_is_untouched():
    from ti5_isaacgym_amd import make_t1_env
    env = make_t1_env(num_envs=4, mesh_type="plane", seed=8, device=DEV)
    twin = make_t1_env(num_envs=4, mesh_type="plane", seed=8, device=DEV, cfg_hook=_depth_hook)
    assert env.depth_sensor is None and twin.depth_sensor is not None
    env.reset()
    twin.reset()
    g = torch.Generator().manual_seed(3)
    for _ in range(4):
        act = torch.randn(4, 12, generator=g).to(DEV)
        a, b = env.step(act), twin.step(act)
        torch.cuda.synchronize()
        assert "depth" not in a[4] and "depth" in b[4]
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x, y)
        for k in ("rigid_state", "root_states", "dof_state", "contact_forces", "torques"):
            assert torch.equal(getattr(env, k), getattr(twin, k)), k


# ---- 11. play --depth
def test_play_depth_end_to_end(tmp_path):
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
    out = tmp_path / "depth"
    summary = play.main(common + ["--out", str(tmp_path / "a"), "--depth", str(out), "--depth_every", "2",
                                  "--depth_size", "16", "12"])
    assert summary["depth_frames"] == 3
    assert sorted(os.listdir(out)) == ["depth.npy"] + ["depth_%06d.png" % k for k in range(3)]
    d = np.load(out / "depth.npy")
    assert d.shape == (3, 12, 16) and d.dtype == np.float16
    assert (d >= np.float16(0.1)).all() and (d <= np.float16(3.0)).all() and np.unique(d).size > 1
    for k in range(3):
        with Image.open(out / ("depth_%06d.png" % k)) as im:
            assert im.size == (16, 12)
            px = np.asarray(im)
        assert (px[..., 0] == px[..., 1]).all() and (px[..., 1] == px[..., 2]).all() and np.unique(px).size > 1
    with open(tmp_path / "a" / "summary.json") as f:
        assert json.load(f)["depth_frames"] == 3
    plain = play.main(common + ["--out", str(tmp_path / "b")])
    assert "depth_frames" not in plain
    with open(tmp_path / "b" / "summary.json") as f:
        assert "depth_frames" not in json.load(f)
    assert sorted(os.listdir(tmp_path)) == ["a", "b", "depth", "model_0.pt"]
