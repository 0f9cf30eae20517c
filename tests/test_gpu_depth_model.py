"""The depth camera's sensor model on the MI355X (csrc/t1render_depth_model.hip, utils/render.DepthSensor's noise and
latency, cfg.env.depth_camera.noise / latency_frames) against the numpy reference tests/depth_model_ref.py.

Masks are exact: with fill = -1, outside [near, far], a pixel without a measurement is read off the output, and the
reference in float32 is the header's definition of which pixels those are.  A measured fp32 value may differ from the
float64 reference by TOL = 8 x 1.49e-7 m: 1.49e-7 m is what the float32 roundings cost the reference itself on these
inputs (tools/depth_model_parity.py, profiles/depth_model_parity.json, recomputed in tests/test_depth_model_host.py), and
8 is the factor tests/test_gpu_render.py uses and justifies for a kernel that may contract and reorder.  This kernel does
neither (the header forbids it), so its fp32 output is also asserted equal to the float32 reference to the bit; the
profile records its own worst error (1.49e-7 m, the reference's own).  An fp16 value is within one fp16 ulp of the rounded
reference (measured: 0 ulp)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import depth_model_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 8.0 * 1.4914181178937724e-07   # profiles/depth_model_parity.json: reference_fp32_vs_fp64 x factor
E_ARG = -1
N = M.NUM_ENVS
DTYPES = [torch.float32, torch.float16]


def _lib():
    from ti5_isaacgym_amd import _lib
    return _lib, _lib.load()


def _pack(p):
    L, _ = _lib()
    return L.RenderDepthNoise(p["seed"], p["env_base"], p["near"], p["far"], p["sigma0"], p["sigma2"], p["p_drop"],
                              p["p_edge"], p["edge_abs"], p["edge_rel"], p["fill"])


def _ptr(t):
    return None if t is None else t.data_ptr()


_call, _dev = M.launch, M.to_device


def _check(out, clean_np, p, frame, f16):
    """out (numpy, the kernel's dtype) against the reference on the clean image the kernel read"""
    ref32 = M.measure(clean_np, p, frame, np.float32)
    ref64 = M.measure(clean_np, p, frame, np.float64)
    fill = np.float32(p["fill"])
    got = out.astype(np.float32)
    none = got == fill
    assert np.array_equal(none, ref32["none"])
    m = ~none
    if f16:
        want = ref32["image"].astype(np.float16)
        ulp = np.spacing(np.abs(want[m])).astype(np.float32)
        err = np.abs(got[m] - want[m].astype(np.float32))
        assert (err <= ulp).all(), float((err / ulp).max())
        return float((err / ulp).max())
    both = m & ~ref64["none"]
    err = np.abs(got[both].astype(np.float64) - ref64["image"][both])
    print("worst |kernel - fp64 reference| [m]:", err.max())
    assert err.max() <= TOL, err.max()
    # the header rounds every operation on its own and fuses none: the float32 reference is then met to the bit
    assert np.array_equal(got[m], ref32["image"][m])
    return float(err.max())


# ---- 1. masks and values, at every size
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: "%dx%d" % s)
def test_masks_are_exact_and_values_within_tolerance(size, dtype):
    w, h = size
    f16 = dtype == torch.float16
    clean = _dev(M.clean_images(w, h), dtype)
    clean_np = clean.cpu().numpy()
    # each mask on its own (the other switched off), then every step of the model together
    p = M.params(p_drop=0.1)
    out = _call(p, clean).cpu().numpy()
    ref = M.measure(clean_np, p, 0)
    assert np.array_equal(out.astype(np.float32) == -1.0, ref["drop"] | ref["beyond"]) and ref["drop"].sum() > 0
    p = M.params(p_edge=0.6)
    out = _call(p, clean).cpu().numpy()
    ref = M.measure(clean_np, p, 0)
    assert np.array_equal(out.astype(np.float32) == -1.0, ref["edge"] | ref["beyond"]) and ref["edge"].sum() > 0
    for frame in (0, 1):
        p = M.params(**M.NOISY)
        _check(_call(p, clean, frame).cpu().numpy(), clean_np, p, frame, f16)


# ---- 2. identity
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_zero_parameters_are_the_identity_below_far(dtype):
    clean = _dev(M.clean_images(33, 7), dtype)
    p = M.params(p_edge=0.0, fill=-1.0)
    out = _call(p, clean, frame=3)
    far = clean >= 3.0
    assert far.sum() > 0 and (out[far] == -1.0).all()
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(out[~far].view(bits), clean[~far].view(bits))


# ---- 3. determinism
def test_draws_are_a_function_of_seed_env_and_frame():
    clean = _dev(M.clean_images(17, 5), torch.float32)
    p = M.params(**M.NOISY)
    a, b = _call(p, clean, 2), _call(p, clean, 2)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for other in (_call(p, clean, 3), _call(M.params(seed=99, **M.NOISY), clean, 2),
                  _call(M.params(env_base=1, **M.NOISY), clean, 2)):
        assert not torch.equal(a, other)
        assert (other == -1.0).sum() > 0 and not torch.equal(a == -1.0, other == -1.0)
    shifted = _call(M.params(env_base=2, **M.NOISY), clean[2:5].contiguous(), 2)
    assert torch.equal(shifted.view(torch.int32), a[2:5].view(torch.int32))


# ---- 4. ring
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
def test_ring_serves_the_delayed_frame(K, dtype, noisy):
    """six frames of a moving image, lags 0, 1, 2, 3 and 9 (clamped to K - 1), every env fresh at frame 0 and env 2 at
    frame 3; the ring starts as NaN, which a read of anything not yet written would show"""
    w, h = 17, 5
    f16 = dtype == torch.float16
    lag_np = np.array([0, 1, 2, 3, 9], dtype=np.int32)
    lag = torch.from_numpy(lag_np).to(DEV)
    ring = torch.full((K, N, h, w), float("nan"), dtype=dtype, device=DEV) if K > 1 else None
    ref_ring, ref64_ring = M.Ring(K), M.Ring(K)
    p = M.params(**M.NOISY) if noisy else M.params()
    base = M.clean_images(w, h)
    for t in range(6):
        clean_np = np.clip(base * (1.0 - 0.05 * t), M.NEAR, M.FAR).astype(np.float32)
        clean = _dev(clean_np, dtype)
        clean_np = clean.cpu().numpy()
        fresh_np = np.ones(N, np.uint8) if t == 0 else np.array([0, 0, 1, 0, 0], np.uint8) if t == 3 else None
        fresh = None if fresh_np is None else torch.from_numpy(fresh_np).to(DEV)
        out = _call(p, clean, t, ring, K, lag, fresh).cpu().numpy()
        assert not np.isnan(out.astype(np.float32)).any()
        ref = M.measure(clean_np, p, t, np.float32)
        want = ref_ring.push(M.stored(ref["image"], f16), t, lag_np, fresh_np)
        if not noisy:
            assert np.array_equal(out, want), (K, t)   # values equal as numbers: no NaN on either side
            continue
        # noise on: the served frame's masks exactly, its values within the tolerance of the float64 reference's ring
        assert np.array_equal(out.astype(np.float32) == -1.0, want.astype(np.float32) == -1.0), (K, t)
        want64 = ref64_ring.push(M.measure(clean_np, p, t, np.float64)["image"], t, lag_np, fresh_np)
        m = (want.astype(np.float32) != -1.0) & (want64 != -1.0)
        err = np.abs(out[m].astype(np.float64) - want64[m])
        if f16:
            assert (np.abs(out[m].astype(np.float32) - want[m].astype(np.float32)) <=
                    np.spacing(np.abs(want[m])).astype(np.float32)).all()
        else:
            assert err.max() <= TOL, (K, t, err.max())
    if ring is not None:
        assert not torch.isnan(ring.float()).any()   # all fresh at frame 0 filled every slot


# ---- 5. no read outside clean with p_edge == 0
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_without_edge_test_nothing_outside_clean_is_read(dtype):
    w, h = 17, 5
    img = _dev(M.clean_images(w, h), dtype)
    count = img.numel()
    big = torch.full((3 * count,), float("nan"), dtype=dtype, device=DEV)
    view = big[count: 2 * count].view(N, h, w)
    view.copy_(img)
    p = M.params(sigma0=0.002, sigma2=0.01, p_drop=0.1, p_edge=0.0)
    a, b = _call(p, view, 1), _call(p, img, 1)
    assert not torch.isnan(a.float()).any()
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(a.view(bits), b.view(bits))
    assert torch.isnan(big[:count].float()).all() and torch.isnan(big[2 * count:].float()).all()
    # with the edge test on, the image's border pixels still read nothing outside it
    p = M.params(**M.NOISY)
    a, b = _call(p, view, 1), _call(p, img, 1)
    assert torch.equal(a.view(bits), b.view(bits)) and not torch.isnan(a.float()).any()


# ---- 6. argument errors
def test_argument_errors_leave_the_outputs_untouched():
    L, lib = _lib()
    n, h, w, K = 2, 4, 6, 3
    clean = torch.full((n, h, w), 1.0, device=DEV)
    out = torch.full((n, h, w), -3.0, device=DEV)
    ring = torch.full((K, n, h, w), -5.0, device=DEV)
    whole = torch.full((2 * n, h, w), 1.0, device=DEV)   # clean and out carved from one allocation: overlaps
    bytes_ = torch.zeros(4 * (K + 1) * n * h * w, dtype=torch.uint8, device=DEV)   # for pointers off their element
    stream = torch.cuda.current_stream().cuda_stream
    good = M.params(**M.NOISY)
    nan, inf = float("nan"), float("inf")

    def call(p=good, clean_=clean, n_=n, w_=w, h_=h, flags=0, ring_=ring, K_=K, out_=out, null=()):
        args = [L.C.byref(_pack(p)), _ptr(clean_), n_, w_, h_, flags, 0, _ptr(ring_), K_, None, None, _ptr(out_), stream]
        return lib.t1render_depth_model(*[None if i in null else a for i, a in enumerate(args)])
    bad = {
        "null m": lambda: call(null=(0,)), "null clean": lambda: call(null=(1,)), "null out": lambda: call(null=(11,)),
        "null ring, K 3": lambda: call(null=(7,)),
        "K 0": lambda: call(K_=0), "K 17": lambda: call(K_=17), "K -1": lambda: call(K_=-1),
        "num_envs 0": lambda: call(n_=0), "width 0": lambda: call(w_=0), "height 0": lambda: call(h_=0),
        "2^31 pixels": lambda: call(n_=2, w_=32768, h_=32768, ring_=None, K_=1),
        "flag 2": lambda: call(flags=2), "flag 1 | 4": lambda: call(flags=5),
        "near 0": lambda: call(dict(good, near=0.0)), "near == far": lambda: call(dict(good, near=3.0)),
        "far 201": lambda: call(dict(good, far=201.0)), "near nan": lambda: call(dict(good, near=nan)),
        "far nan": lambda: call(dict(good, far=nan)),
        "p_drop -0.1": lambda: call(dict(good, p_drop=-0.1)), "p_drop 1.1": lambda: call(dict(good, p_drop=1.1)),
        "p_drop nan": lambda: call(dict(good, p_drop=nan)),
        "p_edge -0.1": lambda: call(dict(good, p_edge=-0.1)), "p_edge 1.1": lambda: call(dict(good, p_edge=1.1)),
        "p_edge nan": lambda: call(dict(good, p_edge=nan)),
        "sigma0 < 0": lambda: call(dict(good, sigma0=-1e-3)), "sigma0 inf": lambda: call(dict(good, sigma0=inf)),
        "sigma2 < 0": lambda: call(dict(good, sigma2=-1e-3)), "sigma2 nan": lambda: call(dict(good, sigma2=nan)),
        "edge_abs < 0": lambda: call(dict(good, edge_abs=-1.0)), "edge_abs inf": lambda: call(dict(good, edge_abs=inf)),
        "edge_rel < 0": lambda: call(dict(good, edge_rel=-1.0)), "edge_rel nan": lambda: call(dict(good, edge_rel=nan)),
        "fill nan": lambda: call(dict(good, fill=nan)), "fill inf": lambda: call(dict(good, fill=-inf)),
        "out is clean": lambda: call(out_=clean),
        "out overlaps clean": lambda: call(clean_=whole[:n], out_=whole.view(-1)[n * h * w - 1:][:n * h * w]),
        "ring overlaps clean": lambda: call(clean_=ring[1]),
        "ring overlaps out": lambda: call(out_=ring[2]),
        "clean off its element": lambda: call(clean_=bytes_[1:].view(-1)[:4 * n * h * w]),
        "out off its element": lambda: call(out_=bytes_[2:].view(-1)[:4 * n * h * w]),
        "ring off its element": lambda: call(ring_=bytes_[3:].view(-1)[:4 * K * n * h * w]),
        "fp16 out off its element": lambda: call(flags=1, clean_=clean.view(torch.float16)[0],
                                                 out_=bytes_[1:].view(-1)[:2 * n * h * w], ring_=None, K_=1),
    }
    for name, f in bad.items():
        assert f() == E_ARG, name
        assert b"t1render_depth_model" in lib.t1env_last_error(), name
    torch.cuda.synchronize()
    assert (out == -3.0).all() and (ring == -5.0).all() and (clean == 1.0).all() and (bytes_ == 0).all()
    assert call(ring_=None, K_=1) == 0   # a null ring is legal with K == 1
    assert call() == 0
    torch.cuda.synchronize()
    assert (out != -3.0).all() and (ring[0] != -5.0).all() and (ring[1:] == -5.0).all()   # frame 0, none fresh: slot 0


# ---- 7. DepthSensor
def _plane_env(n=3, seed=31, hook=None):
    from ti5_isaacgym_amd import make_t1_env
    return make_t1_env(num_envs=n, mesh_type="plane", seed=seed, device=DEV, cfg_hook=hook)


MOUNT = dict(pos=(0.1, 0.0, 0.1), rpy=(0.0, 0.6, 0.0))


def test_sensor_without_a_model_is_what_it_was():
    from ti5_isaacgym_amd.utils.render import DepthSensor
    env = _plane_env()
    env.reset()
    s = DepthSensor(env, 16, 12, noise=None, latency=(0, 0), **MOUNT)
    assert not hasattr(s, "measured") and not hasattr(s, "lag")
    d = s.render()
    assert d is s.depth
    torch.cuda.synchronize()
    assert (d >= 0.1).all() and (d <= 3.0).all() and d.unique().numel() > 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_sensor_with_a_model_measures_its_own_clean_image(dtype):
    from ti5_isaacgym_amd.utils.render import DepthNoise, DepthSensor
    env = _plane_env()
    env.reset()
    g = torch.Generator().manual_seed(6)
    for _ in range(5):
        env.step(torch.randn(3, 12, generator=g).to(DEV))
    noise = DepthNoise(fill=-1.0, **M.NOISY)
    s = DepthSensor(env, 17, 11, dtype=dtype, noise=noise, latency=(0, 2), seed=7, env_base=4, **MOUNT)
    twin = DepthSensor(env, 17, 11, dtype=dtype, **MOUNT)
    assert s.measured.shape == s.depth.shape and s.measured.dtype == dtype and s.measured.data_ptr() != s.depth.data_ptr()
    assert s.lag.dtype == torch.int32 and s.lag.shape == (3,) and 0 <= int(s.lag.min()) and int(s.lag.max()) <= 2
    s.lag.copy_(torch.tensor([0, 1, 2], dtype=torch.int32))   # kept by reference
    p = M.params(seed=7 ^ M.SEED_SALT, env_base=4, **M.NOISY)
    f16 = dtype == torch.float16
    ring = M.Ring(3)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    for t in range(4):
        if t:
            env.step(torch.randn(3, 12, generator=g).to(DEV))
        out = s.render()
        clean = twin.render()
        torch.cuda.synchronize()
        assert out is s.measured and s.frame == t + 1
        assert torch.equal(s.depth.view(bits), clean.view(bits))
        clean_np = s.depth.cpu().numpy()
        ref = M.measure(clean_np, p, t, np.float32)
        want = ring.push(M.stored(ref["image"], f16), t, [0, 1, 2], np.ones(3, np.uint8) if t == 0 else None)
        got = out.cpu().numpy()
        assert np.array_equal(got.astype(np.float32) == -1.0, want.astype(np.float32) == -1.0), t
        m = want.astype(np.float32) != -1.0
        err = np.abs(got[m].astype(np.float64) - want[m].astype(np.float64))
        tol = np.spacing(np.abs(want[m])).astype(np.float64) if f16 else TOL
        assert (err <= tol).all(), (t, err.max())
        assert m.sum() > 100 and (~m).sum() > 5


# ---- 8. env
def _env_hook(interval, model):
    def hook(cfg):
        dc = cfg.env.depth_camera
        dc.enable, dc.update_interval, dc.width, dc.height = True, interval, 16, 12
        if model:
            dc.latency_frames = [2, 2]
            dc.noise.enable = True   # every noise parameter at its zero default
    return hook


@pytest.mark.parametrize("interval", [1, 2])
def test_env_serves_the_delayed_image_and_none_of_the_last_episode(interval):
    env = _plane_env(4, seed=8, hook=_env_hook(interval, True))
    twin = _plane_env(4, seed=8, hook=_env_hook(interval, False))
    assert hasattr(env.depth_sensor, "measured") and not hasattr(twin.depth_sensor, "measured")
    assert env.depth_sensor.lag.tolist() == [2, 2, 2, 2]
    env.reset()
    twin.reset()
    torch.cuda.synchronize()
    assert env.extras["depth"] is env.depth_sensor.measured and twin.extras["depth"] is twin.depth_sensor.depth
    renders = [env.depth_sensor.depth.clone()]          # the clean image of every render so far
    assert torch.equal(env.extras["depth"], renders[0])  # reset() renders with every env fresh
    born = [0, 0, 0, 0]                                  # the render at which an env's history began
    pending = set()                                      # the envs reset since the last render
    g = torch.Generator().manual_seed(3)
    steps, kill_at = 12 * interval, 3 * interval + 1
    seen_after_reset = 0
    for k in range(steps):
        if k == kill_at:
            for e in (env, twin):
                e.episode_length_buf[1] = int(e.max_episode_length)
        act = 0.3 * torch.randn(4, 12, generator=g).to(DEV)
        a, b = env.step(act), twin.step(act)
        torch.cuda.synchronize()
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x, y)
        assert a[4]["episode"].keys() == b[4]["episode"].keys()
        for key, val in a[4]["episode"].items():
            assert torch.equal(torch.as_tensor(val), torch.as_tensor(b[4]["episode"][key])), key
        for name in ("rigid_state", "root_states", "dof_state", "contact_forces", "torques"):
            assert torch.equal(getattr(env, name), getattr(twin, name)), name
        assert torch.equal(env.depth_sensor.depth, twin.depth_sensor.depth)
        rendered = env.common_step_counter % interval == 0
        if rendered:
            renders.append(env.depth_sensor.depth.clone())
            t = len(renders) - 1
            for e in pending:
                born[e] = t
            pending.clear()
            img = a[4]["depth"]
            for e in range(4):
                assert torch.equal(img[e], renders[max(t - 2, born[e])][e]), (k, e)
            if born[1] and t - born[1] < 3:
                seen_after_reset += 1
                assert not torch.equal(renders[born[1]][1], renders[born[1] - 1][1])
        # an env reset in this step was drawn where it fell (if drawn at all): its history begins at the next render
        pending |= set(torch.nonzero(a[3]).flatten().tolist())
        if k == kill_at:
            assert bool(a[3][1])   # env 1 timed out in this step
    assert seen_after_reset == 3 and born[1] > 0


# ---- 9. play --depth_noise
def test_play_writes_the_measured_images(tmp_path):
    from ti5_isaacgym_amd import DHOnPolicyRunner, make_t1_env, task_registry
    from ti5_isaacgym_amd.scripts import play
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    env = make_t1_env(num_envs=64, mesh_type="plane", seed=4, device=DEV)
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(0)
    ckpt = str(tmp_path / "model_0.pt")
    DHOnPolicyRunner(env, class_to_dict(tc), None, device=DEV).save(ckpt)
    common = ["--checkpoint", ckpt, "--num_envs", "4", "--steps", "6", "--mesh_type", "plane", "--depth_every", "1",
              "--depth_size", "16", "12"]
    play.main(common + ["--out", str(tmp_path / "a"), "--depth", str(tmp_path / "clean")])
    summary = play.main(common + ["--out", str(tmp_path / "b"), "--depth", str(tmp_path / "noisy"), "--depth_noise",
                                  "--depth_latency", "2", "2"])
    assert summary["depth_frames"] == 6
    clean, noisy = np.load(tmp_path / "clean" / "depth.npy"), np.load(tmp_path / "noisy" / "depth.npy")
    assert noisy.shape == clean.shape == (6, 12, 16) and noisy.dtype == np.float16
    assert (noisy >= np.float16(0.1)).all() and (noisy <= np.float16(3.0)).all()
    # frames 0 to 2 are the first measurement (every env fresh, then two frames late); frame t >= 2 measures frame t - 2
    near = clean < np.float16(1.5)
    for t in range(6):
        src = clean[max(t - 2, 0)]
        err = np.abs(noisy[t].astype(np.float32) - src.astype(np.float32))[near[max(t - 2, 0)]]
        assert np.median(err) < 0.02 and (err > 0).any(), t   # sigma at 1.5 m is 1.3 cm; dropouts read far
    assert not np.array_equal(noisy[3], noisy[5]) and np.array_equal(noisy[0] == 3.0, noisy[1] == 3.0)
