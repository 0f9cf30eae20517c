"""numpy reference of the depth camera's sensor model, written from the words of include/t1render.h
(t1render_depth_model): the per-pixel measurement in float32 (the header's definition: every operation rounded on its
own) or in float64 (what the float32 roundings cost), and the ring that serves a per-env delay.  Also the synthetic clean
images and the one-launch helper that the host and GPU tests and tools/depth_model_parity.py share."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle.rng import hash4  # noqa: E402

SEED_SALT = 0x5EED0DE7
NEAR, FAR = 0.1, 3.0
NUM_ENVS = 5
SIZES = [(16, 4), (17, 5), (33, 7), (64, 48)]   # (width, height)


def params(**kw):
    """the C struct's fields; seed is the struct's (the Python sensor's seed ^ SEED_SALT)"""
    p = dict(seed=0x1234ABCD, env_base=0, near=NEAR, far=FAR, sigma0=0.0, sigma2=0.0, p_drop=0.0, p_edge=0.0,
             edge_abs=0.05, edge_rel=0.05, fill=-1.0)
    p.update(kw)
    return p


NOISY = dict(sigma0=0.002, sigma2=0.01, p_drop=0.1, p_edge=0.6)   # every step of the model at work


def draws(seed, env_base, frame, n, height, width):
    """h_k (4, n, height, width) uint64 holding 32-bit values"""
    e = (np.arange(n, dtype=np.int64) + int(env_base)).reshape(1, n, 1, 1)
    pix = np.arange(height * width, dtype=np.int64).reshape(1, 1, height, width)
    k = np.arange(4, dtype=np.int64).reshape(4, 1, 1, 1)
    return hash4(np.uint64(int(seed) & 0xFFFFFFFF), e, np.uint64(int(frame) & 0xFFFFFFFF), 4 * pix + k)


def uniform_of(h):
    return (h >> np.uint64(8)).astype(np.float64) * (1.0 / 16777216.0)   # exact in float32 and float64


def gauss_int(h2, h3):
    m = np.uint64(0xFFFF)
    s = (h2 & m) + (h2 >> np.uint64(16)) + (h3 & m) + (h3 >> np.uint64(16))
    return s.astype(np.int64) - 131070


def measure(clean, p, frame, dtype=np.float32):
    """clean (n, H, W) float32 or float16.  Returns dict(image (dtype), none, drop, edge (bool), g): drop are the
    pixels step 2 takes, edge those step 3 takes (after steps 1 and 2), none = nothing in range | drop | edge."""
    T = dtype
    n, H, W = clean.shape
    z = clean.astype(np.float32).astype(T)
    f = lambda x: T(np.float32(x))  # noqa: E731  the struct holds float32
    h = draws(p["seed"], p["env_base"], frame, n, H, W)
    u0, u1 = uniform_of(h[0]).astype(T), uniform_of(h[1]).astype(T)
    beyond = z >= f(p["far"])
    drop = ~beyond & (u0 < f(p["p_drop"]))
    edge = np.zeros_like(drop)
    if np.float32(p["p_edge"]) != 0:
        mn = np.full(z.shape, np.inf, dtype=T)
        mn[:, 1:, :] = np.fmin(mn[:, 1:, :], z[:, :-1, :])
        mn[:, :-1, :] = np.fmin(mn[:, :-1, :], z[:, 1:, :])
        mn[:, :, 1:] = np.fmin(mn[:, :, 1:], z[:, :, :-1])
        mn[:, :, :-1] = np.fmin(mn[:, :, :-1], z[:, :, 1:])
        with np.errstate(invalid="ignore"):
            jump = z - mn
            bound = f(p["edge_abs"]) + f(p["edge_rel"]) * mn
            edge = ~beyond & ~drop & (jump > bound) & (u1 < f(p["p_edge"]))
    s = gauss_int(h[2], h[3])
    c = T(np.float32(np.sqrt(3.0) / 65536.0)) if T is np.float32 else np.sqrt(3.0) / 65536.0
    g = s.astype(T) * c
    v = z + (f(p["sigma0"]) + (f(p["sigma2"]) * z) * z) * g
    v = np.minimum(np.maximum(v, f(p["near"])), f(p["far"]))
    none = beyond | drop | edge
    image = np.where(none, f(p["fill"]), v).astype(T)
    return dict(image=image, none=none, drop=drop, edge=edge, beyond=beyond, g=g)


def stored(image, f16):
    """step 5: what the kernel stores of a float32 image"""
    return image.astype(np.float16) if f16 else image.astype(np.float32)


class Ring:
    """The ring and delay of the header: K slots of (n, H, W); push() stores a measured frame and returns what is served."""

    def __init__(self, K):
        self.K, self.slots = int(K), None

    def push(self, measured, frame, lag=None, fresh=None):
        n = measured.shape[0]
        if self.slots is None:   # content before the first (all fresh) call is never looked at: poison it
            self.slots = np.full((self.K,) + measured.shape, -77.0, dtype=measured.dtype)
        self.slots[frame % self.K] = measured
        if fresh is not None:
            for e in np.nonzero(np.asarray(fresh))[0]:
                self.slots[:, e] = measured[e]
        d = np.zeros(n, dtype=np.int64) if lag is None else np.clip(np.asarray(lag, dtype=np.int64), 0, self.K - 1)
        return np.stack([self.slots[(frame - d[e]) % self.K, e] for e in range(n)])


def clean_images(width, height, near=NEAR, far=FAR):
    """(5, height, width) float32 in [near, far]: two ramps, a step edge, a patch equal to far, and a sloped image with
    a horizontal step."""
    x = (np.arange(width, dtype=np.float64) + 0.5) / width
    y = (np.arange(height, dtype=np.float64) + 0.5) / height
    X, Y = np.meshgrid(x, y)
    img = np.zeros((NUM_ENVS, height, width), dtype=np.float64)
    img[0] = near + (0.95 * far - near) * X
    img[1] = 0.3 + 2.4 * Y
    img[2] = np.where(np.arange(width)[None, :] < width // 2, 0.8, 2.0) + 0.01 * Y
    img[3] = 1.5 + 0.5 * X * Y
    img[3, height // 4: max(height // 4 + 1, 3 * height // 4), width // 3: max(width // 3 + 1, 2 * width // 3)] = far
    img[4] = np.where(np.arange(height)[:, None] < height // 2, 0.6, 2.5) + 0.2 * X
    return img.astype(np.float32)


def f32_vs_f64(frames=(0, 1), f16=False):
    """the largest |float32 - float64| of the reference over the GPU tests' inputs, on the pixels both measure"""
    worst = 0.0
    for w, h in SIZES:
        clean = clean_images(w, h)
        if f16:
            clean = clean.astype(np.float16)
        for frame in frames:
            p = params(**NOISY)
            a, b = measure(clean, p, frame, np.float32), measure(clean, p, frame, np.float64)
            m = ~a["none"] & ~b["none"]
            worst = max(worst, float(np.abs(a["image"][m].astype(np.float64) - b["image"][m]).max()))
    return worst


def to_device(a, dtype, device="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).to(dtype)


def launch(p, clean, frame=0, ring=None, K=1, lag=None, fresh=None, out=None):
    """One t1render_depth_model launch on torch's current stream, synchronised.  clean (n, H, W) device tensor, fp32 or
    fp16; ring, lag, fresh, out: device tensors or None.  Returns out (a new tensor unless given)."""
    import torch
    from ti5_isaacgym_amd import _lib as L
    lib = L.load()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    n, h, w = clean.shape
    out = torch.full_like(clean, 55.0) if out is None else out
    noise = L.RenderDepthNoise(p["seed"], p["env_base"], p["near"], p["far"], p["sigma0"], p["sigma2"], p["p_drop"],
                               p["p_edge"], p["edge_abs"], p["edge_rel"], p["fill"])
    rc = lib.t1render_depth_model(L.C.byref(noise), ptr(clean), n, w, h,
                                  L.RENDER_DEPTH_F16 if clean.dtype == torch.float16 else 0, frame, ptr(ring), K,
                                  ptr(lag), ptr(fresh), ptr(out), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.t1env_last_error()
    torch.cuda.synchronize()
    return out
