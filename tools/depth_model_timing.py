"""Time the depth camera's sensor model (t1render_depth_model) with device events and write
profiles/depth_model_timing.json.

    python tools/depth_model_timing.py [--out profiles/depth_model_timing.json]
    python tools/depth_model_timing.py --bench-lines FILE [--out profiles/depth_model_timing.json]

The protocol of tools/depth_timing.py: 20 launches after 3 warm-ups, one event pair per launch, medians.  32 x 24 and
64 x 48 images at 4096 and 8192 envs on the plane, fp32 and fp16, K = 1 (noise only, no ring) and K = 4 (lags drawn in
[0, 3]), the model's parameters play's --depth_noise.  The clean image is the one t1render_depth drew of the env, and
that launch is timed beside the model's, with their ratio; so is the env's step.  bytes: what the launch must move --
the clean read, the ring write (K > 1) and the out write, plus the delayed read for the envs with a lag (the neighbour
reads of the edge test come from cache and are not counted) -- and the rate that makes of the median.  torch_ops: the
same model written as torch ops over the same tensors (torch's own generator for the draws), timed the same way.

--bench-lines merges the file tools/bench_alternate.py writes (bench.py of the parent commit and of this tree in turn)
into the same profile as "bench_alternated", as tools/render_timing.py does for its profile."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from depth_timing import MOUNT, STEP_MS_QUOTED  # noqa: E402
from render_timing import bench_lines, prepared, timed  # noqa: E402

SIZES = ((32, 24), (64, 48))
ENVS = (4096, 8192)
RINGS = (1, 4)


def model_call(lib, L, noise, clean, ring, lag, out):
    n, h, w = clean.shape
    flags = L.RENDER_DEPTH_F16 if clean.dtype == torch.float16 else 0
    stream = torch.cuda.current_stream().cuda_stream
    K = 1 if ring is None else ring.shape[0]
    state = {"frame": 1}   # frame 0, all fresh, is the caller's first launch below

    def call():
        if lib.t1render_depth_model(L.C.byref(noise), clean.data_ptr(), n, w, h, flags, state["frame"],
                                    None if ring is None else ring.data_ptr(), K, lag.data_ptr(), None,
                                    out.data_ptr(), stream) != 0:
            raise RuntimeError(lib.t1env_last_error().decode())
        state["frame"] += 1
    fresh = torch.ones(n, dtype=torch.uint8, device=clean.device)
    if lib.t1render_depth_model(L.C.byref(noise), clean.data_ptr(), n, w, h, flags, 0,
                                None if ring is None else ring.data_ptr(), K, lag.data_ptr(), fresh.data_ptr(),
                                out.data_ptr(), stream) != 0:
        raise RuntimeError(lib.t1env_last_error().decode())
    return call


def torch_model(p, clean, ring, lag, out):
    """the header's model as torch ops: same steps, torch's generator, a rolled index into the ring"""
    n, h, w = clean.shape
    K = 1 if ring is None else ring.shape[0]
    envs = torch.arange(n, device=clean.device)
    state = {"frame": 1}
    inf = float("inf")

    def call():
        z = clean.float()
        none = (z >= p["far"]) | (torch.rand_like(z) < p["p_drop"])
        pad = torch.nn.functional.pad(z, (1, 1, 1, 1), value=inf)
        mn = torch.minimum(torch.minimum(pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]),
                           torch.minimum(pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]))
        none |= (z - mn > p["edge_abs"] + p["edge_rel"] * mn) & (torch.rand_like(z) < p["p_edge"])
        v = (z + (p["sigma0"] + p["sigma2"] * z * z) * torch.randn_like(z)).clamp_(p["near"], p["far"])
        v = v.masked_fill_(none, p["fill"]).to(clean.dtype)
        if ring is None:
            out.copy_(v)
        else:
            t = state["frame"]
            ring[t % K] = v
            out.copy_(ring[(t - lag) % K, envs])
        state["frame"] += 1
    return call


def main():
    from ti5_isaacgym_amd import _lib as L
    from ti5_isaacgym_amd.scripts.play import DEPTH_NOISE
    from ti5_isaacgym_amd.utils.render import DepthNoise, DepthSensor
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench-lines", default=None, metavar="FILE")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_model_timing.json"))
    a = ap.parse_args()
    if a.bench_lines:
        return bench_lines(a.bench_lines, a.out)
    lib = L.load()
    noise = DepthNoise(**DEPTH_NOISE)
    packed = noise.pack(seed=1, env_base=0, near=MOUNT["near"], far=MOUNT["far"])
    p = dict(DEPTH_NOISE, near=MOUNT["near"], far=MOUNT["far"], edge_abs=noise.edge_abs, edge_rel=noise.edge_rel,
             fill=MOUNT["far"])
    res = {"device": torch.cuda.get_device_name(0), "warmup": 3, "launches": 20,
           "method": "one event pair per launch, launches back to back on one stream",
           "model": p, "step_ms_quoted": STEP_MS_QUOTED}
    for n in ENVS:
        env = prepared(n, "plane")
        g = torch.Generator(device="cuda:0").manual_seed(1)
        act = torch.randn(n, 12, device="cuda:0", generator=g) * 0.3
        row = {"step": timed(lambda: env.step(act))}
        step = row["step"]["median_ms"]
        for w, h in SIZES:
            for name, dtype in (("fp32", torch.float32), ("fp16", torch.float16)):
                s = DepthSensor(env, w, h, MOUNT["pos"], rpy=MOUNT["rpy"], body=MOUNT["body"], vfov=MOUNT["vfov"],
                                near=MOUNT["near"], far=MOUNT["far"], dtype=dtype)
                cell = {"t1render_depth": timed(s.render)}
                clean, esz = s.depth, s.depth.element_size()
                for K in RINGS:
                    ring = torch.zeros(K, n, h, w, dtype=dtype, device=env.device) if K > 1 else None
                    lag = torch.randint(0, K, (n,), generator=torch.Generator().manual_seed(2),
                                        dtype=torch.int32).to(env.device)
                    out = torch.zeros_like(clean)
                    t = timed(model_call(lib, L, packed, clean, ring, lag, out))
                    delayed = int((lag > 0).sum())
                    t["bytes"] = esz * h * w * (n * (3 if K > 1 else 2) + delayed)
                    t["tb_per_s"] = round(t["bytes"] / (t["median_ms"] * 1e-3) / 1e12, 3)
                    t["over_t1render_depth"] = round(t["median_ms"] / cell["t1render_depth"]["median_ms"], 3)
                    t["per_step"] = round(t["median_ms"] / step, 3)
                    t["per_quoted_step"] = round(t["median_ms"] / STEP_MS_QUOTED, 3)
                    t["no_measurement_fraction"] = round(float((out == MOUNT["far"]).float().mean()), 4)
                    tt = timed(torch_model(p, clean, ring, lag, out))
                    tt["over_one_launch"] = round(tt["median_ms"] / t["median_ms"], 1)
                    cell[f"K{K}"] = {"t1render_depth_model": t, "torch_ops": tt}
                    del ring, out
                row[f"{w}x{h}_{name}"] = cell
                print(n, w, h, name, json.dumps(cell), flush=True)
        res[f"plane_{n}"] = row
        del env
    if os.path.exists(a.out):   # keep what --bench-lines put there
        with open(a.out) as f:
            old = json.load(f)
        if "bench_alternated" in old:
            res["bench_alternated"] = old["bench_alternated"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
