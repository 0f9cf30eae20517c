"""Time the headless camera (t1render_frame) with device events and write profiles/render_timing.json.

    python tools/render_timing.py [--num-envs 4096] [--out profiles/render_timing.json]

One follow camera at 640 x 360 and at 1920 x 1080, on the plane and on the default trimesh: 20 launches after 3
warm-ups, each between two events; the env's step (random actions, the same env) timed the same way beside it."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
WARMUP, LAUNCHES = 3, 20


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(LAUNCHES)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    from ti5_isaacgym_amd import make_t1_env
    from ti5_isaacgym_amd.utils.render import Camera, Renderer
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_timing.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "num_envs": a.num_envs, "warmup": WARMUP, "launches": LAUNCHES,
           "cameras": 1, "method": "one event pair per launch, launches back to back on one stream"}
    for mesh in ("plane", "trimesh"):
        env = make_t1_env(num_envs=a.num_envs, mesh_type=mesh, seed=3, device="cuda:0")
        env.reset()
        g = torch.Generator(device="cuda:0").manual_seed(1)
        act = torch.randn(a.num_envs, 12, device="cuda:0", generator=g) * 0.3
        for _ in range(20):
            env.step(act)
        row = {"step": timed(lambda: env.step(act))}
        if mesh == "trimesh":
            row["height_field"] = list(env.height_samples.shape)
        for w, h in ((640, 360), (1920, 1080)):
            r = Renderer(env, w, h, [Camera.follow(0)])
            row[f"{w}x{h}"] = timed(r.render)
            ids = r.ids[0]
            row[f"{w}x{h}"]["pixels"] = {"sky": int((ids < 0).sum()), "terrain": int((ids == 0).sum()),
                                         "robot": int((ids > 0).sum())}
        res[mesh] = row
        del env
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
