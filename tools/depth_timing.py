"""Time the depth camera sensor (t1render_depth) with device events and write profiles/depth_sensor_timing.json.

    python tools/depth_timing.py [--out profiles/depth_sensor_timing.json]
    python tools/depth_timing.py --bench-lines FILE [--out profiles/depth_sensor_timing.json]

The protocol of tools/render_timing.py: 20 launches after 3 warm-ups, one event pair per launch, medians.  32 x 24 and
64 x 48 images at 4096 and 8192 envs, on the plane and on the default trimesh, fp32 and fp16, the camera mounted as
cfg.env.depth_camera's placeholder.  Beside each figure the only way to the same images without the sensor: num_envs / 16
calls of t1render_frame (16 cameras a call, its rgba, depth and ids planes) with the equivalent fixed cameras, computed
on the host from one read of rigid_state that is not timed; one event pair around the whole loop.  And the env's step
(random actions, the same env) timed the same way, with each figure's ratio to it.

--bench-lines merges the file tools/bench_alternate.py writes (bench.py of the parent commit and of this tree in turn)
into the same profile as "bench_alternated", as tools/render_timing.py does for its profile."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from render_timing import bench_lines, prepared, timed  # noqa: E402

SIZES = ((32, 24), (64, 48))
ENVS = (4096, 8192)
MOUNT = dict(pos=(0.1, 0.0, 0.1), rpy=(0.0, 0.6, 0.0), body=0, vfov=0.9, near=0.1, far=3.0)
STEP_MS_QUOTED = 0.111   # profiles/r18a_*: the step at 8192 envs


def quat_rot(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def frame_loop(env, w, h):
    """The loop of t1render_frame calls that draws every env's mounted view: fixed cameras with eye = p_b + R_b pos,
    target = eye + f, up = u, 16 a call, into (num_envs, h, w) planes."""
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.utils import render as R
    n = env.num_envs
    rs = env.rigid_state[:, MOUNT["body"], 0:7].double().cpu().numpy()   # the one read, before the clock starts
    Rb = quat_rot(rs[:, 3:7])
    M = Rb @ quat_rot(np.array(R.rpy_quat(*MOUNT["rpy"])))
    eye = rs[:, 0:3] + Rb @ np.array(MOUNT["pos"])
    tgt, up = eye + M[:, :, 0], M[:, :, 2]
    cams = (_lib.RenderCamera * n)(*[R.Camera.fixed(k, eye[k], tgt[k], up[k], MOUNT["vfov"]).pack() for k in range(n)])
    prims, style = R.robot_primitives(), R.pack_style(R.STYLE)
    pp = R.pack_prims(prims)
    rgba = torch.zeros(n, h, w, dtype=torch.int32, device=env.device)
    depth = torch.zeros(n, h, w, device=env.device)
    ids = torch.zeros(n, h, w, dtype=torch.int32, device=env.device)
    per = _lib.RENDER_MAXCAM
    size = _lib.C.sizeof(_lib.RenderCamera)
    base = _lib.C.addressof(cams)
    stream = torch.cuda.current_stream(env.device).cuda_stream
    calls = [(_lib.C.cast(base + k * size, _lib.C.POINTER(_lib.RenderCamera)), min(per, n - k),
              rgba[k:].data_ptr(), depth[k:].data_ptr(), ids[k:].data_ptr()) for k in range(0, n, per)]
    fn, handle, np_ = env._lib.t1render_frame, env._handle, len(prims)

    def loop():
        for c, m, a, b, d in calls:
            if fn(handle, c, m, pp, np_, _lib.C.byref(style), w, h, a, b, d, stream) != 0:
                raise RuntimeError("t1render_frame failed")
    loop.keep = (cams, pp, style, rgba, depth, ids)
    loop.calls = len(calls)
    return loop


def main():
    from ti5_isaacgym_amd.utils.render import DepthSensor
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench-lines", default=None, metavar="FILE")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_sensor_timing.json"))
    a = ap.parse_args()
    if a.bench_lines:
        return bench_lines(a.bench_lines, a.out)
    res = {"device": torch.cuda.get_device_name(0), "warmup": 3, "launches": 20,
           "method": "one event pair per launch, launches back to back on one stream; frame_loop: one event pair around "
                     "num_envs / 16 t1render_frame calls, the host's pose read outside it",
           "mount": {k: list(v) if isinstance(v, tuple) else v for k, v in MOUNT.items()},
           "step_ms_quoted": STEP_MS_QUOTED}
    for mesh in ("plane", "trimesh"):
        for n in ENVS:
            env = prepared(n, mesh)
            g = torch.Generator(device="cuda:0").manual_seed(1)
            act = torch.randn(n, 12, device="cuda:0", generator=g) * 0.3
            row = {"step": timed(lambda: env.step(act))}
            step = row["step"]["median_ms"]
            for w, h in SIZES:
                cell = {}
                for name, dtype in (("fp32", torch.float32), ("fp16", torch.float16)):
                    s = DepthSensor(env, w, h, MOUNT["pos"], rpy=MOUNT["rpy"], body=MOUNT["body"], vfov=MOUNT["vfov"],
                                    near=MOUNT["near"], far=MOUNT["far"], dtype=dtype, ids=True)
                    cell[name] = timed(s.render)
                    cell[name]["per_step"] = round(cell[name]["median_ms"] / step, 3)
                    cell[name]["per_quoted_step"] = round(cell[name]["median_ms"] / STEP_MS_QUOTED, 3)
                    s.ids = None
                    cell[name + "_no_ids"] = timed(s.render)
                s = DepthSensor(env, w, h, MOUNT["pos"], rpy=MOUNT["rpy"], body=MOUNT["body"], vfov=MOUNT["vfov"],
                                near=MOUNT["near"], far=MOUNT["far"], ids=True)
                s.render()
                ids = s.ids
                cell["pixels"] = {"none_in_range": int((ids < 0).sum()), "terrain": int((ids == 0).sum()),
                                  "robot": int((ids > 0).sum())}
                loop = frame_loop(env, w, h)
                cell["frame_loop"] = timed(loop)
                cell["frame_loop"]["calls"] = loop.calls
                cell["frame_loop_over_one_launch"] = round(cell["frame_loop"]["median_ms"] / cell["fp32"]["median_ms"], 1)
                cell["one_launch_not_slower"] = bool(cell["fp32"]["median_ms"] <= cell["frame_loop"]["median_ms"] and
                                                     cell["fp16"]["median_ms"] <= cell["frame_loop"]["median_ms"])
                row[f"{w}x{h}"] = cell
                print(mesh, n, w, h, json.dumps(cell), flush=True)
            res[f"{mesh}_{n}"] = row
            del env
    if os.path.exists(a.out):   # keep what --bench-lines put there
        with open(a.out) as f:
            old = json.load(f)
        if "bench_alternated" in old:
            res["bench_alternated"] = old["bench_alternated"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "bench_alternated"})[:400])


if __name__ == "__main__":
    main()
