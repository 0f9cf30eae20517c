"""Time the headless camera (t1render_frame) with device events and write profiles/render_timing.json.

    python tools/render_timing.py [--num-envs 4096] [--out profiles/render_timing.json]
    python tools/render_timing.py --scene [--out profiles/render_scene_timing.json]
    python tools/render_timing.py --mesh [--urdf PATH] [--out profiles/render_mesh_timing.json]
    python tools/render_timing.py --bench-lines FILE [--out profiles/render_mesh_timing.json]

One follow camera at 640 x 360 and at 1920 x 1080, on the plane and on the default trimesh: 20 launches after 3
warm-ups, each between two events; the env's step (random actions, the same env) timed the same way beside it.

--scene times t1render_scene instead: 9 and 4096 envs on the plane, 4096 on the default trimesh, each with
t1render_frame in the same run as the yardstick, then flags = 0, OTHERS and OTHERS | TERRAIN_SHADOW through the new
entry; and OTHERS at 32768 envs on the plane, which shows what the pre-pass over the envs costs.

--mesh times t1render_mesh_scene with the full robot: the visual meshes of --urdf, or, without one, the synthesized
description of tests/render_scenes_mesh.py with the ankle STL under every mesh name (24 links, the same 48k triangles).
The same three envs and two sizes, with and without OTHERS, beside t1render_frame and t1render_scene's OTHERS on the
primitives in the same run, and T1RENDER_MESH_BRUTE on the 9-env plane (5 launches after 1 warm-up: it is slow).
--bench-lines merges the file tools/bench_alternate.py writes (bench.py's result lines of the parent commit and of this
tree in turn, a fresh process each, tagged "parent" / "this_tree") into the same profile as "bench_alternated"."""
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


SIZES = ((640, 360), (1920, 1080))


def scene_call(r, flags):
    """r.render() with the flags given, through t1render_scene whatever they are (a Renderer with both switches off
    calls t1render_frame)."""
    from ti5_isaacgym_amd import _lib
    env, ws = r.env, r.workspace

    def call():
        _lib.check(env._lib.t1render_scene(env._handle, r._cams, len(r.cameras), r._prims, len(r.prims),
                                           _lib.C.byref(r._style), flags, r.width, r.height, r.rgba.data_ptr(),
                                           r.depth.data_ptr(), r.ids.data_ptr(), r.envs.data_ptr(),
                                           ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                           torch.cuda.current_stream(env.device).cuda_stream), "t1render_scene")
    return call


def scene_rows(env, others_only=False):
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.utils.render import Camera, Renderer
    O, T = _lib.RENDER_SCENE_OTHERS, _lib.RENDER_SCENE_TERRAIN_SHADOW
    row = {}
    for w, h in SIZES:
        plain = Renderer(env, w, h, [Camera.follow(0)])
        r = Renderer(env, w, h, [Camera.follow(0)], others=True, terrain_shadow=True)
        cell = {}
        if not others_only:
            cell["t1render_frame"] = timed(plain.render)
            cell["flags_0"] = timed(scene_call(r, 0))
            cell["t1render_frame_again"] = timed(plain.render)   # the run-to-run spread of the yardstick
        cell["others"] = timed(scene_call(r, O))
        if not others_only:
            cell["others_terrain_shadow"] = timed(scene_call(r, O | T))
        seen = torch.unique(r.envs)
        cell["envs_in_the_picture"] = int((seen >= 0).sum())
        row[f"{w}x{h}"] = cell
    return row


def prepared(num_envs, mesh):
    from ti5_isaacgym_amd import make_t1_env
    env = make_t1_env(num_envs=num_envs, mesh_type=mesh, seed=3, device="cuda:0")
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(1)
    act = torch.randn(num_envs, 12, device="cuda:0", generator=g) * 0.3
    for _ in range(20):
        env.step(act)
    return env


def scene_main(out):
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "launches": LAUNCHES, "cameras": 1,
           "method": "one event pair per call, calls back to back on one stream; a call with OTHERS is a memset and "
                     "three launches", "camera": "Camera.follow(0)"}
    for mesh, sizes in (("plane", (9, 4096)), ("trimesh", (4096,))):
        for n in sizes:
            env = prepared(n, mesh)
            res[f"{mesh}_{n}"] = scene_rows(env)
            del env
    env = prepared(32768, "plane")
    res["plane_32768"] = scene_rows(env, others_only=True)
    del env
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def mesh_call(r, flags):
    from ti5_isaacgym_amd import _lib
    env, ws = r.env, r.workspace

    def call():
        _lib.check(env._lib.t1render_mesh_scene(env._handle, r._cams, len(r.cameras), r.mesh._handle,
                                                _lib.C.byref(r._style), flags, r.width, r.height, r.rgba.data_ptr(),
                                                r.depth.data_ptr(), r.ids.data_ptr(), r.envs.data_ptr(), r.tris.data_ptr(),
                                                ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                                torch.cuda.current_stream(env.device).cuda_stream), "t1render_mesh_scene")
    return call


def mesh_main(out, urdf):
    global WARMUP, LAUNCHES
    import tempfile
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.utils.render import Camera, Renderer, RobotMesh
    O, MB = _lib.RENDER_SCENE_OTHERS, _lib.RENDER_MESH_BRUTE
    source = urdf
    if urdf is None:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import render_scenes_mesh as SM
        urdf = SM.synth_robot(tempfile.mkdtemp(prefix="t1_robot_"), box=SM.ankle("L"))
        source = "tests/render_scenes_mesh.synth_robot with the left ankle STL under every mesh name"
    mesh = RobotMesh.from_urdf(urdf)
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "launches": LAUNCHES, "cameras": 1,
           "method": "one event pair per call, calls back to back on one stream; a call with OTHERS is a memset and "
                     "three launches", "camera": "Camera.follow(0)", "robot": source, "mesh": {
                         k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in mesh.info().items()}}
    for terrain, sizes in (("plane", (9, 4096)), ("trimesh", (4096,))):
        for n in sizes:
            env = prepared(n, terrain)
            row = {}
            for w, h in SIZES:
                prims = Renderer(env, w, h, [Camera.follow(0)])
                prims_all = Renderer(env, w, h, [Camera.follow(0)], others=True)
                r = Renderer(env, w, h, [Camera.follow(0)], others=True, mesh=mesh)
                cell = {"t1render_frame": timed(prims.render), "t1render_scene_others": timed(prims_all.render),
                        "mesh_flags_0": timed(mesh_call(r, 0))}
                cell["robot_pixels_own"] = int((r.ids > 0).sum())
                cell["mesh_others"] = timed(mesh_call(r, O))
                cell["robot_pixels_others"] = int((r.ids > 0).sum())
                cell["envs_in_the_picture"] = int((torch.unique(r.envs) >= 0).sum())
                cell["t1render_frame_again"] = timed(prims.render)
                if terrain == "plane" and n == 9:
                    keep = WARMUP, LAUNCHES
                    WARMUP, LAUNCHES = 1, 5
                    cell["mesh_brute_flags_0"] = timed(mesh_call(r, MB))
                    cell["mesh_brute_others"] = timed(mesh_call(r, O | MB))
                    WARMUP, LAUNCHES = keep
                row[f"{w}x{h}"] = cell
                print(terrain, n, w, h, json.dumps(cell), flush=True)
            res[f"{terrain}_{n}"] = row
            del env
    if os.path.exists(out):   # keep what --bench-lines put there
        with open(out) as f:
            old = json.load(f)
        if "bench_alternated" in old:
            res["bench_alternated"] = old["bench_alternated"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def bench_lines(path, out):
    arms = {"parent": [], "this_tree": []}
    with open(path) as f:
        for ln in f:
            tag, _, rest = ln.partition(" ")
            if tag in arms and rest.lstrip().startswith("{"):
                arms[tag].append(json.loads(rest))
    first = arms["parent"][0]
    res = {"command": "tools/bench_alternate.py PARENT --rounds %d --steps %d --warmup %d: bench.py --gpus 1 in the parent "
                      "commit's checkout and in this tree in turn, a fresh process per run" % (
                          len(arms["parent"]), first["steps"], first["warmup"])}
    for tag, rows in arms.items():
        ms = [r["ms_per_step"] for r in rows]
        res[tag] = {"ms_per_step": ms, "env_steps_per_s": [r["value"] for r in rows],
                    "median_ms": statistics.median(ms), "spread_ms": round(max(ms) - min(ms), 4),
                    "median_env_steps_per_s": statistics.median(r["value"] for r in rows)}
    res["medians_differ_by_ms"] = round(abs(res["parent"]["median_ms"] - res["this_tree"]["median_ms"]), 4)
    res["larger_spread_ms"] = max(res["parent"]["spread_ms"], res["this_tree"]["spread_ms"])
    doc = {}
    if os.path.exists(out):
        with open(out) as f:
            doc = json.load(f)
    doc["bench_alternated"] = res
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(res))


def main():
    from ti5_isaacgym_amd import make_t1_env
    from ti5_isaacgym_amd.utils.render import Camera, Renderer
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--scene", action="store_true")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--urdf", default=None)
    ap.add_argument("--bench-lines", default=None, metavar="FILE")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.bench_lines:
        return bench_lines(a.bench_lines, a.out or os.path.join(REPO, "profiles", "render_mesh_timing.json"))
    if a.mesh:
        return mesh_main(a.out or os.path.join(REPO, "profiles", "render_mesh_timing.json"), a.urdf)
    if a.scene:
        return scene_main(a.out or os.path.join(REPO, "profiles", "render_scene_timing.json"))
    a.out = a.out or os.path.join(REPO, "profiles", "render_timing.json")
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
