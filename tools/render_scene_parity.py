"""Measure the depth tolerance of tests/test_gpu_render_scene.py and write profiles/render_scene_parity.json.

    python tools/render_scene_parity.py [--out profiles/render_scene_parity.json]

On the CPU: tests/render_ref_scene.py in float32 against float64 on cameras A and B of tests/render_scenes_multi.py
(every env's robot, terrain shadows), the worst absolute and relative depth difference over the non-ambiguous pixels
that both see the same surface.  The test allows the kernel FACTOR times that.  With a device: t1render_scene's own
worst errors on the same two cameras (else "not measured").

Lost entries: at 5 m and more render_ref's float32 run now and then drops a primitive's true entry, because its
on-surface test (3e-5 m) is tighter than float32 places a point out there, and reports a later root 3 to 10 cm
behind it.  That is the reference's root filter, not the number format, and 8 x it would allow the kernel 0.8 m.  A
float32 depth more than LOST (a quarter of a limb's radius) behind the float64 entry is counted as such a lost entry
and left out of the figures; what remains is two orders of magnitude smaller."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
FACTOR = 8.0
LOST = 1e-2


def main():
    import render_ref_scene as RS
    import render_scenes as S
    import render_scenes_multi as M
    from ti5_isaacgym_amd.utils import render as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_scene_parity.json"))
    out = ap.parse_args().out
    prims, (w, h) = R.robot_primitives(), M.SIZE
    scene = dict(rigid=M.poses(), terrain=S.trimesh_terrain())
    cams, a32, r32 = {}, 0.0, 0.0
    for k, name in enumerate("AB"):
        ref = M.reference_of(k, "both")
        f32 = RS.render(scene, M.cameras()[k], w, h, prims, M.style(), np.float32)
        ok = ~ref["ambiguous"]
        m = ok & (ref["ids"] >= 0) & (f32["ids"] == ref["ids"]) & (f32["envs"] == ref["envs"])
        same = m
        with np.errstate(invalid="ignore"):
            lost = same & (f32["depth"].astype(np.float64) - ref["depth"] > LOST)
        m = same & ~lost
        err = np.abs(f32["depth"][m].astype(np.float64) - ref["depth"][m])
        cams[name] = {"size": [w, h], "ambiguous_share": float(ref["ambiguous"].mean()),
                      "farthest_hit_m": float(ref["depth"][np.isfinite(ref["depth"])].max()),
                      "fp32_ids_or_envs_differ": int((ok & ((f32["ids"] != ref["ids"]) | (f32["envs"] != ref["envs"]))).sum()),
                      "fp32_lost_entries": int(lost.sum()),
                      "fp32_abs_with_lost_entries": float(np.abs(f32["depth"][same].astype(np.float64) -
                                                                 ref["depth"][same]).max()),
                      "fp32_abs": float(err.max()), "fp32_rel": float((err / ref["depth"][m]).max())}
        a32, r32 = max(a32, cams[name]["fp32_abs"]), max(r32, cams[name]["fp32_rel"])
    res = {"reference": "tests/render_ref_scene.py float32 against float64, non-ambiguous pixels, cameras A and B of "
                        "tests/render_scenes_multi.py, OTHERS | TERRAIN_SHADOW",
           "lost_entry_m": LOST, "fp32_vs_fp64": {"abs_m": a32, "rel": r32}, "factor": FACTOR,
           "allowed": {"abs_m": FACTOR * a32, "rel": FACTOR * r32}, "cameras": cams, "kernel": "not measured"}
    import torch
    if torch.cuda.is_available():
        from ti5_isaacgym_amd import make_t1_env
        env = make_t1_env(num_envs=M.NUM_ENVS, mesh_type="trimesh", seed=S.SEED, device="cuda:0", cfg_hook=S.terrain_hook)
        assert np.array_equal(env.height_samples.cpu().numpy(), S.trimesh_terrain()["h"])
        env.rigid_state.copy_(torch.from_numpy(np.array(M.poses())))
        r = R.Renderer(env, w, h, [R.Camera(c["env"], c["eye"], c["target"], c["up"], c["vfov"]) for c in M.cameras()],
                       style=M.style(), others=True, terrain_shadow=True)
        rgba = r.render()
        torch.cuda.synchronize()
        ka, kr = 0.0, 0.0
        for k, name in enumerate("AB"):
            a, rel = RS.compare(M.reference_of(k, "both"), rgba[k].cpu().numpy(), r.depth[k].cpu().numpy(),
                                r.ids[k].cpu().numpy(), r.envs[k].cpu().numpy(), np.inf, np.inf)
            cams[name]["kernel_abs"], cams[name]["kernel_rel"] = a, rel
            ka, kr = max(ka, a), max(kr, rel)
        res["kernel"] = {"abs_m": ka, "rel": kr, "device": torch.cuda.get_device_name(0)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("fp32_vs_fp64", "allowed", "kernel")}))


if __name__ == "__main__":
    main()
