"""Measure the depth tolerance of tests/test_gpu_render.py and write profiles/render_parity.json.

    python tools/render_parity.py [--out profiles/render_parity.json]

On the CPU: tests/render_ref.py in float32 against float64 on the trimesh scenes of tests/render_scenes.py, the worst
absolute and relative depth difference over the non-ambiguous pixels that both see the same surface.  The test allows
the kernel FACTOR times that.  With a device: the kernel's own worst errors on the same scenes (else "not measured")."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
FACTOR = 8.0


def main():
    import render_ref
    import render_scenes as S
    from ti5_isaacgym_amd.utils import render as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_parity.json"))
    out = ap.parse_args().out
    prims = R.robot_primitives()
    scenes, a32, r32 = {}, 0.0, 0.0
    for name, scene, cam, w, h in S.trimesh_cases():
        ref = S.reference_of(name)
        f32 = render_ref.render(scene, cam, w, h, prims, R.STYLE, np.float32)
        ok = ~ref["ambiguous"]
        m = ok & (ref["ids"] >= 0) & (f32["ids"] == ref["ids"])
        err = np.abs(f32["depth"][m].astype(np.float64) - ref["depth"][m])
        scenes[name] = {"size": [w, h], "ambiguous_share": float(ref["ambiguous"].mean()),
                        "fp32_ids_differ": int((ok & (f32["ids"] != ref["ids"])).sum()),
                        "fp32_abs": float(err.max()) if m.any() else 0.0,
                        "fp32_rel": float((err / ref["depth"][m]).max()) if m.any() else 0.0}
        a32, r32 = max(a32, scenes[name]["fp32_abs"]), max(r32, scenes[name]["fp32_rel"])
    res = {"reference": "tests/render_ref.py float32 against float64, non-ambiguous pixels, trimesh scenes",
           "fp32_vs_fp64": {"abs_m": a32, "rel": r32}, "factor": FACTOR,
           "allowed": {"abs_m": FACTOR * a32, "rel": FACTOR * r32}, "scenes": scenes, "kernel": "not measured"}
    import torch
    if torch.cuda.is_available():
        from ti5_isaacgym_amd import make_t1_env
        env = make_t1_env(num_envs=S.NUM_ENVS, mesh_type="trimesh", seed=S.SEED, device="cuda:0",
                          cfg_hook=S.terrain_hook)
        assert np.array_equal(env.height_samples.cpu().numpy(), S.trimesh_terrain()["h"])
        env.rigid_state.copy_(torch.from_numpy(np.array(S.trimesh_poses())))
        ka, kr = 0.0, 0.0
        for name, scene, cam, w, h in S.trimesh_cases():
            r = R.Renderer(env, w, h, [R.Camera(cam["env"], cam["eye"], cam["target"], cam["up"], cam["vfov"])])
            rgba = r.render()
            torch.cuda.synchronize()
            a, rel = render_ref.compare(S.reference_of(name), rgba[0].cpu().numpy(), r.depth[0].cpu().numpy(),
                                        r.ids[0].cpu().numpy(), np.inf, np.inf)
            scenes[name]["kernel_abs"], scenes[name]["kernel_rel"] = a, rel
            ka, kr = max(ka, a), max(kr, rel)
        res["kernel"] = {"abs_m": ka, "rel": kr, "device": torch.cuda.get_device_name(0)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("fp32_vs_fp64", "allowed", "kernel")}))


if __name__ == "__main__":
    main()
