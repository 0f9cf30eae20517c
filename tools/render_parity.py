"""Measure the depth tolerance of tests/test_gpu_render.py and write profiles/render_parity.json.

    python tools/render_parity.py [--out profiles/render_parity.json]
    python tools/render_parity.py --mesh [--out profiles/render_mesh_parity.json]

On the CPU: tests/render_ref.py in float32 against float64 on the trimesh scenes of tests/render_scenes.py, the worst
absolute and relative depth difference over the non-ambiguous pixels that both see the same surface.  The test allows
the kernel FACTOR times that.  With a device: the kernel's own worst errors on the same scenes (else "not measured").

--mesh does the same for tests/test_gpu_render_mesh.py: tests/render_ref_mesh.py in float32 against float64 on scenes 1
and 3 of tests/render_scenes_mesh.py, then t1render_mesh_scene's own worst errors on them."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
FACTOR = 8.0


def mesh_main(out):
    import render_ref_mesh as RM
    import render_scenes as S
    import render_scenes_mesh as SM
    import render_scenes_multi as M
    s1 = SM.scene1()
    cases = [("scene1", dict(rigid=s1["rigid"], terrain=None), s1["cam"], SM.SIZE1, s1["mesh"], SM.style(), False, False,
              SM.reference1),
             ("scene3", dict(rigid=M.poses(), terrain=S.trimesh_terrain()), SM.cameras3()[0], SM.SIZE3, SM.mesh3(),
              M.style(), True, True, lambda: SM.reference3(0))]
    scenes, a32, r32, left_out = {}, 0.0, 0.0, []
    for name, scene, cam, (w, h), mesh, style, others, shadow, ref_of in cases:
        ref = ref_of()
        f32 = RM.render(scene, cam, w, h, mesh, style, np.float32, others, shadow)
        ok = ~ref["ambiguous"]
        same = (f32["ids"] == ref["ids"]) & (f32["envs"] == ref["envs"]) & (f32["tris"] == ref["tris"])
        m = ok & (ref["ids"] >= 0) & same
        for i, j in np.argwhere(ok & ~same):
            left_out.append({"scene": name, "pixel": [int(i), int(j)],
                             "why": "the float32 reference shows another surface here (id %d env %d triangle %d, float64 "
                                    "%d %d %d): no depth difference to take" % (
                                        f32["ids"][i, j], f32["envs"][i, j], f32["tris"][i, j], ref["ids"][i, j],
                                        ref["envs"][i, j], ref["tris"][i, j])})
        err = np.abs(f32["depth"][m].astype(np.float64) - ref["depth"][m])
        scenes[name] = {"size": [w, h], "triangles_in_scene": int(len(mesh["tri"]) * (scene["rigid"].shape[0] if others else 1)),
                        "ambiguous_share": float(ref["ambiguous"].mean()),
                        "fp32_abs": float(err.max()), "fp32_rel": float((err / ref["depth"][m]).max())}
        a32, r32 = max(a32, scenes[name]["fp32_abs"]), max(r32, scenes[name]["fp32_rel"])
    res = {"reference": "tests/render_ref_mesh.py float32 against float64, non-ambiguous pixels on which both show the "
                        "same id, env and triangle",
           "fp32_vs_fp64": {"abs_m": a32, "rel": r32}, "factor": FACTOR,
           "allowed": {"abs_m": FACTOR * a32, "rel": FACTOR * r32}, "left_out": left_out, "scenes": scenes,
           "kernel": "not measured"}
    import torch
    if torch.cuda.is_available():
        from ti5_isaacgym_amd import make_t1_env
        from ti5_isaacgym_amd.utils import render as R
        ka, kr = 0.0, 0.0
        for name, scene, cam, (w, h), mesh, style, others, shadow, ref_of in cases:
            if scene["terrain"] is None:
                env = make_t1_env(num_envs=scene["rigid"].shape[0], mesh_type="plane", seed=11, device="cuda:0")
            else:
                env = make_t1_env(num_envs=scene["rigid"].shape[0], mesh_type="trimesh", seed=S.SEED, device="cuda:0",
                                  cfg_hook=S.terrain_hook)
            env.rigid_state.copy_(torch.from_numpy(np.array(scene["rigid"])))
            rm = R.RobotMesh(mesh["tri"], mesh["body"], mesh["rgb"])
            r = R.Renderer(env, w, h, [R.Camera(cam["env"], cam["eye"], cam["target"], cam["up"], cam["vfov"])],
                           style=style, others=others, terrain_shadow=shadow, mesh=rm)
            rgba = r.render()
            torch.cuda.synchronize()
            a, rel = RM.compare(ref_of(), rgba[0].cpu().numpy(), r.depth[0].cpu().numpy(), r.ids[0].cpu().numpy(),
                                r.envs[0].cpu().numpy(), r.tris[0].cpu().numpy(), np.inf, np.inf)
            scenes[name]["kernel_abs"], scenes[name]["kernel_rel"] = a, rel
            ka, kr = max(ka, a), max(kr, rel)
            rm.close()
        res["kernel"] = {"abs_m": ka, "rel": kr, "device": torch.cuda.get_device_name(0)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("fp32_vs_fp64", "allowed", "kernel")}))


def main():
    import render_ref
    import render_scenes as S
    from ti5_isaacgym_amd.utils import render as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mesh", action="store_true")
    a = ap.parse_args()
    if a.mesh:
        return mesh_main(a.out or os.path.join(REPO, "profiles", "render_mesh_parity.json"))
    out = a.out or os.path.join(REPO, "profiles", "render_parity.json")
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
