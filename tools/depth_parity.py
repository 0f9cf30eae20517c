"""Measure the depth tolerance of tests/test_gpu_depth_sensor.py and write profiles/depth_sensor_parity.json.

    python tools/depth_parity.py [--out profiles/depth_sensor_parity.json]

On the CPU: tests/depth_ref.py in float32 against float64, the worst absolute and relative depth difference over the
non-ambiguous hit pixels on which both show the same surface, on the scenes of the test's comparisons 1 and 2: the five
trimesh envs of tests/depth_scenes.py at 21 x 13, and the plane with poses the physics made -- three envs after reset()
and after five random-action steps.  The test takes its plane poses from the device; here they come from the CPU
restatement of the same physics (oracle/cpu_env.py), the same kind of scene: a standing robot seen from inside its own
base.  The test allows the kernel FACTOR times the two numbers.  With a device: the kernel's own worst errors on the
same scenes, its plane poses its own (else "not measured")."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
FACTOR = 8.0
PLANE_ENVS, PLANE_STEPS, PLANE_SEED = 3, 5, 31


def cpu_plane_poses():
    """rigid_state of the CPU restatement after reset() and after PLANE_STEPS random-action steps"""
    from oracle.cpu_env import CpuT1Env
    from ti5_isaacgym_amd import task_registry
    from ti5_isaacgym_amd.envs.t1_env import build_model
    cfg, _ = task_registry.get_cfgs("t1_dh_stand")
    cpu = CpuT1Env(build_model(cfg)[0], PLANE_ENVS, seed=PLANE_SEED, mesh_type="plane")
    cpu.reset()
    out = {"plane_reset": cpu.rigid.copy()}
    rng = np.random.default_rng(6)
    for _ in range(PLANE_STEPS):
        cpu.step(rng.standard_normal((PLANE_ENVS, 12)).astype(np.float32))
    out["plane_steps"] = cpu.rigid.copy()
    return out


def main():
    import depth_ref
    import depth_scenes as S
    from ti5_isaacgym_amd.utils import render as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_sensor_parity.json"))
    a = ap.parse_args()
    prims = R.robot_primitives()
    w, h = S.WIDTH, S.HEIGHT
    cases = [("trimesh_env%d" % n, S.scene(n), S.sensor(), S.reference_of(n)) for n in range(S.NUM_ENVS)]
    for name, rigid in cpu_plane_poses().items():
        for n in range(PLANE_ENVS):
            sc = dict(rigid=rigid[n], terrain=None)
            cases.append(("%s_env%d" % (name, n), sc, S.plane_sensor(), depth_ref.reference(sc, S.plane_sensor(), w, h, prims)))
    scenes, a32, r32 = {}, 0.0, 0.0
    for name, scene, sensor, ref in cases:
        f32 = depth_ref.render(scene, sensor, w, h, prims, np.float32)
        ok = ~ref["ambiguous"]
        m = ok & (ref["ids"] >= 0) & (f32["ids"] == ref["ids"])
        err = np.abs(f32["depth"][m].astype(np.float64) - ref["depth"][m])
        scenes[name] = {"size": [w, h], "ambiguous_share": float(ref["ambiguous"].mean()),
                        "robot_pixels": int((ok & (ref["ids"] > 0)).sum()),
                        "fp32_ids_differ": int((ok & (f32["ids"] != ref["ids"])).sum()),
                        "fp32_abs": float(err.max()) if m.any() else 0.0,
                        "fp32_rel": float((err / ref["depth"][m]).max()) if m.any() else 0.0}
        a32, r32 = max(a32, scenes[name]["fp32_abs"]), max(r32, scenes[name]["fp32_rel"])
    res = {"reference": "tests/depth_ref.py float32 against float64, non-ambiguous hit pixels; trimesh: "
                        "tests/depth_scenes.py, plane: poses of oracle/cpu_env.py after reset() and 5 random-action steps",
           "fp32_vs_fp64": {"abs_m": a32, "rel": r32}, "factor": FACTOR,
           "allowed": {"abs_m": FACTOR * a32, "rel": FACTOR * r32}, "scenes": scenes, "kernel": "not measured"}
    import torch
    if torch.cuda.is_available():
        from ti5_isaacgym_amd import make_t1_env
        dev = "cuda:0"
        kernel, ka, kr = {}, 0.0, 0.0

        def measure(name, env, sensor):
            nonlocal ka, kr
            s = R.DepthSensor(env, w, h, sensor["pos"], quat=sensor["quat"], body=sensor["body"], vfov=sensor["vfov"],
                              near=sensor["near"], far=sensor["far"], ids=True)
            depth, ids = s.render().cpu().numpy(), s.ids.cpu().numpy()
            rigid = env.rigid_state.cpu().numpy()
            T = S.trimesh_terrain() if env.mesh_type == "trimesh" else None
            for n in range(env.num_envs):
                ref = depth_ref.reference(dict(rigid=rigid[n], terrain=T), sensor, w, h, prims)
                e, r = depth_ref.compare(ref, depth[n], ids[n], sensor["far"], np.inf, np.inf)
                kernel["%s_env%d" % (name, n)] = {"kernel_abs": e, "kernel_rel": r}
                ka, kr = max(ka, e), max(kr, r)
        env = make_t1_env(num_envs=S.NUM_ENVS, mesh_type="trimesh", seed=S.SEED, device=dev, cfg_hook=S.terrain_hook)
        assert np.array_equal(env.height_samples.cpu().numpy(), S.trimesh_terrain()["h"])
        env.rigid_state.copy_(torch.from_numpy(np.array(S.trimesh_poses())))
        measure("trimesh", env, S.sensor())
        env = make_t1_env(num_envs=PLANE_ENVS, mesh_type="plane", seed=PLANE_SEED, device=dev)
        env.reset()
        measure("plane_reset", env, S.plane_sensor())
        g = torch.Generator().manual_seed(6)
        for _ in range(PLANE_STEPS):
            env.step(torch.randn(PLANE_ENVS, 12, generator=g).to(dev))
        measure("plane_steps", env, S.plane_sensor())
        res["kernel"] = {"abs_m": ka, "rel": kr, "device": torch.cuda.get_device_name(0), "scenes": kernel}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("fp32_vs_fp64", "allowed")}), json.dumps(res["kernel"])[:200])


if __name__ == "__main__":
    main()
