"""The bits k_dyn6 produces, recorded for tests/test_gpu_dyn6_pinned_bits.py -- needs the MI355X.

    T1ENV_DYN_KERNEL=6 python tests/golden/gen_dyn6_bits.py [--commit ID] [--out tests/golden/dyn6_bits.npz]

Run it inside a checkout of the commit whose results are the reference (its library carries that checkout's source
stamp), and only for a change that means to change what the env step computes: the test requires every recorded array
bit for bit.

Cases: 33 envs (one full workgroup and a ragged one-env one) and 97, on the plane and on the trimesh of
tests/test_gpu_dynamics.py's _terrain_hook.  Seed 6, the seeded 0.3 N(0, 1) actions of
tests/test_gpu_dyn6_core_stream.py, 6 policy steps with four-step episodes that start staggered, so envs reset; the
envs spawn at SPAWN_Z, where the feet land within an episode.  After
every step: root_states, dof_state, contact_vimp, rew_buf, reset_buf and the newest frame of obs_buf (its last 47
columns) and of privileged_obs_buf (its last 73), as raw uint32 so that NaN and -0.0 compare by bits.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dyn6_bits.npz")
CASES = [(33, "plane"), (33, "trimesh"), (97, "plane"), (97, "trimesh")]
STEPS = 6
# From the config's spawn height (1.1 m) the robot is in free fall for 17 policy steps and a four-step episode never
# touches the ground: every contact term would be zero.  At 0.95 m the feet reach the plane within the first steps of an
# episode (the fp32 host dynamics: none at 0.96 m, 1 env of 8 after one step and 4 after three at 0.95 m).
SPAWN_Z = 0.95
FIELDS = (("root_states", None), ("dof_state", None), ("contact_vimp", None), ("rew_buf", None), ("reset_buf", None),
          ("obs_buf", 47), ("privileged_obs_buf", 73))


def bits(t):
    """a tensor's values as uint32: the bit pattern of a float32, the value of anything else"""
    t = t.detach()
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32).copy()
    return t.to(torch.int64).cpu().numpy().astype(np.uint32)


def _terrain_hook(cfg):  # tests/test_gpu_dynamics.py
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 6, 4, 5


def replay(n, mesh):
    """-> ({"<field>": uint32 [STEPS, ...]}, number of resets, number of envs that were ever in contact)"""
    from ti5_isaacgym_amd import make_t1_env
    assert os.environ.get("T1ENV_DYN_KERNEL") == "6", "set T1ENV_DYN_KERNEL=6 before the env is made"

    def hook(cfg):
        if mesh != "plane":
            _terrain_hook(cfg)
        cfg.env.episode_length_s = 3.5 * cfg.control.decimation * cfg.sim.dt  # four policy steps
        cfg.init_state.pos = [0.0, 0.0, SPAWN_Z]
    env = make_t1_env(num_envs=n, mesh_type=mesh, seed=6, device="cuda:0", cfg_hook=hook)
    assert int(env.max_episode_length) == 4
    env.reset()
    env.episode_length_buf[:] = torch.arange(n, device="cuda:0", dtype=env.episode_length_buf.dtype) % 3
    g = torch.Generator(device="cuda:0").manual_seed(9)
    rec = {f: [] for f, _ in FIELDS}
    resets = 0
    touched = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    for _ in range(STEPS):
        env.step(0.3 * torch.randn(n, 12, device="cuda:0", generator=g))
        torch.cuda.synchronize()
        for f, last in FIELDS:
            x = getattr(env, f)
            rec[f].append(bits(x if last is None else x[:, -last:]))
        resets += int(env.reset_buf.sum())
        touched |= (env.contact_forces.reshape(n, -1) != 0).any(1) | (env.contact_vimp.reshape(n, -1) != 0).any(1)
    return {f: np.stack(v) for f, v in rec.items()}, resets, int(touched.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown", help="the commit the checkout is at, recorded in the file")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from ti5_isaacgym_amd import _lib
    out = {"commit": np.array(a.commit), "library": np.array(_lib.load().t1env_version().decode()),
           "command": np.array("T1ENV_DYN_KERNEL=6 python tests/golden/gen_dyn6_bits.py --commit " + a.commit)}
    for n, mesh in CASES:
        rec, resets, touched = replay(n, mesh)
        assert resets > 0 and touched > 0, (n, mesh, resets, touched)
        for f, v in rec.items():
            out[f"{n}_{mesh}_{f}"] = v
        print(f"{n} envs, {mesh}: {resets} resets, {touched} envs in contact")
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
