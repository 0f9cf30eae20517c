"""What the fused step's reward pass and reward state hold, recorded for tests/test_gpu_epilogue_deal.py -- needs the
MI355X.

    T1ENV_DYN_KERNEL=6 python tests/golden/gen_epilogue_bits.py [--commit ID] [--out tests/golden/epilogue_bits.npz]

Run it inside a checkout of the commit whose results are the reference, and only for a change that means to change
what the env step computes: the test requires every recorded word.

Cases as gen_dyn6_bits.py: 33 and 97 envs, plane and the small trimesh, envs spawned at 0.95 m, six policy steps of
seeded 0.3 N(0, 1) actions, four-step episodes that start staggered.  Two reward configurations: `default` (the config's
scales, only_positive_rewards on) and `all28` (tests/rewards28_util.cfg_hook: the four terms the config leaves at scale 0
live, only_positive_rewards off).  After every step, as raw uint32: rew_buf, _episode_sums, feet_air_time, feet_height,
last_feet_z, feet_euler_xyz, last_contacts, reset_buf and the extras["episode"] values (sorted by key).

Conditions on the inputs, asserted per case on the recording commit (the env seed is the first of SEEDS that meets them
and is stored in the file): an env reset; an env was in contact; all28: each of the four formerly dormant terms is
non-zero in some env; default: some env's unclipped reward sum was negative, so the clip acted.

Free fall from 0.95 m for four policy steps (0.04 s) brings no base to the ground, and on a plane a foot's friction
force never exceeds five times its normal force, so no seed makes an env terminate or stumble there.  Two groups of
envs are therefore put into a state that does, before the second step (no env of either group times out on it) and
again before the fifth: LYING envs are laid on the front edge of the base box, 6 mm into the ground
(tests/test_gpu_rewards28.py's _lay_down: ~1 kN on the base, a termination); CROSSED envs get a pair of opposite leg
joints turned against each other by 0.3 or 0.6 rad either way, joint velocities zeroed, so that in some of them the
legs' collision capsules overlap in the air and the feet are pushed sideways with next to no vertical force (a stumble).
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/: rewards28_util
sys.path.insert(0, HERE)
OUT = os.path.join(HERE, "epilogue_bits.npz")
CASES = [(33, "plane"), (33, "trimesh"), (97, "plane"), (97, "trimesh")]
CONFIGS = ("default", "all28")
STEPS = 6
SPAWN_Z = 0.95  # gen_dyn6_bits.py: the feet land within a four-step episode
SEEDS = (6, 7, 8, 9, 10, 11)
FIELDS = ("rew_buf", "_episode_sums", "feet_air_time", "feet_height", "last_feet_z", "feet_euler_xyz", "last_contacts",
          "reset_buf")
NEW_TERMS = ("dof_vel_limits", "feet_stumble", "stand_sysmetry", "termination")
OVERLAY_STEPS = (1, 4)
LYING = (2, 3, 4)  # episode steps 2, 0, 1 at the start: none at its last step when the overlay is applied
LYING_QUAT, LYING_Z = (0.0, -0.70710678, 0.0, 0.70710678), -0.012  # pitched -90 deg, the box edge 6 mm into the ground
# env -> (joint of the left leg, its angle; the right leg's joint of the same kind takes the opposite angle)
CROSSED = {8 + 4 * j + k: (j, a) for j in range(3) for k, a in enumerate((0.3, 0.6, -0.3, -0.6))}


def bits(t):
    """a tensor's values as uint32: the bit pattern of a float32, the value of anything else"""
    t = torch.as_tensor(t).detach()
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32).copy()
    return t.to(torch.int64).cpu().numpy().astype(np.uint32)


def _terrain_hook(cfg):  # tests/test_gpu_dynamics.py
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 6, 4, 5


def overlay(env):
    """put the LYING and CROSSED envs into their states (see the module's text)"""
    dev = env.root_states.device
    ids = torch.tensor(LYING, device=dev)
    r = env.root_states
    r[ids, 2] = env.env_origins[ids, 2] + LYING_Z
    r[ids, 3:7] = torch.tensor(LYING_QUAT, device=dev)
    r[ids, 7:13] = 0.0
    dof = env.dof_state.view(env.num_envs, 12, 2)
    dof[ids, :, 1] = 0.0
    env.contact_vimp[ids] = 0.0
    for e, (j, a) in CROSSED.items():
        dof[e, j, 0] += a
        dof[e, 6 + j, 0] -= a
        dof[e, :, 1] = 0.0


def replay(n, mesh, config, seed):
    """-> ({"<field>": uint32 [STEPS, ...]}, facts about the inputs: resets, envs in contact, ...)"""
    from ti5_isaacgym_amd import make_t1_env
    import rewards28_util
    assert os.environ.get("T1ENV_DYN_KERNEL") == "6", "set T1ENV_DYN_KERNEL=6 before the env is made"

    def hook(cfg):
        if mesh != "plane":
            _terrain_hook(cfg)
        cfg.env.episode_length_s = 3.5 * cfg.control.decimation * cfg.sim.dt  # four policy steps
        cfg.init_state.pos = [0.0, 0.0, SPAWN_Z]
        if config == "all28":
            rewards28_util.cfg_hook(cfg, dict(rewards28_util.SETTINGS, only_positive_rewards=False))
    env = make_t1_env(num_envs=n, mesh_type=mesh, seed=seed, device="cuda:0", cfg_hook=hook)
    assert int(env.max_episode_length) == 4
    env.reset()
    env.episode_length_buf[:] = torch.arange(n, device="cuda:0", dtype=env.episode_length_buf.dtype) % 3
    g = torch.Generator(device="cuda:0").manual_seed(9)
    rec = {f: [] for f in FIELDS + ("extras_episode",)}
    names = list(rewards28_util.REWARD_NAMES)
    facts = {"resets": 0, "clipped": 0, **{k: 0 for k in NEW_TERMS}}
    touched = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    for t in range(STEPS):
        if t in OVERLAY_STEPS:
            overlay(env)
        before = env._episode_sums.clone()
        env.step(0.3 * torch.randn(n, 12, device="cuda:0", generator=g))
        torch.cuda.synchronize()
        for f in FIELDS:
            rec[f].append(bits(getattr(env, f)))
        ep = env.extras["episode"]
        rec["extras_episode"].append(bits(torch.stack([torch.as_tensor(ep[k], dtype=torch.float32).reshape(()).cpu()
                                                       for k in sorted(ep)])))
        live = ~env.reset_buf.bool()
        facts["resets"] += int(env.reset_buf.sum())
        touched |= (env.contact_forces.reshape(n, -1) != 0).any(1) | (env.contact_vimp.reshape(n, -1) != 0).any(1)
        inc = env._episode_sums - before  # the step's scaled terms (rows of envs that did not reset)
        # the clip acted: a live env whose terms sum below zero is paid exactly zero
        facts["clipped"] += int((live & (inc.sum(0) < 0) & (env.rew_buf == 0)).sum())
        for k in NEW_TERMS:
            if k == "termination":  # paid to a resetting env only, whose sums the same step zeroes: it shows in rew_buf
                term = env.reset_buf.bool() & ~env.time_out_buf.bool()
                facts[k] += int(term.sum())
            else:
                facts[k] += int((live & (inc[names.index(k)] != 0)).sum())
    facts["touched"] = int(touched.sum())
    return {f: np.stack(v) for f, v in rec.items()}, facts


def inputs_ok(config, facts):
    ok = facts["resets"] > 0 and facts["touched"] > 0
    if config == "all28":
        return ok and all(facts[k] > 0 for k in NEW_TERMS)
    return ok and facts["clipped"] > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown", help="the commit the checkout is at, recorded in the file")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from ti5_isaacgym_amd import _lib
    out = {"commit": np.array(a.commit), "library": np.array(_lib.load().t1env_version().decode()),
           "command": np.array("T1ENV_DYN_KERNEL=6 python tests/golden/gen_epilogue_bits.py --commit " + a.commit)}
    for n, mesh in CASES:
        for config in CONFIGS:
            for seed in SEEDS:
                rec, facts = replay(n, mesh, config, seed)
                print(f"{n} envs, {mesh}, {config}, seed {seed}: {facts}", flush=True)
                if inputs_ok(config, facts):
                    break
            assert inputs_ok(config, facts), (n, mesh, config, facts)
            out[f"{n}_{mesh}_{config}_seed"] = np.array(seed)
            for f, v in rec.items():
                out[f"{n}_{mesh}_{config}_{f}"] = v
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
