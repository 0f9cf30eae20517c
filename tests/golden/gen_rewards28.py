"""Generate tests/golden/rewards28_16.npz: the reference's own env code (as gen_golden.py runs it, behind the isaacgym
stand-in) with the four reward terms DHT1StandCfg leaves at scale 0 switched on.

    python tests/golden/gen_rewards28.py

16 envs x 10 steps on the plane; the scenario and the synthetic physics with stumbling feet are tests/rewards28_util.py.
gen_golden.run asserts the 24 default terms, so the run is restated here for the 28 (termination has an episode sum but is
not in the reference's reward_names, legged_robot.py:366-371).
"""
import json
import os

import numpy as np

import gen_golden as G   # sets up the paths of the reference and the harness
import torch

import rewards28_util as R28

HERE = os.path.dirname(os.path.abspath(__file__))
NAME, NUM_ENVS, N_STEPS = "rewards28_16", 16, 10


def make_provider(env, num_envs, seed):
    def provider(tensors, g):
        root, dof, rigid, contact = R28.state(seed, num_envs, g, G._np(env.env_origins))
        tensors["root"][:] = torch.from_numpy(root)
        tensors["dof"][:] = torch.from_numpy(dof.reshape(num_envs * 12, 2))
        tensors["rigid"][:] = torch.from_numpy(rigid.reshape(num_envs * 13, 13))
        tensors["contact"][:] = torch.from_numpy(contact.reshape(num_envs * 13, 3))
    return provider


def snapshot(env, gym):
    s = G.snapshot_cfg(env, gym)
    s["episode_sums"] = np.stack([G._np(env.episode_sums[k]) for k in R28.REWARD_NAMES])
    return s


def run():
    n = NUM_ENVS
    env, cfg, gym = G.refenv.make_env(n, "plane", R28.cfg_hook)
    assert sorted(list(env.reward_names) + ["termination"]) == R28.REWARD_NAMES, env.reward_names
    assert sorted(env.episode_sums) == R28.REWARD_NAMES
    gym.provider = make_provider(env, n, G.SYNTH_SEED)
    out = {"num_envs": np.int64(n), "synth_seed": np.int64(G.SYNTH_SEED), "seed": np.int64(cfg.seed),
           "mesh_type": np.array("plane"), "cfg_rewards28": np.array(json.dumps(R28.SETTINGS, sort_keys=True)),
           "dt": np.float64(env.dt), "max_episode_length": np.float64(env.max_episode_length),
           "init_dof_vel_limits": G._np(env.dof_vel_limits), "init_env_origins": G._np(env.env_origins)}
    env.reset()
    rec = [dict(snapshot(env, gym), obs=G._np(env.obs_buf), priv=G._np(env.privileged_obs_buf), rew=G._np(env.rew_buf),
                reset=G._np(env.reset_buf), time_out=G._np(env.time_out_buf))]
    # walk -> stand in 2 steps (envs 0-4), stand -> walk in 3 (5, 8), time-outs at steps 4 (6, 7) and 7 (every 5th env)
    over = G._events(slot1=[(slice(0, 5), 2)], slot2=[([5, 8], 3)], time_out=[([6, 7], 4), ([9, 14], 7)])(env)
    out["override_episode_length_buf"] = G._np(over["episode_length_buf"])
    gen = np.random.default_rng(2828)
    actions = (0.5 * gen.standard_normal((N_STEPS, n, 12))).astype(np.float32)
    out["actions"] = actions
    for t in range(N_STEPS):
        env.step(torch.from_numpy(actions[t]).clone())
        ep = env.extras.get("episode", {})
        rec.append(dict(snapshot(env, gym), obs=G._np(env.obs_buf), priv=G._np(env.privileged_obs_buf),
                        rew=G._np(env.rew_buf), reset=G._np(env.reset_buf), time_out=G._np(env.time_out_buf),
                        extras_episode=np.array([float(ep.get("rew_" + k, np.nan)) for k in R28.REWARD_NAMES],
                                                np.float32)))
    keep = ["obs", "priv", "rew", "reset", "time_out", "episode_sums", "extras_episode", "commands", "episode_length_buf",
            "feet_air_time", "feet_height", "gait_time"]
    for k in keep:
        vals = [r.get(k) for r in rec]
        if vals[0] is None:
            vals[0] = np.zeros_like(vals[1])
        arr = np.stack([np.asarray(v) for v in vals])
        if k == "obs":   # the newest actor frame of every step
            arr = arr[:, :, -47:]
        out["step_" + k] = arr
    out["final_dof_vel_limits"] = G._np(env.dof_vel_limits)   # the reward function overwrote joints 4 and 9
    R28.check_fired(out)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    term = out["step_reset"].astype(bool) & ~out["step_time_out"].astype(bool)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB; resets per step {out['step_reset'].sum(1).tolist()}, "
          f"terminations {term.sum(1).tolist()}")
    return out


if __name__ == "__main__":
    run()
