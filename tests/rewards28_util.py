"""Shared by the generator and the tests of the four reward terms DHT1StandCfg leaves at scale 0 (dof_vel_limits,
feet_stumble, stand_sysmetry, termination): the scenario's settings, the synthetic physics with stumbling feet, and the
conditions the fixture tests/golden/rewards28_16.npz must meet so that every new branch is exercised."""
import json

import numpy as np

import synth
from golden_util import apply_overrides

NEW_TERMS = ["dof_vel_limits", "feet_stumble", "stand_sysmetry", "termination"]
REWARD_NAMES = sorted(["joint_pos", "feet_clearance", "feet_contact_number", "feet_air_time", "foot_slip",
                       "feet_distance", "knee_distance", "feet_rotation", "feet_contact_forces",
                       "tracking_lin_vel", "tracking_ang_vel", "vel_mismatch_exp", "low_speed",
                       "track_vel_hard", "default_joint_pos", "orientation", "base_height", "base_acc",
                       "action_smoothness", "torques", "dof_vel", "dof_acc", "collision", "stand_still"] + NEW_TERMS)

# The scenario.  synth.state draws dof_vel = 2 N(0, 1) and the T1 velocity limits are 9.85 .. 11.7 rad/s (10 for joints
# 4 and 9 inside the reward), so with soft_dof_vel_limit = 0.17 the penalty starts at |dof_vel| = 1.67 .. 2.0: about 63 %
# of the joint samples lie below it, 21 % inside the (0, 1) band and 16 % are clipped at 1.
SCALES = {"dof_vel_limits": -0.5, "feet_stumble": -2.0, "stand_sysmetry": 1.0, "termination": -5.0}
SOFT_DOF_VEL_LIMIT = 0.17
SETTINGS = {"scales": SCALES, "soft_dof_vel_limit": SOFT_DOF_VEL_LIMIT, "only_positive_rewards": True,
            "gait": ["walk_omnidirectional", "stand", "walk_omnidirectional"]}


def cfg_hook(cfg, settings=SETTINGS):
    """Set the scenario on a cfg (the reference's or the HIP env's).  Neither config defines the four scales nor
    soft_dof_vel_limit, so they are plain attribute assignments; the knobs that exist go through apply_overrides."""
    apply_overrides(cfg, {"rewards.only_positive_rewards": settings["only_positive_rewards"],
                          "commands.gait": list(settings["gait"])})
    for k, v in settings["scales"].items():
        setattr(cfg.rewards.scales, k, v)
    cfg.rewards.soft_dof_vel_limit = settings["soft_dof_vel_limit"]


def settings_of(fx):
    return json.loads(str(fx["cfg_rewards28"]))


# ---- synthetic physics: synth.state never makes a foot stumble (|f_xy| ~ 40 N against f_z >= 350 N, or 0 against
# <= 8 N), so foot contact forces are overlaid on a fixed subset of envs and steps: |f_xy| / |f_z| = 8 (a stumble, the
# threshold is 5) or 3 (none).  A negative f_z exercises the |f_z| of the reference.
STUMBLE = {2: (6, (480.0, 640.0, 100.0)), 6: (12, (-320.0, 240.0, -50.0)), 10: (6, (48.0, -64.0, 10.0))}   # ratio 8
NO_STUMBLE = {3: (6, (180.0, 240.0, 100.0)), 7: (12, (90.0, -120.0, -50.0))}                              # ratio 3


def overlaid(step):
    """the overlay is on in every second env step (counted from the first simulate() call)"""
    return step % 2 == 1


def state(seed, num_envs, g, origins=None, env_offset=0, substeps=10):
    root, dof, rigid, contact = synth.state(seed, num_envs, g, origins, env_offset)
    if overlaid(g // substeps):
        for table in (STUMBLE, NO_STUMBLE):
            for e, (body, f) in table.items():
                if env_offset <= e < env_offset + num_envs:
                    contact[e - env_offset, body] = np.asarray(f, np.float32)
    return root, dof, rigid, contact


class Injector:
    """parity_driver.Injector on the overlaid states: the t1env_injected struct of one env step"""

    def __init__(self, env, seed):
        self.env, self.seed, self.g = env, seed, 0

    def next(self):
        import torch
        from ti5_isaacgym_amd import _lib
        env = self.env
        n = env.num_envs
        origins = env.env_origins.cpu().numpy()
        dec = int(env.cfg.control.decimation)
        roots, dofs = [], []
        for s in range(dec):
            r, d, rig, con = state(self.seed, n, self.g + s, origins, substeps=dec)
            roots.append(r)
            dofs.append(d)
        self.g += dec
        dev = env.device
        self._keep = [torch.from_numpy(np.stack(roots)).to(dev), torch.from_numpy(np.stack(dofs)).to(dev),
                      torch.from_numpy(rig).to(dev), torch.from_numpy(con).to(dev), torch.zeros(dec, n, 12, device=dev)]
        inj = _lib.Injected()
        inj.root, inj.dof, inj.rigid, inj.contact, inj.torque_log = [_lib.C.cast(t.data_ptr(), _lib.fp)
                                                                     for t in self._keep]
        return inj


# ---- the fixture must reach every new branch (asserted when it is written and again on the committed file)
def check_fired(fx):
    s = settings_of(fx)
    assert s == json.loads(json.dumps(SETTINGS)), "the fixture was written with other settings than SETTINGS"
    assert all(s["scales"][k] != 0 for k in NEW_TERMS) and s["scales"]["termination"] < 0
    assert s["only_positive_rewards"] is True and "stand" in s["gait"]
    sums, reset, tout = fx["step_episode_sums"], fx["step_reset"].astype(bool), fx["step_time_out"].astype(bool)
    rew, dt = fx["step_rew"], float(fx["dt"])
    idx = {k: REWARD_NAMES.index(k) for k in NEW_TERMS}
    assert sums.shape[1] == 28 and np.isfinite(sums).all()
    for k, i in idx.items():
        if k != "termination":   # only a resetting env is paid it, and its reset zeroes the sum within the same step:
            assert (sums[:, i] != 0).any(), f"{k}: its episode sum never changes"   # that row shows in the extras (below)
    # termination: after the clip -- a negative reward although only_positive_rewards is on
    term = reset & ~tout
    assert term[1:].any(), "no env terminates"
    assert (rew[term] < 0).any() and (rew[~term] >= 0).all(), "termination does not show below the clip"
    assert rew.min() >= np.float32(s["scales"]["termination"] * dt), "more than the termination term below the clip"
    assert tout[1:].any(), "no env times out"
    assert (rew[tout] >= 0).all(), "a time-out was penalised as a termination"
    ep = fx["step_extras_episode"][1:]
    assert (ep[:, idx["termination"]] < 0).any(), "rew_termination never reported below 0"
    # feet_stumble: 1 in some envs and 0 in others on the same step
    w = s["scales"]["feet_stumble"] * dt
    inc = np.diff(sums[:, idx["feet_stumble"]], axis=0)
    live = ~reset[1:]
    both = [(np.isclose(inc[t][live[t]], w).any() and (inc[t][live[t]] == 0).any()) for t in range(len(inc))]
    assert any(both), "no step with stumbling and non-stumbling envs"
    hit = np.isclose(inc, w) & live
    steps = np.arange(1, len(sums))[:, None] + 0 * hit
    assert hit.any() and all(overlaid(t) for t in steps[hit]), "a stumble outside the overlaid steps"
    assert set(np.argwhere(hit)[:, 1]) <= set(STUMBLE), "a stumble in an env without the ratio-8 overlay"
    # stand_sysmetry: non-zero only for standing envs (a standing env's newest actor frame holds sin = 0, cos = 1)
    stand = (fx["step_obs"][:, :, 0] == 0.0) & (fx["step_obs"][:, :, 1] == 1.0)
    inc = np.diff(sums[:, idx["stand_sysmetry"]], axis=0)
    moved = (inc != 0) & live
    cmd_stand = np.linalg.norm(fx["step_commands"][1:, :, :3], axis=2) <= 0.05
    assert moved.any() and (cmd_stand[moved]).all(), "stand_sysmetry paid to a walking env"
    assert (moved[cmd_stand & live]).all() and stand[1:][moved].all(), "a standing env without stand_sysmetry"
    # dof_vel_limits: all three kinds of joints (checked on the injected velocities themselves)
    lim = fx["init_dof_vel_limits"].astype(np.float64).copy()
    lim[[4, 9]] = 10.0
    n, seed = int(fx["num_envs"]), int(fx["synth_seed"])
    vel = np.stack([state(seed, n, 10 * t + 9)[1][:, :, 1] for t in range(len(sums))])   # each step's last substep
    v = np.abs(vel.astype(np.float64)) - lim * s["soft_dof_vel_limit"]
    frac = [float(np.mean(v < 0)), float(np.mean((v > 0) & (v < 1))), float(np.mean(v > 1))]
    assert min(frac) > 0.05, f"dof_vel_limits: below / band / clipped fractions {frac}"
    # the limits the reward overrides (joints 4 and 9) are the reward's alone
    assert (fx["final_dof_vel_limits"][[4, 9]] == 10).all() and (fx["init_dof_vel_limits"][[4, 9]] != 10).all()
    keep = [j for j in range(12) if j not in (4, 9)]
    np.testing.assert_array_equal(fx["final_dof_vel_limits"][keep], fx["init_dof_vel_limits"][keep])
