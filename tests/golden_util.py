"""Helpers shared by the parity tests: load a golden fixture and drive an env through the same inputs."""
import json
import os

import numpy as np

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENARIOS = ["plane16", "events16", "config1_64", "trimesh16", "heights16", "resetidx16", "push16", "trimesh_nocurr16"]
# the non-default configurations (tests/golden/gen_golden.py CONFIG_SCENARIOS): their settings travel in the fixture as
# a flat dict, dotted cfg path -> value (key cfg_overrides, a JSON string)
CONFIG_SCENARIOS = ["gaits16", "gaits_stand_first16", "rewards16", "obs16", "nonoise16", "drfixed16", "drranges16",
                    "decim4_16"]
SCENARIOS = SCENARIOS + CONFIG_SCENARIOS


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: d[k] for k in d.files}


def cfg_overrides(fx):
    """the scenario's config overrides ({} for the default-configuration scenarios)"""
    return json.loads(str(fx["cfg_overrides"])) if "cfg_overrides" in fx else {}


def apply_overrides(cfg, overrides):
    """Set every dotted path of `overrides` on a config object (the reference's cfg classes and the HIP env's restatement
    share their attribute names).  A path that runs into a dict (commands.gait_time_range.<gait>) sets the item.  Every
    path but its last component must exist, so a misspelt knob raises."""
    for path, value in overrides.items():
        *head, last = path.split(".")
        obj = cfg
        for name in head:
            nxt = obj[name] if isinstance(obj, dict) else getattr(obj, name)
            if isinstance(nxt, dict):   # a dict is a class attribute shared by every cfg instance: set it on a copy
                nxt = dict(nxt)
                if isinstance(obj, dict):
                    obj[name] = nxt
                else:
                    setattr(obj, name, nxt)
            obj = nxt
        if isinstance(obj, dict):
            if last not in obj:
                raise KeyError(path)
            obj[last] = value
        else:
            if not hasattr(obj, last):
                raise AttributeError(path)
            setattr(obj, last, value)
    return cfg


def terrain_of(fx):
    if str(fx["mesh_type"]) in ("trimesh", "heightfield"):
        t = {"terrain_origins": fx["init_terrain_origins"], "height_samples": fx["init_height_samples"]}
        if "init_terrain_scales" in fx:   # the height-scan scenario: the scan needs the field's geometry
            hs, vs, border = (float(x) for x in fx["init_terrain_scales"])
            t.update(horizontal_scale=hs, vertical_scale=vs, border_size=border)
        return t
    return None


def mid_reset(fx, t):
    """env ids the reference's reset_idx was called on between step t and t + 1 (scenario resetidx16), or None"""
    if "mid_reset_step" in fx and int(fx["mid_reset_step"]) == t:
        return fx["mid_reset_ids"]
    return None


def push_interval_s(fx):
    """push_robots scenario (push16): the scenario's push_interval_s, else None (push_robots off, the default)"""
    return float(fx["cfg_push_interval_s"]) if "cfg_push_interval_s" in fx else None


def terrain_curriculum(fx):
    """cfg.terrain.curriculum of the scenario (on unless the fixture says otherwise: trimesh_nocurr16)"""
    return bool(int(fx["cfg_terrain_curriculum"])) if "cfg_terrain_curriculum" in fx else True


def measures_heights(fx):
    return "step_measured_heights" in fx


def synth_physics(fx):
    seed = int(fx["synth_seed"])
    n = int(fx["num_envs"])

    def physics(g, torques, env):
        root, dof, rigid, contact = synth.state(seed, n, g, np.asarray(env.env_origins))
        return root, dof, rigid, contact
    return physics


# Parity tolerance (north_star: 1e-4 relative, fp32).  The absolute floor is 1e-6: the smallest per-term reward
# values (episode sums of dof_vel / torques, median ~1e-4) are then checked to ~1%, and a term that a bug zeroed
# fails.  Measured worst floors needed at rtol 1e-4: oracle vs reference 3.8e-7 (one obs element); HIP vs reference /
# oracle are recorded per field by WORST below (tests write them to $T1_PARITY_REPORT).
RTOL, ATOL = 1e-4, 1e-6
# field -> [worst |got - ref| - rtol |ref| (the absolute floor the field needed), worst |got - ref|, max |ref|]
WORST = {}


def _record(name, got, ref, rtol):
    if got.size == 0:
        return
    err = np.abs(got - ref)
    fin = np.isfinite(err)
    if not fin.any():
        return
    need = float(np.max((err - rtol * np.abs(ref))[fin]))
    w = WORST.setdefault(name, [-np.inf, 0.0, 0.0])
    w[0] = max(w[0], need)
    w[1] = max(w[1], float(err[fin].max()))
    w[2] = max(w[2], float(np.abs(ref[np.isfinite(ref)]).max(initial=0.0)))


# T1 torque limits x 0.85, left then right leg
TORQUE_MAX = np.array([86.7, 86.7, 226.95, 226.95, 68.0, 34.0, 86.7, 86.7, 226.95, 226.95, 68.0, 34.17])


def torque_atol():
    """Per-joint absolute floor for torques: tau = Kp (a_lag + q0 - q + off) - Kd qd - visc qd - coul sign(qd), times the
    multiplier, is a difference of terms up to the joint's torque limit, so a torque near zero carries the fp32 rounding of
    those terms (the HIP kernel contracts them into FMAs, numpy rounds every product): 2e-7 x the limit (~3.4 ulp of
    the limit; measured need 3.3e-6 on a 68 N m joint, r03a)."""
    return 2e-7 * TORQUE_MAX


def assert_close_nan(name, got, ref, **kw):
    """assert_close where the reference omits entries (NaN: a reward term with a zero scale is in neither the
    reference's episode_sums nor its extras["episode"]): `got` must omit exactly those, the rest is compared."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{name}{kw.get('ctx', '')}: shape {got.shape} vs {ref.shape}"
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{name}{kw.get('ctx', '')}: omitted entries")
    keep = ~np.isnan(ref)
    assert_close(name, got[keep], ref[keep], **kw)


def assert_close(name, got, ref, rtol=RTOL, atol=ATOL, ctx=""):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{name}{ctx}: shape {got.shape} vs {ref.shape}"
    _record(name, got, ref, rtol)
    bad = ~np.isclose(got, ref, rtol=rtol, atol=atol)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        msg = ", ".join(f"{tuple(i)}: {got[tuple(i)]:.7g} vs {ref[tuple(i)]:.7g}" for i in idx)
        raise AssertionError(f"{name}{ctx}: {bad.sum()} mismatches: {msg}")


# ---- the non-default scenarios must exercise their branch ---------------------------------------------------------
# Conditions on the reference's own outputs, asserted by gen_golden.py when it writes a fixture and again on the
# committed fixture by tests/test_config_surface.py, so no scenario passes without reaching the code it is there for.
REWARD_NAMES = sorted(["joint_pos", "feet_clearance", "feet_contact_number", "feet_air_time", "foot_slip",
                       "feet_distance", "knee_distance", "feet_rotation", "feet_contact_forces",
                       "tracking_lin_vel", "tracking_ang_vel", "vel_mismatch_exp", "low_speed",
                       "track_vel_hard", "default_joint_pos", "orientation", "base_height", "base_acc",
                       "action_smoothness", "torques", "dof_vel", "dof_acc", "collision", "stand_still"])


def _resampled(fx, slot):
    """(step, env) pairs at which gait slot `slot` redrew the command: the episode step equals the slot's start"""
    el, gt = fx["step_episode_length_buf"], fx["step_gait_time"]
    return np.argwhere(el[1:] == gt[1:, :, slot]) + [1, 0]


def _cmd_norm(fx):
    return np.linalg.norm(fx["step_commands"][:, :, :3], axis=2)


def _standing_obs(fx):
    """envs whose newest actor frame shows the held phase of a standing env: sin = 0, cos = 1 (t1_dh_stand_env.py:80-92)"""
    o = fx["step_obs"]
    return (o[:, :, 0] == 0.0) & (o[:, :, 1] == 1.0)


def _stand_to_walk(fx, thr):
    n = _cmd_norm(fx)
    return (n[:-1] <= thr) & (n[1:] > thr) & ~fx["step_reset"][1:].astype(bool)


def _fired_gaits16(fx):
    gait = cfg_overrides(fx)["commands.gait"]
    comp = {"walk_sagittal": 0, "walk_lateral": 1, "rotate": 2}
    assert sorted(gait) == sorted(comp), gait
    for slot, kind in enumerate(gait):
        at = _resampled(fx, slot)
        assert len(set(at[:, 1])) >= 2, f"{kind}: resampled in {len(set(at[:, 1]))} envs"
        cmd = fx["step_commands"][at[:, 0], at[:, 1], :3]
        want = np.zeros(3, bool)
        want[comp[kind]] = True
        assert ((cmd != 0) == want).all(), f"{kind}: components {cmd}"


def _fired_gaits_stand_first16(fx):
    thr = cfg_overrides(fx)["commands.stand_com_threshold"]
    n = _cmd_norm(fx)
    assert int(((n[0] == 0) & _standing_obs(fx)[0]).sum()) >= 2, "no env stands from step 0 with its phase held"
    assert ((n > 0) & (n <= thr) & _standing_obs(fx)).any(), "no non-zero command below the threshold counted as standing"
    assert _stand_to_walk(fx, thr).any(), "no stand -> walk transition"


def _fired_rewards16(fx):
    ov = cfg_overrides(fx)
    assert fx["step_rew"].min() < 0, "no negative reward"
    zero = [k for k in REWARD_NAMES if ov.get("rewards.scales." + k, 1) == 0]
    assert sorted(zero) == ["collision", "dof_acc", "feet_air_time"], zero
    ep = fx["step_extras_episode"][1:]
    for i, k in enumerate(REWARD_NAMES):
        if k in zero:
            assert np.isnan(ep[:, i]).all(), f"{k}: zero scale but reported"
            assert np.isnan(fx["step_episode_sums"][:, i]).all(), k
        else:
            assert np.isfinite(ep[:, i]).all(), k
            assert (fx["step_episode_sums"][:, i] != 0).any(), f"{k}: zero in every env-step"


def _fired_obs16(fx):
    ov = cfg_overrides(fx)
    clip = ov["normalization.clip_observations"]
    for k in ("step_obs", "step_priv"):
        frac = float(np.mean(np.abs(fx[k][1:]) == clip))
        assert frac >= 0.01, f"{k}: {frac:.4f} of the elements at the clip"
    frac = float(np.mean(np.abs(fx["actions"]) > ov["normalization.clip_actions"]))
    assert frac >= 0.10, f"actions: {frac:.3f} beyond clip_actions"


def _fired_nonoise16(fx):
    assert cfg_overrides(fx)["noise.add_noise"] is False


def _fired_drfixed16(fx):
    ov = cfg_overrides(fx)
    assert ov["domain_rand.lag_timesteps_range"][1] == 12 and (fx["step_lag_timestep"] == 12).all()
    assert ov["domain_rand.imu_lag_timesteps_range"][1] == 4 and (fx["step_imu_lag_timestep"] == 4).all()
    assert (fx["step_dof_lag_timestep"] == 0).all()
    assert (fx["step_randomized_p_gains"] == fx["init_p_gains"]).all()
    assert (fx["step_randomized_d_gains"] == fx["init_d_gains"]).all()
    assert (fx["init_env_frictions"] == 0).all() and len(np.unique(fx["init_body_mass"])) == 1
    assert (fx["init_com_displacements"] == 0).all() and (fx["init_link_masses"] == 1).all()
    assert (fx["step_joint_armatures"] == 0).all() and (fx["step_motor_offsets"] == 0).all()
    assert fx["step_reset"][1:].any(), "no reset: the un-lagged joint observation of a reset env is not exercised"


def _fired_drranges16(fx):
    ov = cfg_overrides(fx)
    arm = fx["step_joint_armatures"][1:]
    assert (arm == arm[:, :, :1]).all() and (arm > 0).all(), "the 12 armatures of an env differ"
    assert len(np.unique(arm[:, :, 0])) > 1, "armature equal over the envs"
    for key, rng in (("step_lag_timestep", "lag_timesteps_range"), ("step_dof_lag_timestep", "dof_lag_timesteps_range"),
                     ("step_imu_lag_timestep", "imu_lag_timesteps_range")):
        lo, hi = ov["domain_rand." + rng]
        v = fx[key]
        assert v.min() == lo and v.max() == hi, f"{key}: [{v.min()}, {v.max()}] of [{lo}, {hi}]"
    assert float(fx["max_episode_length"]) == 1200
    assert fx["step_time_out"][1:].any(), "no time-out"
    assert np.abs(fx["step_applied_force"]).max() > 0, "no force applied"


def _fired_decim4_16(fx):
    assert float(fx["max_episode_length"]) == 6000
    assert fx["step_torques"].shape[1] == 4
    thr = 0.05
    n = _cmd_norm(fx)
    moved = ((n[:-1] <= thr) != (n[1:] <= thr)) & ~fx["step_reset"][1:].astype(bool)
    assert moved.any(), "no gait-slot transition"


FIRED = {"gaits16": _fired_gaits16, "gaits_stand_first16": _fired_gaits_stand_first16, "rewards16": _fired_rewards16,
         "obs16": _fired_obs16, "nonoise16": _fired_nonoise16, "drfixed16": _fired_drfixed16,
         "drranges16": _fired_drranges16, "decim4_16": _fired_decim4_16}


def check_fired(name, fx):
    FIRED[name](fx)
