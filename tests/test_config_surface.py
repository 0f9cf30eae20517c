"""The env's configuration surface: every cfg knob the reference reads on its step / reset / creation
path is either honoured by the HIP env and pinned by a golden scenario, or refused when the env is built.  No GPU needed.

  * a refused knob raises NotImplementedError naming it, before any device work (check_supported runs first in
    T1DHStandEnv.__init__, so the env can be asked for on the CPU device here, as tests/test_capi.py does);
  * the non-default golden scenarios (golden_util.CONFIG_SCENARIOS) meet their firing conditions on the committed
    fixtures: the reference's own outputs show the branch each scenario is there for;
  * the domain-randomisation state the oracle keeps (gains, offsets, joint friction, armature, lag lengths) equals the
    reference's in every scenario -- tests/test_oracle_golden.py sees it only through the torques and observations, and
    the product-kernel replays (tests/test_gpu_product_parity.py) compare the env's state with the oracle's.
"""
import numpy as np
import pytest

from golden_util import CONFIG_SCENARIOS, SCENARIOS, apply_overrides, assert_close, cfg_overrides, check_fired, load


def _set(path, value):
    return lambda cfg: apply_overrides(cfg, {path: value})


REFUSED = {
    "heading_command": _set("commands.heading_command", True),
    "sw_switch": _set("commands.sw_switch", False),
    "randomize_joint_friction": _set("domain_rand.randomize_joint_friction", True),
    "randomize_joint_damping": _set("domain_rand.randomize_joint_damping", True),
    "randomize_link_com": _set("domain_rand.randomize_link_com", True),
    "randomize_base_inertia": _set("domain_rand.randomize_base_inertia", True),
    "randomize_link_inertia": _set("domain_rand.randomize_link_inertia", True),
    "num_commands": _set("commands.num_commands", 5),
    "control_type": _set("control.control_type", "V"),
    "gait": _set("commands.gait", ["walk_omnidirectional", "stand", "trot"]),
    "3 gait slots": _set("commands.gait", ["walk_omnidirectional", "stand"]),
    "randomize_lag_timesteps_perstep": _set("domain_rand.randomize_lag_timesteps_perstep", True),
    "add_dof_pos_vel_lag": _set("domain_rand.add_dof_pos_vel_lag", True),
    "lag_timesteps_range": _set("domain_rand.lag_timesteps_range", [0, 40]),
    "decimation": _set("control.decimation", 4),          # with the lags on (DHT1StandCfg)
    "add_ext_force": lambda cfg: apply_overrides(cfg, {"domain_rand.add_ext_force": False,
                                                       "domain_rand.push_robots": True}),
    "use_ref_actions": _set("env.use_ref_actions", True),
    "ext_torque_max": _set("domain_rand.ext_torque_max", 2.0),
}


@pytest.mark.parametrize("knob", sorted(REFUSED))
def test_unsupported_knob_is_refused(knob):
    import ti5_isaacgym_amd as t
    with pytest.raises(NotImplementedError, match=knob):
        t.make_t1_env(num_envs=4, mesh_type="plane", device="cpu", cfg_hook=REFUSED[knob])


def test_supported_configurations_pass_the_check():
    """the default configuration and every golden scenario's overrides are accepted (the check refuses nothing it
    should honour); building the env itself needs the device and is tests/test_gpu_parity.py's part"""
    from ti5_isaacgym_amd.envs.configs import DHT1StandCfg
    from ti5_isaacgym_amd.envs.t1_env import check_supported
    check_supported(DHT1StandCfg())
    for name in CONFIG_SCENARIOS:
        check_supported(apply_overrides(DHT1StandCfg(), cfg_overrides(load(name))))


def test_overrides_name_existing_knobs():
    from ti5_isaacgym_amd.envs.configs import DHT1StandCfg
    with pytest.raises(AttributeError):
        apply_overrides(DHT1StandCfg(), {"commands.stand_threshold": 0.2})
    with pytest.raises(KeyError):
        apply_overrides(DHT1StandCfg(), {"commands.gait_time_range.trot": [1, 2]})
    cfg = apply_overrides(DHT1StandCfg(), {"commands.gait_time_range.rotate": [1, 2], "rewards.scales.torques": -1e-4})
    assert cfg.commands.gait_time_range["rotate"] == [1, 2] and cfg.rewards.scales.torques == -1e-4


@pytest.mark.parametrize("name", CONFIG_SCENARIOS)
def test_scenario_fired(name):
    fx = load(name)
    assert cfg_overrides(fx), "a configuration scenario without overrides"
    assert int(fx["num_envs"]) == 16 and fx["actions"].shape[0] == 10
    check_fired(name, fx)


@pytest.mark.parametrize("name", ["plane16", "drfixed16", "drranges16"])
def test_oracle_dr_state_matches_reference(name):
    from test_oracle_golden import run_oracle
    fx = load(name)
    assert name in SCENARIOS
    o, _ = run_oracle(fx)
    last = {k: fx["step_" + k][-1] for k in ("randomized_p_gains", "randomized_d_gains", "motor_offsets",
                                             "randomized_joint_coulomb", "randomized_joint_viscous", "joint_armatures",
                                             "lag_timestep", "dof_lag_timestep", "imu_lag_timestep")}
    assert_close("kp", o.kp_r, last["randomized_p_gains"])
    assert_close("kd", o.kd_r, last["randomized_d_gains"])
    assert_close("motor_offsets", o.motor_offsets, last["motor_offsets"])
    assert_close("joint_coulomb", o.coulomb, last["randomized_joint_coulomb"])
    assert_close("joint_viscous", o.viscous, last["randomized_joint_viscous"])
    assert_close("armature", o.armature, last["joint_armatures"])
    np.testing.assert_array_equal(o.lag_timestep, last["lag_timestep"])
    np.testing.assert_array_equal(o.dof_lag_timestep, last["dof_lag_timestep"])
    np.testing.assert_array_equal(o.imu_lag_timestep, last["imu_lag_timestep"])
    assert_close("link_masses", o.link_mass_scale, fx["init_link_masses"].reshape(-1, 12))
    assert_close("com_displacements", o.com_disp, fx["init_com_displacements"])
    assert_close("restitution", o.restitution, fx["init_restitution"].reshape(-1))
