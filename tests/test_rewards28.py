"""The four reward terms DHT1StandCfg leaves at scale 0 (dof_vel_limits, feet_stumble, stand_sysmetry, termination), the
parts that need no GPU: the env accepts them, the C ABI and its ctypes mirror grew together, and the committed fixture
tests/golden/rewards28_16.npz reaches every new branch."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rewards28_util as R28
from golden_util import load

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(hook):
    import ti5_isaacgym_amd as t
    return t.make_t1_env(num_envs=4, mesh_type="plane", device="cpu", cfg_hook=hook)


@pytest.mark.parametrize("name", R28.NEW_TERMS)
def test_env_accepts_the_dormant_terms(name):
    """A scale on one of the four terms no longer stops at "reward terms without a HIP kernel": construction gets as
    far as the device check (the env runs on the HIP device only)."""
    def hook(cfg):
        setattr(cfg.rewards.scales, name, -1.0)
        cfg.rewards.soft_dof_vel_limit = 0.9
    with pytest.raises(RuntimeError, match="HIP device only") as e:
        _make(hook)
    assert not isinstance(e.value, NotImplementedError)


def test_env_still_refuses_a_term_without_a_kernel():
    def hook(cfg):
        cfg.rewards.scales.action_rate = -0.01
        cfg.rewards.scales.termination = -1.0
    with pytest.raises(NotImplementedError, match=r"without a HIP kernel: \['action_rate'\]"):
        _make(hook)


def test_dof_vel_limits_needs_its_soft_limit():
    """Neither reference config defines rewards.soft_dof_vel_limit and the reference's reward function raises
    AttributeError without it (t1_dh_stand_env.py:946): so does the env, naming the knob, with no default."""
    def hook(cfg):
        assert not hasattr(cfg.rewards, "soft_dof_vel_limit")
        cfg.rewards.scales.dof_vel_limits = -1.0
    with pytest.raises(AttributeError, match="soft_dof_vel_limit"):
        _make(hook)

    def zero(cfg):   # a zero scale switches the term off: nothing to require
        cfg.rewards.scales.dof_vel_limits = 0.0
    with pytest.raises(RuntimeError, match="HIP device only"):
        _make(zero)


def test_reward_index_space_and_struct_layout_match_the_header():
    from ti5_isaacgym_amd import _lib
    from ti5_isaacgym_amd.envs.t1_env import REWARD_NAMES
    assert _lib.NREW == 28 and REWARD_NAMES == R28.REWARD_NAMES
    enum = ", ".join("T1_REW_" + k.upper() for k in REWARD_NAMES)
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "t1env.h"
int main(void) {
  const int idx[] = {%s};
  printf("%%d %%d %%d %%d\n", T1_NREW, T1_EX_TERRAIN_LEVEL, T1_ACC_COUNT, T1_ACC_LEVEL);
  printf("%%zu %%zu %%zu %%zu %%zu %%zu\n", sizeof(t1env_config), offsetof(t1env_config, reward_scales),
         offsetof(t1env_config, only_positive_rewards), offsetof(t1env_config, max_contact_force),
         offsetof(t1env_config, soft_dof_vel_limit), offsetof(t1env_config, gait_time_range));
  for (size_t i = 0; i < sizeof(idx) / sizeof(idx[0]); ++i) printf("%%d\n", idx[i]);
  return 0;
}
''' % enum
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "r28.c")
        with open(c, "w") as f:
            f.write(prog)
        exe = os.path.join(d, "r28")
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    assert out[:4] == [28, _lib.EX_TERRAIN_LEVEL, _lib.ACC_COUNT, _lib.ACC_LEVEL] and _lib.ACC_LEVEL < 32
    C = _lib.Config
    assert out[4:10] == [ctypes.sizeof(C), C.reward_scales.offset, C.only_positive_rewards.offset,
                         C.max_contact_force.offset, C.soft_dof_vel_limit.offset, C.gait_time_range.offset]
    assert C.reward_scales.size == 28 * 4
    assert out[10:] == list(range(28))   # the header's named indices are the alphabetical order of the Python names


def test_fixture_reaches_every_new_branch():
    fx = load("rewards28_16")
    assert fx["step_rew"].shape == (11, 16) and str(fx["mesh_type"]) == "plane"
    R28.check_fired(fx)


def test_fixture_velocity_limits_are_the_envs():
    """The reference's reward overwrites its dof_vel_limits[[4, 9]] on every call; here that is the reward's alone, and
    the model's limits (env.dof_vel_limits, which also bound the dynamics) stay what the reference started with."""
    from ti5_isaacgym_amd.envs.t1_env import build_model
    from ti5_isaacgym_amd.utils.task_registry import task_registry
    cfg, _ = task_registry.get_cfgs("t1_dh_stand")
    m = build_model(cfg)[0]
    np.testing.assert_array_equal(np.array([m.vel_limit[j] for j in range(12)], np.float32),
                                  load("rewards28_16")["init_dof_vel_limits"])
