"""k_dyn6's reward pass dealt over the waves that idle in the epilogue -- needs the MI355X.

After the epilogue barrier the rewards wave (W0) evaluates only the terms that advance state or read the feet's Euler
angles; W4-W7 evaluate the other terms, write each unscaled r[k] into a row in LDS and count themselves in; W0 waits
for the count, then runs the ordered sum, the clip, the episode sums and every store as before.  The state wave's
reset_idx past the terrain curriculum runs with all 64 lanes on one resetting env at a time.  No result may move:

* tests/golden/epilogue_bits.npz holds rew_buf, the episode sums, the reward state (feet_air_time, feet_height,
  last_feet_z, feet_euler_xyz, last_contacts), reset_buf and the extras["episode"] values after each of six steps, as
  the commit before the deal wrote them (tests/golden/gen_epilogue_bits.py: 33 and 97 envs, plane and trimesh, the
  default scales and all 28 terms live without the clip; a few envs laid on the base box or with their legs crossed so
  that terminations and stumbles occur).  The replay equals every word.
* With all 28 terms live and forced resets (none, one, the workgroup corners, all; as tests/test_gpu_reset_tail.py), the
  fused step equals the split kernel sequence, whose one-wave reward pass and one-lane reset are untouched, on
  test_gpu_fused.py's EXACT / CLOSE lists and on everything reset_idx writes.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import rewards28_util
from test_gpu_fused import CLOSE, EXACT, _sync
from test_gpu_reset_tail import RESET_EXACT, RESET_SETS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_epilogue_bits", os.path.join(GOLDEN, "gen_epilogue_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "epilogue_bits.npz"))


@pytest.mark.parametrize("config", ["default", "all28"])
@pytest.mark.parametrize("mesh", ["plane", "trimesh"])
@pytest.mark.parametrize("n", [33, 97])
def test_replay_equals_the_recorded_bits(n, mesh, config, golden, monkeypatch):
    monkeypatch.setenv("T1ENV_DYN_KERNEL", "6")
    gen = _gen()
    assert (n, mesh) in gen.CASES and config in gen.CONFIGS
    rec, facts = gen.replay(n, mesh, config, int(golden[f"{n}_{mesh}_{config}_seed"]))
    assert gen.inputs_ok(config, facts), f"the inputs do not reach every branch: {facts}"
    bad = []
    for f in rec:
        want, got = golden[f"{n}_{mesh}_{config}_{f}"], rec[f]
        assert want.dtype == np.uint32 and got.dtype == np.uint32 and want.shape == got.shape, f
        d = int((want != got).sum())
        print(f"{n} envs {mesh} {config} {f}: {d} of {want.size} words differ")
        if d:
            bad.append((f, d, [int((want[t] != got[t]).sum()) for t in range(gen.STEPS)]))
    assert not bad, f"(array, differing words, per step) against {str(golden['commit'])}: {bad}"


def _env(n, mesh, fused):
    from ti5_isaacgym_amd import make_t1_env

    def hook(cfg):
        rewards28_util.cfg_hook(cfg, dict(rewards28_util.SETTINGS, only_positive_rewards=False))
    env = make_t1_env(num_envs=n, mesh_type=mesh, seed=11, device="cuda:0", cfg_hook=hook)
    env.set_fused(fused)
    env.reset()
    return env


@pytest.mark.parametrize("which", ["none", "single", "corners", "all"])
@pytest.mark.parametrize("n", [33, 97])
def test_all_terms_live_forced_resets_equal_the_split_sequence(n, which, monkeypatch):
    monkeypatch.setenv("T1ENV_DYN_KERNEL", "6")
    fused, split = _env(n, "plane", True), _env(n, "plane", False)
    forced = torch.tensor(RESET_SETS[which](n), dtype=torch.long, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(3)
    for t in range(3):
        if t == 1:
            split.episode_length_buf[forced] = int(split.max_episode_length)
        a = 0.3 * torch.randn(n, 12, device="cuda:0", generator=g)
        _sync(fused, split)
        fused.step(a)
        split.step(a)
        where = f"step {t}"
        r = split.reset_buf.bool()
        if t == 1:
            for env in (fused, split):
                assert bool((env.reset_buf[forced] == 1).all()), f"{where}: a forced env did not reset"
        for f in EXACT:
            assert torch.equal(getattr(fused, f), getattr(split, f)), f"{where}: {f} differs"
        for f in CLOSE:
            torch.testing.assert_close(getattr(fused, f), getattr(split, f), rtol=1e-5, atol=1e-6,
                                       msg=lambda m, f=f: f"{where}: {f}: {m}")
        for f in RESET_EXACT:
            x, y = getattr(fused, f).reshape(n, -1), getattr(split, f).reshape(n, -1)
            assert torch.equal(x[r], y[r]), f"{where}: {f} differs on a reset row"
