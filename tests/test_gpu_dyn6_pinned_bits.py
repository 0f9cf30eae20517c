"""k_dyn6 computes, bit for bit, what it computed before its core wave's arithmetic was pinned -- needs the MI355X.

The core wave's sums after S2 (fold-in, elimination, base solve, back-substitution, integration) are contracted in the
source (fmad and its kin, t1_common.h), so that how its rows are loaded, or how its code is ordered, cannot move a
rounding.  tests/golden/dyn6_bits.npz holds what the kernel wrote on the commit before that change, generated there by
tests/golden/gen_dyn6_bits.py: 33 and 97 envs, plane and trimesh, seed 6, six policy steps of seeded actions with
four-step staggered episodes, the envs spawned at 0.95 m so that the feet land within an episode; after every step
root_states, dof_state, contact_vimp, rew_buf, reset_buf and the newest frames of obs_buf and privileged_obs_buf.  The replay on this tree has to equal every one of them in every bit (the
arrays are compared as uint32: NaN and -0.0 count).  Each case must see a reset and an env in contact, so the contact
terms' rows are read with something in them.

The fixture is regenerated only by a change that means to change results.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_dyn6_bits", os.path.join(GOLDEN, "gen_dyn6_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dyn6_bits.npz"))


@pytest.mark.parametrize("mesh", ["plane", "trimesh"])
@pytest.mark.parametrize("n", [33, 97])
def test_replay_equals_the_recorded_bits(n, mesh, golden, monkeypatch):
    monkeypatch.setenv("T1ENV_DYN_KERNEL", "6")
    gen = _gen()
    assert (n, mesh) in gen.CASES
    rec, resets, touched = gen.replay(n, mesh)
    assert resets > 0, "no env reset"
    assert touched > 0, "no env had a contact"
    bad = []
    for f, _ in gen.FIELDS:
        want, got = golden[f"{n}_{mesh}_{f}"], rec[f]
        assert want.dtype == np.uint32 and got.dtype == np.uint32 and want.shape == got.shape, f
        for t in range(gen.STEPS):
            d = int((want[t] != got[t]).sum())
            print(f"{n} envs {mesh} step {t} {f}: {d} of {want[t].size} words differ")
            if d:
                bad.append((t, f, d))
    assert not bad, f"(step, array, differing words) against {str(golden['commit'])}: {bad}"
