"""The substep's state update on the host builds of the dynamics header (fp64 and fp32), no GPU: the twin of
tests/test_gpu_state_update.py, with the same inputs and comparisons (tests/state_update_util.py).

The independent references (oracle/dynamics_ref.py) return a velocity change; what integrate_base / integrate_leg do
with it was held only to the same header compiled in fp64.  Here ten single substeps (oracle/dyn_cpu.cpp
t1dyn_substeps, nsub = 1, PD torques toward the nominal pose recomputed per substep) from 33 states -- standing in
contact, airborne tumbling, lying on the base box -- are walked row by row against the numpy restatement of DESIGN.md §4,
and one substep from 33 airborne states with every joint at 0.97-1.0 of its velocity limit and the torque limit pushing
it outward is compared with Kane's equations clipped at the limit.

Five one-line mutants of the header each fail this file (profiles/state_update_mutants.txt): the position from vO_new,
the quaternion from the old angular velocity, q += dt qd_old, vel_limit[k] without 6 * leg, the lower clamp dropped.
"""
import numpy as np
import pytest

import report_scenarios as rs
import state_update_util as su
from test_dynamics_contact import make_setup

FLAGS = {"fp64": 1, "fp32": 0}


@pytest.fixture(scope="module")
def setup():
    return make_setup()


@pytest.fixture(scope="module")
def setup_no_self():
    dyn, m, tab = make_setup()
    m.self_collisions = 0
    return dyn, m, tab


def host_params(m, n, seed):
    """per-env parameters in the ranges the env draws them from (the armatures: oracle/t1_oracle.py ARMATURE_RANGE)"""
    from oracle.t1_oracle import ARMATURE_RANGE
    rng = np.random.default_rng(seed)
    return {"bm": (m.mass[0] + rng.uniform(-1.0, 1.0, n)).astype(np.float32),
            "ls": rng.uniform(0.9, 1.1, (n, 12)).astype(np.float32),
            "cd": rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32),
            "arm": np.stack([rng.uniform(lo, hi, n) for lo, hi in ARMATURE_RANGE], 1).astype(np.float32),
            "fr": rng.uniform(0.2, 1.3, n).astype(np.float32),
            "rst": rng.uniform(0.0, 0.4, n).astype(np.float32)}


def _substep(setup, root, dof, vimp, par, flags, tau):
    case = {"root": root, "dof": dof, "vimp": vimp, "field": None}
    return rs.host_report(setup, case, par, flags, nsub=1, tau=tau, dt=su.DT)


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_state_update_along_ten_substeps(setup, build):
    from oracle.t1_oracle import KD, KP, TORQUE_LIMITS
    dyn, m, tab = setup
    root, dof, kinds = su.log_case(tab)
    par = host_params(m, su.N, seed=21)
    rng = np.random.default_rng(22)
    target = su.Q_NOMINAL + 0.5 * rng.normal(0, 0.5, (su.N, 12))
    vimp = np.zeros((su.N, 6), np.float32)
    rows = [(root, dof)]
    for _ in range(10):
        tau = np.clip(KP * (target - dof[:, :, 0]) - KD * dof[:, :, 1], -TORQUE_LIMITS, TORQUE_LIMITS)
        out = _substep(setup, root, dof, vimp, par, FLAGS[build], tau)
        root, dof, vimp = out["root"], out["dof"], out["vimp"].astype(np.float32)
        rows.append((root, dof))
    com = np.asarray(tab["com"], float)[0] + par["cd"].astype(np.float64)
    vel_limit = [m.vel_limit[j] for j in range(12)]
    assert np.array_equal(np.float32(vel_limit), np.asarray(tab["limits"], np.float32)[:, 3])
    yard, worst, fails = su.walk_rows(rows, com, vel_limit)
    print(su.report_line("host " + build, yard, worst))
    assert not fails, "\n".join(fails[:8])
    # the states move: a check of rows that stand still would pass anything
    assert np.abs(rows[10][0][:, 0:3] - rows[0][0][:, 0:3]).max() > 1e-2
    assert np.abs(rows[10][0][:, 3:7] - rows[0][0][:, 3:7]).max() > 1e-2


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_joint_speed_clamp(setup_no_self, build):
    from oracle.t1_oracle import TORQUE_LIMITS
    dyn, m, tab = setup_no_self
    root, dof, sign = su.clamp_case(tab)
    par = host_params(m, su.N, seed=23)
    tau = (sign * TORQUE_LIMITS).astype(np.float32).astype(np.float64)
    out = _substep(setup_no_self, root, dof, np.zeros((su.N, 6), np.float32), par, FLAGS[build], tau)
    p64 = {k: v.astype(np.float64) for k, v in par.items()}
    su.check_clamp(tab, root, dof, out["dof"][:, :, 1], tau, p64, [m.vel_limit[j] for j in range(12)],
                   label="host " + build)
