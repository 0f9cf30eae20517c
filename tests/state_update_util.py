"""Inputs and comparisons shared by the state-update tests: tests/test_state_update.py (host builds of the header) and
tests/test_gpu_state_update.py (k_dyn6 / k_dyn5 / k_dyn4).

The independent references of oracle/dynamics_ref.py return a velocity change only.  What a substep then does with it
(DESIGN.md §4 "Limits and integration") is restated here in numpy, from the design's words:

  joint speed   qd_s = clip(qd_{s-1} + dqd, -vel_limit_j, +vel_limit_j)      (the description's limit of joint j)
  joint angle   q_s = q_{s-1} + dt qd_s                                      (the NEW, clamped speed)
  position      pos_s = pos_{s-1} + dt vb                                    (vb: the NEW velocity of the base origin)
  orientation   quat_s = normalise(quat_{s-1} + dt/2 [w_s, 0] (x) quat_{s-1})  (the NEW world angular velocity, xyzw)

`walk_rows` checks the last three along a substep log: row s from row s - 1 and row s's own velocities (vb recovered from
the logged COM velocity as tests/test_gpu_dynamics_kane.py does: minus w x R (com + com displacement)), and |qd_s| <=
fp32(vel_limit_j).  Bound per field: 4 x the largest gap between this restatement evaluated in numpy fp32 and in fp64
on the same rows (the builds contract to fma and order the quaternion's sums differently from numpy) + one fp32 ulp of
the field's largest magnitude in the env's row.

`check_clamp` checks the first against Kane's equations (oracle/dynamics_ref.py Robot.accel) with every joint started
at 0.97-1.0 of its limit and torques pushing it outward.
"""
import numpy as np

from oracle.dynamics_ref import ContactRobot, Robot, quat_to_R
from test_dynamics_contact import _place_on_ground, scenario

N = 33            # one full k_dyn6 workgroup (32 envs) plus one env
DT = 0.001
ULP = 2.0 ** -23
FIELDS = ("pos", "quat", "q")
Q_NOMINAL = np.array([0, 0, -0.3, 0.6, -0.3, 0] * 2, float)
DR_MASS_OFF = {"domain_rand.randomize_" + k: False for k in ("base_mass", "com", "link_mass")}


def _fp32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ---- the state update along a log ---------------------------------------------------------------------------------
def log_case(tab, seed=3):
    """(root (33, 13), dof (33, 12, 2), kinds): a third each standing in contact, airborne tumbling (|w| up to 6 rad/s,
    |v| up to 3 m/s) and lying on the base box's side; fp32-exact, positions within 2 m of the origin"""
    rng = np.random.default_rng(seed)
    rob = ContactRobot(tab, solver={})
    per = N // 3
    kinds = ["stand"] * per + ["tumble"] * per + ["lying"] * (N - 2 * per)
    root, dof = scenario("stance", N, rng, tab)
    for i, kind in enumerate(kinds):
        if kind == "tumble":
            quat = rng.normal(size=4)
            root[i, 3:7] = quat / np.linalg.norm(quat)
            root[i, 10:13] = _unit(rng, 1)[0] * rng.uniform(1.0, 6.0)
            root[i, 7:10] = _unit(rng, 1)[0] * rng.uniform(0.5, 3.0)
            dof[i, :, 1] = rng.normal(0, 2.0, 12)
        if kind == "lying":
            # rolled onto a side: the base box is 0.5 m wide, wider than the legs stand apart
            roll = rng.choice([-1.0, 1.0]) * (np.pi / 2 + rng.uniform(-0.1, 0.1))
            yaw = rng.uniform(-np.pi, np.pi)
            qr = np.array([np.sin(roll / 2), 0, 0, np.cos(roll / 2)])
            qy = np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)])
            root[i, 3:7] = _quat_mul(qy, qr)
    root, dof = _fp32(root), _fp32(dof)
    _place_on_ground(rob, root, dof, rng)
    root[[k == "tumble" for k in kinds], 2] = 1.6
    root = _fp32(root)
    # each kind is what it says, on the reference's own contact search
    for i, kind in enumerate(kinds):
        bodies = {c[0] for c in rob.contacts(root[i, 0:3], quat_to_R(root[i, 3:7]), dof[i, :, 0], None, 0, 0, 0, 0,
                                             self_collision=False)}
        if kind == "stand":
            assert bodies and bodies <= {4, 6, 10, 12}, (i, bodies)
        elif kind == "tumble":
            assert not bodies, (i, bodies)
        else:
            assert bodies == {0}, (i, bodies)
    return root, dof, kinds


def _quat_mul(a, b):
    """a (x) b, xyzw"""
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])


def restate(prev_root, prev_q, root, qd, com, dt, T):
    """(pos, quat, q) of a row from the row before it and the row's own velocities and attitude, evaluated in dtype T;
    rows (n, 13) Gym layout (COM velocity), com (n, 3) the base COM in the base frame"""
    c = lambda a: np.asarray(a, T)  # noqa: E731
    one, two, half, dt = T(1), T(2), T(0.5), T(dt)
    # vb: the logged COM velocity minus w x R c, R from the row's own (normalised) quaternion
    qn = c(root[:, 3:7])
    qn = qn / np.sqrt((qn * qn).sum(1, keepdims=True))
    x, y, z, w = qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3]
    cm = c(com)
    Rc = np.stack([(one - two * (y * y + z * z)) * cm[:, 0] + two * (x * y - z * w) * cm[:, 1] + two * (x * z + y * w) * cm[:, 2],
                   two * (x * y + z * w) * cm[:, 0] + (one - two * (x * x + z * z)) * cm[:, 1] + two * (y * z - x * w) * cm[:, 2],
                   two * (x * z - y * w) * cm[:, 0] + two * (y * z + x * w) * cm[:, 1] + (one - two * (x * x + y * y)) * cm[:, 2]], 1)
    om = c(root[:, 10:13])
    vb = c(root[:, 7:10]) - np.cross(om, Rc)
    pos = c(prev_root[:, 0:3]) + dt * vb
    # [w, 0] (x) q = (q_w w + w x q_v, -w . q_v)
    pq = c(prev_root[:, 3:7])
    pv, pw = pq[:, 0:3], pq[:, 3:4]
    h = half * dt
    nv = pv + h * (pw * om + np.cross(om, pv))
    nw = pw - h * (om * pv).sum(1, keepdims=True)
    nq = np.concatenate([nv, nw], 1)
    nq = nq / np.sqrt((nq * nq).sum(1, keepdims=True))
    q = c(prev_q) + dt * c(qd)
    for a in (pos, nq, q):
        assert a.dtype == T
    return {"pos": pos.astype(np.float64), "quat": nq.astype(np.float64), "q": q.astype(np.float64)}


def walk_rows(rows, com, vel_limit, dt=DT):
    """rows: [(root (n, 13), dof (n, 12, 2))] fp32 values, the state before the step then every substep's end.
    Returns (yardstick {field: largest fp32 - fp64 gap of the restatement}, worst {field: |got - fp64 restatement|},
    failures [str]); the bound per env row is 4 yardstick + ulp max|ref|."""
    vl32 = np.asarray(vel_limit, np.float32).astype(np.float64)
    steps = []
    yard = dict.fromkeys(FIELDS, 0.0)
    for s in range(1, len(rows)):
        (pr, pd), (r, d) = rows[s - 1], rows[s]
        r64 = restate(pr, pd[:, :, 0], r, d[:, :, 1], com, dt, np.float64)
        r32 = restate(pr, pd[:, :, 0], r, d[:, :, 1], com, dt, np.float32)
        for f in FIELDS:
            yard[f] = max(yard[f], float(np.abs(r32[f] - r64[f]).max()))
        steps.append((s - 1, {"pos": r[:, 0:3], "quat": r[:, 3:7], "q": d[:, :, 0]}, r64, d[:, :, 1]))
    worst, fails = dict.fromkeys(FIELDS, 0.0), []
    for s, got, ref, qd in steps:
        over = np.abs(qd) > vl32
        if over.any():
            i, j = np.argwhere(over)[0]
            fails.append(f"substep {s} env {i} joint {j}: |qd| {abs(qd[i, j])!r} above fp32(vel_limit) {vl32[j]!r}")
        for f in FIELDS:
            err = np.abs(got[f] - ref[f]).max(axis=1)
            bound = 4 * yard[f] + ULP * np.abs(ref[f]).max(axis=1)
            worst[f] = max(worst[f], float(err.max()))
            for i in np.nonzero(err > bound)[0]:
                fails.append(f"substep {s} env {i} {f}: |got - restated| {err[i]:.3g} > {bound[i]:.3g}")
    return yard, worst, fails


def report_line(label, yard, worst):
    return (f"[{label}] state update: fp32 restatement yardstick " + ", ".join(f"{f} {yard[f]:.2e}" for f in FIELDS)
            + "; worst |got - fp64 restatement| " + ", ".join(f"{f} {worst[f]:.2e}" for f in FIELDS))


# ---- the joint speed clamp ----------------------------------------------------------------------------------------
CLAMP_SEED = 1   # of seeds 1-12 the one whose rarest (joint, direction) clamps most often on the reference: 5-6 times


def clamp_case(tab, seed=CLAMP_SEED):
    """(root (33, 13), dof (33, 12, 2), sign (33, 12)): airborne at 5 m (the Kane test's set-up), every joint at
    0.97-1.0 of its velocity limit in the direction `sign`, which the torques / actions are to push further"""
    rng = np.random.default_rng(seed)
    lim = np.asarray(tab["limits"])
    lo = np.maximum(np.array([-0.5, -0.17, -0.78, 0.01, -1.9, -2.9] * 2), lim[:, 0] + 0.05)
    hi = np.minimum(np.array([0.5, 0.17, 0.78, 2.0, 1.9, 2.9] * 2), lim[:, 1] - 0.05)
    q0 = np.clip(Q_NOMINAL + rng.uniform(-0.15, 0.15, (N, 12)), lo, hi)
    sign = np.where(rng.uniform(size=(N, 12)) < 0.5, -1.0, 1.0)
    # 1 - 0.03 u^2: within 0.97-1.0 and denser toward the limit, since the hip-pitch and knee armatures (up to 3.6 kg m^2)
    # leave those joints about 0.06 rad/s per substep at their torque limit
    qd0 = sign * (1.0 - 0.03 * rng.uniform(0.0, 1.0, (N, 12)) ** 2) * lim[:, 3]
    quat = rng.normal(size=(N, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    root = np.zeros((N, 13))
    root[:, 2] = 5.0
    root[:, 3:7] = quat
    root[:, 7:10] = rng.normal(0, 0.5, (N, 3))
    root[:, 10:13] = rng.normal(0, 0.8, (N, 3))
    return _fp32(root), _fp32(np.stack([q0, qd0], -1)), sign


def check_clamp(tab, root0, dof0, qd1, tau, par, vel_limit, dt=DT, label=""):
    """qd1 (n, 12): the joint speeds after substep 0, as fp32 values.  par: bm (n), ls (n, 12), cd (n, 3), arm (n, 12).
    Expected clip(qd0 + dt a_ref, +-vl): beyond the limit the build's value is fp32(vl_j) bit for bit, inside it is within
    dt 2e-4 (1 + |a_ref|max); a sample whose reference lies within that tolerance of the limit may go either way (at
    most 5% of the samples).  Every joint must clamp upward and downward at least once, on the reference alone."""
    n = root0.shape[0]
    vl32 = np.asarray(vel_limit, np.float32)
    vl = vl32.astype(np.float64)
    mass0, com0 = np.asarray(tab["mass"], float), np.asarray(tab["com"], float)[0]
    up, down, either, inside, fails, worst = np.zeros(12, int), np.zeros(12, int), 0, 0, [], 0.0
    for i in range(n):
        mass = np.concatenate([[par["bm"][i]], mass0[1:] * par["ls"][i]])
        isc = np.concatenate([[par["bm"][i] / mass0[0]], par["ls"][i]])
        R0, w0 = quat_to_R(root0[i, 3:7]), root0[i, 10:13]
        vo0 = root0[i, 7:10] - np.cross(w0, R0 @ (com0 + par["cd"][i]))
        a, _ = Robot(tab, mass, isc, par["cd"][i], par["arm"][i]).accel(root0[i, 0:3], root0[i, 3:7], w0, vo0,
                                                                         dof0[i, :, 0], dof0[i, :, 1], tau[i])
        tol = dt * 2e-4 * (1.0 + np.abs(a).max())
        free = dof0[i, :, 1] + dt * a[6:]
        for j in range(12):
            if abs(abs(free[j]) - vl[j]) <= tol:
                either += 1
                ok = abs(qd1[i, j] - np.clip(free[j], -vl[j], vl[j])) <= tol
            elif abs(free[j]) > vl[j]:
                want = np.float32(np.sign(free[j])) * vl32[j]
                (up if free[j] > 0 else down)[j] += 1
                ok = np.float32(qd1[i, j]) == want
            else:
                inside += 1
                worst = max(worst, abs(qd1[i, j] - free[j]) / tol)
                ok = abs(qd1[i, j] - free[j]) <= tol
            if not ok:
                fails.append(f"env {i} joint {j}: qd {qd1[i, j]!r}, reference {free[j]!r} (limit {vl[j]!r}, tol {tol:.3g})")
    print(f"[{label}] clamp: per joint clamped upward {up.tolist()}, downward {down.tolist()}; inside the limit {inside} "
          f"(worst error {worst:.3f} of its tolerance), within the tolerance of the limit {either} of {12 * n}")
    assert (up > 0).all() and (down > 0).all(), "a joint never clamps in one direction on the reference"
    assert either <= 0.05 * 12 * n, f"{either} samples within the tolerance of the limit"
    assert not fails, "\n".join(fails[:8])
