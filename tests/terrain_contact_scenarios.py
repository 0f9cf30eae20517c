"""Robots in contact with a small synthetic height field -- the inputs shared by tests/test_dynamics_terrain_contact.py
(host builds) and tests/test_gpu_dynamics_terrain_contact.py (the step kernels).

The field (rows along x, FIELD_ROWS x FIELD_COLS samples, non-square so that a rows / cols swap shows; the border is
no multiple of the horizontal scale):
  * rows 0 .. SLOPE_ROWS-1: a rough tilted region, mean slope +0.3 in x and -0.15 in y plus up to 3 raw units
    (15 mm) of roughness per sample, so neighbouring triangles have different normals;
  * the other rows: a low floor with an L-shaped plateau STEP_RAW raw units (0.25 m) above it; one face of the step runs
    along constant x (rows STEP_ROW .. STEP_ROW+1), one along constant y (cols STEP_COL .. STEP_COL+1).  In the triangle
    mesh a face is a one-cell-wide ramp.
All heights are above z = 0, so a reference blind to the field (the plane z = 0) sees no contact at all.

Robots are placed at absolute field coordinates.  Kinds (see scenario()):
  slope   stance on the tilted region, the lowest point 6-15 mm deep (several points on different triangles touch)
  impact  the same, falling faster than the bounce threshold, restitution episodes under way
  edge    a foot's toe on the plateau, its frame origin back over the low floor beyond the ramp: origin height minus the
          foot's contact radius is above the terrain under the origin, so a contact bound that looked only at the
          origin's own cell would skip the body.  Even envs stand at the constant-x face, odd envs at the constant-y face.
          STEP_ROW and STEP_COL are multiples of 3, the solver's coarse bound cell: the ramp's low end is the last sample
          of the origin's coarse cell, the plateau starts in the next one.
  base    the robot lies pitched about 90 degrees, legs folded away: points of the base box touch the slope

Every env is resampled (fixed seed) until the conditions the comparison needs hold -- env_facts() / check_kind():
  * every contact point in contact sits at least MARGIN (barycentric) inside its triangle, so fp32 and fp64 pick the
    same triangle;
  * every contact point of the robot has |h - z| >= CLEARANCE, so the contact set is the same;
  * every env has a terrain contact, and its kind's own condition.
"""
import numpy as np

from oracle.dynamics_ref import ContactRobot, MeshTerrain, quat_to_R

FIELD_ROWS, FIELD_COLS, HS, VS, BORDER = 40, 28, 0.1, 0.005, 0.37
SLOPE_ROWS, STEP_ROW, STEP_COL, FLOOR_RAW, STEP_RAW = 24, 33, 18, 60, 50
MARGIN, CLEARANCE = 1e-3, 1e-5
KINDS = ("slope", "impact", "edge", "base")
PER = 16
BOUNCE_THRESHOLD = 0.5


def make_field():
    """int16 heights (FIELD_ROWS, FIELD_COLS), rows along x"""
    rng = np.random.default_rng(2024)
    i, j = np.meshgrid(np.arange(FIELD_ROWS), np.arange(FIELD_COLS), indexing="ij")
    h = 100 + np.rint(0.3 * HS / VS * i - 0.15 * HS / VS * j).astype(np.int64) + rng.integers(-3, 4, i.shape)
    step = FLOOR_RAW + np.where((i > STEP_ROW) | (j > STEP_COL), STEP_RAW + rng.integers(-2, 3, i.shape), 0)
    h = np.where(i < SLOPE_ROWS, h, step)
    assert h.min() > 0
    return h.astype(np.int16)


def mesh_terrain(field=None):
    return MeshTerrain(make_field() if field is None else field, HS, VS, BORDER)


def contact_radius(tab):
    """each body's largest contact-point distance from its frame origin (what the solver's coarse bound is built on)"""
    pts = np.asarray(tab["contact_point"], float)
    r = np.zeros(13)
    for b in range(13):
        s, n = tab["contact_start"][b], tab["contact_count"][b]
        if n:
            r[b] = np.linalg.norm(pts[s:s + n], axis=1).max()
    return r


def _quat(yaw, pitch):
    """Gym (x, y, z, w) of Rz(yaw) Ry(pitch)"""
    cy, sy, cp, sp = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2)
    return np.array([-sy * sp, cy * sp, sy * cp, cy * cp])


def env_facts(rob, root, dof):
    """what the tests need to know about one env's terrain contacts (rob.terrain: the MeshTerrain)"""
    R = quat_to_R(root[3:7])
    pts = rob.terrain_points(root[0:3], R, dof[:, 0])
    touching = [t for t in pts if t[3] - t[2][2] > 0]
    Rs, ps, _ = rob.fk(root[0:3], R, dof[:, 0])
    rad = contact_radius(rob.tab)
    culled = 0   # touching bodies whose origin clears the terrain under it by more than the body's contact radius
    for b in sorted({t[0] for t in touching}):
        culled += ps[b][2] - rad[b] > rob.terrain.query(ps[b][0], ps[b][1])[0]
    return {"contacts": len(touching),
            "base_contacts": sum(t[0] == 0 for t in touching),
            "base_slots": sorted({4 + (t[1] - rob.tab["contact_start"][0]) * 2 // rob.tab["contact_count"][0]
                                  for t in touching if t[0] == 0}),
            "bodies": sorted({t[0] for t in touching}),
            "margin": min((t[5] for t in touching), default=np.inf),
            "clearance": min(abs(t[3] - t[2][2]) for t in pts),
            "halves": sorted({t[6] for t in touching}),
            "tilt": max((min(abs(t[4][0]), abs(t[4][1])) for t in touching), default=0.0),
            "depth": max((t[3] - t[2][2] for t in touching), default=0.0),
            "cull_condition": int(culled)}


def _settle(rob, root, dof, depth):
    """lower the robot until its deepest contact point is `depth` below the terrain (fp32 state)"""
    root[2] = 0.0
    pts = rob.terrain_points(root[0:3], quat_to_R(root[3:7]), dof[:, 0])
    root[2] = np.float32(max(t[3] - t[2][2] for t in pts) - depth)


def _sample(kind, i, rng, rob):
    q = np.array([0, 0, -0.3, 0.6, -0.3, 0] * 2) + rng.uniform(-0.1, 0.1, 12)
    qd = rng.normal(0, 0.5, 12)
    root = np.zeros(13)
    root[7:13] = rng.normal(0, 0.2, 6)
    yaw, pitch = rng.uniform(-np.pi, np.pi), 0.0
    depth = rng.uniform(0.006, 0.015)
    if kind in ("slope", "impact"):
        root[0:2] = rng.uniform(0.2, 1.3), rng.uniform(0.2, 1.7)
        if kind == "impact":
            root[9] = -rng.uniform(0.8, 1.5)
    elif kind == "base":
        # lying face down (even envs: the box's front half) / on its back (odd: the rear half) on the slope, the thighs
        # swung away from the ground (inside the hip pitch limits) so the legs stay clear
        pitch = rng.uniform(1.2, 1.7) if i % 2 == 0 else -rng.uniform(1.4, 1.7)
        q[2] = q[8] = np.sign(pitch) * rng.uniform(0.45, 0.75)
        root[0:2] = rng.uniform(0.8, 1.0), rng.uniform(0.8, 1.2)
    root[3:7] = _quat(yaw, pitch)
    if kind == "edge":
        along_y = i % 2 == 1
        yaw = (np.pi / 2 if along_y else 0.0) + rng.uniform(-0.25, 0.25)
        root[3:7] = _quat(yaw, 0.0)
        foot = 6 if rng.uniform() < 0.5 else 12
        _, ps, _ = rob.fk(np.zeros(3), quat_to_R(root[3:7]), q)
        # the foot's origin 2-18 mm short of the ramp's low end; the toe points reach 0.12-0.14 m ahead of it
        back = rng.uniform(0.002, 0.018)
        if along_y:
            root[0:2] = rng.uniform(2.35, 2.5), (STEP_COL * HS - BORDER) - back - ps[foot][1]
        else:
            root[0:2] = (STEP_ROW * HS - BORDER) - back - ps[foot][0], rng.uniform(0.1, 1.0)
        depth = rng.uniform(0.003, 0.01)
    root = root.astype(np.float32).astype(np.float64)
    dof = np.stack([q, qd], -1).astype(np.float32).astype(np.float64)
    _settle(rob, root, dof, depth)
    return root, dof


def _accept(kind, i, f):
    if f["contacts"] == 0 or f["margin"] < MARGIN or f["clearance"] < CLEARANCE:
        return False
    if kind == "edge":
        return f["cull_condition"] > 0 and set(f["bodies"]) <= {6, 12}
    if kind == "base":
        return f["base_contacts"] >= (2 if i % 4 < 2 else 1)   # half of them: an edge of the box lies on the slope
    return True


def scenario(kind, tab, terrain, n=PER):
    """(root (n, 13), dof (n, 12, 2), vimp (n, 6), facts per env) of one kind, fp32-exact values"""
    rob = ContactRobot(tab, solver={}, terrain=terrain)
    rng = np.random.default_rng(500 + KINDS.index(kind))
    roots, dofs, facts = [], [], []
    for i in range(n):
        for _ in range(1000):
            try:
                root, dof = _sample(kind, i, rng, rob)
                f = env_facts(rob, root, dof)
            except ValueError:      # a contact point beyond the field's edge
                continue
            if _accept(kind, i, f):
                break
        else:
            raise RuntimeError(f"no acceptable {kind} state for env {i}")
        roots.append(root)
        dofs.append(dof)
        facts.append(f)
    vimp = np.zeros((n, 6), np.float32)
    if kind == "impact":   # restitution episodes under way, most above the bounce threshold
        vimp = np.where(rng.uniform(size=(n, 6)) < 0.6, rng.uniform(0.6, 2.0, (n, 6)), 0.0).astype(np.float32)
    return np.array(roots), np.array(dofs), vimp, facts


def episode_slots(bodies):
    """the restitution episode slots (2 leg + shank / foot) of touching leg bodies"""
    out = set()
    for b in bodies:
        if b != 0:
            out.add(2 * ((b - 1) // 6) + (1 if (b - 1) % 6 == 5 else 0))
    return out


def check_kind(kind, facts, vimp, bounce_threshold=BOUNCE_THRESHOLD):
    """the generator's conditions, asserted by every test that uses a kind"""
    assert all(f["contacts"] > 0 for f in facts), f"{kind}: an env without terrain contact"
    assert min(f["margin"] for f in facts) >= MARGIN, f"{kind}: a contact within {MARGIN} of a triangle's edge"
    assert min(f["clearance"] for f in facts) >= CLEARANCE, f"{kind}: a contact point within {CLEARANCE} m of the surface"
    assert {h for f in facts for h in f["halves"]} == {0, 1}, f"{kind}: contacts in one half of the cells only"
    assert sum(f["tilt"] > 0.05 for f in facts) >= 2, f"{kind}: no normals tilted in both x and y"
    if kind == "slope":
        assert sum(f["contacts"] >= 3 for f in facts) >= len(facts) // 2, "slope: too few points per env touch"
    if kind == "edge":
        assert sum(f["cull_condition"] > 0 for f in facts) >= 4, "edge: fewer than 4 envs meet the cull condition"
        for face, sub in (("constant-x", facts[0::2]), ("constant-y", facts[1::2])):
            assert sum(f["cull_condition"] > 0 for f in sub) >= 2, f"edge: the {face} face lacks cull-condition envs"
    if kind == "base":
        assert all(f["base_contacts"] > 0 for f in facts), "base: an env without a base-box contact"
        assert sum(f["base_contacts"] >= 2 for f in facts) >= 4, "base: no env with two base-box points touching"
        assert {s for f in facts for s in f["base_slots"]} == {4, 5}, "base: one half of the box never touches"
    if kind == "impact":
        open_ = sum(vimp[i, s] > bounce_threshold for i, f in enumerate(facts) for s in episode_slots(f["bodies"]))
        assert open_ >= 4, "impact: no open episodes above the bounce threshold on touching bodies"
