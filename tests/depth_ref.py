"""A plain numpy reference of the depth camera sensor (include/t1render.h, t1render_depth), written from the header's
words and independent of csrc/t1render_depth.hip, in the float type asked for (fp64 is the reference, fp32 measures what
the number format alone costs).

The intersections are tests/render_ref.py's (world_prims, cast_prims, cast_heightfield, quat_rot: world-space face
planes, every root of the capsule's three surfaces, Moeller-Trumbore on every candidate cell -- none of them the
kernel's slab test or DDA).  What is the sensor's own is built here: the camera frame mounted on a body, the ray's range
near <= z <= far in planar depth, the entry-only rule applied per primitive (a primitive entered in front of the near
plane is not seen, the next one behind it is), the terrain-wins tie, and the value: z = t (d.f), exactly far without a
hit in range.

Ties.  The header gives a tie at exactly equal t to the terrain, then to the lower primitive index.  The product's
primitive table makes such ties: the capsules of two consecutive links end and start in the same joint sphere, whose
centre reaches the two primitives through different sums (the parent's origin plus its rotated offset, the child's own
origin), so in float the two entries differ in their last bits and no float32 implementation can realise "exactly
equal".  Where a surface with another id lies within TIE of the nearest hit along the ray, render_many reports that id
as ids_alt, and compare() accepts either; the depth is compared all the same, and such a pixel is not counted as
ambiguous.
"""
import numpy as np

import render_ref
from render_ref import AMBIG_OFFSETS, cast_heightfield, cast_prims, quat_rot, world_prims

NONE, BEFORE, INSIDE, BEYOND = 3, -1, 0, 1   # where a ray's first surface lies relative to [near, far]
TIE = 1e-5   # [m] along the ray: float32 places a point a metre away to 1e-7, a grazing entry magnifies that


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def sensor_mount(sensor, dt):
    """pos and quat as the call passes them to the device: float32, the quat normalised in double and rounded once."""
    q = np.asarray(np.float32(sensor["quat"]), dtype=np.float64)
    q = (q / np.sqrt((q * q).sum())).astype(np.float32)
    return np.float32(sensor["pos"]).astype(dt), q.astype(dt)


def sensor_frame(rigid, sensor, dt, mount=None):
    """eye, f, l, u of the header: eye = p_b + R_b pos, (f, l, u) = the columns of R_b R_m.  mount: a (7,) float32 row
    (pos, unit quat) that replaces the sensor's own, used as it is."""
    row = rigid[sensor["body"]]
    pb, Rb = row[0:3].astype(dt), quat_rot(row[3:7], dt)
    pos, q = sensor_mount(sensor, dt) if mount is None else (np.float32(mount[0:3]).astype(dt), np.float32(mount[3:7]).astype(dt))
    M = Rb @ quat_rot(q, dt)
    return pb + Rb @ pos, M[:, 0], M[:, 1], M[:, 2]


def sensor_rays(frame, sensor, W, H, dt, offset=(0.0, 0.0)):
    """directions (H*W, 3) and d.f (H*W,).  offset: in pixels, added to every pixel centre."""
    _, f, l, u = frame
    r = -l
    th = np.tan(dt(np.float32(sensor["vfov"])) / dt(2))
    jj, ii = np.meshgrid(np.arange(W, dtype=dt), np.arange(H, dtype=dt))
    x = (dt(2) * (jj + dt(0.5) + dt(offset[0])) / dt(W) - dt(1)) * th * dt(W) / dt(H)
    y = (dt(1) - dt(2) * (ii + dt(0.5) + dt(offset[1])) / dt(H)) * th
    d = _unit(f[None, :] + x.reshape(-1, 1) * r[None, :] + y.reshape(-1, 1) * u[None, :]).astype(dt)
    return d, (d @ f).astype(dt)


def _field(T, o, d, tlo, thi, dt):
    """The height field's nearest hit with tlo <= t <= thi per ray (K rays of one origin): t (inf), triangle, and the
    first hit of all beyond render_ref.T_MIN, whatever its range.  render_ref.cast_heightfield searches from T_MIN
    on; a ray whose first hit lies in front of tlo is searched again from a point just short of tlo."""
    t, tri, _ = cast_heightfield(T, o, d, thi, dt)
    first = t.copy()
    for k in np.nonzero(np.isfinite(t) & (t < tlo))[0]:
        s = tlo[k] - dt(render_ref.T_MIN)   # (T_MIN, thi - s] from o + s d is (tlo, thi] from o
        t1, k1, _ = cast_heightfield(T, o + s * d[k], d[k:k + 1], thi[k:k + 1] - s, dt)
        t[k], tri[k] = (t1[0] + s, k1[0]) if k1[0] >= 0 else (np.inf, -1)
    return t, tri, first


def _side(t, c, near, far):
    z = t * c
    return np.where(~np.isfinite(t), NONE, np.where(z < near, BEFORE, np.where(z <= far, INSIDE, BEYOND)))


def render_many(scene, sensor, W, H, prims, dtype, offsets, mount=None):
    """scene: dict(rigid (13, 13) float32 of the env, terrain None (plane) or render_ref's dict).  sensor: dict(body,
    pos, quat, vfov, near, far).  One dict per offset of (H, W) arrays: depth, ids, tri (the terrain triangle shown,
    -1), side (where the ray's first surface of all lies: BEFORE near, INSIDE the range, BEYOND far, NONE)."""
    dt = dtype
    rigid = scene["rigid"]
    frame = sensor_frame(rigid, sensor, dt, mount)
    o = frame[0]
    K, P = len(offsets), W * H
    rays = [sensor_rays(frame, sensor, W, H, dt, off) for off in offsets]
    d = np.concatenate([r[0] for r in rays], 0)   # (K * P, 3), offset-major
    c = np.concatenate([r[1] for r in rays], 0)
    near, far = dt(np.float32(sensor["near"])), dt(np.float32(sensor["far"]))
    tlo, thi = near / c, far / c
    O = np.broadcast_to(o, (K * P, 3))
    # the robot: every primitive's own entry, then the range rule, the nearest, the lower index at a tie
    tp = np.full(K * P, np.inf, dtype=dt)
    ip = np.full(K * P, -1)
    first = np.full(K * P, np.inf, dtype=dt)
    wp = world_prims(prims, rigid, dt)
    body = np.array([w["body"] for w in wp] + [-1])
    every = np.full((len(wp), K * P), np.inf, dtype=dt)   # each primitive's own entry in range
    for k, w in enumerate(wp):
        t, _, _ = cast_prims([w], O, d, 0.0, dt)
        first = np.minimum(first, t)
        every[k] = np.where((t >= tlo) & (t <= thi), t, np.inf)
        upd = every[k] < tp
        tp, ip = np.where(upd, t, tp), np.where(upd, k, ip)
    bound = np.minimum(tp + dt(TIE), thi)   # the terrain is searched a tie's width behind the primitive too
    T = scene.get("terrain")
    tg = np.full(K * P, np.inf, dtype=dt)
    tri = np.full(K * P, -1, dtype=np.int64)
    if T is None:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[2] / d[:, 2]
        t = np.where(np.isfinite(t) & (t > 0), t, np.inf).astype(dt)
        first = np.minimum(first, t)
        ok = (t >= tlo) & (t <= bound)
        tg, tri = np.where(ok, t, np.inf).astype(dt), np.where(ok, 0, -1)
    else:
        for p in range(P):
            sel = np.arange(K) * P + p
            tg[sel], tri[sel], f1 = _field(T, o, d[sel], tlo[sel], bound[sel], dt)
            first[sel] = np.minimum(first[sel], f1)
            miss = ~np.isfinite(f1)   # nothing up to the bound: is there terrain beyond it?
            if miss.any():
                f2, _, _ = cast_heightfield(T, o, d[sel][miss], np.full(miss.sum(), render_ref.T_MAX, dtype=dt), dt)
                first[sel[miss]] = np.minimum(first[sel[miss]], f2)
    behind = np.isfinite(tg) & (tg > tp)   # terrain within TIE behind the primitive: the primitive is nearer
    ground = np.isfinite(tg) & ~behind     # tg <= tp: the terrain wins a tie
    anyhit = ground | (ip >= 0)
    t = np.where(ground, tg, tp)
    depth = np.where(anyhit, np.where(anyhit, t, 0) * c, far).astype(dt)
    ids = np.where(ground, 0, np.where(ip >= 0, 1 + body[ip], -1))
    # another id within TIE of the hit (module docstring): a primitive of another body, or the terrain behind a primitive
    ids_alt = ids.copy()
    for k in range(len(wp)):
        gap = np.abs(np.where(np.isfinite(every[k]) & anyhit, every[k], np.inf) - np.where(anyhit, t, 0))
        near_tie = (gap <= dt(TIE)) & (1 + body[k] != ids)
        ids_alt = np.where(near_tie & (ids_alt == ids), 1 + body[k], ids_alt)
    ids_alt = np.where(behind & (ids_alt == ids), 0, ids_alt)
    tri = np.where(behind, -1, tri)
    side = _side(first, c, near, far)
    out = []
    for k in range(K):
        q = slice(k * P, (k + 1) * P)
        out.append(dict(depth=depth[q].reshape(H, W), ids=ids[q].reshape(H, W), ids_alt=ids_alt[q].reshape(H, W),
                        tri=np.where(ground, tri, -1)[q].reshape(H, W), side=side[q].reshape(H, W)))
    return out


def render(scene, sensor, W, H, prims, dtype=np.float64, mount=None):
    return render_many(scene, sensor, W, H, prims, dtype, ((0.0, 0.0),), mount)[0]


def reference(scene, sensor, W, H, prims, mount=None):
    """The fp64 image plus its ambiguity mask: a pixel is ambiguous when the rays through its centre and through the
    four points AMBIG_OFFSETS pixels beside it do not all give the same id, the same terrain triangle and the same side
    of near and of far for the ray's first surface."""
    ref, *others = render_many(scene, sensor, W, H, prims, np.float64, ((0.0, 0.0),) + AMBIG_OFFSETS, mount)
    amb = np.zeros((H, W), dtype=bool)
    for r in others:
        amb |= (r["ids"] != ref["ids"]) | (r["tri"] != ref["tri"]) | (r["side"] != ref["side"])
    ref["ambiguous"] = amb
    return ref


def compare(ref, depth, ids, far, atol, rtol):
    """The kernel's image (depth as float, ids or None) against reference()'s on the non-ambiguous pixels: ids equal
    (either id where two surfaces tie within TIE), pixels without a hit exactly far, a hit's depth within atol and within rtol of the reference.  Returns the worst
    absolute and relative errors."""
    m = ~ref["ambiguous"]
    if ids is not None:
        bad = m & (ids != ref["ids"]) & (ids != ref["ids_alt"])
        assert not bad.any(), ("ids differ", np.argwhere(bad)[:5], ids[bad][:5], ref["ids"][bad][:5])
        ties = int((m & (ids != ref["ids"])).sum())
        if ties:
            print("ids: %d pixels show the other surface of a tie within %g m" % (ties, TIE))
    nohit = m & (ref["ids"] < 0)
    assert (depth[nohit] == np.float32(far)).all(), ("no hit is not far", np.argwhere(nohit & (depth != np.float32(far)))[:5])
    hit = m & (ref["ids"] >= 0)
    if not hit.any():
        return 0.0, 0.0
    err = np.abs(depth[hit].astype(np.float64) - ref["depth"][hit])
    rel = err / ref["depth"][hit]
    print("depth error: abs %.3e rel %.3e over %d pixels (allowed %.3e, %.3e)" % (err.max(), rel.max(), hit.sum(), atol, rtol))
    assert err.max() <= atol and rel.max() <= rtol, ("depth", err.max(), rel.max(), atol, rtol)
    return float(err.max()), float(rel.max())
