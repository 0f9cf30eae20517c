"""A plain numpy ray caster for the renderer's tests: the scene definition of include/t1render.h written down
independently of csrc/t1render.hip, in the float type asked for (fp64 is the reference, fp32 measures what the number
format alone costs).

Where the kernel slab-tests a box in the body frame, this intersects the six face planes in world space and keeps the
points that lie on the box; where the kernel takes the first entry into two spheres and a cylinder, this collects every
root of those three surfaces and keeps the ones at distance r from the segment; the smallest kept root is where the line
enters the convex solid.  Where the kernel walks the height field's cells (DDA), this intersects every triangle
(Moeller-Trumbore, world coordinates) of every cell that the ray's extent can touch and takes the nearest hit: the
extent is cut to the field's height range and into stretches of at most CHUNK cells, each stretch tests all cells of its
bounding rectangle (plus a margin) and keeps hits inside its own stretch of t.  Testing all rows x cols cells for every
pixel gives the same answer and takes minutes.
"""
import numpy as np

T_MIN, T_MAX, SHADOW_EPS = 0.05, 200.0, 1e-3
CHUNK = 16   # cells of travel per stretch of the height-field search


def quat_rot(q, dt):
    x, y, z, w = (dt(v) for v in q)
    one, two = dt(1), dt(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=dt)


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def camera_rays(cam, base, W, H, dt, offset=(0.0, 0.0)):
    """origin (3,), directions (H*W, 3).  offset: in pixels, added to every pixel centre."""
    eye, tgt, up = (np.asarray(cam[k], dtype=dt) for k in ("eye", "target", "up"))
    if cam.get("follow"):
        eye, tgt = eye + base.astype(dt), tgt + base.astype(dt)
    f = _unit(tgt - eye)
    r = _unit(np.cross(f, up))
    u = np.cross(r, f)
    th = np.tan(dt(np.float32(cam["vfov"])) / dt(2))
    jj, ii = np.meshgrid(np.arange(W, dtype=dt), np.arange(H, dtype=dt))
    x = (dt(2) * (jj + dt(0.5) + dt(offset[0])) / dt(W) - dt(1)) * th * dt(W) / dt(H)
    y = (dt(1) - dt(2) * (ii + dt(0.5) + dt(offset[1])) / dt(H)) * th
    d = f[None, :] + x.reshape(-1, 1) * r[None, :] + y.reshape(-1, 1) * u[None, :]
    return eye, _unit(d).astype(dt)


def _tol(dt):
    return dt(1e-9) if dt is np.float64 else dt(3e-5)


def _box_entry(o, d, c, R, h, dt):
    """o (P,3) origins, d (P,3).  Returns t (P,) entry (+inf on a miss) and the entry face's outward normal (P,3)."""
    P = d.shape[0]
    best = np.full(P, np.inf, dtype=dt)
    nrm = np.zeros((P, 3), dtype=dt)
    tol = _tol(dt)
    for k in range(3):
        for s in (dt(-1), dt(1)):
            n = s * R[:, k]
            fc = c + n * h[k]
            den = d @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((fc[None, :] - o) @ n) / den
            ok = np.isfinite(t)
            p = o + np.where(ok, t, 0)[:, None] * d
            q = (p - c[None, :]) @ R   # body frame
            for m in range(3):
                if m != k:
                    ok &= np.abs(q[:, m]) <= h[m] + tol
            upd = ok & (t < best)
            best = np.where(upd, t, best)
            nrm[upd] = n
    return best, nrm


def _seg_dist(p, a, b):
    ba = b - a
    L = (ba * ba).sum()
    s = np.clip(((p - a[None, :]) @ ba) / L, 0, 1) if L > 0 else np.zeros(p.shape[0], dtype=p.dtype)
    cl = a[None, :] + s[:, None] * ba[None, :]
    return np.sqrt(((p - cl) ** 2).sum(-1)), cl


def _capsule_entry(o, d, a, b, r, dt):
    P = d.shape[0]
    tol = _tol(dt)
    roots = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in ((a,) if np.array_equal(a, b) else (a, b)):
            oc = o - c[None, :]
            aq = (d * d).sum(-1)   # the light's direction is a unit vector only to fp32
            bq = (oc * d).sum(-1)
            cq = (oc * oc).sum(-1) - r * r
            h = bq * bq - aq * cq
            sq = np.sqrt(np.where(h >= 0, h, np.nan))
            roots += [(-bq - sq) / aq, (-bq + sq) / aq]
        if not np.array_equal(a, b):
            ax = _unit(b - a)
            oa = o - a[None, :]
            dp = d - (d @ ax)[:, None] * ax[None, :]
            op = oa - (oa @ ax)[:, None] * ax[None, :]
            A = (dp * dp).sum(-1)
            B = (dp * op).sum(-1)
            Cq = (op * op).sum(-1) - r * r
            h = B * B - A * Cq
            sq = np.sqrt(np.where(h >= 0, h, np.nan))
            roots += [(-B - sq) / A, (-B + sq) / A]
    best = np.full(P, np.inf, dtype=dt)
    for t in roots:
        p = o + np.where(np.isfinite(t), t, 0)[:, None] * d
        dist, _ = _seg_dist(p, a, b)
        ok = np.isfinite(t) & (np.abs(dist - r) <= tol) & (t < best)
        best = np.where(ok, t, best)
    p = o + np.where(np.isfinite(best), best, 0)[:, None] * d
    _, cl = _seg_dist(p, a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = _unit(p - cl)
    return best, n


def world_prims(prims, rigid, dt):
    out = []
    for p in prims:
        row = rigid[p["body"]]
        pos, R = row[0:3].astype(dt), quat_rot(row[3:7], dt)
        a, b = np.asarray(p["a"], dtype=np.float32).astype(dt), np.asarray(p["b"], dtype=np.float32).astype(dt)
        if p["kind"] == 0:
            out.append(dict(kind=0, body=p["body"], rgb=p["rgb"], c=pos + R @ a, R=R, h=b))
        else:
            out.append(dict(kind=1, body=p["body"], rgb=p["rgb"], a=pos + R @ a, b=pos + R @ b,
                            r=np.float32(p["r"]).astype(dt)))
    return out


def cast_prims(wp, o, d, tlo, dt):
    """o (P,3), d (P,3).  Nearest primitive entry in (tlo, T_MAX]: t (inf = none), index (-1), normal."""
    P = d.shape[0]
    best = np.full(P, np.inf, dtype=dt)
    idx = np.full(P, -1)
    nrm = np.zeros((P, 3), dtype=dt)
    for k, p in enumerate(wp):
        t, n = _box_entry(o, d, p["c"], p["R"], p["h"], dt) if p["kind"] == 0 else \
            _capsule_entry(o, d, p["a"], p["b"], p["r"], dt)
        upd = (t > dt(tlo)) & (t <= dt(T_MAX)) & (t < best)
        best = np.where(upd, t, best)
        idx = np.where(upd, k, idx)
        nrm[upd] = n[upd]
    return best, idx, nrm


def _tri_hits(o, d, v0, v1, v2, dt):
    """Moeller-Trumbore, two-sided.  o (3,), d (K,3); v* (n,3).  Returns t (K,n), inf where missed."""
    tol = _tol(dt)
    e1, e2 = v1 - v0, v2 - v0
    pv = np.cross(d[:, None, :], e2[None, :, :])
    det = (e1[None] * pv).sum(-1)
    tv = (o[None, :] - v0)[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1[None])
        v = (d[:, None, :] * qv).sum(-1) / det
        t = (e2[None] * qv).sum(-1) / det
    ok = (det != 0) & (u >= -tol) & (v >= -tol) & (u + v <= dt(1) + tol) & np.isfinite(t)
    return np.where(ok, t, np.inf)


def cast_heightfield(T, o, d, tmax, dt):
    """One origin o (3,), K directions d (K,3), per-ray upper bound tmax (K,).  Nearest hit in (T_MIN, tmax]:
    t (K,) (inf = none), triangle id (K,) (2 * (i * cols + j) + which, -1), upward unit normal (K,3)."""
    h, hs, vs, border = T["h"], T["hscale"], T["vscale"], T["border"]
    rows, cols = h.shape
    K = d.shape[0]
    best = np.full(K, np.inf, dtype=dt)
    tri = np.full(K, -1, dtype=np.int64)
    nrm = np.zeros((K, 3), dtype=dt)
    o64, d64 = o.astype(np.float64), d[0].astype(np.float64)   # the stretches follow the first ray; the others are
    lo, hi = T_MIN, float(np.max(tmax))                        # within a fraction of a pixel of it (margin below)
    zmin, zmax = float(h.min()) * vs - 1e-6, float(h.max()) * vs + 1e-6
    box = ((-border, (rows - 1) * hs - border), (-border, (cols - 1) * hs - border), (zmin, zmax))
    for k in range(3):
        if d64[k] != 0:
            ta, tb = (box[k][0] - o64[k]) / d64[k], (box[k][1] - o64[k]) / d64[k]
            lo, hi = max(lo, min(ta, tb) - 1e-3), min(hi, max(ta, tb) + 1e-3)
        elif not box[k][0] <= o64[k] <= box[k][1]:
            return best, tri, nrm
    if not lo <= hi:
        return best, tri, nrm
    lo = max(lo, T_MIN)
    speed = max(abs(d64[0]), abs(d64[1])) / hs   # cells per unit t
    nchunk = max(1, int(np.ceil((hi - lo) * speed / CHUNK)))
    edges = np.linspace(lo, hi, nchunk + 1)
    hw = h.astype(dt) * dt(vs)
    for ta, tb in zip(edges[:-1], edges[1:]):
        pa, pb = o64 + ta * d64, o64 + tb * d64
        gi = sorted(((pa[0] + border) / hs, (pb[0] + border) / hs))
        gj = sorted(((pa[1] + border) / hs, (pb[1] + border) / hs))
        i0, i1 = max(int(np.floor(gi[0])) - 2, 0), min(int(np.floor(gi[1])) + 2, rows - 2)
        j0, j1 = max(int(np.floor(gj[0])) - 2, 0), min(int(np.floor(gj[1])) + 2, cols - 2)
        if i0 > i1 or j0 > j1:
            continue
        I, J = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1), indexing="ij")
        I, J = I.ravel(), J.ravel()
        X0, X1 = I.astype(dt) * dt(hs) - dt(border), (I + 1).astype(dt) * dt(hs) - dt(border)
        Y0, Y1 = J.astype(dt) * dt(hs) - dt(border), (J + 1).astype(dt) * dt(hs) - dt(border)
        p00 = np.stack([X0, Y0, hw[I, J]], 1)
        p10 = np.stack([X1, Y0, hw[I + 1, J]], 1)
        p11 = np.stack([X1, Y1, hw[I + 1, J + 1]], 1)
        p01 = np.stack([X0, Y1, hw[I, J + 1]], 1)
        for which, (v0, v1, v2) in enumerate(((p00, p10, p11), (p00, p11, p01))):
            t = _tri_hits(o, d, v0, v1, v2, dt)
            t = np.where((t > dt(T_MIN)) & (t <= tmax[:, None]) & (t > dt(ta) - dt(1e-4)) & (t <= dt(tb) + dt(1e-4)),
                         t, np.inf)
            m = t.argmin(1)
            tm = t[np.arange(K), m]
            upd = tm < best
            if upd.any():
                best = np.where(upd, tm, best)
                tri = np.where(upd, 2 * (I[m] * cols + J[m]) + which, tri)
                n = np.cross(v1[m] - v0[m], v2[m] - v0[m])
                n = _unit(n * np.sign(n[:, 2:3]))
                nrm[upd] = n[upd]
        if np.isfinite(best).all():
            break
    return best, tri, nrm


def _shade(style, base, n, lit, dt):
    L = _unit(np.asarray(style["light"], dtype=np.float64)).astype(np.float32).astype(dt)
    amb = np.float32(style["ambient"]).astype(dt)
    nl = np.maximum(n @ L, 0)
    return (amb + (dt(1) - amb) * nl * lit)[:, None] * base, nl, L


def render_many(scene, cam, W, H, prims, style, dtype, offsets):
    """render() for several pixel offsets at once (the rays of one pixel share the height-field search): a list of
    render()'s dicts, one per offset."""
    dt = dtype
    rigid = scene["rigid"]
    K, P = len(offsets), W * H
    rays = [camera_rays(cam, rigid[0, 0:3], W, H, dt, off) for off in offsets]
    o = rays[0][0]
    d = np.concatenate([r[1] for r in rays], 0)   # (K * P, 3), offset-major
    O = np.broadcast_to(o, (K * P, 3))
    wp = world_prims(prims, rigid, dt)
    tp, ip, nprim = cast_prims(wp, O, d, T_MIN, dt)
    T = scene.get("terrain")
    tg = np.full(K * P, np.inf, dtype=dt)
    tri = np.full(K * P, -1, dtype=np.int64)
    ng = np.zeros((K * P, 3), dtype=dt)
    ng[:, 2] = 1
    bound = np.minimum(tp, dt(T_MAX))
    if T is None:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[2] / d[:, 2]
        ok = np.isfinite(t) & (t > dt(T_MIN)) & (t <= bound)
        tg = np.where(ok, t, np.inf).astype(dt)
        tri = np.where(ok, 0, -1)
    else:
        for p in range(P):
            sel = np.arange(K) * P + p
            t1, k1, n1 = cast_heightfield(T, o, d[sel], bound[sel], dt)
            hit1 = k1 >= 0
            tg[sel], tri[sel] = t1, k1
            ng[sel[hit1]] = n1[hit1]
    ground = np.isfinite(tg)   # tg <= bound <= tp: the terrain wins a tie, as in the kernel
    anyhit = ground | (ip >= 0)
    depth = np.where(ground, tg, tp)
    n = np.where(ground[:, None], ng, nprim)
    ids = np.where(ground, 0, np.where(ip >= 0, 1 + np.array([w["body"] for w in wp] + [0])[ip], -1))
    hit = O + np.where(anyhit, depth, 0)[:, None] * d
    base = np.zeros((K * P, 3), dtype=dt)
    par = (np.floor(hit[:, 0]).astype(np.int64) + np.floor(hit[:, 1]).astype(np.int64)) & 1
    trgb = np.asarray(style["terrain_rgb"], dtype=np.float32).astype(dt)
    base[ground] = trgb[par[ground]]
    rgbs = np.array([[(w["rgb"] >> s) & 255 for s in (0, 8, 16)] for w in wp] + [[0, 0, 0]], dtype=dt) * (dt(1) / dt(255))
    isp = anyhit & ~ground
    base[isp] = rgbs[ip[isp]]
    _, nl, L = _shade(style, base, n, np.ones(K * P, dtype=dt), dt)
    so = hit + dt(SHADOW_EPS) * n
    ts, _, _ = cast_prims(wp, so, np.broadcast_to(L, (K * P, 3)), 0.0, dt)
    lit = ~(np.isfinite(ts) & (nl > 0))
    value, _, _ = _shade(style, base, n, lit.astype(dt), dt)
    sky = np.asarray(style["sky_rgb"], dtype=np.float32).astype(dt)
    s = dt(0.5) * (d[:, 2] + dt(1))
    value = np.where(anyhit[:, None], value, sky[0][None] + s[:, None] * (sky[1] - sky[0])[None])
    def to8(v):
        return np.floor(np.clip(v, 0, 1) * dt(255) + dt(0.5)).astype(np.uint8)
    rgb = to8(value)
    alt = to8(_shade(style, base, n, (~lit).astype(dt), dt)[0])   # the colour with the other lit decision
    out = []
    for k in range(K):
        q = slice(k * P, (k + 1) * P)
        out.append(dict(ids=ids[q].reshape(H, W), depth=np.where(anyhit, depth, np.inf)[q].reshape(H, W),
                        lit=(lit | ~anyhit)[q].reshape(H, W), tri=np.where(ground, tri, -1)[q].reshape(H, W),
                        rgb=rgb[q].reshape(H, W, 3), rgb_other=alt[q].reshape(H, W, 3),
                        nl=np.where(anyhit, nl, 0)[q].reshape(H, W), hit=hit[q].reshape(H, W, 3)))
    return out


def render(scene, cam, W, H, prims, style, dtype=np.float64, offset=(0.0, 0.0)):
    """scene: dict(rigid (13,13) float32 of the camera's env, terrain None (plane) or dict(h int16 (rows, cols),
    hscale, vscale, border)).  Returns dict of (H, W[, 3]) arrays: ids, depth, lit (bool; True where nothing is hit or
    the surface faces away from the light), tri, rgb (uint8), rgb_other (the colour had the shadow ray decided the other
    way), nl, hit."""
    return render_many(scene, cam, W, H, prims, style, dtype, (offset,))[0]


AMBIG_OFFSETS = ((1e-3, 0.0), (-1e-3, 0.0), (0.0, 1e-3), (0.0, -1e-3))


def reference(scene, cam, W, H, prims, style):
    """The fp64 image plus its ambiguity mask: a pixel is ambiguous when the rays through its centre and through the four
    points AMBIG_OFFSETS pixels beside it do not all give the same id, the same lit flag and the same terrain triangle."""
    ref, *others = render_many(scene, cam, W, H, prims, style, np.float64, ((0.0, 0.0),) + AMBIG_OFFSETS)
    amb = np.zeros((H, W), dtype=bool)
    for r in others:
        amb |= (r["ids"] != ref["ids"]) | (r["lit"] != ref["lit"]) | (r["tri"] != ref["tri"])
    ref["ambiguous"] = amb
    return ref


def compare(ref, rgba, depth, ids, depth_atol, depth_rtol):
    """The kernel's image (rgba (H, W, 4) uint8, depth, ids) against reference()'s on the non-ambiguous pixels: ids
    equal, the lit decision equal (recovered from the colour wherever the two decisions differ by more than the colour
    tolerance), colour within 1 LSB, depth within depth_atol and within depth_rtol of the reference.  Returns the
    worst absolute and relative depth errors."""
    m = ~ref["ambiguous"]
    assert (rgba[..., 3] == 255).all()
    bad = m & (ids != ref["ids"])
    assert not bad.any(), ("ids differ", np.argwhere(bad)[:5], ids[bad][:5], ref["ids"][bad][:5])
    got = rgba[..., :3].astype(np.int64)
    d_same = np.abs(got - ref["rgb"].astype(np.int64)).max(-1)
    d_other = np.abs(got - ref["rgb_other"].astype(np.int64)).max(-1)
    decides = np.abs(ref["rgb"].astype(np.int64) - ref["rgb_other"].astype(np.int64)).max(-1) > 2
    bad = m & decides & (d_other <= d_same)
    assert not bad.any(), ("lit decision differs", np.argwhere(bad)[:5])
    bad = m & (d_same > 1)
    assert not bad.any(), ("colour differs", np.argwhere(bad)[:5], got[bad][:5], ref["rgb"][bad][:5])
    hit = m & (ref["ids"] >= 0)
    assert np.array_equal(np.isinf(depth[m]), ref["ids"][m] < 0) and (depth[m & ~hit] > 0).all()
    if not hit.any():
        return 0.0, 0.0
    err = np.abs(depth[hit].astype(np.float64) - ref["depth"][hit])
    rel = err / ref["depth"][hit]
    assert err.max() <= depth_atol and rel.max() <= depth_rtol, ("depth", err.max(), rel.max(), depth_atol, depth_rtol)
    return float(err.max()), float(rel.max())
