"""The numpy reference of t1render_mesh_scene (include/t1render.h), built on tests/render_ref.py: its camera rays, its
terrain and its shading; the robot is the set of world triangles p_b + R_b v of every env in the scene, and a ray is
tested against EVERY one of them (Moeller-Trumbore, two-sided), with no acceleration structure of any kind: it shares
nothing with the kernel's hierarchy, its boxes or its margins.

Moeller-Trumbore for one origin and many directions (the camera rays) or many origins and one direction (the shadow
rays) is three matrix products: with tv = o - v0,
    det = d . (e2 x e1),   u det = d . (e2 x tv),   v det = d . (tv x e1),   t det = e2 . (tv x e1) = tv . (e1 x e2),
and each right-hand factor depends on the triangle and on whichever of o, d the rays share.  Triangles are ordered
env-major, then by the caller's index; the first of equal t wins, which is the lower env, then the lower index.
"""
import numpy as np

import render_ref as RR

T_MIN, T_MAX, SHADOW_EPS = RR.T_MIN, RR.T_MAX, RR.SHADOW_EPS
RAYS = 64   # rays per block of the all-pairs test


def world_triangles(mesh, rigid, envs, dt):
    """v0, e1, e2 (M, 3) of every triangle of the envs `envs` (ascending), env-major, and per triangle its env, its
    caller's index, its body and its rgb.  mesh: dict(tri (T, 3, 3) float32, body (T,), rgb (T,))."""
    tri, body = np.asarray(mesh["tri"], np.float32).astype(dt), np.asarray(mesh["body"])
    T = len(tri)
    v = np.zeros((len(envs), T, 3, 3), dtype=dt)
    for k, n in enumerate(envs):
        for b in np.unique(body):
            row = rigid[n][b]
            R = RR.quat_rot(row[3:7], dt)
            v[k, body == b] = tri[body == b] @ R.T + row[0:3].astype(dt)
    v = v.reshape(-1, 3, 3)
    tag = dict(env=np.repeat(np.asarray(list(envs), np.int64), T), idx=np.tile(np.arange(T), len(envs)),
               body=np.tile(body.astype(np.int64), len(envs)), rgb=np.tile(np.asarray(mesh["rgb"], np.int64), len(envs)))
    return v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], tag


def _nearest(det, un, vnum, tnum, tlo, dt):
    """det, un (P, M): the determinants and u's numerators of every pair; vnum(r, k), tnum(r, k): v's and t's numerators
    of the pairs (ray r, triangle k) that pass the test on u (all pairs are tested on u; the two other numerators are
    evaluated only where that leaves a candidate).  Per ray the nearest accepted t (inf: none) and its triangle (-1); of
    equal t the lowest triangle."""
    tol = RR._tol(dt)
    D = np.abs(det)
    U = np.where(det < 0, -un, un)
    r, k = np.nonzero((D > 0) & (U >= -tol * D) & (U <= (dt(1) + tol) * D))
    s, D, U = np.sign(det[r, k]), D[r, k], U[r, k]
    V = vnum(r, k) * s
    ok = (V >= -tol * D) & (U + V <= (dt(1) + tol) * D)
    r, k, s, D = r[ok], k[ok], s[ok], D[ok]
    t = tnum(r, k) * s / D
    ok = (t > dt(tlo)) & (t <= dt(T_MAX))
    r, k, t = r[ok], k[ok], t[ok]
    best, idx = np.full(det.shape[0], np.inf, dtype=dt), np.full(det.shape[0], -1, dtype=np.int64)
    for j in np.lexsort((-k, -t, r)):   # per ray the smallest (t, k) comes last
        best[r[j]], idx[r[j]] = t[j], k[j]
    return best, idx


def cast_from_point(W, o, d, tlo, dt):
    """One origin o (3,), directions d (P, 3): nearest hit in (tlo, T_MAX] over all triangles W = (v0, e1, e2)."""
    v0, e1, e2 = W
    P = len(d)
    best, idx = np.full(P, np.inf, dtype=dt), np.full(P, -1, dtype=np.int64)
    if not len(v0):
        return best, idx
    tv = o[None, :] - v0
    A, Bu, Bv = np.cross(e2, e1), np.cross(e2, tv), np.cross(tv, e1)
    c = (e2 * Bv).sum(-1)
    for a in range(0, P, RAYS):
        q = d[a:a + RAYS]
        best[a:a + RAYS], idx[a:a + RAYS] = _nearest(q @ A.T, q @ Bu.T, lambda r, k: (q[r] * Bv[k]).sum(-1),
                                                     lambda r, k: c[k], tlo, dt)
    return best, idx


def cast_along(W, o, L, tlo, dt):
    """Origins o (P, 3), one direction L (3,): nearest hit in (tlo, T_MAX] over all triangles."""
    v0, e1, e2 = W
    P = len(o)
    best, idx = np.full(P, np.inf, dtype=dt), np.full(P, -1, dtype=np.int64)
    if not len(v0):
        return best, idx
    pv, qe, nn = np.cross(L[None, :], e2), np.cross(e1, L[None, :]), np.cross(e1, e2)
    det = (e1 * pv).sum(-1)
    cu = (v0 * pv).sum(-1)
    for a in range(0, P, RAYS):
        q = o[a:a + RAYS]
        best[a:a + RAYS], idx[a:a + RAYS] = _nearest(np.broadcast_to(det, (len(q), len(det))), q @ pv.T - cu,
                                                     lambda r, k: ((q[r] - v0[k]) * qe[k]).sum(-1),
                                                     lambda r, k: ((q[r] - v0[k]) * nn[k]).sum(-1), tlo, dt)
    return best, idx


def render_many(scene, cam, W, H, mesh, style, dtype, offsets, others=True, shadow=True):
    """scene: dict(rigid (N, 13, 13) float32, terrain None or render_ref's dict).  mesh: dict(tri, body, rgb).  others /
    shadow: T1RENDER_SCENE_OTHERS / _TERRAIN_SHADOW.  One dict per offset: render_ref_scene.render_many's keys, with tris
    (the caller's index of the triangle shown, -1) beside tri (the terrain triangle)."""
    dt = dtype
    rigid = scene["rigid"]
    K, P = len(offsets), W * H
    rays = [RR.camera_rays(cam, rigid[cam["env"], 0, 0:3], W, H, dt, off) for off in offsets]
    o = rays[0][0]
    d = np.concatenate([r[1] for r in rays], 0)
    O = np.broadcast_to(o, (K * P, 3))
    which = list(range(rigid.shape[0])) if others else [cam["env"]]
    v0, e1, e2, tag = world_triangles(mesh, rigid, which, dt)
    Wt = (v0, e1, e2)
    tp, ip = cast_from_point(Wt, o, d, T_MIN, dt)
    nprim = np.zeros((K * P, 3), dtype=dt)
    hitp = ip >= 0
    nn = np.cross(e1[ip[hitp]], e2[ip[hitp]])
    nn = RR._unit(nn)
    nn = np.where(((nn * d[hitp]).sum(-1) > 0)[:, None], -nn, nn)   # towards the ray's origin
    nprim[hitp] = nn
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
            t1, k1, n1 = RR.cast_heightfield(T, o, d[sel], bound[sel], dt)
            hit1 = k1 >= 0
            tg[sel], tri[sel] = t1, k1
            ng[sel[hit1]] = n1[hit1]
    ground = np.isfinite(tg)   # tg <= bound <= tp: the terrain wins a tie
    anyhit = ground | hitp
    depth = np.where(ground, tg, tp)
    n = np.where(ground[:, None], ng, nprim)
    pad = lambda a, fill: np.concatenate([a, [fill]])   # index -1: "no triangle"
    ids = np.where(ground, 0, np.where(hitp, 1 + pad(tag["body"], 0)[ip], -1))
    envs = np.where(ground | ~hitp, -1, pad(tag["env"], -1)[ip])
    tris = np.where(ground | ~hitp, -1, pad(tag["idx"], -1)[ip])
    hit = O + np.where(anyhit, depth, 0)[:, None] * d
    base = np.zeros((K * P, 3), dtype=dt)
    par = (np.floor(hit[:, 0]).astype(np.int64) + np.floor(hit[:, 1]).astype(np.int64)) & 1
    trgb = np.asarray(style["terrain_rgb"], dtype=np.float32).astype(dt)
    base[ground] = trgb[par[ground]]
    isp = anyhit & ~ground
    rgbv = pad(tag["rgb"], 0)[ip[isp]]
    base[isp] = np.stack([(rgbv >> s) & 255 for s in (0, 8, 16)], 1).astype(dt) * (dt(1) / dt(255))
    _, nl, L = RR._shade(style, base, n, np.ones(K * P, dtype=dt), dt)
    so = hit + dt(SHADOW_EPS) * n
    faces = anyhit & (nl > 0)
    by_robot = np.zeros(K * P, dtype=bool)
    by_robot[faces] = np.isfinite(cast_along(Wt, so[faces], L, 0.0, dt)[0])
    by_terrain = np.zeros(K * P, dtype=bool)
    if shadow and T is not None:
        import render_ref_scene as RS
        by_terrain = RS.terrain_shadow(T, so, L, faces, dt)
    lit = ~(by_robot | by_terrain)
    value, _, _ = RR._shade(style, base, n, lit.astype(dt), dt)
    sky = np.asarray(style["sky_rgb"], dtype=np.float32).astype(dt)
    s = dt(0.5) * (d[:, 2] + dt(1))
    value = np.where(anyhit[:, None], value, sky[0][None] + s[:, None] * (sky[1] - sky[0])[None])

    def to8(v):
        return np.floor(np.clip(v, 0, 1) * dt(255) + dt(0.5)).astype(np.uint8)
    rgb = to8(value)
    alt = to8(RR._shade(style, base, n, (~lit).astype(dt), dt)[0])   # the colour with the other lit decision
    out = []
    for k in range(K):
        q = slice(k * P, (k + 1) * P)
        out.append(dict(ids=ids[q].reshape(H, W), envs=envs[q].reshape(H, W), tris=tris[q].reshape(H, W),
                        depth=np.where(anyhit, depth, np.inf)[q].reshape(H, W),
                        lit=(lit | ~anyhit)[q].reshape(H, W), tri=np.where(ground, tri, -1)[q].reshape(H, W),
                        rgb=rgb[q].reshape(H, W, 3), rgb_other=alt[q].reshape(H, W, 3),
                        nl=np.where(anyhit, nl, 0)[q].reshape(H, W), hit=hit[q].reshape(H, W, 3),
                        by_robot=by_robot[q].reshape(H, W), by_terrain=by_terrain[q].reshape(H, W)))
    return out


def render(scene, cam, W, H, mesh, style, dtype=np.float64, others=True, shadow=True):
    return render_many(scene, cam, W, H, mesh, style, dtype, ((0.0, 0.0),), others, shadow)[0]


def reference(scene, cam, W, H, mesh, style, others=True, shadow=True):
    """The fp64 image plus its ambiguity mask: a pixel is ambiguous when the rays through its centre and through the four
    points render_ref.AMBIG_OFFSETS pixels beside it do not all give the same id, env, triangle, lit flag and terrain
    triangle."""
    ref, *rest = render_many(scene, cam, W, H, mesh, style, np.float64, ((0.0, 0.0),) + RR.AMBIG_OFFSETS, others, shadow)
    amb = np.zeros((H, W), dtype=bool)
    for r in rest:
        amb |= (r["ids"] != ref["ids"]) | (r["lit"] != ref["lit"]) | (r["tri"] != ref["tri"]) | \
            (r["envs"] != ref["envs"]) | (r["tris"] != ref["tris"])
    ref["ambiguous"] = amb
    return ref


def compare(ref, rgba, depth, ids, envs, tris, depth_atol, depth_rtol):
    """render_ref_scene.compare, and the tris plane exactly, on the non-ambiguous pixels.  Returns the worst depth
    errors."""
    import render_ref_scene as RS
    out = RS.compare(ref, rgba, depth, ids, envs, depth_atol, depth_rtol)
    bad = ~ref["ambiguous"] & (tris != ref["tris"])
    assert not bad.any(), ("tris differ", np.argwhere(bad)[:5], tris[bad][:5], ref["tris"][bad][:5])
    return out
