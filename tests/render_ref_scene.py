"""The numpy reference of t1render_scene (include/t1render.h), built on tests/render_ref.py: the same rays, the same
primitive and height-field intersections, over a scene that holds every env's robot and in which the height field
casts shadows.

The primitive set is the concatenation of render_ref.world_prims(prims, rigid[n]) over the envs, env-major, with an env
tag per primitive: render_ref.cast_prims keeps the first of equal entries, which is the lower env, then the lower
primitive.  The terrain's shadow is render_ref.cast_heightfield from hit + 1e-3 n towards the light, once per hit that
faces the light.
"""
import numpy as np

import render_ref as RR

T_MIN, T_MAX, SHADOW_EPS = RR.T_MIN, RR.T_MAX, RR.SHADOW_EPS


def scene_prims(prims, rigid, envs, dt):
    """The world primitives of the envs `envs` (ascending) and each one's env tag."""
    wp, tag = [], []
    for n in envs:
        w = RR.world_prims(prims, rigid[n], dt)
        wp += w
        tag += [n] * len(w)
    return wp, np.array(tag + [-1], dtype=np.int64)   # [-1]: the tag of "no primitive"


def terrain_shadow(T, origins, L, need, dt):
    """need (P,) bool: True where the ray from origins[p] along L meets the height field at t in (T_MIN, T_MAX]."""
    out = np.zeros(len(origins), dtype=bool)
    tmax = np.array([T_MAX], dtype=dt)
    for p in np.flatnonzero(need):
        t, _, _ = RR.cast_heightfield(T, origins[p], L[None, :], tmax, dt)
        out[p] = np.isfinite(t[0])
    return out


def render_many(scene, cam, W, H, prims, style, dtype, offsets, others=True, shadow=True):
    """scene: dict(rigid (N, 13, 13) float32, terrain None or render_ref's dict).  others / shadow: the flags
    T1RENDER_SCENE_OTHERS / _TERRAIN_SHADOW.  One dict per offset: render_ref.render's keys and envs, by_robot (a
    primitive shadows the pixel), by_own (a primitive of the camera's env does), by_terrain (the height field does; only
    evaluated where the surface faces the light)."""
    dt = dtype
    rigid = scene["rigid"]
    K, P = len(offsets), W * H
    rays = [RR.camera_rays(cam, rigid[cam["env"], 0, 0:3], W, H, dt, off) for off in offsets]
    o = rays[0][0]
    d = np.concatenate([r[1] for r in rays], 0)
    O = np.broadcast_to(o, (K * P, 3))
    which = range(rigid.shape[0]) if others else [cam["env"]]
    wp, tag = scene_prims(prims, rigid, which, dt)
    tp, ip, nprim = RR.cast_prims(wp, O, d, T_MIN, dt)
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
    anyhit = ground | (ip >= 0)
    depth = np.where(ground, tg, tp)
    n = np.where(ground[:, None], ng, nprim)
    bodies = np.array([w["body"] for w in wp] + [0])
    ids = np.where(ground, 0, np.where(ip >= 0, 1 + bodies[ip], -1))
    envs = np.where(ground, -1, tag[ip])
    hit = O + np.where(anyhit, depth, 0)[:, None] * d
    base = np.zeros((K * P, 3), dtype=dt)
    par = (np.floor(hit[:, 0]).astype(np.int64) + np.floor(hit[:, 1]).astype(np.int64)) & 1
    trgb = np.asarray(style["terrain_rgb"], dtype=np.float32).astype(dt)
    base[ground] = trgb[par[ground]]
    rgbs = np.array([[(w["rgb"] >> s) & 255 for s in (0, 8, 16)] for w in wp] + [[0, 0, 0]], dtype=dt) * (dt(1) / dt(255))
    isp = anyhit & ~ground
    base[isp] = rgbs[ip[isp]]
    _, nl, L = RR._shade(style, base, n, np.ones(K * P, dtype=dt), dt)
    so = hit + dt(SHADOW_EPS) * n
    LL = np.broadcast_to(L, (K * P, 3))
    faces = anyhit & (nl > 0)
    ts = RR.cast_prims(wp, so, LL, 0.0, dt)[0]
    by_robot = np.isfinite(ts) & faces
    own, _ = scene_prims(prims, rigid, [cam["env"]], dt)
    by_own = np.isfinite(RR.cast_prims(own, so, LL, 0.0, dt)[0]) & faces
    by_terrain = np.zeros(K * P, dtype=bool)
    if shadow and T is not None:
        by_terrain = terrain_shadow(T, so, L, faces, dt)
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
        out.append(dict(ids=ids[q].reshape(H, W), envs=envs[q].reshape(H, W),
                        depth=np.where(anyhit, depth, np.inf)[q].reshape(H, W),
                        lit=(lit | ~anyhit)[q].reshape(H, W), tri=np.where(ground, tri, -1)[q].reshape(H, W),
                        rgb=rgb[q].reshape(H, W, 3), rgb_other=alt[q].reshape(H, W, 3),
                        nl=np.where(anyhit, nl, 0)[q].reshape(H, W), hit=hit[q].reshape(H, W, 3),
                        by_robot=by_robot[q].reshape(H, W), by_own=by_own[q].reshape(H, W),
                        by_terrain=by_terrain[q].reshape(H, W)))
    return out


def render(scene, cam, W, H, prims, style, dtype=np.float64, others=True, shadow=True):
    return render_many(scene, cam, W, H, prims, style, dtype, ((0.0, 0.0),), others, shadow)[0]


def reference(scene, cam, W, H, prims, style, others=True, shadow=True):
    """The fp64 image plus its ambiguity mask: as render_ref.reference, and a pixel is also ambiguous when the five rays
    do not all show the same env."""
    ref, *rest = render_many(scene, cam, W, H, prims, style, np.float64, ((0.0, 0.0),) + RR.AMBIG_OFFSETS, others, shadow)
    amb = np.zeros((H, W), dtype=bool)
    for r in rest:
        amb |= (r["ids"] != ref["ids"]) | (r["lit"] != ref["lit"]) | (r["tri"] != ref["tri"]) | (r["envs"] != ref["envs"])
    ref["ambiguous"] = amb
    return ref


def coincident(scene, cam, W, H, prims, tol):
    """Where the fp64 centre ray enters primitives of more than one (id, env) within tol of its nearest entry: the mask
    (H, W) and, per such pixel, the set of those (id, env).  A posed robot has such places by construction: the capsules
    of two adjacent links end in the same joint sphere, posed once through each body."""
    rigid = scene["rigid"]
    o, d = RR.camera_rays(cam, rigid[cam["env"], 0, 0:3], W, H, np.float64)
    O = np.broadcast_to(o, d.shape)
    wp, tag = scene_prims(prims, rigid, range(rigid.shape[0]), np.float64)
    ts = np.stack([(RR._box_entry(O, d, p["c"], p["R"], p["h"], np.float64) if p["kind"] == 0 else
                    RR._capsule_entry(O, d, p["a"], p["b"], p["r"], np.float64))[0] for p in wp])
    ts = np.where((ts > T_MIN) & (ts <= T_MAX), ts, np.inf)
    near = np.isfinite(ts) & (ts <= ts.min(0)[None, :] + tol)
    key = np.array([(1 + p["body"]) * 100000 + n for p, n in zip(wp, tag[:-1])])
    sets = {}
    for q in np.flatnonzero(near.sum(0) > 1):
        ks = set(key[near[:, q]].tolist())
        if len(ks) > 1:
            sets[(q // W, q % W)] = {(k // 100000, k % 100000) for k in ks}
    mask = np.zeros((H, W), dtype=bool)
    for i, j in sets:
        mask[i, j] = True
    return mask, sets


def compare(ref, rgba, depth, ids, envs, depth_atol, depth_rtol):
    """render_ref.compare, and the envs plane exactly, on the non-ambiguous pixels.  Returns the worst depth errors."""
    out = RR.compare(ref, rgba, depth, ids, depth_atol, depth_rtol)
    bad = ~ref["ambiguous"] & (envs != ref["envs"])
    assert not bad.any(), ("envs differ", np.argwhere(bad)[:5], envs[bad][:5], ref["envs"][bad][:5])
    return out
