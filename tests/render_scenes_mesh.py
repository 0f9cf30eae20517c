"""The scenes of the t1render_mesh tests as pure data: small synthetic meshes (an icosphere, an open quad, boxes, the
two ankle STLs of tests/golden/t1_robot), the poses they are drawn in, the cameras, and a robot description whose 22
missing mesh files are written as 12-triangle boxes.  tests/test_render_mesh_host.py examines them without a device
(the ambiguity cap), tests/test_gpu_render_mesh.py compares the kernel's images with tests/render_ref_mesh.py."""
import functools
import os
import re
import shutil
import struct

import numpy as np

import render_scenes as S
import render_scenes_multi as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROBOT = os.path.join(HERE, "golden", "t1_robot")
AMBIGUOUS_CAP = 0.01


# ---- meshes
def box_tris(lo, hi):
    """The 12 triangles of the box lo .. hi, outward wound: (12, 3, 3) float32."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    c = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])   # corner k: bit a picks hi on axis a
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = [[c[q[0]], c[q[i]], c[q[i + 1]]] for q in quads for i in (1, 2)]
    return np.array(t, dtype=np.float32)


def icosphere(radius, centre=(0.0, 0.0, 0.0)):
    """An icosahedron subdivided once: 80 triangles on the sphere, (80, 3, 3) float32."""
    p = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
                  (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)], float)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v /= np.linalg.norm(v[0])
    out = []
    for a, b, c in f:
        A, B, C = v[a], v[b], v[c]
        ab, bc, ca = [(x + y) / np.linalg.norm(x + y) for x, y in ((A, B), (B, C), (C, A))]
        out += [(A, ab, ca), (B, bc, ab), (C, ca, bc), (ab, bc, ca)]
    return (np.array(out) * radius + np.asarray(centre, float)).astype(np.float32)


def write_stl(path, tri):
    """(T, 3, 3) as a binary STL (the normals left zero)."""
    tri = np.asarray(tri, dtype="<f4")
    with open(path, "wb") as f:
        f.write(b"\0" * 80 + struct.pack("<I", len(tri)))
        for t in tri:
            f.write(b"\0" * 12 + t.tobytes() + b"\0\0")


@functools.lru_cache(maxsize=None)
def ankle(side):
    """The ankle-roll STL of tests/golden/t1_robot ('L' or 'R'): (about 2000, 3, 3) float32, link frame."""
    from ti5_isaacgym_amd.utils.urdf import load_stl
    return load_stl(os.path.join(ROBOT, "meshes", side + "_ANKLE_R_S.STL")).reshape(-1, 3, 3).astype(np.float32)


def mesh_of(parts):
    """parts: [(body, tri (T, 3, 3), rgb)] -> dict(tri, body, rgb), the caller's order being the parts' order."""
    tri = np.concatenate([np.asarray(p[1], np.float32).reshape(-1, 3, 3) for p in parts])
    body = np.concatenate([np.full(len(np.asarray(p[1]).reshape(-1, 3, 3)), p[0], np.int32) for p in parts])
    rgb = np.concatenate([np.full(len(np.asarray(p[1]).reshape(-1, 3, 3)), p[2], np.uint32) for p in parts])
    for a in (tri, body, rgb):
        a.setflags(write=False)
    return dict(tri=tri, body=body, rgb=rgb)


# ---- a robot description with every mesh file present
def synth_robot(dst, box=None):
    """Copies the fixture URDF and the two ankle STLs into dst/urdf and dst/meshes and writes every other mesh file the
    URDF names as a binary STL of `box` (default: a 12-triangle box).  Returns the URDF's path."""
    os.makedirs(os.path.join(dst, "urdf"), exist_ok=True)
    os.makedirs(os.path.join(dst, "meshes"), exist_ok=True)
    urdf = os.path.join(dst, "urdf", "t1.urdf")
    shutil.copy(os.path.join(ROBOT, "urdf", "t1.urdf"), urdf)
    text = re.sub(r"<!--.*?-->", "", open(urdf).read(), flags=re.S)
    for name in sorted(set(re.findall(r'filename="\.\./meshes/([^"]+)"', text))):
        src = os.path.join(ROBOT, "meshes", name)
        if os.path.exists(src):
            shutil.copy(src, os.path.join(dst, "meshes", name))
        else:
            write_stl(os.path.join(dst, "meshes", name), box_tris((-0.04, -0.03, -0.05), (0.04, 0.03, 0.05)) if box is None
                      else box)
    return urdf


# ---- scene 1: the plane, one env, every leaf-size edge
SIZE1 = (50, 37)   # no multiple of the tile in either axis
COLORS = (0x3C3CDC, 0xD28C32, 0x50B43C, 0x32C8E6, 0xC040C0, 0x40C0C0, 0x909090)


@functools.lru_cache(maxsize=None)
def scene1():
    """dict(mesh, rigid (1, 13, 13), cam, zero (the zero-area triangle's index), quad (the quad's two)).  Body 0: an
    80-triangle icosphere; body 6: an open quad whose back faces the camera; body 12: the right ankle STL; bodies 1
    to 4: 1, 4, 5 and 9 random triangles; body 5 and the rest: nothing, but body 7 carries one zero-area triangle
    (three points on a line) that spans the view 0.6 m in front of the camera."""
    rng = np.random.default_rng(20260301)
    rs = np.zeros((1, 13, 13), dtype=np.float32)
    where = {0: (0.0, 0.0, 0.95), 1: (0.1, -0.75, 0.9), 2: (0.1, 0.75, 0.9), 3: (0.2, -0.8, 0.35), 4: (0.2, 0.85, 0.35),
             6: (0.5, 0.35, 0.3), 12: (0.6, -0.3, 0.3), 7: (1.6, 0.0, 0.8)}
    for b in range(13):
        q = rng.standard_normal(4)
        rs[0, b, 0:3] = where.get(b, (0.0, 0.0, 5.0))
        rs[0, b, 3:7] = q / np.linalg.norm(q)
    rs[0, 1, 3:7] = (0.0, 0.0, 0.0, 1.0)
    rs[0, 6, 3:7] = (0.0, 0.0, 0.0, 1.0)   # the quad keeps its orientation: wound so that its normal is -x, away from the eye
    rs[0, 7, 3:7] = (0.0, 0.0, 0.0, 1.0)
    quad = np.array([[(0, -0.2, -0.15), (0, 0.2, 0.15), (0, 0.2, -0.15)], [(0, -0.2, -0.15), (0, -0.2, 0.15), (0, 0.2, 0.15)]])
    parts = [(0, icosphere(0.22), COLORS[0])]
    for k, (b, n) in enumerate(((1, 1), (2, 4), (3, 5), (4, 9))):
        c = rng.uniform(-0.12, 0.12, (n, 1, 3))
        t = c + rng.uniform(-0.15, 0.15, (n, 3, 3))
        if n == 1:   # the single triangle faces the camera whatever was drawn
            t = np.array([[(0.0, -0.15, -0.12), (0.0, 0.15, -0.12), (0.0, 0.0, 0.16)]])
        parts.append((b, t, COLORS[1 + k % 3]))
    parts.append((6, quad, COLORS[4]))
    parts.append((7, np.array([[(0, -2.0, 0), (0, 0.0, 0), (0, 2.0, 0)]]), COLORS[5]))
    parts.append((12, ankle("R") * 2.0, COLORS[3]))   # twice its size: a pixel still holds a few of its triangles
    mesh = mesh_of(parts)
    nq = 80 + 1 + 4 + 5 + 9
    cam = dict(env=0, follow=False, eye=(2.2, 0.0, 0.9), target=(0.0, 0.0, 0.55), up=(0.0, 0.0, 1.0), vfov=0.9)
    rs.setflags(write=False)
    return dict(mesh=mesh, rigid=rs, cam=cam, quad=(nq, nq + 1), zero=nq + 2)


def style():
    from ti5_isaacgym_amd.utils import render as R
    return dict(R.STYLE)


@functools.lru_cache(maxsize=None)
def reference1():
    import render_ref_mesh as RM
    s = scene1()
    return RM.reference(dict(rigid=s["rigid"], terrain=None), s["cam"], SIZE1[0], SIZE1[1], s["mesh"], style(), False, False)


# ---- scene 3: the eight robots of render_scenes_multi in the stair pit
SIZE3 = (48, 32)


@functools.lru_cache(maxsize=None)
def mesh3():
    """The two ankle STLs on the feet (twice their size) and a box on every other body."""
    rng = np.random.default_rng(20260302)
    parts = []
    for b in range(13):
        if b == 6:
            parts.append((b, ankle("L") * 2.0, COLORS[3]))
        elif b == 12:
            parts.append((b, ankle("R") * 2.0, COLORS[3]))
        else:
            h = rng.uniform(0.05, 0.16, 3)
            c = rng.uniform(-0.05, 0.05, 3)
            parts.append((b, box_tris(c - h, c + h), COLORS[b % 3]))
    return mesh_of(parts)


def cameras3():
    """Camera A of render_scenes_multi with a narrower field of view: from 5 m out a pixel then holds a few of the ankle
    meshes' triangles, and the reference's ambiguous share stays under the cap (0.6 %; 1.7 % at A's own 0.8 rad)."""
    return [M._look(0, (3.5, 1.5, 3.5), (0.0, 0.0, 0.2), vfov=0.45)]


@functools.lru_cache(maxsize=None)
def reference3(cam):
    import render_ref_mesh as RM
    return RM.reference(dict(rigid=M.poses(), terrain=S.trimesh_terrain()), cameras3()[cam], SIZE3[0], SIZE3[1], mesh3(),
                        M.style(), True, True)


# ---- the crowd of the brute-equality test: 200 envs on the plane
CROWD_ENVS = 200
CROWD_SIZE = (48, 32)
ARM, CASTER = 150, 151   # out of view, an arm-like box reaching into it; out of view, its shadow in it


@functools.lru_cache(maxsize=None)
def crowd_mesh():
    """A small box on every body and, on the base, an arm-like box 1.9 m long along the body's +y."""
    rng = np.random.default_rng(20260303)
    parts = [(0, box_tris((-0.1, -0.1, -0.15), (0.1, 0.1, 0.15)), COLORS[0]),
             (0, box_tris((-0.03, 0.1, 0.05), (0.03, 2.0, 0.11)), COLORS[4])]
    for b in range(1, 13):
        h = rng.uniform(0.04, 0.08, 3)
        parts.append((b, box_tris(-h, h), COLORS[1 + b % 3]))
    return mesh_of(parts)


ARM_BOX = (12, 24)   # the arm box's triangles in crowd_mesh()


def crowd_camera():
    return dict(env=0, follow=False, eye=(6.0, 0.0, 1.6), target=(0.0, 0.0, 0.6), up=(0.0, 0.0, 1.0), vfov=0.7)


@functools.lru_cache(maxsize=None)
def crowd_poses():
    """(200, 13, 13): envs 0..149 within 2.5 m of the origin; ARM stands well beside the view, all its bodies at one
    point, so that the arm box alone reaches into the picture; CASTER hangs 6 m up along the light from a ground point
    in view; the rest on a grid far away."""
    from ti5_isaacgym_amd.utils import render as R
    rng = np.random.default_rng(20260304)
    rs = np.zeros((CROWD_ENVS, 13, 13), dtype=np.float32)
    for n in range(CROWD_ENVS):
        if n < 150:
            r, a = 2.5 * np.sqrt(rng.uniform()), rng.uniform(0, 2 * np.pi)
            rs[n] = M._robot(rng, r * np.cos(a), r * np.sin(a))
        else:
            rs[n] = M._robot(rng, 80.0 + 2.0 * (n % 10), 50.0 + 2.0 * (n // 10))
    # the camera looks down -x from x = 6 with a half width of atan(tan(0.35) * 1.5) = 0.5 rad: at x = 3 the view's
    # edge is 1.64 m from the axis.  All of ARM's bodies sit at (3, -3.3, 0.8) with identity quaternions: whatever is
    # drawn within 0.8 m of a body's origin (every primitive of the product is) ends 0.8 m outside the view, and so
    # does a sphere around it; the arm box runs along +y from y = -3.2 to y = -1.3, across the edge.
    # primitives_cull_arm() below computes that a bound taken from the primitives drops ARM from the arm's own tiles.
    rs[ARM] = 0.0
    rs[ARM, :, 0:3] = (3.0, -3.3, 0.8)
    rs[ARM, :, 6] = 1.0
    L = np.array(R.STYLE["light"]) / np.linalg.norm(R.STYLE["light"])
    p = np.array([3.5, 0.5, 0.0]) + (6.0 / L[2]) * L
    rs[CASTER] = M._robot(rng, p[0], p[1], z0=5.9)
    rs.setflags(write=False)
    return rs


# ---- t1render_scene's culling of one robot, recomputed: what a bound taken from the primitives would do
def primitive_sphere(prims, rigid):
    """k_scene_bounds for one env (rigid (13, 13)): centre and padded radius of the sphere around the posed primitives'
    bounding box (a box by the sphere of its half diagonal, a capsule by its ends and radius)."""
    import render_ref as RR
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for p in prims:
        row = rigid[p["body"]].astype(np.float64)
        R, pos = RR.quat_rot(row[3:7], np.float64), row[0:3]
        a, b = pos + R @ np.asarray(p["a"], float), np.asarray(p["b"], float)
        if p["kind"] == 0:
            pts, r = [a], float(np.linalg.norm(b))
        else:
            pts, r = [a, pos + R @ b], abs(float(p["r"]))
        for q in pts:
            lo, hi = np.minimum(lo, q - r), np.maximum(hi, q + r)
    c = 0.5 * (lo + hi)
    return c, 0.5 * np.linalg.norm(hi - lo) * 1.0001 + 4e-3 + 4e-6 * np.abs(c).sum()


def tile_planes(cam, W, H, tx, ty, tile=16):
    """make_frustum for tile (tx, ty) of a fixed camera: the eye and the four inward unit normals."""
    eye, tgt, up = (np.asarray(cam[k], float) for k in ("eye", "target", "up"))
    f = (tgt - eye) / np.linalg.norm(tgt - eye)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    th = np.tan(0.5 * cam["vfov"])
    r, u = th * W / H * r, th * u
    x0, x1 = 2.0 * tx * tile / W - 1.0, 2.0 * (tx * tile + tile) / W - 1.0
    y0, y1 = 1.0 - 2.0 * (ty * tile + tile) / H, 1.0 - 2.0 * ty * tile / H
    n = [r - x0 * (r @ r) * f, x1 * (r @ r) * f - r, u - y0 * (u @ u) * f, y1 * (u @ u) * f - u]
    return eye, [v / np.linalg.norm(v) for v in n]


def capsule_outside(eye, normals, a, b, r):
    """capsule_outside of the kernels: the capsule of radius r around a .. b lies wholly outside one plane."""
    qa, qb = a - eye, b - eye
    ma, mb = -(r + 8e-6 * np.abs(qa).sum()), -(r + 8e-6 * np.abs(qb).sum())
    return any(qa @ n < ma and qb @ n < mb for n in normals)


def primitives_cull_arm(tiles):
    """True when t1render_scene's bound of ARM -- the sphere around its primitives, swept along the shadow segment down
    to the scene's floor -- lies wholly outside every one of the tiles (tx, ty) of the crowd camera's picture: a
    culling bound taken from the primitives, not from the mesh, drops ARM there."""
    from ti5_isaacgym_amd.utils import render as R
    prims, poses = R.robot_primitives(), crowd_poses()
    spheres = [primitive_sphere(prims, poses[n]) for n in range(CROWD_ENVS)]
    z_floor = min([-1e-3] + [c[2] - r for c, r in spheres])   # scene_floor: the plane's z_bot, the lowest sphere bottom
    L = np.array(R.STYLE["light"], float)
    L /= np.linalg.norm(L)
    c, r = spheres[ARM]
    s = min(200.0, max((c[2] + r - z_floor) / L[2], 0.0)) * 1.0001 + 1e-2   # shadow_end
    w, h = CROWD_SIZE
    return all(capsule_outside(*tile_planes(crowd_camera(), w, h, tx, ty), c, c - s * L, r) for tx, ty in tiles)
