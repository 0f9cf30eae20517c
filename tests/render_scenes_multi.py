"""The scenes of the t1render_scene tests as pure data: eight robots in and around the 0.1 m-step stair pit of the small
trimesh field of tests/render_scenes.py, two cameras over them under a low light (under the default one the shadow of a
0.1 m riser is less than a pixel), and the synthetic crowds of the culling test.  tests/test_render_scene_host.py
examines them without a device, tests/test_gpu_render_scene.py writes the poses into envs and compares the kernel's
images with tests/render_ref_scene.py."""
import functools

import numpy as np

import render_scenes as S

NUM_ENVS = 8
CENTRE = np.array([44.173, 28.357])   # the stair pit of row 5, column 3
# the cluster around env 0; env 6 far away on the flat, env 7 at the cluster's edge
OFFSETS = np.array([[0, 0], [1.3, 0.4], [-0.9, 1.5], [0.6, -1.6], [-1.7, -0.8], [2.3, 1.9], [-40, -24], [5.5, 0.3]])
BASES = CENTRE + OFFSETS
LIGHT = (0.90, 0.30, 0.25)
SIZE = (64, 48)
VFOV = 0.8


def style():
    from ti5_isaacgym_amd.utils import render as R
    return dict(R.STYLE, light=LIGHT)


@functools.lru_cache(maxsize=None)
def poses():
    """(8, 13, 13) float32 rigid_state rows, drawn as render_scenes.trimesh_poses() draws its own."""
    T = S.trimesh_terrain()
    rng = np.random.default_rng(20260101)
    rs = np.zeros((NUM_ENVS, 13, 13), dtype=np.float32)
    for n in range(NUM_ENVS):
        for b in range(13):
            x, y = BASES[n] + (rng.uniform(-0.5, 0.5, 2) if b else 0.0)
            q = rng.standard_normal(4)
            rs[n, b, 0:3] = (x, y, S._ground(T, x, y) + rng.uniform(0.0, 1.2))
            rs[n, b, 3:7] = q / np.linalg.norm(q)
    rs.setflags(write=False)
    return rs


def _look(env, eye_off, tgt_off, up=(0.0, 0.0, 1.0), vfov=VFOV):
    b = poses()[0, 0, 0:3].astype(np.float64)   # both cameras are placed from env 0's base
    return dict(env=env, follow=False, eye=tuple(np.float32(b + eye_off).tolist()),
                target=tuple(np.float32(b + tgt_off).tolist()), up=up, vfov=vfov)


def cameras():
    return [_look(0, (3.5, 1.5, 3.5), (0.0, 0.0, 0.2)), _look(3, (-2.0, -3.2, 4.2), (0.3, 0.0, 0.3))]


FLAG_CASES = {"others": (True, False), "shadow": (False, True), "both": (True, True)}


@functools.lru_cache(maxsize=None)
def reference_of(cam, case="both"):
    """render_ref_scene.reference of camera `cam` (0: A, 1: B) with the product's primitives; computed once, shared."""
    import render_ref_scene as RS
    from ti5_isaacgym_amd.utils import render as R
    others, shadow = FLAG_CASES[case]
    return RS.reference(dict(rigid=poses(), terrain=S.trimesh_terrain()), cameras()[cam], SIZE[0], SIZE[1],
                        R.robot_primitives(), style(), others, shadow)


# ---- the culling test's crowd on the plane: 1000 envs
CROWD_ENVS = 1000
CROWD_CENTRE = np.array([12.0, -7.0])
CROWD_SIZE = (48, 32)


def _robot(rng, x, y, z0=0.0):
    """13 rows around (x, y): bodies within 0.4 m, 0.1 to 1.2 m above z0, random unit quaternions."""
    rs = np.zeros((13, 13), dtype=np.float32)
    for b in range(13):
        dx, dy = rng.uniform(-0.4, 0.4, 2) if b else (0.0, 0.0)
        q = rng.standard_normal(4)
        rs[b, 0:3] = (x + dx, y + dy, z0 + rng.uniform(0.1, 1.2))
        rs[b, 3:7] = q / np.linalg.norm(q)
    return rs


def crowd_cameras():
    c = CROWD_CENTRE
    eye = (c[0] + 7.0, c[1] + 3.0, 2.5)   # 8 m from the cluster's centre at 0.6 m
    return [dict(env=0, follow=False, eye=eye, target=(c[0], c[1], 0.6), up=(0.0, 0.0, 1.0), vfov=0.9),
            dict(env=1, follow=False, eye=(c[0], c[1], 30.0), target=(c[0], c[1], 0.0), up=(1.0, 0.0, 0.0), vfov=0.5)]


# named envs of the crowd
TWIN_LO, TWIN_HI, AT_EYE, FAR, BEHIND, CASTER = 400, 733, 401, 402, 403, 404


@functools.lru_cache(maxsize=None)
def crowd_poses():
    """(1000, 13, 13): envs 0..299 within 3 m of CROWD_CENTRE (more robots than one LDS batch holds, by far); two envs
    with identical rows in view (TWIN_LO < TWIN_HI); one whose base box holds camera 0's eye; one 10 km away; one
    behind camera 0; one beside camera 0's view whose shadow falls into it; the rest on a 2 m grid far from the
    cameras' view."""
    rng = np.random.default_rng(20260102)
    c, eye = CROWD_CENTRE, np.array(crowd_cameras()[0]["eye"])
    rs = np.zeros((CROWD_ENVS, 13, 13), dtype=np.float32)
    for n in range(CROWD_ENVS):
        if n < 300:
            r, a = 3.0 * np.sqrt(rng.uniform()), rng.uniform(0, 2 * np.pi)
            rs[n] = _robot(rng, c[0] + r * np.cos(a), c[1] + r * np.sin(a))
        else:
            k = n - 300
            rs[n] = _robot(rng, 60.0 + 2.0 * (k % 27), 40.0 + 2.0 * (k // 27))
    rs[TWIN_LO] = _robot(rng, c[0] + 4.4, c[1] + 0.6)   # between the cluster and camera 0, 3 m from its eye
    rs[TWIN_HI] = rs[TWIN_LO]
    rs[AT_EYE] = _robot(rng, eye[0], eye[1])
    rs[AT_EYE, 0, 0:3] = eye                              # the base box (body 0) around the eye
    rs[AT_EYE, 0, 3:7] = (0, 0, 0, 1)
    rs[FAR] = _robot(rng, 1.0e4, -1.0e4)
    back = eye[:2] + 3.0 * (eye[:2] - c) / np.linalg.norm(eye[:2] - c)
    rs[BEHIND] = _robot(rng, back[0], back[1])
    rs[CASTER] = caster_rows(rng)
    rs.setflags(write=False)
    return rs


def caster_rows(rng):
    """A robot 6 to 7 m above the ground, displaced along the light from the ground point 4 m in front of camera 0, so
    that its shadow falls there (where a pixel is 0.14 m wide) while the robot itself is far above the camera's view."""
    from ti5_isaacgym_amd.utils import render as R
    L = np.array(R.STYLE["light"]) / np.linalg.norm(R.STYLE["light"])
    h = 6.0
    eye = np.array(crowd_cameras()[0]["eye"])[:2]
    g = eye + 4.0 * (CROWD_CENTRE - eye) / np.linalg.norm(CROWD_CENTRE - eye)
    p = np.array([g[0], g[1], 0.0]) + (h / L[2]) * L
    return _robot(rng, p[0], p[1], z0=h - 0.1)


def crowd_subset():
    """Nine envs of the crowd for the comparison with the reference: the twins, the caster, and six of the cluster."""
    return [0, 1, 2, 3, 4, 5, TWIN_LO, CASTER, TWIN_HI]
