"""The renderer tests' scenes as pure data: the small trimesh field of the golden scenarios (6 x 4 sub-terrains,
border 5 m) with proportions that give flat, rough, sloped and stair cells, seeded body poses for five envs, and the
cameras.  tests/test_render_host.py examines them without a device (the ambiguity cap), tests/test_gpu_render.py writes
the poses into an env built with the same configuration and compares the kernel's images to tests/render_ref.py."""
import functools

import numpy as np

SEED = 3
NUM_ENVS = 5
# positional, as Terrain.make_terrain reads them: flat, rough flat, rough slope (down, up), slope (down, up), stairs
# (down, up), discrete, wave.  With the curriculum layout the four columns are flat, rough flat, slope and stairs.
PROPORTIONS = [0.1, 0.2, 0.1, 0.1, 0.1, 0.1, 0.15, 0.15, 0.0, 0.0]


def terrain_hook(cfg):
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 6, 4, 5
    cfg.terrain.terrain_proportions = list(PROPORTIONS)


@functools.lru_cache(maxsize=None)
def trimesh_terrain():
    """dict(h int16 (rows, cols), hscale, vscale, border): what make_t1_env(mesh_type='trimesh', seed=SEED,
    cfg_hook=terrain_hook) builds (the GPU test checks that its env holds the same samples)."""
    import copy
    from ti5_isaacgym_amd import task_registry
    from ti5_isaacgym_amd.utils.helpers import set_seed
    from ti5_isaacgym_amd.utils.terrain import Terrain
    cfg, _ = task_registry.get_cfgs("t1_dh_stand")
    cfg = copy.deepcopy(cfg)
    cfg.terrain.mesh_type = "trimesh"
    terrain_hook(cfg)
    set_seed(SEED)
    t = Terrain(cfg.terrain, NUM_ENVS)
    h = np.array(t.heightsamples, dtype=np.int16)
    h.setflags(write=False)
    return dict(h=h, hscale=float(cfg.terrain.horizontal_scale), vscale=float(cfg.terrain.vertical_scale),
                border=float(cfg.terrain.border_size))


# base positions (x, y): one per column type, env 2 near the field's -x edge, env 4 on the stairs; off the grid lines
BASES = np.array([[4.037, 4.213], [12.341, 12.127], [-3.563, 10.283], [20.419, 20.731], [28.173, 28.357]])


def _ground(T, x, y):
    i = int(np.clip(np.floor((x + T["border"]) / T["hscale"]), 0, T["h"].shape[0] - 1))
    j = int(np.clip(np.floor((y + T["border"]) / T["hscale"]), 0, T["h"].shape[1] - 1))
    return float(T["h"][i, j]) * T["vscale"]


@functools.lru_cache(maxsize=None)
def trimesh_poses():
    """(NUM_ENVS, 13, 13) float32 rigid_state rows: bodies within 0.5 m of the env's base in x and y and 0 to 1.2 m
    above the local terrain, random unit quaternions, zero velocities."""
    T = trimesh_terrain()
    rng = np.random.default_rng(20240611)
    rs = np.zeros((NUM_ENVS, 13, 13), dtype=np.float32)
    for n in range(NUM_ENVS):
        for b in range(13):
            x, y = BASES[n] + (rng.uniform(-0.5, 0.5, 2) if b else 0.0)
            q = rng.standard_normal(4)
            rs[n, b, 0:3] = (x, y, _ground(T, x, y) + rng.uniform(0.0, 1.2))
            rs[n, b, 3:7] = q / np.linalg.norm(q)
    rs.setflags(write=False)
    return rs


def _look(n, eye_off, tgt_off, up=(0.0, 0.0, 1.0), vfov=0.9):
    b = trimesh_poses()[n, 0, 0:3].astype(np.float64)
    return dict(env=n, follow=False, eye=tuple(np.float32(b + eye_off).tolist()),
                target=tuple(np.float32(b + tgt_off).tolist()), up=up, vfov=vfov)


def trimesh_cameras():
    """B: three fixed cameras on envs 0, 1 and 4 (the last env), one call at 48 x 32."""
    return [_look(0, (1.5, 0.7, 2.2), (0.0, 0.0, 0.3), vfov=0.5), _look(1, (-1.4, 1.1, 2.0), (0.1, 0.0, 0.2), vfov=0.5),
            _look(4, (0.8, -1.7, 2.1), (0.0, 0.1, 0.4), vfov=0.5)]


def down_camera():
    """B, second call (33 x 33): straight down with up = (1, 0, 0); the centre ray has zero x and y components."""
    return _look(3, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), up=(1.0, 0.0, 0.0), vfov=0.5)


def edge_camera():
    """C (40 x 24): from inside the field near its -x edge (x = -5), looking outward and slightly down: the lower rays
    reach the terrain before the edge, the others leave the footprint and show the sky."""
    return _look(2, (1.2, 0.3, 0.6), (-2.0, -0.2, -1.0), vfov=0.5)


# D: (width, height, vfov): camera 0 of B with the field of view that keeps a pixel's angle
SIZES_D = ((1, 1, 0.016), (16, 16, 0.25), (17, 1, 0.016))


def trimesh_cases():
    """(name, scene, cameras, width, height) of every trimesh comparison the GPU test makes."""
    T, rs = trimesh_terrain(), trimesh_poses()

    def scene(n):
        return dict(rigid=rs[n], terrain=T)
    cases = [("B%d" % k, scene(c["env"]), c, 48, 32) for k, c in enumerate(trimesh_cameras())]
    cases.append(("Bdown", scene(3), down_camera(), 33, 33))
    cases.append(("C", scene(2), edge_camera(), 40, 24))
    cases += [("D%dx%d" % s[:2], scene(0), dict(trimesh_cameras()[0], vfov=s[2]), s[0], s[1]) for s in SIZES_D]
    return cases


PLANE_CAMERA = dict(env=1, follow=True, eye=(3.0, 0.0, 1.0), target=(0.0, 0.0, 0.6), up=(0.0, 0.0, 1.0), vfov=0.9)
PLANE_SIZE = (50, 37)   # A: no multiple of the tile in either axis


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """render_ref.reference of a trimesh case with the product's primitives and style; computed once, shared."""
    import render_ref
    from ti5_isaacgym_amd.utils import render as R
    _, scene, cam, w, h = next(c for c in trimesh_cases() if c[0] == name)
    return render_ref.reference(scene, cam, w, h, R.robot_primitives(), R.STYLE)
