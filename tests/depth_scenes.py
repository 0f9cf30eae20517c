"""The depth sensor tests' scenes as pure data: the 6 x 4 trimesh field of tests/render_scenes.py (trimesh_terrain,
terrain_hook, BASES) with five envs of their own -- the base yawed anywhere, rolled and pitched within 0.5 rad and 0.6 to
1.2 m above the local ground, the other twelve bodies scattered around it as in render_scenes.trimesh_poses so that some
lie in view -- and one sensor: mounted forward of the base's origin, pitched down, 21 x 13 pixels (no multiple of any
tile), far = 3 m.  Env 2 stands near the field's -x edge and looks out over it, so its rays leave the footprint; env 4
stands on the stairs.  tests/test_depth_sensor_host.py examines the scenes without a device (the ambiguity cap, the
pixel counts), tests/test_gpu_depth_sensor.py writes the poses into an env built with the same configuration and
compares the kernel's images to tests/depth_ref.py."""
import functools

import numpy as np

from render_scenes import BASES, NUM_ENVS, SEED, _ground, terrain_hook, trimesh_terrain  # noqa: F401

WIDTH, HEIGHT = 21, 13
# roll, pitch, yaw of the mount: 0.7 rad down.  The mount lies inside the base's box, which the entry-only rule hides.
MOUNT_RPY = (0.0, 0.7, 0.0)
SENSOR = dict(body=0, pos=(0.12, 0.0, 0.05), vfov=0.9, near=0.1, far=3.0)
# base yaw per env: env 2 looks towards -x, over the field's edge at x = -5
YAW = (0.4, 2.1, 3.0, -1.3, -2.6)
# image sizes of the size test: (width, height, vfov)
SIZES = ((1, 1, 0.05), (17, 1, 0.08), (16, 16, 0.9))
# the launches of the count test: (which of the five poses each env of the launch has, (width, height, vfov)).  A wave
# draws a 16 x 4 pixel block and four waves share a workgroup: at 16 x 4 and 5 x 3 a workgroup holds four envs (7 is no
# multiple of that, 1 leaves three waves idle), at 16 x 12 an env's three blocks straddle the workgroups.
COUNTS = (((3,), (21, 13, 0.9)), ((3,), (16, 4, 0.3)), ((0, 1, 2, 3, 4, 0, 1), (16, 4, 0.3)), ((1, 2, 4), (16, 12, 0.9)),
          ((3, 0, 1, 2, 3, 0, 1), (5, 3, 0.6)))


def rpy_quat(roll, pitch, yaw):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = (f(0.5 * a) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


def sensor(**kw):
    return dict(SENSOR, quat=tuple(rpy_quat(*MOUNT_RPY)), **kw)


@functools.lru_cache(maxsize=None)
def trimesh_poses():
    """(NUM_ENVS, 13, 13) float32 rigid_state rows, zero velocities."""
    T = trimesh_terrain()
    rng = np.random.default_rng(20250318)
    rs = np.zeros((NUM_ENVS, 13, 13), dtype=np.float32)
    for n in range(NUM_ENVS):
        x, y = BASES[n]
        rs[n, 0, 0:3] = (x, y, _ground(T, x, y) + rng.uniform(0.6, 1.2))
        rs[n, 0, 3:7] = rpy_quat(rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), YAW[n])
        for b in range(1, 13):
            x, y = BASES[n] + rng.uniform(-0.5, 0.5, 2)
            q = rng.standard_normal(4)
            rs[n, b, 0:3] = (x, y, _ground(T, x, y) + rng.uniform(0.0, 1.2))
            rs[n, b, 3:7] = q / np.linalg.norm(q)
    rs.setflags(write=False)
    return rs


def scene(n):
    return dict(rigid=trimesh_poses()[n], terrain=trimesh_terrain())


@functools.lru_cache(maxsize=None)
def reference_of(n, size=None):
    """depth_ref.reference of env n with the product's primitives; size: None (the 21 x 13 sensor) or an entry of
    SIZES.  Computed once, shared."""
    import depth_ref
    from ti5_isaacgym_amd.utils import render as R
    w, h, s = (WIDTH, HEIGHT, sensor()) if size is None else (size[0], size[1], sensor(vfov=size[2]))
    return depth_ref.reference(scene(n), s, w, h, R.robot_primitives())


# the mount that replaces env 3's in the mounts test: further forward, higher, looking less far down and to the left
OTHER_MOUNT = np.concatenate([[0.2, -0.05, 0.15], rpy_quat(0.1, 0.45, 0.5)]).astype(np.float32)

# the plane tests' sensor: steeper and wider, so that the lowest rays look back under the base and the robot's own legs
# are in the picture
PLANE_RPY = (0.0, 1.2, 0.0)
PLANE_SENSOR = dict(body=0, pos=(0.1, 0.0, 0.0), vfov=1.2, near=0.1, far=3.0)


def plane_sensor(**kw):
    return dict(PLANE_SENSOR, quat=tuple(rpy_quat(*PLANE_RPY)), **kw)
