"""Headless camera over the HIP env (include/t1render.h, csrc/t1render.hip): the robot as its collision-level
geometry, the terrain the physics stands on, one light with the robot's shadow.

    from ti5_isaacgym_amd.utils.render import Camera, Renderer, write_png
    r = Renderer(env, 640, 360, [Camera.follow(0)])
    frame = r.render()              # (1, 360, 640, 4) uint8 on the device, one launch on the current stream
    write_png("frame.png", frame[0].cpu().numpy())

By default a camera sees its own env's robot and the terrain.  ``Renderer(..., others=True)`` puts every env's robot
into the scene (t1render_scene: culled on the device, so a frame does not cost num_envs per pixel; ``self.envs`` then
tells whose robot a pixel shows), ``terrain_shadow=True`` lets the height field cast shadows as well.
``Renderer(..., mesh=RobotMesh.from_urdf(path))`` draws the robot as the URDF's visual meshes instead of the
primitives (t1render_mesh_scene: a bounding volume hierarchy per body, walked on the device; ``self.tris`` tells which
triangle a pixel shows); smooth shading, textures and materials are not drawn.  After a
real-dynamics step ``rigid_state`` holds the post-physics, pre-reset pose, so an env reset in that step is drawn where
it fell.

The camera as a sensor is ``DepthSensor``: one launch (t1render_depth, csrc/t1render_depth.hip) writes a small depth
image for every env, from a camera mounted on a body of the env's own robot.

    s = DepthSensor(env, 64, 48, pos=(0.1, 0.0, 0.1), rpy=(0.0, 0.6, 0.0))
    depth = s.render()              # (num_envs, 48, 64) float32 on the device, planar depth in [near, far]

That image is a perfect sensor's, of this instant.  ``DepthSensor(..., noise=DepthNoise(sigma2=0.005, p_drop=0.01,
p_edge=0.5), latency=(1, 3))`` puts a real one's faults behind it in one more launch (t1render_depth_model,
csrc/t1render_depth_model.hip): noise that grows with the square of the depth, pixels without a measurement, and a
per-env delay of whole frames; render() then returns ``self.measured`` and ``self.depth`` stays the clean image.
"""
import struct
import zlib

import numpy as np

from .. import _lib
from .urdf import SELF_BODIES, load_model

BOX, CAPSULE = 0, 1
LIMB_RADIUS = 0.04            # drawing radius of the limb capsules [m] (the links' collision shapes are the boxes)
# colours per body group, 0xBBGGRR
COLOR_BASE, COLOR_LEFT, COLOR_RIGHT, COLOR_FEET = 0x3C3CDC, 0xD28C32, 0x50B43C, 0x32C8E6
FEET = (6, 12)
# light: unit direction towards the light; sky_rgb[0] at d.z = -1, [1] at d.z = +1
STYLE = dict(light=(0.3, 0.2, 0.87 ** 0.5), ambient=0.35,
             terrain_rgb=((0.62, 0.60, 0.55), (0.42, 0.44, 0.42)),
             sky_rgb=((0.85, 0.90, 0.95), (0.35, 0.55, 0.90)))
DEFAULT_VFOV = 0.9            # [rad]


def _body_color(b):
    return COLOR_BASE if b == 0 else COLOR_FEET if b in FEET else COLOR_LEFT if b < 7 else COLOR_RIGHT


def robot_primitives(tab=None):
    """The drawing table of the compiled model (utils/urdf.load_model()): a list of dicts body, kind, a, b, r, rgb.
    The base as the bounding box of its contact points, the four self-collision boxes (shanks and feet), and for every
    body b >= 1 with a child c a capsule from b's origin to joint_offset[c]."""
    tab = tab or load_model()
    prims = []
    pts = np.array([p for p, b in zip(tab["contact_point"], tab["contact_body"]) if b == 0], dtype=np.float64)
    lo, hi = pts.min(0), pts.max(0)
    prims.append(dict(body=0, kind=BOX, a=tuple((lo + hi) / 2), b=tuple((hi - lo) / 2), r=0.0, rgb=COLOR_BASE))
    for body, box in zip(SELF_BODIES, tab["self_box"]):
        prims.append(dict(body=body, kind=BOX, a=tuple(box[:3]), b=tuple(box[3:]), r=0.0, rgb=_body_color(body)))
    for c, b in enumerate(tab["parent"]):
        if b >= 1:
            prims.append(dict(body=b, kind=CAPSULE, a=(0.0, 0.0, 0.0), b=tuple(tab["joint_offset"][c]), r=LIMB_RADIUS,
                              rgb=_body_color(b)))
    return prims


class Camera:
    """A pinhole camera of env ``env``.  follow: eye and target are offsets from the env's base position, added on the
    device (the base's yaw is not followed)."""

    def __init__(self, env, eye, target, up=(0.0, 0.0, 1.0), vfov=DEFAULT_VFOV, follow=False):
        self.env, self.follow, self.vfov = int(env), bool(follow), float(vfov)
        self.eye, self.target, self.up = tuple(map(float, eye)), tuple(map(float, target)), tuple(map(float, up))

    @classmethod
    def fixed(cls, env, eye, target, up=(0.0, 0.0, 1.0), vfov=DEFAULT_VFOV):
        return cls(env, eye, target, up, vfov, follow=False)

    @classmethod
    def follow(cls, env, offset=(3.0, 0.0, 1.0), look=(0.0, 0.0, -0.1), up=(0.0, 0.0, 1.0), vfov=DEFAULT_VFOV):
        """offset and look are relative to the base link's origin, about 1 m above the soles when the robot stands: the
        default looks slightly below it, so that the feet, their shadow and a strip of sky are in the picture."""
        return cls(env, offset, look, up, vfov, follow=True)

    def pack(self):
        return _lib.RenderCamera(self.env, int(self.follow), (_lib.f32 * 3)(*self.eye), (_lib.f32 * 3)(*self.target),
                                 (_lib.f32 * 3)(*self.up), self.vfov)


def pack_prims(prims):
    arr = (_lib.RenderPrim * max(len(prims), 1))()
    for d, p in zip(arr, prims):
        d.body, d.kind, d.r, d.rgb = int(p["body"]), int(p["kind"]), float(p["r"]), int(p["rgb"])
        d.a[:], d.b[:] = [float(x) for x in p["a"]], [float(x) for x in p["b"]]
    return arr


def pack_style(style):
    s = _lib.RenderStyle()
    s.light[:] = [float(x) for x in style["light"]]
    s.ambient = float(style["ambient"])
    for k in range(2):
        s.terrain_rgb[k][:] = [float(x) for x in style["terrain_rgb"][k]]
        s.sky_rgb[k][:] = [float(x) for x in style["sky_rgb"][k]]
    return s


class RobotMesh:
    """The robot as triangle meshes on the device (t1render_mesh_create: one bounding volume hierarchy per body, built
    on the host and uploaded once).  tri (T, 3, 3) float32 vertices in the frame of their body, body (T,) in [0, 13),
    rgb (T,) 0xBBGGRR.  Owns the handle: close() (or the garbage collector) destroys it."""

    def __init__(self, tri, body, rgb):
        tri = np.ascontiguousarray(tri, dtype=np.float32)
        body = np.ascontiguousarray(body, dtype=np.int32)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint32)
        if tri.ndim != 3 or tri.shape[1:] != (3, 3) or body.shape != (len(tri),) or rgb.shape != (len(tri),):
            raise ValueError("RobotMesh takes tri (T, 3, 3), body (T,) and rgb (T,)")
        self._lib = _lib.load()
        self._handle = _lib.C.c_void_p()
        self.ntri = len(tri)
        _lib.check(self._lib.t1render_mesh_create(tri.ctypes.data_as(_lib.C.POINTER(_lib.f32)),
                                                  body.ctypes.data_as(_lib.C.POINTER(_lib.i32)),
                                                  rgb.ctypes.data_as(_lib.C.POINTER(_lib.u32)), self.ntri,
                                                  _lib.C.byref(self._handle)), "t1render_mesh_create")

    @classmethod
    def from_urdf(cls, path, missing_ok=False):
        """The URDF's visual meshes (utils/urdf.visual_meshes), coloured by source link: the feet COLOR_FEET, the
        left and right legs and arm links COLOR_LEFT and COLOR_RIGHT, the rest of the base group COLOR_BASE."""
        from .urdf import visual_meshes
        m = visual_meshes(path, missing_ok=missing_ok)
        per_link = np.array([COLOR_LEFT if n.startswith(("L_", "leg_l")) else
                             COLOR_RIGHT if n.startswith(("R_", "leg_r")) else COLOR_BASE for n in m["links"]] + [0],
                            dtype=np.uint32)
        rgb = per_link[m["link"]]
        rgb[np.isin(m["body"], FEET)] = COLOR_FEET
        return cls(m["tri"], m["body"], rgb)

    def info(self):
        """dict(ntri, nnodes, max_depth, radius (13,)): t1render_mesh_info."""
        n, k, d = _lib.i32(), _lib.i32(), _lib.i32()
        r = (_lib.f32 * 13)()
        _lib.check(self._lib.t1render_mesh_info(self._handle, _lib.C.byref(n), _lib.C.byref(k), _lib.C.byref(d), r),
                   "t1render_mesh_info")
        return dict(ntri=n.value, nnodes=k.value, max_depth=d.value, radius=np.array(r[:], dtype=np.float32))

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.t1render_mesh_destroy(self._handle)
            self._handle = None

    def __del__(self):
        self.close()


class Renderer:
    """Preallocated device outputs for ``cameras`` at width x height over ``env`` (a T1DHStandEnv).  others: every
    env's robot is drawn and casts shadows, not only the camera's own; terrain_shadow: the height field casts shadows.
    With both off render() is t1render_frame; else t1render_scene, with the workspace allocated here, once.  mesh (a
    RobotMesh): render() is t1render_mesh_scene instead -- the robot is drawn as the mesh's triangles, prims is ignored,
    and self.tris tells which triangle a pixel shows."""

    def __init__(self, env, width, height, cameras, prims=None, style=None, others=False, terrain_shadow=False,
                 mesh=None):
        import torch
        self.env, self.width, self.height = env, int(width), int(height)
        self.cameras = list(cameras)
        n = len(self.cameras)
        if not 1 <= n <= _lib.RENDER_MAXCAM:
            raise ValueError(f"1 to {_lib.RENDER_MAXCAM} cameras per renderer, got {n}")
        self.prims = list(robot_primitives() if prims is None else prims)
        if len(self.prims) > _lib.RENDER_MAXPRIM:
            raise ValueError(f"at most {_lib.RENDER_MAXPRIM} primitives, got {len(self.prims)}")
        self.style = dict(STYLE if style is None else style)
        self._cams = (_lib.RenderCamera * n)(*[c.pack() for c in self.cameras])
        self._prims, self._style = pack_prims(self.prims), pack_style(self.style)
        d = env.device
        self.rgba = torch.zeros(n, self.height, self.width, 4, dtype=torch.uint8, device=d)
        self.depth = torch.zeros(n, self.height, self.width, dtype=torch.float32, device=d)
        self.ids = torch.zeros(n, self.height, self.width, dtype=torch.int32, device=d)
        self.others, self.terrain_shadow = bool(others), bool(terrain_shadow)
        self.flags = (_lib.RENDER_SCENE_OTHERS if self.others else 0) | \
            (_lib.RENDER_SCENE_TERRAIN_SHADOW if self.terrain_shadow else 0)
        # whose robot a pixel shows (-1: terrain, sky); stays -1 while both switches are off (t1render_frame has no such plane)
        self.envs = torch.full((n, self.height, self.width), -1, dtype=torch.int32, device=d)
        self.mesh = mesh
        # the caller's index of the triangle a pixel shows (-1: terrain, sky); written with a mesh only
        self.tris = torch.full((n, self.height, self.width), -1, dtype=torch.int32, device=d) if mesh is not None else None
        self.workspace = None
        if self.others:
            size = env._lib.t1render_scene_workspace_bytes(int(env.num_envs), n)
            if size < 0:
                raise ValueError(f"t1render_scene_workspace_bytes({env.num_envs}, {n}) refused")
            self.workspace = torch.zeros(size, dtype=torch.uint8, device=d)   # torch allocates on 256-byte boundaries

    def render(self, rgba_out=None):
        """On the current stream (one launch; with others a memset and three).  Returns the (ncams, H, W, 4) uint8
        device buffer it wrote: rgba_out when given (same shape, contiguous), else self.rgba; self.depth and self.ids
        are written too, and self.envs whenever others or terrain_shadow is on (with a mesh: always, and self.tris)."""
        import torch
        out = self.rgba if rgba_out is None else rgba_out
        if rgba_out is not None and (out.shape != self.rgba.shape or out.dtype != torch.uint8 or
                                     not out.is_contiguous() or out.device != self.rgba.device):
            raise ValueError(f"rgba_out must be a contiguous uint8 {tuple(self.rgba.shape)} tensor on {self.rgba.device}")
        env = self.env
        stream = torch.cuda.current_stream(env.device).cuda_stream
        if self.mesh is not None:
            ws = self.workspace
            _lib.check(env._lib.t1render_mesh_scene(env._handle, self._cams, len(self.cameras), self.mesh._handle,
                                                    _lib.C.byref(self._style), self.flags, self.width, self.height,
                                                    out.data_ptr(), self.depth.data_ptr(), self.ids.data_ptr(),
                                                    self.envs.data_ptr(), self.tris.data_ptr(),
                                                    ws.data_ptr() if ws is not None else None,
                                                    ws.numel() if ws is not None else 0, stream), "t1render_mesh_scene")
            return out
        if self.flags:
            ws = self.workspace
            _lib.check(env._lib.t1render_scene(env._handle, self._cams, len(self.cameras), self._prims, len(self.prims),
                                               _lib.C.byref(self._style), self.flags, self.width, self.height,
                                               out.data_ptr(), self.depth.data_ptr(), self.ids.data_ptr(),
                                               self.envs.data_ptr(), ws.data_ptr() if ws is not None else None,
                                               ws.numel() if ws is not None else 0, stream), "t1render_scene")
            return out
        _lib.check(env._lib.t1render_frame(env._handle, self._cams, len(self.cameras), self._prims, len(self.prims),
                                           _lib.C.byref(self._style), self.width, self.height, out.data_ptr(),
                                           self.depth.data_ptr(), self.ids.data_ptr(), stream), "t1render_frame")
        return out


def rpy_quat(roll, pitch, yaw):
    """The quaternion (x, y, z, w) of the rotation Rz(yaw) Ry(pitch) Rx(roll) (a URDF's rpy): a positive pitch turns the
    camera's +x towards -z, i.e. looks down."""
    cr, sr, cp, sp, cy, sy = (f(0.5 * a) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return (float(sr * cp * cy - cr * sp * sy), float(cr * sp * cy + sr * cp * sy),
            float(cr * cp * sy - sr * sp * cy), float(cr * cp * cy + sr * sp * sy))


SEED_SALT = 0x5EED0DE7   # the model's seed is seed ^ SEED_SALT: its draws never coincide with the env step's


class DepthNoise:
    """The measurement model of t1render_depth_model (include/t1render.h states it to the bit).  sigma0, sigma2: the
    noise's standard deviation [m] is sigma0 + sigma2 z^2 at depth z, as a stereo pair's; p_drop: the probability that a
    pixel has no measurement; p_edge: the same for a pixel on the far side of an occlusion edge, where its depth exceeds
    its nearest 4-neighbour's mn by more than edge_abs + edge_rel mn; fill: the value of a pixel without a measurement
    (None: the sensor's far, what a pixel with nothing in range holds).  The defaults change nothing."""

    def __init__(self, sigma0=0.0, sigma2=0.0, p_drop=0.0, p_edge=0.0, edge_abs=0.05, edge_rel=0.05, fill=None):
        self.sigma0, self.sigma2, self.p_drop, self.p_edge = float(sigma0), float(sigma2), float(p_drop), float(p_edge)
        self.edge_abs, self.edge_rel = float(edge_abs), float(edge_rel)
        self.fill = None if fill is None else float(fill)

    def pack(self, seed, env_base, near, far):
        return _lib.RenderDepthNoise((int(seed) ^ SEED_SALT) & 0xFFFFFFFF, int(env_base), float(near), float(far),
                                     self.sigma0, self.sigma2, self.p_drop, self.p_edge, self.edge_abs, self.edge_rel,
                                     float(far) if self.fill is None else self.fill)


class DepthSensor:
    """A depth camera bolted to body ``body`` of every env's robot (t1render_depth): one launch writes
    ``self.depth`` (num_envs, height, width), the planar depth [m] of the nearest surface in [near, far] and exactly
    ``far`` where there is none, for all envs of ``env`` (a T1DHStandEnv) at once.

    pos, and quat (x, y, z, w) or rpy (roll, pitch, yaw; at most one of the two, default: none, the body's own axes):
    the camera's frame in the body's frame; it looks along its +x, +y is to its left, +z is up.  pos has no default:
    the repository knows no camera of the real robot, so the mount is the caller's to state.  The scene of an env is
    the terrain and its own robot as ``prims`` (None: robot_primitives()); a primitive that contains the camera is not
    seen, so the mount may lie inside the base's box.  dtype: torch.float32 (also what None means: this module imports
    torch only where it needs it), or torch.float16 (the fp32 value rounded once).  ids=True also allocates ``self.ids`` (int8: -1 nothing in range, 0 terrain, 1 + body).  mounts: None, or a
    (num_envs, 7) float32 device tensor of pos and unit quat per env that replaces the mount env by env (kept by
    reference: write into it to re-randomise).  After a real-dynamics step an env that was reset is seen from where it
    fell (rigid_state holds the pre-reset pose).

    noise (a DepthNoise) and latency (lo, hi), in frames: with noise None and latency (0, 0) -- the default -- the sensor
    is the perfect one above and has none of the following.  Otherwise render() makes a second launch
    (t1render_depth_model) and returns ``self.measured`` (the shape and dtype of ``self.depth``, which stays the clean
    image): the measurement of env n as it was ``self.lag[n]`` render() calls ago.  ``self.lag`` (num_envs,) int32 is
    drawn once, uniformly in [lo, hi], from a torch.Generator seeded with ``seed``, and read by reference at every
    render: write into it to re-randomise (values are clamped to [0, hi]).  With hi > 0 the sensor owns a ring of hi + 1
    frames.  seed and env_base (a rank's first global env) key the model's draws together with the frame counter
    ``self.frame``, which render() advances."""

    def __init__(self, env, width, height, pos, quat=None, rpy=None, body=0, vfov=DEFAULT_VFOV, near=0.1, far=3.0,
                 dtype=None, prims=None, ids=False, mounts=None, noise=None, latency=(0, 0), seed=0, env_base=0):
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"DepthSensor writes torch.float32 or torch.float16, got {dtype}")
        if quat is not None and rpy is not None:
            raise ValueError("DepthSensor takes quat or rpy, not both")
        quat = rpy_quat(*rpy) if rpy is not None else (0.0, 0.0, 0.0, 1.0) if quat is None else quat
        self.env, self.width, self.height = env, int(width), int(height)
        self.prims = list(robot_primitives() if prims is None else prims)
        if len(self.prims) > _lib.RENDER_MAXPRIM:
            raise ValueError(f"at most {_lib.RENDER_MAXPRIM} primitives, got {len(self.prims)}")
        self.near, self.far = float(near), float(far)
        self._sensor = _lib.RenderSensor(int(body), (_lib.f32 * 3)(*[float(x) for x in pos]),
                                         (_lib.f32 * 4)(*[float(x) for x in quat]), float(vfov), self.near, self.far)
        self._prims = pack_prims(self.prims)
        self.flags = _lib.RENDER_DEPTH_F16 if dtype == torch.float16 else 0
        n, d = int(env.num_envs), env.device
        if mounts is not None and (tuple(mounts.shape) != (n, 7) or mounts.dtype != torch.float32 or
                                   not mounts.is_contiguous() or mounts.device != d):
            raise ValueError(f"mounts must be a contiguous float32 ({n}, 7) tensor on {d}")
        self.mounts = mounts
        self.depth = torch.zeros(n, self.height, self.width, dtype=dtype, device=d)
        self.ids = torch.zeros(n, self.height, self.width, dtype=torch.int8, device=d) if ids else None
        lo, hi = (int(x) for x in latency)
        if not 0 <= lo <= hi < _lib.RENDER_DEPTH_MAXRING:
            raise ValueError(f"latency must be 0 <= lo <= hi <= {_lib.RENDER_DEPTH_MAXRING - 1} frames, got {latency}")
        self._model = None
        if noise is None and hi == 0:
            return
        self.noise = DepthNoise() if noise is None else noise
        self._model = self.noise.pack(seed, env_base, self.near, self.far)
        self.measured = torch.zeros_like(self.depth)
        g = torch.Generator().manual_seed(int(seed))
        self.lag = torch.randint(lo, hi + 1, (n,), generator=g, dtype=torch.int32).to(d)
        self._ring = torch.zeros(hi + 1, n, self.height, self.width, dtype=dtype, device=d) if hi > 0 else None
        self._all_fresh = torch.ones(n, dtype=torch.uint8, device=d)
        self.frame = 0

    def render(self, stream=None, fresh=None):
        """On ``stream`` (a raw stream handle; None: torch's current stream of the env's device), no allocation.  The
        perfect sensor: one launch; returns self.depth (self.ids is written too when it exists), fresh is ignored.  With a
        model: a second launch behind it; returns self.measured.  fresh: None, or a bool / uint8 (num_envs,) device tensor
        of the envs whose history ends here (reset since the last render): they are served this frame now and nothing
        older later.  The first call makes every env fresh."""
        env = self.env
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(env.device).cuda_stream
        if self._model is not None and fresh is not None and self.frame > 0:
            import torch
            if tuple(fresh.shape) != (self.depth.shape[0],) or fresh.dtype not in (torch.bool, torch.uint8) or \
                    not fresh.is_contiguous() or fresh.device != self.depth.device:
                raise ValueError(f"fresh must be a contiguous bool or uint8 ({self.depth.shape[0]},) tensor on "
                                 f"{self.depth.device}")
        _lib.check(env._lib.t1render_depth(env._handle, _lib.C.byref(self._sensor),
                                           self.mounts.data_ptr() if self.mounts is not None else None, self._prims,
                                           len(self.prims), self.width, self.height, self.flags, self.depth.data_ptr(),
                                           self.ids.data_ptr() if self.ids is not None else None, stream),
                   "t1render_depth")
        if self._model is None:
            return self.depth
        fresh = self._all_fresh if self.frame == 0 else fresh
        ring = self._ring
        _lib.check(env._lib.t1render_depth_model(_lib.C.byref(self._model), self.depth.data_ptr(), self.depth.shape[0],
                                                 self.width, self.height, self.flags, self.frame & 0xFFFFFFFF,
                                                 ring.data_ptr() if ring is not None else None,
                                                 ring.shape[0] if ring is not None else 1, self.lag.data_ptr(),
                                                 fresh.data_ptr() if fresh is not None else None,
                                                 self.measured.data_ptr(), stream), "t1render_depth_model")
        self.frame += 1
        return self.measured


def write_png(path, hwc_uint8):
    """An (H, W, 3) or (H, W, 4) uint8 array as an 8-bit RGB / RGBA PNG (zlib and struct only)."""
    a = np.ascontiguousarray(hwc_uint8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png takes an (H, W, 3) or (H, W, 4) uint8 array")
    h, w, c = a.shape

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    rows = np.zeros((h, 1 + w * c), np.uint8)   # filter type 0 in front of every row
    rows[:, 1:] = a.reshape(h, w * c)
    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 6, 0, 0, 0)) +
           chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
