/* t1render.h -- headless camera over a t1env handle: one launch ray-casts up to T1RENDER_MAXCAM pinhole cameras.
 *
 * Scene of a camera: its own env's robot (the primitives below, posed by rigid_state[env]) and the terrain the env
 * handle holds (t1env_set_terrain; the plane z = 0 without one).  t1render_frame draws no other env's robot;
 * t1render_scene (below) draws every env's and lets the height field cast shadows.  The height field is
 * the surface the physics stands on (two triangles per cell, split along (i,j)-(i+1,j+1)), restricted to the field's
 * footprint: outside it there is no terrain and a ray shows the sky.
 *
 * Which pose: rigid_state after a real-dynamics step holds the post-physics, PRE-reset pose.  An env that was reset in
 * that step is therefore drawn where it fell, and stands up one frame late.
 *
 * Ray of pixel (row i from the top, column j): x = (2(j+0.5)/W - 1) tan(vfov/2) W/H, y = (1 - 2(i+0.5)/H) tan(vfov/2),
 * direction normalize(f + x r + y u) with f = normalize(target - eye), r = normalize(f x up), u = r x f.  A primitive is
 * hit where the ray ENTERS the solid (a ray that starts inside one does not see it); the terrain is hit from either
 * side.  Hits count for t in (0.05, 200] along the unit direction, the nearest wins.  Shading: intensity = ambient +
 * (1 - ambient) max(n.L, 0) lit, with lit = 0 when a ray from hit + 1e-3 n towards the light enters a primitive of the
 * robot at 0 < t <= 200 (the terrain casts no shadow).  Terrain colour: terrain_rgb[(floor(x) + floor(y)) & 1] at the
 * hit; sky: sky_rgb[0] + (sky_rgb[1] - sky_rgb[0]) (d.z + 1) / 2.  Channels: floor(clamp(v, 0, 1) 255 + 0.5).
 */
#ifndef T1RENDER_H
#define T1RENDER_H

#include <stdint.h>

#include "t1env.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T1RENDER_MAXCAM 16
#define T1RENDER_MAXPRIM 32

/* follow = 1: eye and target are offsets added on the device to the env's base position (rigid_state body 0); the
 * base's yaw is not followed.  vfov: vertical field of view [rad]. */
typedef struct t1render_camera { int32_t env, follow; float eye[3], target[3], up[3], vfov; } t1render_camera;
/* in the frame of body `body`.  kind 0: box (a centre, b half extents); kind 1: capsule (a, b the segment's ends, r the
 * radius; a == b is a sphere).  rgb: 0x00BBGGRR. */
typedef struct t1render_prim   { int32_t body, kind; float a[3], b[3], r; uint32_t rgb; } t1render_prim;
/* light: the direction TOWARDS the light (normalised by the call).  sky_rgb[0] straight down, [1] straight up. */
typedef struct t1render_style  { float light[3], ambient, terrain_rgb[2][3], sky_rgb[2][3]; } t1render_style;

/* cams, prims and style: host memory, read during the call.  rgba (ncams, height, width) uint32 R | G<<8 | B<<16 |
 * 255<<24, depth (same shape, fp32: the hit's t, +inf for sky) and ids (int32: -1 sky, 0 terrain, 1 + body): device
 * memory; depth and ids may be NULL.  One launch on `stream`; no allocation, no synchronisation and no write to any env
 * buffer.
 * T1ENV_E_ARG: a null env, cams, prims, style or rgba; ncams outside [1, T1RENDER_MAXCAM]; nprims outside
 * [0, T1RENDER_MAXPRIM]; width or height < 1; a camera's env outside [0, num_envs); a primitive's body outside
 * [0, 13) or kind outside {0, 1}; a degenerate up (zero, or parallel to target - eye; in follow mode of the offsets);
 * a vfov outside (0, pi); a zero light.  T1ENV_E_STATE: a height-field env without terrain samples. */
int t1render_frame(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_prim* prims, int32_t nprims,
                   const t1render_style* style, int32_t width, int32_t height,
                   uint32_t* rgba, float* depth, int32_t* ids, void* stream);

/* t1render_scene: the same camera over a larger scene, chosen by flags. */
#define T1RENDER_SCENE_OTHERS          1  /* every env's robot is in the scene, not only the camera's */
#define T1RENDER_SCENE_TERRAIN_SHADOW  2  /* the height field casts shadows (no effect on the plane) */
#define T1RENDER_SCENE_BRUTE           4  /* test hook: no culling, every env's primitives for every ray */

/* With OTHERS the primitive set is prims posed by rigid_state[n] for every n in [0, num_envs); ray, hit range, the
 * entry-only rule, shading and colour are those above.  The nearest entry wins; at exactly equal t the lower env, then
 * the lower primitive index; the terrain still wins a tie against a primitive.  The shadow ray tests the same primitive
 * set as the camera ray, so a neighbour shadows the camera's robot and the ground under it.  With TERRAIN_SHADOW the
 * shadow ray (origin hit + 1e-3 n, direction L) is also cast against the height field by the camera ray's rule: a hit
 * at t in (0.05, 200] darkens the pixel; the plane casts nothing.  envs (int32, the shape of ids, may be NULL): the env
 * whose robot the pixel shows, -1 for terrain and sky.  With flags == 0 rgba, depth and ids are bit for bit what
 * t1render_frame writes, and envs is the camera's env where ids > 0.
 *
 * Culling: with OTHERS a pre-pass over the envs writes a padded bounding sphere of each posed robot (from rigid_state,
 * whatever the poses are; quaternions are taken to be unit ones) and one bit per env and camera into the workspace, and
 * the render kernel tests only the robots that can touch a tile's rays or cast a shadow into it.  Culling is invisible:
 * with and without BRUTE the four planes are equal to the bit.  BRUTE needs no workspace and costs num_envs per pixel.
 *
 * workspace: device memory of at least t1render_scene_workspace_bytes(num_envs, ncams) bytes on a 16-byte boundary,
 * needed with OTHERS and without BRUTE (else it may be NULL); its content before the call does not matter and the call
 * writes nowhere else but the outputs.  A memset and up to three launches in stream order on `stream`; no allocation,
 * no synchronisation, no host read.  t1render_scene_workspace_bytes returns -1 for num_envs < 0 or ncams outside
 * [1, T1RENDER_MAXCAM] and never shrinks as either grows.
 * Errors, all before any device work: everything t1render_frame refuses; T1ENV_E_ARG also for an unknown flag bit,
 * OTHERS without BRUTE and with a NULL workspace, and a non-NULL workspace that is smaller than the query's size or
 * off a 16-byte boundary. */
long long t1render_scene_workspace_bytes(int32_t num_envs, int32_t ncams);
int t1render_scene(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_prim* prims, int32_t nprims,
                   const t1render_style* style, int32_t flags, int32_t width, int32_t height,
                   uint32_t* rgba, float* depth, int32_t* ids, int32_t* envs,
                   void* workspace, long long workspace_bytes, void* stream);

/* t1render_mesh_*: the same camera with the robot drawn as triangle meshes (its URDF's visual meshes) instead of the
 * primitives.
 *
 * t1render_mesh_create: tri (ntri, 3, 3) float32 vertices in the frame of their body, body (ntri) in [0, 13), rgb
 * (ntri) 0x00BBGGRR: host memory.  It builds one bounding volume hierarchy per body on the host (csrc/t1render_bvh.h)
 * and uploads nodes and triangles once; it is the only call here that allocates or synchronises.  ntri == 0 is legal:
 * a robot that is not drawn.  T1ENV_E_ARG, before any device work: a null pointer, ntri outside [0, 2^20], a body
 * outside [0, 13), a vertex that is not finite.  t1render_mesh_destroy frees the handle (NULL: nothing to do; a handle
 * that is not live: T1ENV_E_ARG).  t1render_mesh_info: the triangle count, the trees' node count, the depth of their
 * deepest leaf and, per body, the padded radius about the body's origin beyond which nothing of it lies (0: no
 * triangle); each output may be NULL.
 *
 * The picture of t1render_mesh_scene.  The robot of env n is the set of world triangles p_b + R_b v, v a vertex of a
 * triangle of body b, p_b = rigid_state[n][b][0:3] and R_b the rotation of the quaternion rigid_state[n][b][3:7] =
 * (x, y, z, w): rows (1 - 2(yy + zz), 2(xy - zw), 2(xz + yw)), (2(xy + zw), 1 - 2(xx + zz), 2(yz - xw)), (2(xz - yw),
 * 2(yz + xw), 1 - 2(xx + yy)).  No primitive is drawn by this call.  A triangle is hit from either side; a triangle of
 * zero area is never hit.  Two rules of the intersection decide hits at a triangle's rim.  The in-triangle test is
 * widened by 1e-5 in the barycentric coordinates (u >= -1e-5, v >= -1e-5, u + v <= 1 + 1e-5), so that a ray along an
 * edge two triangles share cannot slip between them.  And a hit counts only where the hit point, computed in float in
 * the body's frame, lies inside the axis-aligned box of the triangle's three vertices widened by 1e-5 (|o'|_1 + radius),
 * o' being the ray's origin in the body's frame and radius the body's (t1render_mesh_info): this is what lets every
 * bound of the hierarchy err only towards visiting, and it drops a hit whose ray grazes the triangle's plane at less
 * than about 0.3 degrees, where float no longer places the hit point.  Hits count for t in (0.05, 200] along the camera ray, the nearest wins; at exactly equal t
 * the lower env, then the lower triangle index (the caller's); the terrain still wins a tie against the robot.  The
 * normal is the triangle's geometric normal, turned to face the ray's origin (flat shading); the colour is the
 * triangle's rgb.  Ambient, the lit rule, sky, checker and channel rounding are those above.  The shadow ray starts at
 * hit + 1e-3 n and goes towards the light; any triangle at 0 < t <= 200 blocks it, with TERRAIN_SHADOW the height
 * field too (by the rule above), and with OTHERS the triangles of every env.  Without OTHERS the scene holds the
 * camera's env alone.
 *
 * flags: T1RENDER_SCENE_OTHERS, _TERRAIN_SHADOW and _BRUTE (no env culling) as above, and T1RENDER_MESH_BRUTE.  Planes:
 * rgba and depth as above; ids 1 + body, 0 terrain, -1 sky; envs as t1render_scene's; tris (int32) the caller's
 * index of the triangle shown, -1 for terrain and sky.  depth, ids, envs and tris may each be NULL.  All planes are
 * equal to the bit with and without MESH_BRUTE and with and without SCENE_BRUTE.  With an ntri == 0 mesh and
 * flags == 0, rgba, depth and ids are what t1render_frame writes with nprims == 0.
 *
 * Culling and workspace: t1render_scene's, with a robot's sphere taken from the meshes' radii (t1render_mesh_info),
 * not from the primitives.  workspace: at least t1render_mesh_workspace_bytes(num_envs, ncams) bytes of device memory
 * on a 16-byte boundary, needed with OTHERS and without SCENE_BRUTE (else it may be NULL).  A memset and at most three
 * launches in stream order on `stream`; no allocation, no synchronisation, no host read, no write to any env buffer.
 * Errors, all before any device work, outputs and workspace untouched: what t1render_scene refuses of env, cams,
 * style, sizes, flags and workspace, and T1ENV_E_ARG for a mesh that is NULL or not a live handle.
 * Still not drawn: smooth shading, textures and materials; the terrain is the height field, not a mesh. */
typedef struct t1render_mesh t1render_mesh;   /* opaque, device-resident */
int t1render_mesh_create(const float* tri, const int32_t* body, const uint32_t* rgb, int32_t ntri, t1render_mesh** out);
int t1render_mesh_destroy(t1render_mesh* m);
int t1render_mesh_info(const t1render_mesh* m, int32_t* ntri, int32_t* nnodes, int32_t* max_depth, float* radius /*[13]*/);
#define T1RENDER_MESH_BRUTE 8   /* test hook: no BVH, every triangle of a body tested once the body's root box is entered */
long long t1render_mesh_workspace_bytes(int32_t num_envs, int32_t ncams);
int t1render_mesh_scene(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_mesh* mesh,
                        const t1render_style* style, int32_t flags, int32_t width, int32_t height,
                        uint32_t* rgba, float* depth, int32_t* ids, int32_t* envs, int32_t* tris,
                        void* workspace, long long workspace_bytes, void* stream);

/* t1render_depth: the camera as a sensor.  One launch writes a depth image for EVERY env of the handle, each from a
 * pinhole camera fixed to a body of that env's own robot, so the camera turns and pitches with the body.
 *
 * Pose of env n's camera: eye = p_b + R_b pos; forward f = R_b R_m e_x, left l = R_b R_m e_y, up u = R_b R_m e_z, with
 * p_b = rigid_state[n][body][0:3], R_b the rotation of the quaternion rigid_state[n][body][3:7] by the formula above
 * (t1render_mesh_scene), and R_m the rotation of the mount's quat by the same formula; the call normalises the sensor's
 * quat on the host.  It is the pose rule of the top of this file: after a real-dynamics step rigid_state holds the
 * post-physics, PRE-reset pose, and an env that was reset in that step is seen from where it fell.
 * mounts: NULL, or device memory (num_envs, 7) float32, a pos and a UNIT quat (x, y, z, w) per env that replace the
 * sensor's mount for that env (per-env randomisation of the mount); they are used as they are, not normalised.
 *
 * Ray of pixel (row i from the top, column j): x and y by the formula at the top of this file, direction
 * d = normalize(f + x r + y u) with r = -l.  Scene of env n: the terrain by the rule above (the plane z = 0, or the height
 * field restricted to its footprint and hit from either side), and env n's OWN robot, prims posed by rigid_state[n]; no
 * other env's robot.  A primitive is hit where the ray enters it, so a primitive that contains the eye is not seen: the
 * camera may sit inside the base's box.
 *
 * Value: the PLANAR depth z = t (d.f) of the nearest hit, t the distance along the unit direction, among the hits with
 * near <= z <= far.  A primitive entered in front of the near plane is not seen, whatever of it lies behind the plane.
 * Where there is no such hit (sky, beyond far, outside the footprint) the value is exactly far.  Ties: the terrain wins
 * against a primitive, then the lower primitive index.  A hit's value is clamped to [near, far].
 * depth: device memory (num_envs, height, width), fp32, or with T1RENDER_DEPTH_F16 fp16, the fp32 value rounded to
 * nearest even.  ids: NULL, or device memory of the same shape, int8: -1 no hit in range, 0 terrain, 1 + body otherwise.
 * ids == NULL changes no bit of depth.
 *
 * One launch on `stream` for every env of the handle, whatever their number; no allocation, no synchronisation, no host
 * read, no write to any env buffer; sensor and prims are host memory read during the call and travel by value, so the
 * call can be captured in a graph.
 * Errors, all before any device work, outputs untouched.  T1ENV_E_ARG: a null env, sensor or depth; nprims outside
 * [0, T1RENDER_MAXPRIM], or null prims with nprims > 0; the sensor's or a primitive's body outside [0, 13); a kind
 * outside {0, 1}; width or height < 1; width * height * num_envs at or over 2^31; an unknown flag bit; vfov outside
 * (0, pi); anything but 0 < near < far <= 200; a zero or non-finite quat; a non-finite pos.  T1ENV_E_STATE: a
 * height-field env without terrain samples. */
/* A pinhole depth camera fixed to body `body` of every env.  pos, quat (x, y, z, w): the camera's frame in the body's
 * frame.  The camera looks along its own +x, +y is to its left, +z is up.  vfov: vertical field of view [rad]. */
typedef struct t1render_sensor { int32_t body; float pos[3], quat[4], vfov, near, far; } t1render_sensor;
#define T1RENDER_DEPTH_F16 1   /* depth is fp16: the fp32 value rounded to nearest even */
int t1render_depth(t1env* env, const t1render_sensor* sensor, const float* mounts,
                   const t1render_prim* prims, int32_t nprims, int32_t width, int32_t height, int32_t flags,
                   void* depth, int8_t* ids, void* stream);

/* t1render_depth_model: what a real stereo depth camera makes of the clean image -- noise that grows with the square of
 * the depth, pixels without a measurement (random dropouts, and the occlusion shadow on the far side of a depth edge),
 * and a per-env latency served from a ring of the last K measured frames.  A function of device arrays only: no env
 * handle.  One launch on `stream`; no allocation, no synchronisation, no host read; m is host memory read during the
 * call and travels by value, so the call can be captured in a graph (frame is then the captured one).
 *
 * clean: device memory (num_envs, height, width), fp32, or with T1RENDER_DEPTH_F16 fp16 (ring and out then too), as
 * t1render_depth writes it; it is only read.  Measured pixel of env e, row i, column j, from z, the clean value as
 * fp32.  Every operation below is one fp32 operation rounded to nearest, in the order written, none fused.
 *   Draws: h_k = hash4(seed, env_base + e, frame, 4 (i width + j) + k), k = 0..3, the 32-bit counter hash of the env
 *   step (csrc/t1_common.h; all arguments mod 2^32), and u_k = (h_k >> 8) 2^-24 in [0, 1).
 *   1. Nothing in range: z >= far gives fill.
 *   2. Dropout: u_0 < p_drop gives fill.
 *   3. Edge shadow, only with p_edge != 0 (with p_edge == 0 no neighbour is read): mn is the smallest clean value among
 *      the pixels (i-1, j), (i+1, j), (i, j-1), (i, j+1) that lie inside the image (a 1 x 1 image has none: no shadow).
 *      z - mn > edge_abs + edge_rel mn and u_1 < p_edge gives fill: the pixel is on the far side of an occlusion edge.
 *   4. Noise: s = (h_2 & 0xFFFF) + (h_2 >> 16) + (h_3 & 0xFFFF) + (h_3 >> 16) - 131070, an integer in [-131070, 131070];
 *      g = (float)s c with c = sqrt(3) / 65536 rounded to fp32 (an Irwin-Hall sum of four: mean 0, variance 1 to within
 *      3e-10, |g| <= 3.4641).  The value is min(max(z + (sigma0 + (sigma2 z) z) g, near), far).
 *   5. The value, or fill, is stored as fp32, or rounded to nearest even to fp16 (fill too: choose one fp16 can hold).
 *
 * Ring and delay.  ring: device memory (ring_frames, num_envs, height, width) = K frames, owned by the caller and only
 * written by this call.  The measured pixel goes to slot frame mod K, and to all K slots of an env with fresh[e] != 0.
 * out[e] (the shape of clean) is the ring's frame of slot (frame - d) mod K (the true residue, also while frame < d),
 * d = min(max(lag[e], 0), K - 1): what was measured d calls ago, given that the caller counts frame up by one per
 * call.  lag: NULL (no delay), or device int32 (num_envs); fresh: NULL (none), or device uint8 (num_envs).  A fresh env
 * has no history: all its slots hold this call's frame, so for the next K - 1 calls it is served nothing older.  THE
 * CALLER MUST MAKE EVERY ENV FRESH ON THE FIRST CALL (and an env whenever its history ends, e.g. after a reset): the
 * ring's content before that is never looked at, and without it the call serves whatever the memory held.  With K == 1
 * there is no delay, ring may be NULL and the call is the noise pass alone (a non-NULL ring still gets its one slot).
 * frame counts calls and is meant to stay below 2^32; same inputs and same frame give the same bits.
 *
 * Errors, all before any device work, outputs and ring untouched, T1ENV_E_ARG: a null m, clean or out; a null ring with
 * ring_frames > 1; ring_frames outside [1, 16]; num_envs, width or height < 1; width * height * num_envs at or over
 * 2^31; an unknown flag bit; anything but 0 < near < far <= 200; p_drop or p_edge outside [0, 1] (or not a number); a
 * negative or non-finite sigma0, sigma2, edge_abs or edge_rel; a non-finite fill; clean, ring or out off the
 * alignment of its element (4 bytes, 2 with T1RENDER_DEPTH_F16); out or ring overlapping clean, or each other. */
typedef struct t1render_depth_noise {
  uint32_t seed;        /* the sensor's own seed; keep it apart from the env step's, whose draws share the hash */
  int32_t  env_base;    /* added to the env index in every draw (a rank's first global env) */
  float near, far;      /* the clean image's range */
  float sigma0, sigma2; /* noise std [m]: sigma0 + sigma2 * z * z  (stereo: grows with z^2) */
  float p_drop;         /* per-pixel dropout probability */
  float p_edge, edge_abs, edge_rel; /* occlusion-shadow dropout at depth edges */
  float fill;           /* value of a pixel without a measurement (any finite float) */
} t1render_depth_noise;
#define T1RENDER_DEPTH_MAXRING 16
int t1render_depth_model(const t1render_depth_noise* m, const void* clean, int32_t num_envs,
                         int32_t width, int32_t height, int32_t flags /* T1RENDER_DEPTH_F16: clean, ring, out are fp16 */,
                         uint32_t frame, void* ring, int32_t ring_frames /* K, 1..16 */,
                         const int32_t* lag /* (num_envs) or NULL = 0 */,
                         const uint8_t* fresh /* (num_envs) or NULL = none */,
                         void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
