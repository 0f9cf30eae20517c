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

#ifdef __cplusplus
}
#endif
#endif
