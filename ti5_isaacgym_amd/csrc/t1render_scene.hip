// t1render_scene.hip -- t1render_scene (include/t1render.h): the headless camera with every env's robot in the scene
// and shadows cast by the height field.
//
// A pixel cannot test num_envs robots, so the scene is culled twice on the device, both times conservatively:
//   k_scene_bounds  one lane per env: a padded bounding sphere (c, r) of the env's posed primitives into the workspace,
//                   and the lowest sphere bottom of the scene (an atomic min on an order-preserving key: the result
//                   does not depend on the order in which the atomics land);
//   k_scene_bits    one lane per env and a loop over the cameras: the env may matter to a camera when the capsule of
//                   radius r around the segment c .. c - s L meets the camera's frustum (the far end covers the
//                   robot's shadow, so a caster outside the view is kept; s reaches the lowest point that can receive
//                   a shadow -- the field's lowest sample or the lowest sphere bottom -- or T_MAX when L.z <= 0).  One
//                   bit per env and camera, a wave's 64 bits written by its first lane: no atomics.
//   k_scene         16 x 16 pixel workgroups as k_render.  A workgroup scans its camera's bits in env order, 256 envs
//                   at a time, repeats the capsule test against its own tile's frustum, compacts the survivors in env
//                   order (ballot and a prefix over the four waves) and poses them into LDS BATCH_ENVS envs at a time;
//                   every pixel tests the batch and keeps the smallest (t, env, primitive).  The scan runs twice: for
//                   the camera rays, then, from the hits, for the shadow rays.
// The capsule test rejects only when both ends lie more than the (padded) radius outside one frustum plane, so it never
// rejects a capsule that holds a point of the frustum.  With T1RENDER_SCENE_BRUTE the same loop takes every env; since
// both paths run the same intersections in the same order, the images are equal to the bit.
// Without OTHERS there is nothing to cull: k_scene_own is k_render's flow with the envs plane and the field's shadow.
// k_scene_bits, the tile-level scan and a pixel's surface and stores live in t1render_scene_dev.h: t1render_mesh.hip runs them too.
#include "t1render_scene_dev.h"

using namespace t1;

namespace {

constexpr int BATCH_ENVS = 8;        // envs posed into LDS at a time: 8 x T1RENDER_MAXPRIM x 80 bytes = 20 KiB
constexpr int FLAGS_ALL = T1RENDER_SCENE_OTHERS | T1RENDER_SCENE_TERRAIN_SHADOW | T1RENDER_SCENE_BRUTE;
static_assert(CHUNK == BATCH_ENVS * T1RENDER_MAXPRIM, "one lane poses one primitive of a batch");

struct Batch {
  WorldPrim prim[BATCH_ENVS * T1RENDER_MAXPRIM];
  int32_t env[BATCH_ENVS];
  Scan scan;
  Frame cam;
};

// primitive p posed by the env's rigid_state rows rs: the arithmetic of pose_scene (t1render.hip)
__device__ __forceinline__ void pose_prim(WorldPrim& P, const t1render_prim& p, const float* rs) {
  const float* b = rs + p.body * 13;
  const float x = b[3], y = b[4], z = b[5], w = b[6];
  const float R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                      2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                      2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    P.A[k] = b[k] + R[3 * k] * p.a[0] + R[3 * k + 1] * p.a[1] + R[3 * k + 2] * p.a[2];
    P.B[k] = p.kind == 0 ? p.b[k] : b[k] + R[3 * k] * p.b[0] + R[3 * k + 1] * p.b[1] + R[3 * k + 2] * p.b[2];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) P.R[k] = R[k];
  P.r = p.r;
  P.kind = p.kind;
  P.body = p.body;
  P.rgb = p.rgb;
}


__global__ __launch_bounds__(CHUNK) void k_scene_bounds(const SceneArgs A) {
  const int n = blockIdx.x * CHUNK + threadIdx.x;
  uint32_t key = 0xffffffffu;
  if (n < A.num_envs) {
    const float* rs = A.R.rigid_state + (size_t)n * 169;
    F3 lo = f3(INFINITY, INFINITY, INFINITY), hi = f3(-INFINITY, -INFINITY, -INFINITY);
    for (int p = 0; p < A.R.nprims; ++p) {
      WorldPrim P;
      pose_prim(P, A.R.prims[p], rs);
      if (P.kind == 0) {   // the box lies inside the sphere of its half diagonal
        const float hd = sqrtf(P.B[0] * P.B[0] + P.B[1] * P.B[1] + P.B[2] * P.B[2]);
        lo = f3(fminf(lo.x, P.A[0] - hd), fminf(lo.y, P.A[1] - hd), fminf(lo.z, P.A[2] - hd));
        hi = f3(fmaxf(hi.x, P.A[0] + hd), fmaxf(hi.y, P.A[1] + hd), fmaxf(hi.z, P.A[2] + hd));
      } else {
        const float r = fabsf(P.r);
        lo = f3(fminf(lo.x, fminf(P.A[0], P.B[0]) - r), fminf(lo.y, fminf(P.A[1], P.B[1]) - r),
                fminf(lo.z, fminf(P.A[2], P.B[2]) - r));
        hi = f3(fmaxf(hi.x, fmaxf(P.A[0], P.B[0]) + r), fmaxf(hi.y, fmaxf(P.A[1], P.B[1]) + r),
                fmaxf(hi.z, fmaxf(P.A[2], P.B[2]) + r));
      }
    }
    // the sphere around the primitives' bounding box, padded against the rounding of the poses (a quaternion is a unit
    // one to fp32 only) and of the coordinates themselves
    const F3 c = 0.5f * (lo + hi), e = hi - lo;
    float r = 0.5f * sqrtf(dot(e, e));
    r = r * 1.0001f + 4e-3f + 4e-6f * (fabsf(c.x) + fabsf(c.y) + fabsf(c.z));
    A.sphere[n] = make_float4(c.x, c.y, c.z, r);
    if (A.R.nprims > 0) key = min_key(c.z - r);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, s));
  if ((threadIdx.x & 63) == 0 && key != 0xffffffffu) atomicMin(A.zmin, key);
}


// Without OTHERS: the camera's own robot, k_render's flow (one posing, both casts over the same LDS primitives, an
// exact tie inside the robot goes to the later primitive as there) with the envs plane and the height field's shadow.
struct Own {
  WorldPrim prim[T1RENDER_MAXPRIM];
  Frame cam;
};
__global__ __launch_bounds__(CHUNK) void k_scene_own(const SceneArgs A) {
  __shared__ Own S;
  const RenderArgs& R = A.R;
  const int tid = threadIdx.y * TILE + threadIdx.x, cam = blockIdx.z;
  const int env = R.cams[cam].env;
  if (tid < R.nprims) pose_prim(S.prim[tid], R.prims[tid], R.rigid_state + (size_t)env * 169);
  else if (tid == T1RENDER_MAXPRIM) camera_frame(S.cam, R, cam);
  __syncthreads();
  const int j = blockIdx.x * TILE + threadIdx.x, i = blockIdx.y * TILE + threadIdx.y;
  if (j >= R.width || i >= R.height) return;   // edge tiles: no store outside the image
  const F3 o = f3(S.cam.eye[0], S.cam.eye[1], S.cam.eye[2]), d = pixel_ray(S.cam, R, i, j);
  float best = T_MAX;
  int face = 0, hp = -1, henv = env;
  for (int p = 0; p < R.nprims; ++p) {
    const WorldPrim& P = S.prim[p];
    int fc = 0;
    const float t = P.kind == 0 ? box_entry(P, o, d, fc) : capsule_entry(P, o, d);
    if (t > T_MIN && t <= best) {
      best = t;
      hp = p;
      face = fc;
    }
  }
  const Surface h = surface(R, o, d, best, hp, henv, [&](Surface& h, F3 hit) { prim_surface(h, S.prim[hp], face, hit); });
  float lit = 1.0f;
  if (h.need) {
    const F3 L = f3(R.style.light[0], R.style.light[1], R.style.light[2]);
    for (int p = 0; p < R.nprims; ++p) {
      const WorldPrim& P = S.prim[p];
      int fc = 0;
      const float t = P.kind == 0 ? box_entry(P, h.so, L, fc) : capsule_entry(P, h.so, L);
      if (t > 0.0f && t <= T_MAX) lit = 0.0f;
    }
  }
  store_pixel(A, h, lit, best, henv, cam, i, j);
}

// With OTHERS: poses the scene's next batch into LDS and returns its number of envs, 0 when the scene is exhausted.
// Every lane of the workgroup calls it, every decision in it is uniform.
__device__ int next_batch(Batch& S, const SceneArgs& A, const Frustum& Fr, float z_floor, int cam, int tid, Cursor& c) {
  __syncthreads();   // every lane is done with the previous batch
  if (!scan_on(S.scan, A, Fr, z_floor, cam, tid, c)) return 0;
  const int ne = min(BATCH_ENVS, c.m - c.sb);
  const int slot = tid / T1RENDER_MAXPRIM, p = tid % T1RENDER_MAXPRIM;
  if (slot < ne && p < A.R.nprims) {
    const int env = S.scan.surv[c.sb + slot];
    pose_prim(S.prim[tid], A.R.prims[p], A.R.rigid_state + (size_t)env * 169);
    if (p == 0) S.env[slot] = env;
  }
  c.sb += ne;
  __syncthreads();
  return ne;
}

__global__ __launch_bounds__(CHUNK) void k_scene(const SceneArgs A) {
  __shared__ Batch S;
  const RenderArgs& R = A.R;
  const int tid = threadIdx.y * TILE + threadIdx.x, cam = blockIdx.z;
  if (tid == 0) camera_frame(S.cam, R, cam);
  __syncthreads();
  const int j = blockIdx.x * TILE + threadIdx.x, i = blockIdx.y * TILE + threadIdx.y;
  const bool inside = j < R.width && i < R.height;   // edge tiles: no store outside the image
  const bool cull = !(A.flags & T1RENDER_SCENE_BRUTE);
  // the tile's pyramid, from pixel edge to pixel edge (half a pixel wider than its rays)
  const Frustum Fr = make_frustum(S.cam, 2.0f * (float)(blockIdx.x * TILE) / (float)R.width - 1.0f,
                                  2.0f * (float)(blockIdx.x * TILE + TILE) / (float)R.width - 1.0f,
                                  1.0f - 2.0f * (float)(blockIdx.y * TILE + TILE) / (float)R.height,
                                  1.0f - 2.0f * (float)(blockIdx.y * TILE) / (float)R.height);
  const float z_floor = cull ? scene_floor(A) : 0.0f;
  const F3 o = f3(S.cam.eye[0], S.cam.eye[1], S.cam.eye[2]), d = pixel_ray(S.cam, R, i, j);
  float best = T_MAX;
  int face = 0, hp = -1, henv = -1;
  Cursor cur = {0, 0, 0};
  for (int ne = next_batch(S, A, Fr, z_floor, cam, tid, cur); ne > 0; ne = next_batch(S, A, Fr, z_floor, cam, tid, cur)) {
    if (!inside) continue;
    for (int s = 0; s < ne; ++s) {
      for (int p = 0; p < R.nprims; ++p) {
        const WorldPrim& P = S.prim[s * T1RENDER_MAXPRIM + p];
        int fc = 0;
        const float t = P.kind == 0 ? box_entry(P, o, d, fc) : capsule_entry(P, o, d);
        // envs and primitives come in ascending order: a later one wins only when it is nearer
        if (t > T_MIN && t <= T_MAX && (t < best || hp < 0)) {
          best = t;
          hp = p;
          henv = S.env[s];
          face = fc;
        }
      }
    }
  }
  Surface h = {f3(0, 0, 1), f3(0, 0, 0), f3(0, 0, 0), f3(0, 0, 0), 0.0f, -1, false, false};
  if (inside)   // the batch that held the hit primitive is gone: pose that one again
    h = surface(R, o, d, best, hp, henv, [&](Surface& h, F3 hit) {
      WorldPrim P;
      pose_prim(P, R.prims[hp], R.rigid_state + (size_t)henv * 169);
      prim_surface(h, P, face, hit);
    });
  float lit = 1.0f;
  if (__syncthreads_or(h.need)) {   // the shadow rays against the same scene
    const F3 L = f3(R.style.light[0], R.style.light[1], R.style.light[2]);
    cur = Cursor{0, 0, 0};
    for (int ne = next_batch(S, A, Fr, z_floor, cam, tid, cur); ne > 0; ne = next_batch(S, A, Fr, z_floor, cam, tid, cur)) {
      if (!h.need || lit == 0.0f) continue;
      for (int s = 0; s < ne && lit != 0.0f; ++s) {
        for (int p = 0; p < R.nprims; ++p) {
          const WorldPrim& P = S.prim[s * T1RENDER_MAXPRIM + p];
          int fc = 0;
          const float t = P.kind == 0 ? box_entry(P, h.so, L, fc) : capsule_entry(P, h.so, L);
          if (t > 0.0f && t <= T_MAX) lit = 0.0f;
        }
      }
    }
  }
  if (inside) store_pixel(A, h, lit, best, henv, cam, i, j);
}


}  // namespace

extern "C" long long t1render_scene_workspace_bytes(int32_t num_envs, int32_t ncams) {
  if (num_envs < 0 || ncams < 1 || ncams > T1RENDER_MAXCAM) return -1;
  return scene_workspace_bytes(num_envs, ncams, nullptr);
}

extern "C" int t1render_scene(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_prim* prims,
                              int32_t nprims, const t1render_style* style, int32_t flags, int32_t width, int32_t height,
                              uint32_t* rgba, float* depth, int32_t* ids, int32_t* envs, void* workspace,
                              long long workspace_bytes_, void* stream) {
  if (!env || !cams || !prims || !style || !rgba) return t1_fail(T1ENV_E_ARG, "t1render_scene: null argument");
  if (ncams < 1 || ncams > T1RENDER_MAXCAM) return t1_fail(T1ENV_E_ARG, "t1render_scene: ncams outside [1, 16]");
  if (nprims < 0 || nprims > T1RENDER_MAXPRIM) return t1_fail(T1ENV_E_ARG, "t1render_scene: nprims outside [0, 32]");
  if (width < 1 || height < 1) return t1_fail(T1ENV_E_ARG, "t1render_scene: width and height must be >= 1");
  if (flags & ~FLAGS_ALL) return t1_fail(T1ENV_E_ARG, "t1render_scene: unknown flag");
  RenderView v;
  t1_render_view(env, &v);
  SceneArgs S = {};
  RenderArgs& A = S.R;
  for (int c = 0; c < ncams; ++c) {
    const t1render_camera& C = cams[c];
    if (C.env < 0 || C.env >= v.num_envs) return t1_fail(T1ENV_E_ARG, "t1render_scene: a camera's env is out of range");
    // follow mode adds the same base position to eye and target: the view direction is that of the offsets
    const double f[3] = {(double)C.target[0] - C.eye[0], (double)C.target[1] - C.eye[1], (double)C.target[2] - C.eye[2]};
    const double u[3] = {C.up[0], C.up[1], C.up[2]};
    const double x[3] = {f[1] * u[2] - f[2] * u[1], f[2] * u[0] - f[0] * u[2], f[0] * u[1] - f[1] * u[0]};
    const double ff = f[0] * f[0] + f[1] * f[1] + f[2] * f[2], uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const double xx = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (!(xx > 1e-12 * ff * uu)) return t1_fail(T1ENV_E_ARG, "t1render_scene: a camera's up is parallel to its view");
    if (!(C.vfov > 0.0f && C.vfov < 3.14159f)) return t1_fail(T1ENV_E_ARG, "t1render_scene: vfov outside (0, pi)");
    A.cams[c] = C;
  }
  for (int p = 0; p < nprims; ++p) {
    if (prims[p].body < 0 || prims[p].body >= T1_NB) return t1_fail(T1ENV_E_ARG, "t1render_scene: a primitive's body is out of range");
    if (prims[p].kind != 0 && prims[p].kind != 1) return t1_fail(T1ENV_E_ARG, "t1render_scene: a primitive's kind is not 0 or 1");
    A.prims[p] = prims[p];
  }
  if (v.terrain.type != 0 && !v.terrain.h) return t1_fail(T1ENV_E_STATE, "t1render_scene: no terrain set");
  A.style = *style;
  const double ll = sqrt((double)style->light[0] * style->light[0] + (double)style->light[1] * style->light[1] +
                         (double)style->light[2] * style->light[2]);
  if (!(ll > 0.0)) return t1_fail(T1ENV_E_ARG, "t1render_scene: zero light direction");
  for (int k = 0; k < 3; ++k) A.style.light[k] = (float)(style->light[k] / ll);
  const bool cull = (flags & T1RENDER_SCENE_OTHERS) && !(flags & T1RENDER_SCENE_BRUTE);
  long long words = 0;
  const long long need = scene_workspace_bytes(v.num_envs, ncams, &words);
  if (cull && !workspace) return t1_fail(T1ENV_E_ARG, "t1render_scene: OTHERS needs a workspace");
  if (workspace) {
    if ((uintptr_t)workspace % 16) return t1_fail(T1ENV_E_ARG, "t1render_scene: the workspace is not 16-byte aligned");
    if (workspace_bytes_ < need) return t1_fail(T1ENV_E_ARG, "t1render_scene: the workspace is smaller than t1render_scene_workspace_bytes");
  }
  A.rigid_state = v.rigid_state;
  A.h = v.terrain.h;
  A.rows = v.terrain.rows;
  A.cols = v.terrain.cols;
  A.hf = v.terrain.type != 0;
  A.inv_hscale = v.terrain.inv_hscale;
  A.hscale = v.terrain.hscale;
  A.vscale = v.terrain.vscale;
  A.border = v.terrain.border;
  A.z_top = v.z_top + 1e-3f * (1.0f + fabsf(v.z_top));
  A.width = width;
  A.height = height;
  A.nprims = nprims;
  A.rgba = rgba;
  A.depth = depth;
  A.ids = ids;
  S.envs = envs;
  S.flags = flags;
  S.num_envs = v.num_envs;
  S.ncams = ncams;
  S.words = (int32_t)words;
  S.z_bot = v.z_bot - 1e-3f * (1.0f + fabsf(v.z_bot));
  const hipStream_t st = (hipStream_t)stream;
  if (cull) {
    char* ws = (char*)workspace;
    S.sphere = (float4*)ws;
    S.bits = (uint32_t*)(ws + 16 * (size_t)v.num_envs);
    S.zmin = S.bits + (size_t)ncams * words;
    hipError_t err = hipMemsetAsync(S.zmin, 0xff, sizeof(uint32_t), st);
    if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
    const dim3 pre((v.num_envs + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL(k_scene_bounds, pre, dim3(CHUNK), 0, st, S);
    hipLaunchKernelGGL(k_scene_bits, pre, dim3(CHUNK), 0, st, S);
    err = hipGetLastError();
    if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
  }
  const dim3 grid((width + TILE - 1) / TILE, (height + TILE - 1) / TILE, ncams);
  if (flags & T1RENDER_SCENE_OTHERS) hipLaunchKernelGGL(k_scene, grid, dim3(TILE, TILE), 0, st, S);
  else hipLaunchKernelGGL(k_scene_own, grid, dim3(TILE, TILE), 0, st, S);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
  return 0;
}
