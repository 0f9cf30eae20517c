// t1render.hip -- the headless camera (include/t1render.h): one launch ray-casts every camera of the call.
//
// One lane per pixel, 16 x 16 pixel workgroups (a wave is a compact 16 x 4 block of rays, so its lanes mostly take
// the same branches), grid (tiles_x, tiles_y, ncams).  Per workgroup the first lanes pose the camera's env's
// primitives from rigid_state into LDS in world coordinates (every later read of them is an LDS broadcast); cameras,
// primitives and style travel as kernel arguments, so a call allocates and copies nothing.  Boxes are slab-tested in
// the body frame, capsules are the first entry into two spheres and the cylinder between them, and the height field is
// walked cell by cell (2-D DDA from the ray's entry into the footprint), both triangles of a cell solved in closed form
// in the cell's own coordinates -- the triangles terrain_height<true> (t1_dynamics.h) interpolates.
#include "t1render_dev.h"

using namespace t1;

namespace {

struct Scene {
  WorldPrim prim[T1RENDER_MAXPRIM];
  float eye[3], f[3], r[3], u[3];   // the camera: r and u already scaled by tan(vfov/2) (r by the aspect too)
};

// nearest primitive entered in (tlo, best]: its index or -1; best and face are updated on a hit
__device__ __forceinline__ int cast_prims(const Scene& S, int nprims, F3 o, F3 d, float tlo, float& best, int& face) {
  int hit = -1;
  for (int p = 0; p < nprims; ++p) {
    const WorldPrim& P = S.prim[p];
    int fc = 0;
    const float t = P.kind == 0 ? box_entry(P, o, d, fc) : capsule_entry(P, o, d);
    if (t > tlo && t <= best) {
      best = t;
      hit = p;
      face = fc;
    }
  }
  return hit;
}

// lane tid's share of posing camera cam's scene: primitive tid, or (lane T1RENDER_MAXPRIM) the camera's frame
__device__ __forceinline__ void pose_scene(Scene& S, const RenderArgs& A, int cam, int tid) {
  const t1render_camera& C = A.cams[cam];
  const float* rs = A.rigid_state + (size_t)C.env * 169;
  if (tid < A.nprims) {   // pose primitive tid
    const t1render_prim& p = A.prims[tid];
    const float* b = rs + p.body * 13;
    const float x = b[3], y = b[4], z = b[5], w = b[6];
    const float R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                        2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
    WorldPrim& P = S.prim[tid];
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
  } else if (tid == T1RENDER_MAXPRIM) {   // the camera's frame
    F3 eye = f3(C.eye[0], C.eye[1], C.eye[2]), tgt = f3(C.target[0], C.target[1], C.target[2]);
    if (C.follow) {
      const F3 base = f3(rs[0], rs[1], rs[2]);
      eye = eye + base;
      tgt = tgt + base;
    }
    const F3 f = normalize(tgt - eye), r = normalize(cross(f, f3(C.up[0], C.up[1], C.up[2]))), u = cross(r, f);
    const float th = tanf(0.5f * C.vfov), ta = th * (float)A.width / (float)A.height;
    S.eye[0] = eye.x; S.eye[1] = eye.y; S.eye[2] = eye.z;
    S.f[0] = f.x; S.f[1] = f.y; S.f[2] = f.z;
    S.r[0] = ta * r.x; S.r[1] = ta * r.y; S.r[2] = ta * r.z;
    S.u[0] = th * u.x; S.u[1] = th * u.y; S.u[2] = th * u.z;
  }
}

// pixel (row i, column j) of camera cam: cast, shade, store
__device__ __forceinline__ void shade_pixel(const Scene& S, const RenderArgs& A, int cam, int i, int j) {
  const float px = 2.0f * ((float)j + 0.5f) / (float)A.width - 1.0f;
  const float py = 1.0f - 2.0f * ((float)i + 0.5f) / (float)A.height;
  const F3 o = f3(S.eye[0], S.eye[1], S.eye[2]);
  const F3 d = normalize(f3(S.f[0] + px * S.r[0] + py * S.u[0], S.f[1] + px * S.r[1] + py * S.u[1],
                            S.f[2] + px * S.r[2] + py * S.u[2]));
  float best = T_MAX;
  int face = 0;
  const int hp = cast_prims(S, A.nprims, o, d, T_MIN, best, face);
  F3 n = f3(0, 0, 1);
  bool ground = false;
  if (A.hf) {
    ground = cast_heightfield(A, o, d, T_MIN, best, n);
  } else if (d.z != 0.0f) {
    const float t = -o.z / d.z;
    if (t > T_MIN && t <= best) {
      best = t;
      ground = true;
    }
  }
  const t1render_style& St = A.style;
  F3 col;
  int id;
  if (!ground && hp < 0) {
    const float s = 0.5f * (d.z + 1.0f);
    col = f3(St.sky_rgb[0][0] + s * (St.sky_rgb[1][0] - St.sky_rgb[0][0]),
             St.sky_rgb[0][1] + s * (St.sky_rgb[1][1] - St.sky_rgb[0][1]),
             St.sky_rgb[0][2] + s * (St.sky_rgb[1][2] - St.sky_rgb[0][2]));
    id = -1;
    best = INFINITY;
  } else {
    const F3 hit = o + best * d;
    F3 base;
    if (ground) {
      const int par = ((int)floorf(hit.x) + (int)floorf(hit.y)) & 1;
      base = f3(St.terrain_rgb[par][0], St.terrain_rgb[par][1], St.terrain_rgb[par][2]);
      id = 0;
    } else {
      const WorldPrim& P = S.prim[hp];
      if (P.kind == 0) {
        const int k = face & 3;
        const float sg = (face & 4) ? 1.0f : -1.0f;
        n = f3(sg * P.R[k], sg * P.R[3 + k], sg * P.R[6 + k]);
      } else {
        const F3 a = f3(P.A[0], P.A[1], P.A[2]), ba = f3(P.B[0], P.B[1], P.B[2]) - a;
        const float baba = dot(ba, ba);
        const float s = baba > 0.0f ? fminf(fmaxf(dot(hit - a, ba) / baba, 0.0f), 1.0f) : 0.0f;
        n = normalize(hit - (a + s * ba));
      }
      base = f3((float)(P.rgb & 255u) * (1.0f / 255.0f), (float)((P.rgb >> 8) & 255u) * (1.0f / 255.0f),
                (float)((P.rgb >> 16) & 255u) * (1.0f / 255.0f));
      id = 1 + P.body;
    }
    const F3 L = f3(St.light[0], St.light[1], St.light[2]);
    const float nl = fmaxf(dot(n, L), 0.0f);
    float lit = 1.0f;
    if (nl > 0.0f) {   // a surface facing away from the light needs no shadow ray
      float sb = T_MAX;
      int sf = 0;
      if (cast_prims(S, A.nprims, hit + SHADOW_EPS * n, L, 0.0f, sb, sf) >= 0) lit = 0.0f;
    }
    col = (St.ambient + (1.0f - St.ambient) * nl * lit) * base;
  }
  const size_t px_i = ((size_t)cam * A.height + i) * A.width + j;
  A.rgba[px_i] = pack_rgb(col);
  if (A.depth) A.depth[px_i] = best;
  if (A.ids) A.ids[px_i] = id;
}

__global__ __launch_bounds__(TILE * TILE) void k_render(const RenderArgs A) {
  __shared__ Scene S;
  pose_scene(S, A, blockIdx.z, threadIdx.y * TILE + threadIdx.x);
  __syncthreads();
  const int j = blockIdx.x * TILE + threadIdx.x, i = blockIdx.y * TILE + threadIdx.y;
  if (j < A.width && i < A.height) shade_pixel(S, A, blockIdx.z, i, j);   // edge tiles: no store outside the image
}

}  // namespace

extern "C" int t1render_frame(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_prim* prims,
                              int32_t nprims, const t1render_style* style, int32_t width, int32_t height,
                              uint32_t* rgba, float* depth, int32_t* ids, void* stream) {
  if (!env || !cams || !prims || !style || !rgba) return t1_fail(T1ENV_E_ARG, "t1render_frame: null argument");
  if (ncams < 1 || ncams > T1RENDER_MAXCAM) return t1_fail(T1ENV_E_ARG, "t1render_frame: ncams outside [1, 16]");
  if (nprims < 0 || nprims > T1RENDER_MAXPRIM) return t1_fail(T1ENV_E_ARG, "t1render_frame: nprims outside [0, 32]");
  if (width < 1 || height < 1) return t1_fail(T1ENV_E_ARG, "t1render_frame: width and height must be >= 1");
  RenderView v;
  t1_render_view(env, &v);
  RenderArgs A = {};
  for (int c = 0; c < ncams; ++c) {
    const t1render_camera& C = cams[c];
    if (C.env < 0 || C.env >= v.num_envs) return t1_fail(T1ENV_E_ARG, "t1render_frame: a camera's env is out of range");
    // follow mode adds the same base position to eye and target: the view direction is that of the offsets
    const double f[3] = {(double)C.target[0] - C.eye[0], (double)C.target[1] - C.eye[1], (double)C.target[2] - C.eye[2]};
    const double u[3] = {C.up[0], C.up[1], C.up[2]};
    const double x[3] = {f[1] * u[2] - f[2] * u[1], f[2] * u[0] - f[0] * u[2], f[0] * u[1] - f[1] * u[0]};
    const double ff = f[0] * f[0] + f[1] * f[1] + f[2] * f[2], uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const double xx = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (!(xx > 1e-12 * ff * uu)) return t1_fail(T1ENV_E_ARG, "t1render_frame: a camera's up is parallel to its view");
    if (!(C.vfov > 0.0f && C.vfov < 3.14159f)) return t1_fail(T1ENV_E_ARG, "t1render_frame: vfov outside (0, pi)");
    A.cams[c] = C;
  }
  for (int p = 0; p < nprims; ++p) {
    if (prims[p].body < 0 || prims[p].body >= T1_NB) return t1_fail(T1ENV_E_ARG, "t1render_frame: a primitive's body is out of range");
    if (prims[p].kind != 0 && prims[p].kind != 1) return t1_fail(T1ENV_E_ARG, "t1render_frame: a primitive's kind is not 0 or 1");
    A.prims[p] = prims[p];
  }
  if (v.terrain.type != 0 && !v.terrain.h) return t1_fail(T1ENV_E_STATE, "t1render_frame: no terrain set");
  A.style = *style;
  const double ll = sqrt((double)style->light[0] * style->light[0] + (double)style->light[1] * style->light[1] +
                         (double)style->light[2] * style->light[2]);
  if (!(ll > 0.0)) return t1_fail(T1ENV_E_ARG, "t1render_frame: zero light direction");
  for (int k = 0; k < 3; ++k) A.style.light[k] = (float)(style->light[k] / ll);
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
  const dim3 grid((width + TILE - 1) / TILE, (height + TILE - 1) / TILE, ncams);
  hipLaunchKernelGGL(k_render, grid, dim3(TILE, TILE), 0, (hipStream_t)stream, A);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
  return 0;
}
