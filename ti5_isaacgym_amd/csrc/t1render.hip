// t1render.hip -- the headless camera (include/t1render.h): one launch ray-casts every camera of the call.
//
// One lane per pixel, 16 x 16 pixel workgroups (a wave is a compact 16 x 4 block of rays, so its lanes mostly take
// the same branches), grid (tiles_x, tiles_y, ncams).  Per workgroup the first lanes pose the camera's env's
// primitives from rigid_state into LDS in world coordinates (every later read of them is an LDS broadcast); cameras,
// primitives and style travel as kernel arguments, so a call allocates and copies nothing.  Boxes are slab-tested in
// the body frame, capsules are the first entry into two spheres and the cylinder between them, and the height field is
// walked cell by cell (2-D DDA from the ray's entry into the footprint), both triangles of a cell solved in closed form
// in the cell's own coordinates -- the triangles terrain_height<true> (t1_dynamics.h) interpolates.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/t1render.h"
#include "t1env_internal.h"

using namespace t1;

namespace {

constexpr int TILE = 16;
constexpr float T_MIN = 0.05f, T_MAX = 200.0f, SHADOW_EPS = 1e-3f;
constexpr float EDGE_TOL = 1e-5f;   // slack of the in-triangle test [cells]: neighbouring triangles overlap by it, so a
                                    // ray along a shared edge or through a vertex cannot slip between them

struct RenderArgs {
  const float* rigid_state;
  const int16_t* h;
  int32_t rows, cols, hf;
  float inv_hscale, hscale, vscale, border;
  float z_top;   // nothing of the height field lies above it (its highest sample plus a margin)
  int32_t width, height, nprims;
  uint32_t* rgba;
  float* depth;
  int32_t* ids;
  t1render_style style;
  t1render_camera cams[T1RENDER_MAXCAM];
  t1render_prim prims[T1RENDER_MAXPRIM];
};

struct F3 {
  float x, y, z;
};
__device__ __forceinline__ F3 f3(float x, float y, float z) { return F3{x, y, z}; }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ F3 operator-(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ F3 operator*(float s, F3 a) { return f3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ F3 cross(F3 a, F3 b) {
  return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ F3 normalize(F3 a) { return (1.0f / sqrtf(dot(a, a))) * a; }

// a primitive in world coordinates (LDS).  Box: A the centre, B the half extents, R the body-to-world rotation (row
// major).  Capsule: A, B the segment's ends, r the radius.
struct WorldPrim {
  float A[3], B[3], r, R[9];
  int32_t kind, body;
  uint32_t rgb;
};
struct Scene {
  WorldPrim prim[T1RENDER_MAXPRIM];
  float eye[3], f[3], r[3], u[3];   // the camera: r and u already scaled by tan(vfov/2) (r by the aspect too)
};

// entry of the ray into a sphere (the smaller root), +inf when the line misses it
__device__ __forceinline__ float sphere_entry(F3 oc, F3 d, float r) {
  const float b = dot(oc, d), c = dot(oc, oc) - r * r, h = b * b - c;
  return h >= 0.0f ? -b - sqrtf(h) : INFINITY;
}

// Entry of the line o + t d (|d| = 1) into the capsule: the smallest of its entries into the two end spheres and into
// the cylinder's lateral surface between the ends (an entry through an end disc lies inside that end's sphere).
// +inf on a miss; negative when the origin is inside or past it (the caller's range test drops those).
__device__ __forceinline__ float capsule_entry(const WorldPrim& P, F3 o, F3 d) {
  const F3 a = f3(P.A[0], P.A[1], P.A[2]), b = f3(P.B[0], P.B[1], P.B[2]);
  const F3 ba = b - a, oa = o - a;
  float t = sphere_entry(oa, d, P.r);
  const float baba = dot(ba, ba);
  if (baba > 0.0f) {
    t = fminf(t, sphere_entry(o - b, d, P.r));
    const float bard = dot(ba, d), baoa = dot(ba, oa), rdoa = dot(d, oa), oaoa = dot(oa, oa);
    const float qa = baba - bard * bard, qb = baba * rdoa - baoa * bard;
    const float qc = baba * oaoa - baoa * baoa - P.r * P.r * baba;
    const float h = qb * qb - qa * qc;
    if (qa > 0.0f && h >= 0.0f) {
      const float tc = (-qb - sqrtf(h)) / qa, y = baoa + tc * bard;
      if (y > 0.0f && y < baba) t = fminf(t, tc);
    }
  }
  return t;
}

// Entry of the line into the box (slab test in the body frame); face = axis (0..2), + 4 when the entered face is the
// positive one.  +inf on a miss, negative when the origin is inside or past it.
__device__ __forceinline__ float box_entry(const WorldPrim& P, F3 o, F3 d, int& face) {
  const F3 oc = o - f3(P.A[0], P.A[1], P.A[2]);
  const float ob[3] = {P.R[0] * oc.x + P.R[3] * oc.y + P.R[6] * oc.z, P.R[1] * oc.x + P.R[4] * oc.y + P.R[7] * oc.z,
                       P.R[2] * oc.x + P.R[5] * oc.y + P.R[8] * oc.z};
  const float db[3] = {P.R[0] * d.x + P.R[3] * d.y + P.R[6] * d.z, P.R[1] * d.x + P.R[4] * d.y + P.R[7] * d.z,
                       P.R[2] * d.x + P.R[5] * d.y + P.R[8] * d.z};
  float tn = -INFINITY, tf = INFINITY;
  int fc = 0;
  bool miss = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (db[k] != 0.0f) {
      const float inv = 1.0f / db[k];
      const float t1 = (-P.B[k] - ob[k]) * inv, t2 = (P.B[k] - ob[k]) * inv;
      const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
      if (lo > tn) { tn = lo; fc = k + (db[k] < 0.0f ? 4 : 0); }
      tf = fminf(tf, hi);
    } else if (fabsf(ob[k]) > P.B[k]) {
      miss = true;
    }
  }
  face = fc;
  return (miss || tn > tf) ? INFINITY : tn;
}

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

// The height field's nearest hit in (T_MIN, best]: true and best, n (the upward unit normal) updated.
__device__ bool cast_heightfield(const RenderArgs& A, F3 o, F3 d, float& best, F3& n) {
  const float ih = A.inv_hscale;
  const float og[2] = {(o.x + A.border) * ih, (o.y + A.border) * ih}, dg[2] = {d.x * ih, d.y * ih};
  const int last[2] = {A.rows - 2, A.cols - 2};   // last cell of each axis
  float t0 = T_MIN, t1 = best;
#pragma unroll
  for (int k = 0; k < 2; ++k) {   // the footprint [0, rows-1] x [0, cols-1] in cells
    const float ext = (float)(last[k] + 1);
    if (dg[k] != 0.0f) {
      const float inv = 1.0f / dg[k];
      const float ta = -og[k] * inv, tb = (ext - og[k]) * inv;
      t0 = fmaxf(t0, fminf(ta, tb));
      t1 = fminf(t1, fmaxf(ta, tb));
    } else if (og[k] < 0.0f || og[k] > ext) {
      return false;
    }
  }
  // the ray can hit only where it is below the field's top: sky rays stop there, descending rays start there
  if (d.z != 0.0f) {
    const float tz = (A.z_top - o.z) / d.z;
    if (d.z > 0.0f) t1 = fminf(t1, tz); else t0 = fmaxf(t0, tz);
  } else if (o.z > A.z_top) {
    return false;
  }
  if (!(t0 <= t1)) return false;
  int c[2], step[2];
  float inv[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int ck = (int)floorf(og[k] + t0 * dg[k]);
    c[k] = min(max(ck, 0), last[k]);
    step[k] = dg[k] > 0.0f ? 1 : -1;
    inv[k] = dg[k] != 0.0f ? 1.0f / dg[k] : 0.0f;
  }
  const float vs = A.vscale;
  const int cap = A.rows + A.cols + 2;
  for (int it = 0; it < cap; ++it) {
    // c stays inside [0, rows-2] x [0, cols-2]: the four samples of the cell are inside the field
    const int16_t* r0 = A.h + ((size_t)c[0] * A.cols + c[1]);
    const float h00 = vs * r0[0], h01 = vs * r0[1], h10 = vs * r0[A.cols], h11 = vs * r0[A.cols + 1];
    const float u0 = og[0] - (float)c[0], v0 = og[1] - (float)c[1];
    float tc = INFINITY;
    F3 nc = f3(0, 0, 1);
#pragma unroll
    for (int tri = 0; tri < 2; ++tri) {   // 0: u >= v, (i,j)-(i+1,j)-(i+1,j+1); 1: u <= v, (i,j)-(i+1,j+1)-(i,j+1)
      const float a = tri == 0 ? h10 - h00 : h11 - h01, b = tri == 0 ? h11 - h10 : h01 - h00;
      const float den = d.z - a * dg[0] - b * dg[1];
      if (den != 0.0f) {
        const float t = (h00 + u0 * a + v0 * b - o.z) / den;
        const float u = u0 + t * dg[0], v = v0 + t * dg[1];
        const bool in = u >= -EDGE_TOL && u <= 1.0f + EDGE_TOL && v >= -EDGE_TOL && v <= 1.0f + EDGE_TOL &&
                        (tri == 0 ? u - v >= -EDGE_TOL : v - u >= -EDGE_TOL);
        if (in && t > T_MIN && t <= best && t < tc) {
          tc = t;
          nc = f3(-a * ih, -b * ih, 1.0f);
        }
      }
    }
    if (tc < INFINITY) {
      best = tc;
      n = normalize(nc);
      return true;
    }
    // leave the cell through its nearer wall; stop at the footprint's edge or past the nearest hit so far
    const float tx = dg[0] != 0.0f ? ((float)(c[0] + (step[0] > 0 ? 1 : 0)) - og[0]) * inv[0] : INFINITY;
    const float ty = dg[1] != 0.0f ? ((float)(c[1] + (step[1] > 0 ? 1 : 0)) - og[1]) * inv[1] : INFINITY;
    const int k = tx <= ty ? 0 : 1;
    if (fminf(tx, ty) > t1) return false;
    c[k] += step[k];
    if (c[k] < 0 || c[k] > last[k]) return false;
  }
  return false;
}

__device__ __forceinline__ uint32_t pack_rgb(F3 c) {
  const uint32_t r = (uint32_t)floorf(fminf(fmaxf(c.x, 0.0f), 1.0f) * 255.0f + 0.5f);
  const uint32_t g = (uint32_t)floorf(fminf(fmaxf(c.y, 0.0f), 1.0f) * 255.0f + 0.5f);
  const uint32_t b = (uint32_t)floorf(fminf(fmaxf(c.z, 0.0f), 1.0f) * 255.0f + 0.5f);
  return r | (g << 8) | (b << 16) | 0xff000000u;
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
    ground = cast_heightfield(A, o, d, best, n);
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
