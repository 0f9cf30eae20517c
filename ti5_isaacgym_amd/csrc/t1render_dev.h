// t1render_dev.h -- what the renderer's units (t1render.hip: one robot per camera; t1render_scene.hip: every env's
// robot, culled; t1render_mesh.hip; t1render_depth.hip: every env's mounted depth sensor) share on the device: the kernel's view of the terrain and the call, the ray / primitive intersections,
// the height field's walk and the colour packing.  All units must see one text of these, so that a pixel of any
// kernel that meets the same primitives computes the same bits.
#ifndef T1RENDER_DEV_H
#define T1RENDER_DEV_H

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/t1render.h"
#include "t1env_internal.h"

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

// The height field's nearest hit in (tmin, best]: true and best, n (the upward unit normal) updated.  Field: any view
// with h, rows, cols, inv_hscale, vscale, border and z_top (RenderArgs; the depth sensor's narrower DepthArgs).
template <class Field>
__device__ bool cast_heightfield(const Field& A, F3 o, F3 d, float tmin, float& best, F3& n) {
  const float ih = A.inv_hscale;
  const float og[2] = {(o.x + A.border) * ih, (o.y + A.border) * ih}, dg[2] = {d.x * ih, d.y * ih};
  const int last[2] = {A.rows - 2, A.cols - 2};   // last cell of each axis
  float t0 = tmin, t1 = best;
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
        if (in && t > tmin && t <= best && t < tc) {
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

}  // namespace
#endif
