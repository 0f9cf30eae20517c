// t1render_scene_dev.h -- what the two scene-level units (t1render_scene.hip: every env's primitives; t1render_mesh.hip:
// every env's triangle meshes) share on top of t1render_dev.h: the call's scene, the camera's frame and frustum, the
// culling pre-pass's bit kernel, the tile-level scan, and a pixel's surface and stores.  Both units must see one text of
// these, so that both cull alike and a pixel of either that meets the same terrain computes the same bits.
// t1render.hip, which draws one robot per camera, does not include it.
#ifndef T1RENDER_SCENE_DEV_H
#define T1RENDER_SCENE_DEV_H

#include "t1render_dev.h"

namespace {

constexpr int CHUNK = TILE * TILE;   // envs scanned per step, one per lane

struct SceneArgs {
  RenderArgs R;
  int32_t* envs;
  int32_t flags, num_envs, ncams, words;   // words: 32-bit visibility words per camera, 2 per 64 envs
  float4* sphere;                          // workspace: (num_envs) c.xyz, r
  uint32_t* bits;                          //            (ncams, words)
  uint32_t* zmin;                          //            key of the lowest sphere bottom
  float z_bot;                             // below the height field's lowest sample (the plane: below 0)
};

struct Frame {
  float eye[3], f[3], r[3], u[3];   // as Scene's camera in t1render.hip: r and u scaled by tan(vfov/2) (r by the aspect)
};
struct Frustum {
  F3 eye, n[4];   // inward unit normals of the four side planes through the eye
};
struct Cursor {   // uniform over the workgroup
  int base, m, sb;   // next env to scan; survivors of the scanned chunk; the first one not yet posed
};

// order-preserving key of a float for an unsigned min
__device__ __forceinline__ uint32_t min_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the camera's frame: the arithmetic of pose_scene (t1render.hip)
__device__ __forceinline__ void camera_frame(Frame& S, const RenderArgs& A, int cam) {
  const t1render_camera& C = A.cams[cam];
  const float* rs = A.rigid_state + (size_t)C.env * 169;
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

// The pyramid of the rays f + x r + y u with x in [x0, x1], y in [y0, y1] (image coordinates in [-1, 1]).  With
// q = p - eye = a f + b r/|r| + ..., p is on the inner side of the x0 plane when b >= x0 |r| a, i.e. q.(r - x0 |r|^2 f) >= 0.
__device__ __forceinline__ Frustum make_frustum(const Frame& S, float x0, float x1, float y0, float y1) {
  const F3 f = f3(S.f[0], S.f[1], S.f[2]), r = f3(S.r[0], S.r[1], S.r[2]), u = f3(S.u[0], S.u[1], S.u[2]);
  const float rr = dot(r, r), uu = dot(u, u);
  Frustum F;
  F.eye = f3(S.eye[0], S.eye[1], S.eye[2]);
  F.n[0] = normalize(r - (x0 * rr) * f);
  F.n[1] = normalize((x1 * rr) * f - r);
  F.n[2] = normalize(u - (y0 * uu) * f);
  F.n[3] = normalize((y1 * uu) * f - u);
  return F;
}

// true only when the capsule of radius r around a .. b lies wholly outside one plane.  The margin beside r covers the
// rounding of q and of the plane's normal; a NaN anywhere compares false and keeps the env.
__device__ __forceinline__ bool capsule_outside(const Frustum& F, F3 a, F3 b, float r) {
  const F3 qa = a - F.eye, qb = b - F.eye;
  const float ma = -(r + 8e-6f * (fabsf(qa.x) + fabsf(qa.y) + fabsf(qa.z)));
  const float mb = -(r + 8e-6f * (fabsf(qb.x) + fabsf(qb.y) + fabsf(qb.z)));
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (dot(qa, F.n[k]) < ma && dot(qb, F.n[k]) < mb) return true;
  return false;
}

// The far end of the segment a sphere's shadow sweeps: a point h receives the shadow of a point p of the sphere when
// h = p - t L with 0 < t <= T_MAX, and t L.z = p.z - h.z <= c.z + r - z_floor.
__device__ __forceinline__ F3 shadow_end(F3 c, float r, F3 L, float z_floor) {
  float s = T_MAX;
  if (L.z > 0.0f) s = fminf(T_MAX, fmaxf((c.z + r - z_floor) / L.z, 0.0f));
  s = s * 1.0001f + 1e-2f;
  return c - s * L;
}

__device__ __forceinline__ float scene_floor(const SceneArgs& A) { return fminf(A.z_bot, key_value(*A.zmin)); }

// The tile-level scan of k_scene and k_mesh: the next chunk of CHUNK envs that has a survivor, its survivors in env
// order into S.surv (a ballot per wave, a prefix over the waves).  Without BRUTE an env survives when its bit is set and
// its capsule meets the tile's frustum Fr; with BRUTE every env does.  False when the scene is exhausted.  Every lane of
// the workgroup calls it, every decision in it is uniform.
struct Scan {
  int32_t surv[CHUNK];   // the scanned chunk's surviving envs, ascending
  int32_t wcount[CHUNK / 64];
};
__device__ __forceinline__ bool scan_on(Scan& S, const SceneArgs& A, const Frustum& Fr, float z_floor, int cam, int tid,
                                        Cursor& c) {
  const int N = A.num_envs;
  while (c.sb >= c.m) {   // the scanned chunk is used up: scan on
    if (c.base >= N) return false;
    const int n = c.base + tid;
    bool vis = n < N;
    if (!(A.flags & T1RENDER_SCENE_BRUTE)) {
      const uint32_t* w = A.bits + (size_t)cam * A.words + (c.base >> 5);
      const int nw = min(CHUNK / 32, A.words - (c.base >> 5));
      uint32_t any = 0;
      for (int k = 0; k < nw; ++k) any |= w[k];
      if (__builtin_amdgcn_readfirstlane(any) == 0) {   // nothing of these 256 envs matters to the camera
        c.base += CHUNK;
        continue;
      }
      vis = vis && ((w[tid >> 5] >> (tid & 31)) & 1u);
      if (vis) {
        const float4 sp = A.sphere[n];
        const F3 ctr = f3(sp.x, sp.y, sp.z);
        const F3 L = f3(A.R.style.light[0], A.R.style.light[1], A.R.style.light[2]);
        vis = !capsule_outside(Fr, ctr, shadow_end(ctr, sp.w, L, z_floor), sp.w);
      }
    }
    const unsigned long long mask = __ballot(vis);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) S.wcount[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < CHUNK / 64; ++k) {
      if (k < wave) off += S.wcount[k];
      total += S.wcount[k];
    }
    if (vis) S.surv[off + __popcll(mask & ((1ull << lane) - 1ull))] = n;
    c.m = total;
    c.sb = 0;
    c.base += CHUNK;
    __syncthreads();
  }
  return true;
}

__global__ __launch_bounds__(CHUNK) void k_scene_bits(const SceneArgs A) {
  __shared__ Frustum fr[T1RENDER_MAXCAM];
  if ((int)threadIdx.x < A.ncams) {
    Frame S;
    camera_frame(S, A.R, threadIdx.x);
    fr[threadIdx.x] = make_frustum(S, -1.0f, 1.0f, -1.0f, 1.0f);
  }
  __syncthreads();
  const int n = blockIdx.x * CHUNK + threadIdx.x;
  const bool live = n < A.num_envs && A.R.nprims > 0;
  const float4 sp = live ? A.sphere[n] : make_float4(0, 0, 0, 0);
  const F3 c = f3(sp.x, sp.y, sp.z);
  const F3 L = f3(A.R.style.light[0], A.R.style.light[1], A.R.style.light[2]);
  const F3 e = shadow_end(c, sp.w, L, scene_floor(A));
  const int word = 2 * (blockIdx.x * (CHUNK / 64) + (threadIdx.x >> 6));
  for (int cam = 0; cam < A.ncams; ++cam) {
    const bool vis = live && !capsule_outside(fr[cam], c, e, sp.w);
    const unsigned long long mask = __ballot(vis);
    if ((threadIdx.x & 63) == 0 && word < A.words) {
      uint32_t* w = A.bits + (size_t)cam * A.words + word;
      w[0] = (uint32_t)mask;
      w[1] = (uint32_t)(mask >> 32);
    }
  }
}

// what a pixel's hit looks like before the shadow decides its light
struct Surface {
  F3 n, col, base, so;   // the normal, the sky's colour, the surface's colour, the shadow ray's origin
  float nl;
  int id;
  bool sky, need;        // need: the surface faces the light, a shadow ray decides
};

// normal, colour and id of primitive P entered through `face` at `hit`
__device__ __forceinline__ void prim_surface(Surface& h, const WorldPrim& P, int face, F3 hit) {
  if (P.kind == 0) {
    const int k = face & 3;
    const float sg = (face & 4) ? 1.0f : -1.0f;
    // P lives in registers: column k by selection, not by address
    const float c0 = k == 0 ? P.R[0] : k == 1 ? P.R[1] : P.R[2], c1 = k == 0 ? P.R[3] : k == 1 ? P.R[4] : P.R[5];
    const float c2 = k == 0 ? P.R[6] : k == 1 ? P.R[7] : P.R[8];
    h.n = f3(sg * c0, sg * c1, sg * c2);
  } else {
    const F3 a = f3(P.A[0], P.A[1], P.A[2]), ba = f3(P.B[0], P.B[1], P.B[2]) - a;
    const float baba = dot(ba, ba);
    const float s = baba > 0.0f ? fminf(fmaxf(dot(hit - a, ba) / baba, 0.0f), 1.0f) : 0.0f;
    h.n = normalize(hit - (a + s * ba));
  }
  h.base = f3((float)(P.rgb & 255u) * (1.0f / 255.0f), (float)((P.rgb >> 8) & 255u) * (1.0f / 255.0f),
              (float)((P.rgb >> 16) & 255u) * (1.0f / 255.0f));
  h.id = 1 + P.body;
}

// The terrain against the robot's nearest hit (hp, -1: none; fetch(h, hit) fills in its normal, colour and id), then
// normal and colour: the steps of shade_pixel (t1render.hip) between its two casts.  best becomes the hit's t (+inf:
// sky), henv -1 unless a robot shows.
template <class Fetch>
__device__ __forceinline__ Surface surface(const RenderArgs& R, F3 o, F3 d, float& best, int hp, int& henv, Fetch fetch) {
  Surface h = {f3(0, 0, 1), f3(0, 0, 0), f3(0, 0, 0), f3(0, 0, 0), 0.0f, -1, false, false};
  const t1render_style& St = R.style;
  bool ground = false;
  if (R.hf) {
    ground = cast_heightfield(R, o, d, T_MIN, best, h.n);
  } else if (d.z != 0.0f) {
    const float t = -o.z / d.z;
    if (t > T_MIN && t <= best) {
      best = t;
      ground = true;
    }
  }
  if (!ground && hp < 0) {
    const float s = 0.5f * (d.z + 1.0f);
    h.col = f3(St.sky_rgb[0][0] + s * (St.sky_rgb[1][0] - St.sky_rgb[0][0]),
               St.sky_rgb[0][1] + s * (St.sky_rgb[1][1] - St.sky_rgb[0][1]),
               St.sky_rgb[0][2] + s * (St.sky_rgb[1][2] - St.sky_rgb[0][2]));
    best = INFINITY;
    henv = -1;
    h.sky = true;
    return h;
  }
  const F3 hit = o + best * d;
  if (ground) {
    const int par = ((int)floorf(hit.x) + (int)floorf(hit.y)) & 1;
    h.base = f3(St.terrain_rgb[par][0], St.terrain_rgb[par][1], St.terrain_rgb[par][2]);
    h.id = 0;
    henv = -1;
  } else {
    fetch(h, hit);
  }
  h.nl = fmaxf(dot(h.n, f3(St.light[0], St.light[1], St.light[2])), 0.0f);
  h.need = h.nl > 0.0f;   // a surface facing away from the light needs no shadow ray
  h.so = hit + SHADOW_EPS * h.n;
  return h;
}

// the height field's shadow where no primitive cast one, the colour, the four planes
__device__ __forceinline__ void store_pixel(const SceneArgs& A, const Surface& h, float lit, float best, int henv, int cam,
                                            int i, int j) {
  const RenderArgs& R = A.R;
  const t1render_style& St = R.style;
  if (h.need && lit != 0.0f && (A.flags & T1RENDER_SCENE_TERRAIN_SHADOW) && R.hf) {
    float sb = T_MAX;
    F3 sn = f3(0, 0, 1);
    if (cast_heightfield(R, h.so, f3(St.light[0], St.light[1], St.light[2]), T_MIN, sb, sn)) lit = 0.0f;
  }
  const F3 col = h.sky ? h.col : (St.ambient + (1.0f - St.ambient) * h.nl * lit) * h.base;
  const size_t px_i = ((size_t)cam * R.height + i) * R.width + j;
  R.rgba[px_i] = pack_rgb(col);
  if (R.depth) R.depth[px_i] = best;
  if (R.ids) R.ids[px_i] = h.id;
  if (A.envs) A.envs[px_i] = henv;
}

__device__ __forceinline__ F3 pixel_ray(const Frame& C, const RenderArgs& R, int i, int j) {   // as shade_pixel has it
  const float px = 2.0f * ((float)j + 0.5f) / (float)R.width - 1.0f;
  const float py = 1.0f - 2.0f * ((float)i + 0.5f) / (float)R.height;
  return normalize(f3(C.f[0] + px * C.r[0] + py * C.u[0], C.f[1] + px * C.r[1] + py * C.u[1],
                      C.f[2] + px * C.r[2] + py * C.u[2]));
}

inline long long scene_workspace_bytes(long long num_envs, long long ncams, long long* words) {
  const long long w = 2 * ((num_envs + 63) / 64);
  if (words) *words = w;
  return (16 * num_envs + 4 * ncams * w + 4 + 15) / 16 * 16;
}

}  // namespace
#endif
