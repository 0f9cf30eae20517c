// t1render_depth.hip -- the depth camera sensor (include/t1render.h, t1render_depth): one launch ray-casts a small depth
// image for every env of the handle, from a pinhole camera fixed to a body of the env's own robot.
//
// One lane per pixel.  The unit of work is a wave: a compact 16 x 4 pixel block of one env, so that its lanes walk the
// same cells of the height field.  An image is tiles_x x tiles_y such blocks, the blocks of all envs are numbered env
// major, and a 256-lane workgroup takes four consecutive ones: at 64 x 48 four neighbouring blocks of one env, at 16 x 12
// (three blocks per image) the blocks of up to two envs, at 16 x 4 and below one env per wave.  No lane idles for an
// image that is a multiple of the block, whatever the env count.  The first wave of a workgroup that draws an env poses
// that env's primitives and camera frame into its own LDS slot (at most four envs per workgroup), so an env is posed
// once per workgroup and every later read is an LDS broadcast.  Sensor and primitives travel as kernel arguments: the call
// allocates and copies nothing.  The intersections and the height field's walk are t1render_dev.h's, the text the film
// camera uses; the ray's range is the sensor's [near, far] in planar depth instead of the film camera's (T_MIN, T_MAX],
// which also bounds the walk to the few cells within far.
#include <hip/hip_fp16.h>

#include "t1render_dev.h"

using namespace t1;

namespace {

constexpr int WAVES = 4, BLOCK_W = 16, BLOCK_H = 4;   // waves per workgroup; a wave's pixel block

struct DepthArgs {
  const float* rigid_state;
  const int16_t* h;   // the height field, as cast_heightfield reads it
  int32_t rows, cols, hf;
  float inv_hscale, vscale, border, z_top;
  const float* mounts;   // (num_envs, 7) or null
  int32_t body;
  float pos[3], quat[4];   // the sensor's mount, quat normalised by the call
  float th, ta;            // tan(vfov/2), and times width / height
  float near, far;
  int32_t width, height, nprims, f16;
  int32_t tiles_x, units;   // pixel blocks per image row; per image
  long long total;          // num_envs * units
  void* depth;
  int8_t* ids;
  t1render_prim prims[T1RENDER_MAXPRIM];
};

struct Sensor {   // one env's scene (LDS)
  WorldPrim prim[T1RENDER_MAXPRIM];
  float eye[3], f[3], r[3], u[3];   // r and u already scaled by tan(vfov/2) (r by the aspect too)
};

__device__ __forceinline__ void quat_rows(const float* q, float R[9]) {   // (x, y, z, w), the header's formula
  const float x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}

// lane's share of posing env's scene: primitive `lane` (as pose_scene of t1render.hip), or (lane T1RENDER_MAXPRIM) the
// mounted camera's frame
__device__ __forceinline__ void pose_sensor(Sensor& S, const DepthArgs& A, int env, int lane) {
  const float* rs = A.rigid_state + (size_t)env * 169;
  if (lane < A.nprims) {
    const t1render_prim& p = A.prims[lane];
    const float* b = rs + p.body * 13;
    float R[9];
    quat_rows(b + 3, R);
    WorldPrim& P = S.prim[lane];
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
  } else if (lane == T1RENDER_MAXPRIM) {
    const float* b = rs + A.body * 13;
    float mp[3] = {A.pos[0], A.pos[1], A.pos[2]}, mq[4] = {A.quat[0], A.quat[1], A.quat[2], A.quat[3]};
    if (A.mounts) {   // this env's own mount
      const float* m = A.mounts + (size_t)env * 7;
#pragma unroll
      for (int k = 0; k < 3; ++k) mp[k] = m[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) mq[k] = m[3 + k];
    }
    float Rb[9], Rm[9];
    quat_rows(b + 3, Rb);
    quat_rows(mq, Rm);
    const float th = A.th, ta = A.ta;
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // row k of R_b R_m: its columns are the camera's forward, left and up axes
      const float fk = Rb[3 * k] * Rm[0] + Rb[3 * k + 1] * Rm[3] + Rb[3 * k + 2] * Rm[6];
      const float lk = Rb[3 * k] * Rm[1] + Rb[3 * k + 1] * Rm[4] + Rb[3 * k + 2] * Rm[7];
      const float uk = Rb[3 * k] * Rm[2] + Rb[3 * k + 1] * Rm[5] + Rb[3 * k + 2] * Rm[8];
      S.eye[k] = b[k] + Rb[3 * k] * mp[0] + Rb[3 * k + 1] * mp[1] + Rb[3 * k + 2] * mp[2];
      S.f[k] = fk;
      S.r[k] = ta * -lk;
      S.u[k] = th * uk;
    }
  }
}

// pixel (row i, column j): the planar depth of the nearest hit with near <= z <= far (far without one) and its id
__device__ __forceinline__ float cast_pixel(const Sensor& S, const DepthArgs& A, int i, int j, int& id) {
  const float px = 2.0f * ((float)j + 0.5f) / (float)A.width - 1.0f;
  const float py = 1.0f - 2.0f * ((float)i + 0.5f) / (float)A.height;
  const F3 o = f3(S.eye[0], S.eye[1], S.eye[2]), f = f3(S.f[0], S.f[1], S.f[2]);
  const F3 d = normalize(f3(f.x + px * S.r[0] + py * S.u[0], f.y + px * S.r[1] + py * S.u[1],
                            f.z + px * S.r[2] + py * S.u[2]));
  const float c = dot(d, f);   // > 0: d is f plus a part orthogonal to it, scaled
  const float tlo = A.near / c;
  float best = A.far / c;
  int hp = -1;
  for (int p = 0; p < A.nprims; ++p) {
    const WorldPrim& P = S.prim[p];
    int fc = 0;
    const float t = P.kind == 0 ? box_entry(P, o, d, fc) : capsule_entry(P, o, d);
    if (t >= tlo && t <= best) {
      best = t;
      hp = p;
    }
  }
  bool ground = false;
  if (A.hf) {
    F3 n = f3(0, 0, 1);
    ground = cast_heightfield(A, o, d, tlo, best, n);
  } else if (d.z != 0.0f) {
    const float t = -o.z / d.z;
    if (t >= tlo && t <= best) {
      best = t;
      ground = true;
    }
  }
  if (!ground && hp < 0) {
    id = -1;
    return A.far;
  }
  id = ground ? 0 : 1 + S.prim[hp].body;
  return fminf(fmaxf(best * c, A.near), A.far);   // t was in range; the product may round a last bit outside
}

__global__ __launch_bounds__(WAVES * 64) void k_depth(const DepthArgs A) {
  __shared__ Sensor S[WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long g0 = (long long)blockIdx.x * WAVES, g = g0 + wave;   // the workgroup's first block, this wave's
  const bool live = g < A.total;                                      // the last workgroup may have idle waves
  const int env0 = (int)(g0 / A.units);
  int env = 0, unit = 0, slot = 0;
  if (live) {
    env = (int)(g / A.units);
    unit = (int)(g - (long long)env * A.units);
    slot = env - env0;   // < WAVES: every env has at least one block
    // the workgroup's first wave of this env poses it: wave 0, or the wave that starts a new env
    if (wave == 0 || unit == 0) pose_sensor(S[slot], A, env, lane);
  }
  __syncthreads();
  if (!live) return;
  const int j = (unit % A.tiles_x) * BLOCK_W + (lane & (BLOCK_W - 1));
  const int i = (unit / A.tiles_x) * BLOCK_H + (lane >> 4);
  const bool in = j < A.width && i < A.height;   // edge blocks: no store outside the image
  float z = 0.0f;
  int id = -1;
  if (in) z = cast_pixel(S[slot], A, i, j, id);
  const size_t px_i = ((size_t)env * A.height + i) * A.width + j;
  if (A.f16) {
    // two neighbouring pixels of a row as one 4-byte store where the pair starts on a 4-byte boundary; a row's first or
    // last pixel (odd widths shift the rows' parity) and a block's last column go out alone
    __half* out = (__half*)A.depth;
    const uint32_t mine = __half_as_ushort(__float2half_rn(z));
    const uint32_t next = __shfl_down(mine, 1);
    const int x = lane & (BLOCK_W - 1);
    const bool even = ((((uintptr_t)out >> 1) + px_i) & 1) == 0;
    const bool lead = in && even && x < BLOCK_W - 1 && j + 1 < A.width;
    const bool follow = in && !even && x > 0;   // the pixel to its left is in the image, even, and leads
    if (lead) *(uint32_t*)(out + px_i) = mine | (next << 16);
    else if (in && !follow) out[px_i] = __ushort_as_half((unsigned short)mine);
  } else if (in) {
    ((float*)A.depth)[px_i] = z;
  }
  if (A.ids && in) A.ids[px_i] = (int8_t)id;
}

}  // namespace

extern "C" int t1render_depth(t1env* env, const t1render_sensor* sensor, const float* mounts,
                              const t1render_prim* prims, int32_t nprims, int32_t width, int32_t height, int32_t flags,
                              void* depth, int8_t* ids, void* stream) {
  if (!env || !sensor || !depth) return t1_fail(T1ENV_E_ARG, "t1render_depth: null argument");
  if (nprims < 0 || nprims > T1RENDER_MAXPRIM) return t1_fail(T1ENV_E_ARG, "t1render_depth: nprims outside [0, 32]");
  if (nprims > 0 && !prims) return t1_fail(T1ENV_E_ARG, "t1render_depth: null prims with nprims > 0");
  if (width < 1 || height < 1) return t1_fail(T1ENV_E_ARG, "t1render_depth: width and height must be >= 1");
  if (flags & ~T1RENDER_DEPTH_F16) return t1_fail(T1ENV_E_ARG, "t1render_depth: unknown flag bit");
  const t1render_sensor& C = *sensor;
  if (C.body < 0 || C.body >= T1_NB) return t1_fail(T1ENV_E_ARG, "t1render_depth: the sensor's body is out of range");
  if (!((double)C.vfov > 0.0 && (double)C.vfov < 3.14159265358979323846))
    return t1_fail(T1ENV_E_ARG, "t1render_depth: vfov outside (0, pi)");
  if (!(C.near > 0.0f && C.near < C.far && C.far <= 200.0f))
    return t1_fail(T1ENV_E_ARG, "t1render_depth: need 0 < near < far <= 200");
  double qq = 0.0;
  for (int k = 0; k < 4; ++k) {
    if (!isfinite(C.quat[k])) return t1_fail(T1ENV_E_ARG, "t1render_depth: the mount's quat is not finite");
    qq += (double)C.quat[k] * C.quat[k];
  }
  if (!(qq > 0.0)) return t1_fail(T1ENV_E_ARG, "t1render_depth: the mount's quat is zero");
  for (int k = 0; k < 3; ++k)
    if (!isfinite(C.pos[k])) return t1_fail(T1ENV_E_ARG, "t1render_depth: the mount's pos is not finite");
  DepthArgs A = {};
  for (int p = 0; p < nprims; ++p) {
    if (prims[p].body < 0 || prims[p].body >= T1_NB) return t1_fail(T1ENV_E_ARG, "t1render_depth: a primitive's body is out of range");
    if (prims[p].kind != 0 && prims[p].kind != 1) return t1_fail(T1ENV_E_ARG, "t1render_depth: a primitive's kind is not 0 or 1");
    A.prims[p] = prims[p];
  }
  RenderView v;
  t1_render_view(env, &v);
  if ((long long)width * height * v.num_envs >= (1LL << 31))
    return t1_fail(T1ENV_E_ARG, "t1render_depth: width * height * num_envs must be below 2^31");
  if (v.terrain.type != 0 && !v.terrain.h) return t1_fail(T1ENV_E_STATE, "t1render_depth: no terrain set");
  if (v.num_envs < 1) return 0;
  A.rigid_state = v.rigid_state;
  A.h = v.terrain.h;
  A.rows = v.terrain.rows;
  A.cols = v.terrain.cols;
  A.hf = v.terrain.type != 0;
  A.inv_hscale = v.terrain.inv_hscale;
  A.vscale = v.terrain.vscale;
  A.border = v.terrain.border;
  A.z_top = v.z_top + 1e-3f * (1.0f + fabsf(v.z_top));
  A.mounts = mounts;
  A.body = C.body;
  const double qn = sqrt(qq);
  for (int k = 0; k < 3; ++k) A.pos[k] = C.pos[k];
  for (int k = 0; k < 4; ++k) A.quat[k] = (float)(C.quat[k] / qn);
  A.th = tanf(0.5f * C.vfov);
  A.ta = A.th * (float)width / (float)height;
  A.near = C.near;
  A.far = C.far;
  A.width = width;
  A.height = height;
  A.nprims = nprims;
  A.f16 = (flags & T1RENDER_DEPTH_F16) != 0;
  A.tiles_x = (width + BLOCK_W - 1) / BLOCK_W;
  A.units = A.tiles_x * ((height + BLOCK_H - 1) / BLOCK_H);   // <= width * height: the total is below 2^31 too
  A.total = (long long)A.units * v.num_envs;
  A.depth = depth;
  A.ids = ids;
  const dim3 grid((unsigned)((A.total + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(k_depth, grid, dim3(WAVES * 64), 0, (hipStream_t)stream, A);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
  return 0;
}
