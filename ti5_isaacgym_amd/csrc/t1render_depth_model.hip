// t1render_depth_model.hip -- the depth camera's sensor model (include/t1render.h, t1render_depth_model): one launch
// turns the clean image of every env into a measured one (depth-squared noise, dropouts, occlusion shadows) and serves
// it through a ring of the last K frames with a per-env delay.
//
// One lane per pixel over the flat index q = (env, row, column), so a wave reads and writes 64 consecutive elements
// whatever the image's size: rows and even envs may straddle a wave or a workgroup, and an image smaller than a wave
// shares its wave with its neighbours.  The traffic is one read of clean, one write to the ring and one to out per pixel
// and one more read for a delayed env (what the launch costs is measured in DESIGN.md 9.1); the four neighbours of the edge test are re-reads of lines the same
// or a neighbouring wave has just fetched and come from cache.  No LDS, no scratch.  The draws are the env step's counter
// hash: the key of (seed, env, frame), one mix per draw, and a draw is skipped where its parameter is zero for the whole
// launch (the result is the same: see measure()).
//
// Every float operation of the model is rounded on its own (contraction is off for this unit), so the measured value is
// the same to the bit as a float32 evaluation of the header's words.
//
// A lane never reads ring memory that this launch writes: an env with d == 0, or a fresh one, is served the value the lane
// has in its register, and a delayed one the slot (frame - d) mod K != frame mod K, which only earlier launches wrote.
#include <hip/hip_fp16.h>

#include "t1render_dev.h"

#pragma clang fp contract(off)

using namespace t1;

namespace {

constexpr int THREADS = 256;

struct ModelArgs {
  t1render_depth_noise m;
  const void* clean;
  void* ring;
  void* out;
  const int32_t* lag;
  const uint8_t* fresh;
  uint32_t frame;
  int32_t K, cur;          // ring frames; the slot this frame goes to, frame mod K
  uint32_t width, height, hw, total;   // hw = width * height, total = hw * num_envs < 2^31
};

template <bool F16>
__device__ __forceinline__ float load_px(const void* p, size_t i) {
  if constexpr (F16) return __half2float(((const __half*)p)[i]);
  else return ((const float*)p)[i];
}

// the header's steps 1 to 4 for pixel pix of env e (flat index q), z its clean value; true: no measurement (fill).
// The integer multiplies of the hash are what the launch costs, so none is made that cannot matter: a pixel with
// nothing in range draws nothing (a wave of sky returns at once), the key's three mixes run on the scalar unit for the
// env of the wave's first lane and again per lane only in a wave that straddles envs, the slot's multiply is shared by
// the four draws (slot k is 4 pix + k, and the product distributes), and u_1 is drawn only at an edge.
template <bool F16>
__device__ __forceinline__ bool measure(const ModelArgs& A, uint32_t e, uint32_t pix, uint32_t q, float z, float& v) {
  const t1render_depth_noise& M = A.m;
  v = z;
  if (z >= M.far) return true;
  const uint32_t e0 = __builtin_amdgcn_readfirstlane(e);
  RngKey key = rng_key(M.seed, (uint32_t)M.env_base + e0, A.frame);
  if (e != e0) key = rng_key(M.seed, (uint32_t)M.env_base + e, A.frame);
  constexpr uint32_t C = 0x85EBCA77u;          // hash_k(key, slot) = mix32(key.h ^ (slot * C))
  const uint32_t s0 = (4u * pix) * C;
  // p_drop == 0: u_0 < 0 never holds, the draw is not made
  if (M.p_drop != 0.0f && (float)(mix32(key.h ^ s0) >> 8) * (1.0f / 16777216.0f) < M.p_drop) return true;
  if (M.p_edge != 0.0f) {
    const uint32_t i = pix / A.width, j = pix - i * A.width;
    float mn = INFINITY;
    if (i > 0) mn = fminf(mn, load_px<F16>(A.clean, (size_t)q - A.width));
    if (i + 1 < A.height) mn = fminf(mn, load_px<F16>(A.clean, (size_t)q + A.width));
    if (j > 0) mn = fminf(mn, load_px<F16>(A.clean, (size_t)q - 1));
    if (j + 1 < A.width) mn = fminf(mn, load_px<F16>(A.clean, (size_t)q + 1));
    const float jump = z - mn, bound = M.edge_abs + M.edge_rel * mn;
    if (jump > bound) {
      if ((float)(mix32(key.h ^ (s0 + C)) >> 8) * (1.0f / 16777216.0f) < M.p_edge) return true;
    }
  }
  // both sigmas zero: z + (0 + (0 z) z) g is z, the two draws are not made
  if (M.sigma0 != 0.0f || M.sigma2 != 0.0f) {
    const uint32_t h2 = mix32(key.h ^ (s0 + 2u * C)), h3 = mix32(key.h ^ (s0 + 3u * C));
    const int32_t s = (int32_t)((h2 & 0xFFFFu) + (h2 >> 16) + (h3 & 0xFFFFu) + (h3 >> 16)) - 131070;
    const float g = (float)s * (1.7320508075688772f / 65536.0f);
    v = z + (M.sigma0 + (M.sigma2 * z) * z) * g;
  }
  v = fminf(fmaxf(v, M.near), M.far);
  return false;
}

// fp16: element idx of base gets `mine`; two neighbouring pixels of one env go out as one 4-byte store where the pair
// starts on a 4-byte boundary (k_depth's pair store over the flat index): the even one leads with its right neighbour's
// bits, the odd one then stores nothing.  An env's first and last pixel and a wave's first and last lane may go out
// alone.  ok must be the same for the two lanes of a pair: it depends on the env alone.
__device__ __forceinline__ void store_half(__half* base, size_t idx, uint32_t mine, uint32_t next, bool ok, int lane,
                                           uint32_t pix, uint32_t hw) {
  const bool even = ((((uintptr_t)base >> 1) + idx) & 1) == 0;
  const bool lead = ok && even && lane < 63 && pix + 1 < hw;
  const bool follow = ok && !even && lane > 0 && pix > 0;   // the pixel to its left is of this env, even, and leads
  if (lead) *(uint32_t*)(base + idx) = mine | (next << 16);
  else if (ok && !follow) base[idx] = __ushort_as_half((unsigned short)mine);
}

template <bool F16>
__global__ __launch_bounds__(THREADS) void k_depth_model(const ModelArgs A) {
  const uint32_t p = blockIdx.x * THREADS + threadIdx.x;
  const bool live = p < A.total;
  const uint32_t q = live ? p : A.total - 1;   // the last workgroup's idle lanes recompute the last pixel and store nothing
  const uint32_t e = q / A.hw, pix = q - e * A.hw;
  const float z = load_px<F16>(A.clean, q);
  float v;
  const bool none = measure<F16>(A, e, pix, q, z, v);
  if (none) v = A.m.fill;
  const bool fr = A.fresh && A.fresh[e] != 0;
  int d = A.lag ? A.lag[e] : 0;
  d = min(max(d, 0), A.K - 1);
  const bool delayed = d > 0 && !fr;
  const size_t back = (size_t)((A.cur + A.K - d) % A.K) * A.total + q;   // != cur's slot when delayed
  if constexpr (F16) {
    const int lane = threadIdx.x & 63;
    __half* ring = (__half*)A.ring;
    const uint32_t mine = __half_as_ushort(__float2half_rn(v));
    const uint32_t served = delayed ? (uint32_t)__half_as_ushort(ring[back]) : mine;
    const uint32_t next = __shfl_down(mine, 1), next_served = __shfl_down(served, 1);
    if (ring) {
      if (fr) {
        for (int s = 0; s < A.K; ++s) store_half(ring, (size_t)s * A.total + q, mine, next, live, lane, pix, A.hw);
      } else {
        store_half(ring, (size_t)A.cur * A.total + q, mine, next, live, lane, pix, A.hw);
      }
    }
    store_half((__half*)A.out, q, served, next_served, live, lane, pix, A.hw);
  } else {
    if (!live) return;
    float* ring = (float*)A.ring;
    const float served = delayed ? ring[back] : v;
    if (ring) {
      if (fr) {
        for (int s = 0; s < A.K; ++s) ring[(size_t)s * A.total + q] = v;
      } else {
        ring[(size_t)A.cur * A.total + q] = v;
      }
    }
    ((float*)A.out)[q] = served;
  }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int t1render_depth_model(const t1render_depth_noise* m, const void* clean, int32_t num_envs, int32_t width,
                                    int32_t height, int32_t flags, uint32_t frame, void* ring, int32_t ring_frames,
                                    const int32_t* lag, const uint8_t* fresh, void* out, void* stream) {
  if (!m || !clean || !out) return t1_fail(T1ENV_E_ARG, "t1render_depth_model: null argument");
  if (ring_frames < 1 || ring_frames > T1RENDER_DEPTH_MAXRING)
    return t1_fail(T1ENV_E_ARG, "t1render_depth_model: ring_frames outside [1, 16]");
  if (!ring && ring_frames > 1) return t1_fail(T1ENV_E_ARG, "t1render_depth_model: null ring with ring_frames > 1");
  if (num_envs < 1 || width < 1 || height < 1)
    return t1_fail(T1ENV_E_ARG, "t1render_depth_model: num_envs, width and height must be >= 1");
  if ((long long)width * height * num_envs >= (1LL << 31))
    return t1_fail(T1ENV_E_ARG, "t1render_depth_model: width * height * num_envs must be below 2^31");
  if (flags & ~T1RENDER_DEPTH_F16) return t1_fail(T1ENV_E_ARG, "t1render_depth_model: unknown flag bit");
  const t1render_depth_noise& M = *m;
  if (!(M.near > 0.0f && M.near < M.far && M.far <= 200.0f))
    return t1_fail(T1ENV_E_ARG, "t1render_depth_model: need 0 < near < far <= 200");
  if (!(M.p_drop >= 0.0f && M.p_drop <= 1.0f) || !(M.p_edge >= 0.0f && M.p_edge <= 1.0f))
    return t1_fail(T1ENV_E_ARG, "t1render_depth_model: a probability outside [0, 1]");
  for (float x : {M.sigma0, M.sigma2, M.edge_abs, M.edge_rel})
    if (!(x >= 0.0f) || !isfinite(x))
      return t1_fail(T1ENV_E_ARG, "t1render_depth_model: a negative or non-finite sigma or edge threshold");
  if (!isfinite(M.fill)) return t1_fail(T1ENV_E_ARG, "t1render_depth_model: fill is not finite");
  const bool f16 = (flags & T1RENDER_DEPTH_F16) != 0;
  const size_t esz = f16 ? 2 : 4;
  const size_t total = (size_t)width * height * num_envs, bytes = total * esz;
  if (((uintptr_t)clean | (uintptr_t)out | (uintptr_t)ring) & (esz - 1))
    return t1_fail(T1ENV_E_ARG, "t1render_depth_model: clean, ring or out is not aligned to its element");
  if (overlap(out, bytes, clean, bytes)) return t1_fail(T1ENV_E_ARG, "t1render_depth_model: out overlaps clean");
  if (ring && (overlap(ring, bytes * ring_frames, clean, bytes) || overlap(ring, bytes * ring_frames, out, bytes)))
    return t1_fail(T1ENV_E_ARG, "t1render_depth_model: ring overlaps clean or out");
  ModelArgs A = {};
  A.m = M;
  A.clean = clean;
  A.ring = ring;
  A.out = out;
  A.lag = lag;
  A.fresh = fresh;
  A.frame = frame;
  A.K = ring_frames;
  A.cur = (int32_t)(frame % (uint32_t)ring_frames);
  A.width = (uint32_t)width;
  A.height = (uint32_t)height;
  A.hw = (uint32_t)(width * height);
  A.total = (uint32_t)total;
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS));
  if (f16) hipLaunchKernelGGL(k_depth_model<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(k_depth_model<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, A);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
  return 0;
}
