// The DH policy's rollout forward after the first history conv, fused into one kernel (include/t1policy.h,
// t1policy_heads_*): every dense layer of actor_critic_dh.py:8-188 the rollout's act() runs --
//
//   long history tail  conv2 (32 -> 16, k4 s2) + ReLU, flatten (16 x 6), 96 -> 128 ELU -> 64      (actor_critic_dh.py:83-96)
//   state estimator    short history (235) -> 256 ELU -> 128 ELU -> 64 ELU -> 3                  (:98-111)
//   actor              [short | estimate | code] (302) -> 512 ELU -> 256 ELU -> 128 ELU -> 12    (:45-58, :163-170)
//   critic             privileged (219) -> 768 ELU -> 256 ELU -> 128 ELU -> 1                   (:60-73, :185-188)
//
// plus the Normal sample, its log-prob and the broadcast sigma (DHPPO._act_body), from the first conv's output
// (t1policy_conv1d_forward_packed), the actor and critic observations and a standard-normal draw.  The same kernel
// runs the deterministic policy (act_inference: the actor chain alone, the mean and the estimated velocity) and the
// critic's value (evaluate) as one-role launches (t1policy_actor_forward / t1policy_critic_forward, k_heads64's ROLE).
//
// One kernel, k_heads64<TO, ET, ROLE>.  A workgroup owns ET 32-env column tiles -- 64 envs (ET 2: act(), and the larger
// one-role launches; the two tiles share every weight fragment, below) or 32 (ET 1: the smaller one-role launches) --
// and one role (actor chain or critic), eight waves (two per SIMD) splitting each layer's 32-output tiles.  Every layer
// is a chain of v_mfma_f32_32x32x16_f16 with the WEIGHTS as the A operand (32 output features x 16 inputs) and the ACTIVATIONS as
// the B operand (16 inputs x 32 envs), so a layer's 32 x 32 result has the env on the lane and the features in the
// 16 accumulator registers -- exactly the B fragments of the next layer's two k-steps (permuted k order, cdna guide
// "An accumulator tile as the next MFMA's operand"): an output tile goes to LDS as two 1-KB fragments per precision
// half with one ds_write_b128 each, and the next layer reads them back with one ds_read_b128 each, no transposes.
// The weight fragments are packed once per act() (k_heads_pack) in that permuted k order.
//
// fp32 accuracy from the fp16 matrix cores, as the first conv (t1policy.hip): v = hi + lo / 2^11 with hi = fp16(v),
// lo = fp16((v - hi) 2^11), y = sum hi.hi + 2^-11 sum (hi.lo + lo.hi) in two fp32 accumulators; the dropped lo.lo
// and the residual rounding are ~2^-22 of each product.
//
// Bounds: per 32-env tile the actor chain is 976 step-tiles and the critic 792 (one step-tile = a
// 32 x 16 weight fragment pair = 3 MFMAs, 2 KB of fragments): 3.6 MB of fragments streamed from L2 per tile pair and
// 1.4 M MFMA-cycles per tile pair -- at the XCD L2's ~70 GB/s/CU of shared rows the fragment stream, not the matrix
// cores, sets the time.  Every XCD (blockIdx mod 8) runs both roles, alternating in its dispatch order, so the longer
// actor chain is spread over all CUs; its 4 MB L2 holds both roles' 3.6 MB of fragments.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));

constexpr float PH_SPLIT = 2048.0f;
// waves per workgroup, two per SIMD: act() 0.177 -> 0.147 ms at 8192 envs against one per SIMD (profiles/r05h8_*)
constexpr int PH_WAVES = 8;
// ring depth in k-steps: act() 0.1419 ms at 4, 0.1428 at 6, 0.1443 at 8, 0.1470 at 12 (profiles/r05hd_act_ab.txt)
constexpr int PH_RING_DEPTH = 4;
constexpr int PH_OBS_SHORT = 235, PH_CRITIC = 219, PH_Y1 = 14 * 32;
constexpr int PH_NLAYER = 15;
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_ELU = 2 };

// An input segment of a layer's k axis: `steps` k-steps starting at step `s0` map to input columns col0 .. col0 +
// len - 1, in natural order (staged from global memory: element j of lane half h of step s = column 16 (s - s0) +
// 8 h + j) or in the permuted order of an accumulator tile (column 16 (s - s0) + 8 (j >> 2) + 4 h + (j & 3)).
struct Seg {
  int s0, steps, col0, len, perm;
};
struct Layer {
  int n, k, ks, act;  // outputs, inputs (the weight's row length), k-steps, activation
  Seg seg[3];
  int nseg;
};
// layer order = parameter order of t1policy_heads_* (include/t1policy.h)
constexpr Layer PH_L[PH_NLAYER] = {
    // long-history tail: conv2 as a 448 -> 96 Toeplitz layer over the channels-last conv1 output (flatten order
    // o * 6 + l of nn.Flatten on (16, 6)), then the two Linears
    {96, 128, 28, ACT_RELU, {{0, 28, 0, PH_Y1, 0}}, 1},
    {128, 96, 6, ACT_ELU, {{0, 6, 0, 96, 1}}, 1},
    {64, 128, 8, ACT_NONE, {{0, 8, 0, 128, 1}}, 1},
    // state estimator
    {256, PH_OBS_SHORT, 15, ACT_ELU, {{0, 15, 0, PH_OBS_SHORT, 0}}, 1},
    {128, 256, 16, ACT_ELU, {{0, 16, 0, 256, 1}}, 1},
    {64, 128, 8, ACT_ELU, {{0, 8, 0, 128, 1}}, 1},
    {3, 64, 4, ACT_NONE, {{0, 4, 0, 64, 1}}, 1},
    // actor: [short (natural) | estimate (permuted, rows 0..2 of one half-tile) | code (permuted)]
    {512, 302, 20, ACT_ELU, {{0, 15, 0, PH_OBS_SHORT, 0}, {15, 1, 235, 3, 1}, {16, 4, 238, 64, 1}}, 3},
    {256, 512, 32, ACT_ELU, {{0, 32, 0, 512, 1}}, 1},
    {128, 256, 16, ACT_ELU, {{0, 16, 0, 256, 1}}, 1},
    {12, 128, 8, ACT_NONE, {{0, 8, 0, 128, 1}}, 1},
    // critic
    {768, PH_CRITIC, 14, ACT_ELU, {{0, 14, 0, PH_CRITIC, 0}}, 1},
    {256, 768, 48, ACT_ELU, {{0, 48, 0, 768, 1}}, 1},
    {128, 256, 16, ACT_ELU, {{0, 16, 0, 256, 1}}, 1},
    {1, 128, 8, ACT_NONE, {{0, 8, 0, 128, 1}}, 1},
};
constexpr int ph_nt(int l) { return (PH_L[l].n + 31) / 32; }
constexpr int ph_off(int l) {  // first step-tile of layer l in the fragment buffer
  int o = 0;
  for (int i = 0; i < l; ++i) o += ph_nt(i) * PH_L[i].ks;
  return o;
}
constexpr int PH_UNITS = ph_off(PH_NLAYER);          // 1,768 step-tiles
constexpr int ph_toff(int l) {  // first output tile of layer l (bias fragments)
  int o = 0;
  for (int i = 0; i < l; ++i) o += ph_nt(i);
  return o;
}
constexpr int PH_TILES = ph_toff(PH_NLAYER);          // 90 output tiles
// the weight fragments (hi + lo, 64 lanes x 16 B per step-tile), then each output tile's bias in the C/D layout
// (4 x float4 per lane: [tile][quad][lane], register r of lane l = bias of row (r & 3) + 8 (r >> 2) + 4 (l >> 5))
constexpr int PH_WFRAG_BYTES = PH_UNITS * 2 * 64 * 16;  // 3,620,864
constexpr int PH_FRAG_BYTES = PH_WFRAG_BYTES + PH_TILES * 4 * 64 * 16;  // + 368,640

struct PhParams {
  const float* w[PH_NLAYER];
  const float* b[PH_NLAYER];
  const float* std;
};

// the weight element feeding output o from input column col of layer L (conv2 as its Toeplitz matrix)
template <int L>
__device__ __forceinline__ float ph_weight(const PhParams& P, int o, int col) {
  if constexpr (L == 0) {
    const int oc = o / 6, lp = o % 6, p = col >> 5, c = col & 31, t = p - 2 * lp;
    return (t >= 0 && t < 4) ? P.w[0][(oc * 32 + c) * 4 + t] : 0.0f;
  } else {
    return P.w[L][o * PH_L[L].k + col];
  }
}

template <int L>
__device__ __forceinline__ int ph_col(int s, int h, int j) {
  constexpr Layer Y = PH_L[L];
#pragma unroll
  for (int g = 0; g < Y.nseg; ++g) {
    const Seg q = Y.seg[g];
    if (s >= q.s0 && s < q.s0 + q.steps) {
      const int r = 16 * (s - q.s0) + (q.perm ? 8 * (j >> 2) + 4 * h + (j & 3) : 8 * h + j);
      return r < q.len ? q.col0 + r : -1;
    }
  }
  return -1;
}

__device__ __forceinline__ void split8(const float (&v)[8], h8& hi, h8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const _Float16 x = (_Float16)v[j];
    hi[j] = x;
    lo[j] = (_Float16)((v[j] - (float)x) * PH_SPLIT);
  }
}

template <int L>
__device__ __forceinline__ void ph_pack_unit(const PhParams& P, h8* __restrict__ frag, int u, int lane) {
  constexpr Layer Y = PH_L[L];
  const int nt = u / Y.ks, s = u % Y.ks;
  const int o = 32 * nt + (lane & 31), h = lane >> 5;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = ph_col<L>(s, h, j);
    v[j] = (o < Y.n && col >= 0) ? ph_weight<L>(P, o, col) : 0.0f;
  }
  h8 hi, lo;
  split8(v, hi, lo);
  const int unit = ph_off(L) + u;
  frag[(unit * 2 + 0) * 64 + lane] = hi;
  frag[(unit * 2 + 1) * 64 + lane] = lo;
}

template <int L>
__device__ __forceinline__ bool ph_pack_dispatch(const PhParams& P, h8* frag, int unit, int lane) {
  if constexpr (L == PH_NLAYER) {
    return false;
  } else {
    if (unit < ph_off(L + 1)) {
      ph_pack_unit<L>(P, frag, unit - ph_off(L), lane);
      return true;
    }
    return ph_pack_dispatch<L + 1>(P, frag, unit, lane);
  }
}

template <int L>
__device__ __forceinline__ bool ph_pack_bias(const PhParams& P, float4* __restrict__ bf, int tile, int lane) {
  if constexpr (L == PH_NLAYER) {
    return false;
  } else {
    if (tile < ph_toff(L + 1)) {
      const int nt = tile - ph_toff(L), h = lane >> 5;
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * nt + (r & 3) + 8 * (r >> 2) + 4 * h;
        // conv2 (L = 0): one bias per output channel, row = channel * 6 + position (the flatten order)
        v[r] = row < PH_L[L].n ? P.b[L][L == 0 ? row / 6 : row] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) bf[(tile * 4 + q) * 64 + lane] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
      return true;
    }
    return ph_pack_bias<L + 1>(P, bf, tile, lane);
  }
}

__global__ __launch_bounds__(256) void k_heads_pack(PhParams P, h8* __restrict__ frag) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < (PH_UNITS + PH_TILES) * 64; e += gridDim.x * blockDim.x) {
    if (e < PH_UNITS * 64)
      ph_pack_dispatch<0>(P, frag, e >> 6, e & 63);
    else
      ph_pack_bias<0>(P, reinterpret_cast<float4*>(reinterpret_cast<char*>(frag) + PH_WFRAG_BYTES),
                      (e >> 6) - PH_UNITS, e & 63);
  }
}

// ---- the forward kernel
// expm1(v) for ELU's negative branch, branch-free: the device library's expm1f algorithm (range reduction by
// n = rint(v log2 e) with ln 2 in two parts, the same degree-7 polynomial, 2^n expm1(r) + (2^n - 1)) without its
// overflow and v < -17 fix-ups, which v <= 0 never needs once v is clamped at -88: bit-identical to expm1f there (NaN
// included).  act() 0.1336 -> 0.1279 ms at 8192 envs against expm1f under a branch; a hardware-exp2 form that is not
// bit-identical measured the same, 0.1277 (profiles/r07b_act_ab.txt)
__device__ __forceinline__ float ph_expm1_neg(float v) {
  v = v < -88.0f ? -88.0f : v;  // (not fmaxf: a NaN stays a NaN, as in expm1f and torch's ELU)
  const float n = __builtin_rintf(v * __builtin_bit_cast(float, 0x3fb8aa3bu));
  float r = fmaf(n, __builtin_bit_cast(float, 0xbf317218u), v);
  r = fmaf(n, __builtin_bit_cast(float, 0x3102e308u), r);
  float p = fmaf(r, __builtin_bit_cast(float, 0x395133b1u), __builtin_bit_cast(float, 0x3ab69700u));
  p = fmaf(r, p, __builtin_bit_cast(float, 0x3c0887f9u));
  p = fmaf(r, p, __builtin_bit_cast(float, 0x3d2aaa81u));
  p = fmaf(r, p, __builtin_bit_cast(float, 0x3e2aaaabu));
  p = fmaf(r, p, 0.5f);
  p = r * p;
  const float m = fmaf(r, p, r);  // expm1(r)
  const float t = __builtin_ldexpf(1.0f, (int)n);
  return fmaf(t, m, t - 1.0f);
}

__device__ __forceinline__ float ph_act(float v, int act) {
  if (act == ACT_RELU) return v > 0.0f ? v : 0.0f;
  if (act == ACT_ELU) {  // branch-free: expm1 of min(v, 0) (a NaN passes through), then the select
    const float e = ph_expm1_neg(v > 0.0f ? 0.0f : v);
    return v > 0.0f ? v : e;
  }
  return v;
}

enum { OUT_LDS = 0, OUT_LDS_HALF = 1, OUT_MEAN = 2, OUT_VALUE = 3, OUT_MEAN_ONLY = 4, OUT_LDS_HALF_EST = 5 };

// ---- k_heads64: ET 32-env column tiles per workgroup.  A 32-env workgroup that keeps every layer's output in LDS
// (139 KB, one per CU) takes ~42 us whether 256 or 512 of them run (4096 / 8192 envs, profiles/r07e), so 8192 envs took
// two rounds.  With ET = 2 each weight fragment feeds BOTH column tiles (six MFMAs per step-tile instead of three, the
// same fragment stream per workgroup), so 8192 envs take one round.  The LDS holds 64 envs' activations in 144 KB
// because no layer output wider than 256 is ever resident: the actor's 512-wide layer runs in two halves of 8 output
// tiles and the critic's 768-wide one in three, each half / third feeding the next layer's accumulators (held in
// registers across the calls) before the next one overwrites it; the short history is staged twice (the estimator's
// first layer, then the actor's).  Every layer call has one output tile per wave.
// ET = 2: act(), and the one-role inference launches past one 32-env tile per CU.  ET = 1: a 32-env workgroup with the
// same layer calls, k order and epilogues per env column (the one-role inference launches up to one tile per CU: half
// the MFMAs per fragment, 72 KB of LDS).
// Measured +-0 and not built: split-K over spare waves on the layers of fewer than 8 output tiles (act() 0.1276-0.1292
// ms off, 0.1282-0.1298 on, profiles/r07c_act_ab.txt) -- the fragment stream from L2 bounds the kernel, not the waves'
// k chains.
template <int ET> using FragE = h8[ET][2][64];  // one k-step of B fragments of the ET env tiles: [env tile][hi, lo][lane]
template <int ET> struct HeadsLds {
  FragE<ET> px[36];  // actor: PX[0..35]; critic: PX[0..31] (layout per phase in ph6_actor / ph6_critic)
};

// one layer call: layer L's output tiles [TB, TB + 8) (or to the layer's last tile) over its k-steps [KB, KE), and its
// weight-fragment register ring: the loads run D k-steps ahead of their MFMAs through D + 1 slots; the first D are
// issued during the previous call (ph6_prologue), so no call starts on an empty pipeline
template <int L_, int KB_, int KE_, int TB_> struct P6Ring {
  static constexpr int L = L_, KB = KB_, KE = KE_, TB = TB_;
  static constexpr int NTL = ph_nt(L), TE = TB + PH_WAVES < NTL ? TB + PH_WAVES : NTL, NW = TE - TB;
  static constexpr int KL = KE - KB, D = PH_RING_DEPTH < KL ? PH_RING_DEPTH : KL - 1, R = D + 1;
  static_assert(PH_WAVES == 8 && KL >= 1 && NW >= 1 && KE <= PH_L[L].ks, "one output tile per wave");
  static __device__ __forceinline__ int tile(int wave) { return wave < NW ? TB + wave : TE - 1; }
  h8 w[R][2];
};
struct P6None {
  static constexpr int L = -1;
};
template <class RG>
__device__ __forceinline__ void ph6_load(const h8* __restrict__ frag, RG& rg, int slot, int s, int wave, int lane) {
  const h8* w = frag + lane + (size_t)((ph_off(RG::L) + RG::tile(wave) * PH_L[RG::L].ks + RG::KB + s) * 2) * 64;
  rg.w[slot][0] = w[0];
  rg.w[slot][1] = w[64];
}
template <class RG>
__device__ __forceinline__ void ph6_prologue(const h8* __restrict__ frag, RG& rg, int wave, int lane) {
#pragma clang loop unroll(full)
  for (int s = 0; s < RG::D; ++s) ph6_load(frag, rg, s, s, wave, lane);
}

struct PhOut64 {  // the global outputs and the workgroup's envs
  const float* eps;
  const float* std;
  float* mean;
  float* actions;
  float* sigma;
  float* logp;
  float* value;
  float* est;  // (batch, 3): the state estimator's output (the actor-only launch; unused otherwise)
  int env0;
  int batch;
};

// stage `steps` k-steps of natural-order B fragments from rows of global memory, for every env tile: element j of lane
// (r, h) of step s, tile et = src[env0 + 32 et + r][col0 + 16 s + 8 h + j] (0 past len or past the batch), split into
// hi / lo.  Steps round-robin over the waves.  (Non-temporal loads here, so that the once-read inputs would not evict
// fragments: act() 0.129 -> 0.153 ms, profiles/r07c_act_ab.txt.)
// T: the source's element type.  An fp16 source (the env's fp16 histories) is its own hi part and its lo part is
// exactly 0 -- what split8 makes of the widened value, so the staged fragments are the fp32 path's on obs.float() bit
// for bit (finite values) -- read by 16-bit loads: its rows are 2-byte aligned only (an obs row's short history starts
// at half 2867 of a 6204-byte row, a critic row is 438 B).
template <bool RELU, int ET, typename T>
__device__ __forceinline__ void ph6_stage(FragE<ET>* dst, int steps, const T* __restrict__ src, long long stride,
                                          int col0, int len, int env0, int batch, int wave, int lane) {
  const int h = lane >> 5;
  for (int s = wave; s < steps; s += PH_WAVES) {
#pragma unroll
    for (int et = 0; et < ET; ++et) {
      const int env = env0 + 32 * et + (lane & 31);
      const bool live = env < batch;
      const T* row = src + (long long)(live ? env : batch - 1) * stride + col0;
      if constexpr (std::is_same<T, _Float16>::value) {
        static_assert(!RELU, "the fp16 sources are staged as they are");
        h8 hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = 16 * s + 8 * h + j;
          hi[j] = (live && c < len) ? row[c] : (_Float16)0.0f;
        }
        dst[s][et][0][lane] = hi;
        dst[s][et][1][lane] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      } else {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = 16 * s + 8 * h + j;
          const float x = (live && c < len) ? row[c] : 0.0f;
          v[j] = RELU ? (x > 0.0f ? x : 0.0f) : x;
        }
        h8 hi, lo;
        split8(v, hi, lo);
        dst[s][et][0][lane] = hi;
        dst[s][et][1][lane] = lo;
      }
    }
  }
}

// one layer call (see P6Ring): B fragments in[0 .. KL) from LDS, A fragments through the ring rg (prologue issued by the
// previous call), six MFMAs per k-step into acc (ZERO: start from 0; the caller owns acc, so a layer split over calls
// keeps its sums); EPI: result + bias through the activation into out (k-steps out0 + 2 (tile - TB) + {0, 1}) or the
// global outputs.  NX: the next call's ring, whose first fragments are issued before this call's epilogue.
template <class RG, int OUT, bool ZERO, bool EPI, class NX, int ET>
__device__ __forceinline__ void ph6_call(const h8* __restrict__ frag, const FragE<ET>* in, FragE<ET>* out, int out0,
                                         const PhOut64& G, int wave, int lane, RG& rg, NX* nx, f16v (&acc0)[ET],
                                         f16v (&acc1)[ET]) {
  constexpr Layer Y = PH_L[RG::L];
  constexpr int KL = RG::KL, D = RG::D, R = RG::R;
  const int h = lane >> 5;
  const bool busy = wave < RG::NW;  // wave-uniform
  if constexpr (ZERO) {
#pragma unroll
    for (int et = 0; et < ET; ++et)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[et][r] = acc1[et][r] = 0.0f;
  }
  float4 bias[4];
  h8 bq[2][ET][2];  // [buffer][env tile][hi, lo]
#pragma unroll
  for (int et = 0; et < ET; ++et) {
    bq[0][et][0] = in[0][et][0][lane];
    bq[0][et][1] = in[0][et][1][lane];
  }
  if (busy)
#pragma clang loop unroll(full)
    for (int s = 0; s < KL; ++s) {
      if (s + D < KL) ph6_load(frag, rg, (s + D) % R, s + D, wave, lane);
      if (EPI && s == KL - 1 - D) {  // the bias fragments behind the call's last weight loads
        const float4* bf = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(frag) + PH_WFRAG_BYTES);
#pragma unroll
        for (int q = 0; q < 4; ++q) bias[q] = bf[((ph_toff(RG::L) + RG::tile(wave)) * 4 + q) * 64 + lane];
      }
      if (s + 1 < KL) {
#pragma unroll
        for (int et = 0; et < ET; ++et) {
          bq[(s + 1) & 1][et][0] = in[s + 1][et][0][lane];
          bq[(s + 1) & 1][et][1] = in[s + 1][et][1][lane];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      const h8 ah = rg.w[s % R][0], al = rg.w[s % R][1];
#pragma unroll
      for (int et = 0; et < ET; ++et) {
        const h8 bh = bq[s & 1][et][0], bl = bq[s & 1][et][1];
        acc0[et] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc0[et], 0, 0, 0);
        acc1[et] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc1[et], 0, 0, 0);
        acc1[et] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc1[et], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  if constexpr (NX::L >= 0) ph6_prologue(frag, *nx, wave, lane);  // the next call's first fragments in flight
  if constexpr (EPI) {
    if (!busy) return;
    const int nt = RG::TB + wave;
#pragma unroll
    for (int et = 0; et < ET; ++et) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float4 b4 = bias[r >> 2];
        const float b = (r & 3) == 0 ? b4.x : (r & 3) == 1 ? b4.y : (r & 3) == 2 ? b4.z : b4.w;
        v[r] = ph_act(acc0[et][r] + acc1[et][r] * (1.0f / PH_SPLIT) + b, Y.act);
      }
      const int env = G.env0 + 32 * et + (lane & 31);
      const bool live = env < G.batch;
      if constexpr (OUT == OUT_LDS || OUT == OUT_LDS_HALF || OUT == OUT_LDS_HALF_EST) {
        if constexpr (OUT == OUT_LDS_HALF_EST) {  // the estimate (rows 0-2: registers 0-2 of lane half 0) before the split
          if (h == 0 && live) {
#pragma unroll
            for (int r = 0; r < 3; ++r) G.est[(size_t)env * 3 + r] = v[r];
          }
        }
#pragma unroll
        for (int s = 0; s < (OUT == OUT_LDS ? 2 : 1); ++s) {
          float u[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) u[j] = v[8 * s + j];
          h8 hi, lo;
          split8(u, hi, lo);
          out[out0 + 2 * (nt - RG::TB) + s][et][0][lane] = hi;
          out[out0 + 2 * (nt - RG::TB) + s][et][1][lane] = lo;
        }
      } else if constexpr (OUT == OUT_MEAN_ONLY) {  // the deterministic policy: the mean alone (no eps, std, sample)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
          if (row < Y.n && live) G.mean[(size_t)env * Y.n + row] = v[r];
        }
      } else if constexpr (OUT == OUT_MEAN) {
        // the Normal sample a = mean + sigma eps and its log-prob, summed over the 12 actions (DHPPO._act_body;
        // torch.distributions.Normal.log_prob): rows 0-3, 8-11 on lane half 0, rows 4-7 on half 1
        float lp = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
          if (row < Y.n && live) {
            const float sd = G.std[row];
            const size_t ix = (size_t)env * Y.n + row;
            const float a = v[r] + sd * G.eps[ix];
            const float d = a - v[r];
            lp += -(d * d) / (2.0f * (sd * sd)) - logf(sd) - 0.91893853320467274178f;  // log(sqrt(2 pi))
            G.mean[ix] = v[r];
            G.actions[ix] = a;
            G.sigma[ix] = sd;
          }
        }
        lp += __shfl_xor(lp, 32);
        if (h == 0 && live) G.logp[env] = lp;
      } else {
        if (h == 0 && live) G.value[env] = v[0];
      }
    }
  }
}

template <int L, int KB, int KE, int TB = 0> using R6 = P6Ring<L, KB, KE, TB>;
template <int L> using R6F = P6Ring<L, 0, PH_L[L].ks, 0>;  // a whole layer

// the actor chain of one workgroup (history tail, state estimator, actor) on its ET env tiles.  TO: the element type of
// obs (float, or _Float16: the _h entries); y1 is fp32 either way.  DET: the deterministic policy (act_inference) --
// the last epilogue writes the mean alone and layer 6's also stores the estimate to G.est.
template <typename TO, int ET, bool DET>
__device__ __forceinline__ void ph6_actor(const h8* __restrict__ frag, const float* __restrict__ y1,
                                          const TO* __restrict__ obs, int obs_cols, FragE<ET>* X, const PhOut64& G,
                                          int batch, int wave, int lane) {
  f16v a0[ET], a1[ET];  // the current call's accumulators
  f16v b0[ET], b1[ET];  // the layer after a split one: its sums across the split layer's calls
  // PX[0..27] the relu'd conv1 output; L0 -> PX[28..33]; L1 -> PX[0..7]; short history -> PX[16..30]; L2 (the
  // history code) -> PX[32..35]; L3 -> PX[0..15]; L4 -> PX[16..23]; L5 -> PX[0..3]; L6 (the estimate) -> PX[31];
  // short history again -> PX[16..30]; the actor input is PX[16..35]; L7 halves -> PX[0..15], each into L8's sums;
  // L8 -> PX[16..31]; L9 -> PX[0..7]; L10 -> the outputs
  ph6_stage<true, ET>(X, 28, y1, PH_Y1, 0, PH_Y1, G.env0, batch, wave, lane);
  R6F<0> g0;
  ph6_prologue(frag, g0, wave, lane);
  __syncthreads();
  R6F<1> g1;
  ph6_call<R6F<0>, OUT_LDS, true, true>(frag, X, X, 28, G, wave, lane, g0, &g1, a0, a1);
  __syncthreads();
  R6F<2> g2;
  ph6_call<R6F<1>, OUT_LDS, true, true>(frag, X + 28, X, 0, G, wave, lane, g1, &g2, a0, a1);
  __syncthreads();
  ph6_stage<false, ET>(X + 16, 15, obs, obs_cols, obs_cols - PH_OBS_SHORT, PH_OBS_SHORT, G.env0, batch, wave, lane);
  R6F<3> g3;
  ph6_call<R6F<2>, OUT_LDS, true, true>(frag, X, X, 32, G, wave, lane, g2, &g3, a0, a1);
  __syncthreads();
  R6F<4> g4;
  ph6_call<R6F<3>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g3, &g4, a0, a1);
  __syncthreads();
  R6F<5> g5;
  ph6_call<R6F<4>, OUT_LDS, true, true>(frag, X, X, 16, G, wave, lane, g4, &g5, a0, a1);
  __syncthreads();
  R6F<6> g6;
  ph6_call<R6F<5>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g5, &g6, a0, a1);
  __syncthreads();
  R6<7, 0, 20, 0> g7a;
  ph6_call<R6F<6>, DET ? OUT_LDS_HALF_EST : OUT_LDS_HALF, true, true>(frag, X, X, 31, G, wave, lane, g6, &g7a, a0, a1);
  ph6_stage<false, ET>(X + 16, 15, obs, obs_cols, obs_cols - PH_OBS_SHORT, PH_OBS_SHORT, G.env0, batch, wave, lane);
  __syncthreads();
  R6<8, 0, 16> g8a;
  ph6_call<R6<7, 0, 20, 0>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g7a, &g8a, a0, a1);
  __syncthreads();
  R6<7, 0, 20, 8> g7b;
  ph6_call<R6<8, 0, 16>, OUT_LDS, true, false>(frag, X, (FragE<ET>*)nullptr, 0, G, wave, lane, g8a, &g7b, b0, b1);
  __syncthreads();
  R6<8, 16, 32> g8b;
  ph6_call<R6<7, 0, 20, 8>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g7b, &g8b, a0, a1);
  __syncthreads();
  R6F<9> g9;
  ph6_call<R6<8, 16, 32>, OUT_LDS, false, true>(frag, X, X, 16, G, wave, lane, g8b, &g9, b0, b1);
  __syncthreads();
  R6F<10> g10;
  ph6_call<R6F<9>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g9, &g10, a0, a1);
  __syncthreads();
  ph6_call<R6F<10>, DET ? OUT_MEAN_ONLY : OUT_MEAN, true, true, P6None>(frag, X, (FragE<ET>*)nullptr, 0, G, wave, lane,
                                                                        g10, nullptr, a0, a1);
}

// the critic chain of one workgroup on its ET env tiles
template <typename TO, int ET>
__device__ __forceinline__ void ph6_critic(const h8* __restrict__ frag, const TO* __restrict__ cobs, int cobs_cols,
                                           FragE<ET>* X, const PhOut64& G, int batch, int wave, int lane) {
  f16v a0[ET], a1[ET];
  f16v b0[ET], b1[ET];
  // PX[16..29] the privileged observations; L11 thirds -> PX[0..15], each into L12's sums; L12 -> PX[16..31];
  // L13 -> PX[0..7]; L14 -> the value
  ph6_stage<false, ET>(X + 16, 14, cobs, cobs_cols, 0, PH_CRITIC, G.env0, batch, wave, lane);
  R6<11, 0, 14, 0> g11a;
  ph6_prologue(frag, g11a, wave, lane);
  __syncthreads();
  R6<12, 0, 16> g12a;
  ph6_call<R6<11, 0, 14, 0>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g11a, &g12a, a0, a1);
  __syncthreads();
  R6<11, 0, 14, 8> g11b;
  ph6_call<R6<12, 0, 16>, OUT_LDS, true, false>(frag, X, (FragE<ET>*)nullptr, 0, G, wave, lane, g12a, &g11b, b0, b1);
  __syncthreads();
  R6<12, 16, 32> g12b;
  ph6_call<R6<11, 0, 14, 8>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g11b, &g12b, a0, a1);
  __syncthreads();
  R6<11, 0, 14, 16> g11c;
  ph6_call<R6<12, 16, 32>, OUT_LDS, false, false>(frag, X, (FragE<ET>*)nullptr, 0, G, wave, lane, g12b, &g11c, b0, b1);
  __syncthreads();
  R6<12, 32, 48> g12c;
  ph6_call<R6<11, 0, 14, 16>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g11c, &g12c, a0, a1);
  __syncthreads();
  R6F<13> g13;
  ph6_call<R6<12, 32, 48>, OUT_LDS, false, true>(frag, X, X, 16, G, wave, lane, g12c, &g13, b0, b1);
  __syncthreads();
  R6F<14> g14;
  ph6_call<R6F<13>, OUT_LDS, true, true>(frag, X + 16, X, 0, G, wave, lane, g13, &g14, a0, a1);
  __syncthreads();
  ph6_call<R6F<14>, OUT_VALUE, true, true, P6None>(frag, X, (FragE<ET>*)nullptr, 0, G, wave, lane, g14, nullptr, a0, a1);
}

// the roles of a launch: both (act(): actor and critic workgroups interleaved over blockIdx, the sampled policy), or one
// (every workgroup of the grid an actor tile -- the deterministic policy and the estimate -- or a critic tile)
enum { ROLE_BOTH = 0, ROLE_ACTOR = 1, ROLE_CRITIC = 2 };

// TO: the element type of obs and cobs (float, or _Float16: the _h entries); y1 is fp32 either way
template <typename TO, int ET = 2, int ROLE = ROLE_BOTH>
__global__ __launch_bounds__(64 * PH_WAVES) __attribute__((amdgpu_waves_per_eu(PH_WAVES / 4, PH_WAVES / 4)))
void k_heads64(const h8* __restrict__ frag, const float* __restrict__ y1, const TO* __restrict__ obs, int obs_cols,
               const TO* __restrict__ cobs, int cobs_cols, PhOut64 G, int batch) {
  __shared__ HeadsLds<ET> S;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int bid = blockIdx.x;
  // ROLE_BOTH: both roles on every XCD (blockIdx mod 8), alternating in each XCD's dispatch order -- a CU's two
  // workgroups tend to be one actor chain and one critic, and each L2 holds both roles' 3.6 MB of fragments: act()
  // 0.139-0.140 ms, against 0.142 with the actor on XCDs 0-3 and the critic on 4-7 (the actor chain is 23% longer, so
  // its XCDs finish last) and 0.140 with the roles alternating by workgroup (profiles/r05hx_act_ab.txt)
  const bool critic = ROLE == ROLE_BOTH ? ((bid >> 3) & 1) != 0 : ROLE == ROLE_CRITIC;
  const int tile = ROLE == ROLE_BOTH ? ((bid >> 4) << 3) + (bid & 7) : bid;
  G.env0 = tile * (32 * ET);
  G.batch = batch;
  if (G.env0 >= batch) return;
  if constexpr (ROLE == ROLE_BOTH) {
    if (!critic)
      ph6_actor<TO, ET, false>(frag, y1, obs, obs_cols, S.px, G, batch, wave, lane);
    else
      ph6_critic<TO, ET>(frag, cobs, cobs_cols, S.px, G, batch, wave, lane);
  } else if constexpr (ROLE == ROLE_ACTOR) {
    ph6_actor<TO, ET, true>(frag, y1, obs, obs_cols, S.px, G, batch, wave, lane);
  } else {
    ph6_critic<TO, ET>(frag, cobs, cobs_cols, S.px, G, batch, wave, lane);
  }
}

bool ph_params(const uint64_t* params, PhParams& P) {
  for (int l = 0; l < PH_NLAYER; ++l) {
    P.w[l] = reinterpret_cast<const float*>(params[2 * l]);
    P.b[l] = reinterpret_cast<const float*>(params[2 * l + 1]);
    if (!P.w[l] || !P.b[l]) return false;
  }
  P.std = reinterpret_cast<const float*>(params[2 * PH_NLAYER]);
  return P.std != nullptr;
}

// the parameter shapes the kernels are compiled for: (out, in) per layer, conv2 as (16, 32 * 4)
bool ph_dims_match(const int* dims) {
  static const int want[PH_NLAYER][2] = {{16, 128}, {128, 96}, {64, 128}, {256, 235}, {128, 256}, {64, 128}, {3, 64},
                                         {512, 302}, {256, 512}, {128, 256}, {12, 128}, {768, 219}, {256, 768},
                                         {128, 256}, {1, 128}};
  for (int l = 0; l < PH_NLAYER; ++l)
    if (dims[2 * l] != want[l][0] || dims[2 * l + 1] != want[l][1]) return false;
  return true;
}

}  // namespace

extern "C" {

int t1policy_heads_frag_bytes(void) { return PH_FRAG_BYTES; }

int t1policy_heads_pack(const uint64_t* params, const int* dims, void* frag, void* stream) {
  if (!params || !dims || !frag) return -1;
  if (!ph_dims_match(dims)) return 1;
  if ((reinterpret_cast<uintptr_t>(frag) & 15u) != 0) return -1;
  PhParams P;
  if (!ph_params(params, P)) return -1;
  hipLaunchKernelGGL(k_heads_pack, dim3(((PH_UNITS + PH_TILES) * 64 + 255) / 256), dim3(256), 0, (hipStream_t)stream, P,
                     reinterpret_cast<h8*>(frag));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"

namespace {

// the env tile of a one-role launch: 32 envs per workgroup (ET 1) while every 32-env tile gets a CU of its own, 64
// (ET 2) above that -- a workgroup's time grows with its envs (42 us at 32, 80 us at 64 in act()), but past one
// workgroup per CU a second round of 32-env tiles costs more than 64-env tiles in one.  T1POLICY_INFER_TILE=32|64
// overrides (A/B, tests).
int ph_infer_et(int batch) {
  if (const char* tv = getenv("T1POLICY_INFER_TILE")) {
    if (atoi(tv) == 32) return 1;
    if (atoi(tv) == 64) return 2;
  }
  static int cus = 0;  // the device's CU count, read once (t1env.hip reads it the same way for t1_dyn_kernel_default)
  if (cus == 0) {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return (batch + 31) / 32 <= cus ? 1 : 2;
}

template <typename TO, int ROLE>
int ph_infer_launch(const void* frag, const float* y1, const TO* obs, int obs_cols, const TO* cobs, int cobs_cols,
                    const PhOut64& G, int batch, void* stream) {
  const h8* f = reinterpret_cast<const h8*>(frag);
  if (ph_infer_et(batch) == 1)
    hipLaunchKernelGGL((k_heads64<TO, 1, ROLE>), dim3((batch + 31) / 32), dim3(64 * PH_WAVES), 0, (hipStream_t)stream,
                       f, y1, obs, obs_cols, cobs, cobs_cols, G, batch);
  else
    hipLaunchKernelGGL((k_heads64<TO, 2, ROLE>), dim3((batch + 63) / 64), dim3(64 * PH_WAVES), 0, (hipStream_t)stream,
                       f, y1, obs, obs_cols, cobs, cobs_cols, G, batch);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename TO>
int ph_actor_forward(const uint64_t* params, const int* dims, const void* frag, const float* y1, const TO* obs,
                     int obs_cols, float* mean, float* est_vel, int batch, void* stream) {
  if (!params || !dims || !frag || !y1 || !obs || !mean || !est_vel || batch < 0) return -1;
  if (!ph_dims_match(dims)) return 1;
  if (obs_cols < PH_OBS_SHORT) return 1;
  if (batch == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(frag) & 15u) != 0) return -1;
  if (sizeof(TO) == 2 && (reinterpret_cast<uintptr_t>(obs) & 1u) != 0) return -1;
  PhParams P;
  if (!ph_params(params, P)) return -1;
  const PhOut64 G{nullptr, nullptr, mean, nullptr, nullptr, nullptr, nullptr, est_vel, 0, batch};
  return ph_infer_launch<TO, ROLE_ACTOR>(frag, y1, obs, obs_cols, (const TO*)nullptr, 0, G, batch, stream);
}

template <typename TO>
int ph_critic_forward(const uint64_t* params, const int* dims, const void* frag, const TO* critic_obs,
                      int critic_cols, float* value, int batch, void* stream) {
  if (!params || !dims || !frag || !critic_obs || !value || batch < 0) return -1;
  if (!ph_dims_match(dims)) return 1;
  if (critic_cols != PH_CRITIC) return 1;
  if (batch == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(frag) & 15u) != 0) return -1;
  if (sizeof(TO) == 2 && (reinterpret_cast<uintptr_t>(critic_obs) & 1u) != 0) return -1;
  PhParams P;
  if (!ph_params(params, P)) return -1;
  const PhOut64 G{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, value, nullptr, 0, batch};
  return ph_infer_launch<TO, ROLE_CRITIC>(frag, nullptr, (const TO*)nullptr, 0, critic_obs, critic_cols, G, batch,
                                          stream);
}

template <typename TO>
int ph_heads_forward(const uint64_t* params, const int* dims, const void* frag, const float* y1, const TO* obs,
                     int obs_cols, const TO* critic_obs, int critic_cols, const float* eps, float* mean,
                     float* actions, float* sigma, float* logp, float* value, int batch, void* stream) {
  if (!params || !dims || !frag || !y1 || !obs || !critic_obs || !eps || !mean || !actions || !sigma || !logp ||
      !value || batch < 0)
    return -1;
  if (!ph_dims_match(dims)) return 1;
  if (obs_cols < PH_OBS_SHORT || critic_cols != PH_CRITIC) return 1;
  if (batch == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(frag) & 15u) != 0) return -1;
  if (sizeof(TO) == 2 && ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(critic_obs)) & 1u) != 0)
    return -1;
  PhParams P;
  if (!ph_params(params, P)) return -1;
  const PhOut64 G{eps, P.std, mean, actions, sigma, logp, value, nullptr, 0, batch};
  const int tiles = (batch + 63) / 64;
  hipLaunchKernelGGL(k_heads64<TO>, dim3(16 * ((tiles + 7) / 8)), dim3(64 * PH_WAVES), 0, (hipStream_t)stream,
                     reinterpret_cast<const h8*>(frag), y1, obs, obs_cols, critic_obs, critic_cols, G, batch);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

extern "C" {

// act(): both roles in one launch, actor and critic tiles interleaved (k_heads64<.., 2, ROLE_BOTH>)
int t1policy_heads_forward(const uint64_t* params, const int* dims, const void* frag, const float* y1,
                           const float* obs, int obs_cols, const float* critic_obs, int critic_cols, const float* eps,
                           float* mean, float* actions, float* sigma, float* logp, float* value, int batch,
                           void* stream) {
  return ph_heads_forward<float>(params, dims, frag, y1, obs, obs_cols, critic_obs, critic_cols, eps, mean, actions,
                                 sigma, logp, value, batch, stream);
}
int t1policy_heads_forward_h(const uint64_t* params, const int* dims, const void* frag, const float* y1,
                             const void* obs, int obs_cols, const void* critic_obs, int critic_cols, const float* eps,
                             float* mean, float* actions, float* sigma, float* logp, float* value, int batch,
                             void* stream) {
  return ph_heads_forward<_Float16>(params, dims, frag, y1, reinterpret_cast<const _Float16*>(obs), obs_cols,
                                    reinterpret_cast<const _Float16*>(critic_obs), critic_cols, eps, mean, actions,
                                    sigma, logp, value, batch, stream);
}
// the deterministic policy and the estimate: the actor chain alone, every workgroup an actor tile (k_heads64<.., ROLE_ACTOR>)
int t1policy_actor_forward(const uint64_t* params, const int* dims, const void* frag, const float* y1,
                           const float* obs, int obs_cols, float* mean, float* est_vel, int batch, void* stream) {
  return ph_actor_forward<float>(params, dims, frag, y1, obs, obs_cols, mean, est_vel, batch, stream);
}
int t1policy_actor_forward_h(const uint64_t* params, const int* dims, const void* frag, const float* y1,
                             const void* obs, int obs_cols, float* mean, float* est_vel, int batch, void* stream) {
  return ph_actor_forward<_Float16>(params, dims, frag, y1, reinterpret_cast<const _Float16*>(obs), obs_cols, mean,
                                    est_vel, batch, stream);
}
// the value: the critic chain alone (k_heads64<.., ROLE_CRITIC>)
int t1policy_critic_forward(const uint64_t* params, const int* dims, const void* frag, const float* critic_obs,
                            int critic_cols, float* value, int batch, void* stream) {
  return ph_critic_forward<float>(params, dims, frag, critic_obs, critic_cols, value, batch, stream);
}
int t1policy_critic_forward_h(const uint64_t* params, const int* dims, const void* frag, const void* critic_obs,
                              int critic_cols, float* value, int batch, void* stream) {
  return ph_critic_forward<_Float16>(params, dims, frag, reinterpret_cast<const _Float16*>(critic_obs), critic_cols,
                                     value, batch, stream);
}

}  // extern "C"
