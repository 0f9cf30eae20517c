// t1env_prof.h -- the phase marks of the step kernels (k_dyn4, k_dyn5, k_dyn6), one copy for the three units.
//
// A unit includes this header once, right after <hip/hip_runtime.h> and before the headers that place marks, with
//   T1_PROF_WAVES     the waves of its workgroup
//   T1_PROF_NAME(x)   x with the unit's suffix (none, 5, 6): its accumulators and its exported reader
//                     t1env_debug_phase_cycles<suffix>(out[T1_PROF_WAVES][24], reset)
// defined.  The product build compiles every mark out.
//   -DT1_PHASE_PROF (tools/prof_dynamics_phases.py): lane 0 of every wave accumulates shader-clock deltas between
//                   T1_PROF_MARK points into per-phase buckets
//   -DT1_ASM_MARKS  (tools/isa_phases.py): the marks as assembly comments, for static instruction counts
#pragma once

#ifdef T1_PHASE_PROF
constexpr int T1_NPROF = 24;
__device__ unsigned long long T1_PROF_NAME(g_t1_prof)[T1_PROF_WAVES][T1_NPROF];
__shared__ unsigned long long T1_PROF_NAME(t1_prof_acc)[T1_PROF_WAVES][T1_NPROF + 1];  // [wave][bucket], last = previous mark
// a stamp is one asm statement (s_memtime + its lgkmcnt wait) fenced by scheduling barriers, so the compiler
// cannot move work across it (cdna_hip_programming.md, In-kernel stamps)
static __device__ __forceinline__ unsigned long long t1_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
static __device__ __forceinline__ void t1_prof_mark(int i) {
  const int w = threadIdx.x / 64;
  const unsigned long long now = t1_stamp();
  if ((threadIdx.x & 63) == 0) {
    T1_PROF_NAME(t1_prof_acc)[w][i] += now - T1_PROF_NAME(t1_prof_acc)[w][T1_NPROF];
    T1_PROF_NAME(t1_prof_acc)[w][T1_NPROF] = now;
  }
}
static __device__ __forceinline__ void t1_prof_begin() {
  const int w = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
    for (int i = 0; i < T1_NPROF; ++i) T1_PROF_NAME(t1_prof_acc)[w][i] = 0;
    T1_PROF_NAME(t1_prof_acc)[w][T1_NPROF] = t1_stamp();
  }
}
static __device__ __forceinline__ void t1_prof_end() {
  const int w = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < T1_NPROF; ++i) atomicAdd(&T1_PROF_NAME(g_t1_prof)[w][i], T1_PROF_NAME(t1_prof_acc)[w][i]);
}
// summed clock deltas per [wave][bucket] since the last reset (reset != 0: zeroed after the read)
extern "C" int T1_PROF_NAME(t1env_debug_phase_cycles)(unsigned long long* out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(T1_PROF_NAME(g_t1_prof)), sizeof(T1_PROF_NAME(g_t1_prof)));
  if (e == hipSuccess && reset) {
    static const unsigned long long zero[T1_PROF_WAVES][T1_NPROF] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(T1_PROF_NAME(g_t1_prof)), zero, sizeof(zero));
  }
  return (int)e;
}
#define T1_PROF_MARK(i) t1_prof_mark(i)
#define T1_PROF_BEGIN() t1_prof_begin()
#define T1_PROF_END() t1_prof_end()
#elif defined(T1_ASM_MARKS)
#define T1_ASM_STR2(x) #x
#define T1_ASM_STR(x) T1_ASM_STR2(x)
#define T1_PROF_MARK(i) asm volatile(";@@MARK " #i "@L" T1_ASM_STR(__LINE__))
#define T1_PROF_BEGIN() asm volatile(";@@MARK begin")
#define T1_PROF_END() asm volatile(";@@MARK end")
#else
#define T1_PROF_MARK(i) ((void)0)
#define T1_PROF_BEGIN() ((void)0)
#define T1_PROF_END() ((void)0)
#endif
