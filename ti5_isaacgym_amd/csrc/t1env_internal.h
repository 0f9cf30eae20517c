// t1env_internal.h -- entry points shared between the library's translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/t1env.h"
#include "t1_dynamics.h"

#include "t1env_device.h"

// state of the fused step (a step kernel with post-physics in its epilogue)
struct FusedArgs {
  unsigned* done;                  // dynamics-workgroup completion counter (the last one finalises the extras)
  uint32_t* unit_state;            // per shift unit: epoch-tagged handoff word (reset mask inside)
  uint32_t epoch;                  // launch number (unique per fused step)
  float* ep_part;                  // per dynamics workgroup one row of EP_PART_ROW partial extras sums
                                   //    ([0,24) episode sums over reset envs, [24] reset count, [25] terrain levels)
};
constexpr int EP_PART_ROW = 32;

// substep log of the fused k_dyn4 (t1env_substep_log; all null = off)
struct SubLog {
  float* root;
  float* dof;
  float* torque;
};

// the step kernel and where its history shift runs
struct DynLaunch {
  int kernel;        // 6: k_dyn6 (t1env_dyn6.hip: 32 envs per workgroup, eight role waves, two per SIMD), 5: k_dyn5
                     //    (t1env_dyn5.hip: 32 envs per workgroup, four roles, in-workgroup history shift), 4: k_dyn4
                     //    (64 envs per workgroup, leg + contact helper waves; its shift is always the side launch
                     //    k_shift4c); t1_dyn_kernel_default picks k_dyn6 (k_dyn4 for fp16 histories above one round),
                     //    T1ENV_DYN_KERNEL=4|5|6 overrides
  int cus;           // compute units of the device (the shift launches' grid)
  int d5_shift;      // k_dyn5's history shift: 0 = in the workgroup through LDS-DMA (default), 1 = the side launch
                     // k_shift5 on a second stream (T1ENV_D5_SHIFT=1, A/B: the same step time, r04e)
};
int t1_dyn_kernel_default(int num_envs, int cus, bool obs_half);

// The step kernel's launch (t1env_dynamics.hip); fused != nullptr: the whole step (post-physics in the epilogue).
// k_dyn5 with d5_shift = 0 and k_dyn6 shift the histories S in their workgroups; otherwise the caller runs
// t1_launch_shift beside this launch.  log: the substep log (fused k_dyn4 only).  Returns a hipError_t.
int t1_launch_dynamics(const t1::DynModel* d_model, const t1env_config* d_cfg, const t1env_buffers& B,
                       const t1::Terrain& T, const float* actions, const t1env_step_args& A, int num_envs,
                       const t1::ShiftArgs& S, const DynLaunch& cfg, const FusedArgs* fused, hipStream_t s,
                       const SubLog* log = nullptr);
// k_dyn5 (t1env_dyn5.hip): the same contract as t1_launch_dynamics; each workgroup shifts its own history rows
int t1_launch_dyn5(const t1::DynModel* d_model, const t1env_config* d_cfg, const t1env_buffers& B, const t1::Terrain& T,
                   const float* actions, const t1env_step_args& A, int num_envs, const t1::ShiftArgs& S,
                   const FusedArgs* fused, hipStream_t s, const SubLog* log, bool inwg_shift);
// k_dyn6 (t1env_dyn6.hip): k_dyn5's roles on eight waves (two per SIMD), the same contract; each workgroup shifts its own
// history rows
int t1_launch_dyn6(const t1::DynModel* d_model, const t1env_config* d_cfg, const t1env_buffers& B, const t1::Terrain& T,
                   const float* actions, const t1env_step_args& A, int num_envs, const t1::ShiftArgs& S,
                   const FusedArgs* fused, hipStream_t s, const SubLog* log);
// The renderer (t1render.hip, include/t1render.h) reads a handle through this view: the body poses, the terrain and
// the env count; t1_fail sets t1env_last_error()'s string and returns code (both in t1env.hip).
struct RenderView {
  const float* rigid_state;   // (N, 13, 13)
  t1::Terrain terrain;
  int num_envs;
  float z_top;                // the height field's highest sample [m]
  float z_bot;                // its lowest sample [m] (0 on the plane): no terrain receives a shadow below it
};
int t1_render_view(const t1env* e, RenderView* v);
int t1_fail(int code, const char* msg);
// The history shift as a launch of its own (t1env.hip).  beside: the step kernel it shares the CUs with -- 5: k_shift5
// (<= 96 registers per lane, beside a k_dyn5 wave), 4: k_shift4c (<= 72, beside a k_dyn4 wave), one workgroup per CU;
// 0: none (the paths without a step kernel), k_shift4c with four workgroups per CU.  fused: the unit handoff with the
// fused epilogue, else plain (the caller's k_post_b zeroes the reset rows in stream order)
int t1_launch_shift(const t1::ShiftArgs& S, const FusedArgs* fused, int num_envs, int cus, hipStream_t s, int beside);
