"""Dev probe: the shader clock k_dyn6 runs at (a -DT1_PROBE_CLOCK build: lane 0 of every workgroup's wave 0 reads the
shader-cycle counter (s_memtime) and the 100 MHz constant counter (s_memrealtime) at the start and end of the launch and
adds the deltas to two device counters), against the step time -- to tell a clock (power-management) mode from a code
mode when a build's step time differs across processes (VERDICT r5 #1b, the -O2 slow mode).

    T1ENV_LIB=ti5_isaacgym_amd/_lib/var/<probe build>.so python tools/clock_probe.py [--steps 300]

The per-workgroup sums split W0's S1 waits into the first S1 of the launch (W0 waits there for the slowest wave's
prologue: the staging loads) and the S1s of substeps 1+ (it waits for the shift waves' S2 -> S1 tails: their stores and
next loads), and give each shift role's S2 -> S1 tail by shift index (roles 1, 2, 3, 5, 6, 7).  The modes of a build
are per process: run it in several fresh processes.

`tail_by_resets` splits the time of W0 (the rewards wave, which carries the finaliser) and W1 (the state wave, which
carries reset_idx) past the epilogue barrier at the build's tail stamps -- W0: post_a_core, its reset-row work, its
store drain, the wait at E2, the finaliser; W1: post_a_core, its reset work ahead of E2, the level sum, the wait at E2,
what it runs behind E2 -- by the workgroup's reset count that step, over --samples further launches.  With the reward
terms dealt over W4-W7: W0's own terms (stamp 0 to 6), its wait at the hand-over word (6 to 7), and the arrival there of
each helper W4-W7 (14-17), from W0's stamp past the epilogue barrier.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ti5_isaacgym_amd import make_t1_env  # noqa: E402


NSUM = 10  # T1_WGSUM6_N: W0 life, S1 waits of substeps 1+, S2 waits, first S1 wait, six shift roles' S2 -> S1 tails


# the tail stamps of a workgroup (T1_TAIL6_N ticks of 100 MHz, t1env_dyn6.hip): W0 at 0-7, W1 at 8-13, W4-W7 at 14-17
TAIL_SEGMENTS = {"w0_post_a_core": (0, 1), "w0_reset_rows": (1, 2), "w0_store_drain": (2, 3), "w0_e2_wait": (3, 4),
                 "w0_finaliser": (4, 5), "w1_post_a_core": (8, 9), "w1_reset_before_e2": (9, 10),
                 "w1_level_sum_and_drain": (10, 11), "w1_e2_wait": (11, 12), "w1_after_e2": (12, 13),
                 "w0_barrier_to_end": (0, 5), "w1_barrier_to_e2": (8, 11), "w1_barrier_to_end": (8, 13),
                 "w0_own_terms": (0, 6), "w0_deal_wait": (6, 7), "w4_barrier_to_handover": (0, 14),
                 "w5_barrier_to_handover": (0, 15), "w6_barrier_to_handover": (0, 16),
                 "w7_barrier_to_handover": (0, 17)}
TAIL_N = 20  # T1_TAIL6_N


def tail_by_resets(lib, env, acts, wg, samples):
    """The time of W0 and W1 past the epilogue barrier, split at the tail stamps, over `samples` further launches (each
    synchronised and read back): the mean of every segment in workgroups without a reset, with one, and with more; W0's
    loop-end-to-last-instruction time likewise; and how many of each launch's six last-finishing workgroups hold a reset."""
    seg = {k: {"0": [], "1": [], ">=2": []} for k in list(TAIL_SEGMENTS) + ["epilogue"]}
    last6, wgs = [], []
    tl, tail = np.zeros((wg, 4), np.uint64), np.zeros((wg, TAIL_N), np.uint64)
    for i in range(samples):
        env.step(acts[i % 8])
        torch.cuda.synchronize()
        lib.t1env_debug_wgtime6(tl.ctypes.data_as(ctypes.c_void_p), wg)
        lib.t1env_debug_tail6(tail.ctypes.data_as(ctypes.c_void_p), wg)
        rs = env.reset_buf.detach().to(torch.int32).cpu().numpy()[: wg * 32].reshape(wg, 32).sum(1)
        t, w = tail.astype(np.int64) / 100.0, tl.astype(np.int64) / 100.0
        groups = {"0": rs == 0, "1": rs == 1, ">=2": rs >= 2}
        for k, (i0, i1) in TAIL_SEGMENTS.items():
            for g, m in groups.items():
                seg[k][g].extend((t[m, i1] - t[m, i0]).tolist())
        for g, m in groups.items():
            seg["epilogue"][g].extend((w[m, 1] - w[m, 3]).tolist())
        last6.append(int((rs[np.argsort(-w[:, 2])[:6]] > 0).sum()))
        wgs.append(int((rs > 0).sum()))
    mean = lambda v: round(float(np.mean(v)), 2) if v else None  # noqa: E731
    return {"us_mean": {k: {g: mean(v) for g, v in d.items()} for k, d in seg.items()}, "launches": samples,
            "reset_wgs_per_launch_mean": mean(wgs), "reset_wgs_among_last_six_finishers": last6}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--num-envs", type=int, default=8192)
    p.add_argument("--samples", type=int, default=16, help="launches sampled for the tail split (tail_by_resets)")
    p.add_argument("--dump", default=None, help="save the per-workgroup (life, S1 wait, S2 wait) us array (.npy)")
    a = p.parse_args()
    N = a.num_envs
    env = make_t1_env(num_envs=N, mesh_type="trimesh", seed=5, device="cuda:0")
    env.reset()
    acts = torch.randn(8, N, 12, device="cuda:0")
    for i in range(50):
        env.step(acts[i % 8])
    torch.cuda.synchronize()
    lib = ctypes.CDLL(os.environ["T1ENV_LIB"])
    out = np.zeros(4, np.uint64)
    lib.t1env_debug_clock6(out.ctypes.data_as(ctypes.c_void_p), 1)   # read and reset
    wg = (N + 31) // 32
    sums = np.zeros((wg, NSUM), np.uint64)
    lib.t1env_debug_wgsum6(sums.ctypes.data_as(ctypes.c_void_p), wg, 1)
    t0 = time.perf_counter()
    for i in range(a.steps):
        env.step(acts[i % 8])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    lib.t1env_debug_clock6(out.ctypes.data_as(ctypes.c_void_p), 0)
    cycles, ticks, launches = int(out[0]), int(out[1]), int(out[2])
    mhz = cycles / (ticks / 100.0) if ticks else None   # s_memrealtime: 100 MHz
    # per workgroup over the timed steps: W0's lifetime and its S1 / S2 waits (us per launch at the measured clock),
    # and by terrain type (the reference's floor(i / (N / 20)), legged_robot.py:1490) of the workgroup's first env
    lib.t1env_debug_wgsum6(sums.ctypes.data_as(ctypes.c_void_p), wg, 0)
    per = sums.astype(np.float64) / a.steps / (mhz if mhz else 2400.0)   # us per launch
    ttype = (np.arange(wg) * 32) // max(1, N // 20)
    by_type = {int(k): [round(float(per[ttype == k, j].mean()), 2) for j in range(3)] for k in np.unique(ttype)}
    mean = [round(float(x), 2) for x in per.mean(0)]
    slow = np.argsort(-per[:, 0])[:8]
    if a.dump:
        np.save(a.dump, per)
    # the last launch's timeline (us from its first workgroup's start): start spread, W0 lifetimes, last-wave ends
    tl = np.zeros((wg, 4), np.uint64)
    lib.t1env_debug_wgtime6(tl.ctypes.data_as(ctypes.c_void_p), wg)
    t0 = int(tl[:, 0].min())
    st, w0e, end, lend = ((tl[:, k].astype(np.int64) - t0) / 100.0 for k in range(4))
    # the last launch's resets per workgroup (the reset buffer after the step) against its loop / epilogue times
    rs = env.reset_buf.detach().to(torch.int32).cpu().numpy()[: wg * 32].reshape(wg, 32).sum(1)
    loop_t, epi_t = lend - st, w0e - lend
    epi_by_resets = {"0": round(float(epi_t[rs == 0].mean()), 2) if (rs == 0).any() else None,
                     ">=1": round(float(epi_t[rs > 0].mean()), 2) if (rs > 0).any() else None,
                     "wgs_with_resets": int((rs > 0).sum())}
    q = lambda v: [round(float(x), 2) for x in np.quantile(v, [0, 0.5, 0.9, 1.0])]  # noqa: E731
    tail = tail_by_resets(lib, env, acts, wg, a.samples) if hasattr(lib, "t1env_debug_tail6") else None
    print(json.dumps({"tail_by_resets": tail,"ms_per_step": round(ms, 4), "launches_x_workgroups": launches,
                      "shader_mhz": round(mhz, 1) if mhz else None,
                      "w0_lifetime_us_mean": round(ticks / max(1, launches) / 100.0, 2),
                      "last_launch_us": {"start_q0_50_90_100": q(st), "w0_life_q": q(w0e - st),
                                         "wg_end_q": q(end), "after_w0_q": q(end - w0e),
                                         "loop_q": q(loop_t), "epilogue_q": q(epi_t),
                                         "epilogue_by_resets": epi_by_resets,
                                         "slowest_end_wgs": [[int(b), round(float(loop_t[b]), 2), round(float(epi_t[b]), 2),
                                                              int(rs[b])] for b in np.argsort(-end)[:6]]},
                      "per_wg_us_life_s1wait_s2wait_q": [q(per[:, j]) for j in range(3)],
                      "w0_us_mean": {"life": mean[0], "first_s1_wait": mean[3], "s1_waits_substeps_1plus": mean[1],
                                     "s2_waits": mean[2]},
                      "first_s1_wait_q": q(per[:, 3]),
                      "shift_role_s2_to_s1_us_per_launch_mean": dict(zip(("W1", "W2", "W3", "W5", "W6", "W7"), mean[4:])),
                      "by_terrain_type_life_s1sub1plus_s2": by_type,
                      "slowest_wgs": [[int(b), [round(float(x), 2) for x in per[b]]] for b in slow],
                      "lib": os.path.basename(os.environ["T1ENV_LIB"])}))


if __name__ == "__main__":
    main()
