"""Timing of the height scan (terrain.measure_heights = True) on the one-launch step path.

One process, one 8192-env trimesh env with the scan on (fp32 histories), two ways to step it, alternated `--rounds`
times, each window `--warmup` untimed and `--steps` timed steps between two device events:
  (a) the explicit split sequence through the C ABI (tests/height_scan_util.split_scan_step):
      t1env_step_physics_and_rewards -> t1env_measure_heights -> t1env_step_reset_and_observe -> t1env_critic_heights
  (b) T1DHStandEnv.step(): t1env_step (one fused launch), then t1env_height_scan.
Both give the same buffers (tests/test_gpu_height_scan.py), so the one env is stepped by either.  Then 32768 envs on a
height field with fp16 histories and the scan (no split counterpart: t1env_critic_heights is fp32 only).  For each
configuration a shorter window with the library's per-launch events on gives k_height_scan's own time (timer 4) and the
bytes it has to move (scan_bytes, from the shapes; the int16 height samples, a gather from a read-mostly field, are not
counted) over that time as a share of the 8 TB/s HBM peak.

    python tools/height_scan_timing.py [--out profiles/height_scan_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK = 8.0e12  # B/s (spec)


def scan_bytes(npts=187, half=False, npriv=73, chist=3):
    """Bytes k_height_scan reads and writes per env-step, from the shapes: the 73-wide columns of priv_buf, the two older
    heights frames of prev, the pose (7 floats), the root height and the reset flag; out and measured (fp32)."""
    es = 2 if half else 4
    read = chist * npriv * es + (chist - 1) * npts * es + 7 * 4 + 4 + 1
    written = chist * (npriv + npts) * es + npts * 4
    return read, written


def _window(step, acts, warmup, steps):
    import torch
    for i in range(warmup):
        step(acts[i % len(acts)])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        step(acts[i % len(acts)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def _scan_kernel(env, step, acts, steps, half):
    import torch
    torch.cuda.synchronize()
    env.set_timing(True)
    for i in range(steps):
        step(acts[i % len(acts)])
    torch.cuda.synchronize()
    t = env.get_timing()
    env.set_timing(False)
    k = t["k_height_scan"]
    ms = k["ms"] / k["launches"]
    rd, wr = scan_bytes(env.num_height_points, half)
    moved = (rd + wr) * env.num_envs
    return {"launches_per_step": k["launches"] / steps, "kernel_us": round(ms * 1e3, 2),
            "bytes_read_per_env": rd, "bytes_written_per_env": wr, "bytes_per_launch": moved,
            "share_of_8TBps": round(moved / (ms * 1e-3) / HBM_PEAK, 4),
            "launches": {name: v["launches"] for name, v in t.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--num-envs", type=int, default=8192)
    p.add_argument("--big-envs", type=int, default=32768)
    p.add_argument("--warmup", type=int, default=48)
    p.add_argument("--steps", type=int, default=480)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--kernel-steps", type=int, default=96)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from height_scan_util import make_scan_env, split_scan_step
    assert torch.cuda.is_available(), "height_scan_timing needs the MI355X"
    assert scan_bytes(187, False) == (876 + 1496 + 33, 3120 + 748) and scan_bytes(187, True) == (438 + 748 + 33, 1560 + 748)
    out = {"warmup": a.warmup, "steps": a.steps, "rounds": a.rounds}

    env = make_scan_env(a.num_envs, "fp32", seed=5, mesh="trimesh", small=False)
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    acts = [torch.randn(a.num_envs, 12, device="cuda:0", generator=g) for _ in range(8)]
    split = lambda act: split_scan_step(env, act)  # noqa: E731
    ms_a, ms_b = [], []
    for _ in range(a.rounds):
        ms_a.append(_window(split, acts, a.warmup, a.steps))
        ms_b.append(_window(env.step, acts, a.warmup, a.steps))
    med_a, med_b = statistics.median(ms_a), statistics.median(ms_b)
    spread_a = max(ms_a) - min(ms_a)
    out["fp32_trimesh"] = {
        "num_envs": a.num_envs, "split_ms_per_step": [round(x, 4) for x in ms_a],
        "step_ms_per_step": [round(x, 4) for x in ms_b], "split_median_ms": round(med_a, 4),
        "step_median_ms": round(med_b, 4), "split_spread_ms": round(spread_a, 4),
        "step_not_slower_beyond_spread": bool(med_b <= med_a + spread_a),
        "scan": _scan_kernel(env, env.step, acts, a.kernel_steps, False)}
    del env
    torch.cuda.empty_cache()

    env = make_scan_env(a.big_envs, "fp16", seed=5, mesh="heightfield", small=False)
    env.reset()
    acts = [torch.randn(a.big_envs, 12, device="cuda:0", generator=g) for _ in range(8)]
    ms = _window(env.step, acts, a.warmup, a.steps)
    out["fp16_heightfield"] = {"num_envs": a.big_envs, "step_ms_per_step": round(ms, 4),
                               "scan": _scan_kernel(env, env.step, acts, a.kernel_steps, True)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
