"""Run bench.py in two checkouts in turn, a fresh process each time, and write one tagged result line per run.

    python tools/bench_alternate.py PARENT_DIR [--rounds 3] [--steps 480] [--warmup 48] [--out FILE]

PARENT_DIR is a built checkout of the commit to compare against (e.g. `git worktree add PARENT_DIR HEAD~1`, then
`python -m ti5_isaacgym_amd.build` in it); this tree is the other arm.  Each round runs `bench.py --gpus 1 --steps K
--warmup W` in PARENT_DIR and then here.  FILE (default bench_alternate.txt) gets a line `parent {json}` or
`this_tree {json}` per run, bench.py's own result line behind the tag: what `tools/render_timing.py --bench-lines FILE`
merges into a profile as "bench_alternated" (per arm the ms_per_step of every run, their median and their spread).
A run that fails or exceeds its time limit ends the whole comparison."""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=480)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--out", default="bench_alternate.txt")
    a = ap.parse_args()
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    with open(a.out, "w") as f:
        for _ in range(a.rounds):
            for tag, where in (("parent", os.path.abspath(a.parent)), ("this_tree", REPO)):
                p = subprocess.run(cmd, cwd=where, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True,
                                   timeout=300, check=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
                f.write(tag + " " + line + "\n")
                f.flush()
                print(tag, line[:160], flush=True)


if __name__ == "__main__":
    main()
