"""Dev probe: static instruction counts of a step kernel between its phase marks (a -DT1_ASM_MARKS device build turns
every T1_PROF_MARK into an assembly comment).  Counts follow the code layout: a region is the code from a mark to the
next mark in the listing, so it is exact for straight-line phases and indicative where branches interleave.

    python tools/isa_phases.py [--unit dyn5|dyn6|PATH.hip] [--opt -O1] [--kernel-index 0] [--mem]
                                [--skeleton MARK] [--listing PATH.s] [extra hipcc flags]

--mem prints, per region, the memory round trips the wave waits out instead of the instruction mix: its global loads
and stores, the `s_waitcnt vmcnt` waits that have a global load pending (each one is a memory latency the wave sits
through; a prologue that loads everything first has one), the scratch reloads (they count in vmcnt, so each drains
every load before it) and the vmcnt waits that follow the region's first global store (the history shift's store
drain).  A mark is named <id>@L<source line>; k_dyn6's marks 20 / 21 are the role entries of W4 / the term roles, 22
the end of the term roles' epilogue staging, 3 -> 4 a shift role's S2 -> S1 tail.  --skeleton MARK prints the memory
instructions, waits, barriers and branches of the regions after that mark; --listing keeps the assembly (and reads
it back on the next call instead of compiling).
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ti5_isaacgym_amd", "csrc")


def listing(unit, opt, extra, keep=None):
    """the unit's device assembly; keep: a path to read it from if it exists, and to write it to if not"""
    if keep and os.path.exists(keep):
        return open(keep).read().split("\n")
    src = unit if unit.endswith(".hip") else os.path.join(CSRC, f"t1env_{unit}.hip")
    out = keep or os.path.join(tempfile.gettempdir(), f"isa_phases_{os.getpid()}.s")
    subprocess.run(["/opt/rocm/bin/hipcc", opt, "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize",
                    "--cuda-device-only", "-S", "-DT1_ASM_MARKS", "-I", os.path.join(REPO, "include"), "-I", CSRC,
                    *extra, "-o", out, src], check=True)
    return open(out).read().split("\n")


def kernel_lines(s, ki):
    starts = [k for k, l in enumerate(s) if re.match(r"^_Z\w+:", l)]
    ends = [k for k, l in enumerate(s) if l.startswith(".Lfunc_end")]
    i = starts[ki]
    j = [e for e in ends if e > i][0]
    return s[i].split(":")[0], s[i:j]


def regions(lines):
    """(mark name, [instruction text]) per region, in listing order"""
    cur, body, out = "entry", [], []
    for l in lines:
        t = l.strip()
        m = re.search(r";@@MARK (\S+)", t)
        if m:
            out.append((cur, body))
            cur, body = m.group(1), []
            continue
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        body.append(t)
    out.append((cur, body))
    return out


def mix(body):
    c = collections.Counter()
    for t in body:
        op = t.split()[0]
        cat = ("acc" if op.startswith("v_accvgpr") else "lane" if op.startswith(("v_readlane", "v_writelane"))
               else "valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else
               "smem" if op.startswith(("s_load", "s_buffer")) else "wait" if op == "s_waitcnt" else
               "vmem" if op.startswith(("global_", "buffer_", "flat_", "scratch_")) else "salu")
        c[cat] += 1
    return c


def mem(body):
    """global loads, global stores, vmcnt waits with a global load pending, scratch reloads, vmcnt waits after the
    first global store"""
    loads = stores = trips = reloads = after_store = pending = 0
    for t in body:
        op = t.split()[0]
        if op.startswith(("global_load", "global_atomic")):
            loads += 1
            pending += 1
        elif op.startswith("global_store"):
            stores += 1
        elif op.startswith("scratch_load"):
            reloads += 1
        elif op == "s_waitcnt" and "vmcnt" in t:
            trips += 1 if pending else 0
            after_store += 1 if stores else 0
            pending = 0
    return loads, stores, trips, reloads, after_store


def print_skeleton(lines, mark):
    """the memory instructions, waits, barriers, labels and branches of the regions after `mark`, the rest counted"""
    on, run = False, 0
    for l in lines:
        t = l.strip()
        m = re.search(r";@@MARK (\S+)", t)
        if m:
            if run:
                print(f"   ... {run} other")
            on, run = m.group(1).split("@")[0] == mark, 0
            if on:
                print(t)
            continue
        if not on or not t or t.startswith(";") or (t.startswith(".") and not t.endswith(":")):
            continue
        op = t.split()[0]
        if t.endswith(":") or op.startswith(("global_", "buffer_", "flat_", "scratch_", "ds_", "s_waitcnt", "s_barrier",
                                             "s_cbranch", "s_branch")):
            if run:
                print(f"   ... {run} other")
            run = 0
            print("  " + t[:100])
        else:
            run += 1


def main():
    args = sys.argv[1:]
    ki, unit, opt, want_mem, skeleton, keep = 0, "dyn5", "-O1", False, None, None
    while args and args[0] in ("--kernel-index", "--unit", "--opt", "--mem", "--skeleton", "--listing"):
        if args[0] == "--mem":
            want_mem, args = True, args[1:]
            continue
        key, val, args = args[0], args[1], args[2:]
        if key == "--kernel-index":
            ki = int(val)
        elif key == "--unit":
            unit = val
        elif key == "--skeleton":
            skeleton = val
        elif key == "--listing":
            keep = val
        else:
            opt = val
    name, lines = kernel_lines(listing(unit, opt, args, keep), ki)
    print(name[:60], opt)
    if skeleton:
        print_skeleton(lines, skeleton)
        return
    for mark, body in regions(lines):
        if not body:
            continue
        if want_mem:
            ld, st, trips, reloads, after = mem(body)
            if ld or st or reloads:
                print(f"after mark {mark:>9s}: total {len(body):6d}  global loads {ld:3d}  stores {st:3d}  "
                      f"vmcnt waits with a load pending {trips:3d}  scratch reloads {reloads:3d}  "
                      f"vmcnt waits after the first store {after:3d}")
        else:
            c = mix(body)
            print(f"after mark {mark:>9s}: total {len(body):6d}  " +
                  "  ".join(f"{k} {c[k]}" for k in ("valu", "salu", "lds", "smem", "vmem", "wait", "acc", "lane")))


if __name__ == "__main__":
    main()
