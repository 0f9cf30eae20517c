"""Dev probe: static instruction counts of a step kernel between its phase marks (a -DT1_ASM_MARKS device build turns
every T1_PROF_MARK into an assembly comment).  Counts follow the code layout: a region is the code from a mark to the
next mark in the listing, so it is exact for straight-line phases and indicative where branches interleave.

    python tools/isa_phases.py [--unit dyn5|dyn6|PATH.hip] [--opt -O1] [--kernel-index 0] [--mem]
                                [--skeleton MARK] [--listing PATH.s] [--barriers [--near 6]] [extra hipcc flags]

--barriers reads the product's code instead: the listing of a build WITHOUT the marks (their operands cost registers:
the marked k_dyn6 spills 35 VGPRs where the product spills none), cut at its `s_barrier`s and loop edges.  Per region it
prints the instruction mix, the LDS opcode histogram, and for every `s_waitcnt lgkmcnt(N)` with an LDS read pending the
number of VALU instructions issued since the last LDS read (`valu:N`; --near: what counts as directly behind the read).
A wait a few VALU instructions behind its read exposes the whole LDS latency on a wave that runs alone on its SIMD.

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


def listing(unit, opt, extra, keep=None, marks=True):
    """the unit's device assembly; keep: a path to read it from if it exists, and to write it to if not; marks: the
    -DT1_ASM_MARKS build (False: the product's code, which the marks' operands and comments do not perturb)"""
    if keep and os.path.exists(keep):
        return open(keep).read().split("\n")
    src = unit if unit.endswith(".hip") else os.path.join(CSRC, f"t1env_{unit}.hip")
    out = keep or os.path.join(tempfile.gettempdir(), f"isa_phases_{os.getpid()}.s")
    subprocess.run(["/opt/rocm/bin/hipcc", opt, "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize",
                    "--cuda-device-only", "-S", *(["-DT1_ASM_MARKS"] if marks else []), "-I", os.path.join(REPO, "include"), "-I", CSRC,
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


def barrier_regions(lines):
    """The unmarked listing cut at its `s_barrier`s and at the edges of its outermost loops: [(loop header or None,
    segment index within that stretch, first listing line, [instruction text])].  The compiler's block comments
    (`in Loop: Header=BB0_60 Depth=1`, `Parent Loop BB0_60 Depth=1`, `=>This Loop Header: Depth=1`) say which loop a
    block belongs to; a block without one is outside every loop."""
    out, loop, seg, body, first = [], None, 0, [], 0

    def close(k):
        nonlocal body, first
        if body:
            out.append((loop, seg, first, body))
        body, first = [], k

    for k, l in enumerate(lines):
        t = l.strip()
        is_block = re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", t)
        if is_block:
            new = loop
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", t)
            if re.search(r"=>This (Inner )?Loop Header: Depth=1\b", t):
                new = t.split(":")[0].lstrip(".L")
            elif m and m.group(2) == "1":
                new = m.group(1)
            elif m or "Loop Header: Depth=" in t:
                pass  # an inner block: its `Parent Loop ... Depth=1` comment follows; the outer loop stays
            else:
                new = None
            if new != loop:
                close(k)
                loop, seg = new, 0
            continue
        m = re.search(r"Parent Loop (BB\d+_\d+) Depth=1\b", t)
        if m and m.group(1) != loop:
            close(k)
            loop, seg = m.group(1), 0
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        if t.split()[0] == "s_barrier":
            close(k)
            seg += 1
            continue
        if not body:
            first = k
        body.append(t)
    close(len(lines))
    return out


def lgkm_waits(body):
    """[(VALU instructions since the last LDS read, the wait's lgkmcnt)] of the `s_waitcnt lgkmcnt(N)` that have an LDS
    read pending (issued since the last lgkmcnt(0))"""
    out, since, pending = [], 0, False
    for t in body:
        op = t.split()[0]
        if op.startswith("ds_read") or op.startswith("ds_bpermute") or op.startswith("ds_swizzle"):
            since, pending = 0, True
        elif op.startswith("v_") and not op.startswith("v_accvgpr"):
            since += 1
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", t)
            if m and pending:
                out.append((since, int(m.group(1))))
                pending = int(m.group(1)) != 0
    return out


def print_barrier_regions(lines, near):
    """Per region between barriers: the instruction mix, the LDS opcode histogram and, per lgkmcnt wait, the VALU
    instructions since the last LDS read (`valu:lgkmcnt`).  A loop's last segment and its first (from the header to the
    first barrier) are one region at run time: the wrap-around is printed as such.  In k_dyn6 the roles' substep loops
    follow each other in the listing (W4, W1, W5, the terrain halves, W0): the core wave's is the last loop with two
    barriers, its S1 -> S2 region segment 1 and its S2 -> S1 region the wrap-around."""
    regs = barrier_regions(lines)
    loops = collections.OrderedDict()
    for loop, seg, first, body in regs:
        loops.setdefault((loop, first if loop is None else None), []).append((seg, first, body))
    two = [k for k, v in loops.items() if k[0] is not None and max(s for s, _, _ in v) >= 2]
    for key, segs in loops.items():
        loop = key[0]
        merged = {}
        for seg, first, body in segs:  # a segment split by an inner loop's blocks: one region
            merged.setdefault(seg, [first, []])[1].extend(body)
        nseg = max(merged) if merged else 0
        rows = []
        if loop is not None and nseg >= 1:
            for seg in range(1, nseg):
                if seg in merged:
                    rows.append((f"barrier {seg} -> {seg + 1}", merged[seg][0], merged[seg][1]))
            wrap = merged.get(nseg, [0, []])[1] + merged.get(0, [0, []])[1]
            rows.append((f"barrier {nseg} -> 1 (wraps)", merged.get(nseg, merged[min(merged)])[0], wrap))
        else:
            for seg in sorted(merged):
                rows.append((f"segment {seg}", merged[seg][0], merged[seg][1]))
        tag = f"loop {loop}" + ("  [the last two-barrier loop: the core wave's]" if two and key == two[-1] else "") \
            if loop else "outside loops"
        for name, first, body in rows:
            if len(body) < 8:
                continue
            c = mix(body)
            print(f"{tag}, {name}, listing line {first + 1}: total {len(body)}  " +
                  "  ".join(f"{k} {c[k]}" for k in ("valu", "salu", "lds", "smem", "vmem", "wait")))
            h = collections.Counter(t.split()[0] for t in body if t.startswith("ds_"))
            if h:
                print("    lds: " + "  ".join(f"{k} {v}" for k, v in sorted(h.items())))
            fp = collections.Counter()
            for t in body:  # the arithmetic a data-movement change must leave as it was: f32 opcodes, encoding suffix off
                op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", t.split()[0])
                if op.startswith("v_permlane") or re.match(r"v_(pk_)?\w*f32$", op) and not op.startswith("v_cvt"):
                    fp["v_fma_f32+v_fmac_f32" if op in ("v_fma_f32", "v_fmac_f32") else op] += 1
            if fp:
                print("    f32: " + "  ".join(f"{k} {v}" for k, v in sorted(fp.items())))
            w = lgkm_waits(body)
            if w:
                close = sum(1 for v, _ in w if v <= near)
                print(f"    lgkmcnt waits with a read pending: {len(w)}, within {near} VALU of the last read: {close}")
                print("    valu:lgkmcnt  " + " ".join(f"{v}:{n}" for v, n in w))


def main():
    args = sys.argv[1:]
    ki, unit, opt, want_mem, skeleton, keep, barriers, near = 0, "dyn5", "-O1", False, None, None, False, 6
    while args and args[0] in ("--kernel-index", "--unit", "--opt", "--mem", "--skeleton", "--listing", "--barriers",
                               "--near"):
        if args[0] == "--mem":
            want_mem, args = True, args[1:]
            continue
        if args[0] == "--barriers":
            barriers, args = True, args[1:]
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
        elif key == "--near":
            near = int(val)
        else:
            opt = val
    name, lines = kernel_lines(listing(unit, opt, args, keep, marks=not barriers), ki)
    print(name[:60], opt)
    if barriers:
        print_barrier_regions(lines, near)
        return
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
