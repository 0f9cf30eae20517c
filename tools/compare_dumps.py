"""Dev tool: compare two `bench.py --dump-outputs DIR` directories array for array, byte for byte.

    python tools/compare_dumps.py DIR_A DIR_B

One line per .npy of either directory (name, shape, dtype, `equal bit for bit` or `DIFFERENT (<bytes that differ> bytes)`),
then `DIR_A vs DIR_B: ALL EQUAL` or `MISMATCH`; the exit status is 0 only for ALL EQUAL.  The comparison is of the raw
bytes, so a NaN equals itself and -0.0 differs from 0.0: what a change that only moves values between LDS and registers
must leave untouched.  An array that is missing on one side, or differs in shape or dtype, is a mismatch.
"""
import os
import sys

import numpy as np


def compare(dir_a, dir_b, out=sys.stdout):
    names = sorted({f for d in (dir_a, dir_b) for f in os.listdir(d) if f.endswith(".npy")})
    same = bool(names)
    for f in names:
        pa, pb = os.path.join(dir_a, f), os.path.join(dir_b, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{f:28s} missing in {dir_b if os.path.exists(pa) else dir_a}", file=out)
            same = False
            continue
        a, b = np.load(pa), np.load(pb)
        if a.shape != b.shape or a.dtype != b.dtype:
            print(f"{f:28s} {str(a.shape):16s} {str(a.dtype):8s} vs {b.shape} {b.dtype}  DIFFERENT (shape or dtype)", file=out)
            same = False
            continue
        ba = np.ascontiguousarray(a).view(np.uint8).ravel()
        bb = np.ascontiguousarray(b).view(np.uint8).ravel()
        nd = int(np.count_nonzero(ba != bb))
        print(f"{f:28s} {str(a.shape):16s} {str(a.dtype):8s} " +
              ("equal bit for bit" if nd == 0 else f"DIFFERENT ({nd} bytes)"), file=out)
        same = same and nd == 0
    print(f"{os.path.basename(os.path.normpath(dir_a))} vs {os.path.basename(os.path.normpath(dir_b))}: " +
          ("ALL EQUAL" if same else "MISMATCH"), file=out)
    return same


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(0 if compare(sys.argv[1], sys.argv[2]) else 1)
