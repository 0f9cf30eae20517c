"""Measure the value tolerance of tests/test_gpu_depth_model.py and write profiles/depth_model_parity.json.

    python tools/depth_model_parity.py [--out profiles/depth_model_parity.json]

On the CPU: tests/depth_model_ref.py in float32 against float64 on the GPU tests' inputs (the five synthetic clean images
at the four sizes, every step of the model on, frames 0 and 1), the worst absolute difference over the pixels both
measure, and the number of pixels on which the two disagree about having a measurement.  The test allows the kernel
FACTOR times that difference.  With a device: the kernel's own worst error against the float64 reference on the same
inputs, whether it equals the float32 reference to the bit, and for fp16 its worst error in fp16 ulps of the rounded
reference (else "not measured")."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
FACTOR = 8.0
FRAMES = (0, 1)


def kernel_rows():
    import torch
    import depth_model_ref as M
    rows = {}
    for w, h in M.SIZES:
        for name, dtype in (("fp32", torch.float32), ("fp16", torch.float16)):
            clean = M.to_device(M.clean_images(w, h), dtype)
            clean_np = clean.cpu().numpy()
            worst, equal, masks = 0.0, True, True
            for frame in FRAMES:
                p = M.params(**M.NOISY)
                out = M.launch(p, clean, frame).cpu().numpy()
                ref32 = M.measure(clean_np, p, frame, np.float32)
                ref64 = M.measure(clean_np, p, frame, np.float64)
                none = out.astype(np.float32) == np.float32(p["fill"])
                masks = masks and bool(np.array_equal(none, ref32["none"]))
                m = ~none & ~ref32["none"]
                want = M.stored(ref32["image"], name == "fp16")
                equal = equal and bool(np.array_equal(out[m], want[m]))
                if name == "fp16":
                    ulp = np.spacing(np.abs(want[m])).astype(np.float64)
                    worst = max(worst, float((np.abs(out[m].astype(np.float64) - want[m].astype(np.float64)) / ulp).max()))
                else:
                    m = m & ~ref64["none"]
                    worst = max(worst, float(np.abs(out[m].astype(np.float64) - ref64["image"][m]).max()))
            rows[f"{w}x{h}_{name}"] = {("max_fp16_ulps" if name == "fp16" else "max_abs_m_vs_fp64"): worst,
                                       "bit_equal_to_fp32_reference": equal, "masks_equal": masks}
    return rows


def main():
    import depth_model_ref as M
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_model_parity.json"))
    a = ap.parse_args()
    per_size, flips = {}, 0
    for w, h in M.SIZES:
        clean = M.clean_images(w, h)
        worst = 0.0
        for frame in FRAMES:
            p = M.params(**M.NOISY)
            r32, r64 = M.measure(clean, p, frame, np.float32), M.measure(clean, p, frame, np.float64)
            flips += int((r32["none"] != r64["none"]).sum())
            m = ~r32["none"] & ~r64["none"]
            worst = max(worst, float(np.abs(r32["image"][m].astype(np.float64) - r64["image"][m]).max()))
        per_size[f"{w}x{h}"] = worst
    res = {"inputs": {"envs": M.NUM_ENVS, "sizes": [list(s) for s in M.SIZES], "frames": list(FRAMES),
                      "near": M.NEAR, "far": M.FAR, "model": M.NOISY},
           "reference_fp32_vs_fp64": {"max_abs_m": max(per_size.values()), "per_size": per_size,
                                      "pixels_whose_mask_differs": flips},
           "factor": FACTOR, "test_tolerance_m": FACTOR * max(per_size.values())}
    assert res["reference_fp32_vs_fp64"]["max_abs_m"] == M.f32_vs_f64(FRAMES)
    try:
        import torch
        have = torch.cuda.is_available()
    except ImportError:
        have = False
    if have:
        res["device"] = torch.cuda.get_device_name(0)
        res["kernel"] = kernel_rows()
    else:
        res["kernel"] = "not measured"
        if os.path.exists(a.out):   # keep a device's figures when the host part is rerun without one
            with open(a.out) as f:
                old = json.load(f)
            if isinstance(old.get("kernel"), dict):
                res["kernel"], res["device"] = old["kernel"], old.get("device")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
