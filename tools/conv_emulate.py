"""Dev check: a numpy emulation of the fp16-input history conv's algebra (k_conv1d_pair_h, t1policy.hip) against an fp64
conv.  An fp16 input x is its own hi part (lo = 0), the weight is split w = w_hi + 2^-11 w_lo with w_hi = fp16(w) and
w_lo = fp16((w - w_hi) 2^11), and the kernel forms

    y = sum x w_hi + 2^-11 sum x w_lo + bias

with exact fp16 x fp16 products and fp32 accumulation (two MFMAs per K-step).  Emulated here with one fp32 rounding per
added product in the kernel's K order (channel-major, then tap) -- the matrix core adds several products per rounding,
so this is the pessimistic order.  Shows, before any GPU time, that dropping the lo.hi MFMA loses nothing.

    python tools/conv_emulate.py
"""
import numpy as np
import torch

C, L, O, K, S = 66, 47, 32, 6, 3
LOUT = (L - K) // S + 1


def emulate(x16, w, b):
    """x16 (B, C, L) float16, w (O, C, K) and b (O) float32 -> y (B, LOUT, O) float32, the kernel's arithmetic."""
    w_hi = w.astype(np.float16)
    w_lo = ((w - w_hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    xf = x16.astype(np.float32)
    acc0 = np.zeros((x16.shape[0], LOUT, O), np.float32)
    acc1 = np.zeros_like(acc0)
    for c in range(C):
        for t in range(K):
            xs = xf[:, c, t:t + S * (LOUT - 1) + 1:S][:, :, None]                 # (B, LOUT, 1)
            acc0 += xs * w_hi[None, None, :, c, t].astype(np.float32)             # fp16 x fp16: exact in fp32
            acc1 += xs * w_lo[None, None, :, c, t].astype(np.float32)
    return acc0 + acc1 * np.float32(1.0 / 2048.0) + b[None, None, :]


def emulate_error(scale=1.0, batch=777, seed=0):
    """max |emulated - fp64 conv| / (1 + |fp64 conv|) over `batch` samples of randn x 2 clamped to +-18, rounded to
    fp16, through a default-initialised Conv1d(66 -> 32, kernel 6, stride 3) with its parameters x scale."""
    torch.manual_seed(seed)
    conv = torch.nn.Conv1d(C, O, kernel_size=K, stride=S)
    w = (conv.weight.detach() * scale).contiguous()
    b = (conv.bias.detach() * scale).contiguous()
    g = torch.Generator().manual_seed(seed + 1)
    x16 = (torch.randn(batch, C, L, generator=g) * 2.0).clamp(-18, 18).half()
    ref = torch.nn.functional.conv1d(x16.double(), w.double(), b.double(), stride=S).transpose(1, 2).numpy()
    y = emulate(x16.numpy(), w.numpy(), b.numpy())
    return float((np.abs(y.astype(np.float64) - ref) / (1.0 + np.abs(ref))).max())


if __name__ == "__main__":
    for sc in (1.0, 1.5):
        print("weights x", sc, "max err / (1 + |y|):", emulate_error(sc))
