"""The fp32 update's GEMM (t1policy_gemm_nt_f32 / t1policy_gemm_f32, csrc/t1policy_gemm.hip) and weight-gradient
(t1policy_linear_wgrad_f32 / _f32x, csrc/t1policy_wgrad.hip) kernels where their dispatch changes and where their
arithmetic has corners -- needs the MI355X.

Each family has a staged-split kernel that addresses its operands through 32-bit byte offsets (operands below 1 GiB) and
a first-form kernel with 64-bit indexing that the C entry points switch to from 1 GiB on (or under T1_GEMM_STAGED=0 /
T1_WGRAD_STAGED=0, read once per process); dh_policy.gemm_nt_f32 / linear_wgrad_f32 copy a strided operand that the
staged kernel cannot take and go through the contiguous entry.

Bound (tests/test_gpu_linear_wgrad.py's, nowhere wider): every output within 2e-6 (|a| |b|^T + |bias|) of the fp64
value; for the weight gradient the scale is |gy|^T |x|, for the bias gradient sum |gy|; a second call gives the same
bits.  A CPU emulation of the six-product split summed in fp32 (K up to 768, 10 % exact zeros) stays at 6.9e-7 of that
scale for operands spread over 10^+-3 and 5.8e-7 over 10^+-6.  The fused epilogues are held to their own definitions on
the act=0 output y of the same call (the same accumulators): act=1 is ELU of y within the 2e-6 relative that elu1's
comment claims (section C pins elu1 itself) and bit-exact where y > 0; act=2 is exactly y * (aux > 0 ? 1 : aux + 1).

  A  the 1 GiB dispatch edge: one operand of 1 GiB (just above: first-form kernel or the copying fallback; just below:
     the staged kernel with its offsets at the far end), everything else small
  B  the first-form kernels at tile edges: small shapes, run in process on the staged kernels and again in a child
     pytest process under T1_GEMM_STAGED=0 T1_WGRAD_STAGED=0
  C  operand values: twelve decades of dynamic range with exact zeros, NaN containment, ELU's branch points
"""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-6
BLOCK = 65536   # rows per fp64 reference block
DUMP_ENV = "T1_GEMM_EDGES_DUMP"   # the child process of section B writes its outputs here


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _elu_deriv(aux):
    return torch.where(aux > 0, torch.ones_like(aux), aux + 1.0)


def _gemm_ref(a, b, bias):
    """fp64 a b^T + bias and its magnitude scale |a| |b|^T + |bias|, in row blocks."""
    R, N = a.shape[0], b.shape[0]
    bt = b.double().t().contiguous()
    bta = bt.abs()
    ref = torch.empty(R, N, device=DEV, dtype=torch.float64)
    mag = torch.empty(R, N, device=DEV, dtype=torch.float64)
    for r in range(0, R, BLOCK):
        ad = a[r:r + BLOCK].double()
        ref[r:r + BLOCK] = ad @ bt
        mag[r:r + BLOCK] = ad.abs() @ bta
    if bias is not None:
        ref += bias.double()
        mag += bias.double().abs()
    return ref, mag


def _within(y, ref, mag, what):
    err = (y.double() - ref).abs()
    worst = float((err / mag.clamp_min(1e-300)).max())
    print(f"{what}: worst err/mag {worst:.3e}")
    assert bool((err <= TOL * mag).all()), (what, worst)


def _gemm_outputs(a, b, bias, aux):
    """act 0, 1, 2 on the same operands, each called twice (the same bits)."""
    from ti5_isaacgym_amd.algo.dh_policy import gemm_nt_f32
    out = {}
    for act in (0, 1, 2):
        y = gemm_nt_f32(a, b, bias, act=act, aux=aux if act == 2 else None)
        assert y.shape == (a.shape[0], b.shape[0]) and y.dtype == torch.float32
        assert torch.equal(y, gemm_nt_f32(a, b, bias, act=act, aux=aux if act == 2 else None)), f"act {act}: two calls differ"
        out[act] = y
    return out


def _check_gemm(a, b, bias, aux, what):
    out = _gemm_outputs(a, b, bias, aux)
    y = out[0]
    ref, mag = _gemm_ref(a, b, bias)
    _within(y, ref, mag, what)
    # act=1: ELU of the same pre-activation; positives pass through untouched
    yd = y.double()
    elu = torch.where(yd > 0, yd, torch.expm1(yd))
    assert bool(((out[1].double() - elu).abs() <= TOL * elu.abs()).all()), (what, "act=1")
    pos = y > 0
    assert torch.equal(out[1][pos], y[pos]), (what, "act=1 positives")
    # act=2: one fp32 multiply by ELU's derivative at aux
    assert torch.equal(out[2], y * _elu_deriv(aux)), (what, "act=2")
    return out


def _wgrad_ref(gy, x):
    """fp64 gy^T x, sum gy and their magnitude scales, accumulated over row blocks."""
    M, N = gy.shape[1], x.shape[1]
    rw = torch.zeros(M, N, device=DEV, dtype=torch.float64)
    mw = torch.zeros(M, N, device=DEV, dtype=torch.float64)
    rb = torch.zeros(M, device=DEV, dtype=torch.float64)
    mb = torch.zeros(M, device=DEV, dtype=torch.float64)
    for r in range(0, gy.shape[0], BLOCK):
        gd, xd = gy[r:r + BLOCK].double(), x[r:r + BLOCK].double()
        rw += gd.t() @ xd
        mw += gd.abs().t() @ xd.abs()
        rb += gd.sum(0)
        mb += gd.abs().sum(0)
    return rw, mw, rb, mb


def _check_wgrad(gy, x, what, into=True):
    from ti5_isaacgym_amd.algo.dh_policy import linear_wgrad_f32
    M, N = gy.shape[1], x.shape[1]
    gw, gb = linear_wgrad_f32(gy, x)
    assert gw.shape == (M, N) and gb.shape == (M,) and gw.dtype == gb.dtype == torch.float32
    rw, mw, rb, mb = _wgrad_ref(gy, x)
    _within(gw, rw, mw, what + " gw")
    _within(gb, rb, mb, what + " gb")
    gw2, gb2 = linear_wgrad_f32(gy, x)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2), (what, "two calls differ")
    gw3, gb3 = linear_wgrad_f32(gy, x, need_bias=False)
    assert gb3 is None and torch.equal(gw3, gw), (what, "need_bias=False")
    if into:   # added to preset gradients by one fp32 add per element
        g = _gen(M + N)
        base_w, base_b = torch.randn(M, N, device=DEV, generator=g), torch.randn(M, device=DEV, generator=g)
        w, b = base_w.clone(), base_b.clone()
        rw_, rb_ = linear_wgrad_f32(gy, x, into=(w, b))
        assert rw_ is w and rb_ is b
        assert torch.equal(w, base_w + gw) and torch.equal(b, base_b + gb), (what, "into=")
    return gw, gb


# ---------------------------------------------------------------- A. the 1 GiB dispatch edge
# id: (R, N, K, kind); kind c: contiguous a and b; t: b the transpose of a contiguous (K, N) weight (b_kn);
# s: a the last K columns of a (R, 3102) matrix.  The 1 GiB operand is a (c, t) or the matrix a is sliced from (s).
WIDE = 3102
GEMM_EDGE = {
    "G1": (350003, 5, 767, "c"),    # 1,073,809,204 B >= 2^30: first-form kernel; ragged rows, K tail 31, N 5
    "G2": (349526, 130, 768, "c"),  # 1,073,743,872 >= 2^30: first-form kernel, two column tiles
    "G3": (349525, 130, 768, "c"),  # 1,073,740,800 <  2^30: staged kernel, offsets at the far end
    "G4": (349526, 5, 768, "t"),    # >= 2^30: refused in place, copied, first-form kernel
    "G5": (349525, 130, 768, "t"),  # <  2^30: staged in place
    "G6": (86537, 256, 235, "s"),   # 86537 * 3102 * 4 = 1,073,751,096 >= 2^30: refused in place, copied
    "G7": (86536, 256, 235, "s"),   # 1,073,738,688 < 2^30: staged in place
}


@pytest.mark.parametrize("case", sorted(GEMM_EDGE))
def test_gemm_at_the_1gib_edge(case):
    R, N, K, kind = GEMM_EDGE[case]
    g = _gen(R + N + K)
    big = None
    try:
        if kind == "s":
            big = torch.randn(R, WIDE, device=DEV, generator=g)
            a = big[:, WIDE - K:]
            assert R * WIDE * 4 >= 2 ** 30 if case == "G6" else R * WIDE * 4 < 2 ** 30
        else:
            a = torch.randn(R, K, device=DEV, generator=g)
            assert (R * K * 4 >= 2 ** 30) == (case in ("G1", "G2", "G4"))
        if kind == "t":
            b = (torch.randn(K, N, device=DEV, generator=g) * 0.1).t()
            assert b.stride() == (1, N)
        else:
            b = torch.randn(N, K, device=DEV, generator=g) * 0.1
        bias = torch.randn(N, device=DEV, generator=g)
        aux = torch.randn(R, N, device=DEV, generator=g)
        out = _check_gemm(a, b, bias, aux, case)
        if kind != "c":   # the same parts, products and k order as on contiguous copies
            out0 = _gemm_outputs(a.contiguous(), b.contiguous(), bias, aux)
            for act in (0, 1, 2):
                assert torch.equal(out[act], out0[act]), (case, act)
    finally:
        del big
        a = b = aux = out = out0 = None
        torch.cuda.empty_cache()


# id: (rows, M, N, strided x)
WGRAD_EDGE = {
    "W1": (349526, 768, 35, False),  # gy 1,073,743,872 B >= 2^30: first-form k_linear_wgrad_f32
    "W2": (349525, 768, 35, False),  # < 2^30: staged, offsets at the far end
    "W3": (86537, 256, 235, True),   # x the last 235 columns of (86537, 3102), >= 2^30: refused in place, copied
    "W4": (86536, 256, 235, True),   # < 2^30: staged in place
}


@pytest.mark.parametrize("case", sorted(WGRAD_EDGE))
def test_linear_wgrad_at_the_1gib_edge(case):
    rows, M, N, strided = WGRAD_EDGE[case]
    g = _gen(rows + M + N)
    big = None
    try:
        gy = torch.randn(rows, M, device=DEV, generator=g) * 1e-2
        if strided:
            big = torch.randn(rows, WIDE, device=DEV, generator=g)
            x = big[:, WIDE - N:]
            assert (rows * WIDE * 4 >= 2 ** 30) == (case == "W3")
        else:
            x = torch.randn(rows, N, device=DEV, generator=g)
            assert (rows * M * 4 >= 2 ** 30) == (case == "W1")
        gw, gb = _check_wgrad(gy, x, case)
        if strided:
            from ti5_isaacgym_amd.algo.dh_policy import linear_wgrad_f32
            gw0, gb0 = linear_wgrad_f32(gy, x.contiguous())
            assert torch.equal(gw, gw0) and torch.equal(gb, gb0)
    finally:
        del big
        gy = x = gw = gb = None
        torch.cuda.empty_cache()


def test_linear_on_a_slice_of_a_1gib_input():
    """dh_policy.Linear(235, 256), forward and backward, on the last 235 columns of a (86537, 3102) input that requires
    grad (1,073,751,096 B), against torch's addmm / mm on contiguous copies at the tolerances of
    test_gpu_linear_wgrad.test_linear_fp32_forward_and_input_gradient_use_the_gemm; the weight / bias gradients within
    this file's fp64 bound."""
    from ti5_isaacgym_amd.algo import dh_policy
    rows, K, N = 86537, 235, 256
    torch.manual_seed(7)
    lin = dh_policy.Linear(K, N).to(DEV)
    g = _gen(rows)
    big = torch.randn(rows, WIDE, device=DEV, generator=g).requires_grad_(True)
    gy = torch.randn(rows, N, device=DEV, generator=g) * 1e-2
    try:
        y = lin(big[:, WIDE - K:])
        y.backward(gy)
        xc = big.detach()[:, WIDE - K:].contiguous()
        torch.testing.assert_close(y.detach(), torch.addmm(lin.bias.detach(), xc, lin.weight.detach().t()),
                                   rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(big.grad[:, WIDE - K:], gy @ lin.weight.detach(), rtol=1e-5, atol=1e-6)
        assert not bool(big.grad[:, :WIDE - K].any())
        rw, mw, rb, mb = _wgrad_ref(gy, xc)
        _within(lin.weight.grad, rw, mw, "Linear gw")
        _within(lin.bias.grad, rb, mb, "Linear gb")
    finally:
        big.grad = None
        del big
        y = xc = gy = None
        torch.cuda.empty_cache()


def test_linear_backward_with_a_1gib_output_gradient():
    """dh_policy.Linear(5, 768) on 349,526 rows: the output and its gradient are 1,073,743,872 B, so the backward's
    input gradient gemm_nt_f32(gy, W^T) is refused in place (G4's path, the update's crash from about 58k envs per
    rank) and its weight gradient takes the first-form kernel (W1's).  Output, input gradient and weight / bias
    gradients within this file's fp64 bound."""
    from ti5_isaacgym_amd.algo import dh_policy
    rows, K, N = 349526, 5, 768
    torch.manual_seed(9)
    lin = dh_policy.Linear(K, N).to(DEV)
    g = _gen(rows + 1)
    x = torch.randn(rows, K, device=DEV, generator=g).requires_grad_(True)
    gy = torch.randn(rows, N, device=DEV, generator=g) * 1e-2
    try:
        y = lin(x)
        y.backward(gy)
        w, b, xd = lin.weight.detach(), lin.bias.detach(), x.detach()
        _within(y.detach(), *_gemm_ref(xd, w, b), "Linear y")
        _within(x.grad, *_gemm_ref(gy, w.t(), None), "Linear gx")
        rw, mw, rb, mb = _wgrad_ref(gy, xd)
        _within(lin.weight.grad, rw, mw, "Linear gw")
        _within(lin.bias.grad, rb, mb, "Linear gb")
    finally:
        y = gy = None
        torch.cuda.empty_cache()


def test_empty_inputs():
    """No rows: an empty (0, N) product, as addmm gave; zero weight / bias gradients; into= gradients left as they are."""
    from ti5_isaacgym_amd.algo.dh_policy import gemm_nt_f32, linear_wgrad_f32
    b = torch.randn(5, 7, device=DEV)
    bias = torch.randn(5, device=DEV)
    for act in (0, 1, 2):
        y = gemm_nt_f32(torch.empty(0, 7, device=DEV), b, bias, act=act,
                        aux=torch.empty(0, 5, device=DEV) if act == 2 else None)
        assert y.shape == (0, 5) and y.dtype == torch.float32 and y.device.type == "cuda"
    y = gemm_nt_f32(torch.empty(0, 7, device=DEV), b.t().contiguous().t())
    assert y.shape == (0, 5)
    gy, x = torch.empty(0, 5, device=DEV), torch.empty(0, 7, device=DEV)
    gw, gb = linear_wgrad_f32(gy, x)
    assert gw.shape == (5, 7) and gb.shape == (5,) and not bool(gw.any()) and not bool(gb.any())
    gw, gb = linear_wgrad_f32(gy, x, need_bias=False)
    assert gb is None and gw.shape == (5, 7) and not bool(gw.any())
    gw, gb = linear_wgrad_f32(gy, torch.empty(0, 9, device=DEV)[:, 2:])
    assert gw.shape == (5, 7) and not bool(gw.any()) and not bool(gb.any())
    pw, pb = torch.randn(5, 7, device=DEV), torch.randn(5, device=DEV)
    w, bb = pw.clone(), pb.clone()
    rw, rb = linear_wgrad_f32(gy, x, into=(w, bb))
    assert rw is w and rb is bb and torch.equal(w, pw) and torch.equal(bb, pb)


# ---------------------------------------------------------------- B. the first-form kernels at tile edges
B_GEMM = [(1, 1, 1), (31, 5, 7), (33, 65, 17), (128, 128, 32), (129, 129, 33), (200, 97, 31), (257, 130, 64),
          (64, 300, 2), (96, 64, 48), (96, 65, 48)]   # the last two: either side of the staged kernel's NARROW switch
# (rows, M, N, wide): wide > N makes x a column slice of a (rows, wide) matrix
B_WGRAD = [(31, 5, 7, 0), (33, 129, 65, 0), (256, 128, 128, 0), (257, 130, 97, 0), (3001, 1, 3, 0), (777, 219, 235, 0),
           (777, 219, 235, 240)]


def _b_gemm_operands(R, N, K, with_bias):
    g = _gen(1000 * R + 10 * N + K + int(with_bias))
    a = torch.randn(R, K, device=DEV, generator=g)
    b = torch.randn(N, K, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g) if with_bias else None
    aux = torch.randn(R, N, device=DEV, generator=g)
    return a, b, bias, aux


def _b_wgrad_operands(rows, M, N, wide):
    g = _gen(1000 * rows + 10 * M + N + wide)
    gy = torch.randn(rows, M, device=DEV, generator=g) * 1e-2
    x = torch.randn(rows, wide or N, device=DEV, generator=g)
    return gy, (x[:, wide - N:] if wide else x)


def _dump(name, tensors):
    d = os.environ.get(DUMP_ENV)
    if d:
        torch.save([t.cpu() for t in tensors], os.path.join(d, name + ".pt"))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("R,N,K", B_GEMM)
def test_b_gemm_tile_edges(R, N, K, with_bias):
    a, b, bias, aux = _b_gemm_operands(R, N, K, with_bias)
    out = _check_gemm(a, b, bias, aux, f"gemm {R} {N} {K}")
    _dump(f"gemm_{R}_{N}_{K}_{int(with_bias)}", [out[0], out[1], out[2]])


@pytest.mark.parametrize("rows,M,N,wide", B_WGRAD)
def test_b_wgrad_tile_edges(rows, M, N, wide):
    from ti5_isaacgym_amd.algo.dh_policy import linear_wgrad_f32
    gy, x = _b_wgrad_operands(rows, M, N, wide)
    gw, gb = _check_wgrad(gy, x, f"wgrad {rows} {M} {N} {wide}")
    if wide:   # the slice read in place (or, where the staged kernel is off, copied): the same bits as the copy
        gw0, gb0 = linear_wgrad_f32(gy, x.contiguous())
        assert torch.equal(gw, gw0) and torch.equal(gb, gb0)
    _dump(f"wgrad_{rows}_{M}_{N}_{wide}", [gw, gb])


def test_first_form_kernels_in_a_child_process(tmp_path):
    """Section B again with T1_GEMM_STAGED=0 T1_WGRAD_STAGED=0 (read once per process, so in a child pytest): the
    contiguous calls take k_gemm_nt_f32x3 / k_linear_wgrad_f32, the strided weight-gradient case the copying fallback of
    dh_policy.linear_wgrad_f32.  Every case must pass there, and the child's outputs must be the bits the staged kernels
    give in this process: both forms sum k ascending in 16-k steps with the same six-product order (mfma_bf3), the
    weight gradient over the same slices and reduction tree, the bias sum over the same 8-row groups -- and on the
    MI355X every output of every case of section B is bit-identical between the two forms, so that is asserted."""
    env = dict(os.environ, T1_GEMM_STAGED="0", T1_WGRAD_STAGED="0")
    env[DUMP_ENV] = str(tmp_path)
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "gpu",
           os.path.join("tests", os.path.basename(__file__)), "-k", "test_b_"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, f"first-form kernels fail section B:\n{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 2 * len(B_GEMM) + len(B_WGRAD), r.stdout[-2000:]
    assert "failed" not in r.stdout and "skipped" not in r.stdout and "error" not in r.stdout.lower()
    from ti5_isaacgym_amd.algo.dh_policy import linear_wgrad_f32
    differ = []
    for R, N, K in B_GEMM:
        for with_bias in (True, False):
            a, b, bias, aux = _b_gemm_operands(R, N, K, with_bias)
            out = _gemm_outputs(a, b, bias, aux)
            child = torch.load(os.path.join(str(tmp_path), f"gemm_{R}_{N}_{K}_{int(with_bias)}.pt"))
            differ += [("gemm", R, N, K, with_bias, act) for act in (0, 1, 2) if not torch.equal(out[act].cpu(), child[act])]
    for rows, M, N, wide in B_WGRAD:
        gy, x = _b_wgrad_operands(rows, M, N, wide)
        gw, gb = linear_wgrad_f32(gy, x)
        cw, cb = torch.load(os.path.join(str(tmp_path), f"wgrad_{rows}_{M}_{N}_{wide}.pt"))
        if not (torch.equal(gw.cpu(), cw) and torch.equal(gb.cpu(), cb)):
            differ.append(("wgrad", rows, M, N, wide))
    print("staged vs first form, cases with different bits:", differ)
    assert not differ, differ


# ---------------------------------------------------------------- C. operand values
C_SHAPES = [(130, 66, 35), (257, 129, 97)]


def _wide_range(shape, g):
    """randn * 10^U(-6, 6) per element, 10 % exact zeros, the rest inside [1e-30, 1e30] in magnitude (no part of the
    three-part split an fp32 denormal: the bound is not derived for denormal parts)."""
    v = torch.randn(shape, device=DEV, generator=g) * 10.0 ** (torch.rand(shape, device=DEV, generator=g) * 12.0 - 6.0)
    v = torch.sign(v) * v.abs().clamp(1e-30, 1e30)
    return torch.where(torch.rand(shape, device=DEV, generator=g) < 0.1, torch.zeros_like(v), v)


@pytest.mark.parametrize("R,N,K", C_SHAPES)
def test_gemm_wide_dynamic_range_and_exact_zeros(R, N, K):
    g = _gen(R + N + K)
    a, b, bias = _wide_range((R, K), g), _wide_range((N, K), g), _wide_range((N,), g)
    assert bool((a == 0).any()) and bool((b == 0).any())
    aux = torch.randn(R, N, device=DEV, generator=g)
    _check_gemm(a, b, bias, aux, f"range gemm {R} {N} {K}")
    _check_gemm(a, b.t().contiguous().t(), None, aux, f"range gemm b_kn {R} {N} {K}")


@pytest.mark.parametrize("rows,M,N", C_SHAPES)
def test_linear_wgrad_wide_dynamic_range_and_exact_zeros(rows, M, N):
    g = _gen(rows + M + N + 1)
    gy, x = _wide_range((rows, M), g), _wide_range((rows, N), g)
    _check_wgrad(gy, x, f"range wgrad {rows} {M} {N}")


def _tile_points(n):
    """An index inside a full tile / 32-block and one inside the partial last one."""
    return [min(3, n - 1), n - 1]


@pytest.mark.parametrize("R,N,K", C_SHAPES)
def test_gemm_nan_stays_in_its_row_or_column(R, N, K):
    """A NaN in a[r0, k0] makes row r0 of C NaN and leaves every other row the bits of the product with that element
    0 (adding exact zeros changes no fp32 sum); a NaN in b[n0, k0] the same by column."""
    from ti5_isaacgym_amd.algo.dh_policy import gemm_nt_f32
    g = _gen(R * N + K)
    a = torch.randn(R, K, device=DEV, generator=g)
    b = torch.randn(N, K, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g)
    for act in (0, 1):
        for k0 in _tile_points(K):
            for r0 in _tile_points(R):
                a0, an = a.clone(), a.clone()
                a0[r0, k0], an[r0, k0] = 0.0, float("nan")
                y0, yn = gemm_nt_f32(a0, b, bias, act=act), gemm_nt_f32(an, b, bias, act=act)
                assert bool(torch.isnan(yn[r0]).all()), (act, r0, k0)
                keep = torch.arange(R, device=DEV) != r0
                assert torch.equal(yn[keep], y0[keep]), (act, r0, k0)
            for n0 in _tile_points(N):
                b0, bn = b.clone(), b.clone()
                b0[n0, k0], bn[n0, k0] = 0.0, float("nan")
                for tr in (False, True):   # b as given, and as the transpose of a contiguous (K, N) matrix
                    f = (lambda t: t.t().contiguous().t()) if tr else (lambda t: t)
                    y0, yn = gemm_nt_f32(a, f(b0), bias, act=act), gemm_nt_f32(a, f(bn), bias, act=act)
                    assert bool(torch.isnan(yn[:, n0]).all()), (act, n0, k0, tr)
                    keep = torch.arange(N, device=DEV) != n0
                    assert torch.equal(yn[:, keep], y0[:, keep]), (act, n0, k0, tr)


@pytest.mark.parametrize("rows,M,N", C_SHAPES)
def test_linear_wgrad_nan_stays_in_its_row_or_column(rows, M, N):
    """A NaN in gy[r, m0]: row m0 of gw and gb[m0] NaN, the rest the bits of the gradients with that element 0; a NaN in
    x[r, n0]: column n0 of gw NaN, the rest and all of gb unchanged."""
    from ti5_isaacgym_amd.algo.dh_policy import linear_wgrad_f32
    g = _gen(rows * M + N)
    gy = torch.randn(rows, M, device=DEV, generator=g) * 1e-2
    x = torch.randn(rows, N, device=DEV, generator=g)
    for r in _tile_points(rows):
        for m0 in _tile_points(M):
            g0, gn = gy.clone(), gy.clone()
            g0[r, m0], gn[r, m0] = 0.0, float("nan")
            (w0, b0), (wn, bn) = linear_wgrad_f32(g0, x), linear_wgrad_f32(gn, x)
            assert bool(torch.isnan(wn[m0]).all()) and bool(torch.isnan(bn[m0])), (r, m0)
            keep = torch.arange(M, device=DEV) != m0
            assert torch.equal(wn[keep], w0[keep]) and torch.equal(bn[keep], b0[keep]), (r, m0)
        for n0 in _tile_points(N):
            x0, xn = x.clone(), x.clone()
            x0[r, n0], xn[r, n0] = 0.0, float("nan")
            (w0, b0), (wn, bn) = linear_wgrad_f32(gy, x0), linear_wgrad_f32(gy, xn)
            assert bool(torch.isnan(wn[:, n0]).all()), (r, n0)
            keep = torch.arange(N, device=DEV) != n0
            assert torch.equal(wn[:, keep], w0[:, keep]) and torch.equal(bn, b0), (r, n0)


def test_elu_epilogue_over_its_branch_points():
    """elu1 (the act=1 epilogue) alone: zero operands, so the pre-activation is exactly the bias -- 20,001 points on
    [-100, 5] and the branch points.  Against fp64 where(v > 0, v, expm1(v)) at 2e-6 relative (what elu1's comment
    claims); -inf gives exactly -1, nan NaN, positive inputs come back bit-exact.  Measured on the MI355X: worst
    relative error 9.1e-8."""
    from ti5_isaacgym_amd.algo.dh_policy import gemm_nt_f32
    one = torch.tensor(-1.0)
    special = torch.tensor([0.0, -0.0, -1.0, float(torch.nextafter(one, torch.tensor(0.0))),
                            float(torch.nextafter(one, torch.tensor(-2.0))), -1e-7, -1e-30, -88.0, -104.0,
                            float("-inf"), float("nan")])
    v = torch.cat([torch.linspace(-100.0, 5.0, 20001), special]).to(DEV)
    S = v.numel()
    y = gemm_nt_f32(torch.zeros(3, 1, device=DEV), torch.zeros(S, 1, device=DEV), v, act=1)
    assert y.shape == (3, S) and torch.equal(y[0, :-1], y[1, :-1]) and torch.equal(y[0, :-1], y[2, :-1])
    assert bool(torch.isnan(y[:, -1]).all())
    y = y[0]
    assert bool(torch.isnan(y[-1])) and float(y[-2]) == -1.0
    pos = v > 0
    assert torch.equal(y[pos], v[pos])
    fin = torch.isfinite(v)
    vd = v[fin].double()
    ref = torch.where(vd > 0, vd, torch.expm1(vd))
    err = (y[fin].double() - ref).abs()
    rel = err / ref.abs().clamp_min(1e-300)
    print(f"elu1 worst relative error {float(rel[ref != 0].max()):.3e}")
    assert bool((err <= TOL * ref.abs()).all()), float(rel.max())
