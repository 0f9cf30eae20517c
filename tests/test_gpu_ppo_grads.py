"""f1 gradients on the MI355X: the device update's .grad of every parameter tensor against fp64 autograd.

The device minibatch step is assembled unlike the reference's (one state-estimator pass whose two uses' gradients are
summed at its output, the MLPs as one _MlpF32 node with ELU' fused into the input-gradient GEMM, conv1d_train_f32,
_UnfoldRows + _LinearSplitK with t1policy_fold_rows as its backward, the estimator reading obs[:, -235:] in place, the
weight-gradient kernels adding straight into the .grad views of the flat bucket, the project's own flat-bucket clip),
and Adam hides a gradient's scale from tests/test_ppo_golden.py.  Here every eager minibatch step (graph_update =
False) is captured as in tests/test_ppo_grads.py -- the batch it was given, the weights it started from, every .grad
before and after the clip -- and held to test_ppo_grads.reference_grads, the fp64 restatement that test ties to the
reference's own update on the host.

Cases: the golden rollout (2 epochs x 4 minibatches of 192 rows) with the plain storage and with the frame-history
storage (history=(47, 66): the minibatch observations come from t1policy_history_rows; the synthetic rollout is not a
shifting history, so the rebuilt rows are other inputs than the plain ones -- the reference is recomputed from the rows
the step was given, and the recorded reference norms apply to the plain storage only); 258-row minibatches (43 envs x
24 steps in 4: two rows past the weight-gradient kernel's 256-row threshold and the 128-row tile) and one 777-row
minibatch (37 x 21), both with seeded actions and a seeded permutation.

fp32 update, per minibatch and per parameter tensor (33):
  * pre-clip gradient within K x e_host + 1e-7 relative L2 of fp64, and its 2-norm within the same bound, where e_host
    is the relative L2 error of the same loss evaluated in fp32 by torch's own layers on the host (the reference's
    arithmetic; bit-identical to the host build's gradient, test_ppo_grads) on the same batch and weights;
  * the whole gradient's norm within K x (the host's whole-gradient error) + 1e-7 of fp64's; the fused norm of the flat
    bucket (what the clip takes) within 1e-6 of the float64 norm of the same fp32 values (an fp32 tree sum of 857k
    squares: (log2 n + 3) x 2^-24 / 2);
  * the clip decision: clipped exactly when the fp64 norm + 1e-6 exceeds max_grad_norm (every case's norms are more than
    1e-4 from the threshold, asserted), and post-clip = pre-clip x the fp64 coefficient within 2e-6 relative L2;
  * golden rollout, plain storage: the reference's recorded pre-clip norms within 1e-5.

A ReLU unit of the history encoder whose fp64 pre-activation is within rounding of zero has no derivative to hold an
fp32 path to; the device and the host gradient are each compared with the nearest fp64 reference of such a unit's two
derivatives (test_ppo_grads.KINK_BAND, nearest_reference; 6-9 such units per case).

K and K16 are fixed from the first MI355X run (profiles/r13a_update_gradients.txt), as the smallest power of two at
least twice the worst factor seen, capped at 16 and 4; see them below.

bf16 update (amp_dtype=torch.bfloat16; 192- and 258-row cases): per tensor the relative L2 error to fp64 at most K16 x
that of torch's own autocast on a plain_copy of every sub-network (nn.Linear / nn.Conv1d on the device, no project
kernel), which rounds the same operands to bf16.

The graphed update needs no case of its own: test_gpu_ppo.py::test_graphed_update_matches_eager ties its Adam moments
bit for bit to the eager step pinned here.
"""
import os

import numpy as np
import pytest
import torch

from gen_ppo_golden import ALGO, N, T, synthetic_rollout
from golden_util import GOLDEN
from test_ppo_grads import (KINK_BAND, PlainPolicy, capture_update, clip_coef, fill_rollout, golden_inputs, make_alg,
                            minibatch_loss, nearest_reference, reference_grads, rel_l2, total_norm)

pytestmark = pytest.mark.gpu

# K: e_device <= K x e_host + 1e-7.  Measured over the four fp32 cases: every tensor of 64 elements or more is within 2.3
# x its host error (median 1.1 over all); the three-element state_estimator.6.bias within 6.0 x; the one-element
# critic.6.bias is one fp32 ulp off (1.25e-7, golden192_history) where the host's lands within 2.9e-9 of fp64 by chance
# (44 x) -- an error quantised in ulps, what the bound's 1e-7 floor is for -- and needs a factor 8.9 above that floor, the
# worst of all (0.86 of its bound).  Twice that is past the cap, so K is the cap.
K = 16
# K16: e_device <= K16 x e_autocast.  Measured: at most 1.54 on every tensor of more than one element (median 0.98),
# 2.32 on the one-element critic.6.bias (ragged258); twice that is past the cap, so K16 is the cap.
K16 = 4

CASES = {"golden192": dict(n=N, t=T, mbs=4, history=None),
         "golden192_history": dict(n=N, t=T, mbs=4, history=(47, 66)),
         "ragged258": dict(n=43, t=24, mbs=4, history=None, seed=21),
         "ragged777": dict(n=37, t=21, mbs=1, history=None, seed=22)}
_INPUTS, REPORT = {}, []


def case_inputs(name):
    """(rollout, actions, permutation) of a case, made once."""
    if name not in _INPUTS:
        c = CASES[name]
        if name.startswith("golden"):
            _INPUTS[name] = golden_inputs()
        else:
            g = torch.Generator().manual_seed(c["seed"])
            actions = torch.randn(c["t"], c["n"], 12, generator=g)
            _INPUTS[name] = (synthetic_rollout(c["n"], c["t"], seed=c["seed"]), actions,
                             torch.randperm(c["n"] * c["t"], generator=g))
    return _INPUTS[name]


@pytest.fixture(scope="module", autouse=True)
def report():
    """$T1_GRAD_REPORT=path: the measured per-tensor worst errors and ratios of this session."""
    yield
    path = os.environ.get("T1_GRAD_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("\n".join(REPORT) + "\n")


def run_case(name, monkeypatch, **kw):
    c = CASES[name]
    rollout, actions, perm = case_inputs(name)
    algo = dict(ALGO, num_mini_batches=c["mbs"])
    alg = make_alg("cuda:0", c["n"], c["t"], algo=algo, history=c["history"], **kw)
    fill_rollout(alg, rollout, actions, "cuda:0")
    monkeypatch.setattr(torch, "randperm", lambda n, **k: perm.to(k.get("device", "cpu")))
    records = capture_update(alg)
    assert len(records) == algo["num_learning_epochs"] * c["mbs"]
    return alg, algo, records, rollout, perm


class Checks:
    """Every check of a case measured before any of them fails the test: name -> the worst value / bound seen."""

    def __init__(self):
        self.margin, self.failed = {}, []

    def __call__(self, name, value, bound, *info):
        r = value / bound if bound > 0 else (0.0 if value == 0 else float("inf"))
        if r > self.margin.get(name, (-1.0,))[0]:
            self.margin[name] = (r, value, bound, info)
        if not value <= bound:
            self.failed.append((name, value, bound, *info))

    def is_true(self, name, ok, *info):
        self(name, 0.0 if ok else 1.0, 0.5, *info)


def log(case, mode, worst, yard, checks, extra=()):
    REPORT.append(f"{case} ({mode}): per tensor the worst relative L2 error to fp64 over the minibatches and the {yard} "
                  "error there; the worst ratio of the two; the worst factor the bound needs; the worst error / bound")
    for k, (e, eh, r, f, b) in worst.items():
        REPORT.append(f"  {k:32s} {e:9.2e} {eh:9.2e} {r:6.2f} {f:6.2f} {b:6.3f}")
    top = max(worst.items(), key=lambda kv: kv[1][3])
    REPORT.append(f"  worst factor needed {top[1][3]:.2f} ({top[0]})")
    REPORT.extend(f"  {x}" for x in extra)
    REPORT.append("  checks, worst value / bound: " + "; ".join(
        f"{k} {v[0]:.3g}" + (f" ({v[3][0]} [{v[3][1]}])" if len(v[3]) > 1 else "") for k, v in checks.margin.items()))
    print("\n".join(REPORT[-len(worst) - 3 - len(extra):]))


def track(worst, k, e, eh, bound, floor=0.0):
    """Per tensor: the error pair of the worst ratio, that ratio, the worst factor the bound would need (the error above
    the bound's additive floor over the yardstick's) and the worst error / bound."""
    w = worst.get(k, (0.0, 0.0, -1.0, 0.0, 0.0))
    w = (e, eh, e / eh) + w[3:] if e / eh > w[2] else w
    worst[k] = w[:3] + (max(w[3], max(0.0, e - floor) / eh), max(w[4], e / bound))


@pytest.mark.parametrize("case", sorted(CASES))
def test_fp32_update_gradients_match_fp64(case, monkeypatch):
    alg, algo, records, _, _ = run_case(case, monkeypatch)
    max_norm = algo["max_grad_norm"]
    fx_norms = np.load(f"{GOLDEN}/ppo_grads.npz")["pre_norm"] if case == "golden192" else None
    worst, check, clipped, n_kinks = {}, Checks(), [], 0
    for mb, rec in enumerate(records):
        assert rec["batch"][0].dtype == torch.float32 and rec["batch"][0].shape[0] == CASES[case]["n"] * \
            CASES[case]["t"] // CASES[case]["mbs"]
        kinks = []
        g64 = reference_grads(rec["weights"], rec["batch"], algo, kinks=kinks)
        g32 = reference_grads(rec["weights"], rec["batch"], algo, dtype=torch.float32)
        assert list(g64) == list(rec["pre"]) and len(g64) == 33
        # a ReLU unit within rounding of zero (test_ppo_grads.KINK_BAND): each path against the fp64 reference nearest it
        g64_host, g64 = nearest_reference(g32, g64, kinks), nearest_reference(rec["pre"], g64, kinks)
        n_kinks += len(kinks)
        for k, g in rec["pre"].items():
            e, eh = rel_l2(g, g64[k]), rel_l2(g32[k], g64_host[k])
            track(worst, k, e, eh, K * eh + 1e-7, floor=1e-7)
            check("gradient", e, K * eh + 1e-7, k, mb)
            n = g64[k].norm().item()
            check("tensor norm", abs(g.double().norm().item() - n) / n, K * eh + 1e-7, k, mb)
        # the whole gradient: the device's own float64 norm, the fused fp32 norm the clip takes, fp64's
        n64, n_dev = total_norm(g64), total_norm(rec["pre"])
        eh_all = rel_l2(torch.cat([g32[k].reshape(-1) for k in g64]), torch.cat([g64_host[k].reshape(-1) for k in g64]))
        check("total norm", abs(n_dev - n64) / n64, K * eh_all + 1e-7, "all", mb)
        check("fused norm", abs(rec["fused_norm"] - n_dev) / n_dev, 1e-6, "all", mb)
        if fx_norms is not None:
            check("recorded norm", abs(n_dev - fx_norms[mb]) / fx_norms[mb], 1e-5, "all", mb)
        # the clip: its decision and its coefficient, both fp64's
        assert abs(n64 - max_norm) > 1e-4, (mb, n64)
        coef = clip_coef(n64, max_norm)
        clipped.append(coef < 1.0)
        for k, g in rec["pre"].items():
            check.is_true("clip decision", torch.equal(rec["post"][k], g) == (coef == 1.0), k, mb)
            check("clip coefficient", rel_l2(rec["post"][k], g.double() * coef), 2e-6, k, mb)
    which = [i for i, c in enumerate(clipped) if c]
    log(case, "fp32 update", worst, "host fp32", check,
        [f"clipped minibatches {which} of {len(clipped)}; {n_kinks} ReLU units within {KINK_BAND:g} of zero"])
    assert not check.failed, check.failed[:8]
    if case == "golden192":
        assert which == [1, 2, 3, 7]


def autocast_grads(ac, weights, batch, algo):
    """The yardstick of the bf16 update: the same loss through torch's own bf16 autocast on plain torch copies of the
    sub-networks, on the device."""
    from ti5_isaacgym_amd.algo.dh_policy import plain_copy
    p = PlainPolicy(nets=[plain_copy(getattr(ac, n)) for n in ("actor", "critic", "long_history", "state_estimator")])
    p.to("cuda:0")
    p.load_state_dict(weights)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        loss = minibatch_loss(p, batch, algo)
    loss.backward()
    return {k: v.grad.detach() for k, v in p.named_parameters()}


@pytest.mark.parametrize("case", ["golden192", "ragged258"])
def test_bf16_update_gradients_match_autocast(case, monkeypatch):
    alg, algo, records, rollout, perm = run_case(case, monkeypatch, amp_dtype=torch.bfloat16)
    c = CASES[case]
    rows = c["n"] * c["t"] // c["mbs"]
    obs = rollout[0][:c["t"]].flatten(0, 1)
    worst, check = {}, Checks()
    for mb, rec in enumerate(records):
        # the step was given the observations cast once to bf16: the references take the fp32 rows they were cast from
        i = mb % c["mbs"]
        obs32 = obs[perm[i * rows:(i + 1) * rows]]
        assert rec["batch"][0].dtype == torch.bfloat16 and torch.equal(rec["batch"][0].cpu(), obs32.to(torch.bfloat16))
        batch = [obs32] + rec["batch"][1:]
        g64 = reference_grads(rec["weights"], batch, algo)
        gy = autocast_grads(alg.actor_critic, rec["weights"], [x.to("cuda:0") for x in batch], algo)
        for k, g in rec["pre"].items():
            e, ey = rel_l2(g, g64[k]), rel_l2(gy[k], g64[k])
            track(worst, k, e, ey, K16 * ey)
            check("gradient", e, K16 * ey, k, mb)
        # the clip on the bf16 update's own gradients (their norm is percents from fp64's: no decision against it)
        coef = clip_coef(total_norm(rec["pre"]), algo["max_grad_norm"])
        for k, g in rec["pre"].items():
            check("clip coefficient", rel_l2(rec["post"][k], g.double() * coef), 2e-6, k, mb)
    log(case, "bf16 update", worst, "autocast yardstick's", check)
    assert not check.failed, check.failed[:8]
