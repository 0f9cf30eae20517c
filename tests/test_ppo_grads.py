"""f1 gradients: what DHPPO.update hands to the clip and to Adam, against the reference's own update and fp64 autograd.

tests/test_ppo_golden.py sees the update only through Adam, whose first steps move every weight by about +-lr whatever
the gradient's size: a wrong uniform scale on a gradient, or a clip that does nothing, passes it.  Here the gradients
themselves are read, before and after the clip, for every one of the 2 x 4 minibatches of the golden rollout:

  (a) the host build's .grad tensors against tests/golden/ppo_grads.npz, recorded from the reference's DHPPO.update
      (tests/golden/gen_ppo_grads.py): per tensor the float64 sum, 2-norm, 64 probed elements and every tensor of at most
      4096 elements in full, before and after the clip, and the total pre-clip norm, all at 1e-6 relative (a sum
      relative to sqrt(numel x sum of squares), the scale of its terms).  Measured here: the probed and full tensors
      equal bit for bit, the float64 reductions within 1.9e-14;
  (b) reference_grads -- an fp64 restatement of the reference's minibatch loss (dh_ppo.py:123-175) on a policy of plain
      torch layers, plain autograd, sharing nothing with DHPPO._losses_body -- within 1e-5 relative L2 of the host
      gradient for every tensor (measured: worst 2.41e-6, actor.6.bias of minibatch 6; median 6.6e-7);
  (c) post-clip = pre-clip x min(1, max_grad_norm / (norm + 1e-6)) with the fp64 norm (2e-6 relative L2 per tensor: the
      fp32 coefficient and one rounding of each product; measured 5.8e-7);
  (d) exactly the minibatches 1, 2, 3 and 7 clip.

(a) ties the host build to the reference, (b) ties the restatement to both, so tests/test_gpu_ppo_grads.py can hold the
device update's gradients to reference_grads alone.  The same restatement in fp32 (the reference's layers and torch's
Normal on the CPU: the yardstick e_host of the device test) is held to the host gradient at 1e-5 too (measured: equal bit
for bit).  A ReLU unit whose fp64 pre-activation is within rounding of zero has two defensible derivatives: (b) holds a
gradient to the nearest of the fp64 references they give (KINK_BAND below).

The capture replaces two instance attributes of the DHPPO under test (_minibatch_step, to clone the batch and the
weights it starts from; _clip_grads, to read every .grad before and after it); the product code is not changed.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from gen_ppo_golden import ALGO, N, POLICY, POLICY_SEED, T, synthetic_rollout
from gen_ppo_grads import FULL_NUMEL, probe_index64
from golden_util import GOLDEN


# ---------------------------------------------------------------------------------------------- the fp64 restatement
def _plain_mlp(sizes):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(nn.ELU())
    return nn.Sequential(*layers)


# A ReLU pre-activation within rounding of zero has no derivative an fp32 evaluation could be held to: measured on the
# host, an fp32 pre-activation of the first conv is up to 4.3e-7 from its fp64 value and one unit in a few hundred
# thousand changes sign, which moves that conv's gradient by 4e-4 relative L2.  Units within KINK_BAND (4 x that error)
# of zero in fp64 are reported with the change their other derivative makes (reference_grads' kinks), and a gradient
# under test is held to the nearest of those references (nearest_reference).  The forward value is the same either way.
KINK_BAND = 2e-6
MAX_KINKS = 10


class _MaskedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, mask):
        ctx.save_for_backward(mask)
        return z.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


class KinkReLU(nn.Module):
    """ReLU that keeps its last pre-activations and takes the other derivative at the flat positions in flip."""

    def __init__(self):
        super().__init__()
        self.flip, self.z = None, None

    def forward(self, z):
        self.z = z.detach()
        mask = self.z > 0
        if self.flip is not None:
            mask.view(-1)[self.flip] ^= True
        return _MaskedReLU.apply(z, mask)


class PlainPolicy(nn.Module):
    """The t1 policy's four networks and std from plain torch layers (actor_critic_dh.py:45-111), parameter names as the
    reference's.  nets: ready-made sub-networks instead (the device test's autocast yardstick)."""

    def __init__(self, policy=POLICY, short=235, frame=47, critic_obs=219, actions=12, nets=None):
        super().__init__()
        self.short, self.frame, self.frames = short, frame, policy["in_channels"]
        self.std = nn.Parameter(torch.ones(actions))
        if nets is not None:
            self.actor, self.critic, self.long_history, self.state_estimator = nets
            return
        code = policy["lh_output_dim"]
        self.actor = _plain_mlp([short + 3 + code, *policy["actor_hidden_dims"], actions])
        self.critic = _plain_mlp([critic_obs, *policy["critic_hidden_dims"], 1])
        layers, ch, length = [], self.frames, frame
        for o, k, s in zip(policy["filter_size"], policy["kernel_size"], policy["stride_size"]):
            layers += [nn.Conv1d(ch, o, kernel_size=k, stride=s), KinkReLU()]
            ch, length = o, (length - k) // s + 1
        self.long_history = nn.Sequential(*layers, nn.Flatten(), nn.Linear(ch * length, 128), nn.ELU(),
                                          nn.Linear(128, code))
        self.state_estimator = _plain_mlp([short, *policy["state_estimator_hidden_dims"], 3])


def minibatch_loss(p, batch, algo):
    """The reference's minibatch loss (dh_ppo.py:123-175) on a PlainPolicy, in the dtype of p.std: the sub-networks are
    called directly (the product's update_distribution / evaluate end in .float()), the state estimator twice as there."""
    obs, cobs, actions, target_values, adv, returns, old_logp = batch[:7]
    dt = p.std.dtype
    short = obs[:, -p.short:]
    code = p.long_history(obs.reshape(-1, p.frames, p.frame))
    mean = p.actor(torch.cat((short, p.state_estimator(short).to(short.dtype), code.to(short.dtype)), dim=-1)).to(dt)
    dist = torch.distributions.Normal(mean, mean * 0.0 + p.std, validate_args=False)
    est = p.state_estimator(short).to(dt)
    target_vel = cobs[:, algo["lin_vel_idx"]:algo["lin_vel_idx"] + 3].to(dt)
    logp = dist.log_prob(actions.to(dt)).sum(-1)
    value = p.critic(cobs).to(dt)
    entropy = dist.entropy().sum(-1)
    clip = algo["clip_param"]
    ratio = torch.exp(logp - old_logp.to(dt).squeeze(-1))
    a = adv.to(dt).squeeze(-1)
    surrogate = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    tv, ret = target_values.to(dt), returns.to(dt)
    if algo["use_clipped_value_loss"]:
        v_clip = tv + (value - tv).clamp(-clip, clip)
        value_loss = torch.max((value - ret).pow(2), (v_clip - ret).pow(2)).mean()
    else:
        value_loss = (ret - value).pow(2).mean()
    return (surrogate + algo["value_loss_coef"] * value_loss - algo["entropy_coef"] * entropy.mean()
            + (est - target_vel).pow(2).mean())


def reference_grads(state_dict, batch, algo, dtype=torch.float64, kinks=None):
    """{name: d loss / d parameter} of the reference's minibatch loss for the weights state_dict and the minibatch tuple
    batch (mini_batch_generator's), by plain autograd on the CPU in dtype (fp64: the reference; fp32: the reference's own
    arithmetic, whose distance to fp64 is the device test's yardstick).  kinks: a list that receives, for every ReLU unit
    whose pre-activation is within KINK_BAND of zero, {name: the change of the gradient with that unit's other
    derivative}."""
    p = PlainPolicy().to(dtype)
    p.load_state_dict({k: v.detach().to("cpu", dtype) for k, v in state_dict.items()})
    b = [x.detach().to("cpu", dtype) for x in batch[:9]]

    def grads():
        p.zero_grad(set_to_none=True)
        minibatch_loss(p, b, algo).backward()
        return {k: v.grad.detach() for k, v in p.named_parameters()}

    base = grads()
    if kinks is not None:
        relus = [m for m in p.long_history if isinstance(m, KinkReLU)]
        units = [(m, i) for m in relus for i in (m.z.abs().reshape(-1) < KINK_BAND).nonzero().reshape(-1)]
        assert len(units) <= MAX_KINKS, len(units)
        for m, i in units:
            m.flip = i.reshape(1)
            other = grads()
            m.flip = None
            kinks.append({k: other[k] - base[k] for k in base if not torch.equal(other[k], base[k])})
    return base


def nearest_reference(got, ref, kinks):
    """The reference among ref + any subset of the kink changes that is nearest to the gradients got (the sum over the
    tensors of the squared relative L2 distance); ref itself without kinks."""
    best, best_d = ref, None
    if not kinks:
        return ref
    for bits in range(2 ** len(kinks)):
        cand = dict(ref)
        for j, d in enumerate(kinks):
            if bits >> j & 1:
                for k, v in d.items():
                    cand[k] = cand[k] + v
        dist = sum(rel_l2(got[k], cand[k]) ** 2 for k in {k for d in kinks for k in d})
        if best_d is None or dist < best_d:
            best, best_d = cand, dist
    return best


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return ((got - ref).norm() / ref.norm()).item()


def total_norm(grads):
    return math.sqrt(sum(g.detach().double().pow(2).sum().item() for g in grads.values()))


# ------------------------------------------------------------------------------------------------------- the capture
def fill_rollout(alg, rollout, actions, device):
    """The rollout through the storage with the given actions (test_ppo_golden.replay's loop), then the returns."""
    ac = alg.actor_critic
    obs, cobs, rew, dones, tout = (x.to(device) for x in rollout)
    with torch.no_grad():
        for t in range(rew.shape[0]):
            tr = alg.transition
            a = actions[t].to(device)
            ac.act(obs[t])
            tr.actions = a
            tr.values = ac.evaluate(cobs[t])
            tr.actions_log_prob = ac.get_actions_log_prob(a)
            tr.action_mean, tr.action_sigma = ac.action_mean, ac.action_std
            tr.observations, tr.critic_observations = obs[t], cobs[t]
            alg.process_env_step(rew[t], dones[t], {"time_outs": tout[t]})
        alg.compute_returns(cobs[-1])


def capture_update(alg):
    """alg.update() with every minibatch recorded: the batch it was given, the weights it started from, every .grad
    before and after the clip and, on the device, the fused 2-norm of the flat gradient bucket the clip takes."""
    ac = alg.actor_critic
    records = []
    step, clip = alg._minibatch_step, alg._clip_grads

    def grads():
        return {k: p.grad.detach().clone() for k, p in ac.named_parameters()}

    def recording_step(batch, amp, mse):
        records.append({"batch": [x.detach().clone() for x in batch[:9]],
                        "weights": {k: v.detach().clone() for k, v in ac.state_dict().items()}})
        return step(batch, amp, mse)

    def recording_clip():
        rec = records[-1]
        rec["pre"] = grads()
        if alg.grads.flat.is_cuda:
            rec["fused_norm"] = torch.linalg.vector_norm(alg.grads.flat).item()
        clip()
        rec["post"] = grads()

    alg._minibatch_step, alg._clip_grads = recording_step, recording_clip
    try:
        alg.update()
    finally:
        del alg._minibatch_step, alg._clip_grads
    assert all("post" in r for r in records)
    return records


def golden_inputs():
    d = np.load(f"{GOLDEN}/ppo_update.npz")
    return synthetic_rollout(), torch.from_numpy(d["actions"]), torch.from_numpy(d["perm"])


def make_alg(device, n, t, algo=ALGO, history=None, **kw):
    from ti5_isaacgym_amd.algo.dh_policy import ActorCriticDH
    from ti5_isaacgym_amd.algo.dh_update import DHPPO
    torch.manual_seed(POLICY_SEED)
    ac = ActorCriticDH(235, 47, 219, 12, **POLICY)
    alg = DHPPO(ac, device=device, **algo, **kw)
    alg.graph_act = alg.graph_store = alg.graph_update = False   # the eager steps: the Python the capture wraps
    alg.init_storage(n, t, [66 * 47], [219], [12], history=history)
    alg.storage.graph_gae = False
    return alg


def clip_coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


# ---------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def host_records():
    rollout, actions, perm = golden_inputs()
    alg = make_alg("cpu", N, T)
    fill_rollout(alg, rollout, actions, "cpu")
    mp = pytest.MonkeyPatch()
    mp.setattr(torch, "randperm", lambda n, **kw: perm.to(kw.get("device", "cpu")))
    try:
        records = capture_update(alg)
    finally:
        mp.undo()
    assert len(records) == ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
    return records


def test_host_gradients_match_the_reference_update(host_records):
    fx = np.load(f"{GOLDEN}/ppo_grads.npz")
    names = [str(n) for n in fx["names"]]
    assert names == list(host_records[0]["pre"]) and len(names) == 33
    worst = 0.0

    def close(what, got, ref, scale):
        nonlocal worst
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        worst = max(worst, float(np.abs(got - ref).max()) / scale if scale > 0 else 0.0)
        assert np.all(np.abs(got - ref) <= 1e-6 * scale), (what, got, ref)

    full_mb = [int(m) for m in fx["full_mb"]]
    for mb, rec in enumerate(host_records):
        close(f"pre-clip norm [{mb}]", total_norm(rec["pre"]), fx["pre_norm"][mb], fx["pre_norm"][mb])
        for i, k in enumerate(names):
            for j, when in ((0, "pre"), (2, "post")):
                g = rec[when][k].double().reshape(-1)
                s, ss = fx["stats"][mb, i, j], fx["stats"][mb, i, j + 1]
                # a sum of cancelling terms: relative to its terms' scale, sqrt(numel x sum of squares) >= |sum|
                close(f"{when} sum {k} [{mb}]", g.sum().item(), s, math.sqrt(g.numel() * ss))
                close(f"{when} norm {k} [{mb}]", g.norm().item(), math.sqrt(ss), math.sqrt(ss))
                if mb in full_mb:
                    m = full_mb.index(mb)
                    ref = fx[f"probes_{when}"][m, i]
                    got = rec[when][k].reshape(-1)[torch.from_numpy(probe_index64(g.numel()))].numpy()
                    close(f"{when} probes {k} [{mb}]", got, ref, np.abs(ref).max())
                    if g.numel() <= FULL_NUMEL:
                        ref = fx[f"full_{when}_{mb}_{i}"]
                        close(f"{when} full {k} [{mb}]", rec[when][k].numpy(), ref, np.abs(ref).max())
    print(f"host gradients vs the reference's: worst difference / scale {worst:.2e}")


def test_fp64_restatement_matches_the_host_gradients(host_records):
    worst, worst32, per = ("", 0.0), ("", 0.0), []
    for mb, rec in enumerate(host_records):
        kinks = []
        g64 = reference_grads(rec["weights"], rec["batch"], ALGO, kinks=kinks)
        g32 = reference_grads(rec["weights"], rec["batch"], ALGO, dtype=torch.float32)
        assert list(g64) == list(rec["pre"])
        g64 = nearest_reference(rec["pre"], g64, kinks)
        for k, g in rec["pre"].items():
            e, e32 = rel_l2(g, g64[k]), rel_l2(g32[k], g)
            per.append(e)
            worst = max(worst, (f"{k} [{mb}]", e), key=lambda x: x[1])
            worst32 = max(worst32, (f"{k} [{mb}]", e32), key=lambda x: x[1])
            assert e <= 1e-5, (k, mb, e)
            assert e32 <= 1e-5, (k, mb, e32)
    print(f"host vs fp64 restatement: worst relative L2 {worst[1]:.2e} ({worst[0]}), median {np.median(per):.1e}; "
          f"fp32 restatement vs host: worst {worst32[1]:.2e} ({worst32[0]})")


def test_host_clip_is_the_fp64_coefficient(host_records):
    clipped, worst = set(), 0.0
    for mb, rec in enumerate(host_records):
        norm = total_norm(rec["pre"])
        assert abs(norm - ALGO["max_grad_norm"]) > 1e-4, (mb, norm)   # no decision within rounding of the threshold
        coef = clip_coef(norm, ALGO["max_grad_norm"])
        if coef < 1.0:
            clipped.add(mb)
        for k, g in rec["pre"].items():
            e = rel_l2(rec["post"][k], g.double() * coef)
            worst = max(worst, e)
            assert e <= 2e-6, (k, mb, e)
            assert torch.equal(rec["post"][k], g) == (coef == 1.0), (k, mb)
    print(f"post-clip vs pre-clip x fp64 coefficient: worst relative L2 {worst:.2e}; clipped minibatches {sorted(clipped)}")
    assert clipped == {1, 2, 3, 7}
