"""Generate tests/golden/ppo_grads.npz: the gradients of the reference's own DHPPO update, before and after its clip.

gen_ppo_golden.py's setup (the same seeds, POLICY, ALGO, synthetic_rollout and minibatch permutation; the reference's
modules loaded the same way) with the reference's DHPPO.update run on the CPU and torch.nn.utils.clip_grad_norm_
(dh_ppo.py:181) intercepted.  Recorded, for each of the 2 epochs x 4 minibatches of 192 rows:

  pre_norm      the total 2-norm of the gradients before the clip: a float64 reduction of the fp32 .grad tensors
  stats         per parameter tensor the float64 sum and sum of squares of .grad before and after the clip
                (minibatch, tensor, [sum pre, sum-sq pre, sum post, sum-sq post])

and for the minibatches FULL_MB (the first one and the most clipped one) per tensor

  probes_pre / probes_post   .grad at the PROBE positions of probe_index64 (fp32)
  full_pre_<mb>_<i> / full_post_<mb>_<i>   every tensor i of at most FULL_NUMEL elements in full (fp32)

Recorded results only.  tests/test_ppo_grads.py replays the same update through the build on the host and compares.

    python tests/golden/gen_ppo_grads.py [/root/reference]
"""
import os

import numpy as np
import torch

from gen_ppo_golden import (ALGO, N, PERM_SEED, POLICY, POLICY_SEED, ROLLOUT_SEED, T, load_reference_ppo,
                            synthetic_rollout)

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = 64
FULL_MB = (0, 3)
FULL_NUMEL = 4096


def probe_index64(numel):
    return (np.arange(PROBE, dtype=np.int64) * 7919 + 13) % numel


def main():
    dh_ppo, acdh = load_reference_ppo()
    torch.manual_seed(POLICY_SEED)
    ac = acdh.ActorCriticDH(235, 47, 219, 12, **POLICY)
    alg = dh_ppo.DHPPO(ac, device="cpu", **ALGO)
    alg.init_storage(N, T, [66 * 47], [219], [12])
    obs, cobs, rew, dones, tout = synthetic_rollout()
    torch.manual_seed(ROLLOUT_SEED + 1)
    for t in range(T):
        alg.act(obs[t], cobs[t])
        alg.process_env_step(rew[t].clone(), dones[t].clone(), {"time_outs": tout[t].clone()})
    alg.compute_returns(cobs[T])

    names = [k for k, _ in ac.named_parameters()]
    pre_norm, stats, probes_pre, probes_post, full = [], [], [], [], {}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def grads():
        return [p.grad.detach().clone() for _, p in ac.named_parameters()]

    def recording_clip(parameters, max_norm, *a, **k):
        mb = len(pre_norm)
        pre = grads()
        out = orig_clip(parameters, max_norm, *a, **k)
        post = grads()
        pre_norm.append(float(np.sqrt(sum(g.double().pow(2).sum().item() for g in pre))))
        stats.append([[g.double().sum().item(), g.double().pow(2).sum().item(),
                       h.double().sum().item(), h.double().pow(2).sum().item()] for g, h in zip(pre, post)])
        if mb in FULL_MB:
            idx = [torch.from_numpy(probe_index64(g.numel())) for g in pre]
            probes_pre.append(np.stack([g.reshape(-1)[i].numpy() for g, i in zip(pre, idx)]))
            probes_post.append(np.stack([g.reshape(-1)[i].numpy() for g, i in zip(post, idx)]))
            for i, (g, h) in enumerate(zip(pre, post)):
                if g.numel() <= FULL_NUMEL:
                    full[f"full_pre_{mb}_{i}"] = g.numpy()
                    full[f"full_post_{mb}_{i}"] = h.numpy()
        return out

    torch.nn.utils.clip_grad_norm_ = recording_clip
    try:
        torch.manual_seed(PERM_SEED)
        alg.update()
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    assert len(pre_norm) == ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
    path = os.path.join(HERE, "ppo_grads.npz")
    np.savez_compressed(path, names=np.array(names), max_grad_norm=np.float64(ALGO["max_grad_norm"]),
                        pre_norm=np.array(pre_norm, np.float64), stats=np.array(stats, np.float64),
                        full_mb=np.array(FULL_MB), probes_pre=np.stack(probes_pre), probes_post=np.stack(probes_post),
                        **full)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB; pre-clip norms {pre_norm}")


if __name__ == "__main__":
    main()
