"""Dev probe: the rollout's act() (DHPPO.act: policy sample, value, log-prob as one replayed HIP graph) at N envs on
random observations, fused HIP heads vs torch's layers (T1_FUSED_ACT is read at import; --torch flips it here) -- or,
with --mode, the deterministic policy / the critic a trained checkpoint is evaluated with.

    python tools/act_bench.py [--num-envs 8192] [--iters 200] [--torch] [--obs-dtype fp16]
                              [--mode act|inference|critic] [--eager]

--obs-dtype fp16: the observations rounded to fp16 and passed as fp16 tensors, as an env with cfg.env.state_dtype =
"fp16" returns them (BASELINE config 5).
--mode inference: DHOnPolicyRunner.get_inference_policy(graphed=True)'s callable (runner.GraphedInference: the first
conv + the actor-only heads kernel as one replayed graph; --eager: act_inference call by call), timed the same way.
--mode critic: get_inference_critic()'s path (dh_policy.critic_forward, eager).  With --torch both run torch's layers
(T1_FUSED_INFERENCE=0: act_inference / evaluate as they were before the fused inference kernels); torch's layers do not
take fp16 observations, so that arm widens them first (obs.float() inside the timed loop, the copy a user needed).

Prints one JSON line: wall ms per call (back to back, one sync at the end), and for --mode act the heads kernel's own
duration from HIP events around the fused call when it runs eagerly.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / iters * 1e3, 4)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--num-envs", type=int, default=8192)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--torch", action="store_true")
    p.add_argument("--obs-dtype", choices=["fp32", "fp16"], default="fp32")
    p.add_argument("--mode", choices=["act", "inference", "critic"], default="act")
    p.add_argument("--eager", action="store_true", help="--mode inference: no graph")
    a = p.parse_args()
    if a.mode != "act" and a.torch:
        os.environ["T1_FUSED_INFERENCE"] = "0"
    from ti5_isaacgym_amd import task_registry
    from ti5_isaacgym_amd.algo import dh_update
    from ti5_isaacgym_amd.algo.dh_policy import ActorCriticDH, critic_forward, fused_inference_enabled
    from ti5_isaacgym_amd.algo.runner import GraphedInference
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    dh_update.FUSED_ACT = not a.torch
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    cfg = class_to_dict(tc)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ac = ActorCriticDH(235, 47, 219, 12, **cfg["policy"]).to(dev)
    alg = dh_update.DHPPO(ac, device=str(dev), **cfg["algorithm"])
    n = a.num_envs
    obs = torch.randn(n, 66 * 47, device=dev).clamp(-18, 18)
    cobs = torch.randn(n, 219, device=dev)
    if a.obs_dtype == "fp16":
        obs, cobs = obs.half(), cobs.half()
    out = {"num_envs": n, "path": "torch" if a.torch else "fused", "obs_dtype": a.obs_dtype, "mode": a.mode}
    if a.mode != "act":
        out["tile"] = os.environ.get("T1POLICY_INFER_TILE", "auto")
        ac.eval()
        widen = a.torch and a.obs_dtype == "fp16"
        with torch.inference_mode():
            if a.mode == "inference":
                policy = ac.act_inference if (a.eager or a.torch) else GraphedInference(ac)
                out["inference_ms"] = _time((lambda: policy(obs.float())) if widen else (lambda: policy(obs)), a.iters)
                out["graphed"] = bool(getattr(policy, "graphs", None))
            else:
                def critic(x):
                    v = critic_forward(ac, x) if fused_inference_enabled(x) else None
                    return v if v is not None else ac.evaluate(x)
                out["critic_ms"] = _time((lambda: critic(cobs.float())) if widen else (lambda: critic(cobs)), a.iters)
        print(json.dumps(out), flush=True)
        return
    with torch.inference_mode():
        out["act_ms"] = _time(lambda: alg.act(obs, cobs), a.iters)
        out["graphed"] = bool(alg._act_graphs)
        # the eager body, bracketed by events (conv + pack + heads + randn for the fused path)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            alg._act_body(obs, cobs)
        e1.record()
        torch.cuda.synchronize()
        out["act_body_eager_ms"] = round(e0.elapsed_time(e1) / 50, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
