"""The bits the 32-env k_heads kernel produced, recorded for tests/test_gpu_policy_heads.py -- needs the MI355X.

    python tests/golden/gen_heads_bits.py [--commit ID] [--out tests/golden/heads_bits.npz]

Run it inside a checkout of a033595, the last commit that has k_heads (T1POLICY_HEADS64=0 there): the recorded outputs
are that kernel's own, and the script refuses to write unless that commit's k_heads64 (the variable unset) gives the
same bits.  Later commits have one kernel and ignore the variable: run there, both passes are k_heads64 and the file
would hold its bits, not the reference's.  The script stays as the record of how the file was made, and for inputs()
and digest(), which the test shares.

Cases: the policy of the tests' _model(scale=1.5), inputs as test_heads64_equals_heads32 built them (seed n + 1), at
n = 33 (one full 32-env column tile and one env: the workgroup's second tile has one live lane) and n = 545 (nine
64-env tiles: the ninth is in the second group of 16 workgroups of the ((bid >> 4) << 3) + (bid & 7) tile map, and its
tail is again 33 envs).  Per case the five outputs of heads_forward as raw fp32, and the sha256 of the input bytes and
of the parameter bytes, so that the test can tell drifted inputs from drifted results.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "heads_bits.npz")
CASES = (33, 545)
NAMES = ("mean", "actions", "sigma", "logp", "value")
SWITCH = "T1POLICY_HEADS64"


def model():  # tests/test_gpu_policy_heads.py, _model(seed=0, scale=1.5)
    from ti5_isaacgym_amd import task_registry
    from ti5_isaacgym_amd.algo.dh_policy import ActorCriticDH
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    _, tc = task_registry.get_cfgs("t1_dh_stand")
    torch.manual_seed(0)
    ac = ActorCriticDH(235, 47, 219, 12, **class_to_dict(tc)["policy"])
    with torch.no_grad():
        for p in ac.parameters():
            p.mul_(1.5)
        ac.std.copy_(torch.linspace(0.2, 1.3, 12))
    return ac


def inputs(n):
    """-> obs (n, 66 * 47), critic_obs (n, 219), eps (n, 12): fp32 on the host"""
    g = torch.Generator().manual_seed(n + 1)
    obs = (torch.randn(n, 66 * 47, generator=g) * 2.0).clamp(-18, 18)
    cobs = torch.randn(n, 219, generator=g) * 2.0
    eps = torch.randn(n, 12, generator=g)
    return obs, cobs, eps


def digest(tensors):
    """sha256 of the tensors' bytes, one after the other"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def forward(ac, n):
    """-> the five outputs of heads_forward on inputs(n) as host fp32 arrays"""
    from ti5_isaacgym_amd.algo.dh_policy import heads_forward
    dev = torch.device("cuda:0")
    with torch.inference_mode():
        out = heads_forward(ac, *[t.to(dev) for t in inputs(n)])
        assert out is not None, "the fused heads have no instance for the t1 policy"
        return [t.cpu().numpy().copy() for t in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown", help="the commit the checkout is at, recorded in the file")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from ti5_isaacgym_amd import _lib
    ac = model()
    out = {"commit": np.array(a.commit), "library": np.array(_lib.load().t1env_version().decode()),
           "command": np.array("python tests/golden/gen_heads_bits.py --commit " + a.commit),
           "params_sha256": np.array(digest(ac.parameters()))}
    acd = ac.to("cuda:0")
    for n in CASES:
        os.environ.pop(SWITCH, None)
        o64 = forward(acd, n)
        os.environ[SWITCH] = "0"
        o32 = forward(acd, n)
        os.environ.pop(SWITCH, None)
        for name, x64, x32 in zip(NAMES, o64, o32):
            assert x32.dtype == np.float32 and np.isfinite(x32).all(), (n, name)
            assert np.array_equal(x64.view(np.uint32), x32.view(np.uint32)), \
                f"n = {n}, {name}: k_heads64 and k_heads differ -- nothing written"
            out[f"{n}_{name}"] = x32
        out[f"{n}_inputs_sha256"] = np.array(digest(inputs(n)))
        print(f"{n} envs: k_heads64 == k_heads on {', '.join(NAMES)}; inputs {str(out[f'{n}_inputs_sha256'])[:16]}")
    np.savez(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes; parameters", str(out["params_sha256"])[:16])


if __name__ == "__main__":
    main()
