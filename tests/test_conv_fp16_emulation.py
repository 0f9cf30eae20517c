"""The fp16-input history conv's algebra on the CPU (tools/conv_emulate.py): an fp16 input is its own hi part, so
sum x w_hi + 2^-11 sum x w_lo with fp32 accumulation -- two of the fp32 kernel's three split products -- stays within
the project's conv bound, 1e-5 (1 + |y|), of an fp64 conv of the same (widened) input.  The GPU test
(test_gpu_policy_fp16_obs.py) then has the staging, the odd-half alignment and the hardware left to check."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.mark.parametrize("scale", [1.0, 1.5])
def test_fp16_input_conv_algebra_within_the_conv_bound(scale):
    from conv_emulate import emulate_error
    err = emulate_error(scale=scale, batch=777)
    print("weights x", scale, "max err / (1 + |y|) =", err)
    assert err < 1e-5, err
