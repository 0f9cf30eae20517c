"""Host code keeps the plain expressions: t1_common.h's fmad / fnmad return a * b + c and c - a * b exactly as the host
compiler evaluates them, for float and for double, so the CPU oracle build and the fp64 replicas of the dynamics compile
to what they compiled to before the device code's contraction was pinned.  A stand-alone program is compiled with g++
(the oracle build's flags, oracle/build_cpu.py) against the header; its operands are chosen so that the fused and the
unfused result differ, and it compares fmad with the expression spelled out in the same translation unit."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstring>
#include "t1_common.h"
template <typename R> __attribute__((noinline)) int check(R a, R b, R c) {
  const R f = t1::fmad(a, b, c), p = a * b + c, g = t1::fnmad(a, b, c), q = c - a * b;
  const R u = t1::fmad<false>(a, b, c), v = t1::pmul(a, b) + c;
  return std::memcmp(&f, &p, sizeof(R)) || std::memcmp(&g, &q, sizeof(R)) || std::memcmp(&u, &p, sizeof(R)) ||
         std::memcmp(&v, &p, sizeof(R));
}
int main(int argc, char**) {
  // a * b = 1 - eps^2 rounds to 1: the unfused a * b + c is 0, the fused one -eps^2
  const float ef = 1.0f / 4096.0f / 4096.0f * (float)argc;   // 2^-24, not a compile-time constant
  const double ed = 1.0 / 9007199254740992.0 * (double)argc;  // 2^-53
  int bad = check<float>(1.0f + ef * 2, 1.0f - ef * 2, -1.0f) | check<double>(1.0 + ed * 2, 1.0 - ed * 2, -1.0);
  const float fused = __builtin_fmaf(1.0f + ef * 2, 1.0f - ef * 2, -1.0f);
  volatile float prod = (1.0f + ef * 2) * (1.0f - ef * 2);
  const float plain = prod + -1.0f;
  std::printf("bad=%d fused=%a plain=%a\n", bad, fused, plain);
  return bad || fused == plain;
}
"""


@pytest.mark.parametrize("flags", [["-O3", "-march=x86-64-v3"], ["-O2"], ["-O0"]], ids=["oracle-flags", "O2", "O0"])
def test_host_fmad_is_the_plain_expression(flags, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the CPU oracle (oracle/build_cpu.py)"
    src = tmp_path / "fmad_host.cpp"
    src.write_text(SRC)
    exe = tmp_path / "fmad_host"
    subprocess.run([gxx, *flags, "-std=c++17", "-I", os.path.join(REPO, "ti5_isaacgym_amd", "csrc"), "-o", str(exe),
                    str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
