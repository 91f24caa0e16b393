"""The scaling identities of the scan kernel's unscaled staging (tests/cpp/stage4_identities_test.cpp over amatsukaze_amd/csrc/exact_math.h).

The scan (pair) kernel stages DeintY's [1 2 1] row sums without their factor 0.25 and runs on taps the host scaled by 0.25 instead:
four times the reference's window values, the reference's correlations bit for bit.  That rests on scaling by a power of two commuting
with every rounding on the way, which holds while nothing is rounded in the denormal range -- the host checks every logo
(EvalEngine::stage4_eligible; the limits are exact_math.h stage4_coef_ok / stage4_tap_ok) and keeps plain taps otherwise.  The program
replays each identity with the device's operations over the edges of what the rule admits and three million random operands each:
div25(4 x) = 4 div25(x); a (4 s) + b (4 maxv) = 4 (a s + b maxv); (k / 4)(4 w - 4 m) = k (w - m), also as a multiply-add; the bin from four
times the mean (clamp at 1020, >> 5) against the reference's (clamp at 255, >> 3), negatives, means beyond the clamp and NaN included.
It also shows that an operand just below either limit breaks an identity."""
import os
import subprocess

import amtlib

ROOT = amtlib.ROOT


def test_scaling_identities_hold_over_what_the_rule_admits(tmp_path):
    out = str(tmp_path / "stage4_identities_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stage4_identities_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
