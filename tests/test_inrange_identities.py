"""CPU test of the claim behind csrc/rtk_device_math.h's sqrt_inrange / rcp_inrange: inside the admitted exponent range the
instructions they leave out of the compiler's f64 square-root and 1/x expansions do nothing, so short and full forms
return the same bits for every hardware seed -- and the guard sends everything else to the full forms.

tests/helpers/inrange_identities.cpp restates the four sequences with fma() and takes the seed as a parameter (the true
1/sqrt(x) or 1/x moved by up to +-4 x 2^29 ulp, the documented precision of v_rsq_f64 / v_rcp_f64 being 2^29 ulp).  It is a
stand-alone program and is built with the address and undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

from tests.conftest import ROOT


def test_short_forms_equal_the_full_expansions_and_the_guard_refuses_the_rest():
    src = os.path.join(ROOT, "tests", "helpers", "inrange_identities.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "inrange_identities")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", exe, src])
        p = subprocess.run([exe, str(1 << 24)], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "identity mismatches: 0" in out, out[-4000:]
    assert "guard failures: 0" in out, out[-4000:]
    assert "scaled paths seen: 3" in out, out[-4000:]  # the model's full forms do scale outside the range: the comparison is not vacuous
    evaluations = int(out.split("evaluations:")[1].split()[0])
    assert evaluations >= 11 * (1 << 24)  # 2^24 significands x (9 seeds on the +-4 grid + 2 in between), and the per-exponent sweep
