"""CPU: the branch-free rules of enc_mdct_kernel's block loop, csrc/mdct_rule.h - a coefficient's raw exponent, the largest
magnitude of a lane's eight windowed samples, and the twiddle (32768, 0) that multiplies to what the reference gets by not
multiplying.  The checks run in tests/mdct_rule_c/main.cpp (see there), a program of its own built with the host compiler
under -fsanitize=address,undefined; it exits non-zero at the first disagreement with the expressions the rules replaced."""
import os
import subprocess

import pytest

from tests import _harness as H


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mdct_rule")
    exe = str(tmp / "mdct_rule")
    H.build_sanitised([os.path.join(H.ROOT, "tests", "mdct_rule_c", "main.cpp")], exe, includes=[H.CSRC])
    r = subprocess.run([exe, "20252"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return r.stdout.splitlines()


def test_raw_exponent_rule(program_output):
    """every c with |c| < 2^18, both signs, every v in 0..14"""
    assert program_output[0] == "exponent ok checked=%d" % (15 * (2 * (1 << 18) - 1))


def test_magnitude_rule(program_output):
    """200 000 drawn 8-tuples and all 6^8 tuples over the extremes"""
    assert program_output[1] == "magnitude ok checked=%d" % (200000 + 6 ** 8)


def test_unit_twiddle(program_output):
    """every 16-bit q"""
    assert program_output[2] == "twiddle ok checked=65536"
