"""CPU: the window rule of the SNR-offset search, csrc/snr_window.h - how a band's k steps over sixteen consecutive offsets, the
three addresses of a bin, the widening of the packed cost words, a block's ceilings and sixths, and which window is costed next.
The checks run in tests/snr_window_c/main.cpp (see there), a program of its own built with the host compiler under
-fsanitize=address,undefined; it exits non-zero at the first disagreement.  Its `rule` lines are the window rule on drawn states,
which profiles/search_window_sim.py (the simulator the rule's constants were chosen with) must restate exactly."""
import os
import subprocess
import sys

import pytest

from tests import _harness as H

sys.path.insert(0, os.path.join(H.ROOT, "profiles"))

FRAMES = 40


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("snr_window")
    exe = str(tmp / "snr_window")
    H.build_sanitised([os.path.join(H.ROOT, "tests", "snr_window_c", "main.cpp")], exe, includes=[H.CSRC])
    r = subprocess.run([exe, "20251", str(FRAMES)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return r.stdout.splitlines()


def test_step_and_address_rules(program_output):
    """every x in -8192..8191, every t in 0..15, every exponent 0..24 and 255"""
    assert program_output[0] == "step_address ok"


def test_whole_windows_against_a_count_offset_by_offset(program_output):
    """bits, counts, ceilings and sixths of every block at the sixteen offsets; the cases the count must contain"""
    line = program_output[1].split()
    assert line[:2] == ["window", "ok"]
    v = dict(tok.split("=") for tok in line[2:])
    assert int(v["frames"]) == FRAMES and int(v["checked"]) == FRAMES * 16 * 6
    assert int(v["floored"]) > 0          # bands whose k reached 0 inside the window
    assert int(v["lfe"]) > 0              # frames with an LFE row of 7 bins


def test_the_simulator_restates_the_rule(program_output):
    import search_window_sim as W
    rules = [[int(t) for t in ln.split()[1:]] for ln in program_output if ln.startswith("rule ")]
    assert len(rules) == 4000
    for hint, cold, g_prev, first, sweeps, gl, sl, gh, sh, slope, cmin, cmax, gq, nxt in rules:
        assert W.first_lo(hint, bool(cold), g_prev) == first
        assert W.next_lo(sweeps, gl, sl, gh, sh, slope, cmin, cmax, gq) == nxt
