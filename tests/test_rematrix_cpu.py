"""CPU: the rematrixing setter is part of the ABI, and the numpy model of its decision (tests/rematrix_model.py, the
definition in include/ac3mi.h) decides hand-built rows as the rule says."""
import os
import re
import subprocess

import numpy as np

from tests import _harness as H
from tests import rematrix_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setter_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ac3mi.h")).read()
    assert re.search(r"int\s+ac3mi_set_encode_rematrix\s*\(\s*ac3mi_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*\)\s*;", hdr)
    pkg = H.pkg()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "ac3mi_set_encode_rematrix" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "ac3mi_set_encode_rematrix" in pkg.declared_symbols()
    assert hasattr(pkg.Engine, "set_encode_rematrix")


def _row(seed, amp=20000):
    rng = np.random.default_rng(seed)
    return np.round(rng.standard_normal(256) * amp / 4).astype(np.int64)


def test_identical_channels_flag_every_band():
    x = _row(1)
    fl, a, b, m, s = M.decide(x, x, 3, 3)
    assert fl == 0b1111
    assert np.array_equal(m, x) and not s.any()


def test_silent_channel_flags_none():
    fl = M.decide(_row(2), np.zeros(256, np.int64), 3, 14)[0]
    assert fl == 0
    # 40 dB down and independent: never
    assert M.decide(_row(3), _row(4, 200), 3, 9)[0] == 0


def test_band_at_the_threshold_is_not_flagged():
    """In band 0 (bins 13..24): L = (3, 0, ...), R = (1, 0, ...) -> EL = 9, ER = 1, EM = 4, ES = 1: 2 min(EM, ES) = 2 > 1.
    L = (1, 1), R = (1, -1) -> EL = ER = 2, EM = ES = 1: 2 == 2, not flagged.  L = (2, 2), R = (2, 0) -> EL = 8, ER = 4,
    EM = 1 + 4, ES = 1: 2 < 4, flagged."""
    def band0(l, r):
        cl = np.zeros(256, np.int64)
        cr = np.zeros(256, np.int64)
        cl[13:13 + len(l)] = l
        cr[13:13 + len(r)] = r
        return M.decide(cl, cr, 5, 5)[0] & 1
    assert band0([3], [1]) == 0
    assert band0([1, 1], [1, -1]) == 0
    assert band0([2, 2], [2, 0]) == 1
    # the band edges: the same pair one bin below band 0 (bin 12) and at bin 223 count nowhere
    cl = np.zeros(256, np.int64)
    cl[12] = cl[223] = 1000
    assert M.decide(cl, cl.copy(), 5, 5)[0] == 0


def test_rows_with_different_v_align():
    """A row's true scale is c / 2^v: the row with the larger v is shifted down to the smaller one (arithmetic shift)."""
    x = _row(5)
    cl = x << 3                                 # L at v = 6, R the same signal at v = 3
    fl, a, b, m, s = M.decide(cl, x, 6, 3)
    assert fl == 0b1111 and np.array_equal(a, x) and np.array_equal(b, x)
    cl = np.full(256, -5, np.int64)
    a = M.decide(cl, cl.copy(), 7, 5)[1]
    assert np.all(a == -2)                      # -5 >> 2 = -2 (toward minus infinity)
    # the coded rows: shift vm - 9 on both channels, M / S in the flagged bands, aligned L' / R' elsewhere
    rows = np.zeros((1, 6, 2, 256), np.int64)
    v = np.full((1, 6, 2), 5, np.int64)
    rows[0, 0, 0] = x << 2
    rows[0, 0, 1] = x
    v[0, 0, 0] = 7
    out, shift, flags, rs = M.rematrix(rows, v)
    assert flags[0, 0] == 0b1111 and shift[0, 0, 0] == shift[0, 0, 1] == -4
    assert np.array_equal(out[0, 0, 0, 13:223], x[13:223]) and not out[0, 0, 1, 13:223].any()
    assert np.array_equal(out[0, 0, 0, :13], x[:13]) and np.array_equal(out[0, 0, 1, 223:], x[223:])


def test_rematstr_over_a_block_sequence():
    x, y = _row(6), np.zeros(256, np.int64)
    rows = np.zeros((2, 6, 2, 256), np.int64)
    v = np.full((2, 6, 2), 4, np.int64)
    v[0, 2:4, 1] = 14                           # (a silent R row's v)
    # frame 0: flagged, flagged, none, none, flagged, flagged; frame 1: none everywhere
    for b, same in enumerate((1, 1, 0, 0, 1, 1)):
        rows[0, b, 0] = x
        rows[0, b, 1] = x if same else y
    rows[1, :, 0] = x
    out, shift, flags, rs = M.rematrix(rows, v)
    assert list(flags[0]) == [15, 15, 0, 0, 15, 15]
    assert list(rs[0]) == [1, 0, 1, 0, 1, 0]
    assert list(flags[1]) == [0] * 6 and list(rs[1]) == [1, 0, 0, 0, 0, 0]     # block 0 of every frame sends
    assert np.array_equal(out[1], rows[1]) and np.array_equal(out[0, 2:4], rows[0, 2:4])
    # block switching: two channels that differ in blksw get no flags
    bs = np.zeros((2, 6, 2), np.int64)
    bs[0, 1, 1] = 1
    flags2 = M.rematrix(rows, v, bs)[2]
    assert list(flags2[0]) == [15, 0, 0, 0, 15, 15]


def test_block_v():
    """v from the PCM: silence gives 14, a full-scale block 0 (or near it)."""
    pcm = np.zeros((1536, 2), np.int16)
    pcm[:, 0] = 20000
    v = M.block_v(pcm, (0, 1))
    assert v.shape == (1, 6, 2) and np.all(v[0, :, 1] == 14)
    assert v[0, 1:, 0].max() <= 1
