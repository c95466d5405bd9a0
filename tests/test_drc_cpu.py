"""CPU: the dynamic range control model (tests/drc_model.py) against the rule of include/ac3mi.h - table values, the five
static curves at and between their breakpoints, the smoothing, the code round trip - and the tables frozen in the HIP
source against the model's."""
import math
import os
import re

import numpy as np
import pytest

from tests import drc_model as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_values():
    assert D.LG[0] == 0 and D.LG[255] == 255 and D.LG[128] == round(256 * math.log2(1.5))
    assert D.DN[31] == 1318 and D.DN[24] == 1020 and D.DN[1] == 43
    assert D.XT[0] == 0 and D.XT[255] == 32 and D.XT[254] == 32 and D.XT[253] == 31
    assert all(0 <= v <= 32 for v in D.XT) and all(a <= b for a, b in zip(D.XT, D.XT[1:]))
    # no entry is within 1e-4 of a rounding tie: the tables do not depend on how the doubles round
    for vals in ([256 * math.log2(1 + m / 256) for m in range(256)], [32 * (2 ** (f / 256) - 1) for f in range(256)],
                 [256 * d / (20 * math.log10(2)) for d in range(32)]):
        assert min(abs(v % 1 - 0.5) for v in vals) > 1e-4


def test_profile_table():
    assert D.PROFILES[1] == (255, 2, 0, 213, 638, 2, 20)
    assert D.PROFILES[2] == (255, 2, -425, 425, 850, 2, 20)
    assert D.PROFILES[3] == (510, 2, 0, 213, 638, 2, 20)
    assert D.PROFILES[4] == (510, 2, -425, 425, 425, 2, 2)
    assert D.PROFILES[5] == (638, 5, 0, 213, 638, 2, 20)


def test_hip_tables_are_the_model():
    src = open(os.path.join(ROOT, "ac-3-acm-codec_amd", "csrc", "encode.hip")).read()

    def table(name):
        m = re.search(r"\b%s(?:\[\d+\])+\s*=\s*\{([^;]*)\};" % name, src)
        assert m, name
        return [int(v) for v in re.findall(r"-?\d+", m.group(1))]

    assert table("DRC_LG") == D.LG
    assert table("DRC_XT") == D.XT
    assert table("DRC_DN") == D.DN
    curves = table("DRC_CURVE")
    assert [tuple(curves[7 * i:7 * i + 7]) for i in range(5)] == [D.PROFILES[p] for p in range(1, 6)]


def test_level():
    assert D.level(0) == -4096 and D.level(1) == -4096
    t = np.arange(256)
    e = int(np.round(32767 * np.sin(2 * np.pi * t / 32)).astype(np.int64) @ np.round(32767 * np.sin(2 * np.pi * t / 32)).astype(np.int64))
    assert abs(D.level(e)) <= 2                          # a full-scale sine on one channel reads about 0
    assert D.level(e // 100) - D.level(e) in range(-1701 - 2, -1701 + 3)     # -20 dB
    for k in range(1, 40):
        assert D.lg(1 << k) == 256 * k
        assert D.lg(3 << k) - 256 * (k + 1) == D.LG[128]


@pytest.mark.parametrize("profile", [1, 2, 3, 4, 5])
def test_curve_breakpoints_and_segments(profile):
    mb, rb, n0, n1, c0, re_, rc = D.PROFILES[profile]
    g = lambda r: D.curve(r, profile)
    # null band
    assert g(n0) == 0 and g(n1) == 0 and g((n0 + n1) // 2) == 0
    # boost below N0: slope (Rb - 1) / Rb, capped at MB
    assert g(n0 - 1) == (rb - 1) // rb
    assert g(n0 - 100) == (100 * (rb - 1)) // rb
    assert g(n0 - 10000) == mb
    r_cap = n0 - (mb * rb + rb - 2) // (rb - 1)                # the first r whose boost reaches MB
    assert g(r_cap) == mb and g(r_cap + 1) < mb
    # early cut (N1, C0]: slope (Re - 1) / Re
    if c0 > n1:
        assert g(n1 + 1) == -((re_ - 1) // re_)
        assert g(c0) == -(((c0 - n1) * (re_ - 1)) // re_)
        mid = (n1 + c0) // 2
        assert g(mid) == -(((mid - n1) * (re_ - 1)) // re_)
    # late cut above C0: slope (Rc - 1) / Rc on top of the early cut's end
    base = -(((c0 - n1) * (re_ - 1)) // re_)
    assert g(c0 + 1) == base - ((rc - 1) // rc)
    assert g(c0 + 200) == base - ((200 * (rc - 1)) // rc)
    # the cut floor
    assert g(100000) == -1024
    # monotone: never more gain for a louder block
    rs = list(range(-5000, 6000, 7))
    assert all(a >= b for a, b in zip(map(g, rs), map(g, rs[1:])))


def test_smoothing_moves_toward_without_overshoot():
    rng = np.random.default_rng(5)
    for _ in range(200):
        s, g = int(rng.integers(-1024, 700)), int(rng.integers(-1024, 700))
        n = 0
        while s != g:
            t = D.step(s, g)
            assert (g - t) * (g - s) >= 0 and abs(g - t) < abs(g - s)       # toward g, never past it
            s = t
            n += 1
            assert n < 5000
        assert D.step(s, g) == g
    # attack is fast (about 50 ms at 48 kHz), release slow (about 1 s): blocks to cover 90 % of a 600 lv step
    def blocks(s, g):
        n, s0 = 0, s
        while abs(g - s) > abs(g - s0) // 10:
            s = D.step(s, g)
            n += 1
        return n
    assert 15 <= blocks(0, -600) <= 30
    assert 300 <= blocks(0, 600) <= 500


def test_code_round_trip():
    for s in range(-1024, 1024):
        v = D.code_of(s)
        if -128 < v < 127:
            assert abs(20 * math.log10(D.decoded_gain(v) / 2 ** (s / 256))) <= 0.14, s
    assert D.code_of(0) == 0 and D.decoded_gain(0) == 1.0
    assert D.code_of(-1024) == -128 and D.decoded_gain(-128) == 2.0 ** -4
    assert D.code_of(255) == 32 == D.code_of(256)   # XT[255] = 32 carries into the next octave: 2^1 exactly
    assert D.decoded_gain(32) == 2.0


def test_sent_flags():
    c = np.array([[3, 3, 4, 4, 4, 3], [3, 3, 3, 3, 3, 3]])
    assert D.sent(c).tolist() == [[True, False, True, False, False, True], [True, False, False, False, False, False]]


def test_model_on_a_programme():
    """Silence then a loud tone: boost first, then the attack pulls the state down within a few blocks."""
    t = np.arange(4 * 1536)
    x = np.zeros((4 * 1536, 2), np.int64)
    x[2 * 1536:, 0] = np.round(30000 * np.sin(2 * np.pi * 1000 / 48000 * t[2 * 1536:]))
    codes, snt, s, states = D.encode(x.astype(np.int16), (0, 1), 2, 1, dialnorm=31)
    assert states[1, 5] > 0 and states[3, 5] < 0 and s == states[3, 5]
    assert snt[:, 0].all()
    assert codes.min() >= -128 and codes.max() <= 127
