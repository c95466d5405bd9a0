"""The content the loudness range tests share (tests/test_loudness_range_cpu.py checks it with the model alone,
tests/test_loudness_range_gpu.py meters it on the device), each fixture built and run through tests/loudness_range_model.py
once per process and then left unchanged."""
import numpy as np

from tests import loudness_model as M
from tests import loudness_range_model as R
from tests.test_loudness_gpu import AMPS, ROLES6

S_MAIN, F_MAIN = 9, 320             # 320 frames: at 48 kHz whole 3 s blocks lie in the quiet lead-in; the ring wraps three times
SEED = 2000                         # margins of 1.1e-5, 1.3e-5 and 5.1e-6 at the three rates
CHANNEL_FLAGS = (1, 2, 3, 7)        # liba52 output flags: 1, 2, 3 and 5 channels
CHANNEL_RATE = 32000
CHANNEL_ROLES = {1: [1], 2: [1, 1], 3: [1, 1, 1], 7: [1, 1, 1, 2, 2]}  # loudness_roles(flags)
SINE_CASES = (((-40, -30), 100), ((-20, -15), 50), ((-40, -20), 200), ((-50, -35, -20, -35, -50), 150))  # levels -> lra_tenths

_cache = {}


def main():
    """rate -> (pcm int16 [9][320 * 1536][6], the nine RangeMeters): noise programmes over the nine amplitudes whose first 45 %
    lie 45 dB down, the odd streams with a 12 dB dip over 70 - 85 % of their length; the LFE slot is loud and not measured"""
    if "main" not in _cache:
        out = {}
        for fs in M.RATES:
            pcm = [M.programme(SEED + fs // 10 + s, F_MAIN, 6, AMPS[s], quiet=0.0056, quiet_part=0.45, loud_slot=3) for s in range(S_MAIN)]
            pcm = np.stack([R.dipped(x) if s & 1 else x for s, x in enumerate(pcm)])
            out[fs] = (pcm, R.run_batch(pcm, fs, ROLES6))
        _cache["main"] = out
    return _cache["main"]


def channels(flags):
    """flags -> (rate, roles, pcm int16 [4][128 * 1536][C], the four RangeMeters): 128 frames at 32 kHz close 61 hops, 32
    blocks"""
    if ("channels", flags) not in _cache:
        fs = CHANNEL_RATE
        roles = CHANNEL_ROLES[flags]
        C = len(roles)
        pcm = [M.programme(7100 + 10 * C + s, 128, C, (0.8, 0.3, 0.1, 0.03)[s], quiet=0.01, quiet_part=0.3) for s in range(4)]
        pcm = np.stack([R.dipped(x, 0.5, 0.8, 9.0) if s & 1 else x for s, x in enumerate(pcm)])
        _cache[("channels", flags)] = (fs, roles, pcm, R.run_batch(pcm, fs, roles))
    return _cache[("channels", flags)]


def sines():
    """Tech 3342's four synthetic cases at 32 kHz: [(levels, expected lra_tenths, pcm int16 [n][2], its RangeMeter)]"""
    if "sines" not in _cache:
        out = []
        for levels, want in SINE_CASES:
            pcm = R.r128_sine(levels)
            out.append((levels, want, pcm, R.run_batch(pcm[None], 32000, [1, 1])[0]))
        _cache["sines"] = out
    return _cache["sines"]


def meter_of_blocks(z3, hops=None):
    """a RangeMeter whose range state holds these 3 s block energies, in this order (the ring is left empty: the read-out
    does not look at it)"""
    m = R.RangeMeter(48000, [1])
    for z in z3:
        z = float(z)
        m.z3.append(z)
        m.r_blocks += 1
        m.max_short = max(m.max_short, z)
        b = M.bin_of(z)
        if b >= 0:
            m.r_blocks_abs += 1
            m.sum_abs += z
            m.r_count[b] += 1
    m.r_hops = (m.r_blocks + R.HOPS - 1 if m.r_blocks else 0) if hops is None else hops
    m.ring_pos = m.r_hops % R.HOPS
    return m


def cut_bin_blocks():
    """sixty blocks from -20 to -10 LUFS and six spread over the one bin that holds the relative gate, three on either
    side of it -> (the 66 energies, the bin, the gate)"""
    loud = 10.0 ** ((np.linspace(-20.0, -10.0, 60) + 0.0137 + 0.691) / 10.0)
    b = M.bin_of(0.01 * loud.mean())
    for _ in range(4):                                  # the gate depends (slightly) on where the six lie: settle
        six = M.EDGES[b] + (M.EDGES[b + 1] - M.EDGES[b]) * np.array([0.08, 0.22, 0.41, 0.58, 0.77, 0.93])
        z = np.concatenate([loud[:30], six, loud[30:]])
        gamma = 0.01 * z.mean()
        b = M.bin_of(gamma)
    return z, b, gamma
