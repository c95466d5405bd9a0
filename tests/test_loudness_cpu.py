"""CPU: the BS.1770 meter's rule (tests/loudness_model.py) against the standard's own figures, the model's state form against
the model over a whole signal, the 900-bin read-out against plain gating, and the engine's host side - the frozen tables
(ac3mi_loudness_tables), the slot roles (ac3mi_loudness_roles) and the host read-out (ac3mi_loudness_read), which runs the
rule code the kernels run - against the model.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _harness as H
from tests import loudness_model as M


def _lu(a, b):
    return abs(10.0 * np.log10(a / b))


def test_structs_and_exports():
    pkg = H.pkg()
    assert pkg.capi.loudness_result_dtype().itemsize == ctypes.sizeof(pkg.capi.LoudnessResultC) == 40
    assert ctypes.sizeof(pkg.capi.LoudnessDescC) == 16
    assert pkg.loudness_state_bytes() == M.STATE_DTYPE.itemsize and pkg.loudness_state_bytes() % 8 == 0
    lib = pkg.load_library()
    for name in ("ac3mi_loudness_state_bytes", "ac3mi_loudness_roles", "ac3mi_loudness_tables", "ac3mi_loudness_batch",
                 "ac3mi_loudness_read_batch", "ac3mi_loudness_read", "ac3mi_loudness_words_batch"):
        assert hasattr(lib, name) and name in pkg.declared_symbols()


def test_coefficients_and_tables():
    """the design reproduces BS.1770's 48 kHz table to its printed digits; the engine's frozen literals, bin edges and
    dialnorm thresholds are the model's to 1e-12 relative at every rate"""
    c = M.coefs(48000)
    assert np.max(np.abs(c[[0, 1, 2, 3, 4, 8, 9]] - np.array(M.BS1770_48K))) < 1e-12
    assert tuple(c[5:8]) == (1.0, -2.0, 1.0)
    for fs in M.RATES:
        coef, edges, thr = H.pkg().loudness_tables(fs)
        assert np.max(np.abs(coef / M.coefs(fs) - 1.0)) < 1e-12, fs
        assert edges.shape == (901,) and np.max(np.abs(edges / M.EDGES - 1.0)) < 1e-12
        assert thr.shape == (30,) and np.max(np.abs(thr / M.THRESHOLDS - 1.0)) < 1e-12
    assert np.all(np.diff(M.EDGES) > 0) and abs(M.lkfs(M.EDGES[0]) + 70.0) < 1e-9 and abs(M.lkfs(M.EDGES[900]) - 20.0) < 1e-9
    lib = H.pkg().load_library()
    for bad in (0, 24000, 22050, 16000, 11025, 8000, 96000):
        assert lib.ac3mi_loudness_tables(bad, None, None, None) == -1
    assert lib.ac3mi_loudness_tables(48000, None, None, None) == 0


def test_roles_follow_the_s16_layouts():
    """WAVE order: FL FR FC LFE BL BR and its subsets, as ac3mi_decode_s16_batch interleaves them per output flags"""
    pkg = H.pkg()
    want = {1: [1], 2: [1, 1], 0: [1, 1], 10: [1, 1], 8: [1], 3: [1, 1, 1], 4: [1, 1, 2], 5: [1, 1, 1, 2], 6: [1, 1, 2, 2], 7: [1, 1, 1, 2, 2],
            7 | 16: [1, 1, 1, 0, 2, 2], 2 | 16: [1, 1, 0], 6 | 16: [1, 1, 0, 2, 2], 5 | 16: [1, 1, 1, 0, 2], 4 | 16: [1, 1, 0, 2],
            3 | 16: [1, 1, 1, 0], 1 | 16: [1, 0]}
    for flags, roles in want.items():
        assert pkg.loudness_roles(flags) == roles, flags
    role = (ctypes.c_uint8 * 6)()
    assert pkg.load_library().ac3mi_loudness_roles(11, role) == -1 and pkg.load_library().ac3mi_loudness_roles(7, None) == -1


def test_calibration_sine():
    """BS.1770's calibration statement: a 0 dBFS 997 Hz sine on one front channel reads -3.01 LKFS; on a surround slot it
    reads 10 log10(1.41) LU more"""
    n = 3 * 48000
    x = np.round(32767.0 * np.sin(2.0 * np.pi * 997.0 * np.arange(n) / 48000.0)) / 32768.0
    y, _ = M.kweight(x, M.coefs(48000))
    front, surround = M.Meter(48000, [1]), M.Meter(48000, [2])
    front.push_power(y * y)
    surround.push_power(1.41 * y * y)
    a, b = front.read(), surround.read()
    print("997 Hz 0 dBFS: %.6f LKFS front, %.6f surround" % (a["lkfs"], b["lkfs"]))
    assert a["blocks"] == 27 and a["blocks_rel"] == 27 and abs(a["lkfs"] + 3.01) <= 0.01
    assert abs((b["lkfs"] - a["lkfs"]) - 10.0 * np.log10(1.41)) < 1e-6
    assert a["dialnorm"] == 3 and b["dialnorm"] == 2


def test_state_form_equals_the_whole_signal():
    """frame by frame through the state form = the whole signal at once: the same blocks in the same bins (the hop sums are
    grouped differently, so energies agree to rounding)"""
    fs, roles, frames = 44100, [1, 0, 2], 20
    pcm = M.programme(11, frames, 3, 0.3, loud_slot=1)
    whole, streamed = M.Meter(fs, roles), M.Meter(fs, roles)
    whole.push(pcm)
    for f in range(frames):
        streamed.push(pcm[1536 * f:1536 * (f + 1)])
    assert whole.blocks == streamed.blocks == frames * 1536 // 4410 - 3 and whole.blocks_abs == streamed.blocks_abs
    assert np.array_equal(whole.count, streamed.count) and streamed.pos == whole.pos == frames * 1536 % 4410
    assert np.max(np.abs(np.array(whole.z) / np.array(streamed.z) - 1.0)) < 1e-12
    assert np.allclose(whole.sum, streamed.sum, rtol=1e-12, atol=0) and np.allclose(whole.bq, streamed.bq, rtol=1e-12, atol=1e-300)
    assert np.all(streamed.bq[1] == 0)                  # the unmeasured slot has no filter state


def test_bins_agree_with_plain_gating():
    """nine noise programmes with a quiet and a loud part per rate: the relative gate removes blocks, and the bins' read-out
    is the plain gating's (no block lies in the bin the gate cuts, or the rule decides it as plain gating does)"""
    amps = (1.0, 0.6, 0.35, 0.2, 0.12, 0.07, 0.04, 0.025, 0.015)      # the quiet part of the quietest still passes the absolute gate
    pcm = np.stack([M.programme(100 + 9 * r + i, 64, 1, amps[i]) for r in range(3) for i in range(9)])
    meters = M.run_batch(pcm, [fs for fs in M.RATES for _ in range(9)], [1])
    for m in meters:
        a, b = m.read(), M.read_plain(m.z)
        removed = a["blocks_abs"] - a["blocks_rel"]
        assert m.blocks == 64 * 1536 // m.hop - 3 and a["blocks_abs"] == m.blocks and removed >= 5
        assert a["blocks_rel"] == b["blocks_rel"] and _lu(a["mean_energy"], b["mean_energy"]) <= 1e-9, (m.fs, a, b)
        assert abs(a["gamma"] / b["gamma"] - 1.0) < 1e-12


def test_the_bin_the_gate_cuts():
    """forty blocks at energy 1 and six spread over the one bin that holds the relative gate, some on either side of it: the
    bins keep or drop the six together, plain gating keeps those above the gate; the two differ by no more than that bin can
    contribute"""
    b = M.bin_of(0.0883)
    for _ in range(4):                                  # the gate depends (slightly) on where the six lie: settle
        six = M.EDGES[b] + (M.EDGES[b + 1] - M.EDGES[b]) * np.array([0.08, 0.22, 0.41, 0.58, 0.77, 0.93])
        z = np.concatenate([np.ones(40), six])
        gamma = 0.1 * z.mean()
        b = M.bin_of(gamma)
    assert M.EDGES[b] < gamma < M.EDGES[b + 1] and M.bin_of(six[0]) == M.bin_of(six[-1]) == b
    below = int(np.sum(six < gamma))
    assert 1 <= below <= 5
    m = M.Meter(48000, [1])
    for v in z:
        k = M.bin_of(v)
        m.count[k] += 1
        m.sum[k] += v
    a, p = M.read_bins(m.count, m.sum), M.read_plain(z)
    assert a["cut"] == b and p["blocks_rel"] == 46 - below and a["blocks_rel"] in (40, 46)
    bound = _lu(1.0, z.mean())                          # none of the six against all of them
    diff = _lu(a["mean_energy"], p["mean_energy"])
    print("bin %d cut at %.6g: %d of 6 below; bins keep %d, plain %d; differ by %.6f LU (bound %.6f)" %
          (b, gamma, below, a["blocks_rel"] - 40, 6 - below, diff, bound))
    assert 0 < diff <= bound < 0.6
    # the rule itself: the bin's own mean against the gate
    assert (a["blocks_rel"] == 46) == (six.mean() >= gamma)


def _states():
    """(name, meter) for the host read-out: bins written directly"""
    def meter(blocks):
        m = M.Meter(48000, [1])
        for v in blocks:
            k = M.bin_of(v)
            m.blocks += 1
            m.max_block = max(m.max_block, v)
            if k >= 0:
                m.blocks_abs += 1
                m.count[k] += 1
                m.sum[k] += v
        m.hop_count = m.blocks + 3 if m.blocks else 0
        return m
    t = M.THRESHOLDS
    rng = np.random.default_rng(5)
    out = [("empty", meter([])),
           ("sub-gate only", meter([M.EDGES[0] * 0.5, M.EDGES[0] * 0.999999, 1e-12])),
           ("clamps at 1", meter([3.0, 2.5, 4.0])),
           ("top bin and beyond", meter([M.EDGES[900] * 2.0, M.EDGES[899] * 1.01, 50.0])),
           ("clamps at 31", meter([t[29] * 0.2, t[29] * 0.25])),
           ("just above a threshold", meter([t[22] * (1 + 1e-9)] * 3)),
           ("just below a threshold", meter([t[22] * (1 - 1e-9)] * 3)),
           ("gated", meter(list(10.0 ** rng.uniform(-3.0, -1.0, 300)) + list(10.0 ** rng.uniform(-6.5, -4.0, 200)))),
           ]
    b = M.bin_of(0.0883)
    six = M.EDGES[b] + (M.EDGES[b + 1] - M.EDGES[b]) * np.array([0.08, 0.22, 0.41, 0.58, 0.77, 0.93])
    out.append(("gate cuts a bin, bin kept or dropped", meter([1.0] * 40 + list(six))))
    out.append(("gate cuts a bin, high blocks", meter([1.0] * 40 + list(six[3:]))))
    return out


def _check_result(name, got, m):
    want = m.read()
    assert int(got["blocks"]) == want["blocks"] and int(got["blocks_abs"]) == want["blocks_abs"], name
    assert int(got["blocks_rel"]) == want["blocks_rel"] and int(got["dialnorm"]) == want["dialnorm"] and int(got["flags"]) == want["flags"], name
    assert float(got["max_block_energy"]) == want["max_block_energy"], name
    if want["flags"]:
        assert float(got["mean_energy"]) == 0.0 and float(got["lkfs"]) == -70.0 and int(got["dialnorm"]) == 31, name
    else:
        assert abs(float(got["mean_energy"]) / want["mean_energy"] - 1.0) < 1e-12, name
        assert abs(float(got["lkfs"]) - want["lkfs"]) < 1e-4, name


def test_host_read_out_against_the_model():
    pkg = H.pkg()
    seen = {}
    for name, m in _states():
        got = pkg.loudness_read(m.record().tobytes())
        assert np.all(got["reserved"] == 0)
        _check_result(name, got, m)
        seen[name] = (int(got["dialnorm"]), int(got["flags"]), int(got["blocks_rel"]), int(got["blocks_abs"]))
    assert seen["empty"][:2] == (31, M.EMPTY) and seen["sub-gate only"] == (31, M.EMPTY, 0, 0)
    assert seen["clamps at 1"][0] == 1 and seen["top bin and beyond"][0] == 1 and seen["clamps at 31"][:2] == (31, 0)
    assert seen["just above a threshold"][0] == 23 and seen["just below a threshold"][0] == 24
    assert 0 < seen["gated"][2] < seen["gated"][3] == 500
    lib = pkg.load_library()
    res = pkg.capi.LoudnessResultC()
    assert lib.ac3mi_loudness_read(None, ctypes.byref(res)) == -1 and lib.ac3mi_loudness_read(bytes(pkg.loudness_state_bytes()), None) == -1
    # the batched calls refuse a null context before anything else (no GPU needed to say so)
    assert lib.ac3mi_loudness_batch(None, None, None, 0, 1, None) == -1
    assert lib.ac3mi_loudness_read_batch(None, None, 0, None) == -1
    assert lib.ac3mi_loudness_words_batch(None, None, 0, 1, 0, None) == -1


def test_host_read_out_under_the_sanitisers(tmp_path):
    """tests/loudness_c/loudness_main.c with a host-only translation of csrc/loudness.hip (loudness_rule.h's read-out), both
    built with -fsanitize=address,undefined and run on the CPU: the model's results, and not a word from either sanitiser"""
    exe = H.build_sanitised([os.path.join(H.ROOT, "tests", "loudness_c", "loudness_main.c"), os.path.join(H.CSRC, "loudness.hip")], str(tmp_path / "loudness_main"), includes=[os.path.join(H.ROOT, "include")])
    for i, (name, m) in enumerate(_states()):
        path = tmp_path / ("state%d.bin" % i)
        path.write_bytes(m.record().tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.stdout, r.stderr)
        f = r.stdout.split()
        assert f[0] == "result" and len(f) == 10 and f[9] == "0"
        got = dict(mean_energy=float(f[1]), max_block_energy=float(f[2]), lkfs=float(f[3]), blocks=int(f[4]), blocks_abs=int(f[5]),
                   blocks_rel=int(f[6]), dialnorm=int(f[7]), flags=int(f[8]))
        _check_result(name, got, m)
    # a file that is not a state is refused by the program, not read past
    short = tmp_path / "short.bin"
    short.write_bytes(bytes(100))
    assert subprocess.run([exe, str(short)], capture_output=True, text=True).returncode == 2
