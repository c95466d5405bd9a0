"""CPU: the loudness range meter's rule (tests/loudness_range_model.py) - its content, EBU Tech 3342's own synthetic cases, the
binned read-out against the plain list-based one - and the engine's host side: ac3mi_loudness_range_read, which runs the rule
code the kernels run, against the model field for field, in the library and in a stand-alone C program under the
sanitisers.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _harness as H
from tests import loudness_model as M
from tests import loudness_range_content as C
from tests import loudness_range_model as R

MARGIN = 1e-6                           # no decision of the content may hang on less than this (relative)


def _fixtures():
    """(name, RangeMeter) of every stream the tests below and the GPU tests meter"""
    out = [("main %d Hz stream %d" % (fs, s), m) for fs, (_, meters) in C.main().items() for s, m in enumerate(meters)]
    out += [("%d channels stream %d" % (len(C.CHANNEL_ROLES[f]), s), m) for f in C.CHANNEL_FLAGS for s, m in enumerate(C.channels(f)[3])]
    out += [("sine %s" % (levels,), m) for levels, _, _, m in C.sines()]
    return out


def test_structs_and_exports():
    pkg = H.pkg()
    assert pkg.capi.loudness_range_result_dtype().itemsize == ctypes.sizeof(pkg.capi.LoudnessRangeResultC) == 48
    assert pkg.loudness_range_state_bytes() == R.RANGE_STATE_DTYPE.itemsize == 3872
    assert pkg.loudness_state_bytes() == M.STATE_DTYPE.itemsize            # the loudness state is what it was
    lib = pkg.load_library()
    for name in ("ac3mi_loudness_range_state_bytes", "ac3mi_loudness_range_batch", "ac3mi_loudness_range_read_batch",
                 "ac3mi_loudness_range_read"):
        assert hasattr(lib, name) and name in pkg.declared_symbols()
    assert [pkg.loudness_roles(f) for f in C.CHANNEL_FLAGS] == [C.CHANNEL_ROLES[f] for f in C.CHANNEL_FLAGS]


def test_content_decides_nothing_on_a_rounding():
    """(the model alone) no 3 s block within 1e-6 relative of a bin edge, no relative gate within 1e-6 of one; streams in which
    the relative gate removes blocks, streams in which the absolute gate does; three or more different lra_tenths"""
    reads = []
    for name, m in _fixtures():
        r = m.range_read()
        reads.append(r)
        assert m.range_margin() > MARGIN, (name, m.range_margin())
        assert r["flags"] == 0 and r["blocks"] == m.hop_count - 29 > 0, name
    for fs, (_, meters) in C.main().items():
        rd = [m.range_read() for m in meters]
        print("%d Hz: margin %.3g, %d blocks, at or above the absolute gate %s, counted %s, lra_tenths %s" %
              (fs, min(m.range_margin() for m in meters), rd[0]["blocks"], [r["blocks_abs"] for r in rd], [r["blocks_rel"] for r in rd],
               [r["lra_tenths"] for r in rd]))
        assert [r["blocks"] for r in rd] == [C.F_MAIN * 1536 // (fs // 10) - 29] * C.S_MAIN and rd[0]["blocks"] == {48000: 73, 44100: 82, 32000: 124}[fs]
        assert sum(r["blocks_abs"] > r["blocks_rel"] > 0 for r in rd) >= 6
        assert sum(r["blocks"] > r["blocks_abs"] for r in rd) >= 3
        assert len({r["lra_tenths"] for r in rd}) >= 3
        assert all(m.ring_pos == m.r_hops % 30 and m.r_hops >= 90 for m in meters)          # the ring wrapped three times
    assert len({r["lra_tenths"] for r in reads}) >= 3


def test_tech_3342_synthetic_cases():
    """the Recommendation's own four cases, generated: a 1 kHz stereo sine at 32 kHz in plateaus of 20 s, each level 0.05 dB
    down so that the plateaus lie mid-bin; lra_tenths within Tech 3342's +- 1 LU of the expected range"""
    for levels, want, _, m in C.sines():
        r, p = m.range_read(), m.range_plain()
        print("%s: lra_tenths %d (expected %d +- 10), plain %.4f LU, %d blocks, %d counted" % (levels, r["lra_tenths"], want, p["lra"], r["blocks"], r["blocks_rel"]))
        assert r["blocks"] == 20 * len(levels) * 10 - 29
        assert abs(r["lra_tenths"] - want) <= 10, levels
        assert abs(p["lra"] - 0.1 * want) <= 1.0, levels


def test_bins_agree_with_the_plain_rule():
    """wherever no counted block lies in the bin the relative gate cuts, the bins count the blocks the plain rule counts and
    both percentiles floor into 0.1 LU bins: |0.1 lra_tenths - plain| < 0.1 LU"""
    worst, seen = 0.0, 0
    for name, m in _fixtures():
        r, p = m.range_read(), m.range_plain()
        assert abs(r["gamma"] / p["gamma"] - 1.0) < 1e-12, name
        if r["cut_count"]:
            continue
        seen += 1
        assert r["blocks_rel"] == p["blocks_rel"], name
        d = abs(0.1 * r["lra_tenths"] - p["lra"])
        worst = max(worst, d)
        assert d < 0.1, (name, r["lra_tenths"], p["lra"])
    print("largest |0.1 lra_tenths - plain LRA| over %d streams: %.4f LU" % (seen, worst))
    assert seen >= 27


def test_the_bin_the_gate_cuts():
    """sixty blocks from -20 to -10 LUFS and six in the one bin that holds the relative gate, three of them under it: the bins
    keep all six, the plain rule the three above the gate.  The three kept blocks lie at the bottom of the sorted list, so
    they move each percentile down by at most three ranks; the range moves by no more than the larger of those two moves,
    plus the 0.1 LU of the bins"""
    z, b, gamma = C.cut_bin_blocks()
    six = z[30:36]
    assert M.EDGES[b] < gamma < M.EDGES[b + 1] and all(M.bin_of(v) == b for v in six)
    below = int(np.sum(six < gamma))
    assert below == 3
    m = C.meter_of_blocks(z)
    r, p = m.range_read(), m.range_plain()
    assert r["cut"] == b and r["cut_count"] == 6 and p["blocks_rel"] == 66 - below and r["blocks_rel"] == 66
    kept = np.sort(z)                                   # the list the bins read the percentiles of
    d_lo = 10.0 * np.log10(p["low"] / kept[R.rank(66, 10)])
    d_hi = 10.0 * np.log10(p["high"] / kept[R.rank(66, 95)])
    diff = 0.1 * r["lra_tenths"] - p["lra"]
    print("bin %d cut at %.6g: %d of 6 below; lra_tenths %d, plain %.4f LU, difference %.4f LU (the 10th percentile moved %.4f LU, the 95th %.4f)" %
          (b, gamma, below, r["lra_tenths"], p["lra"], diff, d_lo, d_hi))
    assert d_lo >= 0 and d_hi >= 0 and abs(diff) < 0.1 + max(d_lo, d_hi) < 0.8


def _states():
    """(name, state record) for the host read-out"""
    rng = np.random.default_rng(7)
    out = [("empty", C.meter_of_blocks([]).range_record()),
           ("29 hops", C.meter_of_blocks([], hops=29).range_record()),
           ("n = 1", C.meter_of_blocks([0.01]).range_record()),
           ("n = 2", C.meter_of_blocks([0.01, 0.02]).range_record()),
           ("sub-gate only", C.meter_of_blocks([M.EDGES[0] * 0.5, M.EDGES[0] * 0.999999, 1e-12]).range_record()),
           ("every block in bin 899", C.meter_of_blocks([M.EDGES[900] * 2.0, M.EDGES[899] * 1.01, 120.0, 300.0]).range_record()),
           ("bins 0 and 899", C.meter_of_blocks([M.EDGES[0] * 1.01] * 3 + [M.EDGES[900]] * 40).range_record()),
           ("gated", C.meter_of_blocks(list(10.0 ** rng.uniform(-3.0, -1.0, 300)) + list(10.0 ** rng.uniform(-6.5, -4.0, 200))).range_record()),
           ("wide", C.meter_of_blocks(list(10.0 ** rng.uniform(-4.0, 0.5, 1000))).range_record()),
           ("gate cuts a bin", C.meter_of_blocks(C.cut_bin_blocks()[0]).range_record())]
    out += [("main 44100 Hz stream %d" % s, m.range_record()) for s, m in enumerate(C.main()[44100][1])]
    garbage = np.frombuffer(b"\xff" * R.RANGE_STATE_DTYPE.itemsize, R.RANGE_STATE_DTYPE)[0]
    out.append(("all 0xff", garbage))
    big = C.meter_of_blocks([0.01, 0.02]).range_record()
    big["count"][:] = 0xffffffff                        # more blocks than blocks_rel holds: 64-bit ranks, a saturated count
    out.append(("every count at its maximum", big))
    odd = C.meter_of_blocks([0.01, 0.5]).range_record()
    odd["ring_pos"], odd["sum_abs"], odd["max_short"] = 0xfffffff0, -1.0, -3.0
    out.append(("a negative sum", odd))
    return out


def _check(name, got, want):
    """got: field -> value (the floats as float32 / float64 numbers) against the model's read-out, field for field"""
    for k in ("blocks", "blocks_abs", "blocks_rel", "lra_tenths", "low_bin", "high_bin", "flags"):
        assert int(got[k]) == int(want[k]), (name, k, got[k], want[k])
    for k in ("lra", "low_lkfs", "high_lkfs"):          # from the integers: the same bits
        assert np.float32(got[k]).tobytes() == np.float32(want[k]).tobytes(), (name, k, got[k], want[k])
    assert np.float64(got["max_short_energy"]).tobytes() == np.float64(want["max_short_energy"]).tobytes(), name
    # (one float32 step: two double log10 a rounding apart may round to neighbouring floats)
    assert abs(float(got["max_short_lkfs"]) - float(want["max_short_lkfs"])) <= 2.0 ** -23 * abs(float(want["max_short_lkfs"])), name


def test_host_read_out_against_the_model():
    pkg = H.pkg()
    seen = {}
    for name, rec in _states():
        got = pkg.loudness_range_read(rec.tobytes())
        assert np.all(got["reserved"] == 0), name
        want = R.read_record(rec)
        _check(name, got, want)
        seen[name] = want
    w = seen["a negative sum"]                          # a gate below every bin: both blocks count; a maximum that has no logarithm
    assert (w["flags"], w["blocks_rel"], w["lra_tenths"]) == (0, 2, M.bin_of(0.5) - M.bin_of(0.01)) and float(w["max_short_lkfs"]) == -200.0
    for name in ("empty", "29 hops", "sub-gate only", "all 0xff"):
        w = seen[name]
        assert (w["flags"], w["lra_tenths"], w["low_bin"], w["high_bin"], float(w["lra"]), float(w["low_lkfs"]), float(w["high_lkfs"])) == (R.EMPTY, 0, 0, 0, 0.0, -70.0, -70.0), name
    assert float(seen["empty"]["max_short_lkfs"]) == float(seen["all 0xff"]["max_short_lkfs"]) == -200.0
    assert seen["sub-gate only"]["blocks"] == 3 and seen["sub-gate only"]["blocks_abs"] == 0 and float(seen["sub-gate only"]["max_short_lkfs"]) < -70.0
    assert (seen["n = 1"]["blocks_rel"], seen["n = 1"]["lra_tenths"], seen["n = 1"]["low_bin"]) == (1, 0, M.bin_of(0.01))
    assert seen["n = 2"]["lra_tenths"] == M.bin_of(0.02) - M.bin_of(0.01) == 30              # ranks 0 and 1
    w = seen["every block in bin 899"]
    assert (w["blocks_rel"], w["low_bin"], w["high_bin"], w["lra_tenths"]) == (4, 899, 899, 0) and abs(float(w["high_lkfs"]) - 19.95) < 1e-5
    assert (seen["bins 0 and 899"]["blocks_abs"], seen["bins 0 and 899"]["blocks_rel"], seen["bins 0 and 899"]["low_bin"]) == (43, 40, 899)
    assert 0 < seen["gated"]["blocks_rel"] < seen["gated"]["blocks_abs"] == 500 and seen["gated"]["lra_tenths"] > 100
    w = seen["every count at its maximum"]
    assert w["blocks_rel"] == 0xffffffff and w["flags"] == 0 and w["high_bin"] > w["low_bin"] > 0


def test_host_entry_point_refuses_bad_arguments():
    pkg = H.pkg()
    lib = pkg.load_library()
    res = pkg.capi.LoudnessRangeResultC()
    state = bytes(pkg.loudness_range_state_bytes())
    assert lib.ac3mi_loudness_range_read(None, ctypes.byref(res)) == -1 and lib.ac3mi_loudness_range_read(state, None) == -1
    assert lib.ac3mi_loudness_range_read(state, ctypes.byref(res)) == 0 and res.flags == R.EMPTY
    try:
        pkg.loudness_range_read(state[:-1])
        assert False, "a short state was taken"
    except ValueError:
        pass
    # the batched calls refuse a null context before anything else (no GPU needed to say so)
    assert lib.ac3mi_loudness_range_batch(None, None, None, 0, 1, None, None) == -1
    assert lib.ac3mi_loudness_range_read_batch(None, None, 0, None) == -1


def test_host_read_out_under_the_sanitisers(tmp_path):
    """tests/loudness_range_c/range_main.c with a host-only translation of csrc/loudness.hip, both built with
    -fsanitize=address,undefined and run on the CPU over every state above, the all-0xff garbage among them, from stdin: the
    model's results, and not a word from either sanitiser"""
    exe = H.build_sanitised([os.path.join(H.ROOT, "tests", "loudness_range_c", "range_main.c"), os.path.join(H.CSRC, "loudness.hip")], str(tmp_path / "range_main"), includes=[os.path.join(H.ROOT, "include")])
    states = _states()
    r = subprocess.run([exe], input=b"".join(rec.tobytes() for _, rec in states), capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout, r.stderr)
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(states)
    for (name, rec), line in zip(states, lines):
        f = line.split()
        assert f[0] == "result" and len(f) == 14 and f[13] == "0", (name, line)
        got = dict(max_short_energy=np.array([int(f[1], 16)], np.uint64).view(np.float64)[0])
        for k, v in zip(("lra", "low_lkfs", "high_lkfs", "max_short_lkfs"), f[2:6]):
            got[k] = np.array([int(v, 16)], np.uint32).view(np.float32)[0]
        for k, v in zip(("blocks", "blocks_abs", "blocks_rel", "lra_tenths", "low_bin", "high_bin", "flags"), f[6:13]):
            got[k] = int(v)
        _check(name, got, R.read_record(rec))
    # input that is not whole states is refused by the program, not read past
    assert subprocess.run([exe], input=bytes(100), capture_output=True).returncode == 2
