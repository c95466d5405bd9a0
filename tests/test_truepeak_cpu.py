"""CPU: the true-peak meter's rule (tests/truepeak_model.py) against the facts the frozen table was checked by, the model's
state form against the model over a whole signal, and the engine's host side - the table (ac3mi_truepeak_tables), the ceiling
(ac3mi_truepeak_ceiling), the host meter (ac3mi_truepeak_host) and the host read-out (ac3mi_truepeak_read), which run the rule
code the kernels run - against the model, byte for byte.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _harness as H
from tests import truepeak_model as M

ROLES6 = [1, 1, 1, 0, 2, 2]


def _host(roles, pcm, cuts=None, state=None):
    """ac3mi_truepeak_host over pcm [n][C] in calls of `cuts` frames -> the state record"""
    pkg = H.pkg()
    f = 0
    for n in cuts or (pcm.shape[0] // 1536,):
        state = pkg.truepeak_host(roles, pcm[1536 * f:1536 * (f + n)], state)
        f += n
    assert 1536 * f == pcm.shape[0]
    return np.frombuffer(state, M.STATE_DTYPE)[0]


def _same_result(got, want, name=""):
    for k in ("true_peak", "true_peak_index", "true_peak_slot", "sample_peak", "sample_peak_slot", "full_scale", "samples", "flags"):
        assert int(got[k]) == want[k], (name, k, int(got[k]), want[k])
    assert [int(v) for v in got["slot_true_peak"]] == want["slot_true_peak"], name
    assert [int(v) for v in got["slot_sample_peak"]] == want["slot_sample_peak"], name
    assert np.all(np.asarray(got["reserved"]) == 0), name
    for k in ("dbtp", "dbfs"):                          # informative floats: one float32 step
        assert abs(float(got[k]) - want[k]) <= float(np.spacing(np.float32(abs(want[k])))), (name, k, float(got[k]), want[k])


def test_structs_and_exports():
    pkg = H.pkg()
    assert pkg.capi.truepeak_result_dtype().itemsize == ctypes.sizeof(pkg.capi.TruePeakResultC) == 96
    assert pkg.truepeak_state_bytes() == M.STATE_DTYPE.itemsize == 264 and pkg.truepeak_state_bytes() % 8 == 0
    lib = pkg.load_library()
    for name in ("ac3mi_truepeak_state_bytes", "ac3mi_truepeak_tables", "ac3mi_truepeak_ceiling", "ac3mi_truepeak_batch",
                 "ac3mi_truepeak_read_batch", "ac3mi_truepeak_read", "ac3mi_truepeak_host"):
        assert hasattr(lib, name) and name in pkg.declared_symbols()
    # the batched calls refuse a null context before anything else (no GPU needed to say so)
    assert lib.ac3mi_truepeak_batch(None, 6, None, None, 0, 1, None) == -1
    assert lib.ac3mi_truepeak_read_batch(None, None, 0, 0, None) == -1
    assert lib.ac3mi_truepeak_tables(None) == -1


def test_table_and_its_facts():
    """the engine's table is the model's; phase sums 8205 / 7971 / 7971 / 8205, absolute sums 11749 / 16571, phases 2 and 3
    mirror 1 and 0, the first coefficients are Annex 2's first three times 8192, and no phase can leave an int32"""
    h = H.pkg().truepeak_tables()
    assert h.dtype == np.int16 and h.shape == (4, 12) and np.array_equal(h, M.H)
    assert M.H.sum(axis=1).tolist() == [8205, 7971, 7971, 8205]
    assert np.abs(M.H).sum(axis=1).tolist() == [11749, 16571, 16571, 11749]
    assert np.array_equal(M.H[2], M.H[1][::-1]) and np.array_equal(M.H[3], M.H[0][::-1])
    assert (M.H[0][:3] / 8192.0).tolist() == [0.0017089843750, 0.0109863281250, -0.0196533203125]
    assert 32768 * int(np.abs(M.H).sum(axis=1).max()) == 542998528 < 2 ** 31


def test_interpolator_against_the_analytic_sine():
    """phase p of a sampled sine lies on the sine at t = n - 5.875 + p / 4, within 0.03 of full scale (the table's own error,
    0.024, rounded up), from 997 Hz to 20 kHz at 48 kHz"""
    n = np.arange(4800)
    worst = {}
    for f in (997.0, 5000.0, 10000.0, 15000.0, 20000.0):
        w = 2.0 * np.pi * f / 48000.0
        x = np.round(32767.0 * np.sin(w * n + 0.3)).astype(np.int64)
        y = M.oversample(x).reshape(-1, 4)[11:] / M.UNIT
        t = n[11:, None] - 5.875 + np.arange(4)[None, :] / 4.0
        worst[f] = float(np.max(np.abs(y - np.sin(w * t + 0.3))))
        assert worst[f] <= 0.03, (f, worst[f])
    print("largest distance from the analytic sine, of full scale:", worst)


def test_quarter_rate_sine_at_45_degrees():
    """a full-scale fs/4 sine sampled at 45 degrees: every sample is 3.01 dB under full scale, the true peak is not"""
    x = np.round(32767.0 * np.sin(2.0 * np.pi * np.arange(1536) / 4.0 + np.pi / 4.0)).astype(np.int16)
    r = M.Meter([1]).push(x[:, None]).read()
    print("fs/4 at 45 degrees: %.4f dBTP, %.4f dBFS" % (r["dbtp"], r["dbfs"]))
    assert 0.0 < r["dbtp"] < 0.1 and abs(r["dbfs"] + 3.01) < 0.005
    got = H.pkg().truepeak_read(_host([1], x[:, None]).tobytes())
    assert 0.0 < float(got["dbtp"]) < 0.1 and abs(float(got["dbfs"]) + 3.01) < 0.005


def test_state_form_equals_the_whole_signal():
    """20 frames through the state form, frame by frame and in uneven cuts = the whole signal at once, exactly"""
    frames = 20
    pcm = M.noise(11, frames, 3, (0.3, 1.0, 0.7), loud_slot=1)
    roles = [1, 0, 2]
    want = [M.whole(pcm[:, c]) if roles[c] else dict(true_peak=0, index=0, sample_peak=0, full_scale=0) for c in range(3)]
    by_frame, uneven = M.Meter(roles), M.Meter(roles)
    for f in range(frames):
        by_frame.push(pcm[1536 * f:1536 * (f + 1)])
    at = 0
    for n in (1, 10, 11, 12, 1535, 1537, 3000, 23, 7, 20000):
        uneven.push(pcm[at:at + n])
        at += n
    uneven.push(pcm[at:])
    for m in (by_frame, uneven):
        assert m.samples == frames * 1536
        for c in range(3):
            assert (m.true_peak[c], m.index[c], m.sample_peak[c], m.full_scale[c]) == tuple(want[c][k] for k in ("true_peak", "index", "sample_peak", "full_scale")), c
        assert np.all(m.hist[1] == 0) and np.array_equal(m.hist[0], pcm[-11:, 0]) and m.measured == 0b101
    assert by_frame.record().tobytes() == uneven.record().tobytes()
    assert want[0]["true_peak"] > want[0]["sample_peak"] << 13      # the interpolated peak overshoots the samples


def _cases():
    """(name, roles, pcm int16 [n][C])"""
    out = [("%d channels" % C, ([1, 1, 1, 0, 2, 2][:C] if C > 3 else [1] * C), M.noise(40 + C, 3, C, (0.9, 0.5, 0.25, 1.0, 0.1, 0.7), loud_slot=3 if C > 3 else None))
           for C in range(1, 7)]
    out.append(("an unmeasured loud slot", [1, 0], M.noise(50, 2, 2, (0.2, 1.0), loud_slot=1)))
    worst = np.zeros((2 * 1536, 2), np.int16)
    worst[1536 - 5:1536 + 7, 0] = M.worst_case()        # across a frame boundary
    out.append(("worst case", [1, 1], worst))
    out.append(("all -32768", [1, 2, 1], np.full((2 * 1536, 3), -32768, np.int16)))
    out.append(("all zero", ROLES6, np.zeros((2 * 1536, 6), np.int16)))
    burst = np.zeros((3 * 1536, 2), np.int16)
    shape = np.array([900, -12000, 32767, -32768, 15000, -700], np.int16)
    for at in (700, 1536 + 1530):
        burst[at:at + 6, 1] = shape
    out.append(("two identical bursts", [1, 1], burst))
    return out


def test_host_meter_against_the_model():
    """ac3mi_truepeak_host = the model, byte for byte in the state, in one call and frame by frame"""
    seen = {}
    for name, roles, pcm in _cases():
        m = M.Meter(roles).push(pcm)
        want = m.record()
        for cuts in (None, (1,) * (pcm.shape[0] // 1536)):
            got = _host(roles, pcm, cuts)
            assert got.tobytes() == want.tobytes(), (name, cuts, got, want)
        seen[name] = m
    m = seen["worst case"]
    assert m.true_peak[0] == 32768 * 12271 + 32767 * 4300 == M.whole(_cases()[7][2][:, 0])["true_peak"] < 2 ** 31
    assert m.index[0] == 4 * (1536 + 6) + 1 and m.full_scale[0] == 12 and m.true_peak[1] == 0
    m = seen["all -32768"]
    ramp_up = M.whole(np.full(3072, -32768))["true_peak"]      # the first 11 instants see partial sums of the table, some larger than the whole
    assert m.true_peak == [ramp_up] * 3 + [0] * 3 and 32768 * 8205 <= ramp_up < 2 ** 31
    assert m.full_scale[:3] == [3072] * 3 and m.sample_peak[:3] == [32768] * 3 and max(m.index) < 4 * 12
    m = seen["all zero"]
    assert m.true_peak == [0] * 6 and m.index == [0] * 6 and m.samples == 3072 and m.measured == 0b110111
    m = seen["two identical bursts"]
    assert m.true_peak[1] > 0 and 4 * 700 <= m.index[1] < 4 * 720 and m.full_scale[1] == 4
    m = seen["an unmeasured loud slot"]
    assert m.true_peak[1] == 0 and m.sample_peak[1] == 0 and np.all(m.hist[1] == 0) and m.measured == 1
    # argument errors: the state is untouched
    lib = H.pkg().load_library()
    state = ctypes.create_string_buffer(b"\xa5" * 264, 264)
    pcm = np.zeros((1536, 6), np.int16)
    role = (ctypes.c_uint8 * 6)(*ROLES6)
    for ch, r, p, fr, st in ((0, role, pcm.ctypes.data, 1, state), (7, role, pcm.ctypes.data, 1, state), (6, None, pcm.ctypes.data, 1, state),
                             (6, role, None, 1, state), (6, role, pcm.ctypes.data + 1, 1, state), (6, role, pcm.ctypes.data, 0, state),
                             (6, role, pcm.ctypes.data, 1, None)):
        assert lib.ac3mi_truepeak_host(ch, r, p, fr, st) == -1
    assert state.raw == b"\xa5" * 264


def _read_states():
    """(name, record, ceiling) for the read-out"""
    def rec(**kw):
        r = np.zeros((), M.STATE_DTYPE)
        for k, v in kw.items():
            r[k] = v
        return r
    noise = M.Meter(ROLES6).push(M.noise(60, 2, 6, (0.9, 0.5, 0.25, 1.0, 0.1, 0.7), loud_slot=3)).record()
    peak = int(noise["true_peak"].max())
    return [("new stream", rec(), 0),
            ("nothing measured", rec(samples=1536), 0),
            ("silence", rec(samples=1536, measured=3), 1000),
            ("noise", noise, 0),
            ("ceiling at the peak: not over", noise, peak),
            ("ceiling one under: over", noise, peak - 1),
            ("same value, the earlier index wins", rec(samples=9000, measured=7, true_peak=[500, 500, 499, 0, 0, 0], index=[40, 39, 1, 0, 0, 0],
                                                       sample_peak=[7, 9, 9, 0, 0, 0]), 0),
            ("same value and index, the lower slot wins", rec(samples=9000, measured=0x3f, true_peak=[3, 500, 500, 0, 500, 0], index=[0, 39, 39, 0, 39, 0],
                                                              sample_peak=[0, 1, 1, 0, 1, 0], full_scale=[0, 0xfffffff0, 0x20, 0, 0, 0]), 499),
            ]


def test_host_read_out_against_the_model():
    pkg = H.pkg()
    seen = {}
    for name, r, ceiling in _read_states():
        got = pkg.truepeak_read(r.tobytes(), ceiling)
        want = M.read_record(r, ceiling)
        _same_result(got, want, name)
        seen[name] = want
    assert seen["new stream"]["flags"] == seen["nothing measured"]["flags"] == M.EMPTY and seen["silence"]["flags"] == 0
    assert seen["silence"]["dbtp"] == seen["silence"]["dbfs"] == -200.0
    assert seen["ceiling at the peak: not over"]["flags"] == 0 and seen["ceiling one under: over"]["flags"] == M.OVER
    assert seen["noise"]["true_peak_slot"] != 3 and seen["noise"]["slot_true_peak"][3] == 0
    assert (seen["same value, the earlier index wins"]["true_peak_slot"], seen["same value, the earlier index wins"]["sample_peak_slot"]) == (1, 1)
    tie = seen["same value and index, the lower slot wins"]
    assert tie["true_peak_slot"] == 1 and tie["full_scale"] == 0xffffffff and tie["flags"] == M.OVER
    assert pkg.truepeak_ceiling(0) == 2 ** 28 and pkg.truepeak_ceiling(-1) == M.ceiling(-1) == int(2 ** 28 * 10 ** -0.05)
    assert pkg.truepeak_ceiling(-2) == M.ceiling(-2) and pkg.truepeak_ceiling(100) == 0xffffffff and pkg.truepeak_ceiling(-400) == 0
    lib = pkg.load_library()
    res = pkg.capi.TruePeakResultC()
    assert lib.ac3mi_truepeak_read(None, 0, ctypes.byref(res)) == -1 and lib.ac3mi_truepeak_read(bytes(264), 0, None) == -1


def test_host_twins_under_the_sanitisers(tmp_path):
    """tests/truepeak_c/truepeak_main.c with a host-only translation of csrc/truepeak.hip (truepeak_rule.h's meter and
    read-out), both built with -fsanitize=address,undefined and run on the CPU: the model's states and results, and not a word
    from either sanitiser"""
    exe = H.build_sanitised([os.path.join(H.ROOT, "tests", "truepeak_c", "truepeak_main.c"), os.path.join(H.CSRC, "truepeak.hip")], str(tmp_path / "truepeak_main"), includes=[os.path.join(H.ROOT, "include")])
    for i, (name, roles, pcm) in enumerate(_cases()):
        path = tmp_path / ("pcm%d.bin" % i)
        path.write_bytes(pcm.astype("<i2").tobytes())
        m = M.Meter(roles).push(pcm)
        ceiling = max(m.true_peak) - 1 if i % 2 and max(m.true_peak) > 1 else 0
        r = subprocess.run([exe, str(pcm.shape[1]), "".join(str(v) for v in roles), str(path), str(ceiling)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.stdout, r.stderr)
        line, state = r.stdout.strip().split("\n")
        f = line.split()
        assert f[0] == "result" and len(f) == 22 and f[9] == "0"
        want = m.read(ceiling)
        got = [int(v) for v in f[1:]]
        assert got[:8] == [want[k] for k in ("true_peak", "true_peak_index", "true_peak_slot", "sample_peak", "sample_peak_slot", "full_scale",
                                             "samples", "flags")], (name, got, want)
        assert got[9:15] == want["slot_true_peak"] and got[15:21] == want["slot_sample_peak"], name
        assert bytes.fromhex(state.split()[1]) == m.record().tobytes(), name
    # a file that is not whole frames is refused by the program, not read past
    short = tmp_path / "short.bin"
    short.write_bytes(bytes(3072 * 2 - 2))
    assert subprocess.run([exe, "2", "11", str(short), "0"], capture_output=True, text=True).returncode == 2
