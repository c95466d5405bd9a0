"""CPU: the true-peak limiter's rule (tests/limit_model.py, on tests/truepeak_model.py's interpolator) - its state form against
the rule over a whole signal, the two bounds the rule promises on named contents - and the engine's host side: the release
step (ac3mi_limit_release_step), the host limiter (ac3mi_limit_host) and the host read-out (ac3mi_limit_read), which run the
rule code the kernels run, against the model byte for byte.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _harness as H
from tests import limit_model as L
from tests import truepeak_model as M

C1, C2, C6 = M.ceiling(-1.0), M.ceiling(-2.0), M.ceiling(-6.0)
STEPS = (1, 350, 3500, 70000, 1 << 20)
NB = 1560


def _host(roles, C, R, pcm, cuts=None):
    """ac3mi_limit_host over pcm [n][C] in calls of `cuts` frames -> (out, the state's bytes)"""
    pkg = H.pkg()
    f, state, outs = 0, None, []
    for n in cuts or (pcm.shape[0] // 1536,):
        out, state = pkg.limit_host(roles, C, R, pcm[1536 * f:1536 * (f + n)], state)
        outs.append(out)
        f += n
    assert 1536 * f == pcm.shape[0]
    return np.concatenate(outs), state


def _same_result(got, want, name=""):
    for k in ("samples", "reduced", "max_detect", "min_gain_q24", "flags"):
        assert int(got[k]) == want[k], (name, k, int(got[k]), want[k])
    assert np.all(np.asarray(got["reserved"]) == 0), name
    for k in ("in_dbtp", "reduction_db"):               # informative floats: one float32 step
        assert abs(float(got[k]) - want[k]) <= float(np.spacing(np.float32(abs(want[k])))), (name, k, float(got[k]), want[k])


def test_structs_and_exports():
    pkg = H.pkg()
    assert pkg.capi.limit_result_dtype().itemsize == ctypes.sizeof(pkg.capi.LimitResultC) == 40
    assert pkg.limit_state_bytes() == L.STATE_DTYPE.itemsize == NB and NB % 8 == 0
    lib = pkg.load_library()
    for name in ("ac3mi_limit_state_bytes", "ac3mi_limit_release_step", "ac3mi_limit_batch", "ac3mi_limit_read_batch", "ac3mi_limit_read",
                 "ac3mi_limit_host"):
        assert hasattr(lib, name) and name in pkg.declared_symbols()
    # the batched calls refuse a null context before anything else (no GPU needed to say so)
    assert lib.ac3mi_limit_batch(None, 6, None, C1, 3496, None, None, 0, 1, None) == -1
    assert lib.ac3mi_limit_read_batch(None, None, 0, None) == -1
    with open(os.path.join(H.ROOT, "include", "ac3mi.h")) as f:
        assert "#define AC3MI_LIMIT_DELAY 77" in f.read() and L.D == 77


def test_release_step():
    pkg = H.pkg()
    assert pkg.limit_release_step(48000, 100.0) == 3496 == -(-(1 << 24) // 4800) == L.release_step(48000, 100.0)
    assert pkg.limit_release_step(48000, 1e9) == 1 and pkg.limit_release_step(48000, 1e-6) == 1 << 20       # clamped at both ends
    assert pkg.limit_release_step(48000, float("nan")) == 1 and pkg.limit_release_step(48000, -5.0) == 1
    assert pkg.limit_release_step(48000, 0.0) == 1 << 20 and pkg.limit_release_step(0, 100.0) == 1 << 20
    for rate, ms in ((44100, 50.0), (32000, 1000.0), (48000, 0.4), (48000, 349.5253333)):
        assert pkg.limit_release_step(rate, ms) == L.release_step(rate, ms), (rate, ms)


def test_scan_form_equals_the_loop():
    """the min-plus scan of r = the literal recursion, with and without a carried r[-1]"""
    rng = np.random.default_rng(5)
    m = np.where(rng.random(5000) < 0.02, rng.integers(0, L.ONE, 5000), L.ONE).astype(np.int64)
    k = np.arange(len(m), dtype=np.int64)
    for R in STEPS:
        for r_prev in (L.ONE, 0, 12345):
            scan = np.minimum(np.minimum(np.minimum.accumulate(m - k * R) + k * R, r_prev + (k + 1) * R), m)
            assert np.array_equal(scan, L.release_loop(m, R, r_prev)), (R, r_prev)


def test_state_form_equals_the_whole_signal():
    """the state form frame by frame and in uneven cuts = limit() over the whole signal: output bytes and record bytes"""
    cuts = (1, 76, 77, 78, 79, 80, 143, 1535, 1537, 11, 12, 3000, 64, 63, 5)
    for name, roles, pcm in (L.contents()[0], L.contents()[6], L.contents()[7]):
        pcm = np.concatenate([pcm, pcm[::-1]])[:7 * 1536]
        if len(pcm) < 7 * 1536:
            pcm = np.concatenate([pcm, np.zeros((7 * 1536 - len(pcm), pcm.shape[1]), np.int16)])
        assert sum(cuts) < len(pcm)
        for C, R in ((C1, 3496), (C6, 1), (C2, 1 << 20)):
            want, g, d = L.limit(pcm, roles, C, R)
            by_frame, uneven = L.Limiter(roles, C, R), L.Limiter(roles, C, R)
            z1 = np.concatenate([by_frame.push(pcm[1536 * f:1536 * (f + 1)]) for f in range(7)])
            at, parts = 0, []
            for n in cuts:
                parts.append(uneven.push(pcm[at:at + n]))
                at += n
            parts.append(uneven.push(pcm[at:]))
            z2 = np.concatenate(parts)
            assert z1.tobytes() == want.tobytes() and z2.tobytes() == want.tobytes(), (name, C, R)
            assert by_frame.record().tobytes() == uneven.record().tobytes(), (name, C, R)
            rec = by_frame.record()
            assert int(rec["samples"]) == len(pcm) and int(rec["reduced"]) == int(np.sum(g < L.ONE)) and int(rec["max_detect"]) == int(d.max())
            assert int(rec["max_reduction"]) == L.ONE - int(g.min()) and np.array_equal(rec["hist"][:pcm.shape[1]], pcm[-80:].T)


def _host_cases():
    """(name, roles, pcm) for the host twin: 1..6 channels with role subsets, then the corners"""
    out = []
    for ch in range(1, 7):
        for roles in ([1] * ch, [[1], [0, 2], [1, 0, 255], [0, 1, 1, 0], [1, 1, 0, 2, 2], [1, 0, 1, 0, 2, 1]][ch - 1]):
            loud = roles.index(0) if 0 in roles else None
            out.append(("%d channels %s" % (ch, roles), roles, M.noise(80 + ch, 2, ch, (1.0, 0.5, 0.25, 1.0, 0.1, 0.7), loud_slot=loud)))
    worst = np.zeros((2 * 1536, 2), np.int16)
    worst[1536 - 5:1536 + 7, 0] = M.worst_case()        # across a frame boundary
    out.append(("worst case across a frame", [1, 1], worst))
    out.append(("all -32768", [1, 2, 1], np.full((2 * 1536, 3), -32768, np.int16)))
    out.append(("silence", [1] * 6, np.zeros((2 * 1536, 6), np.int16)))
    return out


def test_host_limiter_against_the_model():
    """ac3mi_limit_host = the model, output and state byte for byte, in one call and frame by frame; parameter corners"""
    pkg = H.pkg()
    for name, roles, pcm in _host_cases():
        for C, R in ((C1, 3496), (1, 1), (1 << 28, 1 << 20), (C6, 1 << 20), (C2, 1)):
            lim = L.Limiter(roles, C, R)
            want = lim.push(pcm)
            for cuts in (None, (1,) * (pcm.shape[0] // 1536)):
                got, state = _host(roles, C, R, pcm, cuts)
                assert got.tobytes() == want.tobytes(), (name, C, R, cuts)
                assert state == lim.record().tobytes(), (name, C, R, cuts)
            _same_result(pkg.limit_read(state), lim.read(), name)
            if name == "silence":
                assert not want.any() and lim.reduced == 0 and lim.read()["flags"] == 0
            if name == "all -32768" and C == 1:
                assert lim.min_gain == 0 and not want[200:].any()       # C = 1: floor(2^24 / d) is 0 for any audible d
            if C == 1 << 28 and "channels" in name and 0 not in roles:
                assert lim.max_detect >= C or lim.reduced == 0
    # an undetected loud slot comes out delayed, with the stream's gain, without influencing it
    pcm = M.noise(90, 2, 3, (0.2, 1.0, 0.2), loud_slot=1)
    quiet = pcm.copy()
    quiet[:, 1] = 0
    a, sa = _host([1, 0, 1], C6, 3496, pcm)
    b, sb = _host([1, 0, 1], C6, 3496, quiet)
    assert np.array_equal(a[:, (0, 2)], b[:, (0, 2)]) and sa[:600] == sb[:600]
    assert np.array_equal(a[77:, 1], pcm[:-77, 1]) and pkg.limit_read(sa)["reduced"] == 0       # 0.2 of full scale never reaches -6 dBTP
    # argument errors: state and output untouched
    lib = pkg.load_library()
    state = ctypes.create_string_buffer(b"\xa5" * NB, NB)
    pcm = np.zeros((2 * 1536, 6), np.int16)
    out = np.full((2 * 1536, 6), 0x5a5a, np.int16)
    role = (ctypes.c_uint8 * 6)(1, 1, 1, 0, 2, 2)
    ok = dict(ch=6, r=role, C=C1, R=3496, p=pcm.ctypes.data, o=out.ctypes.data, fr=2, st=state)
    for kw in (dict(ch=0), dict(ch=7), dict(r=None), dict(p=None), dict(o=None), dict(p=pcm.ctypes.data + 1), dict(o=out.ctypes.data + 1),
               dict(fr=0), dict(fr=-1), dict(st=None), dict(C=0), dict(C=(1 << 28) + 1), dict(R=0), dict(R=(1 << 20) + 1),
               dict(p=out.ctypes.data + 768 * 12, fr=1), dict(p=out.ctypes.data, o=out.ctypes.data + 2, fr=1)):    # partial overlaps
        a = dict(ok, **kw)
        assert lib.ac3mi_limit_host(a["ch"], a["r"], a["C"], a["R"], a["p"], a["o"], a["fr"], a["st"]) == -1, kw
    assert state.raw == b"\xa5" * NB and np.all(out == 0x5a5a)
    res = pkg.capi.LimitResultC()
    assert lib.ac3mi_limit_read(None, ctypes.byref(res)) == -1 and lib.ac3mi_limit_read(bytes(NB), None) == -1


def test_read_out():
    pkg = H.pkg()

    def rec(**kw):
        r = np.zeros((), L.STATE_DTYPE)
        for k, v in kw.items():
            r[k] = v
        return r
    for name, r in (("new stream", rec()), ("untouched", rec(samples=1536, max_detect=1000)),
                    ("reduced", rec(samples=4000, reduced=17, max_detect=C1 + 5, max_reduction=12345)),
                    ("gain 0", rec(samples=4000, reduced=4000, max_detect=1 << 29, max_reduction=L.ONE))):
        want = L.read_record(r)
        _same_result(pkg.limit_read(r.tobytes()), want, name)
    assert L.read_record(rec())["flags"] == L.EMPTY and L.read_record(rec())["in_dbtp"] == -200.0 and L.read_record(rec())["reduction_db"] == 0.0
    assert L.read_record(rec(samples=9, reduced=1, max_reduction=L.ONE))["reduction_db"] == -200.0
    assert L.read_record(rec(samples=9, reduced=1))["flags"] == L.ACTIVE


def test_bounds_on_named_contents():
    """for every named content, at -1, -2 and -6 dBTP and every release step: the output's sample peak over the detected slots
    <= (C + 4096) >> 13 (proved for all input) and its true peak <= C + 8286 (proved where the gain is constant; on these
    inputs a condition the rule meets - largest excess per content printed)"""
    pkg = H.pkg()
    worst = {}
    for name, roles, pcm in L.contents():
        for C in (C1, C2, C6):
            for R in STEPS:
                z, g, d = L.limit(pcm, roles, C, R)
                sp, tp = L.sample_peak(z, roles), L.true_peak(z, roles)
                worst[name] = max(worst.get(name, -1 << 40), tp - C)
                assert sp <= (C + 4096) >> 13, (name, C, R, sp)
                assert tp <= C + L.PEAK_SLACK, (name, C, R, tp - C)
                assert int(g.max()) <= L.ONE and int(np.abs(z.astype(np.int64)).max()) <= 32768
        got, _ = _host(roles, C6, 1 << 20, pcm)                 # the host twin on the same content, one setting each
        assert got.tobytes() == L.limit(pcm, roles, C6, 1 << 20)[0].tobytes(), name
    print("largest true-peak excess over the ceiling, per content (2^-28 of full scale; the cap is 8286):", worst)
    assert pkg.truepeak_ceiling(-1.0) == C1


def test_host_twins_under_the_sanitisers(tmp_path):
    """tests/limit_c/limit_main.c with a host-only translation of csrc/limit.hip (limit_rule.h's limiter and read-out), both
    built with -fsanitize=address,undefined and run on the CPU: the model's outputs and states, out of place in two calls and
    in place in one, and not a word from either sanitiser"""
    exe = H.build_sanitised([os.path.join(H.ROOT, "tests", "limit_c", "limit_main.c"), os.path.join(H.CSRC, "limit.hip")], str(tmp_path / "limit_main"), includes=[os.path.join(H.ROOT, "include")])
    cases = _host_cases()[::3] + _host_cases()[-3:]
    for i, (name, roles, pcm) in enumerate(cases):
        C, R = ((C1, 3496), (C6, 1), (1, 1 << 20), (1 << 28, 70000))[i % 4]
        lim = L.Limiter(roles, C, R)
        want = lim.push(pcm)
        paths = [tmp_path / ("%s%d.bin" % (k, i)) for k in ("pcm", "out", "state")]
        for p, data in zip(paths, (pcm.astype("<i2").tobytes(), want.astype("<i2").tobytes(), lim.record().tobytes())):
            p.write_bytes(data)
        args = [exe, str(pcm.shape[1]), "".join(str(min(v, 9)) for v in roles), str(C), str(R)] + [str(p) for p in paths]
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stdout, r.stderr)
        f = r.stdout.split()
        rd = lim.read()
        assert f[0] == "result" and [int(v) for v in f[1:]] == [rd["samples"], rd["reduced"], rd["max_detect"], rd["min_gain_q24"], rd["flags"], 0], name
        # one wrong byte in the expected output is seen
        bad = bytearray(want.astype("<i2").tobytes())
        bad[-1] ^= 1
        paths[1].write_bytes(bytes(bad))
        assert subprocess.run(args, capture_output=True, text=True).returncode == 3, name
    # a file that is not whole frames is refused by the program, not read past
    short = tmp_path / "short.bin"
    short.write_bytes(bytes(3072 * 2 - 2))
    assert subprocess.run([exe, "2", "11", str(C1), "3496", str(short), str(short), str(paths[2])], capture_output=True, text=True).returncode == 2
