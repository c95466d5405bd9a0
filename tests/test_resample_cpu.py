"""CPU: the sample-rate converter's rule (tests/resample_model.py) - its tables' sums, bounds and frequency response, its error on
tones, the elastic buffer's counts, its independence of how a stream is cut into calls - and the engine's host side: the ratio,
the table (ac3mi_resample_tables), the plan (ac3mi_resample_plan) and the host converter (ac3mi_resample_host), which runs the
rule code the kernel runs, against the model byte for byte.  No GPU."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import _harness as H
from tests import resample_model as R

NB = R.STATE_DTYPE.itemsize
TRIPLES = {(44100, 48000): (160, 147, 64), (48000, 44100): (147, 160, 72), (32000, 48000): (3, 2, 64), (48000, 32000): (2, 3, 96),
           (32000, 44100): (441, 320, 64), (44100, 32000): (320, 441, 96)}
CRCS = {(44100, 48000): 0xb5545625, (48000, 44100): 0x40df8493, (32000, 48000): 0x134bb591, (48000, 32000): 0xcf55327c,
        (32000, 44100): 0x49e60bb6, (44100, 32000): 0x18e3680a}
# one-frame calls: (out_frames of the first 14 calls, pending behind some of them)
SEQUENCES = {(44100, 48000): ([1] * 11 + [2, 1, 1], {0: 136, 1: 272, 10: 1495, 11: 95}),
             (48000, 44100): ([0] + [1] * 11 + [0, 1], {0: 1412, 1: 1287}),
             (32000, 48000): ([1, 2] * 7, {0: 768, 1: 0}),
             (48000, 32000): ([0, 1, 1] * 4 + [0, 1], {0: 1024, 1: 512, 2: 0})}
PERIODS = {(44100, 48000): (147, 160), (48000, 44100): (160, 147), (32000, 48000): (2, 3), (48000, 32000): (3, 2), (32000, 44100): (320, 441),
           (44100, 32000): (441, 320)}


def _host(pair, pcm, cuts=None):
    """ac3mi_resample_host over pcm [n][C] in calls of `cuts` frames, each with its planned out_frames -> (out, the state's bytes)"""
    pkg = H.pkg()
    f, state, outs = 0, None, []
    n_in = f_out = 0
    for n in cuts or (pcm.shape[0] // 1536,):
        of, _ = pkg.resample_plan(*pair, n_in, f_out, n)
        out, state, status = pkg.resample_host(pair, pcm[1536 * f:1536 * (f + n)], of, state)
        assert status == 0
        outs.append(out)
        f += n
        n_in += 1536 * n
        f_out += of
    assert 1536 * f == pcm.shape[0]
    return np.concatenate(outs), state


def test_structs_and_exports():
    pkg = H.pkg()
    assert ctypes.sizeof(pkg.capi.ResampleDescC) == 12
    assert pkg.resample_state_bytes() == NB and NB % 8 == 0
    lib = pkg.load_library()
    for name in ("ac3mi_resample_ratio", "ac3mi_resample_tables", "ac3mi_resample_state_bytes", "ac3mi_resample_plan", "ac3mi_resample_batch",
                 "ac3mi_resample_host"):
        assert hasattr(lib, name) and name in pkg.declared_symbols()
    # the batched call refuses a null context before anything else (no GPU needed to say so)
    d = pkg.ResampleDesc(44100, 48000, 2)
    assert lib.ac3mi_resample_batch(None, ctypes.byref(d), None, 0, 1, None, 0, None, None) == -1
    assert set(TRIPLES) == set(R.PAIRS)
    for pair, want in TRIPLES.items():
        assert pkg.resample_ratio(*pair) == want == R.ratio(*pair), pair
    for a, b in ((48000, 48000), (44100, 44100), (24000, 48000), (48000, 24000), (0, 48000), (48000, 0), (22050, 44100)):
        assert lib.ac3mi_resample_ratio(a, b, None, None, None) == -1, (a, b)
    with open(os.path.join(H.ROOT, "include", "ac3mi.h")) as f:
        text = f.read()
    assert "#define AC3MI_RESAMPLE_FRAMES 1" in text and "#define AC3MI_RESAMPLE_STATE 2" in text


@pytest.mark.parametrize("pair", R.PAIRS)
def test_tables(pair):
    """the engine's table is the model's, coefficient for coefficient; every phase sums to 2^23; the split's ranges and the two
    absolute-sum bounds that keep the kernel's sums inside an int32; the CRC-32 the rule's author computed"""
    pkg = H.pkg()
    L, M, T = R.ratio(*pair)
    C = pkg.resample_tables(*pair)
    assert C.shape == (L, T) and C.dtype == np.int32
    assert np.array_equal(C, R.table(*pair))
    assert np.all(C.astype(np.int64).sum(axis=1) == 1 << 23)
    hi, lo = R.split(C.astype(np.int64))
    assert np.array_equal(512 * hi + lo, C)
    assert -3528 <= hi.min() and hi.max() <= 16384 and -256 <= lo.min() and lo.max() <= 255
    ah, al = int(np.abs(hi).sum(axis=1).max()), int(np.abs(lo).sum(axis=1).max())
    assert ah <= 45658 and al <= 14220, (ah, al)
    assert ah * 32768 < 1 << 31 and al * 32768 < 1 << 31        # |A| <= 1.50e9, |B| <= 4.7e8
    assert zlib.crc32(C.astype("<i4").tobytes()) == CRCS[pair]
    assert pkg.load_library().ac3mi_resample_tables(pair[0], pair[1], None) == -1


@pytest.mark.parametrize("pair", R.PAIRS)
def test_frequency_response_of_the_integer_table(pair):
    """the prototype - the engine's phases interleaved - over a 2^20-point FFT: flat within 0.001 dB up to 0.907 of the lower
    Nyquist frequency, at most -90 dB from 1.093 of it on"""
    L, M, T = R.ratio(*pair)
    C = H.pkg().resample_tables(*pair)
    h = C.T.reshape(-1).astype(np.float64)                     # tap k of phase p lies at time k + p / L
    N = 1 << 20
    mag = np.abs(np.fft.rfft(h, N)) / (L * 2.0 ** 23)
    f = np.arange(len(mag)) / N * L * pair[0]
    nyq = min(pair) / 2
    ripple = float(np.abs(20 * np.log10(mag[f <= 0.907 * nyq])).max())
    stop = float(20 * np.log10(mag[f >= 1.093 * nyq].max()))
    print("%d -> %d: pass-band ripple %.5f dB, stop band %.2f dB" % (pair + (ripple, stop)))
    assert ripple <= 0.001 and stop <= -90.0


@pytest.mark.parametrize("pair", R.PAIRS)
def test_tones(pair):
    """a full-scale sine at 997 Hz and at 0.4 of the lower rate, four frames, through the host converter: against the analytic
    sine at time m M / L - T / 2, behind the rise, the error is at most 0.6 LSB rms and 2 LSB (0.29 rms is the rounding alone)"""
    L, M, T = R.ratio(*pair)
    n = 4 * 1536
    for freq in (997.0, 0.4 * min(pair)):
        x = np.round(32767 * np.sin(2 * np.pi * freq * np.arange(n) / pair[0])).astype(np.int16)[:, None]
        y, state = _host(pair, x)
        rec = np.frombuffer(state, R.STATE_DTYPE)[0]
        left = R.out_count(*pair, n) - len(y)
        y = np.concatenate([y[:, 0], rec["pend"][:left]]).astype(np.float64)
        assert len(y) == R.out_count(*pair, n)
        m = np.arange(len(y))
        e = (y - 32767 * np.sin(2 * np.pi * freq * (m * M / L - T / 2) / pair[0]))[-(-T * L // M):]
        rms, peak = float(np.sqrt(np.mean(e * e))), float(np.abs(e).max())
        print("%d -> %d, %.0f Hz: rms %.3f LSB, peak %.3f LSB" % (pair + (freq, rms, peak)))
        assert rms <= 0.6 and peak <= 2.0


def test_counts_and_plan():
    pkg = H.pkg()
    for pair in R.PAIRS:
        n_in = f_out = 0
        seq = []
        for call in range(14):
            got = pkg.resample_plan(*pair, n_in, f_out, 1)
            assert got == R.plan(*pair, n_in, f_out, 1), (pair, call)
            seq.append(got)
            n_in += 1536
            f_out += got[0]
        if pair in SEQUENCES:
            frames, pending = SEQUENCES[pair]
            assert [s[0] for s in seq] == frames, pair
            for call, left in pending.items():
                assert seq[call][1] == left, (pair, call)
        fin, fout = PERIODS[pair]
        assert pkg.resample_plan(*pair, 0, 0, fin) == (fout, 0) == R.plan(*pair, 0, 0, fin), pair
        for k in range(1, min(fin, 50)):
            assert R.plan(*pair, 0, 0, k)[1] != 0, (pair, k)            # ... and no shorter period
    assert pkg.resample_plan(44100, 48000, 0, 0, 147) == (160, 0)
    lib = pkg.load_library()
    of, left = ctypes.c_int(), ctypes.c_int()
    for args in ((48000, 48000, 0, 0, 1), (44100, 48000, 0, 0, 0), (44100, 48000, 0, 0, -1), (44100, 48000, 0, 5, 1), (44100, 48000, 1 << 60, 0, 1),
                 (44100, 48000, 1536, 0, 1)):                        # 1536 in and nothing taken: 1672 pending is no state of a valid call
        assert lib.ac3mi_resample_plan(*args, ctypes.byref(of), ctypes.byref(left)) == -1, args


def test_cuts():
    """24 frames as one call, as one-frame calls and in uneven cuts, each with its planned out_frames: the same output and the
    same final state bytes, in the model's state form and in the host converter"""
    cuts = (1, 5, 2, 7, 1, 1, 4, 3)
    assert sum(cuts) == 24
    for pair, ch in (((44100, 48000), 2), ((48000, 32000), 1), ((32000, 44100), 3)):
        pcm = R.contents(pair[0], 24, ch, seed=7)[2][1]
        whole = R.Converter(*pair, ch)
        want = whole.push(pcm)
        record = whole.record().tobytes()
        for c in ((1,) * 24, cuts):
            conv = R.Converter(*pair, ch)
            at, parts = 0, []
            for n in c:
                parts.append(conv.push(pcm[1536 * at:1536 * (at + n)]))
                at += n
            assert np.concatenate(parts).tobytes() == want.tobytes() and conv.record().tobytes() == record, (pair, c)
        for c in (None, (1,) * 24, cuts):
            got, state = _host(pair, pcm, c)
            assert got.tobytes() == want.tobytes() and state == record, (pair, c)
        # the state form = the rule over the whole signal
        m1 = R.out_count(*pair, 24 * 1536)
        direct = R.convert(pcm, *pair, m0=0, m1=m1).astype(np.int16)
        rec = whole.record()
        assert direct[:len(want)].tobytes() == want.tobytes() and np.array_equal(rec["pend"][:(m1 - len(want)) * ch], direct[len(want):].reshape(-1))
        assert not rec["pend"][(m1 - len(want)) * ch:].any() and np.array_equal(rec["hist"][:ch], pcm[-R.HIST:].T) and not rec["hist"][ch:].any()


@pytest.mark.parametrize("pair", R.PAIRS)
def test_host_twin_equals_the_model(pair):
    """ac3mi_resample_host = the model, output and state byte for byte, on the named contents, channels 1..6"""
    clamped = set()
    for ch in range(1, 7):
        for name, pcm in R.contents(pair[0], 3, ch, seed=ch):
            conv = R.Converter(*pair, ch)
            want = conv.push(pcm)
            for cuts in (None, (1, 2)):
                got, state = _host(pair, pcm, cuts)
                assert got.tobytes() == want.tobytes(), (name, ch, cuts)
                assert state == conv.record().tobytes(), (name, ch, cuts)
            if name == "silence":
                assert not want.any()
            if name == "full-scale random":
                clamped |= {int(want.min()), int(want.max())}
    assert clamped == {-32768, 32767}


def test_refusals():
    pkg = H.pkg()
    lib = pkg.load_library()
    up, down = (44100, 48000), (48000, 44100)
    pcm = R.contents(44100, 2, 2, seed=3)[2][1]
    out, state, status = pkg.resample_host(up, pcm[:1536], 1)
    assert status == 0
    # a wrong out_frames: status 1, the state byte for byte, zeros
    for of in (0, 2, 3):
        got, st, status = pkg.resample_host(up, pcm[1536:], of, state)
        assert status == R.STATUS_FRAMES and st == state and not got.any() and got.shape == (1536 * of, 2), of
    got, st, status = pkg.resample_host(up, pcm[:1536], 0)              # ... and on a new stream
    assert status == R.STATUS_FRAMES and st == bytes(NB)
    # another pair, another channel count: status 2
    got, st, status = pkg.resample_host(down, pcm[:1536], 1, state)
    assert status == R.STATUS_STATE and st == state and not got.any()
    got, st, status = pkg.resample_host(up, np.zeros((1536, 3), np.int16), 1, state)
    assert status == R.STATUS_STATE and st == state and not got.any()
    got, st, status = pkg.resample_host(up, pcm[1536:], 1, state)      # the untouched state goes on
    conv = R.Converter(*up, 2)
    assert status == 0 and np.concatenate([out, got]).tobytes() == conv.push(pcm, 2).tobytes() and st == conv.record().tobytes()
    # argument errors: state, output and status untouched
    buf = ctypes.create_string_buffer(b"\xa5" * NB, NB)
    x = np.zeros((2 * 1536, 6), np.int16)
    o = np.full((2 * 1536, 6), 0x5a5a, np.int16)
    status = ctypes.c_uint32(77)
    ok = dict(rates=up, ch=6, desc=True, p=x.ctypes.data, fin=2, o=o.ctypes.data, fout=2, st=buf, status=True)
    for kw in (dict(rates=(24000, 48000)), dict(rates=(48000, 12000)), dict(rates=(48000, 48000)), dict(rates=(0, 0)), dict(ch=0), dict(ch=7),
               dict(desc=False), dict(p=None), dict(o=None), dict(p=x.ctypes.data + 1), dict(o=o.ctypes.data + 1), dict(fin=0), dict(fin=-2),
               dict(fout=-1), dict(st=None), dict(status=False), dict(p=o.ctypes.data), dict(p=o.ctypes.data + 768 * 12, fin=1),
               dict(p=o.ctypes.data - 3072 * 6 + 2, fin=1)):
        a = dict(ok, **kw)
        d = pkg.ResampleDesc(a["rates"][0], a["rates"][1], a["ch"])
        assert lib.ac3mi_resample_host(ctypes.byref(d) if a["desc"] else None, a["p"], a["fin"], a["o"], a["fout"], a["st"],
                                       ctypes.byref(status) if a["status"] else None) == -1, kw
    assert buf.raw == b"\xa5" * NB and np.all(o == 0x5a5a) and status.value == 77
    # no output frames: h_out may be NULL
    d = pkg.ResampleDesc(48000, 44100, 6)
    new = ctypes.create_string_buffer(NB)
    assert lib.ac3mi_resample_host(ctypes.byref(d), x.ctypes.data, 1, None, 0, new, ctypes.byref(status)) == 0 and status.value == 0
    assert np.frombuffer(new.raw, R.STATE_DTYPE)[0]["samples_in"] == 1536


def test_host_twin_under_the_sanitisers(tmp_path):
    """tests/resample_c/resample_main.c with a host-only translation of csrc/resample.hip (resample_rule.h's table builder, plan
    and converter), both built with -fsanitize=address,undefined and run on the CPU as a program of its own: the model's
    outputs and states, in two calls and in one, a refused call, and not a word from either sanitiser"""
    exe = H.build_sanitised([os.path.join(H.ROOT, "tests", "resample_c", "resample_main.c"), os.path.join(H.CSRC, "resample.hip")], str(tmp_path / "resample_main"), includes=[os.path.join(H.ROOT, "include")])
    for i, pair in enumerate(R.PAIRS):
        ch = (6, 2, 1, 3, 5, 4)[i]
        frames = (3, 2, 1, 3, 2, 1)[i]
        name, pcm = R.contents(pair[0], frames, ch, seed=40 + i)[(2, 3, 4, 1, 3, 2)[i]]
        conv = R.Converter(*pair, ch)
        want = conv.push(pcm)
        paths = [tmp_path / ("%s%d.bin" % (k, i)) for k in ("pcm", "out", "state")]
        for p, data in zip(paths, (pcm.astype("<i2").tobytes(), want.astype("<i2").tobytes(), conv.record().tobytes())):
            p.write_bytes(data)
        args = [exe, str(pair[0]), str(pair[1]), str(ch)] + [str(p) for p in paths]
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (pair, name, r.returncode, r.stdout, r.stderr)
        of, left = len(want) // 1536, len(conv.pend)
        assert r.stdout.split() == ["result", str(of), str(left), str(R.ratio(*pair)[0] << 23)], (pair, r.stdout)
        # one wrong byte in the expected state is seen
        bad = bytearray(conv.record().tobytes())
        bad[0] ^= 1
        paths[2].write_bytes(bytes(bad))
        assert subprocess.run(args, capture_output=True, text=True).returncode == 3, pair
    # a file that is not whole frames is refused by the program, not read past
    short = tmp_path / "short.bin"
    short.write_bytes(bytes(3072 * 2 - 2))
    assert subprocess.run([exe, "44100", "48000", "2", str(short), str(short), str(paths[2])], capture_output=True, text=True).returncode == 2
