"""CPU: the encoder oracle (oracle/ac3enc_oracle.c) against the reference's OWN encoder, byte for byte.

tests/golden/ac3enc_ref.npz (+ .json) holds what the unmodified src/ac3enc/ac3enc.cpp, compiled behind
oracle/ref_ac3enc_glue.cpp, wrote for deterministic H.gen_pcm inputs (generator: tests/golden/make_golden.py
--only ac3enc_ref): frames and every stage array for a small matrix, one SHA-256 per frame for a wide one, the
tables AC3_encode_init fills, init's decision for every argument triple, and three re-initialisation sequences.
Every comparison is exact.  The fixture-based tests run everywhere; the live leg needs oracle/_ref/ac3enc_ref.so.

Two things the reference does that the fixture records as they are:

 * Its _ASSERT(n >= 0) in output_frame_end (ac3enc.cpp:1619: the frame is fuller than its size) does not hold on every
   frame whose search failed (:930-933: the allocation of the last attempt is written although it does not fit) and on
   a few stereo frames (five bits of rematrixing flags are written, one is counted, :889 / :1229-1243: the author's own
   note at :1609-1613).  767 of the 4479 recorded frames; no other assertion of the file trips on any frame.  The
   oracle must overflow on exactly these frames (test_reference_assertions, and frame by frame in the other tests).
 * AC3_encode_init does not clear last_samples (:55, :1673-1681): a second stream in the same instance starts with the
   first one's tail.  The oracle and the engine start clean - a deliberate deviation -
   and reproduce the reference's frames exactly once they are given that tail (test_reinit_*).
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _harness as H

FIX = np.load(os.path.join(H.GOLDEN, "ac3enc_ref.npz"))
with open(os.path.join(H.GOLDEN, "ac3enc_ref.json")) as _f:
    META = json.load(_f)
KINDS = META["kinds"]
OVERFLOW_LINE = "1619"          # _ASSERT(n >= 0) of output_frame_end


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def fixture_pcm(cfg, want_sha):
    """The input of a recorded stream.  A gen_pcm that no longer gives the recorded samples is reported as that."""
    pcm = H.gen_pcm(cfg["frames"], cfg["channels"], seed=cfg["seed"], kind=cfg["kind"])
    assert np.array_equal(sha(pcm), want_sha), "H.gen_pcm drifted: %r no longer gives the samples the fixture was recorded from" % (cfg,)
    return pcm


def wide_streams():
    """The streams of the wide matrix: (cfg dict, recorded pcm sha, first frame's row in wide_digest / wide_status)."""
    out, row = [], 0
    for c, s in zip(FIX["wide_cfg"], FIX["wide_pcm_sha"]):
        freq, bitrate, nch, cm, kind, seed, frames = (int(x) for x in c)
        out.append(({"freq": freq, "bitrate": bitrate, "channels": nch, "chmap": FIX["wide_chmaps"][cm][:nch].tolist(),
                     "kind": KINDS[kind], "seed": seed, "frames": frames}, s, row))
        row += frames
    assert row == len(FIX["wide_digest"]) == len(FIX["wide_status"])
    return out


def tail_of(pcm, cfg):
    """last_samples after a stream: the last 256 samples of every coded channel (ac3enc.cpp:1676-1681), [6][256]."""
    last = np.zeros((6, 256), np.int16)
    for ch in range(cfg["channels"]):
        last[ch] = pcm[-256:, cfg["chmap"][ch]]
    return last


def orc_stream(cfg, pcm, last=None, taps=False):
    """One stream through the oracle -> frames [F][bytes], status [F][returned size, search failed, overflowed], taps."""
    L = H.orc()
    nch, F = cfg["channels"], cfg["frames"]
    fb = H.ci()
    h = L.orc_ac3enc_init(cfg["freq"], cfg["bitrate"], nch, ctypes.byref(fb))
    assert h, "the oracle refuses %r" % (cfg,)
    if last is not None:
        L.orc_ac3enc_set_last(h, H.P(np.ascontiguousarray(last, np.int16), H.i16p))
    cm = (ctypes.c_uint8 * 8)(*(tuple(cfg["chmap"]) + (0,) * 8)[:8])
    frames = np.zeros((F, fb.value), np.uint8)
    status = np.zeros((F, 3), np.int32)
    t = {k: [] for k in ("mdct_coef", "exponent", "encoded_exp", "bap", "exp_strategy", "exp_samples", "snr")}
    pcm = np.ascontiguousarray(pcm)
    for f in range(F):
        r = L.orc_ac3enc_frame(h, H.P(frames[f], H.u8p), ctypes.cast(pcm.ctypes.data + f * 1536 * nch * 2, H.i16p), cm)
        failed, written = H.ci(), H.ci()
        L.orc_ac3enc_get_status(h, ctypes.byref(failed), ctypes.byref(written))
        status[f] = (r, failed.value, written.value > fb.value - 2)
        if taps:
            m = np.zeros((6, 6, 256), np.int32)
            e1, e2, b = (np.zeros((6, 6, 256), np.uint8) for _ in range(3))
            st, sh = np.zeros((6, 6), np.uint8), np.zeros((6, 6), np.int8)
            c, fs = H.ci(), H.ci()
            L.orc_ac3enc_get_mdct(h, H.P(m, H.i32p))
            L.orc_ac3enc_get_exp(h, H.P(e1, H.u8p), H.P(e2, H.u8p))
            L.orc_ac3enc_get_bap(h, H.P(b, H.u8p))
            L.orc_ac3enc_get_misc(h, H.P(st, H.u8p), H.P(sh, H.i8p), ctypes.byref(c), ctypes.byref(fs))
            for k, v in (("mdct_coef", m), ("exponent", e1), ("encoded_exp", e2), ("bap", b), ("exp_strategy", st), ("exp_samples", sh)):
                t[k].append(v[:, :nch].copy())
            t["snr"].append((c.value, fs.value))
    L.orc_ac3enc_free(h)
    return frames, status, ({k: np.array(v) for k, v in t.items()} if taps else None)


def check_full_record(name, cfg, frames, status, taps):
    """Frames, returned sizes, failed searches, overflows and every stage array of one stream against full record `name`."""
    nch = cfg["channels"]
    g = lambda k: FIX["full_%s_%s" % (name, k)]
    assert np.array_equal(status, g("status")), "returned size / search failed / overflowed: %r, the reference %r" % (status.tolist(), g("status").tolist())
    for k in ("mdct_coef", "exponent", "exp_samples", "exp_strategy"):
        assert np.array_equal(taps[k], g(k)), "%s differs in %d places" % (k, int((taps[k] != g(k)).sum()))
    for ch in range(nch):
        n = 7 if nch == 6 and ch == 5 else 223          # beyond the coded coefficients the reference holds nothing defined
        for k in ("encoded_exp", "bap"):
            assert np.array_equal(taps[k][:, :, ch, :n], g(k)[:, :, ch, :n]), "%s of channel %d" % (k, ch)
    snr = g("snr")                                       # [frames][csnroffst, fsnroffst x 6, fgaincod x 6]
    assert np.array_equal(np.array(taps["snr"])[:, 0], snr[:, 0]), "csnroffst"
    assert (snr[:, 1:1 + nch] == np.array(taps["snr"])[:, 1:2]).all(), "fsnroffst"
    assert (snr[:, 7:7 + nch] == 4).all(), "fgaincod"   # the one value the oracle writes for every channel (:868)
    assert np.array_equal(frames, g("frames")), "frames differ in %d bytes" % int((frames != g("frames")).sum())


@pytest.mark.parametrize("rec", META["full"], ids=[r["name"] for r in META["full"]])
def test_full_records(rec):
    """Frames and every stage array - mdct_coef, exponent, exp_strategy, encoded_exp, bap, exp_samples, the offsets the search
    settled on - of the streams recorded in full: 5.1 at 384 and 640 kbps, stereo, mono, 44.1 kHz, half and quarter rate,
    and two streams whose search fails (one frame by a hair; every frame by kilobytes)."""
    pcm = fixture_pcm(rec, FIX["full_%s_pcm_sha" % rec["name"]])
    frames, status, taps = orc_stream(rec, pcm, taps=True)
    check_full_record(rec["name"], rec, frames, status, taps)


def test_full_records_cover_what_they_must():
    by = {r["name"]: r for r in META["full"]}
    assert (by["51_384k"]["channels"], by["51_384k"]["bitrate"]) == (6, 384000) and (by["51_640k"]["channels"], by["51_640k"]["bitrate"]) == (6, 640000)
    assert (by["20_192k"]["channels"], by["20_192k"]["bitrate"]) == (2, 192000) and (by["10_64k"]["channels"], by["10_64k"]["bitrate"]) == (1, 64000)
    assert by["20_44k1"]["freq"] == 44100 and by["30_half"]["freq"] == 24000
    assert FIX["full_30_yack_status"][:, 1].sum() == 1 and FIX["full_51_starved_status"][:, 1].all()
    assert (FIX["full_30_yack_status"][:, 0] == 384).all()      # the reference returns the frame size after a failed search too


@pytest.mark.parametrize("nch", [1, 2, 3, 4, 5, 6])
def test_wide_matrix_digests(nch):
    """Every stream of the wide matrix with this channel count: SHA-256 and returned size of every frame, which searches
    failed, which frames overflowed."""
    bad, n = [], 0
    for cfg, pcm_sha, row in wide_streams():
        if cfg["channels"] != nch:
            continue
        frames, status, _ = orc_stream(cfg, fixture_pcm(cfg, pcm_sha))
        n += 1
        for f in range(cfg["frames"]):
            if not (np.array_equal(sha(frames[f]), FIX["wide_digest"][row + f]) and np.array_equal(status[f], FIX["wide_status"][row + f])):
                bad.append((cfg, f, status[f].tolist(), FIX["wide_status"][row + f].tolist()))
    assert n >= 19 * 9 * 2
    assert not bad, "%d frames differ from the reference's, the first: %r" % (len(bad), bad[:3])


def test_wide_matrix_covers_what_it_must():
    cfg = FIX["wide_cfg"]
    accepted = {tuple(int(x) for x in a) for a, r in zip(FIX["init_args"], FIX["init_ret"]) if r > 0 and a[1] % 1000 == 0}
    assert {(int(c[0]), int(c[1]), int(c[2])) for c in cfg} == accepted, "every triple init accepts is encoded, for every channel count"
    assert len({(int(c[0]), int(c[1])) for c in cfg}) == 9 * 19 and {int(c[2]) for c in cfg} == {1, 2, 3, 4, 5, 6}
    assert {KINDS[int(c[4])] for c in cfg} >= {"tones", "noise", "quiet", "music", "bursts", "strobe"}
    identity, driver = [0, 1, 2, 3, 4, 5], list(H.CHMAP6[:6])
    assert sum(1 for m in FIX["wide_chmaps"].tolist() if m not in (identity, driver)) >= 2
    assert cfg[:, 6].max() >= 40
    assert META["counts"]["wide_frames"] == len(FIX["wide_digest"]) == int(cfg[:, 6].sum())


def test_init_decisions():
    """orc_ac3enc_init accepts exactly the argument triples AC3_encode_init accepts and returns the same frame size."""
    L = H.orc()
    assert (FIX["init_ret"] == 0).sum() > 1000 and (FIX["init_ret"] > 0).sum() >= 6 * 9 * 19
    bad = []
    for (freq, bitrate, nch), want in zip(FIX["init_args"].tolist(), FIX["init_ret"].tolist()):
        fb = H.ci(-1)
        h = L.orc_ac3enc_init(freq, bitrate, nch, ctypes.byref(fb))
        if bool(h) != (want > 0) or fb.value != want:
            bad.append((freq, bitrate, nch, want, fb.value))
        if h:
            L.orc_ac3enc_free(h)
    assert not bad, bad[:10]


def test_runtime_tables():
    """The tables AC3_encode_init fills at run time: costab, sintab, xcos1, xsin1, crc_table (orc_ac3enc_tables) and
    fft_rev, bndtab, masktab (orc_ac3enc_index_tables)."""
    L = H.orc()
    cos, sin, xc, xs = (np.zeros(n, np.int16) for n in (64, 64, 128, 128))
    crc = np.zeros(256, np.uint16)
    L.orc_ac3enc_tables(H.P(cos, H.i16p), H.P(sin, H.i16p), H.P(xc, H.i16p), H.P(xs, H.i16p), H.P(crc, H.u16p))
    rev, bnd, msk = np.zeros(128, np.uint8), np.zeros(51, np.uint8), np.zeros(253, np.uint8)
    L.orc_ac3enc_index_tables(H.P(rev, H.u8p), H.P(bnd, H.u8p), H.P(msk, H.u8p))
    for name, got in (("costab", cos), ("sintab", sin), ("xcos1", xc), ("xsin1", xs), ("crc_table", crc), ("bndtab", bnd), ("masktab", msk)):
        assert FIX["tab_" + name].dtype == got.dtype and np.array_equal(FIX["tab_" + name], got), name
    assert np.array_equal(FIX["tab_fft_rev"][:128], rev) and not FIX["tab_fft_rev"][128:].any()      # fft_init(7) fills 128 of the 512


def reinit_case(ent):
    a, b = ent["a"], ent["b"]
    pa = fixture_pcm(a, FIX["reinit_%s_a_pcm_sha" % ent["name"]])
    pb = fixture_pcm(b, FIX["reinit_%s_b_pcm_sha" % ent["name"]])
    return a, b, pa, pb, (lambda k: FIX["reinit_%s_%s" % (ent["name"], k)])


@pytest.mark.parametrize("ent", META["reinit"], ids=[e["name"] for e in META["reinit"]])
def test_reinit_overlap_state_alone_explains_the_reference(ent):
    """Stream A, AC3_encode_init again, stream B in one instance of the reference: B's first block overlaps with A's tail.
    The oracle gives the reference's frames of B exactly when its overlap state starts from that tail - and only then;
    from its own clean start it gives the frames of a reference instance that has coded nothing before."""
    a, b, pa, pb, g = reinit_case(ent)
    assert np.array_equal(orc_stream(a, pa)[0], g("a_frames"))
    assert np.array_equal(orc_stream(b, pb, last=tail_of(pa, a))[0], g("b_frames"))
    assert np.array_equal(orc_stream(b, pb)[0], g("b_fresh_frames"))
    assert not np.array_equal(g("b_frames")[0], g("b_fresh_frames")[0]), "the recorded sequence does not show the stale overlap"


def test_reinit_cases_cover_what_they_must():
    pairs = [(e["a"]["channels"], e["b"]["channels"]) for e in META["reinit"]]
    assert any(x == y for x, y in pairs) and any(x > y for x, y in pairs)


def test_reference_assertions():
    """The reference's own _ASSERTs over all 4479 recorded frames.  The issue of record: they should all hold.  They do,
    except `n >= 0` in output_frame_end (a frame fuller than its size), which trips once on each of the 760 frames whose
    search failed and on 7 stereo frames (the rematrixing flags the bit count leaves out); see the module docstring.  The
    tests above check frame by frame that the oracle overflows exactly where the reference's assertion tripped; here: no
    other assertion ever tripped, never more than one per frame, and never on a frame that is neither."""
    assert set(META["assert_sites"]) <= {OVERFLOW_LINE}
    tripped = 0
    for st, nch in [(FIX["wide_status"], np.repeat(FIX["wide_cfg"][:, 2], FIX["wide_cfg"][:, 6]))] + \
                   [(FIX["full_%s_status" % r["name"]], np.full(r["frames"], r["channels"])) for r in META["full"]]:
        trips, failed = st[:, 2], st[:, 1] != 0
        assert trips.max() <= 1
        assert (trips[failed] == 1).all(), "a failed search always overflows"
        assert (nch[(trips > 0) & ~failed] == 2).all(), "an overflow without a failed search is the stereo undercount"
        assert trips[~failed & (nch != 2)].sum() == 0
        tripped += int(trips.sum())
    assert tripped == META["assert_sites"].get(OVERFLOW_LINE, 0)


# ---- live: the oracle against the reference encoder itself, on streams outside the fixture -----------------------------

needs_refenc = pytest.mark.skipif(not H.have_refenc(), reason="oracle/_ref/ac3enc_ref.so not built")


def ref_stream(cfg, pcm, R=None):
    R = R or H.RefEncoder()
    assert R.init(cfg["freq"], cfg["bitrate"], cfg["channels"]) > 0
    frames, status, taps = [], [], {k: [] for k in ("mdct_coef", "exponent", "encoded_exp", "bap", "exp_strategy", "exp_samples", "snr")}
    before = R.assert_trips()[0]
    for f in range(cfg["frames"]):
        r, fr = R.frame(pcm[f * 1536:(f + 1) * 1536], cfg["chmap"])
        now = R.assert_trips()[0]
        frames.append(fr)
        status.append((r, int(R.yack), now - before))
        before = now
        for k in ("mdct_coef", "exponent", "encoded_exp", "bap", "exp_strategy", "exp_samples"):
            taps[k].append(R.array(k)[:, :cfg["channels"]])
        taps["snr"].append(R.snr())
    return np.stack(frames), np.array(status, np.int32), taps, R


@needs_refenc
def test_live_random_streams():
    """60 streams drawn from a seed of their own - channel count, sample rate, bit-rate code, kind, channel map, 1 to 6
    frames - through a fresh instance of the reference and through the oracle: frames, status and stage arrays."""
    rng = np.random.default_rng(20240917)
    rates = (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 448, 512, 576, 640)
    freqs = (48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000)
    for i in range(60):
        nch, fi = int(rng.integers(1, 7)), int(rng.integers(0, 9))
        code = int(rng.integers(max(0, 2 * nch - 2), 19))       # mostly rates that can hold the channels: the fixture has the starved ones
        cfg = {"freq": freqs[fi], "bitrate": (rates[code] >> (fi // 3)) * 1000, "channels": nch,
               "chmap": [int(x) for x in (rng.permutation(nch) if i % 3 else rng.integers(0, nch, nch))],
               "kind": KINDS[int(rng.integers(0, len(KINDS)))], "seed": 900000 + i, "frames": int(rng.integers(1, 7))}
        pcm = H.gen_pcm(cfg["frames"], nch, seed=cfg["seed"], kind=cfg["kind"])
        want, wstat, wt, R = ref_stream(cfg, pcm)
        got, gstat, gt = orc_stream(cfg, pcm, taps=True)
        assert set(R.assert_trips()[1]) <= {int(OVERFLOW_LINE)}, cfg
        assert np.array_equal(gstat, wstat), (cfg, gstat.tolist(), wstat.tolist())
        for k in ("mdct_coef", "exponent", "exp_samples", "exp_strategy"):
            assert np.array_equal(gt[k], np.array(wt[k])), (cfg, k)
        for ch in range(nch):
            n = 7 if nch == 6 and ch == 5 else 223
            for k in ("encoded_exp", "bap"):
                assert np.array_equal(gt[k][:, :, ch, :n], np.array(wt[k])[:, :, ch, :n]), (cfg, k, ch)
        assert [s[0] for s in wt["snr"]] == [s[0] for s in gt["snr"]], cfg
        assert all((s[1][:nch] == g[1]).all() for s, g in zip(wt["snr"], gt["snr"])), cfg
        assert np.array_equal(got, want), (cfg, int((got != want).sum()))


@needs_refenc
def test_live_reinit_random():
    """Re-initialisation outside the fixture: ten A/B pairs in one reference instance each; the oracle with A's tail."""
    rng = np.random.default_rng(77001)
    for i in range(10):
        cfgs = []
        for j in range(2):
            nch = int(rng.integers(1, 7))
            cfgs.append({"freq": (48000, 44100, 32000)[int(rng.integers(0, 3))], "bitrate": 64000 * nch, "channels": nch,
                         "chmap": [int(x) for x in rng.permutation(nch)], "kind": KINDS[int(rng.integers(0, 6))],
                         "seed": 910000 + 2 * i + j, "frames": 2})
        pa, pb = (H.gen_pcm(2, c["channels"], seed=c["seed"], kind=c["kind"]) for c in cfgs)
        _, _, _, R = ref_stream(cfgs[0], pa)
        want, _, _, _ = ref_stream(cfgs[1], pb, R)
        assert np.array_equal(orc_stream(cfgs[1], pb, last=tail_of(pa, cfgs[0]))[0], want), cfgs


@needs_refenc
def test_live_fixture_is_what_the_reference_gives_now():
    """The full records and the run-time tables, taken again from the reference as built here, equal the stored ones."""
    for rec in META["full"]:
        pcm = fixture_pcm(rec, FIX["full_%s_pcm_sha" % rec["name"]])
        frames, status, taps, R = ref_stream(rec, pcm)
        assert np.array_equal(frames, FIX["full_%s_frames" % rec["name"]]) and np.array_equal(status, FIX["full_%s_status" % rec["name"]])
        assert np.array_equal(np.array(taps["mdct_coef"]), FIX["full_%s_mdct_coef" % rec["name"]])
    for name in H.REFENC_TABLES:
        assert np.array_equal(R.array(name), FIX["tab_" + name]), name
