#!/usr/bin/env python3
"""Generates tests/golden/*.npz.  Runs ONLY in the build container, where oracle/_ref/liba52_ref.so
(the real liba52, compiled from /root/reference by oracle/Makefile) exists.

What is pinned and by what:
  decode_*.npz   bitstreams (made by our encoder oracle, whose frames are ac3enc's: ac3enc_ref.npz) and what
                 the REAL liba52 decodes from them: float PCM for several output modes, exponents, bap
  imdct.npz      random coefficient planes + delay -> REAL a52_imdct_512 / a52_imdct_256 output
  downmix.npz    REAL a52_downmix_init / a52_downmix_coeff / a52_downmix / a52_upmix results
  encoder.npz    our encoder oracle's own output and stage dumps for one 5.1 stream; tests/test_oracle_golden.py holds
                 it against the same stream as recorded from ac3enc itself in ac3enc_ref.npz
  ac3enc_ref.npz, ac3enc_ref.json   the REAL encoder (src/ac3enc/ac3enc.cpp compiled unmodified behind
                 oracle/ref_ac3enc_glue.cpp and the stand-in headers of oracle/winstub/, one fresh instance per stream):
                 frames and every stage array for a small matrix, SHA-256 and returned size per frame for a wide one,
                 the tables AC3_encode_init fills, its decision for every argument triple, re-initialisation sequences,
                 which searches failed, which of its assertions tripped   (`--only ac3enc_ref` regenerates just these,
                 bit for bit)
  a52dec_drivers.npz   tests/test_tools_gpu.py's streams through the reference's own liba52 + libao file drivers
                 (oracle/_ref/a52dec_ref): WAV and float output   (`--only a52dec_drivers` regenerates just this file)
  ac3tab.npz     the REAL encoder's constant tables (src/ac3enc/ac3tab.h:3-171 compiled unmodified behind
                 oracle/ref_ac3tab_glue.cpp): ac3_window, latab, hth, baptab, sdecaytab ... fgaintab, bndsz,
                 ac3_freqs, ac3_bitratetab   (`make_golden.py --only ac3tab` regenerates just this file)
  liba52_records.json   not written here: fingerprints of what the REAL liba52 gives on the seeded sweeps of
                 tests/test_oracle_vs_ref.py, test_oracle_encoder.py, test_mixlevel_switch.py, test_packer_streams.py
                 (tests/_harness.liba52_record); the tests write it themselves with oracle/_ref present:
                 AC3MI_RECORD_LIBA52=1 python -m pytest tests -m "not gpu"
Fixtures are data (inputs + expected outputs); no reference source text is stored.
"""
import ctypes
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _harness as H  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def ref_decode_with_taps(frames, flags, level, bias):
    L = H.ref()
    F, fb = frames.shape
    st = L.a52_init(0)
    buf = np.zeros(F * fb + 64, np.uint8)
    buf[:F * fb] = frames.reshape(-1)
    exps = np.zeros((F, 6, 6, 256), np.uint8)
    baps = np.zeros((F, 6, 6, 256), np.int8)
    pcm = None
    for f in range(F):
        fl, lv = H.ci(flags), H.cf(level)
        p = ctypes.cast(buf.ctypes.data + f * fb, H.u8p)
        assert L.a52_frame(st, p, ctypes.byref(fl), ctypes.byref(lv), bias) == 0
        nout = H.NFCHANS[fl.value & 15] + (1 if fl.value & 16 else 0)
        if pcm is None:
            pcm = np.zeros((F, 6, nout, 256), np.float32)
        for b in range(6):
            assert L.a52_block(st) == 0
            pcm[f, b] = np.ctypeslib.as_array(L.a52_samples(st), (1536,))[:nout * 256].reshape(nout, 256)
            for w in range(6):
                L.refglue_get_exp(st, w, H.P(exps[f, b, w], H.u8p))
                L.refglue_get_bap(st, w, H.P(baps[f, b, w], H.i8p))
    lfsr = L.refglue_get_lfsr(st)
    L.a52_free(st)
    return pcm, exps, baps, lfsr, fl.value


AC3TAB_NAMES = ("ac3_freqs", "ac3_bitratetab", "ac3_window", "latab", "hth", "baptab", "sdecaytab", "fdecaytab",
                "sgaintab", "dbkneetab", "floortab", "fgaintab", "bndsz")


def make_ac3tab():
    path = os.path.join(ROOT, "oracle", "_ref", "ac3tab_ref.so")
    assert os.path.exists(path), "oracle/_ref/ac3tab_ref.so missing: run `make -C oracle` in the build container"
    T = ctypes.CDLL(path)
    T.refglue_ac3tab.restype = ctypes.c_void_p
    T.refglue_ac3tab.argtypes = [ctypes.c_char_p, H.ip, H.ip]
    d = {}
    for name in AC3TAB_NAMES:
        n, eb = H.ci(), H.ci()
        ptr = T.refglue_ac3tab(name.encode(), ctypes.byref(n), ctypes.byref(eb))
        assert ptr and n.value > 0, name
        signed = name == "ac3_window"                       # the only signed table (short); the rest are unsigned
        dt = {1: np.uint8, 2: np.int16 if signed else np.uint16}[eb.value]
        d[name] = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), (n.value,)).copy()
    d["hth"] = d["hth"].reshape(50, 3)
    np.savez_compressed(os.path.join(OUT, "ac3tab.npz"), **d)
    print("ac3tab.npz", os.path.getsize(os.path.join(OUT, "ac3tab.npz")), {k: v.shape for k, v in d.items()})


def make_a52dec_drivers():
    from tests import test_tools_gpu as T
    assert os.path.exists(T.REF_TOOL), "oracle/_ref/a52dec_ref missing: run `make -C oracle` in the build container"
    d, paths = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for key, data in T.make_streams().items():
            d["stream_" + key] = np.frombuffer(data, np.uint8)
            paths[key] = os.path.join(tmp, key + ".ac3")
            with open(paths[key], "wb") as f:
                f.write(data)
        runs = [(mode, key, {}) for mode, key in T.WAV_CASES] + [("float", "51", opts) for _, opts in T.FLOAT_CASES]
        for mode, key, opts in runs:
            d[T.ref_driver_name(mode, key, **opts)] = np.frombuffer(T.run_ref_tool(mode, paths[key], **opts), np.uint8)
    np.savez_compressed(os.path.join(OUT, "a52dec_drivers.npz"), **d)
    print("a52dec_drivers.npz", os.path.getsize(os.path.join(OUT, "a52dec_drivers.npz")), sorted(d))


MIXFLIP = (("a7_st", 7, 2, (1, 1, 2, 2, 0, 0, 2, 1), 0.0), ("a7_mono", 7, 1, (0, 2, 2, 1, 2, 0), 0.0), ("a7_dolby", 7, 10, (3, 2, 0, 2, 2, 1), 0.0),
           ("a6_st", 6, 2, (1, 2, 2, 0, 2, 1), 0.0), ("a5_st", 5, 2, (0, 2, 1, 2, 2, 3), 0.0), ("a4_mono", 4, 1, (1, 2, 0, 2, 2, 1), 0.0),
           # at bias 384 (what the ACM driver decodes at): 2/x -> stereo and 3/x -> 3F lose the bias in blocks of mixed block sizes
           ("a6_st_b384", 6, 2, (1, 2, 2, 0, 2, 1), 384.0), ("a7_3f_b384", 7, 3, (2, 2, 1, 2, 2, 0), 384.0), ("a4_st_b384", 4, 2, (2, 2, 2, 3, 2, 2), 384.0))


def make_mixflip():
    """Streams whose surmixlev changes between frames (tests/packer.make_flip_stream), decoded by the real liba52."""
    from tests import packer
    assert H.have_ref()
    d = {}
    for tag, acmod, flags, levels, bias in MIXFLIP:
        fr = packer.make_flip_stream(2600 + acmod + flags, levels, acmod=acmod)
        pcm, errs, oflags = H.ref_decode(fr, flags, 1.0, bias)
        assert errs == 0
        d["frames_" + tag] = fr
        d["pcm_" + tag] = pcm
        d["args_" + tag] = np.array([flags, oflags], np.int32)
        d["levels_" + tag] = np.array(levels, np.int32)
        d["bias_" + tag] = np.array([bias], np.float32)
    np.savez_compressed(os.path.join(OUT, "mixflip.npz"), **d)
    print("mixflip.npz", os.path.getsize(os.path.join(OUT, "mixflip.npz")))


# ---- the reference's own encoder: tests/golden/ac3enc_ref.npz + ac3enc_ref.json -----------------------------------------
# Every stream is encoded by a fresh instance of the unmodified ac3enc (H.RefEncoder: a privately copied
# oracle/_ref/ac3enc_ref.so per stream); the re-initialisation cases alone run two streams through one instance.

ENC_KINDS = ("tones", "noise", "quiet", "music", "bursts", "strobe", "silence", "rails", "impulses", "dc")
ENC_RATES = (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 448, 512, 576, 640)
ENC_FREQS = (48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000)
IDMAP = (0, 1, 2, 3, 4, 5)
# name, freq, bitrate, channels, chmap, kind, seed, frames: recorded in full (frames + every stage array)
ENC_FULL = (("51_384k", 48000, 384000, 6, H.CHMAP6[:6], "tones", 7, 3),        # the streams of encoder.npz
            ("51_640k", 48000, 640000, 6, H.CHMAP6[:6], "music", 11, 2),
            ("20_192k", 48000, 192000, 2, IDMAP, "bursts", 12, 3),            # stereo: the rematrix-flag undercount (:892 / :1228-1236)
            ("10_64k", 48000, 64000, 1, IDMAP, "noise", 13, 3),
            ("20_44k1", 44100, 128000, 2, IDMAP, "strobe", 14, 3),
            ("30_half", 24000, 96000, 3, IDMAP, "tones", 15, 3),              # bsid 9
            ("40_quarter", 11025, 40000, 4, IDMAP, "music", 16, 2),           # bsid 10
            ("30_yack", 24000, 48000, 3, IDMAP, "music", 101000 + 25 * 7, 4), # frame 3: start value 3 does not fit, 3 - 4 < 0: search fails
            ("51_starved", 48000, 64000, 6, H.CHMAP6[:6], "noise", 880, 2))   # every frame fails and overflows by kilobytes
# name, (freq, bitrate, channels, chmap, kind, seed, frames) of stream A and of stream B, coded one after the other in ONE instance
ENC_REINIT = (("same_51", (48000, 384000, 6, H.CHMAP6[:6], "tones", 21, 2), (48000, 384000, 6, H.CHMAP6[:6], "music", 22, 2)),
              ("fewer_51_to_20", (48000, 448000, 6, H.CHMAP6[:6], "bursts", 23, 2), (44100, 192000, 2, IDMAP, "tones", 24, 2)),
              ("more_10_to_30", (32000, 96000, 1, IDMAP, "noise", 25, 2), (48000, 256000, 3, (2, 0, 1, 3, 4, 5), "strobe", 26, 2)))
ENC_STAGES = ("mdct_coef", "exponent", "exp_strategy", "encoded_exp", "bap", "exp_samples")


def enc_half(freq):
    return ENC_FREQS.index(freq) // 3


def enc_wide_matrix():
    """(freq, bitrate, channels, chmap, kind, seed, frames) of the streams recorded by digest."""
    out = []
    # every channel count x every sample rate x every bit-rate code init accepts, two kinds each (all ten kinds in turn)
    for nch in range(1, 7):
        for fi, freq in enumerate(ENC_FREQS):
            for code, kbps in enumerate(ENC_RATES):
                for k in range(2):
                    kind = ENC_KINDS[(2 * (nch + fi + code) + k) % len(ENC_KINDS)]
                    out.append((freq, (kbps >> enc_half(freq)) * 1000, nch, H.CHMAP6[:6] if nch == 6 else IDMAP, kind,
                                5000 + 1000 * nch + 100 * fi + 2 * code + k, 2))
    # the six programme kinds on every channel count at a rate that codes them well, longer
    for nch, kbps in ((1, 96), (2, 192), (3, 256), (4, 320), (5, 448), (6, 384)):
        for k, kind in enumerate(ENC_KINDS[:6]):
            out.append((48000, kbps * 1000, nch, H.CHMAP6[:6] if nch == 6 else IDMAP, kind, 7000 + 10 * nch + k, 5))
    # channel maps other than the driver's
    for k, (nch, kbps, chmap) in enumerate(((6, 384, IDMAP), (6, 384, (5, 4, 3, 2, 1, 0)), (6, 448, (3, 1, 4, 0, 5, 2)), (2, 192, (1, 0, 2, 3, 4, 5)),
                                            (3, 256, (2, 0, 1, 3, 4, 5)), (5, 448, (4, 3, 2, 1, 0, 5)), (2, 128, (0, 0, 2, 3, 4, 5)))):
        for j, kind in enumerate(("tones", "bursts")):
            out.append((48000, kbps * 1000, nch, chmap, kind, 7500 + 2 * k + j, 3))
    # long streams: the csnroffst carry-over (:921, :969) over 40 frames and more
    out.append((48000, 384000, 6, H.CHMAP6[:6], "bursts", 7600, 48))
    out.append((44100, 192000, 2, IDMAP, "tones", 7601, 40))
    out.append((24000, 48000, 3, IDMAP, "music", 7602, 40))            # starves now and then: failed searches inside a long stream
    return out


def enc_init_triples():
    """Argument triples of AC3_encode_init: every channel count 0..7, every accepted sample rate and some that are not,
    every accepted bit rate of every rate family and some that are not (among them rates that are no multiple of 1000)."""
    freqs = ENC_FREQS + (0, 4000, 6000, 47999, 48001, 64000, 88200, 96000)
    rates = sorted({(k >> h) * 1000 for k in ENC_RATES for h in range(3)} | {0, 1000, 7000, 31000, 383000, 384999, 385000, 641000, 768000, 1000000})
    return [(f, r, c) for c in range(0, 8) for f in freqs for r in rates]


def enc_sha(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def enc_ref_stream(R, cfg, full):
    """Runs one stream through instance R (initialised here).  -> dict of per-frame records."""
    freq, bitrate, nch, chmap, kind, seed, frames = cfg
    size = R.init(freq, bitrate, nch)
    assert size > 0, cfg
    pcm = H.gen_pcm(frames, nch, seed=seed, kind=kind)
    rec = {"pcm_sha": enc_sha(pcm), "frames": [], "ret": [], "yack": [], "trips": [], "snr": []}
    rec.update({k: [] for k in ENC_STAGES} if full else {})
    trips0 = R.assert_trips()[0]
    for f in range(frames):
        r, fr = R.frame(pcm[f * 1536:(f + 1) * 1536], chmap[:nch])
        t = R.assert_trips()[0]
        rec["frames"].append(fr)
        rec["ret"].append(r)
        rec["yack"].append(int(R.yack))
        rec["trips"].append(t - trips0)
        trips0 = t
        if full:
            c, fs, fg = R.snr()
            rec["snr"].append(np.concatenate([[c], fs, fg]))
            for k in ENC_STAGES:
                a = R.array(k)[:, :nch]                           # [6 blocks][channels]...: the channels beyond are not this stream's
                if k in ("bap", "encoded_exp"):                   # beyond the coded coefficients the reference never writes
                    for ch in range(nch):                         # encoded_exp and copies uninitialised stack into bap (:857, :940)
                        a[:, ch, 7 if nch == 6 and ch == 5 else 223:] = 0
                rec[k].append(a)
    return rec


def make_ac3enc_ref():
    import json
    assert H.have_refenc(), "oracle/_ref/ac3enc_ref.so missing: run `make -C oracle` in the build container"
    d, meta = {}, {"kinds": ENC_KINDS, "full": [], "reinit": [], "assert_sites": {}}
    sites = {}

    def note_sites(R):
        for line, n in R.assert_trips()[1].items():
            sites[line] = sites.get(line, 0) + n

    # ---- run-time tables (filled by AC3_encode_init) and init's decisions
    R = H.RefEncoder()
    triples = enc_init_triples()
    d["init_args"] = np.array(triples, np.int32)
    d["init_ret"] = np.array([R.init(*t) for t in triples], np.int32)
    R = H.RefEncoder()
    assert R.init(48000, 384000, 6) == 1536
    for name in H.REFENC_TABLES:
        d["tab_" + name] = R.array(name)
    # ---- full records
    for name, *cfg in ENC_FULL:
        R = H.RefEncoder()
        rec = enc_ref_stream(R, tuple(cfg), True)
        note_sites(R)
        freq, bitrate, nch, chmap, kind, seed, frames = cfg
        meta["full"].append({"name": name, "freq": freq, "bitrate": bitrate, "channels": nch, "chmap": list(chmap[:nch]), "kind": kind,
                             "seed": seed, "frames": frames})
        d["full_%s_pcm_sha" % name] = rec["pcm_sha"]
        d["full_%s_frames" % name] = np.stack(rec["frames"])
        d["full_%s_status" % name] = np.array([rec["ret"], rec["yack"], rec["trips"]], np.int32).T      # [frames][returned size, search failed, assertions tripped]
        d["full_%s_snr" % name] = np.stack(rec["snr"]).astype(np.int32)                               # [frames][csnroffst, fsnroffst x 6, fgaincod x 6]
        for k in ENC_STAGES:
            d["full_%s_%s" % (name, k)] = np.stack(rec[k])
    # ---- re-initialisation: A, AC3_encode_init again, B in one instance; and B in a fresh one
    for name, a, b in ENC_REINIT:
        R = H.RefEncoder()
        ra = enc_ref_stream(R, a, False)
        rb = enc_ref_stream(R, b, False)
        note_sites(R)
        R2 = H.RefEncoder()
        rc = enc_ref_stream(R2, b, False)
        assert not any(ra["yack"] + rb["yack"] + rc["yack"])
        ent = {"name": name}
        for tag, cfg in (("a", a), ("b", b)):
            freq, bitrate, nch, chmap, kind, seed, frames = cfg
            ent[tag] = {"freq": freq, "bitrate": bitrate, "channels": nch, "chmap": list(chmap[:nch]), "kind": kind, "seed": seed, "frames": frames}
        meta["reinit"].append(ent)
        d["reinit_%s_a_pcm_sha" % name], d["reinit_%s_b_pcm_sha" % name] = ra["pcm_sha"], rb["pcm_sha"]
        d["reinit_%s_a_frames" % name] = np.stack(ra["frames"])
        d["reinit_%s_b_frames" % name] = np.stack(rb["frames"])            # B after A in the same instance
        d["reinit_%s_b_fresh_frames" % name] = np.stack(rc["frames"])      # B in an instance of its own
    # ---- the wide matrix, by digest
    wide = enc_wide_matrix()
    chmaps = sorted({c[3] for c in wide})
    cfgs, shas, dig, status = [], [], [], []
    for cfg in wide:
        R = H.RefEncoder()
        rec = enc_ref_stream(R, cfg, False)
        note_sites(R)
        freq, bitrate, nch, chmap, kind, seed, frames = cfg
        cfgs.append([freq, bitrate, nch, chmaps.index(chmap), ENC_KINDS.index(kind), seed, frames])
        shas.append(rec["pcm_sha"])
        dig += [enc_sha(fr) for fr in rec["frames"]]
        status += list(zip(rec["ret"], rec["yack"], rec["trips"]))
    d["wide_cfg"] = np.array(cfgs, np.int32)              # [streams][freq, bitrate, channels, chmap index, kind index, seed, frames]
    d["wide_chmaps"] = np.array(chmaps, np.uint8)
    d["wide_pcm_sha"] = np.stack(shas)
    d["wide_digest"] = np.stack(dig)                      # [all frames, stream after stream][32]: SHA-256 of the frame's bytes
    d["wide_status"] = np.array(status, np.int32)         # [all frames][returned size, search failed, assertions tripped]
    meta["assert_sites"] = {str(k): v for k, v in sorted(sites.items())}
    meta["counts"] = {"full_frames": sum(e["frames"] for e in meta["full"]), "wide_streams": len(wide), "wide_frames": len(dig),
                      "wide_failed_searches": int(d["wide_status"][:, 1].sum()), "init_triples": len(triples),
                      "init_accepted": int((d["init_ret"] > 0).sum())}
    np.savez_compressed(os.path.join(OUT, "ac3enc_ref.npz"), **d)
    with open(os.path.join(OUT, "ac3enc_ref.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("ac3enc_ref.npz", os.path.getsize(os.path.join(OUT, "ac3enc_ref.npz")), meta["counts"], meta["assert_sites"])


def main():
    if "--only" in sys.argv and sys.argv[sys.argv.index("--only") + 1] == "mixflip":
        make_mixflip()
        return
    if "--only" in sys.argv and sys.argv[sys.argv.index("--only") + 1] == "ac3tab":
        make_ac3tab()
        return
    if "--only" in sys.argv and sys.argv[sys.argv.index("--only") + 1] == "a52dec_drivers":
        make_a52dec_drivers()
        return
    if "--only" in sys.argv and sys.argv[sys.argv.index("--only") + 1] == "ac3enc_ref":
        make_ac3enc_ref()
        return
    make_ac3tab()
    assert H.have_ref(), "oracle/_ref/liba52_ref.so missing: run `make -C oracle` in the build container"
    R = H.ref()
    # ---- decode fixtures -------------------------------------------------
    for kind, nfr in (("tones", 4), ("noise", 2), ("quiet", 2)):
        pcm_in = H.gen_pcm(nfr, 6, seed=2024, kind=kind)
        frames = H.orc_encode(pcm_in)
        d = {"pcm_in": pcm_in, "frames": frames}
        for tag, flags, level, bias in (("51", 7 | 16, 1.0, 0.0), ("stereo", 2, 1.0, 0.0),
                                         ("dolby_adj", 10 | 32, 1.0, 0.0), ("51_bias384", 7 | 16 | 32, 1.0, 384.0)):
            pcm, exps, baps, lfsr, oflags = ref_decode_with_taps(frames, flags, level, bias)
            d["pcm_" + tag] = pcm
            d["args_" + tag] = np.array([flags, level, bias, oflags, lfsr], np.float64)
            if tag == "51":
                d["exp"], d["bap"] = exps, baps
            if tag == "51_bias384":
                s16 = np.zeros((nfr, 6, 256, 6), np.int16)
                for f in range(nfr):
                    for b in range(6):
                        R.convert2s16_multi(H.P(np.ascontiguousarray(pcm[f, b]), H.fp), H.P(s16[f, b], H.i16p), oflags)
                d["s16_multi_" + tag] = s16      # libao channel order (convert2s16.c:113-181), in-range values
        np.savez_compressed(os.path.join(OUT, "decode_%s.npz" % kind), **d)

    # ---- transform-only fixtures ----------------------------------------
    rng = np.random.default_rng(99)
    x = (rng.standard_normal((8, 256)) * 0.1).astype(np.float32)
    dl = (rng.standard_normal((8, 256)) * 0.1).astype(np.float32)
    kinds = np.array([0, 0, 1, 1, 0, 1, 0, 1], np.uint8)        # 0: imdct_512, 1: imdct_256
    biases = np.array([0, 384, 0, 384, 0.5, 0, -1, 0], np.float32)
    y, dn = x.copy(), dl.copy()
    for i in range(8):
        (R.a52_imdct_256 if kinds[i] else R.a52_imdct_512)(H.P(y[i], H.fp), H.P(dn[i], H.fp), float(biases[i]))
    # a chained sequence long/short/long through one delay plane
    seq_x = (rng.standard_normal((6, 256)) * 0.1).astype(np.float32)
    seq_k = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    seq_d = np.zeros(256, np.float32)
    seq_y = seq_x.copy()
    for i in range(6):
        (R.a52_imdct_256 if seq_k[i] else R.a52_imdct_512)(H.P(seq_y[i], H.fp), H.P(seq_d, H.fp), 0.0)
    np.savez_compressed(os.path.join(OUT, "imdct.npz"), x=x, delay_in=dl, kind=kinds, bias=biases, y=y, delay_out=dn,
                        seq_x=seq_x, seq_kind=seq_k, seq_y=seq_y, seq_delay=seq_d)

    # ---- downmix fixtures ------------------------------------------------
    cases, res_init, res_coeff, res_mix, res_up = [], [], [], [], []
    planes0 = (rng.standard_normal((6, 256)) * 0.1).astype(np.float32)
    for acmod in range(8):
        for req in range(11):
            for adj in (0, 32):
                for clev, slev in ((0.7071067811865476, 0.7071067811865476), (0.5946035575013605, 0.5), (0.5, 0.0)):
                    lv = H.cf(1.0)
                    out = R.a52_downmix_init(acmod, req | adj, ctypes.byref(lv), np.float32(clev), np.float32(slev))
                    if out < 0:
                        continue
                    g = np.zeros(5, np.float32)
                    mask = R.a52_downmix_coeff(H.P(g, H.fp), acmod, out, lv.value, np.float32(clev), np.float32(slev))
                    p = planes0.copy()
                    R.a52_downmix(H.P(p, H.fp), acmod, out, 0.25, np.float32(clev), np.float32(slev))
                    u = planes0.copy()
                    R.a52_upmix(H.P(u, H.fp), acmod, out)
                    cases.append([acmod, req | adj, clev, slev])
                    res_init.append([out, lv.value])
                    n = H.NFCHANS[acmod]
                    gg = np.zeros(5, np.float32)
                    gg[:n] = g[:n]
                    if (acmod, out) == (1, 10):
                        gg[1:] = 0                      # only coeff[0] is defined for mono -> dolby
                    res_coeff.append(np.concatenate([gg, [mask]]))
                    res_mix.append(p)
                    res_up.append(u)
    np.savez_compressed(os.path.join(OUT, "downmix.npz"), planes=planes0, cases=np.array(cases, np.float64),
                        init=np.array(res_init, np.float64), coeff=np.array(res_coeff, np.float32),
                        mixed=np.array(res_mix, np.float32), upmixed=np.array(res_up, np.float32))

    # ---- encoder oracle stage dumps (the same stream from ac3enc itself: ENC_FULL "51_384k") --------
    L = H.orc()
    pcm_in = H.gen_pcm(3, 6, seed=7, kind="tones")
    fb = H.ci()
    h = L.orc_ac3enc_init(48000, 384000, 6, ctypes.byref(fb))
    cm = (ctypes.c_uint8 * 8)(*H.CHMAP6)
    frames = np.zeros((3, fb.value), np.uint8)
    mdct = np.zeros((3, 6, 6, 256), np.int32)
    expo = np.zeros((3, 6, 6, 256), np.uint8)
    eexp = np.zeros((3, 6, 6, 256), np.uint8)
    bap = np.zeros((3, 6, 6, 256), np.uint8)
    strat = np.zeros((3, 6, 6), np.uint8)
    shift = np.zeros((3, 6, 6), np.int8)
    snr = np.zeros((3, 2), np.int32)
    for f in range(3):
        assert L.orc_ac3enc_frame(h, H.P(frames[f], H.u8p), ctypes.cast(pcm_in.ctypes.data + f * 1536 * 12, H.i16p), cm) == fb.value
        L.orc_ac3enc_get_mdct(h, H.P(mdct[f], H.i32p))
        L.orc_ac3enc_get_exp(h, H.P(expo[f], H.u8p), H.P(eexp[f], H.u8p))
        L.orc_ac3enc_get_bap(h, H.P(bap[f], H.u8p))
        c, fs = H.ci(), H.ci()
        L.orc_ac3enc_get_misc(h, H.P(strat[f], H.u8p), H.P(shift[f], H.i8p), ctypes.byref(c), ctypes.byref(fs))
        snr[f] = (c.value, fs.value)
    L.orc_ac3enc_free(h)
    cos, sin, xc, xs = (np.zeros(n, np.int16) for n in (64, 64, 128, 128))
    crc = np.zeros(256, np.uint16)
    L.orc_ac3enc_tables(H.P(cos, H.i16p), H.P(sin, H.i16p), H.P(xc, H.i16p), H.P(xs, H.i16p), H.P(crc, H.u16p))
    np.savez_compressed(os.path.join(OUT, "encoder.npz"), pcm_in=pcm_in, frames=frames, mdct=mdct, exponent=expo,
                        encoded_exp=eexp, bap=bap, exp_strategy=strat, exp_samples=shift, snroffst=snr,
                        costab=cos, sintab=sin, xcos1=xc, xsin1=xs, crc_table=crc)
    # ---- packer streams: coupling, rematrix, delta bit allocation, dynrng, block switching ... --------
    from tests import packer
    d = {}
    for tag, acmod, lfe, fscod, bsid, fsz, flags in (("a7", 7, 1, 0, 8, 36, 7 | 16), ("a7_st", 7, 1, 0, 8, 36, 2 | 32),
                                                    ("a2", 2, 0, 0, 8, 30, 2), ("a2_mono", 2, 0, 1, 8, 31, 1),
                                                    ("a0", 0, 0, 2, 8, 28, 0), ("a5_half", 5, 1, 0, 9, 36, 5 | 16),
                                                    ("a3_dolby", 3, 0, 0, 10, 34, 10)):
        fr = packer.make_stream(4242 + acmod, 3, acmod, lfe, fscod=fscod, bsid=bsid, frmsizecod=fsz)
        pcm, errs, oflags = H.ref_decode(fr, flags, 1.0, 0.0)
        assert errs == 0
        d["frames_" + tag] = fr
        d["pcm_" + tag] = pcm
        d["args_" + tag] = np.array([flags, oflags], np.int32)
    np.savez_compressed(os.path.join(OUT, "packer.npz"), **d)
    make_mixflip()
    make_a52dec_drivers()
    make_ac3enc_ref()

    for fn in sorted(os.listdir(OUT)):
        if fn.endswith(".npz"):
            print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
