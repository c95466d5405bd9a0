"""Shared test plumbing: package import, oracle (liborc.so) and reference-build
(oracle/_ref/liba52_ref.so) bindings, liba52's stored sweep results, seeded synthetic inputs.

The oracle is TEST INFRASTRUCTURE: only tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg import this module.
"""
import atexit
import ctypes
import hashlib
import importlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORC_PATH = os.path.join(ORACLE_DIR, "liborc.so")
REF_PATH = os.path.join(ORACLE_DIR, "_ref", "liba52_ref.so")
REFENC_PATH = os.path.join(ORACLE_DIR, "_ref", "ac3enc_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")

u8p = ctypes.POINTER(ctypes.c_uint8)
i8p = ctypes.POINTER(ctypes.c_int8)
i16p = ctypes.POINTER(ctypes.c_int16)
u16p = ctypes.POINTER(ctypes.c_uint16)
i32p = ctypes.POINTER(ctypes.c_int32)
fp = ctypes.POINTER(ctypes.c_float)
ip = ctypes.POINTER(ctypes.c_int)
vp = ctypes.c_void_p
ci = ctypes.c_int
cf = ctypes.c_float

NFCHANS = (2, 1, 2, 3, 3, 4, 4, 5, 1, 1, 2)
CHMAP6 = (0, 2, 1, 4, 5, 3, 0, 0)      # create_channel_map, src/AC3ACM.cpp:1631-1662 (6-ch WAVE order)


def pkg():
    return importlib.import_module("ac-3-acm-codec_amd")


CSRC = os.path.join(ROOT, "ac-3-acm-codec_amd", "csrc")
SANITISE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
_LANG = {"c++": ["g++", "-std=c++17"], "c": ["gcc", "-std=c99"], "hip": ["g++", "-std=c++17", "-x", "c++"]}


def build_sanitised(sources, exe, lang=None, includes=()):
    """The one recipe of the stand-alone sanitiser programs: `sources` built by the host compiler with SANITISE, -Wall -Werror,
    into the program `exe`, which the caller runs on its own (never loaded into Python).  One source is compiled and linked
    in one call; several are compiled to objects beside `exe` and linked by g++.  lang: "c++", "c" or "hip" for every source,
    by default each one's by its suffix (.cpp, .c; .hip: a kernel file's host-only translation, compiled as C++).  includes:
    -I directories of the .c and .cpp sources (a .hip source finds its headers beside itself)."""
    def compile_(src):
        kind = lang or {".cpp": "c++", ".c": "c", ".hip": "hip"}[os.path.splitext(src)[1]]
        inc = [] if kind == "hip" else [a for d in includes for a in ("-I", d)]
        return _LANG[kind] + SANITISE + ["-Wall", "-Werror"] + inc
    if len(sources) == 1:
        cmds = [compile_(sources[0]) + [sources[0], "-o", exe]]
    else:
        objs = [os.path.join(os.path.dirname(exe), os.path.splitext(os.path.basename(s))[0] + ".o") for s in sources]
        assert len(set(objs)) == len(objs)
        cmds = [compile_(s) + ["-c", s, "-o", o] for s, o in zip(sources, objs)] + [["g++"] + SANITISE + objs + ["-o", exe]]
    for cmd in cmds:
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return exe


def P(a, t):
    return a.ctypes.data_as(t)


_orc = None
_ref = None


def build_oracle():
    if not os.path.exists(ORC_PATH) or os.path.getmtime(ORC_PATH) < max(
            os.path.getmtime(os.path.join(ORACLE_DIR, f)) for f in ("a52_oracle.c", "ac3enc_oracle.c", "orc.h")):
        subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, os.path.join(ORACLE_DIR, "liborc.so")])


def orc():
    global _orc
    if _orc is not None:
        return _orc
    build_oracle()
    L = ctypes.CDLL(ORC_PATH)
    L.orc_a52_init.restype = vp
    L.orc_a52_samples.restype = fp
    L.orc_a52_samples.argtypes = [vp]
    L.orc_a52_syncinfo.argtypes = [u8p, ip, ip, ip]
    L.orc_a52_frame.argtypes = [vp, u8p, ip, fp, cf]
    L.orc_a52_block.argtypes = [vp]
    L.orc_a52_free.argtypes = [vp]
    L.orc_a52_free.restype = None
    L.orc_a52_dynrng.argtypes = [vp, vp, vp]
    L.orc_a52_get_exp.argtypes = [vp, ci, u8p]
    L.orc_a52_get_bap.argtypes = [vp, ci, i8p]
    L.orc_a52_get_lfsr.argtypes = [vp]
    L.orc_a52_set_lfsr.argtypes = [vp, ci]
    L.orc_a52_bitpos.argtypes = [vp]
    L.orc_a52_bitpos.restype = ctypes.c_long
    L.orc_imdct_512.argtypes = [fp, fp, cf]
    L.orc_imdct_256.argtypes = [fp, fp, cf]
    L.orc_imdct_tables.argtypes = [fp] * 5
    L.orc_downmix_init.argtypes = [ci, ci, fp, cf, cf]
    L.orc_downmix_coeff.argtypes = [fp, ci, ci, cf, cf, cf]
    L.orc_downmix.argtypes = [fp, ci, ci, cf, cf, cf]
    L.orc_upmix.argtypes = [fp, ci, ci]
    L.orc_xform_batch.argtypes = [fp, u8p, fp, ip, fp, ci, ci, ci, ci, ci, cf, cf, cf]
    L.orc_convert_s16.argtypes = [fp, i16p, ci]
    L.orc_a52_decode_frames.argtypes = [u8p, ci, ci, ci, cf, cf, fp]
    L.orc_ac3enc_init.restype = vp
    L.orc_ac3enc_init.argtypes = [ci, ci, ci, ip]
    L.orc_ac3enc_frame.argtypes = [vp, u8p, i16p, u8p]
    L.orc_ac3enc_free.argtypes = [vp]
    L.orc_ac3enc_free.restype = None
    L.orc_ac3enc_get_mdct.argtypes = [vp, i32p]
    L.orc_ac3enc_get_exp.argtypes = [vp, u8p, u8p]
    L.orc_ac3enc_get_bap.argtypes = [vp, u8p]
    L.orc_ac3enc_get_misc.argtypes = [vp, u8p, i8p, ip, ip]
    L.orc_ac3enc_tables.argtypes = [i16p, i16p, i16p, i16p, u16p]
    L.orc_ac3enc_index_tables.argtypes = [u8p, u8p, u8p]
    L.orc_ac3enc_get_status.argtypes = [vp, ip, ip]
    L.orc_ac3enc_set_last.argtypes = [vp, i16p]
    L.orc_ac3enc_get_last.argtypes = [vp, i16p]
    L.orc_ac3enc_mdct512.argtypes = [i32p, i16p]
    L.orc_ac3enc_encode_frames.argtypes = [ci, ci, ci, i16p, ci, u8p, u8p]
    _orc = L
    return L


def have_ref():
    return os.path.exists(REF_PATH)


def ref():
    """The real liba52 built from /root/reference by oracle/Makefile (this container,
    or the prebuilt binary shipped to the GPU box)."""
    global _ref
    if _ref is not None:
        return _ref
    L = ctypes.CDLL(REF_PATH)
    L.a52_init.restype = vp
    L.a52_init.argtypes = [ctypes.c_uint32]
    L.a52_samples.restype = fp
    L.a52_samples.argtypes = [vp]
    L.a52_syncinfo.argtypes = [u8p, ip, ip, ip]
    L.a52_frame.argtypes = [vp, u8p, ip, fp, cf]
    L.a52_block.argtypes = [vp]
    L.a52_dynrng.argtypes = [vp, vp, vp]
    L.a52_free.argtypes = [vp]
    L.a52_free.restype = None
    L.a52_imdct_init.argtypes = [ctypes.c_uint32]
    L.a52_imdct_512.argtypes = [fp, fp, cf]
    L.a52_imdct_256.argtypes = [fp, fp, cf]
    L.a52_downmix_init.argtypes = [ci, ci, fp, cf, cf]
    L.a52_downmix_coeff.argtypes = [fp, ci, ci, cf, cf, cf]
    L.a52_downmix.argtypes = [fp, ci, ci, cf, cf, cf]
    L.a52_upmix.argtypes = [fp, ci, ci]
    L.refglue_get_exp.argtypes = [vp, ci, u8p]
    L.refglue_get_bap.argtypes = [vp, ci, i8p]
    L.refglue_get_lfsr.argtypes = [vp]
    L.refglue_bitpos.argtypes = [vp, u8p]
    L.refglue_bitpos.restype = ctypes.c_long
    L.convert2s16_multi.argtypes = [fp, i16p, ci]
    L.convert2s16_2.argtypes = [fp, i16p]
    L.a52_imdct_init(0)
    _ref = L
    return L


def have_refenc():
    return os.path.exists(REFENC_PATH)


REFENC_ARRAYS = {"mdct_coef": (np.int32, (6, 6, 256)), "exponent": (np.uint8, (6, 6, 256)), "exp_strategy": (np.uint8, (6, 6)),
                 "encoded_exp": (np.uint8, (6, 6, 256)), "bap": (np.uint8, (6, 6, 256)), "exp_samples": (np.int8, (6, 6)),
                 "costab": (np.int16, (64,)), "sintab": (np.int16, (64,)), "xcos1": (np.int16, (128,)), "xsin1": (np.int16, (128,)),
                 "fft_rev": (np.int16, (512,)), "crc_table": (np.uint16, (256,)), "bndtab": (np.uint8, (51,)), "masktab": (np.uint8, (253,))}
REFENC_TABLES = ("costab", "sintab", "xcos1", "xsin1", "fft_rev", "crc_table", "bndtab", "masktab")


class RefEncoder:
    """One fresh instance of the reference's own ac3enc (oracle/ref_ac3enc_glue.cpp -> oracle/_ref/ac3enc_ref.so).  The
    reference keeps a single static context that its init does not clear, so every instance is a privately copied
    library: its statics start zeroed and no other instance shares them."""

    def __init__(self):
        fd, self.path = tempfile.mkstemp(prefix="ac3enc_ref_", suffix=".so")
        os.close(fd)
        shutil.copyfile(REFENC_PATH, self.path)
        L = self.L = ctypes.CDLL(self.path)
        os.unlink(self.path)                               # the mapping keeps the copy alive
        L.refenc_init.argtypes = [ci, ci, ci]
        L.refenc_frame.argtypes = [u8p, i16p, u8p]
        L.refenc_array.restype = vp
        L.refenc_array.argtypes = [ctypes.c_char_p, ip, ip]
        L.refenc_snr.argtypes = [ip]
        L.refenc_assert_trips.argtypes = [ip]
        self.frame_bytes = 0
        self.nch = 0

    def init(self, freq, bitrate, channels):
        self.frame_bytes = self.L.refenc_init(freq, bitrate, channels)
        self.nch = channels
        return self.frame_bytes

    def frame(self, samples, chmap):
        """Encodes 1536 x nch interleaved s16 samples -> (returned size, the frame's bytes).  self.yack says whether the
        reference reported on stderr that its search failed (ac3enc.cpp:930-933: the only trace it leaves, its caller
        ignores the result)."""
        dst = np.zeros(32768, np.uint8)                    # the reference's bit writer does not check its end
        samples = np.ascontiguousarray(samples, np.int16)
        assert samples.size == 1536 * self.nch
        cm = (ctypes.c_uint8 * 8)(*(tuple(chmap) + (0,) * 8)[:8])
        with tempfile.TemporaryFile() as err:
            saved = os.dup(2)
            os.dup2(err.fileno(), 2)
            try:
                r = self.L.refenc_frame(P(dst, u8p), P(samples, i16p), cm)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            err.seek(0)
            self.yack = b"Yack" in err.read()
        return r, dst[:self.frame_bytes].copy()

    def encode(self, pcm, chmap):
        """pcm [frames * 1536][nch] -> ([frames][frame_bytes] u8, [frames] returned sizes)."""
        pcm = np.ascontiguousarray(pcm, np.int16).reshape(-1, 1536, self.nch)
        out = [self.frame(x, chmap) for x in pcm]
        return np.stack([o[1] for o in out]), np.array([o[0] for o in out], np.int32)

    def array(self, name):
        dt, shape = REFENC_ARRAYS[name]
        n, eb = ci(), ci()
        ptr = self.L.refenc_array(name.encode(), ctypes.byref(n), ctypes.byref(eb))
        assert ptr and n.value == int(np.prod(shape)) and eb.value == np.dtype(dt).itemsize, name
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), (n.value,)).reshape(shape).copy()

    def snr(self):
        """(csnroffst, fsnroffst[6], fgaincod[6]) of the context."""
        a = np.zeros(13, np.int32)
        self.L.refenc_snr(P(a, ip))
        return int(a[0]), a[1:7].copy(), a[7:13].copy()

    def assert_trips(self):
        """(how many of the reference's own _ASSERT conditions did not hold so far, {source line: trips})."""
        sites = np.zeros((16, 2), np.int32)
        n = self.L.refenc_assert_trips(P(sites, ip))
        return n, {int(l): int(c) for l, c in sites if l}


# ---------------------------------------------------------------------------
# synthetic inputs

def gen_pcm(nframes, nch=6, seed=12345, kind="tones"):
    """s16 interleaved WAVE-order PCM, 1536*nframes samples per channel.

    tones : per channel a sine (amp 8000, phase step 0.01*(c+1) + slow chirp) + uniform noise +-2048
    noise : full-scale white noise (stresses bit allocation, many new-exponent blocks)
    quiet : digital silence with an occasional +-1 (exp 24, zero bap, dither path)
    music : a few in-band partials per channel, low noise (codes well: SNR check)
    bursts: tones whose level jumps x1 <-> x1/64 at random block boundaries per channel (new exponent sets in most
            blocks: D15/D25/D45 mixes, bit allocation in most blocks)
    strobe: the same with the level alternating every block (new exponents in all 36 channel-blocks: the encoder's
            per-block search sweep)
    """
    n = nframes * 1536
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    out = np.zeros((n, nch), np.float64)
    for c in range(nch):
        if kind == "tones":
            out[:, c] = 8000 * np.sin(0.01 * (c + 1) * t + 1e-7 * (c + 1) * t * t) + rng.integers(-2048, 2049, n)
        elif kind == "noise":
            out[:, c] = rng.integers(-30000, 30001, n)
        elif kind == "quiet":
            out[:, c] = (rng.random(n) < 0.001) * rng.integers(-1, 2, n)
        elif kind == "music":
            for k in range(4):
                out[:, c] += 2500 * np.sin(2 * np.pi * (110.0 * (c + 1) * (k + 1) / 48000.0) * t + k)
            out[:, c] += rng.integers(-8, 9, n)
        elif kind == "bursts":
            base = 12000 * np.sin(0.013 * (c + 1) * t) + rng.integers(-3000, 3001, n)
            gain = np.where(rng.random(n // 256) < 0.5, 1.0, 1.0 / 64)
            out[:, c] = base * np.repeat(gain, 256)
        elif kind == "strobe":
            base = 12000 * np.sin(0.013 * (c + 1) * t) + rng.integers(-3000, 3001, n)
            out[:, c] = base * np.repeat(np.where(np.arange(n // 256) % 2 == 0, 1.0, 1.0 / 64), 256)
        elif kind == "silence":
            pass
        elif kind == "rails":                   # full-scale square waves incl. -32768 (abs(-32768), int16 wrap in the FFT)
            period = 2 + 3 * c
            out[:, c] = np.where((np.arange(n) // period) % 2 == 0, 32767, -32768)
        elif kind == "impulses":                # one full-scale sample every ~300 samples over digital silence
            out[(np.arange(n) % (293 + 17 * c)) == 5 * c, c] = -32768 if c % 2 else 32767
        elif kind == "dc":                      # constant full-scale level, a different sign per channel
            out[:, c] = -32768 if c % 2 else 32767
        else:
            raise ValueError(kind)
    return np.clip(np.round(out), -32768, 32767).astype(np.int16)


def orc_encode(pcm, nch=6, bitrate=384000, freq=48000, chmap=CHMAP6):
    """Encode interleaved s16 PCM as one stream with the encoder oracle -> [nframes][frame_bytes] u8."""
    L = orc()
    nframes = pcm.shape[0] // 1536
    fb = ci()
    h = L.orc_ac3enc_init(freq, bitrate, nch, ctypes.byref(fb))
    assert h, "orc_ac3enc_init rejected %d/%d/%d" % (freq, bitrate, nch)
    out = np.zeros((nframes, fb.value), np.uint8)
    cm = (ctypes.c_uint8 * 8)(*chmap)
    pcm = np.ascontiguousarray(pcm)
    for f in range(nframes):
        r = L.orc_ac3enc_frame(h, P(out[f], u8p), ctypes.cast(pcm.ctypes.data + f * 1536 * nch * 2, i16p), cm)
        assert r == fb.value, "oracle encoder failed on frame %d" % f
    L.orc_ac3enc_free(h)
    return out


def _decode_stream(L, prefix, frames, flags, level, bias, dynrng_off=False, taps=False):
    init = getattr(L, prefix + "init")
    st = init() if prefix == "orc_a52_" else init(0)
    nfr, fb = frames.shape
    buf = np.zeros(nfr * fb + 64, np.uint8)
    buf[:nfr * fb] = frames.reshape(-1)
    pcm, errs, outflags = [], 0, flags
    for f in range(nfr):
        fl, lv = ci(flags), cf(level)
        p = ctypes.cast(buf.ctypes.data + f * fb, u8p)
        errs += getattr(L, prefix + "frame")(st, p, ctypes.byref(fl), ctypes.byref(lv), bias)
        if dynrng_off:
            getattr(L, prefix + "dynrng")(st, None, None)
        outflags = fl.value
        nout = NFCHANS[outflags & 15] + (1 if outflags & 16 else 0)
        for b in range(6):
            errs += getattr(L, prefix + "block")(st)
            pcm.append(np.ctypeslib.as_array(getattr(L, prefix + "samples")(st), (1536,))[:nout * 256].copy())
    getattr(L, prefix + "free")(st)
    nout = NFCHANS[outflags & 15] + (1 if outflags & 16 else 0)
    return np.array(pcm, np.float32).reshape(nfr, 6, nout, 256), errs, outflags


def orc_decode(frames, flags=7 | 16, level=1.0, bias=0.0, dynrng_off=False):
    return _decode_stream(orc(), "orc_a52_", frames, flags, level, bias, dynrng_off)


def orc_decode_status(frames, flags, bias=0.0, level=1.0, dynrng_off=False, state=None):
    """the restatement on [S][F][fb], a fresh decoder per stream -> (status bits 0-5 and 8 per frame, pcm [S][F][6][n_out][256],
    per stream the number of leading frames it decoded whole).  level: a52_frame's; dynrng_off: a52_dynrng(state, NULL, NULL)
    after every a52_frame, as the drivers call it; state = (delay [S][n_out][128], lfsr [S]): what each stream's overlap planes
    (one per output plane, for requests without a downmix) and dither generator hold at its start, instead of zeros and 1.  A frame is refused by a52_syncinfo (as the drivers call it
    ahead of a52_frame), for a size above the batch's or a layout other than the batch's (stream 0's), or by a52_frame.  After
    a frame it refuses or a block that fails, liba52's caller decides what the overlap tails become, so a stream's PCM is
    compared up to there only."""
    L = orc()
    S, F, fb = frames.shape
    layout = None
    status = np.zeros((S, F), np.uint32)
    whole = np.zeros(S, np.int64)
    pcm = None
    for s in range(S):
        st = L.orc_a52_init()
        if state is not None:
            planes = np.ctypeslib.as_array(L.orc_a52_samples(st), (3072,))[1536:].reshape(6, 256)
            planes[:state[0].shape[1], :128] = state[0][s]
            L.orc_a52_set_lfsr(st, int(state[1][s]) & 0xffff)
        ok = True
        for f in range(F):
            buf = np.zeros(fb + 64, np.uint8)
            buf[:fb] = frames[s, f]
            fl, lv = ci(flags), cf(level)
            sf, sr, br = ci(), ci(), ci()
            n = L.orc_a52_syncinfo(P(buf, u8p), ctypes.byref(sf), ctypes.byref(sr), ctypes.byref(br))
            coded = sf.value & 0x1f
            if coded & 15 == 10:                   # a 2/0 frame whose dsurmod says Dolby Surround: the same coded layout
                coded ^= 8
            if layout is None:
                assert n == fb and (s, f) == (0, 0)
                layout = coded
            if n == 0 or n > fb or coded != layout or L.orc_a52_frame(st, P(buf, u8p), ctypes.byref(fl), ctypes.byref(lv), bias):
                status[s, f] = 0x13f
                ok = False
                continue
            if dynrng_off:
                L.orc_a52_dynrng(st, None, None)
            n_out = NFCHANS[fl.value & 15] + (1 if fl.value & 16 else 0)
            if pcm is None:
                pcm = np.zeros((S, F, 6, n_out, 256), np.float32)
            for b in range(6):
                if L.orc_a52_block(st):
                    status[s, f] = (0x3f << b) & 0x3f
                    ok = False
                    break
                if ok:
                    pcm[s, f, b] = np.ctypeslib.as_array(L.orc_a52_samples(st), (1536,))[:n_out * 256].reshape(n_out, 256)
            whole[s] += ok
        L.orc_a52_free(st)
    return status, pcm, whole


def ref_decode(frames, flags=7 | 16, level=1.0, bias=0.0, dynrng_off=False):
    return _decode_stream(ref(), "a52_", frames, flags, level, bias, dynrng_off)


# ---------------------------------------------------------------------------
# the real liba52's results on the seeded sweeps, stored for machines without oracle/_ref

LIBA52_RECORDS = os.path.join(GOLDEN, "liba52_records.json")
_records = None


def fingerprint(*parts):
    """Bit-exact fingerprint (sha256, 128 bits kept) of arrays (dtype, shape and bytes) and plain values."""
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, np.ndarray):
            a = np.ascontiguousarray(p)
            h.update(("%s%r" % (a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        else:
            h.update(repr(p).encode())
        h.update(b"|")
    return h.hexdigest()[:32]


def _save_records():
    with open(LIBA52_RECORDS, "w") as f:
        json.dump(_records, f, indent=0, sort_keys=True)
        f.write("\n")


def liba52_record(key, live):
    """The real liba52's result for one sweep case, as a JSON value.  Where oracle/_ref exists it is computed by live()
    and must equal the one stored in tests/golden/liba52_records.json; elsewhere the stored one stands in for it.
    With oracle/_ref and AC3MI_RECORD_LIBA52=1 the computed results are written to that file instead (at exit)."""
    global _records
    recording = os.environ.get("AC3MI_RECORD_LIBA52") == "1"
    if _records is None:
        _records = {}
        if os.path.exists(LIBA52_RECORDS):
            with open(LIBA52_RECORDS) as f:
                _records = json.load(f)
        if recording:
            atexit.register(_save_records)
    if have_ref():
        rec = json.loads(json.dumps(live()))
        if recording:
            _records[key] = rec
        else:
            assert _records.get(key) == rec, "liba52 gives %r for case %s, %s holds %r" % (
                rec, key, os.path.basename(LIBA52_RECORDS), _records.get(key))
        return rec
    assert key in _records, "case %s has no stored liba52 result in %s" % (key, os.path.basename(LIBA52_RECORDS))
    return _records[key]


def decode_record(pcm, errs, flags):
    """[fingerprint of the PCM's bits, summed return codes, output flags] of a decoded stream."""
    return [fingerprint(np.ascontiguousarray(pcm, np.float32).view(np.uint32)), int(errs), int(flags)]


def ref_decode_record(frames, flags=7 | 16, level=1.0, bias=0.0, dynrng_off=False):
    """decode_record of the real liba52's decode of one stream (computed, or stored: liba52_record)."""
    key = "decode:" + fingerprint(np.ascontiguousarray(frames, np.uint8), int(flags), float(level), float(bias), bool(dynrng_off))
    return liba52_record(key, lambda: decode_record(*ref_decode(frames, flags, level, bias, dynrng_off)))


def orc_xform(coef, blksw, acmod, lfeon, output, bias=0.0, clev=0.0, slev=0.0, state=None):
    """Transform-only oracle.  coef [S][F][6][n_in][256] -> pcm [S][F][6][n_out][256];
    returns (pcm, (planes, downmixed)) with the liba52-style carry-over state."""
    L = orc()
    S, F = coef.shape[:2]
    n_out = NFCHANS[output & 15] + (1 if output & 16 else 0)
    if state is None:
        state = (np.zeros((S, 3072), np.float32), np.ones(S, np.int32))
    planes, dm = state
    pcm = np.zeros((S, F, 6, n_out, 256), np.float32)
    coef = np.ascontiguousarray(coef, np.float32)
    sw = None if blksw is None else np.ascontiguousarray(blksw, np.uint8)
    r = L.orc_xform_batch(P(coef, fp), P(sw, u8p) if sw is not None else None, P(planes, fp), P(dm, ip),
                          P(pcm, fp), S, F, acmod, lfeon, output, bias, clev, slev)
    assert r == 0
    return pcm, (planes, dm)


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0
