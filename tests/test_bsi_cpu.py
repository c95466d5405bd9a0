"""CPU: ac3mi_bsi_read and ac3mi_encode_metadata_word (host code of libac3mi.so, no GPU) against tests/ac3_syntax.py and
tests/bsi_model.py.

Frames: 1 008 packer.make_frame frames - every acmod, both lfeon values, bsi_opts 0, 0.5 and 1, 21 each, all three sample rates
and the half-rate bsids among them - which bring reserved codes 3, dialnorm 0, both dual-mono programmes and addbsi of 1 to 4
bytes (the packer writes no longer one).  addbsi of up to 64 bytes, which only the reader's skip has to get right, comes
from 3 000 heads written here field by field (syncinfo + BSI + random bytes: the reader never looks behind the BSI)."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import _harness as H
from tests import ac3_syntax as A
from tests import bsi_model as M
from tests import packer

NAMES = ("verdict", "fscod", "frmsizecod", "bsid", "bsmod", "acmod", "lfeon", "cmixlev", "surmixlev", "dsurmod", "dialnorm",
         "dialnorm2", "compr", "compr2", "langcod", "langcod2", "audprodi", "audprodi2", "copyrightb", "origbs", "addbsil",
         "present", "timecod1", "timecod2", "block0_bit", "word")


def _read(data):
    return H.pkg().bsi_read(data)


def _as_dict(rec):
    assert rec["reserved"] == 0 and rec["reserved2"] == 0
    return {k: int(rec[k]) for k in NAMES}


@pytest.fixture(scope="module")
def packer_frames():
    out = []
    for acmod in range(8):
        for lfeon in (0, 1):
            for opts in (0.0, 0.5, 1.0):
                rng = np.random.default_rng(1000 * acmod + 100 * lfeon + int(10 * opts))
                for i in range(21):
                    kw = (dict(frmsizecod=20), dict(fscod=1, frmsizecod=21), dict(fscod=2, frmsizecod=16), dict(bsid=9, frmsizecod=24),
                          dict(bsid=10, frmsizecod=18), dict(bsid=6, frmsizecod=22))[i % 6]
                    if A.NFCHANS[acmod] >= 4:
                        kw = dict(kw, frmsizecod=kw["frmsizecod"] + 8)
                    out.append(packer.make_frame(rng, acmod, lfeon, features=dict(bsi_opts=opts), **kw))
    return out


def test_reader_agrees_with_ac3_syntax_on_packer_frames(packer_frames):
    seen = dict(c3=0, s3=0, d3=0, dn0=0, dual=0, addbsi=set())
    for fr in packer_frames:
        P = M.parse_head(fr)
        want = M.info_of(P)
        got = _as_dict(_read(fr))
        assert got == want, (got, want)
        assert got["word"] == M.sanitise(got["word"])
        g = P.fields
        seen["c3"] += g.get("cmixlev") == 3
        seen["s3"] += g.get("surmixlev") == 3
        seen["d3"] += g.get("dsurmod") == 3
        seen["dn0"] += g["dialnorm"] == 0
        seen["dual"] += P.acmod == 0 and g["dialnorm2"] != g["dialnorm"]
        if g.get("addbsie"):
            seen["addbsi"].add(g["addbsil"] + 1)
        # the head alone reads the same: the frame's own size is not held against len
        nb = (P.header_bits + 7) // 8
        assert _as_dict(_read(fr[:nb])) == want
    assert len(packer_frames) == 1008
    assert seen["c3"] and seen["s3"] and seen["dn0"] and seen["dual"] and seen["addbsi"] == {1, 2, 3, 4}, seen
    assert seen["d3"] == 0          # (the packer never writes dsurmod 3: the synthetic heads below do)


def _synthetic_head(rng):
    """syncinfo + a random BSI (addbsi of 1..64 bytes half of the time) + 8 random bytes -> bytes"""
    bits = []

    def put(n, v):
        bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    acmod = int(rng.integers(0, 8))
    put(16, 0x0b77)
    put(16, int(rng.integers(0, 65536)))
    put(2, int(rng.integers(0, 3)))
    put(6, int(rng.integers(0, 38)))
    put(5, int(rng.integers(0, 11)))                # (ac3_syntax reads bsid 0..10)
    put(3, int(rng.integers(0, 8)))
    put(3, acmod)
    for k in ("cmixlev", "surmixlev", "dsurmod"):
        if k in M.sends(acmod):
            put(2, int(rng.integers(0, 4)))
    put(1, int(rng.integers(0, 2)))
    for _ in range(2 if acmod == 0 else 1):
        put(5, int(rng.integers(0, 32)))
        for width in (8, 8, 7):
            e = int(rng.integers(0, 2))
            put(1, e)
            if e:
                put(width, int(rng.integers(0, 1 << width)))
    put(2, int(rng.integers(0, 4)))
    for _ in range(2):
        e = int(rng.integers(0, 2))
        put(1, e)
        if e:
            put(14, int(rng.integers(0, 1 << 14)))
    e = int(rng.integers(0, 2))
    put(1, e)
    if e:
        n = int(rng.integers(0, 64))
        put(6, n)
        for _ in range(n + 1):
            put(8, int(rng.integers(0, 256)))
    while len(bits) % 8:
        bits.append(int(rng.integers(0, 2)))
    return np.packbits(np.array(bits, np.uint8)).tobytes() + rng.integers(0, 256, 8, dtype=np.uint8).tobytes()


def test_reader_agrees_with_ac3_syntax_on_synthetic_heads():
    rng = np.random.default_rng(64)
    lens, d3 = set(), 0
    for _ in range(3000):
        head = _synthetic_head(rng)
        P = M.parse_head(head)
        want = M.info_of(P)
        assert _as_dict(_read(head)) == want
        if P.fields.get("addbsie"):
            lens.add(P.fields["addbsil"] + 1)
        d3 += P.fields.get("dsurmod") == 3
    assert {1, 64} <= lens and len(lens) >= 60 and d3


def test_verdict_bits(packer_frames):
    fr = np.array(packer_frames[5], np.uint8)
    assert _read(fr)["verdict"] == 0
    blank = {k: 0 for k in NAMES}
    for pos, val in ((0, 0x0a), (1, 0x00), (4, (fr[4] & 0xc0) | 38), (4, (fr[4] & 0xc0) | 63), (4, fr[4] | 0xc0), (5, 0x60 | (fr[5] & 7)),
                     (5, 0xf8 | (fr[5] & 7))):
        bad = fr.copy()
        bad[pos] = val
        assert _as_dict(_read(bad)) == dict(blank, verdict=0x80), (pos, val)
    for n in range(6):
        assert _read(fr[:n])["verdict"] == 0x80
    # bsid 11 is the last one a52_syncinfo accepts
    ok = fr.copy()
    ok[5] = 0x58 | (fr[5] & 7)
    assert _read(ok)["verdict"] == 0 and _read(ok)["bsid"] == 11
    # cut inside addbsi, at every byte from its first to its last: bit 6, the fields read up to there, no block offset
    rng = np.random.default_rng(6)
    cut = 0
    while cut < 20:
        head = _synthetic_head(rng)
        P = M.parse_head(head)
        if not P.fields.get("addbsie"):
            continue
        first = (P.pos["addbsi"] + 7) // 8
        want = dict(M.info_of(P), verdict=0x40, block0_bit=0)
        for n in range(first, (P.header_bits + 7) // 8):
            assert _as_dict(_read(head[:n])) == want, n
        assert _read(head[:(P.header_bits + 7) // 8])["verdict"] == 0
        cut += 1
    # cut before origbs: bit 6 again, and the word holds what was read
    short = _as_dict(_read(fr[:7]))
    assert short["verdict"] == 0x40 and short["acmod"] == M.parse_head(fr).acmod and short["block0_bit"] == 0
    lib = H.pkg().load_library()
    buf = (ctypes.c_uint8 * 8)()
    capi = importlib.import_module(H.pkg().__name__ + ".capi")
    info = capi.BsiInfoC()
    assert lib.ac3mi_bsi_read(None, 8, ctypes.byref(info)) == -1
    assert lib.ac3mi_bsi_read(buf, -1, ctypes.byref(info)) == -1
    assert lib.ac3mi_bsi_read(buf, 8, None) == -1


def test_sanitising_rule_and_source_word():
    assert M.sanitise(M.pack_word(dialnorm=0, bsmod=5, cmixlev=3, surmixlev=3, dsurmod=3, copyrightb=1, origbs=0)) == \
        M.pack_word(dialnorm=31, bsmod=5, cmixlev=1, surmixlev=1, dsurmod=0, copyrightb=1, origbs=0)
    for w in range(0, 1 << 16, 7):
        s = M.sanitise(w | 0xabcd0000)
        f = M.fields_of(s)
        assert s < (1 << 16) and f["dialnorm"] and f["cmixlev"] < 3 and f["surmixlev"] < 3 and f["dsurmod"] < 3 and M.sanitise(s) == s
        g = M.fields_of(w)
        assert all(f[k] == g[k] for k in ("bsmod", "copyrightb", "origbs"))
    # a 1/0 frame sends none of the three mix fields: the word holds the defaults
    rng = np.random.default_rng(10)
    fr = packer.make_frame(rng, 1, 0, frmsizecod=16)
    f = M.fields_of(int(_read(fr)["word"]))
    assert (f["cmixlev"], f["surmixlev"], f["dsurmod"]) == (1, 1, 0)


def test_encode_metadata_word():
    pkg = H.pkg()
    assert pkg.encode_metadata_word() == M.pack_word() == 31 | 1 << 8 | 1 << 10 | 1 << 15
    rng = np.random.default_rng(2)
    for _ in range(300):
        f = dict(dialnorm=int(rng.integers(1, 32)), bsmod=int(rng.integers(0, 8)), cmixlev=int(rng.integers(0, 3)),
                 surmixlev=int(rng.integers(0, 3)), dsurmod=int(rng.integers(0, 3)), copyrightb=int(rng.integers(0, 2)),
                 origbs=int(rng.integers(0, 2)))
        w = pkg.encode_metadata_word(**f)
        assert w == f["dialnorm"] | f["bsmod"] << 5 | f["cmixlev"] << 8 | f["surmixlev"] << 10 | f["dsurmod"] << 12 | \
            f["copyrightb"] << 14 | f["origbs"] << 15
        assert w == M.pack_word(**f) == M.sanitise(w)
    for k, bad in (("dialnorm", (0, 32, -1)), ("bsmod", (-1, 8)), ("cmixlev", (-1, 3)), ("surmixlev", (-1, 3)), ("dsurmod", (-1, 3)),
                   ("copyrightb", (-1, 2)), ("origbs", (-1, 2))):
        for v in bad:
            with pytest.raises(pkg.AC3MIError):
                pkg.encode_metadata_word(**{k: v})
    lib = pkg.load_library()
    md = (ctypes.c_int * 7)(31, 0, 1, 1, 0, 0, 1)
    w = ctypes.c_uint32(0x12345678)
    assert lib.ac3mi_encode_metadata_word(None, ctypes.byref(w)) == -1 and lib.ac3mi_encode_metadata_word(md, None) == -1
    md[0] = 0
    assert lib.ac3mi_encode_metadata_word(md, ctypes.byref(w)) == -1 and w.value == 0x12345678
