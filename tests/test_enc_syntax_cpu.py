"""CPU: the encoder's side-information syntax of csrc/enc_syntax.h - the field lists of the frame header and of an audio
block that both packers write through, the 64-bit field accumulator, the closed-form counts enc_packb_kernel places its
blocks by and the constant parts of the sum enc_search_kernel charges a frame - on every layout and tool flag.  The lists run in
tests/enc_syntax_c/main.cpp (see there for the shapes), a program of its own built with the host compiler under
-fsanitize=address,undefined; what it wrote is read back by tests/ac3_syntax.parse_frame, the independent reader.  Nothing
here comes from the engine."""
import os
import subprocess

import pytest

from tests import _harness as H
from tests import ac3_syntax as AS

DRAWS = 2               # drawn exponent-strategy patterns per shape, besides all-D15 and block-0-only
STRATS_READ = 3         # strategy patterns whose frames are read back per shape: the two extremes and the first draw


def _ints(s):
    return [int(v) for v in s.split(",")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("enc_syntax")
    exe = str(tmp / "enc_syntax")
    H.build_sanitised([os.path.join(H.ROOT, "tests", "enc_syntax_c", "main.cpp")], exe, includes=[H.CSRC])
    return exe


@pytest.fixture(scope="module")
def cases(exe):
    r = subprocess.run([exe, "20250", str(DRAWS), str(STRATS_READ)], capture_output=True, text=True)
    # (b) the accumulator never held more than 64 bits (the sink aborts with the field's position), and neither sanitiser spoke
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        c = dict(tok.split("=", 1) for tok in line.split(" "))
        for k in ("acmod", "lfe", "m", "chbwcod", "csnr", "fsnr", "fscod", "frmsizecod", "remat_on", "cplw", "begf", "endf", "fixed", "expbits", "end"):
            c[k] = int(c[k])
        for k in ("compr", "bsw", "dyn", "remat", "cstrat", "hdr", "blk", "cnt", "closed"):
            c[k] = _ints(c[k])
        c["nfbw"] = AS.NFCHANS[c["acmod"]]
        c["nch"] = c["nfbw"] + c["lfe"]
        c["strat"] = [[int(d) for d in c["strat"][b * c["nch"]:(b + 1) * c["nch"]]] for b in range(6)]
        out.append(c)
    return out


def test_group_counts(exe):
    """syn_exp_groups and syn_cpl_exp_groups, the one statement of the 7-bit group counts in csrc/, against the exponent-strategy
    model and the frame reader's own counts: every n in 1..253, every coupling range the setters can produce (cs = 37 + 12
    begf, ce = 73 + 12 endf, cs < ce), the three strategies"""
    from tests import exp_strategy_model as X
    r = subprocess.run([exe, "groups"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    ch, cpl = {}, {}
    for line in r.stdout.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        (ch if kind == "ch" else cpl)[tuple(v[:-1])] = v[-1]
    assert set(ch) == {(n, s) for n in range(1, 254) for s in (1, 2, 3)}
    assert set(cpl) == {(37 + 12 * b, 73 + 12 * e, s) for b in range(13) for e in range(13) if b <= e + 2 for s in (1, 2, 3)}
    for (n, s), g in ch.items():
        assert g == X.groups(n, s) == AS.chan_ngrps(n, s), (n, s, g)
    for (cs, ce, s), g in cpl.items():
        assert g == X.cpl_groups(cs, ce, s) == AS.cpl_ngrps(cs, ce, s), (cs, ce, s, g)
    assert ch[(7, 1)] == 2                  # nlfegrps


def test_the_matrix_is_whole(cases):
    """every acmod with and without the LFE; per layout every tool: metadata word, compr per programme, block switching, dynrng
    words in none / some / all blocks per programme (dual mono: independently), rematrixing in every subset of blocks 1..5,
    coupling at cplbegf 0, 2, 3 with cplendf 12 and 7, the two extreme strategy patterns"""
    for acmod in range(8):
        for lfe in (0, 1):
            cs = [c for c in cases if (c["acmod"], c["lfe"]) == (acmod, lfe)]
            assert {c["m"] != (31 | 1 << 8 | 1 << 10 | 1 << 15) for c in cs} == {False, True}     # the reference's BSI (dialnorm 31, cmixlev 1, surmixlev 1, origbs 1) and other words
            np_ = 2 if acmod == 0 else 1
            assert {tuple(w >> 8 for w in c["compr"][:np_]) for c in cs} == ({(0, 0), (1, 0), (0, 1), (1, 1)} if acmod == 0 else {(0,), (1,)})
            assert {any(c["bsw"]) for c in cs} == {False, True}
            sent = lambda c, p: sum(c["dyn"][2 * b + p] >> 8 for b in range(6))
            assert {tuple(sent(c, p) for p in range(np_)) for c in cs} == ({(a, b) for a in (0, 3, 6) for b in (0, 3, 6)} if acmod == 0 else {(0,), (3,), (6,)})
            if acmod == 2:
                assert {tuple(r >> 4 for r in c["remat"][1:]) for c in cs if c["remat_on"]} == {tuple((s >> i) & 1 for i in range(5)) for s in range(32)}
                assert any(not c["remat_on"] for c in cs)
            want_cpl = {(0, 0, 12)} | ({(1, b, e) for b in (0, 2, 3) for e in (12, 7)} if acmod >= 2 else set())
            assert {(c["cplw"] & 1, c["begf"], c["endf"]) for c in cs} == want_cpl
            assert any(all(s == 1 for row in c["strat"] for s in row) for c in cs)
            assert any(all(s == 0 for row in c["strat"][1:] for s in row) for c in cs)


def test_counts_agree(cases):
    """(a) written = counted for the header and every block of every case, and = the closed forms enc_packb_kernel places its
    blocks by wherever they apply (uncoupled frames)"""
    for i, c in enumerate(cases):
        assert c["hdr"][0] == c["hdr"][1] == c["hdr"][2], (i, c["hdr"])
        assert c["blk"] == c["cnt"], (i, c["blk"], c["cnt"])
        if c["cplw"] & 1:
            assert c["closed"] == [-1] * 6
        else:
            assert c["closed"] == c["blk"], (i, c["blk"], c["closed"])
        assert c["end"] == c["hdr"][0] + sum(c["blk"])


def test_priced_against_written(cases):
    """(c) what the search charges (syn_priced_fixed / syn_priced_cpl and the frame's own terms, + the channels' exponent bits) minus what the lists write is a function of
    the shape alone, term by term:"""
    for i, c in enumerate(cases):
        want = 16          # crc2, the frame's last word (ac3enc.cpp:915-916 "CRC"): behind the blocks, not side information
        want += 2          # auxdatae, crcrsv before it (ac3enc.cpp:912-913)
        if c["acmod"] == 2:
            # block 0's rematrixing flags, which the reference never prices (ac3enc.cpp:889 counts rematstr alone): 4 uncoupled,
            # liba52's cplinu-1 band set of 2 / 3 / 4 by cplbegf coupled
            want -= 4 if not c["cplw"] & 1 else 2 if c["begf"] == 0 else 3 if c["begf"] <= 2 else 4
        assert c["fixed"] + c["expbits"] - c["end"] == want, (i, c["fixed"], c["expbits"], c["end"], want)


def test_the_bytes_read_back(cases):
    """(d) the frames (exponents of zeros, offsets of zero: every bap 0, no mantissas) through parse_frame: no SyntaxError_, the
    fields that were put in, block 5 ending at the bit the sink reached"""
    n = 0
    for i, c in enumerate(cases):
        if not c["hex"]:
            continue
        n += 1
        fr = AS.parse_frame(bytes.fromhex(c["hex"]), check_size=False)
        F, m, acmod, nfbw = fr.fields, c["m"], c["acmod"], c["nfbw"]
        assert (fr.header_bits, fr.block_end[5]) == (c["hdr"][0], c["end"]), i
        assert [b.side_bits for b in fr.blocks] == c["blk"] and fr.mant_bits == [0] * 6, i
        assert (F["fscod"], F["frmsizecod"], F["bsid"], acmod, F["lfeon"]) == (c["fscod"], c["frmsizecod"], 8, F["acmod"], c["lfe"]), i
        assert (F["dialnorm"], F["bsmod"], F["copyrightb"], F["origbs"]) == (m & 31, (m >> 5) & 7, (m >> 14) & 1, (m >> 15) & 1), i
        assert (F.get("cmixlev"), F.get("surmixlev"), F.get("dsurmod")) == (
            (m >> 8) & 3 if (acmod & 1) and acmod != 1 else None, (m >> 10) & 3 if acmod & 4 else None, (m >> 12) & 3 if acmod == 2 else None), i
        for p, sfx in enumerate(("", "2") if acmod == 0 else ("",)):
            assert F["dialnorm" + sfx] == m & 31 and F["langcod%se" % sfx] == 0 and F["audprodi%se" % sfx] == 0, i
            assert (F["compr%se" % sfx], F.get("compr" + sfx)) == (c["compr"][p] >> 8, c["compr"][p] & 0xff if c["compr"][p] >> 8 else None), i
        assert (F["timecod1e"], F["timecod2e"], F["addbsie"]) == (0, 0, 0), i
        cpl = c["cplw"] & 1
        ncb = 3 + c["endf"] - c["begf"]
        for b, B in enumerate(fr.blocks):
            G = B.fields
            assert [G["blksw%d" % ch] for ch in range(nfbw)] == [(c["bsw"][b] >> ch) & 1 for ch in range(nfbw)], (i, b)
            assert all(G["dithflag%d" % ch] == 1 for ch in range(nfbw)), (i, b)
            for p, sfx in enumerate(("", "2") if acmod == 0 else ("",)):
                w = c["dyn"][2 * b + p]
                assert (G["dynrng%se" % sfx], G.get("dynrng" + sfx)) == (w >> 8, w & 0xff if w >> 8 else None), (i, b)
            assert G["cplstre"] == (b == 0) and B.cplinu == cpl, (i, b)
            if cpl:
                assert (B.cplbegf, B.cplendf, B.ncplbnd, B.chincpl[:nfbw]) == (c["begf"], c["endf"], ncb, [1] * nfbw), (i, b)
                for ch in range(nfbw):
                    assert G["cplcoe%d" % ch] == (b == 0), (i, b)
                    if b == 0:
                        assert G["mstrcplco%d" % ch] == (c["cplw"] >> (8 + 2 * ch)) & 3, i
                        co = bytes.fromhex(c["co"])[16 * ch:16 * ch + ncb]
                        assert [G["cplcoexp%d_%d" % (ch, k)] << 4 | G["cplcomant%d_%d" % (ch, k)] for k in range(ncb)] == list(co), (i, ch)
                assert B.expstr[AS.CPL] == c["cstrat"][b] and G["cplleake"] == (b == 0), (i, b)
                if b == 0:
                    assert (G["cplfsnroffst"], G["cplfgaincod"], G["cplfleak"], G["cplsleak"], G.get("phsflginu", 0)) == (c["fsnr"], 4, 0, 0, 0), i
            if acmod == 2:
                r = c["remat"][b] if c["remat_on"] else (0x10 if b == 0 else 0)
                nrem = 4 if not cpl else 2 if c["begf"] == 0 else 3 if c["begf"] <= 2 else 4
                assert G["rematstr"] == r >> 4 and [G.get("rematflg%d" % k) for k in range(4)] == [
                    (r >> k) & 1 if r >> 4 and k < nrem else None for k in range(4)], (i, b)
            rows = list(range(nfbw)) + ([AS.LFE] if c["lfe"] else [])
            assert [B.expstr[r] for r in rows] == c["strat"][b], (i, b)
            for ch in range(nfbw):
                assert G.get("chbwcod%d" % ch) == (c["chbwcod"] if c["strat"][b][ch] and not cpl else None), (i, b, ch)
                assert G.get("gainrng%d" % ch) == (0 if c["strat"][b][ch] else None), (i, b, ch)
            assert (G["baie"], G["snroffste"], G["deltbaie"], G["skiple"]) == (b == 0, b == 0, 0, 0), (i, b)
            if b == 0:
                assert (G["sdcycod"], G["fdcycod"], G["sgaincod"], G["dbpbcod"], G["floorcod"], G["csnroffst"]) == (2, 1, 1, 2, 4, c["csnr"]), i
                assert all(v == c["fsnr"] for v in B.fsnroffst.values()) and all(v == 4 for v in B.fgaincod.values()), i
            assert not B.exp.any(), (i, b)
    assert n == len(cases) * STRATS_READ // (2 + DRAWS)
