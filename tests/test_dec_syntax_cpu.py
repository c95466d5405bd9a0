"""CPU: the decoder's side-information syntax of csrc/dec_syntax.h - the field lists of a52_frame and of an audio block that both
front ends read through - against tests/ac3_syntax.parse_frame, the independent reader.  The lists run in
tests/dec_syntax_c/main.cpp (see there for what it prints), a program of its own built with the host compiler under
-fsanitize=address,undefined, over a byte-buffer reader and a plain-struct state; nothing here comes from the engine.

How a printed value maps to the reader's names (B = a parse_frame block, F = its fields; a state value is compared where the
frame has sent it, last sender wins, as the decoder keeps it):
    err, end            0, B.start + B.side_bits                   blksw, dith       F["blksw<ch>"], F["dithflag<ch>"] at bit ch
    chincpl             B.chincpl at bit ch where B.cplinu, else 0   phs               F["phsflginu"]
    cplstrt, cplend     B.rng[CPL]                                   ncplbnd           B.ncplbnd
    strc                F["cplbndstrc<sb>"] at bit sb - 1            remat             F["rematflg<bnd>"] at bit bnd
    exps                per row with B.expstr != 0, in bitstream order (coupling, channels, LFE): the strategy, chan_ngrps /
                        cpl_ngrps of its range, F["exps<ch>_0"] / F["lfeexps0"] / F["cplabsexp"] << 1, B.pos[that field] + 4
    endm                B.rng[ch][1]                                 bai               sdcycod << 9 | fdcycod << 7 | sgaincod << 5 | dbpbcod << 3 | floorcod
    csnr, cbai          B.csnroffst, B.fsnroffst[row] << 3 | B.fgaincod[row] (rows 0..4, LFE, CPL = slots 0..6)
    fleak, sleak        9 - F["cplfleak"], 9 - F["cplsleak"] (liba52 keeps them so)
    deltbae             F["deltbae<row>"], slot 5 = row CPL; 2 in every slot at the frame's start
    deltba              a row per slot with deltbae 1: F["deltoffst / deltlen / deltba<row>_<seg>"] laid out as parse_deltba does
    dyn                 F["dynrng"], F["dynrng2"] where sent         reuse0            0 (parse_frame refuses such a block 0)
    co, flips           F["cplcoexp / cplcomant / mstrcplco"] (master = 3 mstrcplco), the number of F["phsflg<bnd>"] set"""
import os
import subprocess

import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import ac3_syntax as AS

FLIPS = 24              # single-bit flips inside block 0 per frame of the damaged cases (72 frames: ~1 900 damaged frames, seconds)
ERRORS = {1: "acmod < 2 coupled", 2: "cplendf + 3 - cplbegf < 0", 3: "chbwcod > 60", 4: "deltba segment reaches band 50"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return H.build_sanitised([os.path.join(H.ROOT, "tests", "dec_syntax_c", "main.cpp")], str(tmp_path_factory.mktemp("dec_syntax") / "dec_syntax"),
                             includes=[H.CSRC])


def _run(exe, tmp, lines):
    """the program on the given input lines -> per frame (hdr dict, [block dicts]); exit status 0 and not a word from either sanitiser"""
    path = os.path.join(str(tmp), "frames.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = []
    for line in r.stdout.splitlines():
        d = dict(tok.split("=", 1) for tok in line.split(" ")[1:] if "=" in tok) if line.startswith("hdr") else dict(tok.split("=", 1) for tok in line.split(" "))
        if line.startswith("hdr"):
            out.append((d, []))
        else:
            out[-1][1].append(d)
    assert len(out) == len(lines)
    return out


def _frames(case):
    fb = M.CASES[case]
    return np.concatenate([M.multi(case).reshape(-1, fb), M.single(case).reshape(-1, fb)])


def _ints(s):
    return [int(v) for v in s.split(",")]


def _expected_blocks(fr):
    """the program's block lines as tests/ac3_syntax.parse_frame has them (see the module's head), and the features seen"""
    nf, CPL, LFE = fr.nfchans, AS.CPL, AS.LFE
    st = dict(phs=0, strc=0, remat=0, bai=0, fleak=0, sleak=0, deltbae=[2] * 6, deltba=[[0] * 50 for _ in range(6)])
    want, seen = [], set()
    for B in fr.blocks:
        F = B.fields
        w = dict(err=0, end=B.start + B.side_bits, reuse0=0)
        w["blksw"] = sum(F["blksw%d" % ch] << ch for ch in range(nf))
        w["dith"] = sum(F["dithflag%d" % ch] << ch for ch in range(nf))
        w["dyn"] = ";".join("%d:%d" % (F["dynrng" + sfx], p) for p, sfx in enumerate(("", "2") if fr.acmod == 0 else ("",)) if F["dynrng%se" % sfx])
        if F.get("dynrng2e"):
            seen.add("dynrng2")
        w["chincpl"] = sum(c << ch for ch, c in enumerate(B.chincpl)) if B.cplinu else 0
        if B.cplinu:
            if F.get("cplinu"):
                st["phs"] = F.get("phsflginu", 0)
                st["strc"] = sum(F["cplbndstrc%d" % sb] << (sb - 1) for sb in range(1, 3 + B.cplendf - B.cplbegf))
            w.update(phs=st["phs"], cplstrt=B.rng[CPL][0], cplend=B.rng[CPL][1], ncplbnd=B.ncplbnd, strc=st["strc"])
            if st["strc"]:
                seen.add("merged bands")
        co = []
        for ch in range(nf):
            if F.get("cplcoe%d" % ch):
                co += ["%d:%d:%d:%d:%d" % (ch, b, F["cplcoexp%d_%d" % (ch, b)], F["cplcomant%d_%d" % (ch, b)], 3 * F["mstrcplco%d" % ch]) for b in range(B.ncplbnd)]
        w["co"] = ";".join(co)
        w["flips"] = sum(v for k, v in F.items() if k.startswith("phsflg") and k != "phsflginu")
        if any(k.startswith("phsflg") and k != "phsflginu" for k in F):
            seen.add("phase flags")
        if F.get("rematstr"):
            st["remat"] = sum(v << int(k[8:]) for k, v in F.items() if k.startswith("rematflg"))
        if fr.acmod == 2:
            w["remat"] = st["remat"]
        exps = []
        for r in ([CPL] if B.cplinu else []) + list(range(nf)) + ([LFE] if fr.lfeon else []):
            s = B.expstr[r]
            if not s:
                seen.add("reuse")
                continue
            if r == CPL:
                name, e0, n = "cplabsexp", F["cplabsexp"] << 1, AS.cpl_ngrps(B.rng[CPL][0], B.rng[CPL][1], s)
            elif r == LFE:
                name, e0, n = "lfeexps0", F["lfeexps0"], 2
            else:
                name, e0, n = "exps%d_0" % r, F["exps%d_0" % r], AS.chan_ngrps(B.rng[r][1], s)
            exps.append("%d:%d:%d:%d:%d" % (r, s, n, e0, B.pos[name] + 4))
        w["exps"] = ";".join(exps)
        w["endm"] = [B.rng[ch][1] for ch in range(nf)]
        if F["baie"]:
            st["bai"] = F["sdcycod"] << 9 | F["fdcycod"] << 7 | F["sgaincod"] << 5 | F["dbpbcod"] << 3 | F["floorcod"]
        w.update(bai=st["bai"], csnr=B.csnroffst, cbai={r: B.fsnroffst[r] << 3 | B.fgaincod[r] for r in B.fsnroffst})
        if F.get("cplleake"):
            st["fleak"], st["sleak"] = 9 - F["cplfleak"], 9 - F["cplsleak"]
        if B.cplinu:
            w.update(fleak=st["fleak"], sleak=st["sleak"])
        if F["deltbaie"]:
            for r in ([CPL] if B.cplinu else []) + list(range(nf)):
                slot = 5 if r == CPL else r
                st["deltbae"][slot] = F["deltbae%d" % r]
                if F["deltbae%d" % r] == 1:
                    row, band = [0] * 50, 0
                    for s in range(F["deltnseg%d" % r] + 1):
                        band += F["deltoffst%d_%d" % (r, s)]
                        ln, d = F["deltlen%d_%d" % (r, s)], F["deltba%d_%d" % (r, s)]
                        row[band:band + ln] = [d - 3 if d >= 4 else d - 4] * ln
                        band += ln
                        seen.add("deltba")
                    st["deltba"][slot] = row
        w["deltbae"] = list(st["deltbae"])
        w["deltba"] = [list(r) for r in st["deltba"]]
        if F["skiple"]:
            seen.add("skip field")
        want.append(w)
    return want, seen


def _compare(got, w, nf, what):
    for k in ("err", "end", "reuse0", "blksw", "dith", "chincpl", "bai", "csnr"):
        assert int(got[k]) == w[k], (what, k, got[k], w[k])
    for k in ("phs", "cplstrt", "cplend", "ncplbnd", "strc", "remat", "fleak", "sleak"):
        if k in w:
            assert int(got[k]) == w[k], (what, k, got[k], w[k])
    for k in ("dyn", "co", "exps"):
        assert got[k] == w[k], (what, k, got[k], w[k])
    assert int(got["flips"]) == w["flips"], (what, "flips")
    assert _ints(got["endm"])[:nf] == w["endm"], (what, "endm", got["endm"], w["endm"])
    cbai = _ints(got["cbai"])
    for r, v in w["cbai"].items():
        assert cbai[r] == v, (what, "cbai", r, cbai, w["cbai"])
    assert _ints(got["deltbae"]) == w["deltbae"], (what, "deltbae", got["deltbae"], w["deltbae"])
    rows = [[int(c, 16) - 8 for c in row] for row in got["deltba"].split(",")]
    for slot in range(6):
        if w["deltbae"][slot] == 1:
            assert rows[slot] == w["deltba"][slot], (what, "deltba", slot)


def test_undamaged_frames(exe, tmp_path):
    """the frames of multi(case) and single(case) of all thirteen cases: the header, then every block read from Block.start;
    every printed value against parse_frame (the table at the head of this module), and the features the comparison rests on"""
    lines, parses = [], []
    for case in M.CASE_LIST:
        for fr in _frames(case):
            P = AS.parse_frame(fr)
            parses.append((case, P))
            lines.append("F %d %d %s %s" % (case[1], case[0] | (16 if case[1] else 0), bytes(fr).hex(), " ".join(str(B.start) for B in P.blocks)))
    out = _run(exe, tmp_path, lines)
    seen = set()
    for i, ((case, P), (hdr, blocks)) in enumerate(zip(parses, out)):
        acmod = case[0]
        want_out = (10 if acmod == 2 and P.fields["dsurmod"] == 2 else acmod) | (16 if case[1] else 0)
        assert (int(hdr["out"]), int(hdr["at"]), int(hdr["nf"]), int(hdr["lfeon"])) == (want_out, P.header_bits, P.nfchans, case[1]), (i, hdr)
        assert len(blocks) == 6
        want, s = _expected_blocks(P)
        seen |= s
        for b in range(6):
            _compare(blocks[b], want[b], P.nfchans, (M.case_id(case), i, b))
    assert seen == {"merged bands", "phase flags", "deltba", "skip field", "dynrng2", "reuse"}, seen


def test_damaged_frames(exe, tmp_path):
    """single bits flipped inside block 0's side information of every frame of the three damaged cases (positions drawn from the
    undamaged parse, FLIPS a frame; and each of the header's three acmod bits: no flip inside block 0 makes one of these
    layouts mono or dual mono, the only frames that can take the `acmod < 2 coupled` exit): the program reads header and block 0 of each
    without a word from the sanitisers or a state value outside St's packing, every block 0 (or header) it refuses is one
    whose frame the restatement of liba52 fails in block 0 or refuses, and each of the list's four exits was taken"""
    rng = np.random.default_rng(M.DAMAGED_SEED)
    taken = set()
    for case in M.DAMAGED_CASES:
        lines, damaged = [], []
        frames = _frames(case)
        for fr in frames:
            P = AS.parse_frame(fr)
            B = P.blocks[0]
            drawn = rng.choice(np.arange(B.start, B.start + B.side_bits), FLIPS, replace=False)
            for at in np.concatenate([drawn, np.arange(P.pos["acmod"], P.pos["acmod"] + 3)]):
                bits = np.unpackbits(fr)
                bits[at] ^= 1
                damaged.append(np.packbits(bits))
                lines.append("D %d %d %s" % (case[1], case[0] | (16 if case[1] else 0), bytes(damaged[-1]).hex()))
        out = _run(exe, tmp_path, lines)
        # the restatement: one stream per damaged frame behind an undamaged one that sets the batch's layout
        batch = np.stack([frames[0]] + damaged)[:, None, :]
        status = H.orc_decode_status(batch, case[0] | (16 if case[1] else 0))[0][1:, 0]
        for i, (hdr, blocks) in enumerate(out):
            refused = int(hdr["out"]) < 0 or int(blocks[0]["err"]) != 0
            if blocks and int(blocks[0]["err"]):
                taken.add(int(blocks[0]["err"]))
            if refused:
                assert status[i] & 1, (M.case_id(case), i, hdr, blocks and blocks[0]["err"], hex(status[i]))
    assert taken >= set(ERRORS), {ERRORS[e] for e in set(ERRORS) - taken}
