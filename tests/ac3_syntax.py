"""A plain AC-3 frame reader and bit counter (Python integers + numpy), written from the A/52 syntax (§5.3 syncinfo / bsi /
audblk) and the parametric bit allocation (§7.2), independently of the kernels and of the C oracles.

    fr = parse_frame(bytes)        every field with its bit position, exponents and bap per block and row, the bit position
                                   at the end of each block, mantissa bits per block
    spent_bits(fr, g)              bits the frame would spend with every channel at 16 csnroffst + fsnroffst = g: the parsed
                                   side information plus the mantissa bits recounted (lazily, memoised per frame)

Rows: 0..4 the full-bandwidth channels, LFE = 5, CPL = 6.  The allocation tables come from the pinned fixture
tests/golden/ac3tab.npz (the reference's ENC/ac3tab.h, frozen entry by entry).  One thing below is not in A/52: the
half-sample-rate streams (bsid 9 / 10) follow liba52 (decays shifted right, hearing threshold indexed by band >> 1).
parse_frame does not decode mantissa values: it only counts their bits, grouped codes (bap 1, 2: three to a code, bap 4:
two) shared over the channels of a block in coding order.

    read_mantissas(bytes, fr)      the mantissa codes of every block, bin by bin (A/52 7.3), and the unclaimed members of each
                                   block's last groups; tests/mantissa_audit.py compares them with a quantiser model
"""
import os

import numpy as np

LFE, CPL = 5, 6
NFCHANS = (2, 1, 2, 3, 3, 4, 4, 5)
KBPS = (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 448, 512, 576, 640)
MANT_BITS = (0, 0, 0, 3, 0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16)     # bap 1, 2, 4 are grouped: counted apart
TAIL_BITS = 18                                                        # auxdatae, crcrsv, crc2

_T = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ac3tab.npz"))
BNDSZ = [int(v) for v in _T["bndsz"]]
BNDTAB = [sum(BNDSZ[:k]) for k in range(50)]
MASKTAB = [k for k in range(50) for _ in range(BNDSZ[k])]
MASKTAB += [49] * (256 - len(MASKTAB))
LATAB = [int(v) for v in _T["latab"]]
HTH = [[int(v) for v in row] for row in _T["hth"]]                    # [band][fscod]
BAPTAB = np.array(_T["baptab"], np.int64)
SLOWDEC = [int(v) for v in _T["sdecaytab"]]
FASTDEC = [int(v) for v in _T["fdecaytab"]]
SLOWGAIN = [int(v) for v in _T["sgaintab"]]
DBPBTAB = [int(v) for v in _T["dbkneetab"]]
FLOORTAB = [int(np.int16(v)) for v in _T["floortab"]]                 # the last entry is -2048
FASTGAIN = [int(v) for v in _T["fgaintab"]]
assert BNDTAB[49] + BNDSZ[49] == 253 and MASKTAB[252] == 49 and len(LATAB) >= 256 and FLOORTAB[7] == -2048


class SyntaxError_(Exception):
    """the frame is not a decodable AC-3 frame (or runs past its end)"""


class Bits:
    def __init__(self, data):
        self.data = bytes(bytearray(data))
        self.n = 8 * len(self.data)
        self.big = int.from_bytes(self.data, "big")
        self.pos = 0

    def get(self, n):
        if self.pos + n > self.n:
            raise SyntaxError_("read past the end of the frame at bit %d" % self.pos)
        v = (self.big >> (self.n - self.pos - n)) & ((1 << n) - 1) if n else 0
        self.pos += n
        return v


def frame_bytes(fscod, frmsizecod):
    rate = KBPS[frmsizecod >> 1]
    if fscod == 0:
        return 4 * rate
    if fscod == 1:
        return 2 * (320 * rate // 147 + (frmsizecod & 1))
    return 6 * rate


class Block:
    """one audio block: fields (name -> value) and their bit positions, exponents / bap [7][256], which rows carry
    mantissas and over which bins"""

    def __init__(self):
        self.fields, self.pos = {}, {}
        self.exp = np.zeros((7, 256), np.uint8)
        self.bap = np.zeros((7, 256), np.uint8)
        self.rng = {}                 # row -> (start, end) of the bins whose mantissas the block carries
        self.expstr = {}              # row -> exponent strategy code (0 = reuse)
        self.side_bits = 0            # everything of the block that is not a mantissa
        self.mant_bits = 0
        self.start = self.end = 0
        self.alloc = {}               # row -> (psd per bin, mask per band before the SNR offset, floor)


class Frame:
    def __init__(self):
        self.fields, self.pos = {}, {}
        self.blocks = []
        self.header_bits = 0          # syncinfo + bsi
        self._spent = {}

    @property
    def side_bits(self):
        return self.header_bits + sum(b.side_bits for b in self.blocks)

    @property
    def mant_bits(self):
        return [b.mant_bits for b in self.blocks]

    @property
    def block_end(self):
        return [b.end for b in self.blocks]

    def rows(self):
        """the coded rows: full-bandwidth channels, then the LFE"""
        return list(range(self.nfchans)) + ([LFE] if self.lfeon else [])


# ---------------------------------------------------------------------------------------------------------------------
# §7.2.2 parametric bit allocation

def _logadd(a, b):
    c = a - b
    adr = min(abs(c) >> 1, 255)
    return a + LATAB[adr] if c >= 0 else b + LATAB[adr]


def _calc_lowcomp(a, b0, b1, b):
    if b < 7:
        if b0 + 256 == b1:
            a = 384
        elif b0 > b1:
            a = max(0, a - 64)
    elif b < 20:
        if b0 + 256 == b1:
            a = 320
        elif b0 > b1:
            a = max(0, a - 64)
    else:
        a = max(0, a - 128)
    return a


def masking_curve(exps, start, end, fgain, p, fscod, halfrate, fastleak=0, slowleak=0, delta=None):
    """§7.2.2.1 - 7.2.2.6: exponents -> (psd per bin, mask per band, before the SNR offset is taken off).
    p = (sdecay, fdecay, sgain, dbknee, floor); delta = list of (offset, length, code) segments or None."""
    sdecay, fdecay, sgain, dbknee, _ = p
    psd = [0] * 256
    for b in range(start, end):
        psd[b] = 3072 - (int(exps[b]) << 7)
    bndpsd = [0] * 51
    j, k = start, MASKTAB[start]
    while True:
        lastbin = min(BNDTAB[k] + BNDSZ[k], end)
        v = psd[j]
        j += 1
        while j < lastbin:
            v = _logadd(v, psd[j])
            j += 1
        bndpsd[k] = v
        k += 1
        if not end > lastbin:
            break
    bndstrt, bndend = MASKTAB[start], MASKTAB[end - 1] + 1
    excite = [0] * 50
    if bndstrt == 0:
        lowcomp = _calc_lowcomp(0, bndpsd[0], bndpsd[1], 0)
        excite[0] = bndpsd[0] - fgain - lowcomp
        lowcomp = _calc_lowcomp(lowcomp, bndpsd[1], bndpsd[2], 1)
        excite[1] = bndpsd[1] - fgain - lowcomp
        begin = 7
        for b in range(2, 7):
            if bndend != 7 or b != 6:
                lowcomp = _calc_lowcomp(lowcomp, bndpsd[b], bndpsd[b + 1], b)
            fastleak = bndpsd[b] - fgain
            slowleak = bndpsd[b] - sgain
            excite[b] = fastleak - lowcomp
            if (bndend != 7 or b != 6) and bndpsd[b] <= bndpsd[b + 1]:
                begin = b + 1
                break
        for b in range(begin, min(bndend, 22)):
            if bndend != 7 or b != 6:
                lowcomp = _calc_lowcomp(lowcomp, bndpsd[b], bndpsd[b + 1], b)
            fastleak = max(fastleak - fdecay, bndpsd[b] - fgain)
            slowleak = max(slowleak - sdecay, bndpsd[b] - sgain)
            excite[b] = max(fastleak - lowcomp, slowleak)
        begin = 22
    else:
        begin = bndstrt
    for b in range(begin, bndend):
        fastleak = max(fastleak - fdecay, bndpsd[b] - fgain)
        slowleak = max(slowleak - sdecay, bndpsd[b] - sgain)
        excite[b] = max(fastleak, slowleak)
    mask = [0] * 50
    for b in range(bndstrt, bndend):
        e = excite[b]
        if bndpsd[b] < dbknee:
            e += (dbknee - bndpsd[b]) >> 2
        mask[b] = max(e, HTH[b >> halfrate][fscod])
    if delta is not None:
        band = 0
        for off, ln, code in delta:
            band += off
            d = (code - 3) << 7 if code >= 4 else (code - 4) << 7
            for _ in range(ln):
                if band < 50:
                    mask[band] += d
                band += 1
    return psd, mask


def bap_of(psd, mask, start, end, snroffset, floor):
    """§7.2.2.7: the offset-dependent tail -> bap over [start, end) (numpy arrays in, uint8 [end - start] out)"""
    m = np.maximum(mask - snroffset - floor, 0)
    m = (m & 0x1fe0) + floor
    adr = np.clip((psd[start:end] - m[_BAND_OF_BIN[start:end]]) >> 5, 0, 63)
    return BAPTAB[adr].astype(np.uint8)


_BAND_OF_BIN = np.array(MASKTAB, np.int64)
_BITS = np.array(MANT_BITS, np.int64)


def count_mantissa_bits(baps):
    """mantissa bits of one block from the bap of all its coded bins (any order: a block's grouped codes are shared over
    its channels, so only the totals matter)"""
    h = np.bincount(np.asarray(baps, np.int64).ravel(), minlength=16)
    return int((h * _BITS).sum()) + 5 * (-(-int(h[1]) // 3)) + 7 * (-(-int(h[2]) // 3)) + 7 * (-(-int(h[4]) // 2))


# ---------------------------------------------------------------------------------------------------------------------
# §5.3 the syntax

def _exponents(br, strat, absexp, ngrps, out, first):
    """§7.1.3: `ngrps` 7-bit groups of three differentials after `absexp`, each value held for 1 / 2 / 4 bins from `first`"""
    rep = 1 << (strat - 1)
    e = absexp
    k = first
    for _ in range(ngrps):
        g = br.get(7)
        if g >= 125:
            raise SyntaxError_("exponent group %d" % g)
        for d in (g // 25, (g % 25) // 5, g % 5):
            e += d - 2
            if e < 0 or e > 24:
                raise SyntaxError_("exponent %d out of range" % e)
            for _ in range(rep):
                if k < 256:
                    out[k] = e
                k += 1


def chan_ngrps(endmant, strat):
    """§5.4.3 nchgrps of a channel ending at `endmant` (the LFE: nlfegrps = 2, which is this at 7 with D15)"""
    gs = 3 << (strat - 1)
    return (endmant + gs - 4) // gs


def cpl_ngrps(cplstrtmant, cplendmant, strat):
    """§5.4.3 ncplgrps"""
    return (cplendmant - cplstrtmant) // (3 << (strat - 1))


def parse_frame(data, check_size=True, nblocks=6):
    br = Bits(data)
    fr = Frame()
    fr.data = br.data

    def field(obj, name, n):
        obj.pos[name] = br.pos
        obj.fields[name] = v = br.get(n)
        return v

    # syncinfo
    if field(fr, "syncword", 16) != 0x0b77:
        raise SyntaxError_("no syncword")
    field(fr, "crc1", 16)
    fscod = field(fr, "fscod", 2)
    frmsizecod = field(fr, "frmsizecod", 6)
    if fscod == 3 or frmsizecod >= 38:
        raise SyntaxError_("fscod / frmsizecod")
    fr.frame_bytes = frame_bytes(fscod, frmsizecod)
    if check_size and len(br.data) < fr.frame_bytes:
        raise SyntaxError_("%d bytes given, the frame has %d" % (len(br.data), fr.frame_bytes))
    # bsi
    bsid = field(fr, "bsid", 5)
    if bsid > 10:
        raise SyntaxError_("bsid %d" % bsid)
    halfrate = max(0, bsid - 8)
    field(fr, "bsmod", 3)
    acmod = field(fr, "acmod", 3)
    if (acmod & 1) and acmod != 1:
        field(fr, "cmixlev", 2)
    if acmod & 4:
        field(fr, "surmixlev", 2)
    if acmod == 2:
        field(fr, "dsurmod", 2)
    lfeon = field(fr, "lfeon", 1)
    for sfx in ("", "2") if acmod == 0 else ("",):
        field(fr, "dialnorm" + sfx, 5)
        if field(fr, "compr%se" % sfx, 1):
            field(fr, "compr" + sfx, 8)
        if field(fr, "langcod%se" % sfx, 1):
            field(fr, "langcod" + sfx, 8)
        if field(fr, "audprodi%se" % sfx, 1):
            field(fr, "mixlevel" + sfx, 5)
            field(fr, "roomtyp" + sfx, 2)
    field(fr, "copyrightb", 1)
    field(fr, "origbs", 1)
    if field(fr, "timecod1e", 1):
        field(fr, "timecod1", 14)
    if field(fr, "timecod2e", 1):
        field(fr, "timecod2", 14)
    if field(fr, "addbsie", 1):
        n = field(fr, "addbsil", 6)
        fr.pos["addbsi"] = br.pos
        fr.fields["addbsi"] = br.get(8 * (n + 1))
    fr.header_bits = br.pos
    nf = NFCHANS[acmod]
    fr.fscod, fr.bsid, fr.halfrate, fr.acmod, fr.lfeon, fr.nfchans = fscod, bsid, halfrate, acmod, lfeon, nf

    # state that lives from block to block
    cplinu, chincpl, phsflginu, cplbegf, cplendf, ncplbnd = 0, [0] * 5, 0, 0, 0, 0
    cplstrtmant = cplendmant = 0
    endmant = [0] * 5
    exps = np.zeros((7, 256), np.uint8)
    have = [False] * 7
    ba = None                       # (sdcycod, fdcycod, sgaincod, dbpbcod, floorcod)
    csnr = None
    fsnr, fgain = [0] * 7, [0] * 7
    cplfleak = cplsleak = 0
    deltbae = [2] * 7
    delta = [None] * 7

    for blk in range(nblocks):
        B = Block()
        B.start = br.pos
        f = lambda name, n: field(B, name, n)
        for ch in range(nf):
            f("blksw%d" % ch, 1)
        for ch in range(nf):
            f("dithflag%d" % ch, 1)
        for sfx in ("", "2") if acmod == 0 else ("",):
            if f("dynrng%se" % sfx, 1):
                f("dynrng" + sfx, 8)
        # coupling strategy
        if f("cplstre", 1):
            cplinu = f("cplinu", 1)
            chincpl = [0] * 5
            if cplinu:
                for ch in range(nf):
                    chincpl[ch] = f("chincpl%d" % ch, 1)
                phsflginu = f("phsflginu", 1) if acmod == 2 else 0
                cplbegf = f("cplbegf", 4)
                cplendf = f("cplendf", 4)
                nsub = 3 + cplendf - cplbegf
                if nsub < 1:
                    raise SyntaxError_("cplendf + 3 <= cplbegf")
                ncplbnd = nsub
                for sb in range(1, nsub):
                    ncplbnd -= f("cplbndstrc%d" % sb, 1)
                cplstrtmant, cplendmant = 37 + 12 * cplbegf, 73 + 12 * cplendf
        elif blk == 0:
            raise SyntaxError_("block 0 without a coupling strategy")
        # coupling coordinates
        if cplinu:
            anyco = 0
            for ch in range(nf):
                if chincpl[ch] and f("cplcoe%d" % ch, 1):
                    anyco = 1
                    f("mstrcplco%d" % ch, 2)
                    for bnd in range(ncplbnd):
                        f("cplcoexp%d_%d" % (ch, bnd), 4)
                        f("cplcomant%d_%d" % (ch, bnd), 4)
            if acmod == 2 and phsflginu and anyco:
                for bnd in range(ncplbnd):
                    f("phsflg%d" % bnd, 1)
        # rematrixing
        if acmod == 2:
            if f("rematstr", 1):
                nrem = 4 if (not cplinu or cplbegf > 2) else 3 if cplbegf > 0 else 2
                for bnd in range(nrem):
                    f("rematflg%d" % bnd, 1)
            elif blk == 0:
                raise SyntaxError_("block 0 without rematrixing flags")
        # exponent strategies
        strat = [0] * 7
        if cplinu:
            strat[CPL] = f("cplexpstr", 2)
        for ch in range(nf):
            strat[ch] = f("chexpstr%d" % ch, 2)
        if lfeon:
            strat[LFE] = f("lfeexpstr", 1)
        for ch in range(nf):
            if strat[ch]:
                if cplinu and chincpl[ch]:
                    endmant[ch] = cplstrtmant
                else:
                    c = f("chbwcod%d" % ch, 6)
                    if c > 60:
                        raise SyntaxError_("chbwcod %d" % c)
                    endmant[ch] = 73 + 3 * c
        # exponents
        if cplinu and strat[CPL]:
            ngrps = cpl_ngrps(cplstrtmant, cplendmant, strat[CPL])
            _exponents(br, strat[CPL], f("cplabsexp", 4) << 1, ngrps, exps[CPL], cplstrtmant)
            have[CPL] = True
        for ch in range(nf):
            if strat[ch]:
                exps[ch, 0] = f("exps%d_0" % ch, 4)
                _exponents(br, strat[ch], int(exps[ch, 0]), chan_ngrps(endmant[ch], strat[ch]), exps[ch], 1)
                f("gainrng%d" % ch, 2)
                have[ch] = True
        if lfeon and strat[LFE]:
            exps[LFE, 0] = f("lfeexps0", 4)
            _exponents(br, 1, int(exps[LFE, 0]), 2, exps[LFE], 1)
            have[LFE] = True
        # bit-allocation parameters
        if f("baie", 1):
            ba = (f("sdcycod", 2), f("fdcycod", 2), f("sgaincod", 2), f("dbpbcod", 2), f("floorcod", 3))
        elif blk == 0:
            raise SyntaxError_("block 0 without bit-allocation parameters")
        if f("snroffste", 1):
            csnr = f("csnroffst", 6)
            if cplinu:
                fsnr[CPL], fgain[CPL] = f("cplfsnroffst", 4), f("cplfgaincod", 3)
            for ch in range(nf):
                fsnr[ch], fgain[ch] = f("fsnroffst%d" % ch, 4), f("fgaincod%d" % ch, 3)
            if lfeon:
                fsnr[LFE], fgain[LFE] = f("lfefsnroffst", 4), f("lfefgaincod", 3)
        elif blk == 0:
            raise SyntaxError_("block 0 without SNR offsets")
        if cplinu and f("cplleake", 1):
            cplfleak, cplsleak = f("cplfleak", 3), f("cplsleak", 3)
        if f("deltbaie", 1):
            rows = ([CPL] if cplinu else []) + list(range(nf))
            for r in rows:
                deltbae[r] = f("deltbae%d" % r, 2)
                if deltbae[r] == 3:
                    raise SyntaxError_("reserved deltbae")
            for r in rows:
                if deltbae[r] == 1:
                    n = f("deltnseg%d" % r, 3)
                    delta[r] = [(f("deltoffst%d_%d" % (r, s), 5), f("deltlen%d_%d" % (r, s), 4), f("deltba%d_%d" % (r, s), 3))
                                for s in range(n + 1)]
        if f("skiple", 1):
            n = f("skipl", 9)
            B.pos["skipfld"] = br.pos
            if br.pos + 8 * n > br.n:
                raise SyntaxError_("skip field past the end of the frame")
            br.pos += 8 * n
        B.side_bits = br.pos - B.start

        # the allocation of every row that carries mantissas in this block
        p = (SLOWDEC[ba[0]] >> halfrate, FASTDEC[ba[1]] >> halfrate, SLOWGAIN[ba[2]], DBPBTAB[ba[3]], FLOORTAB[ba[4]])
        rows = []
        for ch in range(nf):
            rows.append((ch, 0, endmant[ch]))
            if cplinu and chincpl[ch] and not any(r[0] == CPL for r in rows):
                rows.append((CPL, cplstrtmant, cplendmant))
        if lfeon:
            rows.append((LFE, 0, 7))
        zero = csnr == 0 and all(fsnr[r] == 0 for r, _, _ in rows)      # §5.4.3.37-40: all offsets 0 -> every bap is 0
        for r, s, e in rows:
            if not have[r]:
                raise SyntaxError_("row %d reuses exponents nobody sent" % r)
            if r == CPL:
                psd, mask = masking_curve(exps[r], s, e, FASTGAIN[fgain[r]], p, fscod, halfrate,
                                          (cplfleak << 8) + 768, (cplsleak << 8) + 768, delta[r] if deltbae[r] < 2 else None)
            else:
                psd, mask = masking_curve(exps[r], s, e, FASTGAIN[fgain[r]], p, fscod, halfrate,
                                          delta=delta[r] if deltbae[r] < 2 else None)
            psd, mask = np.array(psd, np.int64), np.array(mask, np.int64)
            B.alloc[r] = (psd, mask, p[4])
            B.rng[r] = (s, e)
            B.exp[r, s:e] = exps[r, s:e]
            if not zero:
                B.bap[r, s:e] = bap_of(psd, mask, s, e, (((csnr - 15) << 4) + fsnr[r]) << 2, p[4])
        B.expstr = {r: strat[r] for r, _, _ in rows}
        B.csnroffst, B.fsnroffst, B.fgaincod = csnr, {r: fsnr[r] for r, _, _ in rows}, {r: fgain[r] for r, _, _ in rows}
        B.cplinu, B.chincpl, B.cplbegf, B.cplendf, B.ncplbnd = cplinu, list(chincpl), cplbegf, cplendf, ncplbnd
        B.mant_bits = count_mantissa_bits(np.concatenate([B.bap[r, s:e] for r, s, e in rows]))
        if br.pos + B.mant_bits > br.n:
            raise SyntaxError_("block %d's mantissas run past the end of the frame" % blk)
        br.pos += B.mant_bits
        B.end = br.pos
        fr.blocks.append(B)
    return fr


# ---------------------------------------------------------------------------------------------------------------------
# the mantissas

SYM_LEVELS = {1: 3, 2: 5, 3: 7, 4: 11, 5: 15}                        # bap -> levels of the symmetric quantisers
GROUPS = {1: (3, 3, 5), 2: (5, 3, 7), 4: (11, 2, 7)}                  # bap -> (levels, members of a group, bits of its code)


class Mantissas:
    """one block's mantissa codes, rows as in Block: `codes` [7][256], -1 where bap is 0 or the bin is not coded (a
    member of a grouped code holds its own digit); `pos` [7][256] the first bit of the field that carries the bin's code
    (a group's, for each of its members); `bad` [7][256] true where the code is no level of its quantiser (a group code
    >= 27 / 125 / 121, or code 7 of bap 3, 15 of bap 5): reported, never to be compared; `unused` bap -> the digits of the
    block's last group that no bin claimed."""

    def __init__(self):
        self.codes = np.full((7, 256), -1, np.int64)
        self.pos = np.full((7, 256), -1, np.int64)
        self.width = np.zeros((7, 256), np.int64)
        self.bad = np.zeros((7, 256), bool)
        self.unused = {1: [], 2: [], 4: []}


def _fields(data, pos, width):
    """the unsigned fields of `width` bits (0..16) that start at bits `pos` of the uint8 array `data`"""
    d = np.concatenate([np.asarray(data, np.uint8), np.zeros(4, np.uint8)]).astype(np.int64)
    k = pos >> 3
    word = d[k] << 24 | d[k + 1] << 16 | d[k + 2] << 8 | d[k + 3]
    return (word >> (32 - (pos & 7) - width)) & ((1 << width) - 1)


def read_mantissas(frame, P):
    """The mantissa codes of every block of `frame` (its bytes), whose parse P = parse_frame(frame) is.  A/52 5.4.3.61 and
    7.3: from the end of a block's side information the rows follow in the order of Block.rng - channel order, the
    coupling row after the first coupled channel, the LFE last - each with the codes of its coded bins in bin order.  bap 3
    and bap 5 and up are fields of their own; bap 1, 2 and 4 are grouped, three, three and two to a code (5, 7, 7 bits:
    g // 9, (g // 3) % 3, g % 3; g // 25, (g // 5) % 5, g % 5; g // 11, g % 11), the code standing where its first member
    would and ONE pending group per bap shared by all rows of the block.  -> a list of Mantissas, one per block.  The walk
    has to end exactly at Block.end."""
    data = np.frombuffer(bytes(bytearray(frame)), np.uint8)
    out = []
    for blk, B in enumerate(P.blocks):
        M = Mantissas()
        rows = np.concatenate([np.full(hi - lo, r, np.int64) for r, (lo, hi) in B.rng.items()])
        bins = np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in B.rng.values()])
        bap = B.bap[rows, bins].astype(np.int64)
        width = _BITS[bap].copy()
        member = {}
        for b, (levels, per, bits) in GROUPS.items():
            idx = np.nonzero(bap == b)[0]
            member[b] = idx
            width[idx[::per]] = bits
        pos = B.start + B.side_bits + np.cumsum(width) - width
        end = B.start + B.side_bits + int(width.sum())
        if end != B.end or end > 8 * data.size:
            raise SyntaxError_("block %d's mantissas end at bit %d, the block at %d" % (blk, end, B.end))
        raw = _fields(data, pos, width)
        code, bad = raw.copy(), np.zeros(raw.size, bool)
        for b, levels in SYM_LEVELS.items():
            if b not in GROUPS:
                bad |= (bap == b) & (raw >= levels)
        for b, (levels, per, bits) in GROUPS.items():
            idx = member[b]
            k = np.arange(idx.size)
            first = idx[k - k % per]                                      # the bin that opens this member's group
            g = raw[first]
            digit = g // levels ** (per - 1 - k % per)
            code[idx] = np.where(k % per == 0, digit, digit % levels)
            bad[idx] = g >= levels ** per
            pos[idx] = pos[first]
            width[idx] = bits
            if idx.size % per:
                g = int(raw[idx[idx.size - idx.size % per]])
                M.unused[b] = [g // levels ** (per - 1 - j) % levels for j in range(idx.size % per, per)]
        coded = bap > 0
        M.codes[rows[coded], bins[coded]] = code[coded]
        M.pos[rows[coded], bins[coded]] = pos[coded]
        M.width[rows[coded], bins[coded]] = width[coded]
        M.bad[rows[coded], bins[coded]] = bad[coded]
        out.append(M)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the bit budget

def mantissa_bits_at(fr, g):
    """mantissa bits per block if every row's offsets were csnroffst = g >> 4, fsnroffst = g & 15: §7.2.2.7 recounted with
    everything before it held.  (The rule that offsets which are ALL zero mean bap 0 everywhere is a decoder's reading of a
    frame that carries them; an encoder's count at g = 0, the reference's included, prices the allocation the formula gives.)"""
    snroffset = (((g >> 4) - 15) << 4) + (g & 15) << 2
    out = []
    for B in fr.blocks:
        baps = [bap_of(B.alloc[r][0], B.alloc[r][1], s, e, snroffset, B.alloc[r][2]) for r, (s, e) in B.rng.items()]
        out.append(count_mantissa_bits(np.concatenate(baps)))
    return out


def spent_bits(fr, g):
    """side information as parsed + mantissa bits at offset g, without the 18 bits of auxdatae, crcrsv and crc2"""
    if g not in fr._spent:
        fr._spent[g] = fr.side_bits + sum(mantissa_bits_at(fr, g))
    return fr._spent[g]


class SpareCurve:
    """spare bits of a frame as a lazy 1024-entry curve, in the form the reference's search reads it (search_allocation):
    8 frame_bytes - 18 - spent_bits(g) + c, c = the bits that rule leaves uncounted"""

    def __init__(self, fr, uncounted=0):
        self.fr, self.c = fr, uncounted

    def __getitem__(self, g):
        return 8 * self.fr.frame_bytes - TAIL_BITS - spent_bits(self.fr, int(g)) + self.c

    def __len__(self):
        return 1024


def uncounted_bits(fr):
    """What the reference's budget (search_allocation) leaves out of a frame's count: it prices rematstr as one bit in every
    block of a 2/0 frame and never the flags, which only block 0 sends: 4 without coupling, 2 / 3 / 4 by the coupling start
    with it.  Nothing else, in any layout."""
    if fr.acmod != 2:
        return 0
    return sum(1 for k in fr.blocks[0].fields if k.startswith("rematflg"))


def tail_is_zero(fr):
    """every bit between the end of block 5 and auxdatae is zero (nothing lies between them when block 5 ends at or, in the
    2/0 overshoot, behind that point: the bound on the end is the caller's)"""
    end = fr.blocks[5].end
    last = 8 * fr.frame_bytes - TAIL_BITS
    if end >= last:
        return True
    br = Bits(fr.data[:fr.frame_bytes])
    br.pos = end
    return br.get(last - end) == 0
