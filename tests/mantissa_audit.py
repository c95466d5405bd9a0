"""The mantissa audit: every mantissa code of an encoded frame, read back by tests/ac3_syntax.read_mantissas, against what
the reference's quantisers (tests/quantiser_model.py) make of the coefficient the encoder says it coded there.

    audit_mantissas(rep, frames, rows, shifts, label)

frames [S][F][fb]; rows[s][f][b] maps a coded row (ac3_syntax's numbering: 0..4 the full-bandwidth channels, LFE = 5,
CPL = 6) to its 256 integer coefficients, shifts[s][f][b] the same rows to their block shift (exp_samples): frame_rows builds
both from arrays in tap layout; or rows is a function (s, f, P) -> (rows[b], shifts[b]) of the frame's parse P, for callers
whose coupling row depends on what the frame sends.  Exponents and bap are the READER's, from the bitstream; only the coefficients and shifts come
from the encoder.  Per coded bin with bap > 0 that is in contract (quantiser_model.in_contract) the code read must equal
expected_codes(c, exponent - shift, bap); the members of a block's last grouped codes that no bin claims must be 0, as the
reference leaves them (anything else is bytes that depend on what a buffer held before); a code that is no level of its
quantiser is a failure of its own.  Bins out of contract are counted and left out.  So are, counted apart, the fields that
reach into the frame's last 16 bits in a frame with acmod 2: the reference's budget leaves the rematrixing flags of block 0
uncounted (ac3_syntax.uncounted_bits), a full 2/0 frame runs that many bits past auxdatae, and crc2 is then stored over its
last mantissa bits - in the reference and in this encoder alike (the stereo bit-budget overshoot).  That is one
field, three bins at the most, of such a frame; in any other frame a field there is a failure.  Nothing else is left out.
No GPU import."""
import numpy as np

from tests import ac3_syntax as A
from tests import quantiser_model as Q


class Report:
    """failures collected over many calls, reported together by kind: `kind | where | block, row, bin, got, want`"""

    def __init__(self):
        self.fails = []
        self.bins = []                # (stream, frame, block, row, bin) of every mismatch
        self.n = dict(frames=0, compared=0, left_out=0, under_crc2=0, unused=0, coupled=0, cpl_rows=0, remat_bands=0, short_blocks=0,
                      reduced_bw=0, dynrng=0, dynrng2=0)
        self.per_bap = np.zeros(16, np.int64)

    def fail(self, kind, where, msg):
        self.fails.append("%s | %s | %s" % (kind, where, msg))

    def summary(self, title):
        n = self.n
        coded = n["compared"] + n["left_out"]
        return ("%s: %d frames, %d bins compared, %d left out as out of contract (%.3f %%), %d under crc2 of full 2/0 frames, %d "
                "unused group members, per bap %s; "
                "%d coupled frames (%d coupling rows audited), %d flagged rematrix bands, %d short blocks, %d chbwcod below "
                "50 or cplendf below 12, %d dynrng and %d dynrng2 words" % (
                    title, n["frames"], n["compared"], n["left_out"], 100.0 * n["left_out"] / max(coded, 1), n["under_crc2"], n["unused"],
                    " ".join("%d:%d" % (b, v) for b, v in enumerate(self.per_bap) if v), n["coupled"], n["cpl_rows"],
                    n["remat_bands"], n["short_blocks"], n["reduced_bw"], n["dynrng"], n["dynrng2"]))

    def finish(self, title):
        print(self.summary(title))
        kinds = {}
        for f in self.fails:
            kinds[f.split(" | ")[0]] = kinds.get(f.split(" | ")[0], 0) + 1
        assert not self.fails, "%d failures %r, the first 25:\n%s" % (len(self.fails), kinds, "\n".join(self.fails[:25]))


def frame_rows(mdct, shift, nfchans, lfeon, cpl=None):
    """One frame's rows and shifts from arrays in tap layout - mdct [6][K][256], shift [6][K], coded channel k at index k,
    the LFE behind the full-bandwidth channels - and, for a coupled frame, cpl = (coupling rows [6][256], their shifts [6])."""
    ids = list(range(nfchans)) + ([A.LFE] if lfeon else [])
    rows = [{r: np.asarray(mdct[b][k], np.int64) for k, r in enumerate(ids)} for b in range(6)]
    shifts = [{r: int(shift[b][k]) for k, r in enumerate(ids)} for b in range(6)]
    if cpl is not None:
        for b in range(6):
            rows[b][A.CPL] = np.asarray(cpl[0][b], np.int64)
            shifts[b][A.CPL] = int(cpl[1][b])
    return rows, shifts


def tap_rows(t):
    """rows(s, f, P) for audit_mantissas from the `mdct` / `exp_samples` taps [S][F]... of the encode call that made the
    frames: the coded rows as the taps show them, the coupling row of a coupled frame from tests/coupling_model.py"""
    from tests import coupling_model as C

    def rows(s, f, P):
        cpl = None
        if P.blocks[0].cplinu:
            cpl = C.coupling_rows(t["mdct"][s, f], t["exp_samples"][s, f], P.nfchans, P.blocks[0].cplbegf)
        return frame_rows(t["mdct"][s, f], t["exp_samples"][s, f], P.nfchans, P.lfeon, cpl)
    return rows


def audit_mantissas(rep, frames, rows, shifts, label, parsed=None):
    """see the module docstring; parsed[s][f], when given, receives each frame's parse (for the caller's own checks)"""
    S, nfr = frames.shape[:2]
    for s in range(S):
        for f in range(nfr):
            where = "%s stream %d frame %d" % (label, s, f)
            rep.n["frames"] += 1
            try:
                P = A.parse_frame(frames[s, f])
                mant = A.read_mantissas(frames[s, f], P)
            except A.SyntaxError_ as e:
                rep.fail("syntax", where, str(e))
                continue
            if parsed is not None:
                parsed[s][f] = P
            rep.n["coupled"] += P.blocks[0].cplinu
            rep.n["reduced_bw"] += int(P.blocks[0].cplinu and P.blocks[0].cplendf < 12)
            frows, fshifts = rows(s, f, P) if callable(rows) else (rows[s][f], shifts[s][f])
            crc2 = 8 * P.frame_bytes - 16
            under = 0
            for b, (B, M) in enumerate(zip(P.blocks, mant)):
                fl = B.fields
                rep.n["short_blocks"] += sum(fl["blksw%d" % ch] for ch in range(P.nfchans))
                rep.n["remat_bands"] += sum(v for k, v in fl.items() if k.startswith("rematflg"))
                rep.n["reduced_bw"] += sum(1 for k, v in fl.items() if k.startswith("chbwcod") and v < 50)
                rep.n["dynrng"] += fl["dynrnge"]
                rep.n["dynrng2"] += fl.get("dynrng2e", 0)
                for r, (lo, hi) in B.rng.items():
                    if r not in frows[b]:
                        rep.fail("rows", where, "block %d: row %d is coded over [%d, %d) and was not given" % (b, r, lo, hi))
                        continue
                    bap = B.bap[r, lo:hi].astype(np.int64)
                    c = np.asarray(frows[b][r], np.int64)[lo:hi]
                    e = B.exp[r, lo:hi].astype(np.int64) - int(fshifts[b][r])
                    got, bad = M.codes[r, lo:hi], M.bad[r, lo:hi]
                    for k in np.nonzero(bad & (M.pos[r, lo:hi] + M.width[r, lo:hi] <= crc2))[0]:
                        rep.fail("range", where, "block %d, row %d, bin %d, bap %d: code %d is no level" % (b, r, lo + k, bap[k], got[k]))
                    want = Q.expected_codes(c, e, bap)
                    lost = (bap > 0) & (M.pos[r, lo:hi] + M.width[r, lo:hi] > crc2)
                    under += int(lost.sum())
                    coded = (bap > 0) & ~bad & ~lost
                    out = coded & (want == -2)
                    cmp = coded & ~out
                    rep.n["left_out"] += int(out.sum())
                    rep.n["compared"] += int(cmp.sum())
                    rep.n["cpl_rows"] += int(r == A.CPL)
                    rep.per_bap += np.bincount(bap[cmp], minlength=16)
                    for k in np.nonzero(cmp & (got != want))[0]:
                        rep.bins.append((s, f, b, r, lo + int(k)))
                        rep.fail("mantissa", where, "block %d, row %d, bin %d, got %d, want %d (bap %d, c %d, e %d)" % (
                            b, r, lo + k, got[k], want[k], bap[k], c[k], e[k]))
                for cls, members in M.unused.items():
                    if members and (M.pos + M.width)[B.bap == cls].max() > crc2:
                        continue
                    rep.n["unused"] += len(members)
                    if any(members):
                        rep.fail("unused", where, "block %d, bap %d: the last group's unclaimed members are %r, not 0" % (b, cls, members))
            rep.n["under_crc2"] += under
            if under > (3 if A.uncounted_bits(P) else 0):
                rep.fail("crc2", where, "%d bins have their field in the frame's last 16 bits (acmod %d)" % (under, P.acmod))
