"""The encoder's channel layouts (ac3mi_set_encode_layout, include/ac3mi.h) restated: channel counts, the layout a
transcode follows, the channel map that inverts the s16 converter's WAVE interleave, and a BSI reader that knows dual
mono's second-programme fields."""

NFCHANS = (2, 1, 2, 3, 3, 4, 4, 5)
# the reference's table (mode 0): channel count -> (acmod, lfeon)
REF_LAYOUT = {1: (1, 0), 2: (2, 0), 3: (3, 0), 4: (6, 0), 5: (7, 0), 6: (7, 1)}
A52_CHANNEL1, A52_CHANNEL2, A52_DOLBY, A52_LFE = 8, 9, 10, 16
_NFCH_OUT = (2, 1, 2, 3, 3, 4, 4, 5, 1, 1, 2)


def channels(acmod, lfeon):
    return NFCHANS[acmod] + lfeon


def layouts():
    """Every (acmod, lfeon)."""
    return [(a, l) for a in range(8) for l in (0, 1)]


def granted_layout(out_flags):
    """Mode 2: the layout a transcode codes for the decoder's granted output flags."""
    cfg = out_flags & 15
    acmod = cfg if cfg <= 7 else (2 if cfg == A52_DOLBY else 1)
    return acmod, 1 if out_flags & A52_LFE else 0


def wave_planes(flags):
    """WAVE slot -> liba52 output plane (the LFE is plane 0 when present) for output `flags`: the MapTab interleave."""
    cfg, lfe = flags & 15, 1 if flags & A52_LFE else 0
    o = lfe
    out = []
    lfe_done = [False]

    def put_lfe():
        if lfe and not lfe_done[0]:
            out.append(0)
            lfe_done[0] = True
    if cfg == 3:
        out += [o, o + 2, o + 1]
    elif cfg == 4:
        out += [o, o + 1]; put_lfe(); out += [o + 2]
    elif cfg == 5:
        out += [o, o + 2, o + 1]; put_lfe(); out += [o + 3]
    elif cfg == 6:
        out += [o, o + 1]; put_lfe(); out += [o + 2, o + 3]
    elif cfg == 7:
        out += [o, o + 2, o + 1]; put_lfe(); out += [o + 3, o + 4]
    else:
        out += [o + i for i in range(_NFCH_OUT[cfg])]
    put_lfe()
    return out


def follow_map(out_flags):
    """Mode 2's chmap: coded channel k (full-bandwidth channels in A/52 order, the LFE last) -> WAVE slot, such that the
    re-encoded coded channel k carries decoded coded channel k."""
    acmod, lfeon = granted_layout(out_flags)
    planes = wave_planes(out_flags)
    nf = NFCHANS[acmod]
    return [planes.index(lfeon + k if k < nf else 0) for k in range(nf + lfeon)]


class Bits:
    def __init__(self, frame):
        self.v = int.from_bytes(bytes(frame), "big")
        self.n = len(frame) * 8
        self.p = 0

    def get(self, n):
        self.p += n
        return (self.v >> (self.n - self.p)) & ((1 << n) - 1)


def bsi(frame):
    """The BSI fields this encoder writes (no optional fields besides dual mono's second programme)."""
    r = Bits(frame)
    r.get(32)
    f = dict(fscod=r.get(2), frmsizecod=r.get(6), bsid=r.get(5), bsmod=r.get(3), acmod=r.get(3))
    a = f["acmod"]
    if (a & 1) and a != 1:
        f["cmixlev"] = r.get(2)
    if a & 4:
        f["surmixlev"] = r.get(2)
    if a == 2:
        f["dsurmod"] = r.get(2)
    f["lfeon"] = r.get(1)
    f["dialnorm"] = r.get(5)
    f["compre"], f["langcode"], f["audprodie"] = r.get(1), r.get(1), r.get(1)
    if a == 0:
        f["dialnorm2"] = r.get(5)
        f["compr2e"], f["langcod2e"], f["audprodi2e"] = r.get(1), r.get(1), r.get(1)
    f["copyrightb"], f["origbs"] = r.get(1), r.get(1)
    f["timecod1e"], f["timecod2e"], f["addbsie"] = r.get(1), r.get(1), r.get(1)
    f["bsi_end"] = r.p
    return f


def decode_flags(acmod, lfeon):
    """liba52 output flags that keep every coded channel: the layout itself (dual mono: A52_CHANNEL, both programmes)."""
    return acmod | (A52_LFE if lfeon else 0)
