"""The BSI metadata rules of include/ac3mi.h (ac3mi_bsi_info, ac3mi_set_encode_metadata_frames, ac3mi_set_encode_metadata_source)
in plain Python on top of tests/ac3_syntax.parse_frame, written from their text and independently of csrc/bsi.hip:

    pack_word / fields_of      the encoder's metadata word: dialnorm bits 0-4, bsmod 5-7, cmixlev 8-9, surmixlev 10-11,
                               dsurmod 12-13, copyrightb 14, origbs 15
    sanitise(word)             what the packers code for a raw word
    source_word(P)             the word of a parsed source frame
    followed_word(P, ...)      the word a transcode that follows its source codes for that frame
    coded_fields(word, acmod)  the BSI fields a frame coded from `word` carries under `acmod`
    info_of(P)                 every field of ac3mi_bsi_info from a parsed frame
"""
from tests import ac3_syntax as A

FIELDS = ("dialnorm", "bsmod", "cmixlev", "surmixlev", "dsurmod", "copyrightb", "origbs")
DEFAULTS = dict(dialnorm=31, bsmod=0, cmixlev=1, surmixlev=1, dsurmod=0, copyrightb=0, origbs=1)
SHIFT = dict(dialnorm=0, bsmod=5, cmixlev=8, surmixlev=10, dsurmod=12, copyrightb=14, origbs=15)
WIDTH = dict(dialnorm=5, bsmod=3, cmixlev=2, surmixlev=2, dsurmod=2, copyrightb=1, origbs=1)
PRESENT = ("compre", "langcode", "audprodie", "compr2e", "langcod2e", "audprodi2e", "timecod1e", "timecod2e", "addbsie")


def pack_word(**f):
    w = 0
    for k in FIELDS:
        v = int(f.get(k, DEFAULTS[k]))
        assert 0 <= v < (1 << WIDTH[k]), (k, v)
        w |= v << SHIFT[k]
    return w


def fields_of(word):
    return {k: (word >> SHIFT[k]) & ((1 << WIDTH[k]) - 1) for k in FIELDS}


def sanitise(word):
    """dialnorm 0 -> 31, cmixlev 3 -> 1, surmixlev 3 -> 1, dsurmod 3 -> 0; bsmod, copyrightb, origbs pass; bits 16+ dropped"""
    f = fields_of(word & 0xffff)
    if f["dialnorm"] == 0:
        f["dialnorm"] = 31
    if f["cmixlev"] == 3:
        f["cmixlev"] = 1
    if f["surmixlev"] == 3:
        f["surmixlev"] = 1
    if f["dsurmod"] == 3:
        f["dsurmod"] = 0
    return pack_word(**f)


def sends(acmod):
    """the mix-level fields an acmod sends"""
    s = set()
    if (acmod & 1) and acmod != 1:
        s.add("cmixlev")
    if acmod & 4:
        s.add("surmixlev")
    if acmod == 2:
        s.add("dsurmod")
    return s


def source_word(P):
    """a parsed source frame's metadata as an encoder word: a field its acmod does not send takes the default"""
    f = {k: P.fields.get(k, DEFAULTS[k]) for k in FIELDS}
    return sanitise(pack_word(**f))


def followed_word(P, coded_acmod, ctx_word, refused=False):
    """ac3mi_set_encode_metadata_source 1: the word of the new frame for source frame P (None or refused: the context's whole)"""
    if P is None or refused:
        return ctx_word
    src, out = fields_of(source_word(P)), fields_of(ctx_word)
    for k in ("dialnorm", "bsmod", "copyrightb", "origbs"):
        out[k] = src[k]
    for k in sends(P.acmod) & sends(coded_acmod):
        out[k] = src[k]
    return pack_word(**out)


def coded_fields(word, acmod):
    """the metadata fields of a frame coded from `word` under `acmod` (dual mono: dialnorm2 = dialnorm)"""
    f = fields_of(sanitise(word))
    out = {k: f[k] for k in ("dialnorm", "bsmod", "copyrightb", "origbs")}
    for k in sends(acmod):
        out[k] = f[k]
    if acmod == 0:
        out["dialnorm2"] = f["dialnorm"]
    return out


def info_of(P):
    """ac3mi_bsi_info of a frame ac3_syntax parsed (parse_frame(..., nblocks=0) is enough), verdict 0"""
    g = P.fields
    present = sum(1 << i for i, k in enumerate(PRESENT) if g.get(k, 0))

    def audprodi(sfx):
        return (g["mixlevel" + sfx] << 2 | g["roomtyp" + sfx]) if g.get("audprodi%se" % sfx, 0) else 0

    return dict(verdict=0, fscod=g["fscod"], frmsizecod=g["frmsizecod"], bsid=g["bsid"], bsmod=g["bsmod"], acmod=g["acmod"],
                lfeon=g["lfeon"], cmixlev=g.get("cmixlev", 0xff), surmixlev=g.get("surmixlev", 0xff), dsurmod=g.get("dsurmod", 0xff),
                dialnorm=g["dialnorm"], dialnorm2=g.get("dialnorm2", 0xff), compr=g.get("compr", 0), compr2=g.get("compr2", 0),
                langcod=g.get("langcod", 0), langcod2=g.get("langcod2", 0), audprodi=audprodi(""), audprodi2=audprodi("2"),
                copyrightb=g["copyrightb"], origbs=g["origbs"], addbsil=g.get("addbsil", 0), present=present,
                timecod1=g.get("timecod1", 0), timecod2=g.get("timecod2", 0), block0_bit=P.header_bits, word=source_word(P))


def metadata_bits(P):
    """bit positions of the metadata fields (and dialnorm2) in a parsed frame: what a change of the word may change"""
    names = FIELDS + ("dialnorm2",)
    width = dict(WIDTH, dialnorm2=5)
    return [p for k in names if k in P.pos for p in range(P.pos[k], P.pos[k] + width[k])]


def parse_head(data):
    """syncinfo + BSI of a frame or of its head alone"""
    return A.parse_frame(data, check_size=False, nblocks=0)
