"""The rule of ac3mi_set_encode_dynrng_frames / ac3mi_set_encode_drc_source (include/ac3mi.h) in plain Python: which word is
in force in each block of a source frame, which blocks of the new frame send one, and the gain a decoder applies.  Frames
are read with tests/ac3_syntax.py; nothing here touches the library."""
import numpy as np

from tests import ac3_syntax as A
from tests import drc_model

COMPR_SENT = 0x100
DAMAGED = 0x13f         # d_status: bit 8 (refused / concealed) or any block's bit


def frame_words(P):
    """A parsed frame -> (raw [6][2] (dynrnge << 8 | dynrng per block and programme), compr [2] (compre << 8 | compr))"""
    raw = np.zeros((6, 2), np.int64)
    compr = np.zeros(2, np.int64)
    for p, sfx in enumerate(("", "2") if P.acmod == 0 else ("",)):
        if P.fields["compr%se" % sfx]:
            compr[p] = COMPR_SENT | P.fields["compr" + sfx]
        for b, B in enumerate(P.blocks):
            if B.fields["dynrng%se" % sfx]:
                raw[b, p] = 0x100 | B.fields["dynrng" + sfx]
    return raw, compr


def in_force(raw):
    """raw [6][2] -> codes [6][2]: e = 0 at the frame's start, a word that is sent holds to the frame's end"""
    codes = np.zeros((6, 2), np.uint8)
    for p in range(2):
        e = 0
        for b in range(6):
            if raw[b][p] & 0x100:
                e = int(raw[b][p]) & 0xff
            codes[b, p] = e
    return codes


def effective(frames, status=None, prog=-1):
    """Source frames [S][F][fb] (status [S][F], None: all clean) -> (codes [S][F][6][2] uint8, compr [S][F][2] uint16) as
    ac3mi_set_encode_drc_source 1 resolves them.  prog -1: both programmes of a dual-mono source stay where they are; 0 / 1:
    that programme of a dual-mono source becomes programme 0 and programme 1 carries nothing (a source of any other acmod has
    one programme, whatever prog says).  A damaged frame (status & 0x13f) carries nothing."""
    S, F = frames.shape[:2]
    codes = np.zeros((S, F, 6, 2), np.uint8)
    compr = np.zeros((S, F, 2), np.uint16)
    for s in range(S):
        for f in range(F):
            if status is not None and int(status[s][f]) & DAMAGED:
                continue
            P = A.parse_frame(frames[s, f])
            raw, c = frame_words(P)
            e = in_force(raw)
            if prog < 0:
                codes[s, f], compr[s, f] = e, c
            else:
                p = prog if P.acmod == 0 else 0
                codes[s, f, :, 0], compr[s, f, 0] = e[:, p], c[p]
    return codes, compr


def sends(codes):
    """codes [...][6][2] -> bool [...][6][2]: per programme, block b sends iff its code differs from block b - 1's, block 0's
    from 0"""
    c = np.asarray(codes)
    prev = np.zeros_like(c)
    prev[..., 1:, :] = c[..., :-1, :]
    return c != prev


def gain(code):
    """the gain a decoder applies under dynrng word `code` (word 0: 1.0)"""
    return drc_model.decoded_gain(code)


def frame_fields(P, nprog):
    """what a parsed output frame carries, in the arrays' terms: (sent [6][nprog] bool, word [6][nprog], compr [nprog])"""
    raw, c = frame_words(P)
    return (raw[:, :nprog] & 0x100) != 0, raw[:, :nprog] & 0xff, c[:nprog]


def check_frames(frames, codes, compr, acmod):
    """every frame [S][F][fb] codes `acmod` and carries exactly the words of sends(codes) and compr (programme 1: acmod 0 only);
    returns the number of dynrng words and compr words seen"""
    nprog = 2 if acmod == 0 else 1
    snd = sends(codes)
    nd = nc = 0
    S, F = frames.shape[:2]
    for s in range(S):
        for f in range(F):
            P = A.parse_frame(frames[s, f])
            assert P.acmod == acmod, (s, f, P.acmod)
            sent, word, c = frame_fields(P, nprog)
            assert np.array_equal(sent, snd[s, f, :, :nprog]), (s, f, sent.T, snd[s, f].T)
            assert np.array_equal(word[sent], codes[s, f, :, :nprog][sent]), (s, f)
            want_c = [int(v) & 0x1ff if int(v) & COMPR_SENT else 0 for v in compr[s, f, :nprog]]
            assert list(c) == want_c, (s, f, list(c), want_c)
            nd += int(sent.sum())
            nc += sum(1 for v in want_c if v)
    return nd, nc
