"""Batches whose frames differ in size (not collected): 44.1 kHz streams, which alternate between the two sizes of an odd and an
even frmsizecod, and batches of streams of several bit rates and sample rates, as ac3mi_frame_gather_batch builds them.  Every
frame lies at the start of a slot of the batch's largest size and carries its own size in its header; what lies between its own
end and the slot's is not the frame's - the liba52 restatement copies a frame by its own syncinfo size and reads zeros behind it
(oracle/a52_oracle.c, orc_a52_frame), frame_gather_kernel zeroes a slot's tail, crc_kernel sums by the frame's own size.

tests/test_mixed_sizes_cpu.py pins these inputs, tests/test_mixed_sizes_gpu.py runs them through every decoder front end with
the comparators and the plumbing of tests/_decode_matrix.py.

A case is (acmod, lfeon, name); tests/_decode_matrix.py's decode, requests and downmix_request read its first two members.  It
has, built once per process,
  streams(case, "multi"):   one stream of MULTI_F frames per entry of its stream list, stream s = mixed_stream(9400 + 31 s + acmod, ...)
  streams(case, "single"):  nine one-frame streams (no multiple of 8), stream s = one frame of entry s % n of the list at its
                            code s // n, seed 9500 + 31 s + acmod: every size of the case, the largest first
  overrun_short(case):      the short frames of both whose last block's mantissas run on behind the frame's own end."""
import numpy as np

from tests import packer

MULTI_F, SINGLE_S = 4, 9

# name -> (acmod, lfeon, per stream (fscod, the frmsizecod of frame f is codes[f % len(codes)]), the sizes that occur, the slot)
_ALT = lambda odd: [(1, (odd, odd - 1)), (1, (odd - 1, odd))] * 2 + [(1, (odd, odd - 1))]     # noqa: E731
TABLE = {
    "A": (2, 0, _ALT(21), (834, 836)),               # the short one ends in mid-dword; rematrixing, phase flags
    "B": (7, 1, _ALT(23), (974, 976)),               # the shape the fixed-shape kernels take
    "C": (7, 1, [(0, (30,)), (0, (24,)), (1, (28, 29)), (2, (24,)), (1, (29, 28)), (0, (26, 30))],
          (1024, 1280, 1536, 1670, 1672, 1792)),     # tails of hundreds of bytes, three sample rates, one stream changes its bit rate
    "D": (1, 0, _ALT(5), (208, 210)),                # the smallest
}
CASE_LIST = [(v[0], v[1], k) for k, v in TABLE.items()]
FIXED_SHAPE_CASE = (7, 1, "B")
FILLS = (0x00, 0xff, "random")


def case_id(case):
    return "%s_a%d_lfe%d" % (case[2], case[0], case[1])


def slot(case):
    return max(TABLE[case[2]][3])


def own_size(frame):
    """the size a frame's header gives it"""
    return packer.frame_bytes(int(frame[4]) >> 6, int(frame[4]) & 63)


def mixed_stream(seed, F, acmod, lfeon, fscod, codes, bsid=8):
    """F frames of one stream, frame f of frmsizecod codes[f % len(codes)] -> list of 1-D arrays.  One generator per stream, the
    mix levels drawn once per stream, as packer.make_stream does."""
    rng = np.random.default_rng(seed)
    feats = dict(cmixlev=int(rng.integers(0, 4)), surmixlev=int(rng.integers(0, 4)))
    return [packer.make_frame(rng, acmod, lfeon, fscod=fscod, frmsizecod=codes[f % len(codes)], bsid=bsid, features=feats)
            for f in range(F)]


def lay(streams, fb, fill=0, seed=77):
    """streams: S lists of F frames -> [S][F][fb] u8, every frame at the start of its slot, `fill` (a byte, or "random" from
    `seed`) from its own end to fb"""
    S, F = len(streams), len(streams[0])
    if fill == "random":
        out = np.random.default_rng(seed).integers(0, 256, (S, F, fb)).astype(np.uint8)
    else:
        out = np.full((S, F, fb), fill, np.uint8)
    for s, stream in enumerate(streams):
        assert len(stream) == F
        for f, fr in enumerate(stream):
            assert own_size(fr) == len(fr) <= fb
            out[s, f, :len(fr)] = fr
    return out


_BUILT = {}


def streams(case, which):
    """the case's "multi" or "single" batch as lists of frames (see the module's text)"""
    key = (case, which)
    if key not in _BUILT:
        acmod, lfe, entries, _ = TABLE[case[2]]
        n = len(entries)
        if which == "multi":
            out = [mixed_stream(9400 + 31 * s + acmod, MULTI_F, acmod, lfe, fscod, codes) for s, (fscod, codes) in enumerate(entries)]
        else:
            out = []
            for s in range(SINGLE_S):
                fscod, codes = entries[s % n]
                out.append(mixed_stream(9500 + 31 * s + acmod, 1, acmod, lfe, fscod, (codes[(s // n) % len(codes)],)))
        assert len(out[0][0]) == slot(case), "stream 0's first frame is the largest: H.orc_decode_status takes the batch's layout and size from it"
        _BUILT[key] = out
    return _BUILT[key]


def laid(case, which, fill=0):
    """lay() of streams(case, which) (or of overrun_short(case) for "overrun") at the case's slot size, once, read-only"""
    key = (case, which, "laid", fill)
    if key not in _BUILT:
        src = overrun_short(case)[0] if which == "overrun" else streams(case, which)
        _BUILT[key] = lay(src, slot(case), fill)
        _BUILT[key].setflags(write=False)
    return _BUILT[key]


def short_entries(case):
    """(fscod, frmsizecod) of the case's sizes below its slot size, in the order of its stream list"""
    out = []
    for fscod, codes in TABLE[case[2]][2]:
        for c in codes:
            if packer.frame_bytes(fscod, c) < slot(case) and (fscod, c) not in out:
                out.append((fscod, c))
    return out


def overrun_short(case):
    """(streams of two frames, [n] bit positions): tests/_decode_matrix.overrun's construction on the frames of both batches
    that are shorter than the slot, and of sixteen more one-frame streams of the short sizes (seeds 9600 + 31 i + acmod): where
    the last block has a skip field, its length is raised (to 511 bytes at the most) so that the block's mantissas begin in the
    frame's own last byte and run on behind it - into what the slot holds there.  Each such frame is the second frame of a
    stream whose first is the case's full-size frame (stream 0's first frame of the multi batch), so that the batch's slot is
    the case's.  The positions are where the mantissas of those second frames begin."""
    from tests import ac3_syntax as A
    key = (case, "overrun")
    if key not in _BUILT:
        acmod, lfe = case[:2]
        shorts = short_entries(case)
        more = [mixed_stream(9600 + 31 * i + acmod, 1, acmod, lfe, shorts[i % len(shorts)][0], (shorts[i % len(shorts)][1],))
                for i in range(16)]
        full = streams(case, "multi")[0][0]
        out, start = [], []
        for stream in streams(case, "single") + streams(case, "multi") + more:
            for fr in stream:
                own = len(fr)
                if own == slot(case):
                    continue
                B = A.parse_frame(fr).blocks[5]
                if not B.fields["skiple"]:
                    continue
                at = B.pos["skipl"]
                n = min(511, -(-(own * 8 - 8 - (at + 9)) // 8))
                bits = np.unpackbits(fr)
                bits[at:at + 9] = [(n >> (8 - i)) & 1 for i in range(9)]
                out.append([full, np.packbits(bits)])
                start.append(at + 9 + 8 * n)
        _BUILT[key] = (out, np.array(start))
    return _BUILT[key]


def too_long(case):
    """(streams, s): the multi batch with the last frame of stream s - the first stream whose last frame is shorter than the
    slot - given frmsizecod 37 in its header and nothing else changed: by its header it no longer fits the slot"""
    key = (case, "too long")
    if key not in _BUILT:
        src = streams(case, "multi")
        s = next(i for i, st in enumerate(src) if len(st[-1]) < slot(case))
        out = [list(st) for st in src]
        fr = out[s][-1].copy()
        fr[4] = (fr[4] & 0xc0) | 37
        assert packer.frame_bytes(int(fr[4]) >> 6, 37) > slot(case)
        out[s][-1] = fr
        _BUILT[key] = (out, s)
    return _BUILT[key]


def lay_edited(streams_, fb, fill=0):
    """lay() for batches that hold a frame whose header no longer gives its length (too_long)"""
    S, F = len(streams_), len(streams_[0])
    out = np.full((S, F, fb), fill, np.uint8)
    for s, stream in enumerate(streams_):
        for f, fr in enumerate(stream):
            out[s, f, :len(fr)] = fr
    return out


def byte_stream(stream, seed, gaps=True):
    """the frames of one stream end to end, a few bytes without a sync word between some of them"""
    from tests import frame_scan_model
    rng = np.random.default_rng(seed)
    parts = []
    for f, fr in enumerate(stream):
        if gaps and f and rng.random() < 0.5:
            parts.append(frame_scan_model.garbage(int(rng.integers(1, 12)), int(rng.integers(0, 1 << 30))))
        parts.append(fr)
    return np.concatenate(parts)


def sealed(case, which):
    """streams(case, which) with both CRC words of every frame set right (crc_model.seal): the packer leaves a frame's last 18
    bits free and liba52 never reads crc1, so the frames decode to the same samples"""
    from tests import crc_model
    key = (case, which, "sealed")
    if key not in _BUILT:
        _BUILT[key] = [[crc_model.seal(fr) for fr in st] for st in streams(case, which)]
    return _BUILT[key]
