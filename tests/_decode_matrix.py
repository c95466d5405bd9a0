"""The decoder conformance matrix (not collected): thirteen packer layouts off the 48 kHz / 5.1 path, the output requests
liba52 grants for each, the comparator that holds an engine result to the liba52 restatement, and the plumbing of one decode
call.  tests/test_decode_matrix_cpu.py pins the case list (frame sizes, features, the restatement against liba52 itself),
tests/test_decode_matrix_gpu.py runs it through every decoder front end; tests/test_workspace_independence_gpu.py shares the
comparator.

A case is (acmod, lfeon, fscod, bsid, frmsizecod).  It has two batches, built once per process:
  multi(case):  5 streams x 3 frames, stream s = packer.make_stream(8800 + 31 s + acmod, 3, ...)
  single(case): 9 streams x 1 frame,  stream s = packer.make_stream(8900 + 31 s + acmod, 1, ...); nine is no multiple of 8, so
                both branches of the XCD remap in mant_kernel and mantx_kernel run."""
import ctypes

import numpy as np

from tests import _harness as H
from tests import packer

# (acmod, lfeon, fscod, bsid, frmsizecod) -> frame bytes; what each adds is in DESIGN.md §1
CASES = {
    (7, 1, 2, 8, 37): 3840,       # the largest frame the API admits; 32 kHz
    (7, 0, 1, 8, 37): 2788,       # 3/2 without LFE; 44.1 kHz
    (7, 1, 1, 8, 23): 976,        # a small 5.1 frame: the shape the fixed-shape kernels take
    (2, 0, 1, 8, 20): 834,        # bytes 2 mod 4; phase flags, rematrixing; dsurmod turns STEREO into DOLBY per frame
    (2, 1, 0, 8, 14): 448,        # 2/0 + LFE, small
    (1, 0, 0, 8, 4): 192,         # the smallest frame; mono
    (1, 1, 2, 8, 12): 576,        # 1/0 + LFE
    (0, 0, 1, 9, 25): 1116,       # dual mono, dynrng2; bsid 9
    (0, 1, 2, 10, 28): 2304,      # dual mono + LFE; bsid 10
    (3, 1, 1, 8, 29): 1672,       # 3/0 + LFE
    (4, 1, 2, 8, 26): 1920,       # 2/1 + LFE
    (5, 0, 1, 10, 33): 2230,      # 3/1; bytes 2 mod 4; bsid 10
    (6, 1, 1, 9, 35): 2508,       # 2/2 + LFE; bsid 9
}
CASE_LIST = list(CASES)
FIXED_SHAPE_CASE = (7, 1, 1, 8, 23)
THRESHOLD_CASES = [(7, 1, 1, 8, 23), (2, 0, 1, 8, 20), (7, 1, 2, 8, 37)]
DAMAGED_CASES = [(2, 0, 1, 8, 20), (5, 0, 1, 10, 33), (7, 1, 2, 8, 37)]
DAMAGED_SEED = 37

# per source acmod: the layout itself, then the downmixes a52_downmix_init grants
REQUESTS = {0: (0, 1, 8, 9), 1: (1, 2), 2: (2, 1, 10), 3: (3, 2, 10, 1), 4: (4, 2, 10, 1), 5: (5, 3, 2, 10, 1),
            6: (6, 2, 10, 4, 1), 7: (7, 2, 10, 1, 3, 6)}
ADJUST_LEVEL = 32
MULTI_S, MULTI_F, SINGLE_S = 5, 3, 9


def case_id(case):
    return "a%d_lfe%d_fs%d_bsid%d_fsz%d" % case


def requests(case):
    """the case's output requests, the layout first, each with the LFE where the source has one"""
    return [r | (16 if case[1] else 0) for r in REQUESTS[case[0]]]


def forgotten_bias(case, frames, flags, bias):
    """[S] bool: the streams on which the plain linear mix (no ac3mi_set_mix_state) is documented to differ from liba52
    (include/ac3mi.h): a frame with surmixlev "no surround" decoded at a non-zero bias from 2/1 or 2/2 to STEREO or from 3/1
    or 3/2 to 3F.  In the blocks of such a frame whose channels differ in block size liba52 sends the left and right outputs
    out without the bias (downmix.c:528-530, 548-550, 569-580)."""
    from tests import ac3_syntax as A
    acmod, out = case[0], flags & 15
    if not bias or not (acmod & 4) or (out, acmod & 1) not in ((2, 0), (3, 1)):
        return np.zeros(frames.shape[0], bool)
    return np.array([any(A.parse_frame(fr, nblocks=0).fields["surmixlev"] == 2 for fr in stream) for stream in frames])


def downmix_request(case):
    """the 2/0 downmix, or the mono one where 2/0 is the layout or is not granted (dual mono)"""
    return (1 if case[0] in (0, 2) else 2) | (16 if case[1] else 0)


_BATCH = {}


def _batch(case, seed0, S, F):
    key = (case, seed0)
    if key not in _BATCH:
        acmod, lfe, fscod, bsid, fsz = case
        _BATCH[key] = np.stack([packer.make_stream(seed0 + 31 * s + acmod, F, acmod, lfe, fscod=fscod, bsid=bsid, frmsizecod=fsz)
                                for s in range(S)])
        _BATCH[key].setflags(write=False)
    return _BATCH[key]


def multi(case):
    return _batch(case, 8800, MULTI_S, MULTI_F)


def single(case):
    return _batch(case, 8900, SINGLE_S, 1)


def tail_cases():
    """the cases whose frames end inside a dword: the only ones where the masked last dword of the staging loops matters"""
    return [c for c in CASE_LIST if CASES[c] % 4]


def overrun(case):
    """([n][1][fb], [n] bit positions): the frames of both batches, and of sixteen more one-frame streams (seeds 9000 + 31 s +
    acmod), whose last block has a skip field, its length raised (to 511 bytes at the most)
    so that the block's mantissas begin in the frame's last bytes and run on behind them, and where those mantissas begin.  No undamaged frame reads its last
    18 bits (the packer leaves them free), let alone what follows, so only such frames show what a decoder takes for the bytes
    between a frame's end and the end of its last dword.  liba52 reads on into its caller's buffer; the restatement's harness
    keeps zeros there, and so does the engine: it masks the last dword and stages zero words behind it."""
    from tests import ac3_syntax as A
    key = (case, "overrun")
    if key not in _BATCH:
        fb = CASES[case]
        out, start = [], []
        more = _batch(case, 9000, 16, 1)                   # (a skip field reaches 511 bytes: few last blocks of a large frame begin that late)
        for fr in np.concatenate([single(case).reshape(-1, fb), multi(case).reshape(-1, fb), more.reshape(-1, fb)]):
            B = A.parse_frame(fr).blocks[5]
            if not B.fields["skiple"]:
                continue
            at = B.pos["skipl"]
            n = min(511, -(-(fb * 8 - 8 - (at + 9)) // 8))
            bits = np.unpackbits(fr)
            bits[at:at + 9] = [(n >> (8 - i)) & 1 for i in range(9)]
            out.append(np.packbits(bits))
            start.append(at + 9 + 8 * n)
        _BATCH[key] = (np.stack(out)[:, None, :], np.array(start))
        _BATCH[key][0].setflags(write=False)
    return _BATCH[key]


# ---------------------------------------------------------------------------------------------------------------------
# the comparators (moved here from tests/test_workspace_independence_gpu.py, which imports them)

def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        if x.tobytes() != y.tobytes():
            d = np.argwhere(x.view(np.uint8).reshape(x.shape[0], -1) != y.view(np.uint8).reshape(y.shape[0], -1))
            raise AssertionError("%s: `%s` differs in %d bytes of %d rows, first (row, byte) %r" % (
                what, k, len(d), len(set(d[:, 0].tolist())), d[:6].tolist()))


def held_to_liba52(got, ref, first_bad, s16=False):
    """status bits 0-5 and 8 of every frame; PCM of every stream's frames before its damaged one (first_bad[s]; F: none).  A
    damaged frame's PCM is compared among the engine's runs only: where damage leaves bins that liba52 never writes, its
    buffers' contents are no reference (tests/fuzz_corrupt.py blanks them).  Returns the worst figures it saw, for reports:
    float: (RMS error / max(1, RMS level), peak error / max(1, peak level)); s16: (largest step, RMS error in steps / level)."""
    want_status, want_pcm, whole = ref
    assert np.array_equal(got["status"].astype(np.uint32) & 0x13f, want_status), (got["status"] & 0x13f, want_status)
    assert (whole >= first_bad).all(), (whole, first_bad)
    L = H.orc()
    worst = [0.0, 0.0]
    for s in range(got["pcm"].shape[0]):
        n = int(first_bad[s])
        if not n:
            continue
        g = got["pcm"][s, :n]
        w = want_pcm[s, :n]
        if s16:
            # the reference's converter on the restatement's planes at bias 384.  One float32 ulp there is one s16 step, so one
            # step is the floor (as in tests/test_decode_wg_gpu.py); above it the bound is the float path's, 1e-5 of the level
            # where packer mantissas at random exponents reach above +-1.0 (samples that cancel out of such planes carry the
            # rounding of the large terms), in steps - and 4e-5 RMS of the level, the project's figure at bias 384
            oflags = int(got["status"][s, 0] >> 16) & 0xff
            w16 = np.zeros(g.shape, np.int16)
            for f in range(n):
                for b in range(6):
                    L.orc_convert_s16(H.P(np.ascontiguousarray(w[f, b]), H.fp), H.P(w16[f, b], H.i16p), oflags)
            err = g.astype(np.float64) - w16
            level_max, level_rms = max(1.0, float(np.abs(w - 384.0).max())), max(1.0, H.rms(w - 384.0))
            steps = max(1, int(np.ceil(1e-5 * level_max * 32768.0)))
            assert np.abs(err).max() <= steps and H.rms(err) <= 4e-5 * level_rms * 32768.0, (s, np.abs(err).max(), steps, H.rms(err), level_rms)
            worst = [max(worst[0], float(np.abs(err).max())), max(worst[1], H.rms(err) / (level_rms * 32768.0))]
        else:
            # (packer mantissas at random exponents reach far above +-1.0: the bar is relative to full scale or to the level)
            err = g.astype(np.float64) - w
            assert H.rms(err) <= 1e-6 * max(1.0, H.rms(w)), (s, H.rms(err), H.rms(w))
            worst = [max(worst[0], H.rms(err) / max(1.0, H.rms(w))), max(worst[1], float(np.abs(err).max()) / max(1.0, float(np.abs(w).max())))]
    return tuple(worst)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement

_REF = {}


def liba52(key, frames, flags, bias=0.0, level=1.0, dynrng_off=False, state=None):
    """H.orc_decode_status, once per (key, request): (status, pcm, whole).  state: (delay [S][n_out][128], lfsr [S]) the
    streams start from"""
    k = (key, flags, bias, level, dynrng_off, state is not None)
    if k not in _REF:
        _REF[k] = H.orc_decode_status(frames, flags, bias, level=level, dynrng_off=dynrng_off, state=state)
    return _REF[k]


def liba52_stages(key, frames, acmod, flags):
    """the restatement with its stage taps on [S][F][fb], level 1, bias 0, once per (key, request): dict of pcm
    [S][F][6][n_out][256], coef [S][F][6][6][256] (its plane order: the LFE first when it is an output), blksw [S][F][6][5],
    flags [S][F] (granted, per frame: dsurmod can turn STEREO into DOLBY), lfsr [S] (final)"""
    k = ("stages", key, flags)
    if k in _REF:
        return _REF[k]
    L = H.orc()
    L.orc_a52_get_coefs.argtypes = [H.vp, H.fp, H.u8p]
    S, F, fb = frames.shape
    pcm = None
    coef = np.zeros((S, F, 6, 6, 256), np.float32)
    sw = np.zeros((S, F, 6, 5), np.uint8)
    lfsr = np.zeros(S, np.int64)
    granted = np.zeros((S, F), np.int64)
    for s in range(S):
        st = L.orc_a52_init()
        buf = np.zeros(F * fb + 64, np.uint8)
        buf[:F * fb] = frames[s].reshape(-1)
        for f in range(F):
            fl, lv = H.ci(flags), H.cf(1.0)
            assert L.orc_a52_frame(st, ctypes.cast(buf.ctypes.data + f * fb, H.u8p), ctypes.byref(fl), ctypes.byref(lv), 0.0) == 0
            nout = H.NFCHANS[fl.value & 15] + (1 if fl.value & 16 else 0)
            granted[s, f] = fl.value
            if pcm is None:
                pcm = np.zeros((S, F, 6, nout, 256), np.float32)
            for b in range(6):
                assert L.orc_a52_block(st) == 0
                pcm[s, f, b] = np.ctypeslib.as_array(L.orc_a52_samples(st), (1536,))[:nout * 256].reshape(nout, 256)
                L.orc_a52_get_coefs(st, H.P(coef[s, f, b], H.fp), H.P(sw[s, f, b], H.u8p))
        lfsr[s] = L.orc_a52_get_lfsr(st)
        L.orc_a52_free(st)
    _REF[k] = dict(pcm=pcm, coef=coef, blksw=sw, flags=granted, lfsr=lfsr)
    return _REF[k]


# ---------------------------------------------------------------------------------------------------------------------
# one call on the engine

def pad(frames):
    """frames on a stride of whole dwords; what lies between a frame's end and its slot's is 0xff: not the frame's, never read"""
    fb = frames.shape[-1]
    buf = np.full(frames.shape[:-1] + ((fb + 3) & ~3,), 0xff, np.uint8)
    buf[..., :fb] = frames
    return buf


def mid_run_state(S, n_out, seed):
    """overlap tails and dither states of streams in mid-run (the pattern of tests/test_fixed_shape_gpu.py): no tail zero, no
    state 0 or 1.  The tails stay within +-0.5, so that block 0 of an s16 call is samples and not the converter's rails, and
    the bars, which are relative to max(1, level), are at their tightest."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (S, n_out, 128)).astype(np.float32), rng.integers(2, 32768, S).astype(np.int16)


def decode(engine, frames, case, flags, s16=False, level=1.0, dynrng=1, state=None, taps=False, mix=False):
    """frames [S][F][fb] of `case` -> dict of host arrays: pcm, status, delay, lfsr (and coef, blksw with taps) of one call
    on new streams, or on streams that start from state = (delay, lfsr).  s16: ac3mi_decode_s16_batch (level 1, bias 384).
    mix: under ac3mi_set_mix_state, its two arrays new as well and returned (mix_pending, mix_flags)."""
    import torch
    S, F, fb = frames.shape
    desc = H.pkg().DecodeDesc(flags=flags, level=level, bias=384.0 if s16 else 0.0, dynrng=dynrng, acmod=case[0], lfeon=case[1],
                              frame_bytes=fb)
    n_out, _ = engine.decode_planes(desc)
    if state is None:
        delay = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
        lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    else:
        delay, lfsr = torch.from_numpy(state[0].copy()).cuda(), torch.from_numpy(state[1].copy()).cuda()
        assert tuple(delay.shape) == (S, n_out, 128)
    d_frames = torch.from_numpy(pad(frames)).cuda()
    tp = None
    pending = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
    mflags = torch.zeros((S, 6), dtype=torch.int32, device="cuda")
    try:
        if mix:
            engine.set_mix_state(pending, mflags)
        if s16:
            assert level == 1.0 and not taps
            out, status = engine.decode_s16_batch(desc, d_frames, delay, lfsr)
        elif taps:
            out, status, tp = engine.decode_batch(desc, d_frames, delay, lfsr, taps=True)
        else:
            out, status = engine.decode_batch(desc, d_frames, delay, lfsr)
        engine.sync()
    finally:
        if mix:
            engine.set_mix_state(None, None)
    host = lambda t: np.ascontiguousarray(t.cpu().numpy())
    res = dict(pcm=host(out), status=host(status), delay=host(delay), lfsr=host(lfsr))
    if mix:
        res.update(mix_pending=host(pending), mix_flags=host(mflags))
    if tp:
        res.update(coef=host(tp["coef"]), blksw=host(tp["blksw"]))
    return res
