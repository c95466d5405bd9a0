"""GPU: ac3mi_set_fixed_shape.  A 5.1 call of one-frame streams takes the kernels that have that shape compiled in (parse,
mantissa + transform, MDCT, search, frame packer); with the switch off it takes the generic ones.  Every output and every
piece of carried state must be byte-equal between the two, from identical state that is NOT a fresh stream's: a non-zero
overlap tail and dither state, a non-zero encoder history, search states other than 40.  The source frames are the
project's own encoder's, from `bursts` content: plain, coupled (chincpl != 0 through the parse and mantissa kernels) and
block-switched (short blocks in the transform); one batch holds frames the decoder refuses.  Batches of 1, 9 and 130
streams: 9 and 130 are no multiples of 8 (both branches of the XCD remap), 130 x 6 channel units leave a remainder too.
Calls of another shape, or with a tool on, take the generic kernels whatever the switch says: same bytes as well."""
import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import ac3_syntax as A
from tests import variant_matrix as V

pytestmark = pytest.mark.gpu

SMAX = 130
SIZES = (1, 9, 130)
SOURCES = {"plain": {}, "coupled": {"cpl": (1, 2)}, "switched": {"bsw": 1}}


def _bursts(S, F=1, nch=6, seed=7100):
    """[S][F*1536][nch]: S streams cut from one run of the harness's `bursts` content"""
    return H.gen_pcm(S * F, nch, seed=seed, kind="bursts").reshape(S, F * 1536, nch)


@pytest.fixture(scope="module")
def sources(engine):
    """name -> frames [SMAX][1][fb] of the project's encoder, computed once; the tools' effect is checked here"""
    pcm = _bursts(SMAX)
    out = {k: T.encode(engine, pcm, **tools) for k, tools in SOURCES.items()}
    first = [A.parse_frame(fr[0], nblocks=6) for fr in out["coupled"][:9]]
    assert any(B.cplinu and any(B.chincpl) for P in first for B in P.blocks), "no coupled frame among the first nine"
    first = [A.parse_frame(fr[0], nblocks=6) for fr in out["switched"][:9]]
    assert any(B.fields.get("blksw%d" % c, 0) for P in first for B in P.blocks for c in range(5)), "no short block among the first nine"
    return out


def _padded(frames):
    S, F, fb = frames.shape
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = frames
    return buf


def _state(S, n_out, seed):
    """carried state of streams in mid-run: overlap tails, dither states, encoder history, search states"""
    rng = np.random.default_rng(seed)
    return dict(delay=rng.uniform(-300.0, 300.0, (S, n_out, 128)).astype(np.float32),
                lfsr=rng.integers(1, 32768, S).astype(np.int16),
                last=rng.integers(-9000, 9001, (S, n_out, 256)).astype(np.int16),
                csnr=(rng.integers(6, 34, S) | (rng.integers(0, 16, S) << 8)).astype(np.int32))


def _fx(log):
    """the fixed-shape kernels among a log's names: the five FX instantiations of csrc/launch_rule.h"""
    fx = {V.dec(4, fx=1), V.mantx(s16=1, fx=1), V.mdct(fx=1), V.search(1, fx=1)} | {V.packf(fx=1, bw=b, md=m, dw=w) for b in (0, 1) for m, w in ((0, 0), (1, 0), (1, 1))}
    return [k for k in log if k in fx]


DEC_FX = {V.dec(4, fx=1), V.mantx(s16=1, fx=1)}


def _both(engine, call, fixed=True, mode=0):
    """call() with the switch on and off, under ac3mi_set_decode_mode `mode` -> the two lists of host arrays.  What the switch
    is said to do, it did (ac3mi_debug_launch_log): a call of the fixed shape (`fixed`) launched fixed-shape kernels with the
    switch on and none with it off; any other call launched none either way.  Mode 6: the decoder's two among them (the
    default mode hands batches of up to 512 streams to the one-workgroup-per-stream kernel, which has no such instantiation)"""
    res = []
    try:
        engine.set_decode_mode(mode)
        for on in (1, 0):
            engine.set_fixed_shape(on)
            with V.tap(engine) as log:
                res.append([np.ascontiguousarray(t.cpu().numpy()) for t in call()])
            assert bool(_fx(log)) == bool(fixed and on), (on, log)
            assert mode != 6 or DEC_FX <= set(log) or not (fixed and on), (on, log)
    finally:
        engine.set_fixed_shape(1)
        engine.set_decode_mode(0)
    return res


def _same(names, got, want):
    for n, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), n


def _transcode(engine, frames, acmod=7, lfeon=1, flags=7 | 16 | 32, chmap=H.CHMAP6, rate=384000, seed=1):
    """-> a function that runs one transcode from the same mid-run state each time: frames, status, delay, lfsr, last, csnr"""
    import torch
    pkg = H.pkg()
    S, F, fb = frames.shape
    dec = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0, dynrng=1, acmod=acmod, lfeon=lfeon, frame_bytes=fb)
    n_out, _ = engine.decode_planes(dec)
    enc = pkg.EncodeDesc(48000, rate, n_out)
    src = torch.from_numpy(_padded(frames)).cuda()
    st0 = _state(S, n_out, seed)

    def call():
        st = {k: torch.from_numpy(v.copy()).cuda() for k, v in st0.items()}
        out, status = engine.transcode_batch(dec, enc, src, st["delay"], st["lfsr"], chmap, st["last"], st["csnr"])
        engine.sync()
        return out, status, st["delay"], st["lfsr"], st["last"], st["csnr"]
    return call


TC_NAMES = "frames status delay lfsr last_samples csnroffst".split()


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("kind", sorted(SOURCES))
def test_transcode(engine, sources, kind, S):
    for mode in (0, 6):         # (6: the split front end's fixed-shape kernels, whatever the batch size)
        on, off = _both(engine, _transcode(engine, sources[kind][:S], seed=10 + S), mode=mode)
        _same(TC_NAMES, on, off)
        assert int((on[1] & 0x1ff).max()) == 0 and on[0].any()


def test_transcode_refused_frames(engine, sources):
    """a broken sync word, a header that claims acmod 2, a frame of zeros: refused alike, the status words equal"""
    fr = sources["plain"][:9].copy()
    fr[2, 0, 0] ^= 0x40
    fr[4, 0, 6] = (fr[4, 0, 6] & 0x1f) | (2 << 5)
    fr[7, 0, :] = 0
    on, off = _both(engine, _transcode(engine, fr, seed=31))
    _same(TC_NAMES, on, off)
    st = on[1][:, 0]
    assert all(st[s] & 0x100 for s in (2, 4, 7)) and not any(st[s] & 0x1ff for s in (0, 1, 3, 5, 6, 8))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("kind", sorted(SOURCES))
def test_decode_s16(engine, sources, kind, S):
    import torch
    frames = sources[kind][:S]
    dec = H.pkg().DecodeDesc(flags=7 | 16 | 32, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=frames.shape[2])
    src = torch.from_numpy(_padded(frames)).cuda()
    st0 = _state(S, 6, 50 + S)

    def call():
        delay, lfsr = torch.from_numpy(st0["delay"].copy()).cuda(), torch.from_numpy(st0["lfsr"].copy()).cuda()
        pcm, status = engine.decode_s16_batch(dec, src, delay, lfsr)
        engine.sync()
        return pcm, status, delay, lfsr
    # the default mode decodes so small a batch in the one-workgroup-per-stream kernel, which has no fixed-shape
    # instantiation; mode 6 takes the split front end, whose parse and mantissa kernels have
    on, off = _both(engine, call, fixed=False)
    _same("pcm status delay lfsr".split(), on, off)
    on6, off6 = _both(engine, call, mode=6)
    _same("pcm status delay lfsr".split(), on6, off6)
    _same("pcm status delay lfsr".split(), on6, on)
    assert int((on[1] & 0x1ff).max()) == 0 and on[0].any()


@pytest.mark.parametrize("S", SIZES)
def test_encode(engine, S):
    import torch
    pcm = torch.from_numpy(_bursts(S, seed=7300).reshape(S, 1, 1536, 6)).cuda()
    enc = H.pkg().EncodeDesc(48000, 384000, 6)
    st0 = _state(S, 6, 70 + S)

    def call():
        last, csnr = torch.from_numpy(st0["last"].copy()).cuda(), torch.from_numpy(st0["csnr"].copy()).cuda()
        out = engine.encode_batch(enc, pcm, H.CHMAP6, last, csnr)
        engine.sync()
        return out, last, csnr
    on, off = _both(engine, call)
    _same("frames last_samples csnroffst".split(), on, off)
    assert on[0].any()


def test_tiled_transcode(engine, sources):
    """ac3mi_set_tile_frames 8, 20 streams: the call goes through in three tiles, whose kernels address the streams' state
    through slot tables"""
    call = _transcode(engine, sources["plain"][:20], seed=90)
    whole = [np.ascontiguousarray(t.cpu().numpy()) for t in call()]
    try:
        engine.set_tile_frames(8)
        on, off = _both(engine, call)
    finally:
        engine.set_tile_frames(131072)
    _same(TC_NAMES, on, off)
    _same(TC_NAMES, on, whole)


def test_other_calls_take_the_generic_kernels(engine, sources):
    """2/0, 3/2 without the LFE, two frames a stream, and 5.1 with DRC on: the same bytes whatever the switch says"""
    import torch
    S = 9
    calls = {"2/0": _transcode(engine, T.encode(engine, _bursts(S, nch=2, seed=7400)), 2, 0, 2, (0, 1), 192000, seed=91),
             "3/2": _transcode(engine, T.encode(engine, _bursts(S, nch=5, seed=7500)), 7, 0, 7, tuple(range(5)), 384000, seed=92),
             "two frames": _transcode(engine, T.encode(engine, _bursts(S, F=2, seed=7600)), seed=93)}
    for name, call in calls.items():
        on, off = _both(engine, call, fixed=False)
        _same(TC_NAMES, on, off)
        assert int((on[1] & 0x1ff).max()) == 0, name
    plain = _transcode(engine, sources["plain"][:S], seed=94)

    def with_drc():
        engine.set_encode_drc(1, torch.zeros((S,), dtype=torch.int32, device="cuda"))
        try:
            return plain()
        finally:
            engine.set_encode_drc(0)
    on, off = _both(engine, with_drc, fixed=False)
    _same(TC_NAMES, on, off)
    assert not np.array_equal(on[0], plain()[0].cpu().numpy())          # (DRC was on: other bytes than without)
