"""GPU: every byte a batch call returns, and all state it hands back, is a function of its arguments and the context's settings -
never of what the context's workspaces held before ("Workspaces carry nothing from call to call").

The fourteen workspaces come from hipMalloc, are never cleared, only grow, and are reused by every call whatever its shape,
front end or tool set.  The variant-equality tests of the suite run one variant after another on the same context, so a kernel
that read a cell its own call never wrote would find the right value there, left a moment earlier by the variant before it.
Here every call runs four times (`four_runs`):

1. a larger call of another configuration first - more streams, more frames, another layout and front end, every tool on
   (the large batches: more frames of the same layout through other kernels) - so that the workspaces are larger than the
   call under test needs and hold foreign data at other strides;
2. the call itself, unfilled: the baseline;
3. three more times, each after ac3mi_fill_workspaces with 0x00, 0xff, 0xa5, from state tensors (overlap tails, dither and
   search state, encoder history, DRC state, the mix state's two arrays) built afresh from the same seeds, the outputs the header documents as fully written pre-filled with another byte pattern each time (d_status is not
   documented so: zeroed, as engine.py does), ac3mi_workspace_bytes the same and non-zero around each run.

The four runs must agree bit for bit in every output and every piece of returned state.  Equality among the engine's own runs
is not enough, so each baseline is also held to the reference the project has for it: decode to the liba52 restatement (status
bits, first failing block, PCM to 1e-6 RMS on the undamaged streams), mode-0 encodes to the encoder oracle byte for byte, encodes
with tools to a clean decode plus the bit-budget and mantissa audits, transcodes to decode + convert + encode as three calls
on a context filled with yet another byte.

The control (test_control_*): what the suite documents as a leak - rows and bins of the exponent tap that the frame does not
define - does not come from a workspace: the parse kernel dumps its LDS rows there (decode_kernel.h), which hold the stream's
earlier frames under the per-stream parse kernel and zeros under the per-frame one.  The control pins that: the tap's undefined
cells are the same under every fill, differ between the two front ends, and the defined ones agree.  No output byte of the
library follows the fill, so no test here can show one that does; that the fill is in place over a non-zero extent is checked
around every run, and that it reaches what kernels read was shown once with a scratch build (not kept) whose mant_kernel
leaves a failed block's coefficient planes unwritten instead of zeroing them: 18 of the decode and transcode cases below then
fail under the first fill, in `pcm` or `frames` - every case whose front end hands planes to the transform through ws_coef."""
import ctypes
import os

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import ac3_syntax as A
from tests import bsi_model as BM
from tests import coupling_model as C
from tests import crc_model
from tests import dynrng_model as D
from tests import mantissa_audit as MA
from tests import packer
from tests import test_frame_budget_gpu as B
from tests._decode_matrix import held_to_liba52 as _held_to_liba52, same      # (shared with tests/test_decode_matrix_gpu.py)

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
PATTERNS = (0x3C, 0xC3, 0x69, 0x96)       # what the outputs hold before run 0..3
OTHER_FILL = 0x5A                         # the context of a reference made of other calls


# ---------------------------------------------------------------------------------------------------------------------
# the four runs

def _host(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _restore(engine):
    """the settings the rest of the suite runs under (the modes: what the environment selects, as the other tests restore)"""
    engine.set_decode_mode(int(os.environ.get("AC3MI_DECODE_MODE", "0")))
    engine.set_decode_crc(0)
    engine.set_fixed_shape(1)
    engine.set_tile_frames(131072)
    engine.set_mix_state(None, None)
    engine.set_encode_mode(int(os.environ.get("AC3MI_ENCODE_MODE", "0")))
    engine.set_encode_layout(0)
    engine.set_encode_metadata()
    engine.set_encode_metadata_frames(None)
    engine.set_encode_metadata_source(0)
    engine.set_encode_dynrng_frames(None, None)
    engine.set_encode_drc_source(0)
    engine.set_encode_drc(0)
    for k in ("bsw", "remat", "cpl", "bw", "xs"):
        getattr(engine, T.TOOLS[k][0])(*T.TOOLS[k][2])


_PRIME = {}


def _prime_inputs():
    if not _PRIME:
        _PRIME["src51"] = np.stack([H.orc_encode(H.gen_pcm(4, 6, seed=8800 + s, kind=("tones", "bursts", "music", "noise")[s % 4]))
                                    for s in range(14)])
        _PRIME["pcm2"] = T.stereo("music_nearmono", 12, 5, seed=8900)
    return _PRIME


def prime(engine):
    """14 x 4 5.1 frames transcoded through the frame-parallel split front end with the CRC kernel and both source modes on
    (ws_coef, ws_blksw, ws_draws, ws_split, ws_tc, ws_enc, ws_crc, ws_bsi, ws_dyn), then 12 x 5 stereo frames encoded with
    every tool (ws_bsw, ws_remat, ws_cpl, ws_cplr, ws_drc): more streams and frames than any small case below, at other
    strides.  Settings are the defaults again afterwards."""
    import torch
    P = _prime_inputs()
    pkg = H.pkg()
    src = P["src51"]
    S, F, fb = src.shape
    try:
        engine.set_decode_mode(5)
        engine.set_decode_crc(1)
        engine.set_encode_metadata_source(1)
        engine.set_encode_drc_source(1)
        dec = pkg.DecodeDesc(flags=7 | 16, level=1.0, bias=384.0, dynrng=0, acmod=7, lfeon=1, frame_bytes=fb)
        enc = pkg.EncodeDesc(48000, 448000, 6)
        engine.transcode_batch(dec, enc, torch.from_numpy(src).cuda(), torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda"),
                               torch.ones((S,), dtype=torch.int16, device="cuda"), H.CHMAP6,
                               torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda"),
                               torch.full((S,), 40, dtype=torch.int32, device="cuda"))
        engine.sync()
    finally:
        _restore(engine)
    T.encode(engine, P["pcm2"], rate=192000, bsw=1, remat=1, cpl=(1, 2), bw=(2, 0), xs=1, drc=1)


def prime_large(engine, S, F, what):
    """for the large batches, more 5.1 frames than the call under test has, through other kernels: `what` = "decode": S x F
    encoder frames through the frame-parallel front end to 5.1 float; "encode": S x F frames with block switching"""
    import torch
    key = ("large", S, F, what)
    if key not in _PRIME:
        if what == "decode":
            base = np.stack([H.orc_encode(H.gen_pcm(F, 6, seed=8950 + s, kind="tones")) for s in range(4)])
        else:
            base = T.pcm("attack", 4, F, 6, seed=8960)
        _PRIME[key] = np.ascontiguousarray(base[np.arange(S) % 4])
    data = _PRIME[key]
    if what == "encode":
        T.encode(engine, data, bsw=1)
        return
    try:
        engine.set_decode_mode(5)
        desc = H.pkg().DecodeDesc(flags=7 | 16, level=1.0, bias=0.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=data.shape[2])
        engine.decode_batch(desc, torch.from_numpy(data).cuda(), torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda"),
                            torch.ones((S,), dtype=torch.int16, device="cuda"))
        engine.sync()
    finally:
        _restore(engine)


def four_runs(engine, call, configure=None, primer=prime):
    """call(run) -> dict of host arrays, run = 0..3 (it builds its state afresh and pre-fills its outputs with PATTERNS[run]).
    configure(): the context's settings of the call under test - applied after the larger call, which leaves the defaults
    behind; the caller restores them in a `finally`.  Returns the baseline's."""
    primer(engine)
    if configure:
        configure()
    base = call(0)
    assert engine.workspace_bytes() > 0
    for run, byte in enumerate(FILLS, 1):
        before = engine.workspace_bytes()
        engine.fill_workspaces(byte)
        got = call(run)
        assert engine.workspace_bytes() == before and before > 0, "a workspace was re-allocated: the fill was not in place"
        same(got, base, "workspaces filled with %#04x against the unfilled run" % byte)
    return base


def test_fill_workspaces_arguments(engine):
    """a byte outside 0..255 is AC3MI_ERR_ARG and fills nothing; a context that holds no workspace yet has nothing to fill"""
    ctx = ctypes.c_void_p(engine.ctx)
    prime(engine)
    before = engine.workspace_bytes()
    for byte in (-1, 256, 0x1a5):
        assert engine.lib.ac3mi_fill_workspaces(ctx, byte) == -1
    for byte in (0, 255):
        assert engine.lib.ac3mi_fill_workspaces(ctx, byte) == 0
    engine.sync()
    assert engine.workspace_bytes() == before > 0
    fresh = H.pkg().Engine(0)
    try:
        assert fresh.workspace_bytes() == 0
        fresh.fill_workspaces(0xa5)
        fresh.sync()
        assert fresh.workspace_bytes() == 0
    finally:
        fresh.close()


def _pattern(shape, dtype, run):
    import torch
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(PATTERNS[run])
    return t


# ---------------------------------------------------------------------------------------------------------------------
# decode

def _pad(frames):
    fb = frames.shape[-1]
    buf = np.zeros(frames.shape[:-1] + ((fb + 3) & ~3,), np.uint8)
    buf[..., :fb] = frames
    return buf


def _decode(engine, frames, acmod, lfe, flags, run, s16=False, mix=False):
    """frames [S][F][fb] -> pcm, status, delay, lfsr of one call on new streams (what the restatement starts from); mix: with
    ac3mi_set_mix_state on, its two arrays new as well and returned"""
    import torch
    pkg = H.pkg()
    S, F, fb = frames.shape
    desc = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0 if s16 else 0.0, dynrng=1, acmod=acmod, lfeon=lfe, frame_bytes=fb)
    n_out, _ = engine.decode_planes(desc)
    delay = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    status = torch.zeros((S, F), dtype=torch.int32, device="cuda")
    d_frames = torch.from_numpy(_pad(frames)).cuda()
    out = _pattern((S, F, 6, 256, n_out) if s16 else (S, F, 6, n_out, 256), torch.int16 if s16 else torch.float32, run)
    pending = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
    mflags = torch.zeros((S, 6), dtype=torch.int32, device="cuda")
    try:
        if mix:
            engine.set_mix_state(pending, mflags)
        if s16:
            engine.decode_s16_batch(desc, d_frames, delay, lfsr, out=out, status=status)
        else:
            engine.decode_batch(desc, d_frames, delay, lfsr, out=out, status=status)
        engine.sync()
    finally:
        if mix:
            engine.set_mix_state(None, None)
    res = dict(pcm=_host(out), status=_host(status), delay=_host(delay), lfsr=_host(lfsr))
    if mix:
        res.update(mix_pending=_host(pending), mix_flags=_host(mflags))
    return res


_liba52 = H.orc_decode_status


_DEC = {}


FLIP_LEVELS = ((1, 2, 1), (2, 1, 2), (2, 2, 1), (1, 1, 2))      # surmixlev codes frame by frame; 2 = "no surround", level 0


def _decode_batch(acmod, lfe, S, F, flip=False):
    """[S][F][fb] packer streams (coupling, rematrixing, block switching, delta bit allocation; one pair of mix levels, as a
    programme has) with, in the one batch, a broken sync word, bits flipped in mid-frame, and frames of
    fuzz_corrupt.make_damaged at the head of the last streams (failed blocks, AC3MI_STATUS_REUSE0) -> (frames, per stream the
    index of its damaged frame, F where it has none).  flip: the surround mix level changes from stream to stream and from
    frame to frame, to zero and back (packer.make_flip_stream) - what ac3mi_set_mix_state exists for."""
    from tests import fuzz_corrupt
    key = (acmod, lfe, S, F, flip)
    if key in _DEC:
        return _DEC[key]
    feats = dict(cmixlev=1, surmixlev=1, dsur=0.0)
    if flip:
        frames = np.stack([packer.make_flip_stream(9200 + 37 * s, FLIP_LEVELS[s % 4][:F], acmod, lfe, frmsizecod=30) for s in range(S)])
    else:
        frames = np.stack([packer.make_stream(9100 + 37 * s + acmod, F, acmod, lfe, frmsizecod=30, features=feats) for s in range(S)])
    fb = frames.shape[2]
    rng = np.random.default_rng(acmod + S)
    if ("damaged", acmod, lfe) not in _DEC:
        _DEC[("damaged", acmod, lfe)] = fuzz_corrupt.make_damaged(21, acmod, lfe, S=48)
    bad, _, want_fail, want_foreign, _ = _DEC[("damaged", acmod, lfe)]
    assert bad.shape[1] == fb
    pick = [i for i in range(6, 48) if not want_foreign[i]]
    pick = [i for i in pick if want_fail[i] < 6][:2 if F == 1 else 1] + [i for i in pick if want_fail[i] == 6][:1 if F == 1 else 0]
    n_dmg = len(pick) + 1
    clean = S - 2 - n_dmg
    assert clean >= 2
    frames[clean, F // 2, 0] ^= 0x40                                                  # a broken sync word
    frames[clean + 1, F - 1, fb // 2:fb // 2 + 8] ^= rng.integers(1, 255, 8).astype(np.uint8)      # bits flipped in mid-frame
    for k, i in enumerate(pick):
        frames[clean + 2 + k, 0] = bad[i]
    # ... and one whose block 0 says "no bit-allocation parameters" (baie 0): it reuses what no block sent (REUSE0), decodes,
    # and the blocks after it fail on the bits that were the parameters
    fr = frames[S - 1, 0]
    bits = np.unpackbits(fr)
    bits[A.parse_frame(fr, nblocks=1).blocks[0].pos["baie"]] = 0
    frames[S - 1, 0] = np.packbits(bits)
    first_bad = np.array([F] * clean + [F // 2, F - 1] + [0] * n_dmg)
    _DEC[key] = (frames, first_bad)
    return _DEC[key]


_REF = {}


def _decode_reference(key, frames, flags, bias=0.0):
    if (key, flags, bias) not in _REF:
        _REF[(key, flags, bias)] = _liba52(frames, flags, bias)
    return _REF[(key, flags, bias)]


DECODE_MODES = (1, 3, 4, 5, 6, 0)
OUTPUTS = {(7, 1): ((7 | 16, False), (7 | 16, True), (2, False), (2, True), (1, False), (1, True)), (2, 0): ((2, False), (2, True))}


@pytest.mark.parametrize("mode", DECODE_MODES)
@pytest.mark.parametrize("S,F", [(10, 1), (6, 3)])
@pytest.mark.parametrize("acmod,lfe", [(7, 1), (2, 0)])
def test_decode(engine, acmod, lfe, S, F, mode):
    """every front end and auto; float and s16; the layout itself and, from 5.1, the downmixes to 2/0 and to mono, which read
    ws_blksw and run the mixing transform on ws_coef's planes - those of refused frames and failed blocks included"""
    frames, first_bad = _decode_batch(acmod, lfe, S, F)
    clean = int((first_bad == F).sum())
    try:
        seen = 0
        for flags, s16 in OUTPUTS[(acmod, lfe)]:
            base = four_runs(engine, lambda run: _decode(engine, frames, acmod, lfe, flags | (32 if s16 else 0), run, s16),
                             lambda: engine.set_decode_mode(mode))
            ref = _decode_reference((acmod, lfe, S, F), frames, flags | (32 if s16 else 0), 384.0 if s16 else 0.0)
            _held_to_liba52(base, ref, first_bad, s16)
            st = base["status"]
            seen |= int(np.bitwise_or.reduce(st.ravel()))
            assert (st[clean, F // 2] & 0x100) and np.abs(base["pcm"][:clean]).max() > 0
        print("decode acmod %d mode %d %dx%d: status bits seen %#x (0x200 = REUSE0)" % (acmod, mode, S, F, seen & 0xffff))
        assert seen & 0x3f and seen & 0x100 and seen & 0x200
        # the downmixes again under ac3mi_set_mix_state, on streams whose surround level goes to zero and back: the front end
        # leaves a "level 0" flag per frame behind the block-switch flags in ws_blksw - for refused frames too - and the
        # transform reads the frame's and the next frame's
        if acmod == 7:
            flipped, first_bad = _decode_batch(acmod, lfe, S, F, flip=True)
            for flags, s16 in ((2, False), (2, True), (1, False), (1, True)):
                req = flags | (32 if s16 else 0)
                base = four_runs(engine, lambda run: _decode(engine, flipped, acmod, lfe, req, run, s16, mix=True),
                                 lambda: engine.set_decode_mode(mode))
                _held_to_liba52(base, _decode_reference((acmod, lfe, S, F, "flip"), flipped, req, 384.0 if s16 else 0.0), first_bad, s16)
                assert base["status"][clean, F // 2] & 0x100
                if F > 1:           # the flags decided something: without them (the plain linear mix) other samples, other tails
                    engine.set_decode_mode(mode)
                    linear = _decode(engine, flipped, acmod, lfe, req, 0, s16)
                    assert not np.array_equal(linear["pcm"][:clean], base["pcm"][:clean])
                    assert base["mix_flags"][:clean].any()
    finally:
        _restore(engine)


@pytest.mark.parametrize("crc", [1, 2])
@pytest.mark.parametrize("mode", [0, 4, 5])
def test_decode_crc(engine, crc, mode):
    """ws_crc: one frame failing each CRC in a 5 x 3 batch of sealed packer frames; the status is the model's, and under
    mode 2 the outputs are mode 0's on the batch with the failing frames' sync words zeroed"""
    S, F = 5, 3
    feats = dict(cmixlev=1, surmixlev=1)
    frames = np.stack([np.stack([crc_model.seal(f) for f in packer.make_stream(9300 + s, F, 7, 1, frmsizecod=30, features=feats)])
                       for s in range(S)])
    fb = frames.shape[2]
    frames[1, 2, 40] ^= 0x04                     # in the first 5/8: crc1
    frames[3, 0, fb - 30] ^= 0x20                # in the rest: crc2
    v = crc_model.verdicts(frames.reshape(S * F, fb)).reshape(S, F)
    assert v[1, 2] == 1 and v[3, 0] == 2 and np.count_nonzero(v) == 2
    def configure():
        engine.set_decode_mode(mode)
        engine.set_decode_crc(crc)

    try:
        base = four_runs(engine, lambda run: _decode(engine, frames, 7, 1, 7 | 16, run), configure)
        assert np.array_equal((base["status"].astype(np.uint32) >> 10) & 3, v & 3)
        zeroed = frames.copy()
        if crc == 2:
            zeroed[v != 0, :2] = 0
        engine.set_decode_crc(0)
        engine.fill_workspaces(OTHER_FILL)
        plain = _decode(engine, zeroed, 7, 1, 7 | 16, 0)
        plain["status"] = plain["status"] | ((v.astype(np.int32) & 3) << 10)
        same(base, plain, "CRC mode %d against mode 0" % crc)
        _held_to_liba52(plain, _liba52(zeroed, 7 | 16), np.array([F, 2, F, 0, F]))
    finally:
        _restore(engine)


def test_decode_large_batch(engine):
    """5120 streams of two frames, eight originals replicated: the first stream count at which auto leaves the frame-parallel
    front end for the parse kernel per stream.  The restatement checks the originals, the replicas are compared with them."""
    S, F = 5120, 2
    orig, first_bad = _decode_batch(7, 1, 8, F)
    frames = np.ascontiguousarray(orig[np.arange(S) % 8])
    # (to 2/0: the mixing transform reads ws_coef and ws_blksw, and the PCM that crosses PCIe eight times is a third)
    base = four_runs(engine, lambda run: _decode(engine, frames, 7, 1, 2, run), primer=lambda e: prime_large(e, 5200, 3, "decode"))
    _held_to_liba52({k: v[:8] for k, v in base.items()}, _decode_reference((7, 1, 8, F), orig, 2), first_bad)
    for k, v in base.items():
        r = v.view(np.uint8).reshape(S // 8, -1)
        assert np.array_equal(r, np.broadcast_to(r[:1], r.shape)), k


# ---------------------------------------------------------------------------------------------------------------------
# encode

def _encode(engine, pcm, run, drc_state=False, **kw):
    """pcm [S][F*1536][nch] -> frames [:frame_bytes], last, csnroffst[, the DRC state] of one T.encode call on new streams"""
    import torch
    S, n, nch = pcm.shape
    fb = H.pkg().EncodeDesc(kw.get("sr", 48000), kw.get("rate") or T.RATE[nch], nch).frame_bytes()
    last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    state = torch.zeros((S,), dtype=torch.int32, device="cuda") if drc_state else None
    out = _pattern((S, n // 1536, (fb + 3) & ~3), torch.uint8, run)
    frames = T.encode(engine, pcm, last=last, csnr=csnr, state=state, out=out, **kw)
    res = dict(frames=np.ascontiguousarray(frames), last=_host(last), csnr=_host(csnr))
    if drc_state:
        res["drc_state"] = _host(state)
    return res


def _oracle_encode(pcm, nch=6, rate=384000, sr=48000, chmap=H.CHMAP6):
    return np.stack([H.orc_encode(p, nch, rate, sr, chmap) for p in pcm])


KINDS = ("bursts", "tones", "strobe", "music", "noise", "quiet", "bursts")


@pytest.mark.parametrize("S,F,fixed,pack", [(7, 1, 1, 0), (7, 1, 0, 0), (7, 1, 1, 1), (7, 1, 1, 2), (3, 4, 1, 0), (3, 4, 1, 1), (3, 4, 1, 2)])
def test_encode_mode_0(engine, S, F, fixed, pack):
    """5.1 with no tool: 7 one-frame streams (the fixed-shape kernels, and the generic ones), 3 x 4 (the ws_memo tabulation), both
    packers - the encoder oracle's bytes"""
    pcm = np.stack([H.gen_pcm(F, 6, seed=9400 + s, kind=KINDS[s]) for s in range(S)])
    try:
        base = four_runs(engine, lambda run: _encode(engine, pcm, run, pack=pack), lambda: engine.set_fixed_shape(fixed))
    finally:
        _restore(engine)
    assert np.array_equal(base["frames"], _oracle_encode(pcm))


def test_encode_large_batch(engine):
    """2048 streams of two frames, eight originals replicated: the first stream count whose search runs without the memo"""
    S, F = 2048, 2
    orig = np.stack([H.gen_pcm(F, 6, seed=9450 + s, kind=KINDS[s % 7]) for s in range(8)])
    pcm = np.ascontiguousarray(orig[np.arange(S) % 8])
    base = four_runs(engine, lambda run: _encode(engine, pcm, run), primer=lambda e: prime_large(e, 2100, 3, "encode"))
    assert np.array_equal(base["frames"][:8], _oracle_encode(orig))
    for k, v in base.items():
        r = v.view(np.uint8).reshape(S // 8, -1)
        assert np.array_equal(r, np.broadcast_to(r[:1], r.shape)), k


def test_encode_failed_search_follows_the_reference(engine):
    """3 channels at 48 kb/s and 24 kHz (test_encode_gpu.test_failed_search_follows_the_reference): frames whose search fails
    repeat the offsets of the frame before, which reach the packers through ws_snr - the oracle's bytes, under both packers"""
    from tests.test_encode_gpu import _oracle
    pcm = np.stack([H.gen_pcm(4, 3, seed=101000 + 25 * 7 + s, kind=k) for s, k in enumerate(("music", "tones", "tones", "music"))])
    want, taps = _oracle(list(pcm), 3, 48000, 24000, tuple(range(8)))
    snr = taps["snr"].reshape(4, 4, 2)
    assert np.array_equal(snr[0, 3], snr[0, 2]) and np.array_equal(snr[3, 2], snr[3, 1]), "no frame repeats stale offsets: no search failed"
    for pack in (0, 1, 2):
        try:
            base = four_runs(engine, lambda run: _encode(engine, pcm, run, rate=48000, sr=24000, chmap=(0, 1, 2), pack=pack))
        finally:
            _restore(engine)
        assert np.array_equal(base["frames"], want), pack


@pytest.mark.parametrize("F", [1, 2])
def test_encode_starved_bit_rate(engine, F):
    """6 channels of noise at 64 kb/s (test_encode_gpu.test_starved_bit_rate_is_survivable): no offset fits, every search fails;
    the frames keep their header and the search state its start value"""
    pcm = np.stack([H.gen_pcm(F, 6, seed=880 + s, kind="noise") for s in range(3)])
    for pack in (0, 1, 2):
        try:
            base = four_runs(engine, lambda run: _encode(engine, pcm, run, rate=64000, pack=pack))
        finally:
            _restore(engine)
        assert (base["frames"][:, :, 0] == 0x0b).all() and (base["frames"][:, :, 1] == 0x77).all() and (base["csnr"] == 40).all()


def _audits(engine, pcm, want, label, acmod, lfeon, fired, **kw):
    """the filled runs' frames: a clean decode, then - with the stage taps of one more call that must give the same bytes - the
    mantissa audit and the bit-budget audit"""
    S = pcm.shape[0]
    T.decodes_cleanly(want, acmod, lfeon, engine)
    engine.fill_workspaces(OTHER_FILL)
    frames, t = T.encode(engine, pcm, taps=True, **kw)
    assert np.array_equal(frames, want), "the call with stage taps gives other bytes"
    rep = MA.Report()

    def rows(s, f, P):
        cpl = None
        if P.blocks[0].cplinu:
            cpl = C.coupling_rows(t["mdct"][s, f], t["exp_samples"][s, f], P.nfchans, P.blocks[0].cplbegf)
        return MA.frame_rows(t["mdct"][s, f], t["exp_samples"][s, f], P.nfchans, P.lfeon, cpl)

    MA.audit_mantissas(rep, frames, rows, None, label)
    rep.finish(label)
    coded = rep.n["compared"] + rep.n["left_out"]
    assert rep.n["compared"] > 0 and rep.n["left_out"] <= 0.01 * coded, rep.n
    for k in fired:
        assert rep.n[k] > 0, (k, rep.n)
    brep = B.Report()
    B.audit(brep, frames, t, np.full(S, 40), label)
    brep.finish(label)


# name: (content, the tools, (acmod, lfeon), the audit's counters that show the tool fired)
TOOL_CASES = {
    "block switching": (lambda: T.pcm("attack", 3, 2, 6, seed=9500), dict(bsw=1), (7, 1), ("short_blocks",)),
    "rematrixing": (lambda: T.stereo("nearmono", 3, 2, seed=9510), dict(remat=1), (2, 0), ("remat_bands",)),
    "coupling 2 ch": (lambda: T.content("music", 2, 3, 2, seed=9520), dict(cpl=(1, 2)), (2, 0), ("coupled", "cpl_rows")),
    "coupling 6 ch": (lambda: T.content("music", 6, 3, 2, seed=9530), dict(cpl=(1, 2)), (7, 1), ("coupled", "cpl_rows")),
    "coupling + rematrixing": (lambda: T.stereo("music_nearmono", 3, 2, seed=9540), dict(cpl=(1, 2), remat=1), (2, 0), ("coupled", "remat_bands")),
    "bandwidth 1": (lambda: T.content("music", 6, 3, 2, seed=9550), dict(bw=(1, 30)), (7, 1), ("reduced_bw",)),
    "bandwidth 2": (lambda: T.content("music", 6, 3, 2, seed=9560), dict(bw=(2, 0), rate=224000), (7, 1), ("reduced_bw",)),
    "exponent strategy": (lambda: B.matrix_content(6, 1), dict(xs=1, rate=320000), (7, 1), ()),
    "DRC": (lambda: T.programme(6, seed=9570)[:, :8 * 1536], dict(md=B.META, drc=1), (7, 1), ("dynrng",)),
    "2/0+LFE rematrixing": (lambda: T.with_lfe(T.content("music", 2, 2, 3, seed=41), 43), dict(layout=(1, 2, 1), remat=1, rate=192000), (2, 1), ("remat_bands",)),
    "dual mono": (lambda: T.tones(0, 0, 2, 3, seed=5), dict(layout=(1, 0, 0), rate=256000, chmap=(0, 1)), (0, 0), ()),
}


@pytest.mark.parametrize("name", list(TOOL_CASES))
def test_encode_tool(engine, name):
    """each tool alone on the content that makes it fire (ws_bsw, ws_remat, ws_cpl, ws_cplr, ws_drc, the extra LFE-row launch)"""
    content, kw, (acmod, lfeon), fired = TOOL_CASES[name]
    pcm = content()
    drc = bool(kw.get("drc"))
    try:
        base = four_runs(engine, lambda run: _encode(engine, pcm, run, drc_state=drc, **kw))
        _audits(engine, pcm, base["frames"], name, acmod, lfeon, fired, **kw)
        # (the two tools the audit has no counter for)
        if name == "exponent strategy":
            _, t1 = T.encode(engine, pcm, taps=True, **kw)
            _, t0 = T.encode(engine, pcm, taps=True, **dict(kw, xs=0))
            assert not np.array_equal(t1["exp_strategy"], t0["exp_strategy"]), "the strategies are the reference rule's"
        if name == "dual mono":
            heads = [A.parse_frame(f, nblocks=0) for f in base["frames"].reshape(-1, base["frames"].shape[2])]
            assert all(P.acmod == 0 and "dialnorm2" in P.fields for P in heads)
    finally:
        _restore(engine)


@pytest.mark.parametrize("what", ["metadata words", "dynrng words"])
def test_encode_per_frame_arrays(engine, what):
    """a metadata word per frame; dynrng / compr words per frame (the packers' MD and DW instantiations), 5.1 and both packers"""
    from tests.test_bsi_gpu import _random_words, _words_tensor
    from tests.test_dynrng_source_gpu import _random_arrays, _tensors
    S, F = 3, 2
    pcm = T.content("music", 6, S, F, seed=9600)
    words = _random_words(np.random.default_rng(17), S, F)

    def configure():
        if what == "metadata words":
            engine.set_encode_metadata_frames(_words_tensor(words))
        else:
            engine.set_encode_dynrng_frames(*_tensors(*_random_arrays(np.random.default_rng(23), S, F)))

    try:
        for pack in (1, 2):
            base = four_runs(engine, lambda run: _encode(engine, pcm, run, pack=pack), configure)
            _audits(engine, pcm, base["frames"], "%s, pack %d" % (what, pack), 7, 1, ("dynrng",) if what == "dynrng words" else (), pack=pack)
            if what == "metadata words":
                for s_ in range(S):
                    for f in range(F):
                        want = BM.coded_fields(int(words[s_, f]), 7)
                        got = BM.parse_head(base["frames"][s_, f]).fields
                        assert {k: got[k] for k in want} == want, (s_, f)
                assert len({BM.parse_head(fr).fields["dialnorm"] for fr in base["frames"].reshape(S * F, -1)}) > 2
    finally:
        _restore(engine)


@pytest.mark.parametrize("nch", [2, 6])
def test_encode_all_tools(engine, nch):
    """everything on at once, as one call of three frames a stream and as a call of one-frame streams (other search and packer
    kernels); the first frames of new streams are the same bytes either way"""
    names = B.tool_sets(nch)[-1]
    kw = dict(B.settings(names), rate=B.matrix_rate(nch, 0, names))
    pcm = B.matrix_content(nch)
    acmod, lfeon = T.layout_of(nch)
    fired = ("short_blocks", "coupled", "reduced_bw", "dynrng") + (("remat_bands",) if nch == 2 else ())
    try:
        three = four_runs(engine, lambda run: _encode(engine, pcm, run, drc_state=True, **kw))
        one = four_runs(engine, lambda run: _encode(engine, pcm[:, :1536], run, drc_state=True, **kw))
        assert np.array_equal(one["frames"][:, 0], three["frames"][:, 0])
        _audits(engine, pcm, three["frames"], "%d ch, all tools" % nch, acmod, lfeon, fired, **kw)
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# transcode

def _tc_state(engine, src, rate, dynrng, flags):
    """descriptors and new streams' state of a transcode of 5.1 src [S][F][fb] to output `flags`"""
    import torch
    pkg = H.pkg()
    S, F, fb = src.shape
    dec = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0, dynrng=dynrng, acmod=7, lfeon=1, frame_bytes=fb)
    n, oflags = engine.decode_planes(dec)
    enc = pkg.EncodeDesc(48000, rate, n)
    st = dict(delay=torch.zeros((S, n, 128), dtype=torch.float32, device="cuda"),
              lfsr=(torch.arange(S, dtype=torch.int32) * 5 + 1).to(torch.int16).cuda(),
              last=torch.zeros((S, n, 256), dtype=torch.int16, device="cuda"),
              csnr=torch.full((S,), 40, dtype=torch.int32, device="cuda"),
              mix_pending=torch.zeros((S, n, 128), dtype=torch.float32, device="cuda"),
              mix_flags=torch.zeros((S, 6), dtype=torch.int32, device="cuda"))
    return dec, enc, n, oflags, H.CHMAP6 if n == 6 else tuple(range(n)), st


def _tc_result(out, ofb, status, st, mix):
    res = dict(frames=np.ascontiguousarray(_host(out)[:, :, :ofb]), status=_host(status))
    res.update({k: _host(v) for k, v in st.items() if mix or not k.startswith("mix_")})
    return res


def _transcode(engine, src, run, rate=448000, dynrng=1, flags=7 | 16, mix=False):
    """5.1 src [S][F][fb] -> frames [:frame_bytes], status and the four state arrays (mix: under ac3mi_set_mix_state, its two
    arrays as well)"""
    import torch
    S, F, fb = src.shape
    dec, enc, n, _, chmap, st = _tc_state(engine, src, rate, dynrng, flags)
    ofb = enc.frame_bytes()
    out = _pattern((S, F, (ofb + 3) & ~3), torch.uint8, run)
    status = torch.zeros((S, F), dtype=torch.int32, device="cuda")
    try:
        if mix:
            engine.set_mix_state(st["mix_pending"], st["mix_flags"])
        engine.transcode_batch(dec, enc, torch.from_numpy(_pad(src)).cuda(), st["delay"], st["lfsr"], chmap, st["last"], st["csnr"],
                               out=out, status=status)
        engine.sync()
    finally:
        if mix:
            engine.set_mix_state(None, None)
    return _tc_result(out, ofb, status, st, mix)


def _three_calls(engine, src, rate=448000, dynrng=1, words=None, codes=None, compr=None, flags=7 | 16, mix=False):
    """decode (level 1, bias 384) + convert + encode on the same context, its workspaces filled with another byte first; the
    per-frame words a source mode resolves are handed to the encode call as arrays"""
    import torch
    from tests.test_bsi_gpu import _words_tensor
    from tests.test_dynrng_source_gpu import _tensors
    S, F, fb = src.shape
    dec, enc, n, oflags, chmap, st = _tc_state(engine, src, rate, dynrng, flags)
    ofb = enc.frame_bytes()
    engine.fill_workspaces(OTHER_FILL)
    try:
        if mix:
            engine.set_mix_state(st["mix_pending"], st["mix_flags"])
        pcm, status = engine.decode_batch(dec, torch.from_numpy(_pad(src)).cuda(), st["delay"], st["lfsr"])
        engine.sync()
    finally:
        if mix:
            engine.set_mix_state(None, None)
    s16 = torch.empty((S * F * 6, 256, n), dtype=torch.int16, device="cuda")
    engine._check(engine.lib.ac3mi_convert_s16_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(pcm.data_ptr()),
                                                     ctypes.c_void_p(s16.data_ptr()), oflags, ctypes.c_size_t(S * F * 6)))
    try:
        if words is not None:
            engine.set_encode_metadata_frames(_words_tensor(words))
        if codes is not None:
            engine.set_encode_dynrng_frames(*_tensors(codes, compr))
        out = engine.encode_batch(enc, s16.view(S, F, 1536, n), chmap, st["last"], st["csnr"])
        engine.sync()
    finally:
        engine.set_encode_metadata_frames(None)
        engine.set_encode_dynrng_frames(None, None)
    return _tc_result(out, ofb, status, st, mix)


_TC = {}


def _tc_source(S, F):
    """the oracle encoder's 5.1 frames; one frame with a broken sync word when the batch has room for it"""
    if (S, F) not in _TC:
        src = np.stack([H.orc_encode(H.gen_pcm(F, 6, seed=9700 + s, kind=KINDS[s % 7])) for s in range(S)])
        src[S - 2, F - 1, 0] ^= 0x40
        _TC[(S, F)] = src
    return _TC[(S, F)]


@pytest.mark.parametrize("S,F,tile,mode", [(9, 1, 0, 0), (9, 1, 0, 6), (4, 3, 0, 0), (4, 3, 0, 4), (4, 3, 0, 5), (9, 1, 3, 6)])
def test_transcode(engine, S, F, tile, mode):
    """nine one-frame 5.1 streams (under decode mode 6 the fixed-shape parse and mantissa + transform kernels, under auto one
    workgroup per stream; the fixed-shape encoder either way), 4 x 3 (the generic kernels: auto, parse kernel per stream and per
    frame), and the nine in three tiles of whole streams, where tile 2 runs on what tile 1 left as well; one frame of each batch
    is refused"""
    src = _tc_source(S, F)
    def configure():
        engine.set_decode_mode(mode)
        if tile:
            engine.set_tile_frames(tile)

    try:
        base = four_runs(engine, lambda run: _transcode(engine, src, run), configure)
    finally:
        _restore(engine)
    assert base["status"][S - 2, F - 1] & 0x100 and np.count_nonzero(base["status"] & 0x1ff) == 1
    same(base, _three_calls(engine, src), "transcode against decode + convert + encode")


@pytest.mark.parametrize("flags,rate", [(2, 192000), (1, 96000)])
@pytest.mark.parametrize("mode", [0, 4, 5])
def test_transcode_downmix_with_mix_state(engine, mode, flags, rate):
    """5.1 to 2/0 and to mono under ac3mi_set_mix_state, 6 x 3 packer frames whose surround level goes to zero and back, a
    refused frame, a failed block and a REUSE0 frame among them: the transcode's own "level 0" flags behind the block-switch
    flags in ws_blksw, written by its front end and read by its s16 transform"""
    src, first_bad = _decode_batch(7, 1, 6, 3, flip=True)
    clean = int((first_bad == 3).sum())
    try:
        base = four_runs(engine, lambda run: _transcode(engine, src, run, rate, flags=flags, mix=True), lambda: engine.set_decode_mode(mode))
        assert base["status"][clean, 1] & 0x100 and (base["status"][:clean] & 0x1ff).max() == 0 and base["mix_flags"][:clean].any()
        same(base, _three_calls(engine, src, rate, flags=flags, mix=True), "transcode against decode + convert + encode")
        linear = _transcode(engine, src, 0, rate, flags=flags)
        assert not np.array_equal(linear["frames"][:clean], base["frames"][:clean]), "the level flags decided nothing"
        T.decodes_cleanly(base["frames"][:clean], flags, 0)
    finally:
        _restore(engine)


@pytest.mark.parametrize("mode", [0, 4])
@pytest.mark.parametrize("S,F", [(9, 1), (4, 3)])
def test_transcode_source_modes(engine, S, F, mode):
    """ac3mi_set_encode_metadata_source 1 and ac3mi_set_encode_drc_source 1 under ac3mi_set_decode_crc 2, on sources that
    carry metadata, dynrng and compr words - one frame refused, one concealed for its CRC: ws_bsi, ws_dyn, ws_crc, and
    "damaged frames carry none".  Against the three calls, the encoder given the models' words as arrays."""
    from tests.test_dynrng_source_gpu import _random_arrays, _tensors
    ctx = dict(dialnorm=20, bsmod=3, cmixlev=2, surmixlev=0, dsurmod=1, copyrightb=1, origbs=0)
    pcm = T.content("music", 6, S, F, seed=9800)
    codes, compr = _random_arrays(np.random.default_rng(29), S, F)
    try:
        engine.set_encode_dynrng_frames(*_tensors(codes, compr))
        src = T.encode(engine, pcm, rate=448000, md=dict(dialnorm=9, cmixlev=0, surmixlev=2, bsmod=5))
        engine.set_encode_dynrng_frames(None, None)
        fb = src.shape[2]
        src[1, 0, :2] = 0                                  # refused
        src[S - 1, F - 1, fb - 40] ^= 0x08                  # a mantissa bit: crc2 fails, concealed

        def configure():
            engine.set_decode_mode(mode)
            engine.set_decode_crc(2)
            engine.set_encode_metadata(**ctx)
            engine.set_encode_metadata_source(1)
            engine.set_encode_drc_source(1)

        base = four_runs(engine, lambda run: _transcode(engine, src, run, dynrng=0), configure)
        st = base["status"].astype(np.uint32)
        assert (st[1, 0] & 0x1ff) == 0x13f and (st[S - 1, F - 1] & 0x9ff) == 0x93f and np.count_nonzero(st & 0x1ff) == 2
        engine.set_encode_metadata_source(0)
        engine.set_encode_drc_source(0)
        want_codes, want_compr = D.effective(src, st, -1)
        assert not want_codes[1, 0].any() and not want_codes[S - 1, F - 1].any() and D.sends(want_codes).sum() > S * F
        ctx_word = BM.pack_word(**ctx)
        words = np.array([[BM.followed_word(None if st[s, f] & 0x100 else BM.parse_head(src[s, f]), 7, ctx_word) for f in range(F)]
                          for s in range(S)], np.int64)
        assert len(set(words.ravel().tolist())) == 2
        D.check_frames(base["frames"], want_codes, want_compr, 7)
        same(base, _three_calls(engine, src, dynrng=0, words=words, codes=want_codes, compr=want_compr),
             "source modes against decode + convert + encode with the models' arrays")
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# the control

def test_control_exponent_tap_leftovers_are_not_the_workspaces(engine):
    """tests/test_decode_gpu.py notes that the exponent tap of the split front end also dumps rows and bins the frame does not
    define - leftovers of earlier frames under the per-stream parse kernel (mode 4), zeros under the per-frame one (mode 5).
    Those cells are the parse kernel's LDS rows, not a workspace: under every fill they are the same, the two front ends differ
    in them and nowhere else, and the defined cells (every one shapes the coefficient planes, which are compared too) agree."""
    import torch
    pkg = H.pkg()
    S, F = 6, 3
    frames = np.stack([packer.make_stream(4000 + s, F, 2, 0, fscod=0, bsid=8, frmsizecod=30) for s in range(S)])
    fb = frames.shape[2]
    desc = pkg.DecodeDesc(flags=2, level=1.0, bias=0.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    d_frames = torch.from_numpy(_pad(frames)).cuda()

    def call(run):
        delay = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
        lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
        pcm, status, taps = engine.decode_batch(desc, d_frames, delay, lfsr, taps=True)
        engine.sync()
        return dict(pcm=_host(pcm), status=_host(status), exp=_host(taps["exp"]), bap=_host(taps["bap"]), coef=_host(taps["coef"]))

    res = {}
    try:
        for mode in (4, 5):
            res[mode] = four_runs(engine, call, lambda: engine.set_decode_mode(mode))
    finally:
        _restore(engine)
    a, b = res[4], res[5]
    assert (a["status"] & 0x3ff).max() == 0
    for k in ("pcm", "status", "coef"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # the cells a frame defines: rows 0-1 over [0, endmant) and the coupling row over its range, read from the bitstream
    defined = np.zeros(a["exp"].shape, bool)
    for s in range(S):
        for f in range(F):
            P = A.parse_frame(frames[s, f])
            for blk, Bk in enumerate(P.blocks):
                for r, (lo, hi) in Bk.rng.items():
                    defined[s, f, blk, 6 if r == A.CPL else r, lo:hi] = True
    assert np.array_equal(a["exp"][defined], b["exp"][defined])
    differ = a["exp"] != b["exp"]
    print("exponent tap: %d defined cells, %d undefined cells differ between parse kernel per stream and per frame" % (
        int(defined.sum()), int(differ.sum())))
    assert differ.any() and not (differ & defined).any()
    assert not differ[:, 0].any()                            # a stream's first frame starts from cleared rows in both
