"""GPU: sources that decode beyond full scale.  The reference encoder's 5.1 / 384 kb/s frames of full-scale squares, DC and
noise (tests/_tools.corner) decode to samples outside +-1.0 - 3 % to 32 % of them, asserted below on the restatement's
output - so the fused s16 paths (ac3mi_decode_s16_batch through decode_mx.hip and the fixed-shape instantiations,
ac3mi_transcode_batch) must saturate exactly as ac3mi_convert_s16_batch and the reference's converter do.  The other
transcode and fixed-shape tests use tones, music, bursts and noise at moderate levels; saturation was held to liba52 on
packer streams only.

* ac3mi_decode_s16_batch under the 5.1, stereo and mono requests: every decode mode, fixed shape on and off, gives the same
  bytes, status, delay and lfsr, and the result is the restatement's through the reference's converter
  (_decode_matrix.held_to_liba52); both rails appear in the output;
* ac3mi_transcode_batch equals ac3mi_decode_batch + ac3mi_convert_s16_batch + ac3mi_encode_batch byte for byte and state for
  state, fixed shape on and off, with no tool and with every tool;
* the second generation passes the budget audit's items 1 to 3 and decodes cleanly.
Nine one-frame streams (the fixed shape) and five two-frame streams, the four kinds repeated."""
import contextlib

import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import _tools as T
from tests.test_frame_budget_gpu import META, RATES, Report, audit
from tests.test_transcode_gpu import _three_calls

pytestmark = pytest.mark.gpu

KINDS = ("rails", "rails_identical", "dc", "noise")
CASE = (7, 1, 0, 8, 30)                         # 5.1, 48 kHz, 1 536-byte frames (_decode_matrix.decode reads the layout only)
SHAPES = {"one-frame": (9, 1), "two-frame": (5, 2)}
_SRC = {}


def sources(shape):
    """[S][F][1536] u8: the oracle's frames of KINDS (seed 900 + the kind's index in the corner batch), the kinds repeated.
    A one-frame stream is the second frame of its source: full scale from its first sample to its last."""
    if not _SRC:
        two = [H.orc_encode(T.corner(k, 6, 2, 900 + T.CORNER_KINDS.index(k))) for k in KINDS]
        for k, fr in zip(KINDS, two):
            pcm, errs, _ = H.orc_decode(fr, 7 | 16, 1.0, 384.0)
            steps = (pcm.astype(np.float64) - 384.0) * 32768.0
            hot = float(((steps > 32767) | (steps < -32768)).mean())
            print("%s: %.1f %% of the restatement's 5.1 decode lies outside the s16 range" % (k, 100 * hot))
            assert errs == 0 and hot > 0.01, (k, hot)
        _SRC["two-frame"] = np.stack([two[s % 4] for s in range(5)])
        _SRC["one-frame"] = np.stack([two[s % 4][1:] for s in range(9)])
        for v in _SRC.values():
            v.setflags(write=False)
    return _SRC[shape]


def _restore(engine):
    import os
    engine.set_decode_mode(int(os.environ.get("AC3MI_DECODE_MODE", "0")))
    engine.set_fixed_shape(1)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_decode_s16_saturates_like_the_reference(engine, shape):
    frames = sources(shape)
    whole = np.full(frames.shape[0], frames.shape[1])
    try:
        for req in (7 | 16, 2, 1):
            engine.set_decode_mode(1)
            engine.set_fixed_shape(1)
            base = M.decode(engine, frames, CASE, req, s16=True)
            assert (base["status"] & 0x1ff).max() == 0
            fig = M.held_to_liba52(base, M.liba52(("hot", shape), frames, req, 384.0), whole, s16=True)
            lo, hi = (base["pcm"] == -32768).mean(), (base["pcm"] == 32767).mean()
            print("%s request %d: s16 largest step %d, RMS %.3g of level; %.2f %% of the samples at -32768, %.2f %% at 32767" % (
                shape, req, fig[0], fig[1], 100 * lo, 100 * hi))
            assert lo > 0 and hi > 0
            for mode in (0, 1, 3, 4, 5, 6):
                for fixed in (1, 0):
                    engine.set_decode_mode(mode)
                    engine.set_fixed_shape(fixed)
                    M.same(M.decode(engine, frames, CASE, req, s16=True), base, "request %d: mode %d, fixed shape %d, against mode 1" % (req, mode, fixed))
    finally:
        _restore(engine)


@contextlib.contextmanager
def all_tools(engine, state):
    """every encoder tool that applies to 5.1 (and rematrixing, which does not), DRC on `state`"""
    engine.set_encode_block_switch(1)
    engine.set_encode_rematrix(1)
    engine.set_encode_coupling(1, 2)
    engine.set_encode_bandwidth(2, 0)
    engine.set_encode_exp_strategy(1)
    engine.set_encode_metadata(**META)
    engine.set_encode_drc(1, state)
    try:
        yield
    finally:
        engine.set_encode_block_switch(0)
        engine.set_encode_rematrix(0)
        engine.set_encode_coupling(0, 0)
        engine.set_encode_bandwidth(0)
        engine.set_encode_exp_strategy(0)
        engine.set_encode_metadata()
        engine.set_encode_drc(0)


@pytest.mark.parametrize("tools", [0, 1], ids=["mode0", "all-tools"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_transcode_equals_the_three_calls(engine, shape, tools):
    import torch
    pkg = H.pkg()
    frames = sources(shape)
    S, F, fb = frames.shape
    frames_t = torch.from_numpy(frames.copy()).cuda()
    dec = pkg.DecodeDesc(flags=7 | 16 | 32, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=fb)
    enc = pkg.EncodeDesc(48000, RATES[6][1], 6)
    names = "frames status delay lfsr last_samples csnroffst drc_state".split()

    def state():
        return torch.zeros((S,), dtype=torch.int32, device="cuda")

    def on(st):
        return all_tools(engine, st) if tools else contextlib.nullcontext()

    def transcode():
        delay = torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda")
        lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
        last = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        st = state()
        with on(st):
            out, status = engine.transcode_batch(dec, enc, frames_t, delay, lfsr, H.CHMAP6, last, csnr)
            engine.sync()
        return [np.ascontiguousarray(t.cpu().numpy()) for t in (out, status, delay, lfsr, last, csnr, st)]

    try:
        st = state()
        with on(st):
            want = [np.ascontiguousarray(t.cpu().numpy()) for t in _three_calls(engine, pkg, frames_t, dec, enc, H.CHMAP6, S, F, 6) + (st,)]
        for fixed in (1, 0):
            engine.set_fixed_shape(fixed)
            got = transcode()
            for n, g, w in zip(names, got, want):
                assert g.shape == w.shape and g.tobytes() == w.tobytes(), "fixed shape %d: `%s` differs from the three calls'" % (fixed, n)
    finally:
        engine.set_fixed_shape(1)
    assert int((want[1] & 0x1ff).max()) == 0
    # the second generation
    out = want[0][:, :, :enc.frame_bytes()]
    title = "second generation of hot sources, %s, %s" % (shape, "all tools" if tools else "mode 0")
    rep = Report()
    rep.n["configs"] += 1
    audit(rep, out, None, np.full(S, 40), title)
    rep.finish(title)
    assert rep.n["frames"] == S * F
    if tools:
        assert rep.n["dynrng"] > 0 and rep.n["coupled"] > 0, rep.n
    T.decodes_cleanly(out, 7, 1, engine=engine)
