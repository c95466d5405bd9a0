"""GPU: enc_mdct_kernel's block loop on the inputs where its branch-free rules (csrc/mdct_rule.h, wave_ops.h quad_trade2) can
go wrong and the seeded tests/_harness.gen_pcm kinds do not reach:

  zeros      every coefficient 0: the zero's exponent 24 with no case of its own
  neg        constant -32768
  sq_dc      a full-scale square (32767 / -32768) of one period per transform length: all energy next to DC, v = 0
  sq_ny      the same at the Nyquist period (the rails alternate every sample): the largest coefficients there are
  impulse    a single +1 or -1 per block over silence: v = 14, coefficients that exponent 24 zeroes
  pm1        +-1 noise
  onset      silence, then the full-scale square: the history crosses the corner (in mid-frame, and - stream `quiet_loud` of the
             5.1 batch - a whole frame of silence before a frame of full scale)

5.1 at 384 kb/s, 8 streams x 2 frames: the stage taps (mdct, exp_samples, encoded_exp, exp_strategy) and the bytes equal the
ac3enc restatement's.  The same PCM as 16 one-frame streams takes the fixed-shape kernel (and, with the fixed shape off, the
generic one): the same bytes.  Every other enc_mdct_kernel instantiation that tests/variant_matrix.py lists gets the corner
kinds on 2 streams x 2 frames, is seen in the launch log, and is held to the model the matrix holds it to (the restatement's
bytes with every tool off; else the CRCs, a clean decode, the budget audit and the mantissa audit), rematrixing also to its
row model and block switching to its decisions."""
import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import variant_matrix as V
from tests import test_variant_matrix_gpu as M
from tests.test_block_switch_gpu import _check_decisions
from tests.test_encode_gpu import _gpu, _oracle
from tests.test_rematrix_gpu import _check_rows

pytestmark = pytest.mark.gpu

KINDS = ("zeros", "neg", "sq_dc", "sq_ny", "impulse", "pm1", "onset")


def segment(kind, rng, flip=False):
    """one frame (1536 samples) of one channel"""
    t = np.arange(1536)
    hi, lo = (-32768, 32767) if flip else (32767, -32768)
    if kind == "zeros":
        x = np.zeros(1536)
    elif kind == "neg":
        x = np.full(1536, -32768)
    elif kind == "sq_dc":
        x = np.where((t // 256) % 2 == 0, hi, lo)
    elif kind == "sq_ny":
        x = np.where(t % 2 == 0, hi, lo)
    elif kind == "impulse":
        x = np.zeros(1536)
        x[256 * np.arange(6) + rng.integers(0, 256, 6)] = rng.choice([-1, 1], 6)
    elif kind == "pm1":
        x = rng.choice([-1, 1], 1536)
    elif kind == "onset":
        x = np.where(t < 700, 0, np.where((t // 5) % 2 == 0, hi, lo))
    else:
        raise ValueError(kind)
    return x.astype(np.int16)


def corner_streams(S, F, nch, seed):
    """[S][F * 1536][nch]: cell (stream, frame, channel) holds kind (nch (F s + f) + c) mod 7, odd channels with the rails swapped"""
    rng = np.random.default_rng(seed)
    out = np.zeros((S, F * 1536, nch), np.int16)
    for s in range(S):
        for f in range(F):
            for c in range(nch):
                out[s, 1536 * f:1536 * (f + 1), c] = segment(KINDS[(nch * (F * s + f) + c) % 7], rng, flip=bool(c & 1))
    return out


def batch_5_1():
    """[8][2 * 1536][6]: streams 0 .. 6 hold one kind each in every channel and both frames (odd channels with the rails
    swapped), stream 7 (`quiet_loud`) a frame of silence, then a frame of full scale: sq_ny in the even channels, sq_dc in the odd"""
    rng = np.random.default_rng(1201)
    out = np.zeros((8, 2 * 1536, 6), np.int16)
    for s, kind in enumerate(KINDS):
        for f in range(2):
            for c in range(6):
                out[s, 1536 * f:1536 * (f + 1), c] = segment(kind, rng, flip=bool(c & 1))
    for c in range(6):
        out[7, 1536:, c] = segment(("sq_ny", "sq_dc")[c & 1], rng, flip=bool(c & 2))
    return out


_REF = {}


def reference_5_1():
    """the batch and the restatement's frames and taps, computed once"""
    if not _REF:
        pcm = batch_5_1()
        want, wt = _oracle(list(pcm), 6, 384000)
        for a in (pcm, want) + tuple(wt.values()):
            a.setflags(write=False)
        _REF.update(pcm=pcm, want=want, wt=wt)
    return _REF["pcm"], _REF["want"], _REF["wt"]


def test_stages_and_bytes_equal_the_oracle(engine):
    pcm, want, wt = reference_5_1()
    # the corners are reached: rows of exponent 24 throughout, block shifts at both ends (v = 0 and v >= 14)
    assert (wt["exponent"][0, :, :, :5, :223] == 24).all() and wt["shift"].min() == -9 and wt["shift"].max() >= 5
    got, gt = _gpu(engine, list(pcm), 6, 384000)
    assert np.array_equal(gt["mdct"], wt["mdct"]), "mdct_coef"
    assert np.array_equal(gt["exp_samples"], wt["shift"]), "exp_samples"
    assert np.array_equal(gt["exp_strategy"], wt["strat"]), "exp_strategy"
    for ch, n in [(0, 223), (1, 223), (2, 223), (3, 223), (4, 223), (5, 7)]:
        assert np.array_equal(gt["encoded_exp"][:, :, :, ch, :n], wt["encoded_exp"][:, :, :, ch, :n]), "encoded_exp %d" % ch
    assert np.array_equal(got, want), "bitstream differs in %d bytes" % int((got != want).sum())


def test_fixed_shape_path_equals_the_generic_one_and_the_oracle(engine):
    """16 one-frame streams: the eight first frames from a new stream's state, the eight second frames from the state the
    first frames leave (history and search state, taken from a generic call on the first frames)"""
    import torch
    pcm, want, _ = reference_5_1()
    desc = H.pkg().EncodeDesc(48000, 384000, 6)
    x = torch.from_numpy(pcm.reshape(8, 2, 1536, 6).copy()).cuda()
    last0 = torch.zeros((8, 6, 256), dtype=torch.int16, device="cuda")
    csnr0 = torch.full((8,), 40, dtype=torch.int32, device="cuda")
    x16 = torch.cat([x[:, 0:1], x[:, 1:2]], 0).contiguous()
    out = {}
    try:
        engine.set_fixed_shape(0)
        engine.encode_batch(desc, x[:, 0:1].contiguous(), H.CHMAP6, last0, csnr0)
        engine.sync()
        for fixed in (1, 0):
            engine.set_fixed_shape(fixed)
            last = torch.cat([torch.zeros_like(last0), last0], 0).contiguous()
            csnr = torch.cat([torch.full_like(csnr0, 40), csnr0], 0).contiguous()
            with V.tap(engine) as names:
                frames = engine.encode_batch(desc, x16, H.CHMAP6, last, csnr)
                engine.sync()
            assert (V.mdct(fx=1) in names) == bool(fixed) and (V.mdct() in names) == (not fixed), names
            out[fixed] = frames.cpu().numpy()[:, 0, :want.shape[2]]
    finally:
        engine.set_fixed_shape(1)
    assert np.array_equal(out[1], out[0]), "the fixed shape's bytes are not the generic kernels'"
    assert np.array_equal(out[1][:8], want[:, 0]) and np.array_equal(out[1][8:], want[:, 1]), "not the oracle's bytes"


def _variant_cases():
    """the first recipe of the matrix that launches each enc_mdct_kernel instantiation, but the fixed shape's (above)"""
    seen, out = {V.mdct(fx=1)}, []
    for r in V.RECIPES:
        if r.kind != "encode" or r.words is not None:
            continue
        new = [k for k in r.chain if k.startswith("enc_mdct_kernel<") and k not in seen]
        if new:
            seen.update(new)
            out.append((r, new))
    return out


VARIANTS = _variant_cases()


def test_every_listed_variant_has_a_case():
    listed = {k for k in V.word_table().values() if k.startswith("enc_mdct_kernel<")}
    assert {k for _, new in VARIANTS for k in new} | {V.mdct(fx=1)} == listed


@pytest.mark.parametrize("r,new", VARIANTS, ids=[V.recipe_id(r) for r, _ in VARIANTS])
def test_other_variants_on_the_corners(engine, r, new):
    S, F = 2, 2
    rc = V.Enc(r.name + ", corners", r.chain, nch=r.nch, layout=r.layout, shape=(S, F), tools=r.tools, content="mdct corners", ref=r.ref)
    pcm = corner_streams(S, F, r.nch, 1300 + r.nch)
    M._PCM[(rc.content, rc.nch, rc.layout, S, F)] = (pcm, np.zeros((S, r.nch, 256), np.int16))       # new streams: the oracle's state
    res = M._encode(engine, rc, rc.tools, None)
    assert all(k in res["logs"][0] for k in new), "launched %r" % res["logs"]
    M._reference(engine, rc, rc.tools, None, res)
    if r.nch == 2 and rc.tools.get("remat") and not rc.tools.get("bw"):
        _check_rows(engine, pcm, bsw=rc.tools.get("bsw", 0))
    if r.nch == 2 and rc.tools.get("bsw") and not rc.tools.get("bw"):
        _check_decisions(engine, T.encode(engine, pcm, bsw=1), pcm, 2)
