"""GPU: every kernel instantiation of csrc/launch_rule.h, launched and held to a reference - one case per recipe of
tests/variant_matrix.py.  The rule chooses between kernels that return the same bytes, so a byte test cannot see which one
ran; ac3mi_debug_launch_log can.  Every case asserts

(a) the log: the kernels the call launched are the recipe's chain, in order, and nothing else;
(b) the feature: the output shows what the variant's own code is for (a coupled frame, a short block, a set rematrixing
    flag, a reduced bandwidth, strategies other than the reference's, dynrng words that change inside a frame, two
    programmes, BSI fields other than the defaults, source frames that carry words), read with tests/ac3_syntax.py;
(c) the siblings: every other route the project defines to the same result - the fixed shape off, the other packer,
    bandwidth mode 1 at chbwcod 50 against mode 0, one call of three frames against three calls of one, a metadata array of
    default words against none, decode modes 3 - 6 against mode 1 - logs its own chain, other kernels, and returns the same
    frames or PCM, status and carried state (overlap tails, dither state, last_samples, csnroffst, the DRC state);
(d) a reference that is not the code under test: the decoder against the liba52 restatement at the bars of
    _decode_matrix.held_to_liba52; the encoder with every tool off against the ac3enc restatement, byte for byte; with a tool
    on, both CRCs and a clean decode by the restatement, the independent reader's bit-budget audit
    (tests/test_frame_budget_gpu.audit) and mantissa audit (tests/mantissa_audit.py), and for words from arrays or from a
    transcode's source the words in force per block as the reader finds them (tests/dynrng_model.check_frames).

The taps that the audits need change the route (a call with stage taps takes no fixed-shape front kernel or search), so
the audited call is one more call, with taps, whose frames must be the recipe's."""
import numpy as np
import pytest

from tests import _decode_matrix as DM
from tests import _harness as H
from tests import _tools as T
from tests import ac3_syntax as A
from tests import dynrng_model as D
from tests import mantissa_audit as MA
from tests import variant_matrix as V
from tests import test_frame_budget_gpu as B
from tests.test_bsi_gpu import _words_tensor
from tests.test_dynrng_source_gpu import _padded, _random_arrays, _source, _tensors, _transcode

pytestmark = pytest.mark.gpu

ENC = [r for r in V.RECIPES if r.kind == "encode"]
DEC = [r for r in V.RECIPES if r.kind == "decode"]
SRC = [r for r in V.RECIPES if r.kind == "transcode"]
STATE = ("frames", "last_samples", "csnroffst", "drc_state")


def _restore(engine):
    engine.set_encode_dynrng_frames(None, None)
    engine.set_encode_metadata_frames(None)
    engine.set_encode_drc_source(0)
    engine.set_decode_mode(0)
    engine.set_fixed_shape(1)
    engine.set_tile_frames(131072)


# ---------------------------------------------------------------------------------------------------------------------
# the encoder's calls

_PCM = {}


def _content(r):
    """(pcm [S][F * 1536][nch], last [S][nch][256] in coded channel order): "plain" starts new streams; every other kind is
    the second frame on of a stream in progress, whose first frame's tail is the history"""
    S, F = r.shape
    key = (r.content, r.nch, r.layout, S, F)
    if key not in _PCM:
        if r.content == "plain":
            full = np.stack([H.gen_pcm(F + 1, r.nch, seed=3 + s, kind=("tones", "music")[s % 2]) for s in range(S)])
            full[:, :1536] = 0
        elif r.content == "attack":
            full = T.stereo("attack", S, F + 1, seed=8100)
        else:
            full = T.content("music", 2 if r.nch == 3 else r.nch, S, F + 1, seed=8200 + r.nch)
            if r.content == "stepped":      # the level steps every two blocks, in every channel alike
                env = np.repeat(np.where((np.arange((F + 1) * 6) // 2) % 2 == 0, 1.0, 0.05), 256)
                full = np.round(full * env[None, :, None]).astype(np.int16)
            if r.nch == 3:
                full = T.with_lfe(full, 8300)
        chmap = list(range(r.nch)) if r.layout else list(T.chmap_of(r.nch)[:r.nch])
        last = np.ascontiguousarray(full[:, 1536 - 256:1536, chmap].transpose(0, 2, 1))
        _PCM[key] = (np.ascontiguousarray(full[:, 1536:]), last)
    return _PCM[key]


def _arrays(r):
    """the recipe's per-frame arrays: (dynrng codes [S][F][6][2], compr words [S][F][2]), default metadata words [S][F]"""
    S, F = r.shape
    codes, compr = _random_arrays(np.random.default_rng(41), S, F)
    return codes, compr, np.full((S, F), H.pkg().encode_metadata_word(), np.int64)


def _encode(engine, r, tools, words, fixed=1, split=False, taps=False, tile=None):
    """the recipe's call under `tools` and the words rule -> dict of host arrays (frames and the carried state), `logs` (the
    kernels of each call) and `taps`.  split: one call per frame, the state carried by the caller"""
    import torch
    pcm, last0 = _content(r)
    S, F = r.shape
    kw = {k: v for k, v in tools.items() if v is not None}
    kw["layout"] = (1,) + tuple(r.layout) if r.layout else (0,)
    chmap = tuple(range(r.nch)) if r.layout else T.chmap_of(r.nch)
    last = torch.from_numpy(last0.copy()).cuda()
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    state = torch.zeros((S,), dtype=torch.int32, device="cuda") if kw.get("drc") else None
    codes, compr, mdw = _arrays(r)
    logs, frames, tp = [], [], None
    try:
        engine.set_fixed_shape(fixed)
        if tile:
            engine.set_tile_frames(tile)
        for a, b in ([(f, f + 1) for f in range(F)] if split else [(0, F)]):
            if words == "dw":
                engine.set_encode_dynrng_frames(*_tensors(codes[:, a:b], compr[:, a:b]))
            elif words == "md_default":
                engine.set_encode_metadata_frames(_words_tensor(mdw[:, a:b]))
            with V.tap(engine) as names:
                got = T.encode(engine, pcm[:, a * 1536:b * 1536], rate=V.RATE[r.nch], chmap=chmap, last=last, csnr=csnr, state=state, taps=taps, **kw)
            logs.append(names)
            if taps:
                got, tp = got
            frames.append(got)
    finally:
        _restore(engine)
    return dict(frames=np.concatenate(frames, 1), last_samples=last.cpu().numpy(), csnroffst=csnr.cpu().numpy(),
                drc_state=state.cpu().numpy() if state is not None else np.zeros(0, np.int32), logs=logs, taps=tp)


def _same(got, want, what):
    for k in STATE:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), "%s: `%s` differs" % (what, k)


def _features(r, frames, pcm, plain_strategies):
    """(b): the output shows every feature the recipe names"""
    flat = frames.reshape(-1, frames.shape[-1])
    parsed = [A.parse_frame(fr) for fr in flat]
    blocks = [Bk for P in parsed for Bk in P.blocks]
    for tag in r.features:
        if tag == "CPL":
            assert any(Bk.cplinu and any(Bk.chincpl) for Bk in blocks), "no coupled frame"
        elif tag == "BSW":
            assert any(v for Bk in blocks for k, v in Bk.fields.items() if k.startswith("blksw")), "no short block"
        elif tag == "REMAT":
            assert any(v for Bk in blocks for k, v in Bk.fields.items() if k.startswith("rematflg")), "no rematrixing flag set"
        elif tag == "BW":
            cut = [v for Bk in blocks for k, v in Bk.fields.items() if k.startswith("chbwcod")]
            cut += [50 if Bk.cplendf >= 12 else 0 for Bk in blocks if Bk.cplinu]
            assert cut and min(cut) < 50, "no channel codes a reduced bandwidth"
        elif tag == "XS":
            mine = [repr(Bk.expstr) for Bk in blocks]
            assert mine != plain_strategies, "the strategies are the reference rule's"
        elif tag in ("DRC", "DW"):
            per_frame = [{Bk.fields["dynrng"] for Bk in P.blocks if Bk.fields["dynrnge"]} for P in parsed]
            assert any(len(w) >= 2 for w in per_frame), "no frame whose dynrng word changes inside it"
        elif tag == "DUAL":
            assert all(P.acmod == 0 for P in parsed) and not np.array_equal(pcm[..., 0], pcm[..., 1]), "not two programmes"
        elif tag == "MD":
            for P in parsed:
                got = {k: P.fields[k] for k in V.META if k in P.fields}
                assert got == {k: V.META[k] for k in got} and got["dialnorm"] != 31 and got["bsmod"] != 0, got
        else:
            raise AssertionError("unknown feature %s" % tag)
    return parsed


def _reference(engine, r, tools, words, res):
    """(d)"""
    frames = res["frames"]
    pcm, _ = _content(r)
    S, F = r.shape
    if r.ref == "oracle":
        chmap = tuple(range(r.nch)) if r.layout else T.chmap_of(r.nch)
        for s in range(S):
            want = H.orc_encode(pcm[s], r.nch, bitrate=V.RATE[r.nch], chmap=chmap)
            assert np.array_equal(frames[s], want), "stream %d is not the ac3enc restatement's" % s
        return
    t = _encode(engine, r, tools, words, taps=True)
    _same(t, res, "the call with stage taps")
    rep = B.Report()
    B.audit(rep, frames, t["taps"], np.full(S, 40), r.name)
    rep.finish(r.name)
    mrep = MA.Report()
    MA.audit_mantissas(mrep, frames, MA.tap_rows(t["taps"]), None, r.name)
    mrep.finish(r.name)
    coded = mrep.n["compared"] + mrep.n["left_out"]
    assert mrep.n["frames"] == S * F and mrep.n["compared"] > 0 and 100 * mrep.n["left_out"] <= coded, mrep.n
    assert mrep.n["cpl_rows"] == 6 * mrep.n["coupled"], mrep.n
    T.decodes_cleanly(frames, r.acmod, r.lfeon, engine)
    if words == "dw":
        codes, compr, _ = _arrays(r)
        nd, nc = D.check_frames(frames, codes, compr, r.acmod)
        assert nd > S * F and nc > 0


@pytest.mark.parametrize("r", ENC, ids=V.recipe_id)
def test_encoder_variant(engine, r):
    res = _encode(engine, r, r.tools, r.words)
    assert res["logs"] == [r.chain], "(a) launched %r" % res["logs"]
    assert res["frames"].any()
    # (c) before anything else is asked of the bytes: every sibling route, its own chain, the same bytes and state
    for s in r.siblings:
        other = _encode(engine, r, dict(r.tools, **s.tools), r.words if s.words == "keep" else s.words, fixed=s.fixed, split=s.split)
        assert other["logs"] == [s.chain] * len(other["logs"]) and s.chain != r.chain, "(c) %s launched %r" % (s.what, other["logs"])
        assert len(other["logs"]) == (r.shape[1] if s.split else 1)
        _same(other, res, "(c) " + s.what)
    # (b) and (d) on the call that shows the features: the recipe's own, or its feature call (the same chain)
    tools, words, shown = r.tools, r.words, res
    if r.feature_tools is not None:
        tools, words = r.feature_tools, r.words if r.feature_words == "keep" else r.feature_words
        shown = _encode(engine, r, tools, words)
        assert shown["logs"] == [r.chain], "(a) the feature call launched %r" % shown["logs"]
        assert not np.array_equal(shown["frames"], res["frames"])
    plain = None
    if "XS" in r.features:
        ref = _encode(engine, r, dict(tools, xs=None), words)["frames"]
        plain = [repr(Bk.expstr) for fr in ref.reshape(-1, ref.shape[-1]) for Bk in A.parse_frame(fr).blocks]
    _features(r, shown["frames"], _content(r)[0], plain)
    _reference(engine, r, tools, words, shown)
    if shown is not res and r.ref != "oracle":
        T.decodes_cleanly(res["frames"], r.acmod, r.lfeon, engine)


def test_tiled_call_logs_every_tile(engine):
    """ac3mi_set_tile_frames 8 on 20 one-frame 5.1 streams: three tiles, the chain three times, the untiled call's bytes"""
    chain = [V.mdct(fx=1), V.search(1, fx=1), V.packf(fx=1)]
    r = V.Enc("tiled", chain, nch=6, shape=(20, 1), tools=dict(pack=1), content="plain", ref="oracle")
    whole = _encode(engine, r, r.tools, None)
    tiled = _encode(engine, r, r.tools, None, tile=8)
    assert whole["logs"] == [chain] and tiled["logs"] == [chain * 3]
    _same(tiled, whole, "tiled against whole")
    _reference(engine, r, r.tools, None, whole)


# ---------------------------------------------------------------------------------------------------------------------
# the decoder's calls

def _decode_batch(r):
    case = DM.FIXED_SHAPE_CASE
    frames = DM.single(case) if r.shape == V.ONE else np.ascontiguousarray(DM.multi(case)[:r.shape[0]])
    assert frames.shape[:2] == r.shape
    return case, frames


@pytest.mark.parametrize("r", DEC, ids=V.recipe_id)
def test_decoder_variant(engine, r):
    case, frames = _decode_batch(r)
    flags = DM.requests(case)[1 if r.downmix else 0]

    def run(mode, fixed):
        try:
            engine.set_decode_mode(mode)
            engine.set_fixed_shape(fixed)
            with V.tap(engine) as names:
                got = DM.decode(engine, frames, case, flags, s16=r.s16)
        finally:
            _restore(engine)
        return got, names

    got, names = run(r.mode, r.fixed)
    assert names == r.chain, "(a) launched %r" % names
    assert (got["status"] & 0x1ff).max() == 0 and got["pcm"].any()
    # (b) the packer's 5.1 frames hold what the front ends branch on: coupling, short blocks, dynrng words
    blocks = [Bk for fr in frames.reshape(-1, frames.shape[-1]) for Bk in A.parse_frame(fr).blocks]
    assert any(Bk.cplinu for Bk in blocks) and any(Bk.fields["dynrnge"] for Bk in blocks)
    assert any(v for Bk in blocks for k, v in Bk.fields.items() if k.startswith("blksw"))
    if r.mode != 1:             # (c)
        base, base_names = run(1, 1)
        assert base_names == [V.dec(0)], base_names
        DM.same(got, base, "(c) mode %d against mode 1" % r.mode)
    if r.sibling_fixed is not None:
        other, other_names = run(r.mode, r.sibling_fixed)
        assert other_names != names and V.families(other_names) == V.families(names), other_names
        assert V.dec(4, fx=1) not in other_names and V.mantx(s16=1, fx=1) not in other_names, other_names
        DM.same(other, got, "(c) the generic kernels")
    ref = DM.liba52((case, "variant matrix", r.shape), frames, flags, 384.0 if r.s16 else 0.0)        # (d)
    fig = DM.held_to_liba52(got, ref, np.full(frames.shape[0], frames.shape[1]), r.s16)
    print("%s: %s" % (r.name, "s16 largest step %d, RMS %.3g of level" % fig if r.s16 else "float RMS %.3g of level, peak %.3g of peak" % fig))


_SRC = {}


@pytest.mark.parametrize("r", SRC, ids=V.recipe_id)
def test_source_variant(engine, r):
    S, F = r.shape
    src = _source(7, 1, 30, S, F, seed=5)
    fb = src.shape[2]
    batch = _padded(src)

    def run(mode):
        try:
            engine.set_decode_mode(mode)
            engine.set_encode_drc_source(1)
            with V.tap(engine) as names:
                got = _transcode(engine, batch, fb, 7, 1, 7 | 16, 448000, H.CHMAP6)
        finally:
            _restore(engine)
        return got, names

    got, names = run(r.mode)
    assert names == r.chain, "(a) launched %r" % names
    assert (got["status"] & 0x1ff).max() == 0
    codes, compr = D.effective(batch[:, :, :fb], got["status"], -1)
    assert D.sends(codes).sum() > S * F and (compr & 0x100).any(), "(b) the source frames carry no words"
    if r.mode != 1:             # (c)
        if "base" not in _SRC:
            _SRC["base"] = run(1)
        base, base_names = _SRC["base"]
        assert base_names[0] == V.dec(0, src=1) and base_names[1:] == r.chain[-4:]
        for k in base:
            assert np.array_equal(got[k], base[k]), "(c) mode %d against mode 1: `%s` differs" % (r.mode, k)
    frames = got["frames"]      # (d)
    nd, nc = D.check_frames(frames, codes, compr, 7)
    assert nd > S * F and nc > 0
    rep = B.Report()
    B.audit(rep, frames, None, np.full(S, 40), r.name)
    rep.finish(r.name)
    T.decodes_cleanly(frames, 7, 1, engine)
