"""GPU: the mantissas of every encoder tool, audited with the independent reader (tests/ac3_syntax.read_mantissas) and the
quantiser model (tests/quantiser_model.py); tests/test_mantissa_reader_cpu.py proves both on the CPU first.

Mode 0 is pinned byte for byte to the reference.  With a tool on, what the other tool tests pin (side information against the
numpy models, CRCs, clean decodes, quality floors, the bit budget) counts a frame's mantissa bits and never reads them: a
wrong rounding at one bap, grouped members in the wrong order around a coupling row, a rematrixed band quantised at the wrong
shift, an off-by-one bin at cplstrtmant or at a reduced chbwcod, stale members in a block's last group would all pass.
tests/mantissa_audit.audit_mantissas asserts, for every coded bin of every frame below, that the code in the bitstream is the
reference quantisers' code of the coefficient the encoder held there.

Rows.  The full-bandwidth channels' and the LFE's coefficients and block shifts are the same call's `mdct` / `exp_samples`
taps, which show the coded rows under rematrixing, bandwidth and block switching (include/ac3mi.h).  The coupling row is
tests/coupling_model.coupling_rows of the same taps, audited over [cplstrtmant, cplendmant) as the frame sends them; channels
in coupling are audited on [0, cplstrtmant).  Rematrixing + coupling: the header defines the coupling row on the rows BEFORE
rematrixing and the taps show the rows after it.  Above cplstrtmant, where the coupling row lives, no band is rematrixed, and
a flagged block's coded rows are the unflagged rows aligned to the pair's common shift - which is the alignment the coupling
sum applies itself - so the taps still give the coupling row exactly and the combination is audited like every other, the
coupling row included (it would show as mismatches in that row alone if this stopped holding).

Left out, and counted per case: bins out of the quantisers' contract (at most 1 % of a case's coded bins; the reference
encoder itself leaves none on this content, test_mantissa_reader_cpu.py), and the one field that crc2 overwrites in a full
2/0 frame (tests/mantissa_audit.py).  Every comparison is an integer equality; nothing here measures time."""
import numpy as np
import pytest

from tests import _tools as T
from tests import layout_model as M
from tests import mantissa_audit as MA
from tests.test_frame_budget_gpu import RATES, TOOLS, matrix_content, matrix_rate, settings, tool_sets

pytestmark = pytest.mark.gpu

CAP = 0.01                    # bins left out as out of contract, of a case's coded bins


def audited_encode(engine, rep, pcm, label, **kw):
    """one encode call with taps, then the audit of its frames against its own taps; -> (frames, the frames' parses)"""
    frames, t = T.encode(engine, pcm, taps=True, **kw)
    S, F = frames.shape[:2]
    parsed = [[None] * F for _ in range(S)]
    MA.audit_mantissas(rep, frames, MA.tap_rows(t), None, label, parsed)
    return frames, parsed


def finish(rep, title, frames):
    rep.finish(title)
    coded = rep.n["compared"] + rep.n["left_out"]
    assert rep.n["frames"] == frames and rep.n["compared"] > 0, rep.n
    assert rep.n["left_out"] <= CAP * coded, "%d of %d coded bins are out of contract" % (rep.n["left_out"], coded)
    assert rep.n["cpl_rows"] == 6 * rep.n["coupled"], rep.n


def exercised(rep, names, nch):
    """every tool of the set left its mark on the case's frames"""
    n = rep.n
    if "bsw" in names:
        assert n["short_blocks"] > 0, n
    if "remat" in names and nch == 2:
        assert n["remat_bands"] > 0, n
    if "cpl" in names and nch >= 2:
        assert n["coupled"] > 0 and n["cpl_rows"] > 0, n
    if "bw" in names:
        assert n["reduced_bw"] > 0, n
    if "drc" in names:
        assert n["dynrng"] > 0, n


CASES = [(nch, names) for nch in (1, 2, 6) for names in tool_sets(nch)]


@pytest.mark.parametrize("nch,names", CASES, ids=["%d-%s" % (nch, "+".join(names)) for nch, names in CASES])
def test_tools_alone_in_pairs_and_together(engine, nch, names):
    """every tool alone, every pair, all together, on the budget matrix's content at its lower rates (where bandwidth mode 2
    cuts).  Among them the coupling row audited under coupling alone and with exponent strategies, bandwidth and DRC, for 2
    and for 6 channels."""
    rep = MA.Report()
    rate = matrix_rate(nch, 0, names)
    title = "%d ch %d b/s %s" % (nch, rate, "+".join(names))
    audited_encode(engine, rep, matrix_content(nch), title, rate=rate, **settings(names))
    finish(rep, title, 18)
    exercised(rep, names, nch)


@pytest.mark.parametrize("tools", [0, 1])
@pytest.mark.parametrize("acmod,lfeon", M.layouts())
def test_every_layout(engine, acmod, lfeon, tools):
    """layout mode 1: rows map to channels in the layout's coded order, the LFE last; with no tool, and with every tool
    (each applies where its rule says: coupling from two full-bandwidth channels on and not in dual mono, rematrixing in
    acmod 2)"""
    rep = MA.Report()
    nch = M.channels(acmod, lfeon)
    title = "layout %d/%d %s" % (acmod, lfeon, "all tools" if tools else "no tool")
    _, parsed = audited_encode(engine, rep, T.tones(acmod, lfeon, 2, 2, seed=40 + 2 * acmod + lfeon), title, layout=(1, acmod, lfeon),
                               rate=RATES[nch][1], chmap=tuple(range(nch)), **(settings(TOOLS) if tools else {}))
    finish(rep, title, 4)
    assert all(P.acmod == acmod and P.lfeon == lfeon for row in parsed for P in row)
    if tools:
        assert rep.n["dynrng"] > 0 and (rep.n["dynrng2"] > 0) == (acmod == 0), rep.n
    else:
        assert rep.n["coupled"] + rep.n["remat_bands"] + rep.n["short_blocks"] + rep.n["reduced_bw"] + rep.n["dynrng"] == 0, rep.n


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_one_frame_streams_with_all_tools(engine, nch):
    """9 streams of one frame: the call shape that searches and packs in other kernels than a multi-frame stream's.  Each
    stream enters with the overlap state (d_last) of the frame before it, as a stream in progress does: from silence every
    first block is an onset, block switching switches it and no frame couples."""
    import torch
    rep = MA.Report()
    names = tool_sets(nch)[-1]
    pcm = np.concatenate([matrix_content(nch, frames=2), T.content("music", nch, 3, 2, seed=730)])
    last = np.ascontiguousarray(pcm[:, 1536 - 256:1536, list(T.chmap_of(nch)[:nch])].transpose(0, 2, 1))
    title = "%d ch, 9 one-frame streams, %s" % (nch, "+".join(names))
    audited_encode(engine, rep, pcm[:, 1536:], title, rate=matrix_rate(nch, 0, names), last=torch.from_numpy(last).cuda(),
                   **settings(names))
    finish(rep, title, 9)
    exercised(rep, names, nch)


INSTANCES = {"2/0": dict(nch=2, acmod=2, kw=dict(rate=192000)), "5.1": dict(nch=6, acmod=7, kw=dict()),
             "dual mono": dict(nch=2, acmod=0, kw=dict(layout=(1, 0, 0), rate=256000, chmap=(0, 1)))}


@pytest.mark.parametrize("config", list(INSTANCES))
def test_per_frame_metadata_words(engine, config):
    """the packers' instantiation that reads a metadata word per frame (ac3mi_set_encode_metadata_frames), both packers"""
    from tests.test_bsi_gpu import _random_words, _words_tensor
    c = INSTANCES[config]
    S, F = 4, 3
    pcm = T.content("music", c["nch"], S, F, seed=300 + c["nch"])
    words = _random_words(np.random.default_rng(17), S, F)
    rep = MA.Report()
    try:
        engine.set_encode_metadata_frames(_words_tensor(words))
        for pack in (1, 2):
            _, parsed = audited_encode(engine, rep, pcm, "%s metadata words, pack %d" % (config, pack), pack=pack, **c["kw"])
            assert len({(P.fields["dialnorm"], P.fields["bsmod"]) for row in parsed for P in row}) > S * F // 2
    finally:
        engine.set_encode_metadata_frames(None)
        engine.set_encode_mode(0)
    finish(rep, "%s, a metadata word per frame" % config, 2 * S * F)
    assert all(P.acmod == c["acmod"] for row in parsed for P in row)


@pytest.mark.parametrize("config", list(INSTANCES))
def test_per_frame_dynrng_words(engine, config):
    """the packers' instantiation that reads dynrng and compr words per frame (ac3mi_set_encode_dynrng_frames), both
    packers; dual mono carries both programmes' words"""
    from tests.test_dynrng_source_gpu import _random_arrays, _tensors
    c = INSTANCES[config]
    S, F = 4, 3
    pcm = T.content("music", c["nch"], S, F, seed=320 + c["nch"])
    codes, compr = _random_arrays(np.random.default_rng(23), S, F)
    assert len({codes[s, f].tobytes() for s in range(S) for f in range(F)}) == S * F
    rep = MA.Report()
    try:
        engine.set_encode_dynrng_frames(*_tensors(codes, compr))
        for pack in (1, 2):
            _, parsed = audited_encode(engine, rep, pcm, "%s dynrng words, pack %d" % (config, pack), pack=pack, **c["kw"])
            sent = sum(P.fields["compre"] + P.fields.get("compr2e", 0) for row in parsed for P in row)
            assert sent > 0 and (sum(P.fields.get("compr2e", 0) for row in parsed for P in row) > 0) == (c["acmod"] == 0)
    finally:
        engine.set_encode_dynrng_frames(None, None)
        engine.set_encode_mode(0)
    finish(rep, "%s, dynrng and compr words per frame" % config, 2 * S * F)
    assert rep.n["dynrng"] > 2 * S * F and (rep.n["dynrng2"] > 2 * S * F) == (c["acmod"] == 0), rep.n


def test_mode_0_control(engine):
    """5.1 at 384 kb/s with no tool - the bytes the reference pins: nothing differs and nothing is left out"""
    rep = MA.Report()
    audited_encode(engine, rep, matrix_content(6), "5.1 384 kb/s no tool", rate=384000)
    finish(rep, "mode 0, 5.1 at 384 kb/s", 18)
    assert rep.n["left_out"] == 0 and rep.n["under_crc2"] == 0, rep.n
    assert rep.n["coupled"] + rep.n["remat_bands"] + rep.n["short_blocks"] + rep.n["reduced_bw"] + rep.n["dynrng"] == 0, rep.n
