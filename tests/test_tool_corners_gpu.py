"""GPU: every encoder tool on the level corners (tests/_tools.corner_batch: digital silence, full-scale squares with -32768,
single full-scale samples, full-scale DC and noise, one square in every channel, the square with its rails swapped between
channels, silence into full scale in mid-frame).

Mode 0 is pinned to the reference byte for byte on such content (tests/test_encode_gpu.py::test_encode_extreme_levels).  The
tools have no oracle encoder: they are held to the numpy models, the budget audit and the mantissa audit, and those ran on
moderate levels only.  Here the tools' kernels do arithmetic mode 0 never does - coupling sums five rows that each sit at
the top of the coefficient range and quantises coordinates from zero energies, rematrixing forms L + R and L - R of two such
rows, DRC sums block energies of full-scale PCM, the strategy search runs over rows that are exponent 24 or 0 everywhere -
and the models are exact integers: a kernel that wraps, saturates or divides differently is an integer mismatch below.
tests/test_tool_corners_cpu.py proves the content well posed first (the reference leaves no bin out of the quantisers'
contract on it; the models' decisions are pinned there).

Per case - every tool that applies to the channel count alone, and all together; sets without exponent strategies at both
rates of the budget matrix, sets with them at the higher one - the side information equals the models' from the mode-0
taps, the budget audit's five items hold (the 1 + 2 frame split lands just before `onset`'s onset), the mantissa audit
holds under the project's cap, every stream decodes cleanly, and every tool of the set left its mark.  Every comparison is
an integer equality but the decoders' 1e-6 RMS; the noise table at the end of a case is printed, not asserted."""
import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import bandwidth_model as W
from tests import block_switch_model as B
from tests import coupling_model as C
from tests import drc_model as D
from tests import layout_model as L
from tests import mantissa_audit as MA
from tests.test_block_switch_gpu import _check_decisions
from tests.test_coupling_gpu import _check_side_info, _model
from tests.test_frame_budget_gpu import APPLIES, RATES, TOOLS, Report, audit, run_config, settings
from tests.test_rematrix_gpu import _check_rows
from tests.test_tool_mantissas_gpu import audited_encode, finish

pytestmark = pytest.mark.gpu

F = 3
BEGF = TOOLS["cpl"]["cpl"][1]
DIALNORM = TOOLS["drc"]["md"]["dialnorm"]
SILENCE, ANTIPHASE = T.CORNER_KINDS.index("silence"), T.CORNER_KINDS.index("rails_antiphase")


def corner_sets(nch):
    """every tool that applies to the channel count alone, and all together (the pairs are in the matrix on moderate content)"""
    names = [t for t in TOOLS if APPLIES.get(t, lambda n: True)(nch)]
    return [(t,) for t in names] + [tuple(names)]


CASES = [(nch, names, hi) for nch in (1, 2, 6) for names in corner_sets(nch) for hi in (0, 1) if hi or "xs" not in names]


def side_information(engine, pcm, nch, rate, names, frames, t1, state):
    """the frames of one call with the set's tools against the models, from the taps of the call with the tools off"""
    S, nfbw = pcm.shape[0], min(nch, 5)
    bsw = int("bsw" in names)
    cpl = "cpl" in names and nch >= 2
    c = W.mode2_chbwcod(48000, rate, nch) if "bw" in names else None
    n = W.nbc(c) if "bw" in names else 223
    sw = np.stack([B.decisions(p, T.chmap_of(nch), nfbw) for p in pcm])
    if bsw:
        _check_decisions(engine, frames, pcm, nch)
    t0 = None
    if cpl:
        _, t0 = T.encode(engine, pcm, rate=rate, taps=True, bsw=bsw)        # (the rows before rematrixing, short where switched)
        if c is None:
            _check_side_info(frames, _model(t0, nch, BEGF, sw=sw if bsw else None), nch, BEGF)
        else:
            for s in range(S):
                for f in range(F):
                    want = W.cpl_decide(t0["mdct"][s, f], t0["exp_samples"][s, f], nfbw, BEGF, c, switched=bool(bsw and sw[s, f].any()))
                    cplinu, chincpl, bf, ef, co = T.coupling_view(frames[s, f], nch)
                    assert cplinu == want[0], (s, f)
                    if cplinu:
                        assert chincpl == (1 << nfbw) - 1 and bf == BEGF and ef == W.cplendf(c)
                        assert [m for m, _ in co] == want[1] and [cd for _, cd in co] == want[2], (s, f)
                    else:
                        assert T.uncoupled_view(frames[s, f], nch)[1] == [c] * nfbw
    if "remat" in names and nch == 2:
        _, flags, _ = _check_rows(engine, pcm, bsw=bsw)
        for s in range(S):
            for f in range(F):
                if cpl and T.coupling_view(frames[s, f], nch)[0]:
                    rm = []
                    T.coupling_view(frames[s, f], nch, remat=rm)
                    assert rm == [1, C.remat_coupled(t0["mdct"][s, f], t0["exp_samples"][s, f], BEGF)[0]], (s, f, rm)
                elif "bw" in names:
                    rows, x = t0["mdct"][s, f, 0].astype(np.int64), t0["exp_samples"][s, f, 0]
                    want = 0 if bsw and sw[s, f, 0, 0] != sw[s, f, 0, 1] else W.remat_flags(rows[0], rows[1], int(x[0]), int(x[1]), n)
                    assert T.uncoupled_view(frames[s, f], 2)[0] == want, (s, f)
                else:
                    assert T.uncoupled_view(frames[s, f], 2)[0] == flags[s, f, 0], (s, f)
    if "drc" in names:
        _, status, tp = T.decode(engine, frames, *T.layout_of(nch), taps=True)
        assert (status & 0x1ff).max() == 0
        end = state.cpu().numpy()
        for s in range(S):
            codes, snt, s_end, _ = D.encode(pcm[s], T.chmap_of(nch), nfbw, TOOLS["drc"]["drc"], DIALNORM)
            w = tp["dynrng"][s, :, :, 0]
            assert np.array_equal(~np.isnan(w), snt), (s, snt, w)
            want = np.array([[D.decoded_gain(v) for v in row] for row in codes], np.float32)
            assert np.array_equal(w[snt], want[snt]), s
            assert int(end[s]) == s_end, (s, int(end[s]), s_end)
    if "xs" in names:
        if cpl:
            assert T.check_coupled_frames(engine, pcm, nch, BEGF, c) > 0
        else:
            T.check_rows(t1, nch, n)


def exercised(rep, names, nch, frames):
    n = rep.n
    if "bsw" in names:
        assert n["short_blocks"] > 0, n
    if "remat" in names and nch == 2:
        assert n["remat_bands"] > 0, n
    if "cpl" in names and nch >= 2:
        assert n["coupled"] > 0 and n["cpl_rows"] > 0, n
        on = [[T.coupling_view(frames[s, f], nch)[0] for f in range(F)] for s in (SILENCE, ANTIPHASE)]
        assert on == [[1] * F, [0] * F], on               # zero energies couple; rails that cancel never do
    if "drc" in names:
        assert n["dynrng"] > 0, n


# ---------------------------------------------------------------------------------------------------------------------
# reported, not asserted: the noise of a decode against its source

_MODE0 = {}


def noise(frames, pcm, nch):
    """[S] RMS of (the restatement's decode, 256 samples later) - source, in s16 steps, over the whole stream"""
    acmod, lfeon = T.layout_of(nch)
    flags = acmod | (16 if lfeon else 0)
    planes = L.wave_planes(flags)
    out = []
    for s in range(frames.shape[0]):
        dec, errs, _ = H.orc_decode(frames[s], flags, 1.0, 0.0)
        assert errs == 0
        d = dec.transpose(0, 1, 3, 2).reshape(-1, nch).astype(np.float64)[:, planes] * 32768.0
        out.append(H.rms(d[256:] - pcm[s][:d.shape[0] - 256]))
    return np.array(out)


def report_noise(engine, frames, pcm, nch, rate, names):
    if (nch, rate) not in _MODE0:
        _MODE0[(nch, rate)] = noise(T.encode(engine, pcm, rate=rate), pcm, nch)
    n0, n1 = _MODE0[(nch, rate)], noise(frames, pcm, nch)
    for i, kind in enumerate(T.CORNER_KINDS):
        db = 20 * np.log10(n1[i] / n0[i]) if n0[i] > 0 and n1[i] > 0 else 0.0 if n1[i] == n0[i] else float("inf")
        print("noise | %d ch %d b/s | %s | %s | mode 0 %.2f | tools %.2f | %+.2f dB" % (nch, rate, "+".join(names), kind, n0[i], n1[i], db))


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch,names,hi", CASES, ids=["%d-%s-%s" % (nch, "+".join(names), ("lo", "hi")[hi]) for nch, names, hi in CASES])
def test_tools_on_the_level_corners(engine, nch, names, hi):
    import torch
    rate = RATES[nch][hi]
    pcm = T.corner_batch(nch, F)
    title = "corners %d ch %d b/s %s" % (nch, rate, "+".join(names))
    state = torch.zeros((pcm.shape[0],), dtype=torch.int32, device="cuda")
    frames, t1 = T.encode(engine, pcm, rate=rate, taps=True, state=state, **settings(names))
    side_information(engine, pcm, nch, rate, names, frames, t1, state)
    # the budget audit, items 1 to 5.  No failed search is tolerated: a case that exponent strategies overrun (DESIGN.md
    # 4.3f) would have to be proven that defect and listed here by name, and none is
    rep = Report()
    assert np.array_equal(run_config(engine, rep, pcm, title, rate=rate, **settings(names)), frames)
    rep.finish(title)
    assert rep.n["frames"] == 8 * F
    # the mantissa audit
    mrep = MA.Report()
    got, _ = audited_encode(engine, mrep, pcm, title, rate=rate, **settings(names))
    assert np.array_equal(got, frames)
    finish(mrep, title, 8 * F)
    T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
    exercised(mrep, names, nch, frames)
    if hi and "drc" not in names:
        report_noise(engine, frames, pcm, nch, rate, names)


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_one_frame_streams_with_all_tools(engine, nch):
    """nine one-frame streams, the call shape that searches and packs in other kernels: frame 2 of each corner stream and
    `rails_identical` once more, each entering with the overlap state of the frame before it"""
    import torch
    names = corner_sets(nch)[-1]
    rate = RATES[nch][1]
    batch = T.corner_batch(nch, F)
    pcm = np.concatenate([batch, batch[5:6]])[:, 1536:]
    last = np.ascontiguousarray(pcm[:, 1536 - 256:1536, list(T.chmap_of(nch)[:nch])].transpose(0, 2, 1))
    title = "corners %d ch, 9 one-frame streams, %s" % (nch, "+".join(names))
    mrep = MA.Report()
    frames, _ = audited_encode(engine, mrep, pcm[:, 1536:], title, rate=rate, last=torch.from_numpy(last).cuda(), **settings(names))
    finish(mrep, title, 9)
    T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
    rep = Report()
    rep.n["configs"] += 1
    for pack in (0, 1, 2):
        got, taps = T.encode(engine, pcm[:, 1536:], rate=rate, last=torch.from_numpy(last).cuda(), taps=True, pack=pack, **settings(names))
        assert np.array_equal(got, frames), pack
    audit(rep, frames, taps, np.full(9, 40), title)
    rep.finish(title)
    n = mrep.n
    assert n["short_blocks"] > 0 and n["dynrng"] > 0 and (n["coupled"] > 0) == (nch >= 2) and (n["remat_bands"] > 0) == (nch == 2), n


@pytest.mark.parametrize("acmod,lfeon", [(0, 0), (2, 1), (7, 1)])
def test_layouts_with_all_tools(engine, acmod, lfeon):
    """layout mode 1 with every tool: dual mono (dynrng2), 2/0 + LFE (rematrixing beside an LFE) and 3/2 + LFE (the
    five-row coupling sum)"""
    nch = L.channels(acmod, lfeon)
    rate = RATES[nch][1]
    pcm = T.corner_batch(nch, F)
    kw = settings(TOOLS)
    title = "corners layout %d/%d all tools" % (acmod, lfeon)
    rep = Report()
    frames = run_config(engine, rep, pcm, title, layout=(1, acmod, lfeon), rate=rate, **kw)
    rep.finish(title)
    mrep = MA.Report()
    got, parsed = audited_encode(engine, mrep, pcm, title, layout=(1, acmod, lfeon), rate=rate, chmap=tuple(range(nch)), **kw)
    assert np.array_equal(got, frames)
    finish(mrep, title, 8 * F)
    assert all(P.acmod == acmod and P.lfeon == lfeon for row in parsed for P in row)
    T.decodes_cleanly(frames, acmod, lfeon, engine=engine)
    n = mrep.n
    assert n["short_blocks"] > 0 and n["dynrng"] > 0 and (n["dynrng2"] > 0) == (acmod == 0), n
    assert (n["remat_bands"] > 0) == (acmod == 2) and (n["coupled"] > 0) == (acmod >= 2), n
    if acmod >= 2:
        on = [[int(parsed[s][f].blocks[0].cplinu) for f in range(F)] for s in (SILENCE, ANTIPHASE)]
        assert on == [[1] * F, [0] * F], on
