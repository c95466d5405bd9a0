"""GPU: the two packers write one side-information syntax (csrc/enc_syntax.h).  enc_packf_kernel (pack mode 1) and
enc_packb_kernel (mode 2) must give the same bytes, and tests/ac3_syntax.parse_frame must read every frame to the end of block
5, on the smallest shapes at which a shared field list can still go wrong: one channel; dual mono with each programme's own
dynrng and compr words; 2/0 with rematrixing and coupling (both modes take enc_packf_kernel: coupled frames have no block
packer); 5.1 with the fixed shape on and off.  The 5.1 and one coupled case run with a reduced bandwidth and the word arrays,
and dual mono once with no tool at all: enc_packf_kernel's instantiations <FIXED51, BW, MD, DW>, <CPL, BW, MD, DW> and <DUAL>
alone are launched by no other test (the byte-exact references and test_frame_budget_gpu, test_dynrng_source_gpu,
test_layout_gpu, test_coupling_gpu, test_tool_mantissas_gpu reach the rest).  Two streams show a slip
in the frame index, two frames block 0 against the blocks after it with carried state."""
import numpy as np
import pytest

from tests import _tools as T
from tests import ac3_syntax as A
from tests import test_dynrng_source_gpu as DS
from tests import test_frame_budget_gpu as B

pytestmark = pytest.mark.gpu

S, F = 2, 2
CASES = {"1/0": dict(nch=1, kw={}),
         "1+1": dict(nch=2, kw=dict(layout=(1, 0, 0))),
         "1+1 words per programme": dict(nch=2, kw=dict(layout=(1, 0, 0)), words=True),
         "2/0 rematrixing, coupling at 2": dict(nch=2, kw=dict(remat=1, cpl=(1, 2))),
         "2/0 coupling at 2, chbwcod 30, words": dict(nch=2, kw=dict(cpl=(1, 2), bw=(1, 30)), words=True),
         "3/2+LFE chbwcod 30, words, fixed shape": dict(nch=6, kw=dict(bw=(1, 30)), words=True, fixed=1),
         "3/2+LFE chbwcod 30, words, generic": dict(nch=6, kw=dict(bw=(1, 30)), words=True, fixed=0)}


@pytest.mark.parametrize("name", list(CASES))
def test_both_packers_write_the_same_frames(engine, name):
    c = CASES[name]
    nch = c["nch"]
    pcm = T.content("music", nch, S, F, seed=4100 + nch)
    try:
        engine.set_fixed_shape(c.get("fixed", 1))
        if c.get("words"):
            engine.set_encode_dynrng_frames(*DS._tensors(*DS._random_arrays(np.random.default_rng(77), S, F)))
        got = [T.encode(engine, pcm, pack=pack, rate=B.RATES[nch][1], **c["kw"]) for pack in (1, 2)]
    finally:
        DS._restore(engine)
    assert got[0].shape[:2] == (S, F) and np.array_equal(got[0], got[1]), "%d frames differ" % int((got[0] != got[1]).any(axis=2).sum())
    sent = coupled = 0
    for s in range(S):
        for f in range(F):
            P = A.parse_frame(got[0][s, f])
            # (the audit's accounting, test_frame_budget_gpu item 2: a 2/0 frame may run over by block 0's unpriced rematrixing flags)
            assert P.frame_bytes == got[0].shape[2] and P.block_end[5] + A.TAIL_BITS <= 8 * P.frame_bytes + A.uncounted_bits(P), (s, f, P.block_end)
            sent += sum(Bk.fields["dynrnge"] + Bk.fields.get("dynrng2e", 0) for Bk in P.blocks)
            coupled += P.blocks[0].cplinu
    assert (sent > 0) == bool(c.get("words")) and (coupled > 0) == ("cpl" in c["kw"]), (sent, coupled)
