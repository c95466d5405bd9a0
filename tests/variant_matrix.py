"""The variant matrix (not collected): for every kernel instantiation that csrc/launch_rule.h lists, one call at the smallest
shape the rule sends to it - the recipes - and the test aid that says what a call launched.

ac3mi_debug_launch_log hands out family << 24 | variant word of every launch of the rule's kernels.  `tap` sets it around
calls and decodes the words through the table that tests/launch_rule_c/main.cpp prints in its mode `words` (word_table): the
one place that ties a word to a kernel's name.  Nothing here knows a V_* bit; the helpers below spell a kernel's name from
its template arguments, in the order of the kernel's parameter list, as `main lists` prints it.

A recipe holds the entry point, the layout, streams x frames, the context's settings, the content, the expected ordered
chain of kernels, the features its output must show, its sibling routes (each with its own expected chain: other kernels,
the same bytes) and the reference it is held to.  One-frame batches have 9 streams (no multiple of 8: both branches of the
XCD remap run), multi-frame batches 3 streams x 3 frames; every threshold of the rule has a setter that forces either side,
so nothing larger is needed.  tests/test_variant_matrix_cpu.py holds the recipes' chains to the 79 listed variants,
tests/test_variant_matrix_gpu.py runs them."""
import contextlib
import os
import subprocess
import tempfile

import numpy as np

from tests import _harness as H

ONE, MULTI = (9, 1), (3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# names

def _b(*flags):
    return ", ".join("true" if f else "false" for f in flags)


def dec(mode, fx=0, src=0):
    return "decode_kernel<%d, %s>" % (mode, _b(fx, src))


def wg(out, src=0):
    return "decode_wg_kernel<%d, %s>" % (out, _b(src))


LFSR, MANT = "lfsr_prefix_kernel", "mant_kernel"


def mantx(s16=0, fx=0):
    return "mantx_kernel<%s>" % _b(s16, fx)


def mdct(bsw=0, remat=0, bw=0, xs=0, lferow=0, fx=0):
    return "enc_mdct_kernel<%s>" % _b(bsw, remat, bw, xs, lferow, fx)


def cplk(bw=0, xs=0, r3=0):
    return "enc_cpl_kernel<%s>" % _b(bw, xs, r3)


def search(part, cpl=0, bw=0, drc=0, fx=0, dw=0):
    return "enc_search_kernel<%d, %s>" % (part, _b(cpl, bw, drc, fx, dw))


def packf(fx=0, cpl=0, bw=0, md=0, dual=0, dw=0):
    return "enc_packf_kernel<%s>" % _b(fx, cpl, bw, md, dual, dw)


def packb(md=0, dw=0):
    return "enc_packb_kernel<%s>" % _b(md, dw)


# ---------------------------------------------------------------------------------------------------------------------
# the log

_TABLE = None


def word_table():
    """{family << 24 | variant word: kernel name} of the 79 listed variants, from `main words` (built once per process)"""
    global _TABLE
    if _TABLE is None:
        src = os.path.join(H.ROOT, "tests", "launch_rule_c", "main.cpp")
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "launch_rule")
            subprocess.run(["g++", "-std=c++17", "-O0", "-I", os.path.join(H.ROOT, "ac-3-acm-codec_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
            out = subprocess.run([exe, "words"], check=True, capture_output=True, text=True).stdout
        table = {}
        for line in out.splitlines():
            family, word, name = line.split(" ", 2)
            table[int(family) << 24 | int(word)] = name
        _TABLE = table
    return _TABLE


def decode_log(log):
    """the array a tap filled -> the kernels' names in launch order; a word outside the table is an error, and so is a log
    that did not hold every launch"""
    n = int(log[0])
    assert n < log.size, "%d launches, room for %d" % (n, log.size - 1)
    table = word_table()
    return [table[int(w)] for w in log[1:1 + n]]


@contextlib.contextmanager
def tap(engine, capacity=256):
    """with tap(engine) as names: ... - the tap is set around the block; `names` holds the launches' names once it ends"""
    log = np.zeros(capacity, np.uint32)
    names = []
    engine.debug_launch_log(log)
    try:
        yield names
    finally:
        engine.debug_launch_log(None)
        names.extend(decode_log(log))


def families(names):
    """the kernel families of a list of names (a name without its template arguments)"""
    return {n.split("<")[0] for n in names}


# ---------------------------------------------------------------------------------------------------------------------
# encoder recipes

META = dict(dialnorm=24, bsmod=2, cmixlev=0, surmixlev=2, dsurmod=1, copyrightb=0, origbs=0)
RATE = {2: 256000, 3: 320000, 6: 448000}        # (tests/test_frame_budget_gpu.py's generous rates: no search fails at them)
BW_CUT = 30                                     # the chbwcod of the calls that show a BW variant's bandwidth matters
BEGF = 2


class Sibling:
    """another route to the same bytes: the recipe's call with `tools` merged in (a value None takes the tool out), the
    words rule replaced when `words` is given, the fixed shape switched, or (split) one call per frame with the state carried
    by the caller; `chain`: what that route launches (per call)"""

    def __init__(self, what, chain, tools=None, fixed=1, split=False, words="keep"):
        self.what, self.chain, self.tools, self.fixed, self.split, self.words = what, chain, tools or {}, fixed, split, words


class Enc:
    """one ac3mi_encode_batch call through tests/_tools.encode.
    layout: None = the reference's for nch channels, else (acmod, lfeon); tools: tests/_tools.encode's; words: None, "md_default"
    (a per-frame metadata array holding the default word) or "dw" (ac3mi_set_encode_dynrng_frames with random words);
    content: "music", "attack" (stereo, a burst per frame), "stepped" (music whose level steps every two blocks), "plain" (the
    harness's music and tones from a new stream's state: the oracle's input); feature_tools: a second call, expected to launch
    the same chain, on whose output the features and the audits are checked (None: the call itself); ref: "oracle" (every tool
    off: byte for byte the ac3enc restatement) or "audit"."""
    kind = "encode"

    def __init__(self, name, chain, nch=2, layout=None, shape=ONE, tools=None, words=None, content="music", features=(),
                 feature_tools=None, feature_words="keep", siblings=(), ref="audit"):
        self.name, self.chain, self.nch, self.layout, self.shape = name, chain, nch, layout, shape
        self.tools, self.words, self.content, self.features = tools or {}, words, content, tuple(features)
        self.feature_tools, self.feature_words, self.siblings, self.ref = feature_tools, feature_words, list(siblings), ref

    @property
    def acmod(self):
        return self.layout[0] if self.layout else {2: 2, 6: 7}[self.nch]

    @property
    def lfeon(self):
        return self.layout[1] if self.layout else int(self.nch == 6)


def _enc_recipes():
    out = []
    # the front kernel's tools on 2/0, one-frame streams, the block packer (every tool off: the oracle's bytes)
    for xs in (0, 1):
        for bsw, remat, bw in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)):
            tools = dict(pack=2)
            tools.update(dict(bsw=1) if bsw else {}, **(dict(remat=1) if remat else {}))
            if xs:
                tools["xs"] = 1
            if bw:
                tools["bw"] = (1, 50)
            on = [k for k, v in (("bsw", bsw), ("remat", remat), ("bw", bw), ("xs", xs)) if v]
            chain = [mdct(bsw=bsw, remat=remat, bw=bw, xs=xs), search(1), packb()]
            sib = []
            if bw:      # "mode 1 at chbwcod 50 is mode 0 byte for byte"
                sib.append(Sibling("bandwidth off", [mdct(bsw=bsw, remat=remat, xs=xs), search(1), packb()], dict(bw=None)))
            if not on:
                sib.append(Sibling("one wavefront per frame packs", [mdct(), search(1), packf()], dict(pack=1)))
            out.append(Enc("2/0 " + ("+".join(on) or "plain, block packer"), chain, tools=tools, content="attack" if bsw else ("music" if on else "plain"),
                           features=[k.upper() for k in on if k != "bw"], feature_tools=dict(tools, bw=(1, BW_CUT)) if bw else None,
                           siblings=sib, ref="audit" if on else "oracle"))
            if bw:
                out[-1].features += ("BW",)
    # 5.1, one-frame streams, nothing on: the fixed-shape front kernel, search and frame packer
    out.append(Enc("5.1 plain, fixed shape", [mdct(fx=1), search(1, fx=1), packf(fx=1)], nch=6, tools=dict(pack=1), content="plain", ref="oracle",
                   siblings=[Sibling("fixed shape off", [mdct(), search(1), packf()], fixed=0),
                             Sibling("block packer", [mdct(fx=1), search(1, fx=1), packb()], dict(pack=2))]))
    # 2/0 + LFE with rematrixing: the LFE row in a launch of its own
    for xs in (0, 1):
        out.append(Enc("2/0+LFE remat" + ("+xs" if xs else ""), [mdct(remat=1, xs=xs), mdct(lferow=1, xs=xs), search(1), packb()], nch=3,
                       layout=(2, 1), tools=dict(pack=2, remat=1, **(dict(xs=1) if xs else {})), features=["REMAT"] + (["XS"] if xs else [])))
    # coupling x bandwidth x strategies, on 2/0 and (R3) on 2/0 + LFE with rematrixing
    for r3 in (0, 1):
        for bw in (0, 1):
            for xs in (0, 1):
                tools = dict(pack=1, cpl=(1, BEGF))
                if r3:
                    tools["remat"] = 1
                if xs:
                    tools["xs"] = 1
                if bw:
                    tools["bw"] = (1, 50)

                def chain(bw):
                    return (([mdct()] if r3 else []) + [mdct(remat=r3, bw=bw and r3, xs=xs)] + ([mdct(lferow=1, xs=xs)] if r3 else []) +
                            [cplk(bw=bw, xs=xs, r3=r3), search(1, cpl=1, bw=bw), packf(cpl=1, bw=bw)])
                on = ["cpl"] + [k for k, v in (("remat", r3), ("bw", bw), ("xs", xs)) if v]
                out.append(Enc(("2/0+LFE " if r3 else "2/0 ") + "+".join(on), chain(bw), nch=3 if r3 else 2, layout=(2, 1) if r3 else None,
                               tools=tools, features=[k.upper() for k in on], feature_tools=dict(tools, bw=(1, BW_CUT)) if bw else None,
                               siblings=[Sibling("bandwidth off", chain(0), dict(bw=None))] if bw else []))
    # the searches: three-frame streams tabulate (PART 3) and replay (PART 1); their sibling is three calls of one-frame
    # streams, PART 1 alone.  x {uncoupled, coupled, coupled + bandwidth} x {no words, a DRC profile, words from arrays};
    # one wavefront per frame packs
    for cpl, bw in ((0, 0), (1, 0), (1, 1)):
        for rule in ("none", "drc", "dw"):
            d, w = int(rule != "none"), int(rule == "dw")
            tools = dict(pack=1)
            if cpl:
                tools["cpl"] = (1, BEGF)
            if bw:
                tools["bw"] = (1, 50)
            if rule == "drc":
                tools.update(drc=1, md=META)

            def chain(bw, tabulate=True, block=False):
                return ([mdct()] + ([cplk(bw=bw)] if cpl else []) + ([search(3, cpl=cpl, bw=bw, drc=d, dw=w)] if tabulate else []) +
                        [search(1, cpl=cpl, bw=bw, drc=d, dw=w), packb(md=d, dw=w) if block else packf(cpl=cpl, bw=bw, md=d, dw=w)])
            sib = [Sibling("three calls of one frame", chain(bw, tabulate=False), split=True)]
            if bw:
                sib.append(Sibling("bandwidth off", chain(0), dict(bw=None)))
            if not cpl:
                sib.append(Sibling("block packer", chain(0, block=True), dict(pack=2)))
            plain = not cpl and rule == "none"
            feats = (["CPL"] if cpl else []) + (["BW"] if bw else []) + {"none": [], "drc": ["DRC", "MD"], "dw": ["DW"]}[rule]
            out.append(Enc("2/0 three frames, %s, words: %s" % ("coupled + bandwidth" if bw else "coupled" if cpl else "uncoupled", rule),
                           chain(bw), shape=MULTI, tools=tools, words="dw" if w else None, content="plain" if plain else "stepped",
                           features=feats, feature_tools=dict(tools, bw=(1, BW_CUT)) if bw else None, siblings=sib,
                           ref="oracle" if plain else "audit"))
    # the frame packer's shapes x {plain, metadata, metadata + words} that the recipes above do not name, on one-frame
    # streams.  "md": a per-frame array that holds the default word (its sibling: no array, the plain packer, the same
    # bytes); the feature call sets other BSI fields through the context instead
    shapes = {"generic": dict(nch=2), "dual mono": dict(nch=2, layout=(0, 0)), "5.1": dict(nch=6), "5.1 + bandwidth": dict(nch=6, bw=1),
              "coupled": dict(nch=2, cpl=1), "coupled + bandwidth": dict(nch=2, cpl=1, bw=1)}
    named = {("generic", "plain"), ("generic", "dw"), ("5.1", "plain"), ("coupled", "plain"), ("coupled", "dw"), ("coupled + bandwidth", "plain"),
             ("coupled + bandwidth", "dw")}
    for shape, s in shapes.items():
        for rule in ("plain", "md", "dw"):
            if (shape, rule) in named:
                continue
            m, w = int(rule != "plain"), int(rule == "dw")
            cpl, bw, six, dual = s.get("cpl", 0), s.get("bw", 0), s["nch"] == 6, int(shape == "dual mono")
            tools = dict(pack=1)
            if cpl:
                tools["cpl"] = (1, BEGF)
            if bw:
                tools["bw"] = (1, 50)

            def chain(bw=bw, m=m, fixed=1, block=False):
                fx = int(six and fixed)
                fx_plain = int(fx and not bw and not w)                 # the front kernel and the search: no tool or word of theirs
                pack = packb(md=m, dw=w) if block else packf(fx=fx, cpl=cpl, bw=bw and (cpl or fx), md=m, dual=dual, dw=w)
                return ([mdct(fx=fx_plain)] + ([cplk(bw=bw)] if cpl else []) +
                        [search(1, cpl=cpl, bw=bw and cpl, drc=w, fx=fx_plain, dw=w), pack])
            sib = []
            if rule == "md":
                sib.append(Sibling("no metadata array", chain(m=0), words=None))
            if bw:
                sib.append(Sibling("bandwidth off", chain(bw=0), dict(bw=None)))
            if six:
                sib.append(Sibling("fixed shape off", chain(fixed=0), fixed=0))
            if not cpl:
                sib.append(Sibling("block packer", chain(block=True), dict(pack=2)))
            feats = (["CPL"] if cpl else []) + (["BW"] if bw else []) + (["DUAL"] if dual else []) + {"plain": [], "md": ["MD"], "dw": ["DW"]}[rule]
            ftools = dict(tools)
            if bw:
                ftools["bw"] = (1, BW_CUT)
            if rule == "md":
                ftools["md"] = META
            out.append(Enc("%s, frame packer, %s" % (shape, rule), chain(), nch=s["nch"], layout=s.get("layout"), tools=tools,
                           words={"plain": None, "md": "md_default", "dw": "dw"}[rule], features=feats,
                           feature_tools=ftools if ftools != tools else None, feature_words=None if rule == "md" else "keep", siblings=sib))
    # the block packer with metadata and with words
    for rule in ("md", "dw"):
        w = int(rule == "dw")
        chain = [mdct(), search(1, drc=w, dw=w), packb(md=1, dw=w)]
        sib = [Sibling("one wavefront per frame packs", chain[:2] + [packf(md=1, dw=w)], dict(pack=1))]
        if rule == "md":
            sib.append(Sibling("no metadata array", [mdct(), search(1), packb()], words=None))
        out.append(Enc("2/0 block packer, %s" % rule, chain, tools=dict(pack=2), words="dw" if w else "md_default", features=["DW" if w else "MD"],
                       feature_tools=dict(pack=2, md=META) if rule == "md" else None, feature_words=None if rule == "md" else "keep", siblings=sib))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# decoder and transcode recipes (the batches of tests/_decode_matrix.py: the small 5.1 case, the shape the fixed-shape kernels take)

class Dec:
    """one ac3mi_decode_batch / ac3mi_decode_s16_batch call under ac3mi_set_decode_mode `mode`: the case's one-frame batch (9
    streams) or the first three streams of its three-frame batch; downmix: the case's first downmix request instead of the layout.
    sibling: mode 1 on the same call, bit for bit (mode 1 itself: held to liba52 only)."""
    kind = "decode"

    def __init__(self, name, chain, mode, shape=MULTI, s16=False, fixed=1, downmix=False, sibling_fixed=None):
        self.name, self.chain, self.mode, self.shape, self.s16, self.fixed, self.downmix = name, chain, mode, shape, s16, fixed, downmix
        self.sibling_fixed = sibling_fixed


class Src:
    """one ac3mi_transcode_batch call of 3 x 3 5.1 frames that carry dynrng and compr words, under ac3mi_set_encode_drc_source 1
    and ac3mi_set_decode_mode `mode`: the decoder's SRC front end, then the encoder's chain with the words from arrays"""
    kind = "transcode"
    shape = MULTI

    def __init__(self, name, front, mode):
        self.name, self.mode = name, mode
        self.chain = front + [mdct(), search(3, drc=1, dw=1), search(1, drc=1, dw=1), packb(md=1, dw=1)]


def _dec_recipes():
    return [Dec("mode 1", [dec(0)], 1),
            Dec("mode 4", [dec(4), MANT], 4),
            Dec("mode 5", [dec(5), LFSR, MANT], 5),
            Dec("mode 6, float, fixed shape", [dec(4, fx=1), mantx()], 6, shape=ONE, sibling_fixed=0),
            Dec("mode 6, s16, fixed shape", [dec(4, fx=1), mantx(s16=1, fx=1)], 6, shape=ONE, s16=True, sibling_fixed=0),
            Dec("mode 6, s16, generic", [dec(4), mantx(s16=1)], 6, shape=ONE, s16=True, fixed=0),
            Dec("mode 3, float", [wg(1)], 3),
            Dec("mode 3, s16", [wg(2)], 3, s16=True),
            Dec("mode 3, downmix", [wg(0)], 3, downmix=True),
            Src("source words, mode 1", [dec(0, src=1)], 1),
            Src("source words, mode 3", [wg(2, src=1)], 3),
            Src("source words, mode 4", [dec(4, src=1), MANT], 4),
            Src("source words, mode 5", [dec(5, src=1), LFSR, MANT], 5)]


RECIPES = _enc_recipes() + _dec_recipes()


def recipe_id(r):
    return r.name.replace(" ", "_")
