"""What the encoder-tool GPU tests share (tests/_harness.py stays the CPU / oracle harness): one encode call that knows
every ac3mi_set_encode_* setter, one decode call, one clean-decode check, the content generators, and views of a frame's
BSI and block 0 read through tests/ac3_syntax.parse_frame - the reader that audits the bit budget."""
import numpy as np

from tests import _harness as H
from tests import ac3_syntax as A

RATE = {1: 192000, 2: 192000, 3: 384000, 4: 384000, 5: 384000, 6: 384000}
ACMOD = {1: 1, 2: 2, 5: 7, 6: 7}


def chmap_of(nch):
    return H.CHMAP6 if nch == 6 else tuple(range(nch))


def layout_of(nch):
    """(acmod, lfeon) of the reference's layouts for 1, 2, 5 and 6 channels"""
    return ACMOD[nch], 1 if nch == 6 else 0


# ---------------------------------------------------------------------------------------------------------------------
# encode, decode, transcode

KEEP = object()             # a tool given as KEEP is not touched, before or after the call: the context's setting holds
# tool -> (setter, default, reset arguments); a value is the setter's argument, or a tuple of them
TOOLS = {"layout": ("set_encode_layout", KEEP, (0,)),
         "pack": ("set_encode_mode", KEEP, (0,)),
         "bsw": ("set_encode_block_switch", 0, (0,)),
         "remat": ("set_encode_rematrix", 0, (0,)),
         "cpl": ("set_encode_coupling", (0, 0), (0, 0)),
         "bw": ("set_encode_bandwidth", (0, 50), (0,)),
         "xs": ("set_encode_exp_strategy", 0, (0,)),
         "md": ("set_encode_metadata", None, ()),           # a dict of fields, None = the defaults
         "drc": ("set_encode_drc", 0, (0,))}                # the profile; its state is `state`


def encode(engine, pcm, *, rate=None, sr=48000, chmap=None, last=None, csnr=None, state=None, taps=False, out=None, **tools):
    """pcm [S][F*1536][nch] s16 -> frames [S][F][fb][, taps], one call.  `tools`: layout=(mode, acmod, lfeon), pack, bsw,
    remat, cpl=(mode, begf), bw=(mode, chbwcod), xs, md=dict, drc (with `state`, int32 [S] on the device, zeros when None).
    Every tool not given is set to its default (layout and pack: kept); everything set is reset afterwards.  `out`: the
    output tensor [S][F][stride] u8 (Engine.encode_batch), whatever it holds."""
    import torch
    unknown = set(tools) - set(TOOLS)
    if unknown:
        raise TypeError("unknown tool(s): %s" % ", ".join(sorted(unknown)))
    S, n, nch = pcm.shape
    F = n // 1536
    enc = H.pkg().EncodeDesc(sr, rate or RATE[nch], nch)
    if last is None:
        last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    if csnr is None:
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    want = {k: tools.get(k, TOOLS[k][1]) for k in TOOLS}
    if want["drc"] is not KEEP and want["drc"] and state is None:
        state = torch.zeros((S,), dtype=torch.int32, device="cuda")
    try:
        for k, v in want.items():
            setter = getattr(engine, TOOLS[k][0])
            if v is KEEP:
                continue
            if k == "md":
                if v:
                    setter(**v)
            elif k == "drc":
                setter(v, state if v else None)
            else:
                setter(*(v if isinstance(v, tuple) else (v,)))
        r = engine.encode_batch(enc, torch.from_numpy(np.ascontiguousarray(pcm, np.int16).reshape(S, F, 1536, nch)).cuda(),
                                chmap if chmap is not None else chmap_of(nch), last, csnr, out=out, taps=taps)
        engine.sync()
    finally:
        for k, v in want.items():
            if v is not KEEP:
                getattr(engine, TOOLS[k][0])(*TOOLS[k][2])
    fb = enc.frame_bytes()
    if taps:
        return r[0].cpu().numpy()[:, :, :fb], {k: v.cpu().numpy() for k, v in r[1].items()}
    return r.cpu().numpy()[:, :, :fb]


def decode(engine, frames, acmod, lfeon, flags=None, taps=False):
    """frames [S][F][fb] -> (pcm [S][F][6][n_out][256], status [S][F], the taps or None) for output `flags` (None: the
    layout itself)"""
    import torch
    S, F, fb = frames.shape
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = frames
    if flags is None:
        flags = acmod | (16 if lfeon else 0)
    dec = H.pkg().DecodeDesc(flags=flags, level=1.0, bias=0.0, dynrng=1, acmod=acmod, lfeon=lfeon, frame_bytes=fb)
    nout, _ = engine.decode_planes(dec)
    delay = torch.zeros((S, nout, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    r = engine.decode_batch(dec, torch.from_numpy(buf).cuda(), delay, lfsr, taps=taps)
    engine.sync()
    return r[0].cpu().numpy(), r[1].cpu().numpy(), {k: v.cpu().numpy() for k, v in r[2].items()} if taps else None


def decodes_cleanly(frames, acmod, lfeon, engine=None):
    """Both CRCs hold and the liba52 restatement decodes every stream [S][F][fb] without an error.  With an `engine` the GPU
    decoder's status bits are clear and its output is the restatement's to 1e-6 RMS; without one the restatement's output
    flags are the layout's (a stream whose metadata says Dolby Surround is granted other flags than it was asked for)."""
    import bench
    assert bench.ac3_crc_ok(frames.reshape(-1, frames.shape[2])) == 0
    flags = acmod | (16 if lfeon else 0)
    if engine is not None:
        got, status, _ = decode(engine, frames, acmod, lfeon)
        assert (status & 0x1ff).max() == 0
    for s in range(frames.shape[0]):
        ref, errs, oflags = H.orc_decode(frames[s], flags, 1.0, 0.0)
        assert errs == 0
        if engine is None:
            assert oflags == flags
        else:
            err = got[s].astype(np.float64) - ref.reshape(got[s].shape)
            assert H.rms(err) <= 1e-6, H.rms(err)


def transcode(engine, src, acmod, lfeon, flags, chmap, rate=384000):
    import torch
    pkg = H.pkg()
    S, F, fb = src.shape
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = src
    dec = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0, dynrng=1, acmod=acmod, lfeon=lfeon, frame_bytes=fb)
    n_out, oflags = engine.decode_planes(dec)
    enc = pkg.EncodeDesc(48000, rate, n_out)
    delay = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    last = torch.zeros((S, n_out, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    out, status = engine.transcode_batch(dec, enc, torch.from_numpy(buf).cuda(), delay, lfsr, chmap, last, csnr)
    engine.sync()
    assert int((status.cpu() & 0x1ff).max()) == 0
    return out.cpu().numpy()[:, :, :enc.frame_bytes()], oflags


# ---------------------------------------------------------------------------------------------------------------------
# views of a frame, read by tests/ac3_syntax.py

METADATA_WIDTHS = (("bsmod", 3), ("cmixlev", 2), ("surmixlev", 2), ("dsurmod", 2), ("dialnorm", 5), ("dialnorm2", 5),
                   ("copyrightb", 1), ("origbs", 1))
BSI_OPTIONS = ("compre", "langcode", "audprodie", "compr2e", "langcod2e", "audprodi2e", "timecod1e", "timecod2e", "addbsie")


def bsi_view(frame):
    """A frame's BSI -> (fields, the bit positions of the fields ac3mi_set_encode_metadata writes).  This encoder sends
    none of the optional fields."""
    P = A.parse_frame(frame, nblocks=0)
    fields = {k: v for k, v in P.fields.items() if P.pos[k] >= P.pos["bsid"]}
    assert not any(fields.get(k, 0) for k in BSI_OPTIONS), fields
    where = [p for k, n in METADATA_WIDTHS if k in P.pos for p in range(P.pos[k], P.pos[k] + n)]
    return fields, where


def _block0(frame, nch):
    P = A.parse_frame(frame, nblocks=1)
    B = P.blocks[0]
    assert P.acmod == ACMOD[nch] and B.fields["cplstre"] == 1
    return P, B, B.fields


def coupling_view(frame, nch, remat=None):
    """cplinu, chincpl (the first channel in the highest bit), begf, endf, [(mstrcplco, [exp << 4 | mant codes])] of
    block 0; with remat=[] a 2/0 frame's rematstr and flag word (rematflg0 in bit 0) are appended to it."""
    P, B, f = _block0(frame, nch)
    if not B.cplinu:
        return 0, None, None, None, None
    assert f.get("phsflginu", 0) == 0 and not any(v for k, v in f.items() if k.startswith("cplbndstrc"))
    co = []
    for ch in range(P.nfchans):
        if B.chincpl[ch]:
            assert f["cplcoe%d" % ch] == 1
            co.append((f["mstrcplco%d" % ch],
                       [f["cplcoexp%d_%d" % (ch, b)] << 4 | f["cplcomant%d_%d" % (ch, b)] for b in range(B.ncplbnd)]))
    if remat is not None and P.acmod == 2:
        remat.append(f["rematstr"])
        remat.append(sum(f.get("rematflg%d" % i, 0) << i for i in range(4)))
    return 1, int("".join(str(v) for v in B.chincpl[:P.nfchans]), 2), B.cplbegf, B.cplendf, co


def uncoupled_view(frame, nch):
    """An uncoupled frame's block 0 -> (the rematrixing flag word, rematflg0 in bit 0, or None where none is sent, [chbwcod
    of each full-bandwidth channel]).  Block 0 sends exponents for every channel, so every channel sends chbwcod."""
    P, B, f = _block0(frame, nch)
    assert B.cplinu == 0 and all(f["chexpstr%d" % ch] for ch in range(P.nfchans))
    flags = sum(f["rematflg%d" % i] << i for i in range(4)) if f.get("rematstr") else None
    return flags, [f["chbwcod%d" % ch] for ch in range(P.nfchans)]


def remat_view(frames):
    """rematstr and the flag word of block 0 of uncoupled 2/0 frames [...][fb] -> two arrays [...]"""
    words = [uncoupled_view(fr, 2)[0] for fr in frames.reshape(-1, frames.shape[-1])]
    rs = np.array([w is not None for w in words], np.uint8).reshape(frames.shape[:-1])
    return rs, np.array([w or 0 for w in words], np.uint8).reshape(frames.shape[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# exponent strategies and coded exponents against tests/exp_strategy_model.py

def check_rows(t1, nch, n):
    """Every channel-frame of an uncoupled call: strategies and exponents on [0, n) are the model's on the d_exponent tap.
    Returns the strategy sequences seen."""
    from tests import exp_strategy_model as X
    S, F = t1["exponent"].shape[:2]
    seqs = []
    for s in range(S):
        for f in range(F):
            for ch in range(nch):
                lfe = nch == 6 and ch == 5
                k, hi = ("lfe", 7) if lfe else ("fbw", n)
                raw = t1["exponent"][s, f, :, ch].astype(np.int64)
                J, st = X.choose(k, raw, 0, hi)
                got = [int(v) for v in t1["exp_strategy"][s, f, :, ch]]
                assert got == st, (s, f, ch, got, st)
                assert np.array_equal(t1["encoded_exp"][s, f, :, ch, :hi], X.coded(k, raw, st, 0, hi)), (s, f, ch)
                seqs.append((k, st))
    return seqs


def cpl_raw(t, s, f, nfbw, begf):
    """The coupling row's raw exponents [6][256] (24 outside [cs, 217)) from the mode-0 taps."""
    from tests import coupling_model as C
    v, xb = C.coupling_rows(t["mdct"][s, f], t["exp_samples"][s, f], nfbw, begf)
    a = np.abs(v)
    lg = np.where(a > 0, np.frexp(np.maximum(a, 1).astype(np.float64))[1] - 1, 0)
    return np.where(a > 0, 23 - lg + xb[:, None], 24).astype(np.int64)


def check_coupled_frames(engine, pcm, nch, begf, c=None, mode0=False):
    """Cost-based strategies with coupling at `begf` (and bandwidth mode 1 at chbwcod `c`): in a coupled frame the coupled
    channels choose over [0, cplstrtmant) (gainrng, no chbwcod) and the coupling channel over [cplstrtmant, cplendmant); its
    exponents are read back from the GPU decoder's coupling plane.  mode0: the strategy-mode-0 call is held to its own model
    too - the channels to bandwidth_model.encode_exp under the tapped strategies, the coupling row to the reference's rule.
    Returns the number of coupled frames."""
    from tests import bandwidth_model as W
    from tests import exp_strategy_model as X
    nfbw = min(nch, 5)
    cs, ce, n = 37 + 12 * begf, 217 if c is None else W.cplendmant(c), 223 if c is None else W.nbc(c)
    kw = dict(cpl=(1, begf)) if c is None else dict(cpl=(1, begf), bw=(1, c))
    frames, t1 = encode(engine, pcm, xs=1, taps=True, **kw)
    frames0, t0 = encode(engine, pcm, xs=0, taps=True, **kw)
    decodes_cleanly(frames, *layout_of(nch), engine=engine)
    _, status, tp = decode(engine, frames, *layout_of(nch), taps=True)
    assert (status & 0x1ff).max() == 0
    if mode0:
        _, status0, tp0 = decode(engine, frames0, *layout_of(nch), taps=True)
        assert (status0 & 0x1ff).max() == 0
    S, F = frames.shape[:2]
    n_cpl = 0
    for s in range(S):
        for f in range(F):
            cplinu = coupling_view(frames[s, f], nch)[0]
            assert cplinu == coupling_view(frames0[s, f], nch)[0]            # (the coupling decision does not change)
            for ch in range(nch):
                lfe = nch == 6 and ch == 5
                k, hi = ("lfe", 7) if lfe else (("cplch", cs) if cplinu else ("fbw", n))
                raw = t0["exponent"][s, f, :, ch].astype(np.int64)
                _, st = X.choose(k, raw, 0, hi)
                assert [int(v) for v in t1["exp_strategy"][s, f, :, ch]] == st, (s, f, ch, k)
                assert np.array_equal(t1["encoded_exp"][s, f, :, ch, :hi], X.coded(k, raw, st, 0, hi)), (s, f, ch)
                if mode0:
                    want = W.encode_exp(raw, t0["exp_strategy"][s, f, :, ch], hi)
                    assert np.array_equal(t0["encoded_exp"][s, f, :, ch, :hi], want), (s, f, ch)
            if cplinu:
                n_cpl += 1
                raw = cpl_raw(t0, s, f, nfbw, begf)
                _, st = X.choose("cpl", raw, cs, ce)
                assert np.array_equal(tp["exp"][s, f, :, 6, cs:ce].astype(np.int64), X.coded("cpl", raw, st, cs, ce)), (s, f)
                if mode0:
                    st0 = X.ref_rule(raw, lo=cs, hi=ce)
                    assert np.array_equal(tp0["exp"][s, f, :, 6, cs:ce].astype(np.int64), X.coded("cpl", raw, st0, cs, ce)), (s, f)
    return n_cpl


# ---------------------------------------------------------------------------------------------------------------------
# content

def content(kind, nch, S, F, seed):
    """[S][F*1536][nch] s16 (WAVE order)."""
    out = []
    n = F * 1536
    for s in range(S):
        rng = np.random.default_rng(seed + s)
        p = H.gen_pcm(F, max(nch, 2), seed=seed + s, kind="music").astype(np.float64)
        base = p[:, 0]
        if kind == "music":                     # one source at per-channel gains + small independent components
            gains = rng.uniform(0.4, 1.0, nch)
            x = np.stack([gains[c] * base + 0.05 * p[:, c % p.shape[1]] * (c > 0) for c in range(nch)], -1)
        elif kind == "identical":
            x = np.stack([base] * nch, -1)
        elif kind == "antiphase":              # (broadband: every coupling band carries energy that cancels in the sum)
            w = base + rng.standard_normal(n) * 2000
            x = np.stack([w, -w], -1)
        elif kind == "noise":
            x = rng.standard_normal((n, nch)) * 3000
        elif kind == "attack":
            t = np.arange(n)
            bed = 3000 * np.sin(2 * np.pi * 200.0 / 48000.0 * t) + 600 * np.sin(2 * np.pi * 2500.0 / 48000.0 * t)
            x = np.stack([bed + rng.integers(-20, 21, n) for _ in range(nch)], -1)
            for f in range(0, F, 2):
                o = 1536 * f + 256 * int(rng.integers(0, 6)) + int(rng.integers(0, 256))
                m = (t >= o) & (t < o + 400)
                x[m, 0] += 16000 * np.sin(2 * np.pi * 3000.0 / 48000.0 * (t[m] - o))
        else:
            raise ValueError(kind)
        out.append(x)
    return np.clip(np.round(np.array(out)), -32768, 32767).astype(np.int16)


CORNER_KINDS = ("silence", "rails", "impulses", "dc", "noise", "rails_identical", "rails_antiphase", "onset")


def corner(kind, nch, F, seed):
    """[F*1536][nch] s16: the level corners.  silence, rails, impulses, dc, noise: the harness's; rails_identical: one
    full-scale square (period 10, -32768 included) in every channel; rails_antiphase: the same with the rails swapped in the
    odd channels (the sum of a pair is -1 everywhere); onset: rails_identical after 1536 + 700 samples of digital silence."""
    if kind in ("silence", "rails", "impulses", "dc", "noise"):
        return H.gen_pcm(F, nch, seed=seed, kind=kind)
    t = np.arange(F * 1536)
    sq = np.where((t // 5) % 2 == 0, 32767, -32768)
    if kind == "rails_identical":
        x = np.stack([sq] * nch, -1)
    elif kind == "rails_antiphase":
        x = np.stack([sq if c % 2 == 0 else -1 - sq for c in range(nch)], -1)
    elif kind == "onset":
        x = np.stack([np.where(t < 1536 + 700, 0, sq)] * nch, -1)
    else:
        raise ValueError(kind)
    return x.astype(np.int16)


def corner_batch(nch, F=3):
    """[8][F*1536][nch]: CORNER_KINDS in order, kind i with seed 900 + i"""
    return np.stack([corner(k, nch, F, 900 + i) for i, k in enumerate(CORNER_KINDS)])


def stereo(kind, S, F, seed):
    """[S][F*1536][2] s16 stereo test content."""
    n = F * 1536
    t = np.arange(n)
    out = []
    for s in range(S):
        rng = np.random.default_rng(seed + s)
        x = rng.standard_normal(n) * 3000
        y = rng.standard_normal(n) * 3000
        if kind == "tones":
            p = H.gen_pcm(F, 2, seed=seed + s, kind="tones").astype(np.float64)
            l, r = p[:, 0], p[:, 1]
        elif kind == "noise":
            l, r = x, y
        elif kind == "identical":
            l = r = x + 4000 * np.sin(2 * np.pi * 1700.0 / 48000.0 * t)
        elif kind == "nearmono":
            l, r = x + 0.05 * y, x - 0.05 * y
        elif kind in ("music_identical", "music_nearmono"):      # tonal content (the harness's music), mono or near it
            p = H.gen_pcm(F, 2, seed=seed + s, kind="music").astype(np.float64)
            l = r = p[:, 0]
            if kind == "music_nearmono":
                l, r = p[:, 0] + 0.05 * p[:, 1], p[:, 0] - 0.05 * p[:, 1]
        elif kind == "changing":                # the correlation changes from block to block
            c = np.repeat(rng.uniform(-1.0, 1.0, n // 256 + 1), 256)[:n]
            l, r = x, c * x + np.sqrt(1 - c * c) * y
        elif kind == "quietR":                  # R 40 dB below L, independent
            l, r = x, 0.01 * y
        elif kind == "silentR":
            l, r = x, 0 * y
        elif kind == "attack":                  # a steady correlated bed, tone bursts in one channel or both: mixed blksw
            bed = 3000 * np.sin(2 * np.pi * 200.0 / 48000.0 * t) + 600 * np.sin(2 * np.pi * 2500.0 / 48000.0 * t)
            l = bed + rng.integers(-20, 21, n)
            r = bed + rng.integers(-20, 21, n)
            for f in range(F):
                o = 1536 * f + 256 * int(rng.integers(0, 6)) + int(rng.integers(0, 256))
                m = (t >= o) & (t < o + 400)
                burst = 16000 * np.sin(2 * np.pi * 3000.0 / 48000.0 * (t[m] - o))
                l[m] += burst
                if f % 2:
                    r[m] += burst
        else:
            raise ValueError(kind)
        out.append(np.stack([l, r], -1))
    return np.clip(np.round(np.array(out)), -32768, 32767).astype(np.int16)


def programme(nch, seed):
    """Tone and noise segments at -60, -40, -31, -20 and -5 dBFS, two frames each, then silence: [1][12*1536][nch]."""
    rng = np.random.default_rng(seed)
    t = np.arange(1536 * 2)
    segs = []
    for i, db in enumerate((-60, -40, -31, -20, -5)):
        a = 32767 * 10 ** (db / 20)
        if i % 2 == 0:
            x = a * np.sin(2 * np.pi * (400 + 300 * i) / 48000 * t)[:, None] * np.ones(nch)
        else:
            x = a / 3 * rng.standard_normal((t.size, nch))
        segs.append(x)
    segs.append(np.zeros((1536 * 2, nch)))
    return np.clip(np.round(np.concatenate(segs)), -32768, 32767).astype(np.int16)[None]


def tones(acmod, lfeon, S, F, seed):
    """[S][F*1536][nch]: every full-bandwidth channel its own three tones and a little noise (a channel swap reads as
    noise), the LFE two tones below 100 Hz (inside its 7 coded bins)."""
    nch = A.NFCHANS[acmod] + lfeon
    t = np.arange(F * 1536)
    out = np.zeros((S, F * 1536, nch))
    for s in range(S):
        rng = np.random.default_rng(seed + 97 * s)
        for c in range(nch):
            if lfeon and c == nch - 1:
                out[s, :, c] = 7000 * np.sin(2 * np.pi * 45 / 48000 * t) + 5000 * np.sin(2 * np.pi * 80 / 48000 * t + 1.0)
                continue
            f = (310 + 530 * c) * rng.uniform(0.95, 1.05) * np.array([1.0, 2.37, 4.11])
            out[s, :, c] = sum(a * np.sin(2 * np.pi * fr / 48000 * t + rng.uniform(0, 6)) for a, fr in zip((6000, 3000, 1500), f))
            out[s, :, c] += rng.standard_normal(F * 1536) * 60
    return np.round(out).astype(np.int16)


def with_lfe(pcm2, seed):
    lfe = tones(1, 1, pcm2.shape[0], pcm2.shape[1] // 1536, seed)[:, :, 1:]
    return np.concatenate([pcm2, lfe], 2)


def pcm(kind, S, F, nch, seed):
    if kind == "attack":
        from tests import block_switch_model as M
        rng = np.random.default_rng(seed)
        onsets = [1536 * f + 256 * int(rng.integers(0, 6)) + int(rng.integers(0, 256)) for f in range(F)]
        return np.stack([M.attack_pcm(F, nch, [o + 37 * s for o in onsets], seed=seed + s) for s in range(S)])
    return np.stack([H.gen_pcm(F, nch, seed=seed + s, kind=kind) for s in range(S)])
