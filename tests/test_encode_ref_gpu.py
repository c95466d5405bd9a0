"""GPU: ac3mi_encode_batch in mode 0 and the drop-in AC3_encode_init / AC3_encode_frame against what the reference's OWN
encoder wrote, from tests/golden/ac3enc_ref.npz alone (recorded from the unmodified src/ac3enc/ac3enc.cpp by
tests/golden/make_golden.py --only ac3enc_ref; layout and findings: tests/test_oracle_vs_ac3enc.py).  Neither the
reference nor the encoder oracle is consulted: inputs are H.gen_pcm streams whose SHA-256 the fixture holds, expected
frames are the recorded bytes (streams recorded in full) or their recorded SHA-256 (the wide matrix).  All exact.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _harness as H

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(H.GOLDEN, "ac3enc_ref.npz"))
with open(os.path.join(H.GOLDEN, "ac3enc_ref.json")) as _f:
    META = json.load(_f)
KINDS = META["kinds"]


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def fixture_pcm(cfg, want_sha):
    pcm = H.gen_pcm(cfg["frames"], cfg["channels"], seed=cfg["seed"], kind=cfg["kind"])
    assert np.array_equal(sha(pcm), want_sha), "H.gen_pcm drifted: %r no longer gives the samples the fixture was recorded from" % (cfg,)
    return pcm


def wide_streams():
    out, row = [], 0
    for c, s in zip(FIX["wide_cfg"], FIX["wide_pcm_sha"]):
        freq, bitrate, nch, cm, kind, seed, frames = (int(x) for x in c)
        out.append(({"freq": freq, "bitrate": bitrate, "channels": nch, "chmap": FIX["wide_chmaps"][cm][:nch].tolist(),
                     "kind": KINDS[kind], "seed": seed, "frames": frames}, s, row))
        row += frames
    return out


def wide_calls():
    """The wide matrix as batched calls: streams of one configuration, channel map and length go into one call."""
    groups = {}
    for cfg, pcm_sha, row in wide_streams():
        key = (cfg["freq"], cfg["bitrate"], cfg["channels"], tuple(cfg["chmap"]), cfg["frames"])
        groups.setdefault(key, []).append((cfg, pcm_sha, row))
    return list(groups.values())


def tail_of(pcm, cfg):
    """last_samples after a stream: the last 256 samples of every coded channel (ac3enc.cpp:1676-1681), [channels][256]."""
    return np.stack([pcm[-256:, cfg["chmap"][ch]] for ch in range(cfg["channels"])]).astype(np.int16)


def gpu_encode(engine, cfg, pcms, last=None, taps=False, split=None):
    """pcms: list of [F*1536][nch] streams of configuration cfg -> frames [S][F][frame bytes][, taps]."""
    import torch
    pkg = H.pkg()
    nch, F, S = cfg["channels"], cfg["frames"], len(pcms)
    desc = pkg.EncodeDesc(cfg["freq"], cfg["bitrate"], nch)
    fb = desc.frame_bytes()
    x = torch.from_numpy(np.stack(pcms).reshape(S, F, 1536, nch)).cuda()
    d_last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    if last is not None:
        d_last = torch.from_numpy(np.ascontiguousarray(last, np.int16).reshape(S, nch, 256)).cuda()
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    if split is None:
        res = engine.encode_batch(desc, x, cfg["chmap"], d_last, csnr, taps=taps)
        engine.sync()
        out = (res[0] if taps else res).cpu().numpy()[:, :, :fb]
        return (out, {k: v.cpu().numpy() for k, v in res[1].items()}) if taps else out
    a = engine.encode_batch(desc, x[:, :split].contiguous(), cfg["chmap"], d_last, csnr)
    b = engine.encode_batch(desc, x[:, split:].contiguous(), cfg["chmap"], d_last, csnr)
    engine.sync()
    return np.concatenate([a.cpu().numpy(), b.cpu().numpy()], axis=1)[:, :, :fb]


@pytest.mark.parametrize("rec", META["full"], ids=[r["name"] for r in META["full"]])
def test_batch_full_records(engine, rec):
    """The streams recorded in full, each beside a second copy of itself in the batch: frames byte for byte, and the
    stage taps against the reference's own arrays (bap on the frames whose search succeeded: after a failed search the
    reference's array holds its last attempt, which the frame's bytes pin)."""
    name, nch = rec["name"], rec["channels"]
    g = lambda k: FIX["full_%s_%s" % (name, k)]
    pcm = fixture_pcm(rec, g("pcm_sha"))
    got, t = gpu_encode(engine, rec, [pcm, pcm], taps=True)
    ok = g("status")[:, 1] == 0
    for s in range(2):
        assert np.array_equal(t["mdct"][s], g("mdct_coef")), "mdct_coef"
        assert np.array_equal(t["exp_samples"][s], g("exp_samples")), "exp_samples"
        assert np.array_equal(t["exp_strategy"][s], g("exp_strategy")), "exp_strategy"
        assert np.array_equal(t["snroffst"][s][:, 0], g("snr")[:, 0]), "csnroffst"
        assert (g("snr")[:, 1:1 + nch] == t["snroffst"][s][:, 1:2]).all(), "fsnroffst"
        for ch in range(nch):
            n = 7 if nch == 6 and ch == 5 else 223
            assert np.array_equal(t["encoded_exp"][s][:, :, ch, :n], g("encoded_exp")[:, :, ch, :n]), "encoded_exp %d" % ch
            assert np.array_equal(t["bap"][s][ok][:, :, ch, :n], g("bap")[ok][:, :, ch, :n]), "bap %d" % ch
        assert np.array_equal(got[s], g("frames")), "stream %d: frames differ in %d bytes, frames %r" % (
            s, int((got[s] != g("frames")).sum()), [f for f in range(rec["frames"]) if not np.array_equal(got[s, f], g("frames")[f])])


def test_batch_wide_matrix(engine):
    """Every stream of the wide matrix - every channel count, sample rate and bit-rate code AC3_encode_init accepts, all
    kinds of input, five channel maps beside the driver's and the identity, starved rates whose searches fail - batched
    by configuration, by the SHA-256 of every frame."""
    bad, frames_checked = [], 0
    for call in wide_calls():
        cfg = call[0][0]
        got = gpu_encode(engine, cfg, [fixture_pcm(c, s) for c, s, _ in call])
        assert got.shape[2] == FIX["wide_status"][call[0][2], 0]             # the size the reference returned
        for i, (c, _, row) in enumerate(call):
            for f in range(c["frames"]):
                frames_checked += 1
                if not np.array_equal(sha(got[i, f]), FIX["wide_digest"][row + f]):
                    bad.append((c, f, "search failed" if FIX["wide_status"][row + f, 1] else "search succeeded"))
    assert frames_checked == len(FIX["wide_digest"])
    assert not bad, "%d of %d frames differ from the reference's, the first: %r" % (len(bad), frames_checked, bad[:4])


def test_batch_long_streams_across_two_calls(engine):
    """The streams of 40 frames and more once more, split across two calls with last_samples and the search state carried
    by the caller."""
    n = 0
    for call in wide_calls():
        cfg = call[0][0]
        if cfg["frames"] < 40:
            continue
        n += 1
        got = gpu_encode(engine, cfg, [fixture_pcm(c, s) for c, s, _ in call], split=cfg["frames"] // 2 - 3)
        for i, (c, _, row) in enumerate(call):
            bad = [f for f in range(c["frames"]) if not np.array_equal(sha(got[i, f]), FIX["wide_digest"][row + f])]
            assert not bad, (c, bad)
    assert n >= 2


@pytest.mark.parametrize("ent", META["reinit"], ids=[e["name"] for e in META["reinit"]])
def test_batch_reinit_with_the_tail_as_incoming_state(engine, ent):
    """The reference's frames of stream B, coded after stream A in one instance (AC3_encode_init does not clear
    last_samples), are what ac3mi_encode_batch gives when A's tail comes in through `last`; with zeros it gives the frames
    of a reference instance that coded nothing before."""
    g = lambda k: FIX["reinit_%s_%s" % (ent["name"], k)]
    a, b = ent["a"], ent["b"]
    pa, pb = fixture_pcm(a, g("a_pcm_sha")), fixture_pcm(b, g("b_pcm_sha"))
    tail = np.zeros((b["channels"], 256), np.int16)
    n = min(a["channels"], b["channels"])
    tail[:n] = tail_of(pa, a)[:n]                       # coded channel ch of B overlaps with coded channel ch of A
    assert np.array_equal(gpu_encode(engine, a, [pa])[0], g("a_frames"))
    assert np.array_equal(gpu_encode(engine, b, [pb], last=tail[None])[0], g("b_frames"))
    assert np.array_equal(gpu_encode(engine, b, [pb])[0], g("b_fresh_frames"))


# ---- the drop-in surface: AC3_encode_init / AC3_encode_frame with the reference's C++ linkage ---------------------------

def dropin(engine):
    init = getattr(engine.lib, "_Z15AC3_encode_initiii")
    frame = getattr(engine.lib, "_Z16AC3_encode_framePhPsS_")
    init.argtypes, init.restype = [H.ci, H.ci, H.ci], H.ci
    frame.argtypes, frame.restype = [H.u8p, H.i16p, H.u8p], H.ci
    return init, frame


def dropin_stream(engine, cfg, pcm):
    """AC3_encode_init + one AC3_encode_frame per frame -> (init's return, frames [F][bytes], returned sizes)."""
    init, frame = dropin(engine)
    size = init(cfg["freq"], cfg["bitrate"], cfg["channels"])
    assert size > 0, cfg
    cm = (ctypes.c_uint8 * 8)(*(tuple(cfg["chmap"]) + (0,) * 8)[:8])
    out, rets = np.zeros((cfg["frames"], 3840), np.uint8), []
    pcm = np.ascontiguousarray(pcm)
    for f in range(cfg["frames"]):
        rets.append(frame(H.P(out[f], H.u8p), ctypes.cast(pcm.ctypes.data + f * 1536 * cfg["channels"] * 2, H.i16p), cm))
    assert not out[:, size:].any(), "AC3_encode_frame wrote behind the frame"
    return size, out[:, :size], rets


def test_dropin_full_records(engine):
    """Every stream recorded in full through the drop-in, among them the two whose search fails: same bytes, and the
    reference's return value (the frame size, after a failed search too)."""
    for rec in META["full"]:
        g = lambda k: FIX["full_%s_%s" % (rec["name"], k)]
        size, got, rets = dropin_stream(engine, rec, fixture_pcm(rec, g("pcm_sha")))
        assert rets == g("status")[:, 0].tolist() and size == rets[0], (rec["name"], rets)
        assert np.array_equal(got, g("frames")), (rec["name"], [f for f in range(rec["frames"]) if not np.array_equal(got[f], g("frames")[f])])


def test_dropin_init_decisions(engine):
    """AC3_encode_init's decision and returned size for every recorded argument triple (ac3mi_encode_frame_bytes, which
    the drop-in's init returns, for all of them; the drop-in itself for every 16th)."""
    init, _ = dropin(engine)
    pkg = H.pkg()
    bad = []
    for i, ((freq, bitrate, nch), want) in enumerate(zip(FIX["init_args"].tolist(), FIX["init_ret"].tolist())):
        got = pkg.EncodeDesc(freq, bitrate, nch).frame_bytes()
        if got != want or (i % 16 == 0 and init(freq, bitrate, nch) != want):
            bad.append((freq, bitrate, nch, want, got))
    assert not bad, bad[:10]


def test_dropin_wide_matrix_sample(engine):
    """Every fifth stream of the wide matrix and the long ones, frame by frame through the drop-in."""
    bad, n = [], 0
    for i, (cfg, pcm_sha, row) in enumerate(wide_streams()):
        if i % 5 and cfg["frames"] < 40:
            continue
        size, got, rets = dropin_stream(engine, cfg, fixture_pcm(cfg, pcm_sha))
        n += cfg["frames"]
        for f in range(cfg["frames"]):
            if rets[f] != FIX["wide_status"][row + f, 0] or not np.array_equal(sha(got[f]), FIX["wide_digest"][row + f]):
                bad.append((cfg, f, rets[f]))
    assert n > 900
    assert not bad, "%d of %d frames differ from the reference's, the first: %r" % (len(bad), n, bad[:4])


@pytest.mark.parametrize("ent", META["reinit"], ids=[e["name"] for e in META["reinit"]])
def test_dropin_reinit_starts_clean(engine, ent):
    """Stream A, AC3_encode_init again, stream B through the drop-in: B's frames are those of a reference instance that
    coded nothing before (the deliberate deviation of INTEGRATION.md: the reference would carry A's tail into B's first
    block), not the ones the reference gives in this sequence."""
    g = lambda k: FIX["reinit_%s_%s" % (ent["name"], k)]
    a, b = ent["a"], ent["b"]
    _, fa, _ = dropin_stream(engine, a, fixture_pcm(a, g("a_pcm_sha")))
    _, fb, _ = dropin_stream(engine, b, fixture_pcm(b, g("b_pcm_sha")))
    assert np.array_equal(fa, g("a_frames"))
    assert np.array_equal(fb, g("b_fresh_frames"))
    assert not np.array_equal(fb[0], g("b_frames")[0])
