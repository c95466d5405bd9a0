#!/usr/bin/env python3
"""How many WINDOW sweeps (sixteen consecutive offsets costed at once, csrc/snr_window.h) does enc_search_kernel<1> need to replay
the reference's SNR-offset search exactly?  CPU only, on the oracle's spare-bit curves like profiles/search_sim.py, whose
`curves`, `Search` and `reference` this file uses.  first_lo / next_lo restate win_first_lo / win_next_lo of snr_window.h; `run`
restates the kernel's loop around them.  `python profiles/search_window_sim.py [frames]` prints the mean and the histogram of
sweeps per frame for transcoded, fresh-cold and fresh-warm content, beside the three-offset policy's on the same frames."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from search_sim import Search, curves, reference, run as run3     # noqa: E402

WIN_N = 16
HINT_BELOW, COLD_LO, WARM_BELOW = 5, 176, 6
LINE_SWEEPS, ASK_SWEEPS = 4, 7


def clamp_lo(lo):
    return 0 if lo < 0 else 1008 if lo > 1008 else lo


def first_lo(hint, cold, g_prev, hint_below=HINT_BELOW, cold_lo=COLD_LO, warm_below=WARM_BELOW):
    return clamp_lo(hint - hint_below if hint and hint > 0 else cold_lo if cold else g_prev - warm_below)


def next_lo(sweeps, gl, sl, gh, sh, slope15, cmin, cmax, gq):
    if sweeps >= ASK_SWEEPS: return clamp_lo(gq - 8)
    around = clamp_lo(cmin - WIN_N if gq < cmin else cmax + 1 if gq > cmax else gq - 8)
    if gl >= 0 and gh >= 0:
        if gh <= gl + 1 or gq <= gl or gq >= gh: return around
        w = gh - gl
        if w - 1 <= WIN_N: return clamp_lo(gl + 1)
        est = gl + (w >> 1)
        if sweeps < LINE_SWEEPS: est = gl + (w * sl + ((sl - sh) >> 1)) // (sl - sh)
        lo = min(max(est - 8, gl + 1), gh - WIN_N)
        return clamp_lo(lo)
    if (gq <= gl) if gh < 0 else (gq >= gh): return around
    if gh < 0:
        est = gl + (15 * sl) // slope15 if slope15 > 0 else 1023
        if sweeps >= LINE_SWEEPS: est = gl + ((1024 - gl) >> 1)
        est = min(est, 1023)
        return clamp_lo(max(est - 8, gl + 1))
    est = gh - (15 * -sh) // slope15 if slope15 > 0 else 0
    if sweeps >= LINE_SWEEPS: est = gh >> 1
    est = max(est, 0)
    return clamp_lo(min(est - 7, gh - WIN_N))


def run(curve, start, hint=None, fsnr_prev=0, **first_kw):
    """(sweeps, (csnr, fsnr)) from the stream state (start, fsnr_prev); hint: the source frame's offsets (a transcode)"""
    extra = curve.extra
    costed = {}
    fit_hi, fail_lo = -1, 1 << 20
    gl = gh = -1
    sl = sh = 0
    slope15 = 0
    cmin, cmax = 1 << 20, -1
    ss = Search(start)
    sweeps = 0
    cold = start == 40 and fsnr_prev == 0

    def lookup(g):
        if g <= fit_hi: return True
        if g >= fail_lo: return False
        return costed.get(g)

    while True:
        q = None
        while True:
            q = ss.next()
            if q is None: break
            v = lookup(16 * q[0] + q[1])
            if v is None: break
            ss.consume(v)
        if q is None: break
        gq = 16 * q[0] + q[1]
        if sweeps == 0:
            lo = first_lo(hint if cold else None, cold, 16 * start + fsnr_prev, **first_kw)
        else:
            lo = next_lo(sweeps, gl, sl, gh, sh, slope15, cmin, cmax, gq)
        sweeps += 1
        assert sweeps <= 64, "the window rule does not end"
        for g in range(lo, lo + WIN_N):
            sp, e6 = int(curve[g]), int(extra[g])
            costed[g] = sp >= 0
            if 6 * sp >= 414 - e6 and g > fit_hi: fit_hi = g
            if 6 * sp < -e6 and g < fail_lo: fail_lo = g
            if sp >= 0 and g > gl: gl, sl = g, sp
            if sp < 0 and (gh < 0 or g < gh): gh, sh = g, sp
        slope15 = int(curve[lo]) - int(curve[lo + 15])
        cmin, cmax = min(cmin, lo), max(cmax, lo + 15)
    return sweeps, (ss.c, ss.f)


def table(name, sweeps, base):
    n = len(sweeps)
    hist = {}
    for s in sweeps: hist[s] = hist.get(s, 0) + 1
    print("%-34s window %.2f sweeps per frame (three-offset policy %.2f); histogram %s" % (
        name, sum(sweeps) / n, sum(base) / n, " ".join("%d:%d" % (k, hist[k]) for k in sorted(hist))))


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    tr, trb, cold, coldb, warm, warmb, land, delta = [], [], [], [], [], [], [], []
    for seed in (7, 99):
        for c, g_src in curves(n, seed=seed, second_gen=True, with_source=True):
            want = reference(c, 40)
            sw, got = run(c, 40, hint=g_src)
            assert got == want
            tr.append(sw); trb.append(run3(c, 40, "probe", hint=g_src)[0])
            delta.append(16 * want[0] + want[1] - g_src)
        prev = None
        for c in curves(n, seed=seed):
            want = reference(c, 40)
            sw, got = run(c, 40)
            assert got == want
            cold.append(sw); coldb.append(run3(c, 40, "probe")[0])
            land.append(16 * want[0] + want[1])
            # warm: the stream state a previous frame of like material leaves (the previous curve's result)
            if prev is not None:
                sw, got = run(c, prev[0], fsnr_prev=prev[1])
                assert got == reference(c, prev[0])
                warm.append(sw); warmb.append(run3(c, prev[0], "probe")[0])
            prev = want
    table("transcoded (hint = source offsets)", tr, trb)
    table("fresh, cold", cold, coldb)
    table("fresh, warm", warm, warmb)
    print("the re-encode lands %d .. %d steps from its source; fresh frames land at g = %d .. %d, mean %.0f" % (
        min(delta), max(delta), min(land), max(land), sum(land) / len(land)))
