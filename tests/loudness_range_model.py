"""The loudness range meter of include/ac3mi.h (ac3mi_loudness_range_*, EBU Tech 3342) restated in numpy, float64, on top of
tests/loudness_model.Meter, which supplies the closed hop energies: the ring of 30 hops, the 3 s block as the ordered sum of
the ring, the bins, the read-out on the bins - and, beside it, plain Tech 3342: both gates and both percentiles over the stored
list of block energies, which the bins approximate to 0.1 LU.
numpy only; where scipy.signal.lfilter can be imported, long signals are filtered with it (the same transposed direct form II
recursion in C), else with the model's sample loop."""
import numpy as np

from tests import loudness_model as M

HOPS = 30                           # hops in a 3 s block
EMPTY = 1                           # AC3MI_LOUDNESS_RANGE_EMPTY

# the engine's range state record (loudness_rule.h, RangeState)
RANGE_STATE_DTYPE = np.dtype([("ring", "<f8", (HOPS,)), ("sum_abs", "<f8"), ("max_short", "<f8"), ("hops", "<u4"), ("ring_pos", "<u4"),
                              ("blocks", "<u4"), ("blocks_abs", "<u4"), ("count", "<u4", (M.BINS,))])
assert RANGE_STATE_DTYPE.itemsize == 3872

try:
    from scipy.signal import lfilter as _lfilter
except ImportError:                 # the sample loop does it
    _lfilter = None
HAVE_LFILTER = _lfilter is not None


def rank(n, pct):
    """the 0-based rank, ascending, of the pct-th percentile among n blocks: (n - 1) pct / 100 + 0.5, truncated, in integers"""
    return (pct * (n - 1) + 50) // 100


def bin_lkfs(b):
    """a bin's centre, -70 + 0.1 b + 0.05, as the engine evaluates it: one division of integers, rounded to float32"""
    return np.float32((10 * int(b) - 6995) / 100.0)


def max_short_lkfs(energy):
    return np.float32(-0.691 + 10.0 * np.log10(energy)) if energy > 0 else np.float32(-200.0)


def read_bins(count, sum_abs, blocks_abs):
    """the read-out rule on the bins -> dict(blocks_rel, lra_tenths, low_bin, high_bin, flags, lra, low_lkfs, high_lkfs, gamma,
    cut: the bin the gate cuts or None, cut_count: the counted blocks in it)"""
    count = np.asarray(count, np.uint64).astype(object)             # Python integers: a garbage state does not overflow them
    gamma = 0.01 * (float(sum_abs) / int(blocks_abs)) if int(blocks_abs) else 0.0
    keep = np.array([c != 0 for c in count]) & (M.EDGES[1:] > gamma)        # (a gate that is not a number keeps nothing)
    cut, cut_count = None, 0
    b = int(np.searchsorted(M.EDGES, gamma, side="left")) - 1       # E_b < gamma <= E_(b+1)
    if gamma == gamma and 0 <= b < M.BINS and M.EDGES[b] < gamma < M.EDGES[b + 1]:
        cut, cut_count = b, int(count[b])
    n = int(sum(count[keep]))
    out = dict(blocks_rel=min(n, 0xffffffff), gamma=gamma, cut=cut, cut_count=cut_count)
    if not n:
        out.update(lra_tenths=0, low_bin=0, high_bin=0, flags=EMPTY, lra=np.float32(0), low_lkfs=np.float32(-70), high_lkfs=np.float32(-70))
        return out
    cum = np.cumsum(np.where(keep, count, 0))
    lo = int(np.argmax(cum > rank(n, 10)))
    hi = int(np.argmax(cum > rank(n, 95)))
    out.update(lra_tenths=hi - lo, low_bin=lo, high_bin=hi, flags=0, lra=np.float32(0.1) * np.float32(hi - lo), low_lkfs=bin_lkfs(lo),
               high_lkfs=bin_lkfs(hi))
    return out


def read_plain(z3):
    """plain Tech 3342 over the list of 3 s block energies: absolute gate -70 LUFS, relative gate -20 LU under the mean of
    what passed, then the 10th and 95th percentile of the sorted rest at rank (n - 1) p + 0.5 truncated
    -> dict(lra: LU, blocks_rel, gamma, low, high: energies); lra 0 if nothing passes"""
    z = np.asarray(z3, np.float64)
    za = z[z >= M.EDGES[0]]
    if not len(za):
        return dict(lra=0.0, blocks_rel=0, gamma=0.0, low=0.0, high=0.0)
    gamma = 0.01 * float(za.mean())
    zr = np.sort(za[za >= gamma])
    n = len(zr)
    lo, hi = float(zr[rank(n, 10)]), float(zr[rank(n, 95)])
    return dict(lra=10.0 * np.log10(hi / lo), blocks_rel=n, gamma=gamma, low=lo, high=hi)


class RangeMeter(M.Meter):
    """One stream's two meters: loudness_model.Meter as it is (its state is the engine's loudness state) and, fed with every
    hop it closes, the range meter in the engine's state form (the r_ fields); `z3` additionally keeps every 3 s block
    energy, for the plain rule."""

    def __init__(self, fs, roles):
        super().__init__(fs, roles)
        self.ring = np.zeros(HOPS)
        self.sum_abs, self.max_short = 0.0, 0.0
        self.r_hops = self.ring_pos = self.r_blocks = self.r_blocks_abs = 0
        self.r_count = np.zeros(M.BINS, np.uint32)
        self.z3 = []

    def push_power(self, p):
        """Meter.push_power hop by hop (it cuts at the same boundaries itself: the same sums), each closed hop into the ring"""
        i = 0
        while i < len(p):
            m = min(self.hop - self.pos, len(p) - i)
            before = self.hop_count
            super().push_power(p[i:i + m])
            i += m
            if self.hop_count != before:
                self.push_hop(self.hops[2])

    def push_hop(self, h):
        pos = self.ring_pos % HOPS
        self.r_hops = min(self.r_hops + 1, 0xffffffff)
        self.ring[pos] = h
        self.ring_pos = (pos + 1) % HOPS
        if self.r_hops < HOPS:
            return
        s = float(self.ring[(pos + 1) % HOPS])          # oldest first, one addition after the other
        for k in range(2, HOPS + 1):
            s = s + float(self.ring[(pos + k) % HOPS])
        z3 = s / (30.0 * self.hop)
        self.z3.append(z3)
        self.r_blocks += 1
        self.max_short = max(self.max_short, z3)
        b = M.bin_of(z3)
        if b >= 0:
            self.r_blocks_abs += 1
            self.sum_abs += z3
            self.r_count[b] += 1

    def range_record(self):
        """the range state as the engine's record (RANGE_STATE_DTYPE)"""
        r = np.zeros((), RANGE_STATE_DTYPE)
        r["ring"], r["sum_abs"], r["max_short"], r["hops"], r["ring_pos"] = self.ring, self.sum_abs, self.max_short, self.r_hops, self.ring_pos
        r["blocks"], r["blocks_abs"], r["count"] = self.r_blocks, self.r_blocks_abs, self.r_count
        return r

    def range_read(self):
        out = read_bins(self.r_count, self.sum_abs, self.r_blocks_abs)
        out.update(blocks=self.r_blocks, blocks_abs=self.r_blocks_abs, max_short_energy=self.max_short,
                   max_short_lkfs=max_short_lkfs(self.max_short))
        return out

    def range_plain(self):
        return read_plain(self.z3)

    def range_margin(self):
        """the smallest relative distance of any 3 s block energy from a bin edge (the absolute gate is one), and of the
        relative gate from a bin edge: what decides whether two float64 evaluations can disagree on a decision"""
        r = self.range_read()
        d = [np.inf]
        z = np.asarray(self.z3)
        if len(z):
            d.append(np.min(np.abs(z[:, None] - M.EDGES[None, :]) / M.EDGES[None, :]))
        if r["gamma"] > 0:
            d.append(np.min(np.abs(r["gamma"] - M.EDGES) / M.EDGES))
        return float(min(d))


def read_record(rec):
    """range_read of a state record (RANGE_STATE_DTYPE), garbage included: what the engine's read-out must say"""
    out = read_bins(rec["count"], float(rec["sum_abs"]), int(rec["blocks_abs"]))
    out.update(blocks=int(rec["blocks"]), blocks_abs=int(rec["blocks_abs"]), max_short_energy=float(rec["max_short"]),
               max_short_lkfs=max_short_lkfs(float(rec["max_short"])))
    return out


def kweight(x, coef, state=None):
    """loudness_model.kweight; with scipy, the two biquads through lfilter (one row of the leading axes at a time)"""
    if _lfilter is None:
        return M.kweight(x, coef, state)
    x = np.asarray(x, np.float64)
    c = np.broadcast_to(np.asarray(coef, np.float64), x.shape[:-1] + (10,)).reshape(-1, 10)
    st = np.zeros((c.shape[0], 4)) if state is None else np.array(state, np.float64).reshape(-1, 4)
    xf = x.reshape(-1, x.shape[-1])
    y = np.empty_like(xf)
    for i in range(xf.shape[0]):
        y1, st[i, 0:2] = _lfilter(c[i, 0:3], np.array([1.0, c[i, 3], c[i, 4]]), xf[i], zi=st[i, 0:2])
        y[i], st[i, 2:4] = _lfilter(c[i, 5:8], np.array([1.0, c[i, 8], c[i, 9]]), y1, zi=st[i, 2:4])
    return y.reshape(x.shape), st.reshape(x.shape[:-1] + (4,))


def run_batch(pcm, fs, roles, meters=None):
    """loudness_model.run_batch with RangeMeters: pcm int16 [S][n][channels], fs one rate or one per stream, roles shared ->
    the meters (new ones, or `meters` continued)"""
    pcm = np.asarray(pcm)
    S = pcm.shape[0]
    fs = [fs] * S if np.isscalar(fs) else list(fs)
    if meters is None:
        meters = [RangeMeter(f, roles) for f in fs]
    if _lfilter is None:
        return M.run_batch(pcm, fs, roles, meters)
    idx = [c for c, r in enumerate(roles) if r]
    for s, m in enumerate(meters):
        p = np.zeros(pcm.shape[1])
        if idx and pcm.shape[1]:
            y, m.bq[idx] = kweight(pcm[s][:, idx].T.astype(np.float64) / 32768.0, m.coef, m.bq[idx])
            for k, c in enumerate(idx):
                p += M.WEIGHT[roles[c]] * y[k] * y[k]
        m.push_power(p)
    return meters


def dipped(pcm, first=0.70, last=0.85, db=12.0):
    """int16 [n][channels] with its samples from `first` to `last` of its length `db` down"""
    x = pcm.astype(np.float64)
    n = len(x)
    x[int(n * first):int(n * last)] *= 10.0 ** (-db / 20.0)
    return np.round(x).astype(np.int16)


def r128_sine(levels, seconds=20, fs=32000, shift_db=-0.05):
    """Tech 3342's synthetic cases: a 1 kHz stereo sine, `seconds` at each of `levels` (LUFS, taken as each channel's peak in
    dBFS as the Recommendation states them), every level moved by shift_db so that the plateaus lie mid-bin
    -> int16 [seconds * fs * len(levels)][2]"""
    t = np.arange(seconds * fs * len(levels))
    amp = np.repeat(10.0 ** ((np.asarray(levels, np.float64) + shift_db) / 20.0), seconds * fs)
    x = np.round(32768.0 * amp * np.sin(2.0 * np.pi * 1000.0 * t / fs))
    return np.clip(x, -32768, 32767).astype(np.int16)[:, None].repeat(2, axis=1)
