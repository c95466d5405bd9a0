"""The BS.1770 meter of include/ac3mi.h (ac3mi_loudness_*) restated in numpy, float64, sample by sample: K-weighting from
the bilinear design, 100 ms hops, 400 ms blocks, the 900-bin state with its read-out rule - and, beside it, the plain BS.1770
gating over the stored list of block energies, which the bins approximate inside the one bin the relative gate cuts.
numpy only.  The engine filters a frame in 64 segments of 24 samples; this model runs the recursion as written."""
import numpy as np

RATES = (48000, 44100, 32000)
WEIGHT = (0.0, 1.0, 1.41)           # by role: not measured, front / mono, surround
BINS = 900
EMPTY = 1                           # AC3MI_LOUDNESS_EMPTY

# the 48 kHz table of ITU-R BS.1770, as printed: shelf b0 b1 b2 a1 a2, high-pass a1 a2
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621)

# the engine's state record (loudness_rule.h, LoudState), for the tests that write states and read the engine's
STATE_DTYPE = np.dtype([("bq", "<f8", (6, 4)), ("hop_sum", "<f8"), ("hops", "<f8", (3,)), ("max_block", "<f8"), ("pos", "<u4"),
                        ("hop_count", "<u4"), ("blocks", "<u4"), ("blocks_abs", "<u4"), ("count", "<u4", (BINS,)), ("sum", "<f8", (BINS,))])


def coefs(fs):
    """shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (a0 = 1) for sample rate fs"""
    f0, g, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = np.tan(np.pi * f0 / fs)
    vh = 10.0 ** (g / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / q + k * k
    shelf = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]
    f0, q = 38.13547087602444, 0.5003270373238773
    k = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + k / q + k * k
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0])


def edges():
    """E_b, b = 0..900: bin b holds the blocks with E_b <= z < E_(b+1)"""
    return 10.0 ** ((-70.0 + 0.1 * np.arange(BINS + 1) + 0.691) / 10.0)


def dialnorm_thresholds():
    """T_d, d = 1..30"""
    return 10.0 ** ((-np.arange(1, 31) - 0.5 + 0.691) / 10.0)


EDGES = edges()
THRESHOLDS = dialnorm_thresholds()


def lkfs(energy):
    return -0.691 + 10.0 * np.log10(energy)


def kweight(x, coef, state=None):
    """The two biquads over the last axis of x (float64 [..., n]), transposed direct form II, all leading axes at once.
    coef [10] or [..., 10] (one set per leading index); state [..., 4] = shelf s1 s2, high-pass s1 s2 (None: zeros)
    -> (y [..., n], the state behind the last sample)"""
    x = np.asarray(x, np.float64)
    c = np.broadcast_to(np.asarray(coef, np.float64), x.shape[:-1] + (10,))
    b0, b1, b2, a1, a2, d0, d1, d2, c1, c2 = (c[..., i] for i in range(10))
    st = np.zeros(x.shape[:-1] + (4,)) if state is None else np.array(state, np.float64)
    s1, s2, t1, t2 = (st[..., i].copy() for i in range(4))
    y = np.empty_like(x)
    for n in range(x.shape[-1]):
        xn = x[..., n]
        y1 = b0 * xn + s1
        s1 = b1 * xn - a1 * y1 + s2
        s2 = b2 * xn - a2 * y1
        yn = d0 * y1 + t1
        t1 = d1 * y1 - c1 * yn + t2
        t2 = d2 * y1 - c2 * yn
        y[..., n] = yn
    return y, np.stack([s1, s2, t1, t2], axis=-1)


def bin_of(z):
    """-1 below the absolute gate, else the b with E_b <= z < E_(b+1), 899 from E_900 on"""
    if not z >= EDGES[0]:
        return -1
    return min(int(np.searchsorted(EDGES, z, side="right")) - 1, BINS - 1)


def dialnorm_of(mean_energy):
    return 1 + int(np.sum(mean_energy < THRESHOLDS))


def read_bins(count, total):
    """the read-out rule on the bins -> dict(mean_energy, blocks_rel, dialnorm, flags, lkfs, gamma, cut: the bin the gate
    cuts or None)"""
    count = np.asarray(count, np.int64)
    total = np.asarray(total, np.float64)
    n = int(count.sum())
    gamma = 0.1 * (float(total.sum()) / n) if n else 0.0
    keep = (count > 0) & (EDGES[:-1] >= gamma)
    cut = None
    if n:
        b = int(np.searchsorted(EDGES, gamma, side="left")) - 1         # E_b < gamma <= E_(b+1)
        if 0 <= b < BINS and EDGES[b] < gamma < EDGES[b + 1]:
            cut = b
            if count[b] and total[b] / count[b] >= gamma:
                keep[b] = True
    k = int(count[keep].sum())
    if not k:
        return dict(mean_energy=0.0, blocks_rel=0, dialnorm=31, flags=EMPTY, lkfs=-70.0, gamma=gamma, cut=cut)
    mean = float(total[keep].sum()) / k
    return dict(mean_energy=mean, blocks_rel=k, dialnorm=dialnorm_of(mean), flags=0, lkfs=float(lkfs(mean)), gamma=gamma, cut=cut)


def read_plain(z):
    """plain BS.1770 gating over the list of block energies -> dict(mean_energy, blocks_rel, gamma, lkfs), mean_energy 0 if
    nothing passes"""
    z = np.asarray(z, np.float64)
    za = z[z >= EDGES[0]]
    if not len(za):
        return dict(mean_energy=0.0, blocks_rel=0, gamma=0.0, lkfs=-70.0)
    gamma = 0.1 * float(za.mean())
    zr = za[za >= gamma]
    mean = float(zr.mean())
    return dict(mean_energy=mean, blocks_rel=len(zr), gamma=gamma, lkfs=float(lkfs(mean)))


def programme(seed, nframes, channels, amp, quiet=0.0562, quiet_part=0.45, loud_slot=None):
    """Test content: seeded uniform noise, int16 [nframes * 1536][channels], peak amp (of full scale) with the first
    quiet_part of it 25 dB down - a programme whose quiet part the relative gate removes; loud_slot: a slot at full scale
    throughout (an LFE that must not be measured)"""
    rng = np.random.default_rng(seed)
    n = nframes * 1536
    x = rng.integers(-32767, 32768, (n, channels)).astype(np.float64) * amp
    x[:int(n * quiet_part)] *= quiet
    if loud_slot is not None:
        x[:, loud_slot] = rng.integers(-32767, 32768, n)
    return np.round(x).astype(np.int16)


def run_batch(pcm, fs, roles, meters=None):
    """Many streams at once (one pass of the sample loop for all of them): pcm int16 [S][n][channels], fs one rate or one per
    stream, roles shared -> the meters (new ones, or `meters` continued)"""
    pcm = np.asarray(pcm)
    S = pcm.shape[0]
    fs = [fs] * S if np.isscalar(fs) else list(fs)
    if meters is None:
        meters = [Meter(f, roles) for f in fs]
    idx = [c for c, r in enumerate(roles) if r]
    if idx and pcm.shape[1]:
        x = pcm[:, :, idx].transpose(0, 2, 1).astype(np.float64) / 32768.0
        coef = np.stack([m.coef for m in meters])[:, None, :]
        y, st = kweight(x, coef, np.stack([m.bq[idx] for m in meters]))
        p = np.zeros((S, pcm.shape[1]))
        for k, c in enumerate(idx):
            p += WEIGHT[roles[c]] * y[:, k] * y[:, k]
    else:
        p = np.zeros((S, pcm.shape[1]))
    for s, m in enumerate(meters):
        if idx and pcm.shape[1]:
            m.bq[idx] = st[s]
        m.push_power(p[s])
    return meters


class Meter:
    """One stream's meter in the engine's state form; `z` additionally keeps every block energy, for the plain gating."""

    def __init__(self, fs, roles):
        assert fs in RATES
        self.fs, self.hop, self.roles = fs, fs // 10, list(roles)
        self.coef = coefs(fs)
        self.bq = np.zeros((6, 4))
        self.hop_sum, self.hops, self.max_block = 0.0, [0.0, 0.0, 0.0], 0.0
        self.pos = self.hop_count = self.blocks = self.blocks_abs = 0
        self.count = np.zeros(BINS, np.uint32)
        self.sum = np.zeros(BINS)
        self.z = []

    def power(self, pcm):
        """pcm int16 [n][channels] -> the weighted K-weighted power per sample instant [n]; moves the filter states"""
        pcm = np.asarray(pcm)
        assert pcm.ndim == 2 and pcm.shape[1] == len(self.roles)
        p = np.zeros(pcm.shape[0])
        for c, role in enumerate(self.roles):
            if role:
                y, self.bq[c] = kweight(pcm[:, c].astype(np.float64) / 32768.0, self.coef, self.bq[c])
                p += WEIGHT[role] * y * y
        return p

    def push_power(self, p):
        """the hops, blocks and bins over the next len(p) sample instants of weighted power"""
        i = 0
        while i < len(p):
            m = min(self.hop - self.pos, len(p) - i)
            self.hop_sum += float(np.sum(p[i:i + m]))
            self.pos += m
            i += m
            if self.pos == self.hop:
                h = self.hop_sum
                self.hop_count += 1
                if self.hop_count >= 4:
                    z = (self.hops[0] + self.hops[1] + self.hops[2] + h) / (4.0 * self.hop)
                    self.z.append(z)
                    self.blocks += 1
                    self.max_block = max(self.max_block, z)
                    b = bin_of(z)
                    if b >= 0:
                        self.blocks_abs += 1
                        self.count[b] += 1
                        self.sum[b] += z
                self.hops = [self.hops[1], self.hops[2], h]
                self.hop_sum, self.pos = 0.0, 0

    def push(self, pcm):
        self.push_power(self.power(pcm))

    def record(self):
        """the state as the engine's record (STATE_DTYPE)"""
        r = np.zeros((), STATE_DTYPE)
        r["bq"], r["hop_sum"], r["hops"], r["max_block"] = self.bq, self.hop_sum, self.hops, self.max_block
        r["pos"], r["hop_count"], r["blocks"], r["blocks_abs"] = self.pos, self.hop_count, self.blocks, self.blocks_abs
        r["count"], r["sum"] = self.count, self.sum
        return r

    def read(self):
        out = read_bins(self.count, self.sum)
        out.update(blocks=self.blocks, blocks_abs=self.blocks_abs, max_block_energy=self.max_block)
        return out

    def margin(self):
        """the smallest relative distance of any block energy from a bin edge, the absolute gate or the relative gate, and of
        the mean from a dialnorm threshold: what decides whether two float64 evaluations can disagree on a decision"""
        r = self.read()
        z = np.asarray(self.z)
        d = [np.inf]
        if len(z):
            d.append(np.min(np.abs(z[:, None] - EDGES[None, :]) / EDGES[None, :]))
            if r["gamma"] > 0:
                d.append(np.min(np.abs(z - r["gamma"]) / r["gamma"]))
        if r["blocks_rel"]:
            d.append(np.min(np.abs(r["mean_energy"] - THRESHOLDS) / THRESHOLDS))
        return float(min(d))
