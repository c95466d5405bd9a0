"""The true-peak meter of include/ac3mi.h (ac3mi_truepeak_*) restated in numpy int64: BS.1770-4 Annex 2's 48-tap, 4x
interpolator as four 12-tap phases with coefficients times 8192, the maximum |y| with its first index, the sample peak and
the full-scale count per slot - in a whole-signal form (one convolution per phase) and in the engine's state form, whose
record has the engine's layout.  numpy only; nothing here rounds."""
import numpy as np

H0 = (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
H1 = (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
H = np.array([H0, H1, H1[::-1], H0[::-1]], np.int64)        # H[p][k]: y[4 n + p] = sum_k H[p][k] x[n - k]
UNIT = 1 << 28                                              # y's unit is 2^-28 of full scale (2^-15 of x, 2^-13 of H)
EMPTY, OVER = 1, 2                                          # AC3MI_TRUEPEAK_EMPTY, AC3MI_TRUEPEAK_OVER
U32 = 0xffffffff

# the engine's state record (truepeak_rule.h, TruePeakState) and result record (ac3mi_truepeak_result)
STATE_DTYPE = np.dtype([("samples", "<u8"), ("index", "<u8", (6,)), ("true_peak", "<u4", (6,)), ("sample_peak", "<u4", (6,)),
                        ("full_scale", "<u4", (6,)), ("hist", "<i2", (6, 11)), ("measured", "u1"), ("reserved", "u1", (3,))])
assert STATE_DTYPE.itemsize == 264


def oversample(x):
    """x int [n] (x[m] = 0 for m < 0) -> y int64 [4 n], y[4 m + p] = sum_k H[p][k] x[m - k]: one convolution per phase"""
    x = np.asarray(x, np.int64)
    y = np.empty((len(x), 4), np.int64)
    for p in range(4):
        y[:, p] = np.convolve(x, H[p])[:len(x)]
    return y.reshape(-1)


def whole(x):
    """the rule over a whole slot signal -> dict(true_peak, index, sample_peak, full_scale)"""
    x = np.asarray(x, np.int64)
    a = np.abs(oversample(x))
    peak = int(a.max()) if len(a) else 0
    return dict(true_peak=peak, index=int(np.argmax(a)) if peak else 0, sample_peak=int(np.abs(x).max()) if len(x) else 0,
                full_scale=int(np.sum((x == -32768) | (x == 32767))))


def ceiling(dbtp):
    """floor(2^28 10^(dbtp / 20)) clamped to a u32"""
    return int(min(max(np.floor(UNIT * 10.0 ** (dbtp / 20.0)), 0), U32))


def db(value, full):
    return float(np.float32(20.0 * np.log10(value / full))) if value else -200.0


class Meter:
    """One stream's meter in the engine's state form."""

    def __init__(self, roles):
        self.roles = list(roles)
        self.samples = 0
        self.index, self.true_peak, self.sample_peak, self.full_scale = [0] * 6, [0] * 6, [0] * 6, [0] * 6
        self.hist = np.zeros((6, 11), np.int64)
        self.measured = 0

    def push(self, pcm):
        """pcm int16 [n][channels]: the next n sample instants"""
        pcm = np.asarray(pcm)
        assert pcm.ndim == 2 and pcm.shape[1] == len(self.roles)
        n = pcm.shape[0]
        for c, role in enumerate(self.roles):
            if not role:
                continue
            x = np.concatenate([self.hist[c], pcm[:, c].astype(np.int64)])
            a = np.abs(oversample(x))[44:]                  # the history's own outputs are not new (and assume zeros before it)
            if n and int(a.max()) > self.true_peak[c]:      # strictly greater replaces; argmax is the first
                self.true_peak[c] = int(a.max())
                self.index[c] = 4 * self.samples + int(np.argmax(a))
            self.sample_peak[c] = max(self.sample_peak[c], int(np.abs(x[11:]).max()) if n else 0)
            self.full_scale[c] = min(self.full_scale[c] + int(np.sum((x[11:] == -32768) | (x[11:] == 32767))), U32)
            self.hist[c] = x[-11:]
            self.measured |= 1 << c
        self.samples += n
        return self

    def record(self):
        """the state as the engine's record (STATE_DTYPE)"""
        r = np.zeros((), STATE_DTYPE)
        r["samples"], r["index"], r["true_peak"], r["sample_peak"] = self.samples, self.index, self.true_peak, self.sample_peak
        r["full_scale"], r["hist"], r["measured"] = self.full_scale, self.hist, self.measured
        return r

    def read(self, ceiling_q28=0):
        """the read-out -> a dict with the result record's fields"""
        return read_record(self.record(), ceiling_q28)


def read_record(r, ceiling_q28=0):
    """the read-out rule on a state record: the larger value, then the smaller index, then the lower slot"""
    tp, idx, sp = [int(v) for v in r["true_peak"]], [int(v) for v in r["index"]], [int(v) for v in r["sample_peak"]]
    slot = min(range(6), key=lambda c: (-tp[c], idx[c], c))
    sslot = min(range(6), key=lambda c: (-sp[c], c))
    flags = (EMPTY if int(r["samples"]) == 0 or int(r["measured"]) == 0 else 0) | (OVER if ceiling_q28 and tp[slot] > ceiling_q28 else 0)
    return dict(true_peak=tp[slot], true_peak_index=idx[slot], true_peak_slot=slot, sample_peak=sp[sslot], sample_peak_slot=sslot,
                full_scale=min(sum(int(v) for v in r["full_scale"]), U32), samples=int(r["samples"]), slot_true_peak=tp,
                slot_sample_peak=sp, dbtp=db(tp[slot], UNIT), dbfs=db(sp[sslot], 32768), flags=flags)


def run_batch(pcm, roles, meters=None):
    """pcm int16 [S][n][channels] -> the meters (new ones, or `meters` continued)"""
    pcm = np.asarray(pcm)
    if meters is None:
        meters = [Meter(roles) for _ in range(pcm.shape[0])]
    for s, m in enumerate(meters):
        m.push(pcm[s])
    return meters


def records(meters):
    return np.array([m.record() for m in meters], STATE_DTYPE)


def noise(seed, nframes, channels, amps, loud_slot=None):
    """Test content: seeded uniform noise int16 [nframes * 1536][channels], slot c at amps[c] of full scale; loud_slot: a
    slot at full scale throughout (an LFE that must not be measured)"""
    rng = np.random.default_rng(seed)
    n = nframes * 1536
    x = rng.integers(-32767, 32768, (n, channels)).astype(np.float64) * np.asarray(amps, np.float64)[None, :channels]
    if loud_slot is not None:
        x[:, loud_slot] = rng.integers(-32768, 32768, n)
    return np.round(x).astype(np.int16)


def worst_case():
    """12 samples in time order that drive phase 1 to its largest magnitude at the last of them: -32768 where H[1][k] > 0,
    32767 elsewhere (x[n - k] meets H[1][k])"""
    return np.array([-32768 if H[1][k] > 0 else 32767 for k in range(12)][::-1], np.int16)
