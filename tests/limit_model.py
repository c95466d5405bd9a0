"""The true-peak limiter of include/ac3mi.h (ac3mi_limit_*) restated in numpy int64: the detector on the meter's interpolator
(tests/truepeak_model.py), the exact quotient, the hold minimum, the release as a min-plus scan, the smoothing sum and the
gain's application - in a whole-signal form, limit(), and in the engine's state form, whose record has the engine's layout.
numpy only; nothing here rounds."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import truepeak_model as M

ONE = 1 << 24
W, B, D = 80, 64, 77                    # hold window, smoothing window, delay (AC3MI_LIMIT_DELAY)
MAX_CEILING, MAX_STEP = 1 << 28, 1 << 20
EMPTY, ACTIVE = 1, 2                    # AC3MI_LIMIT_EMPTY, AC3MI_LIMIT_ACTIVE
PEAK_SLACK = 8286                       # half an output step times the interpolator's largest absolute phase sum, 16571 / 2

# the engine's state record (limit_rule.h, LimitState) and result record (ac3mi_limit_result)
STATE_DTYPE = np.dtype([("samples", "<u8"), ("reduced", "<u8"), ("max_detect", "<u4"), ("max_reduction", "<u4"), ("q_red", "<u4", (80,)),
                        ("r_red", "<u4", (64,)), ("hist", "<i2", (6, 80))])
assert STATE_DTYPE.itemsize == 1560


def limit(pcm, roles, C, R):
    """the rule over a whole signal: pcm int16 [n][ch] -> z int16 [n][ch], g, d"""
    n, ch = pcm.shape
    x = pcm.astype(np.int64)
    d = np.zeros(n, np.int64)
    for c in range(ch):
        if not roles[c]:
            continue
        a = np.abs(M.oversample(x[:, c])).reshape(-1, 4).max(axis=1)
        ax = np.abs(x[:, c]) << 13
        for s in (5, 6):
            sh = np.zeros(n, np.int64)
            sh[s:] = ax[:n - s]
            a = np.maximum(a, sh)
        d = np.maximum(d, a)
    q = np.where(d <= C, ONE, (C << 24) // np.maximum(d, 1))
    m = sliding_window_view(np.concatenate([np.full(79, ONE), q]), 80).min(axis=1)
    k = np.arange(n, dtype=np.int64)
    r = np.minimum(np.minimum(np.minimum.accumulate(m - k * R) + k * R, ONE), m)
    g = sliding_window_view(np.concatenate([np.full(63, ONE), r]), 64).sum(axis=1) >> 6
    xd = np.zeros_like(x)
    xd[77:] = x[:n - 77]
    return ((xd * g[:, None] + (1 << 23)) >> 24).astype(np.int16), g, d


def release_loop(m, R, r_prev=ONE):
    """r[n] = min(m[n], r[n - 1] + R) as the literal loop (what the scan form must equal)"""
    r = np.empty(len(m), np.int64)
    for i, v in enumerate(m):
        r_prev = r[i] = min(int(v), r_prev + R)
    return r


def release_step(sample_rate, ms):
    """ceil(2^24 / (rate ms / 1000)) clamped to [1, 2^20]; not a number: 1"""
    with np.errstate(all="ignore"):
        v = np.ceil(np.float64(ONE) / (np.float64(sample_rate) * np.float64(ms) / 1000.0))
    return 1 if not v >= 1 else int(min(v, MAX_STEP))


class Limiter:
    """One stream's limiter in the engine's state form."""

    def __init__(self, roles, C, R):
        assert 1 <= C <= MAX_CEILING and 1 <= R <= MAX_STEP
        self.roles, self.C, self.R = list(roles), int(C), int(R)
        self.samples = self.reduced = self.max_detect = 0
        self.min_gain = ONE
        self.q = np.full(80, ONE, np.int64)             # q of the last 80 instants, oldest first
        self.r = np.full(64, ONE, np.int64)             # r of the last 64
        self.hist = np.zeros((6, 80), np.int64)         # the last 80 input samples of every slot

    def push(self, pcm):
        """pcm int16 [n][channels]: the next n sample instants -> z int16 [n][channels]"""
        pcm = np.asarray(pcm)
        n, ch = pcm.shape
        assert ch == len(self.roles)
        if n == 0:
            return np.zeros((0, ch), np.int16)
        x = np.concatenate([self.hist[:ch].T, pcm.astype(np.int64)])        # [80 + n][ch]; new instant i is row 80 + i
        d = np.zeros(n, np.int64)
        for c in range(ch):
            if not self.roles[c]:
                continue
            a = np.abs(M.oversample(x[:, c])).reshape(-1, 4).max(axis=1)[80:]   # rows 80 on have their 11 samples of history
            ax = np.abs(x[:, c]) << 13
            d = np.maximum(d, np.maximum(a, np.maximum(ax[75:75 + n], ax[74:74 + n])))
        q = np.where(d <= self.C, ONE, (self.C << 24) // np.maximum(d, 1))
        qq = np.concatenate([self.q, q])
        m = sliding_window_view(qq[1:], 80).min(axis=1)
        k = np.arange(n, dtype=np.int64)
        r = np.minimum(np.minimum(np.minimum.accumulate(m - k * self.R) + k * self.R, self.r[-1] + (k + 1) * self.R), m)
        rr = np.concatenate([self.r, r])
        g = sliding_window_view(rr[1:], 64).sum(axis=1) >> 6
        z = ((x[80 - 77:80 - 77 + n] * g[:, None] + (1 << 23)) >> 24).astype(np.int16)
        self.q, self.r, self.hist[:ch] = qq[-80:], rr[-64:], x[-80:].T
        self.samples += n
        self.reduced += int(np.sum(g < ONE))
        self.max_detect = max(self.max_detect, int(d.max()))
        self.min_gain = min(self.min_gain, int(g.min()))
        return z

    def record(self):
        """the state as the engine's record (STATE_DTYPE)"""
        s = np.zeros((), STATE_DTYPE)
        s["samples"], s["reduced"], s["max_detect"], s["max_reduction"] = self.samples, self.reduced, self.max_detect, ONE - self.min_gain
        s["q_red"], s["r_red"], s["hist"] = ONE - self.q, ONE - self.r, self.hist
        return s

    def read(self):
        return read_record(self.record())


def read_record(s):
    """the read-out rule on a state record -> a dict with the result record's fields"""
    gain = ONE - int(s["max_reduction"])
    return dict(samples=int(s["samples"]), reduced=int(s["reduced"]), max_detect=int(s["max_detect"]), min_gain_q24=gain,
                in_dbtp=M.db(int(s["max_detect"]), M.UNIT), reduction_db=0.0 if gain == ONE else M.db(gain, ONE),
                flags=(EMPTY if int(s["samples"]) == 0 else 0) | (ACTIVE if int(s["reduced"]) > 0 else 0))


def run_batch(pcm, roles, C, R, limiters=None):
    """pcm int16 [S][n][channels] -> (z int16 of the same shape, the limiters: new ones, or `limiters` continued)"""
    pcm = np.asarray(pcm)
    if limiters is None:
        limiters = [Limiter(roles, C, R) for _ in range(pcm.shape[0])]
    return np.stack([lim.push(pcm[s]) for s, lim in enumerate(limiters)]), limiters


def records(limiters):
    return np.array([lim.record() for lim in limiters], STATE_DTYPE)


def true_peak(z, roles):
    """the meter's true peak of z int16 [n][ch] over the detected slots"""
    return max([M.whole(z[:, c])["true_peak"] for c in range(z.shape[1]) if roles[c]] or [0])


def sample_peak(z, roles):
    return max([int(np.abs(z[:, c].astype(np.int64)).max()) for c in range(z.shape[1]) if roles[c]] or [0])


def contents():
    """the named test contents: (name, roles, pcm int16 [n][ch])"""
    out = [("noise %d" % s, [1, 1, 0], M.noise(s, 3, 3, (1.0, 0.8, 0.3))) for s in range(6)]
    out.append(("noise 7", [1, 1], M.noise(7, 4, 2, (1.0, 0.6))))
    worst = np.zeros((3 * 1536, 2), np.int16)
    worst[1531:1543, 0] = M.worst_case()
    worst[2000:2012, 1] = M.worst_case()
    out.append(("worst case", [1, 1], worst))
    n = np.arange(3 * 1536)
    out.append(("fs/4 at 45 degrees", [1], np.round(32767.0 * np.sin(2.0 * np.pi * n / 4.0 + np.pi / 4.0)).astype(np.int16)[:, None]))
    n = np.arange(4 * 1536)
    gate = np.where((n % 600) < 300, 1.0, 0.05)
    out.append(("gated 997 Hz", [1], np.round(32767.0 * gate * np.sin(2.0 * np.pi * 997.0 * n / 48000.0)).astype(np.int16)[:, None]))
    n = np.arange(3 * 1536)
    out.append(("square 194", [1], np.where((n % 194) < 97, 32767, -32768).astype(np.int16)[:, None]))
    out.append(("all -32768", [1, 1, 1], np.full((3 * 1536, 3), -32768, np.int16)))
    return out
