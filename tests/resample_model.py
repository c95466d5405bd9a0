"""The sample-rate converter of include/ac3mi.h (ac3mi_resample_*) restated in numpy: the Q23 table in float64 by the header's
expression, in its order; the signal and the state in int64; a Converter whose record has the engine's layout (resample_rule.h,
ResampleState).  numpy and math only; nothing but the table's design uses a float."""
import math

import numpy as np

RATES = (32000, 44100, 48000)
# (in_rate, out_rate) in the order of the header's table; a state's tag is 1 + 6 * index + (channels - 1)
PAIRS = ((44100, 48000), (48000, 44100), (32000, 48000), (48000, 32000), (32000, 44100), (44100, 32000))
ONE = 1 << 23
BETA = 9.2
HIST = 96                               # input samples kept per slot (the longest filter reads 95 of them)
STATUS_FRAMES, STATUS_STATE = 1, 2      # AC3MI_RESAMPLE_FRAMES, AC3MI_RESAMPLE_STATE

STATE_DTYPE = np.dtype([("samples_in", "<u8"), ("frames_out", "<u8"), ("tag", "u1"), ("zero", "u1", (7,)), ("hist", "<i2", (6, HIST)),
                        ("pend", "<i2", (1536 * 6,))])
assert STATE_DTYPE.itemsize == 19608


def ratio(in_rate, out_rate):
    """(L, M, T) of a pair"""
    assert in_rate in RATES and out_rate in RATES and in_rate != out_rate
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    T = 64 if L > M else 8 * -(-(64 * M) // (8 * L))
    return L, M, T


def _i0(x):
    """the header's series, element by element: stop when term < 1e-21 * s"""
    s = np.ones_like(x)
    term = np.ones_like(x)
    live = np.ones(x.shape, bool)
    j = 1
    while live.any():
        v = x / 2 / j
        term = term * (v * v)
        s = np.where(live, s + term, s)
        live &= ~(term < 1e-21 * s)
        j += 1
    return s


_TABLES = {}


def table(in_rate, out_rate):
    """C[L][T] int64, Q23, every phase summing to 2^23"""
    key = (in_rate, out_rate)
    if key in _TABLES:
        return _TABLES[key]
    L, M, T = ratio(in_rate, out_rate)
    r = min(1.0, float(L) / M)
    p = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(T, dtype=np.float64)[None, :]
    t = (k + p / L) - float(T // 2)
    a = r * t
    pa = math.pi * a
    sin = np.array([[math.sin(v) for v in row] for row in pa])          # libm's sin, as the engine's builder calls it
    with np.errstate(all="ignore"):
        sinc = np.where(a == 0, 1.0, sin / pa)
    q = (2 * t) / T
    u = 1 - q * q
    w = _i0(BETA * np.sqrt(np.maximum(u, 0.0))) / _i0(np.array(BETA))
    h = (r * sinc) * w
    C = np.floor(8388608 * h + 0.5).astype(np.int64)
    for row in C:
        row[int(np.argmax(row))] += ONE - int(row.sum())
    C.setflags(write=False)
    _TABLES[key] = C
    return C


def split(C):
    """hi, lo with C = 512 hi + lo, lo in [-256, 255]"""
    hi = (C + 256) >> 9
    return hi, C - 512 * hi


def out_count(in_rate, out_rate, n):
    """output instants that exist after n input instants: ceil(n L / M)"""
    L, M, _ = ratio(in_rate, out_rate)
    return -(-(n * L) // M)


def plan(in_rate, out_rate, samples_in, frames_out, in_frames):
    """(out_frames, pending_after) of a call that pushes in_frames frames"""
    total = out_count(in_rate, out_rate, samples_in + 1536 * in_frames) - 1536 * frames_out
    return total // 1536, total % 1536


def convert(x, in_rate, out_rate, first_in=0, m0=None, m1=None):
    """y[m0:m1] int64 [m][ch] of the stream whose inputs from instant first_in on are x int64 [n][ch] (zeros before it, and the
    caller asks for no output that reads past x)"""
    L, M, T = ratio(in_rate, out_rate)
    C = table(in_rate, out_rate)
    m = np.arange(m0, m1, dtype=np.int64)
    i = (m * M) // L - first_in
    p = (m * M) % L
    xp = np.concatenate([np.zeros((T, x.shape[1]), np.int64), x.astype(np.int64)])
    assert len(m) == 0 or (i.max() < len(x) and i.min() >= -1)
    idx = (i + T)[:, None] - np.arange(T)[None, :]                      # [m][k] -> x[i - k]
    acc = np.einsum("mk,mkc->mc", C[p], xp[idx])
    return np.clip((acc + (1 << 22)) >> 23, -32768, 32767)


class Converter:
    """one stream in the engine's state form"""

    def __init__(self, in_rate, out_rate, channels):
        self.pair = (in_rate, out_rate)
        self.ch = channels
        self.tag = 1 + 6 * PAIRS.index(self.pair) + channels - 1
        self.samples_in = 0
        self.frames_out = 0
        self.hist = np.zeros((HIST, channels), np.int64)               # the last 96 inputs, oldest first
        self.pend = np.zeros((0, channels), np.int64)

    def plan(self, in_frames):
        return plan(*self.pair, self.samples_in, self.frames_out, in_frames)

    def push(self, pcm, out_frames=None):
        """pcm int16 [1536 f][ch] -> int16 [1536 out_frames][ch] (default: the planned count); a wrong out_frames raises"""
        assert pcm.shape[0] % 1536 == 0 and pcm.shape[0] > 0 and pcm.shape[1] == self.ch
        f = pcm.shape[0] // 1536
        want, left = self.plan(f)
        if out_frames is None:
            out_frames = want
        if out_frames != want:
            raise ValueError("out_frames %d, planned %d" % (out_frames, want))
        x = np.concatenate([self.hist, pcm.astype(np.int64)])
        m0 = 1536 * self.frames_out + len(self.pend)
        m1 = out_count(*self.pair, self.samples_in + 1536 * f)
        y = np.concatenate([self.pend, convert(x, *self.pair, first_in=self.samples_in - HIST, m0=m0, m1=m1)])
        assert len(y) == 1536 * out_frames + left
        self.hist = x[-HIST:]
        self.pend = y[1536 * out_frames:]
        self.samples_in += 1536 * f
        self.frames_out += out_frames
        return y[:1536 * out_frames].astype(np.int16)

    def record(self):
        r = np.zeros((), STATE_DTYPE)
        r["samples_in"], r["frames_out"], r["tag"] = self.samples_in, self.frames_out, self.tag if self.samples_in else 0
        r["hist"][:self.ch] = self.hist.T
        r["pend"][:self.pend.size] = self.pend.reshape(-1)
        return r


def tone(freq, rate, n, ch, amp=32767.0, phase=0.0):
    """amp sin(2 pi freq t / rate + phase + slot) rounded to int16 [n][ch]"""
    t = np.arange(n, dtype=np.float64)[:, None]
    return np.round(amp * np.sin(2 * np.pi * freq * t / rate + phase + np.arange(ch)[None, :])).astype(np.int16)


def contents(in_rate, frames, ch, seed=0):
    """the named contents, int16 [frames * 1536][ch] each: silence, tones, noise, +- full-scale random (clamps at both rails),
    an impulse pair at a frame seam"""
    n = frames * 1536
    rng = np.random.default_rng(1000 + seed)
    out = [("silence", np.zeros((n, ch), np.int16)),
           ("tones", tone(997.0, in_rate, n, ch)),
           ("noise", np.clip(np.round(rng.standard_normal((n, ch)) * 6000), -32768, 32767).astype(np.int16)),
           ("full-scale random", np.where(rng.random((n, ch)) < 0.5, -32768, 32767).astype(np.int16))]
    seam = np.zeros((n, ch), np.int16)
    at = 1536 * (1 if frames > 1 else 0)
    seam[at - 1 if at else 700, :] = 32767
    seam[at if at else 701, ::2] = -32768
    out.append(("impulse at a frame seam", seam))
    return out


def run_batch(in_rate, out_rate, pcm):
    """pcm int16 [S][n][ch], every stream new, one push each -> (out int16 [S][m][ch], the converters)"""
    convs = [Converter(in_rate, out_rate, pcm.shape[2]) for _ in range(pcm.shape[0])]
    return np.stack([c.push(x) for c, x in zip(convs, pcm)]), convs
