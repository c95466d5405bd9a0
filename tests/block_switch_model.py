"""numpy model of the encoder's transient detector (ac3mi_set_encode_block_switch 1, include/ac3mi.h) and signals for it."""
import numpy as np


def detect(z):
    """z: int [..., 512] = the 256 samples before a block's new ones || its 256 new ones -> blksw [...] (0 / 1)."""
    z = np.asarray(z, np.int64)
    a = np.zeros(z.shape, np.int64)
    a[..., 2:] = np.abs(z[..., 2:] - 2 * z[..., 1:-1] + z[..., :-2])
    seg = a.reshape(z.shape[:-1] + (8, 64)).max(-1)          # maxima of the 64-sample segments (a[0] = a[1] = 0)
    p1 = np.stack([seg[..., 0:4].max(-1), seg[..., 4:8].max(-1)], -1)
    p2 = np.stack([seg[..., 2:4].max(-1), seg[..., 4:6].max(-1), seg[..., 6:8].max(-1)], -1)
    p3 = seg[..., 3:8]
    hit = (p1[..., 1] > 10 * p1[..., 0]) | (3 * p2[..., 1:] > 40 * p2[..., :-1]).any(-1) | (p3[..., 1:] > 20 * p3[..., :-1]).any(-1)
    return ((p1[..., 1] > 400) & hit).astype(np.uint8)


def decisions(pcm, chmap, nfbw, last=None):
    """pcm [F*1536][nch] s16 interleaved (input order), last [nch][256] (coded-channel order) or None for zeros
    -> blksw [F][6][nfbw] as the encoder codes it (channel ch reads input column chmap[ch])."""
    F = pcm.shape[0] // 1536
    out = np.zeros((F, 6, nfbw), np.uint8)
    for ch in range(nfbw):
        h = np.zeros(256, np.int64) if last is None else np.asarray(last[ch], np.int64)
        x = np.concatenate([h, pcm[:, chmap[ch]].astype(np.int64)])
        z = np.lib.stride_tricks.sliding_window_view(x, 512)[::256][:F * 6]
        out[:, :, ch] = detect(z).reshape(F, 6)
    return out


def attack_pcm(nframes, nch, onsets, amp=16000.0, seed=7):
    """Quiet noise (+-3), then from each onset a 3 kHz tone burst of 400 samples on every channel."""
    n = nframes * 1536
    rng = np.random.default_rng(seed)
    out = rng.integers(-3, 4, (n, nch)).astype(np.float64)
    t = np.arange(n)
    for o in onsets:
        m = (t >= o) & (t < o + 400)
        for c in range(nch):
            out[m, c] += amp * np.sin(2 * np.pi * 3000.0 / 48000.0 * (t[m] - o) + c)
    return np.clip(np.round(out), -32768, 32767).astype(np.int16)
