"""The truth for the CRC tests: A/52's CRC-16 straight from its definition - polynomial x^16 + x^15 + x^2 + 1, MSB first,
start value 0, one message bit per step, no tables - and the two regions of a frame it protects.

With fs the frame's size in 16-bit words from its own header and fs58 = (fs >> 1) + (fs >> 3):
    region 1 = bytes [2, 2 fs58)   (holds crc1 in bytes 2-3)     must sum to 0
    region 2 = bytes [2 fs58, 2 fs) (ends with crc2), from 0 again, must sum to 0
Nothing here comes from the engine's code; numpy only carries many frames through the same bit steps at once."""
import numpy as np

POLY = 0x8005            # x^16 (implicit) + x^15 + x^2 + 1
KBPS = (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 448, 512, 576, 640)
CRC1, CRC2, NOT_SUMMED = 1, 2, 0x80


def crc16(data, crc=0):
    """CRC-16 of a byte sequence, bit by bit."""
    for byte in bytes(bytearray(data)):
        for k in range(7, -1, -1):
            top = ((crc >> 15) & 1) ^ ((byte >> k) & 1)
            crc = (crc << 1) & 0xffff
            if top:
                crc ^= POLY
    return crc


def crc16_rows(rows, crc=None):
    """The same for every row of a [n][len] uint8 array at once -> [n] (uint32)."""
    rows = np.asarray(rows, np.uint8)
    crc = np.zeros(rows.shape[0], np.uint32) if crc is None else crc.astype(np.uint32).copy()
    for i in range(rows.shape[1]):
        col = rows[:, i].astype(np.uint32)
        for k in range(7, -1, -1):
            top = ((crc >> 15) & 1) ^ ((col >> k) & 1)
            crc = ((crc << 1) & 0xffff) ^ (top * POLY)
    return crc


def frame_size(hdr):
    """Frame size in bytes from bytes 0-5 (a52_syncinfo's test: sync word, bsid < 12, frmsizecod < 38, fscod != 3); 0 = no frame.
    bsid 9 / 10 (half / quarter rate) keep the table."""
    hdr = [int(b) for b in hdr[:6]]
    if hdr[0] != 0x0b or hdr[1] != 0x77 or hdr[5] >= 0x60:
        return 0
    code, fscod = hdr[4] & 63, hdr[4] >> 6
    if code >= 38 or fscod == 3:
        return 0
    rate = KBPS[code >> 1]
    if fscod == 0:
        return 4 * rate
    if fscod == 1:
        return 2 * (320 * rate // 147 + (code & 1))
    return 6 * rate


def regions(nbytes):
    """(end of region 1 = start of region 2, end of region 2) in bytes for a frame of nbytes."""
    fs = nbytes // 2
    return 2 * ((fs >> 1) + (fs >> 3)), 2 * fs


def verdict(frame, frame_bytes=None):
    """bit 0: region 1 does not sum to 0, bit 1: region 2 does not, bit 7: not summed (no frame by its first six bytes, or
    longer than frame_bytes - default: the bytes given)."""
    frame = np.asarray(frame, np.uint8)
    limit = frame.shape[0] if frame_bytes is None else frame_bytes
    n = frame_size(frame[:6])
    if n == 0 or n > limit:
        return NOT_SUMMED
    e1, e2 = regions(n)
    return (CRC1 if crc16(frame[2:e1]) else 0) | (CRC2 if crc16(frame[e1:e2]) else 0)


def verdicts(frames, frame_bytes=None):
    """verdict() of every row of [n][stride] -> [n] uint8 (frames that share a size go through the bit steps together)."""
    frames = np.asarray(frames, np.uint8)
    limit = frames.shape[1] if frame_bytes is None else frame_bytes
    sizes = np.array([frame_size(f[:6]) for f in frames[:, :6]], np.int64)
    out = np.full(frames.shape[0], NOT_SUMMED, np.uint8)
    for n in np.unique(sizes):
        if n == 0 or n > limit:
            continue
        idx = np.nonzero(sizes == n)[0]
        e1, e2 = regions(int(n))
        c1 = crc16_rows(frames[idx, 2:e1])
        c2 = crc16_rows(frames[idx, e1:e2])
        out[idx] = (c1 != 0) * CRC1 + (c2 != 0) * CRC2
    return out


def seal(frame):
    """A copy of `frame` with crc1 (bytes 2-3) and crc2 (the last two bytes) rewritten so that both regions sum to 0.
    The CRC is linear over GF(2): the sum of region 1 is the sum with a zero crc1 field plus the responses of the field's 16
    bits; crc2 is the running sum of region 2 without its last two bytes."""
    f = np.array(frame, np.uint8, copy=True)
    n = frame_size(f[:6])
    assert n and n <= f.shape[0], "not a frame"
    e1, e2 = regions(n)
    f[2] = f[3] = 0
    target = crc16(f[2:e1])
    zero = np.zeros(e1 - 2, np.uint8)
    resp = []
    for bit in range(16):                       # bit 15 = MSB of byte 2
        z = zero.copy()
        z[(15 - bit) // 8] = 1 << (bit % 8)
        resp.append(crc16(z))
    # Gauss-Jordan over GF(2): x with XOR_i x_i resp[i] == target
    rows = [(resp[i], 1 << i) for i in range(16)]
    x = 0
    for col in range(15, -1, -1):
        piv = next((r for r in rows if (r[0] >> col) & 1), None)
        assert piv is not None, "crc1 field does not span the CRC space"
        rows.remove(piv)
        rows = [(r[0] ^ piv[0], r[1] ^ piv[1]) if (r[0] >> col) & 1 else r for r in rows]
        if (target >> col) & 1:
            target ^= piv[0]
            x ^= piv[1]
    assert target == 0
    f[2], f[3] = x >> 8, x & 0xff
    c = crc16(f[e1:e2 - 2])
    f[e2 - 2], f[e2 - 1] = c >> 8, c & 0xff
    return f
