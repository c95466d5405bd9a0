"""CPU: what the encoder oracle's frames must satisfy whatever the reference's encoder writes (byte-for-byte parity
with src/ac3enc is the business of tests/test_oracle_vs_ac3enc.py, against fixtures recorded from ac3enc itself):

 * both CRCs of every frame verify (ac3enc.cpp:1599-1638; crc1 covers the first 5/8, crc2 the rest)
 * the frame is exactly filled: sync word, header fields, zero padding only at the tail
 * the REAL liba52 decodes every frame without error (build container) and returns the input signal
   (so syntax, exponent coding, bit allocation and mantissa packing agree with the reference decoder)
 * stage invariants: exponent deltas within +-2, bap from the encoder's spec-literal allocation equals
   what the decoder derives from the same exponents
"""
import ctypes

import numpy as np
import pytest

from tests import _harness as H


def crc16(data, crc=0):
    for byte in data:
        crc ^= int(byte) << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x8005) & 0xffff if crc & 0x8000 else (crc << 1) & 0xffff
    return crc


@pytest.mark.parametrize("kind", ["tones", "noise", "quiet", "music"])
def test_frames_are_wellformed(kind):
    frames = H.orc_encode(H.gen_pcm(8, 6, seed=1, kind=kind))
    for fr in frames:
        assert fr[0] == 0x0b and fr[1] == 0x77
        assert fr[4] == (0 << 6) | 28                      # fscod 0, frmsizecod 28 (384 kbps)
        assert fr[5] >> 3 == 8                             # bsid
        assert fr[6] >> 5 == 7                             # acmod 3/2
        words = 768
        w58 = (words >> 1) + (words >> 3)
        assert crc16(fr[2:2 * w58]) == 0, "crc1"
        assert crc16(fr[2:]) == 0, "crc2 (whole frame after the sync word)"


def test_decoder_oracle_rederives_encoder_allocation():
    """The encoder writes mantissas with bap from the spec-literal allocator (ac3enc.cpp:220-421); the
    decoder must derive the same widths from the transmitted exponents (bit_allocate.c) or the frame
    would not parse.  Check bap code -> width equality on every coefficient."""
    L = H.orc()
    pcm = H.gen_pcm(4, 6, seed=9, kind="tones")
    fb = H.ci()
    h = L.orc_ac3enc_init(48000, 384000, 6, ctypes.byref(fb))
    cm = (ctypes.c_uint8 * 8)(*H.CHMAP6)
    st = L.orc_a52_init()
    width_of_code = {0: 0, 1: -1, 2: -2, 3: 3, 4: -3, 5: 4, 14: 14, 15: 16}
    width_of_code.update({c: c - 1 for c in range(6, 14)})
    out = np.zeros(1600, np.uint8)
    for f in range(4):
        assert L.orc_ac3enc_frame(h, H.P(out, H.u8p), ctypes.cast(pcm.ctypes.data + f * 1536 * 12, H.i16p), cm) == 1536
        bap = np.zeros((6, 6, 256), np.uint8)
        eexp = np.zeros((6, 6, 256), np.uint8)
        raw = np.zeros((6, 6, 256), np.uint8)
        L.orc_ac3enc_get_bap(h, H.P(bap, H.u8p))
        L.orc_ac3enc_get_exp(h, H.P(raw, H.u8p), H.P(eexp, H.u8p))
        fl, lv = H.ci(23), H.cf(1.0)
        assert L.orc_a52_frame(st, H.P(out, H.u8p), ctypes.byref(fl), ctypes.byref(lv), 0.0) == 0
        for b in range(6):
            assert L.orc_a52_block(st) == 0
            for ch in range(6):
                n = 223 if ch < 5 else 7
                e, w = np.zeros(256, np.uint8), np.zeros(256, np.int8)
                L.orc_a52_get_exp(st, ch, H.P(e, H.u8p))
                L.orc_a52_get_bap(st, ch, H.P(w, H.i8p))
                assert np.array_equal(e[:n], eexp[b, ch, :n])
                assert [width_of_code[int(c)] for c in bap[b, ch, :n]] == w[:n].tolist()
                assert np.abs(np.diff(eexp[b, ch, :n].astype(int))).max() <= 2
    L.orc_ac3enc_free(h)
    L.orc_a52_free(st)


@pytest.mark.parametrize("nch,bitrate", [(6, 384000), (6, 640000), (2, 192000), (1, 64000), (5, 448000)])
def test_real_liba52_decodes_oracle_frames(nch, bitrate):
    pcm = H.gen_pcm(12, nch, seed=4, kind="music")
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    frames = H.orc_encode(pcm, nch=nch, bitrate=bitrate, chmap=chmap)
    acmod = {1: 1, 2: 2, 5: 7, 6: 7}[nch]
    # liba52's decode; without oracle/_ref the oracle's, which must then be liba52's stored result bit for bit
    want = H.ref_decode_record(frames, acmod | 16, 1.0, 0.0)
    dec, errs, flags = (H.ref_decode if H.have_ref() else H.orc_decode)(frames, acmod | 16, 1.0, 0.0)
    assert H.decode_record(dec, errs, flags) == want
    assert errs == 0
    assert flags == (acmod | (16 if nch == 6 else 0))
    # decoded plane p (liba52 order) vs input channel (interleaved WAVE order through chmap)
    x = pcm.astype(np.float64) / 32768.0
    planes = dec.transpose(2, 0, 1, 3).reshape(dec.shape[2], -1)      # [plane][time]
    if nch == 6:
        wave_of_plane = [3, 0, 2, 1, 4, 5]
    elif nch == 5:
        wave_of_plane = [0, 2, 1, 3, 4]          # coded L,C,R,SL,SR <- chmap identity: input order L,C,R,SL,SR
        wave_of_plane = [0, 1, 2, 3, 4]
    else:
        wave_of_plane = list(range(nch))
    for p, c in enumerate(wave_of_plane):
        if nch == 6 and p == 0:
            continue                               # LFE keeps 7 coefficients only
        d, s = planes[p][256:], x[:-256, c]        # the codec delays by one block
        snr = 10 * np.log10((s ** 2).mean() / ((d - s) ** 2).mean())
        assert snr > 25.0, (p, c, snr)
