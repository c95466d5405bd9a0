// crc_lanes.h — the lane rule of a frame's two CRC-16 words, stated once: how ONE wavefront sums both CRC regions of a frame
// it has packed in one pass, with one GF(2)[x] multiplication per lane.  The packers (encode.hip: enc_packf_kernel,
// enc_packb_kernel), the host that builds the rule's table (launch_encode) and the host program of tests/crc_lanes_c follow
// this file.
//
// A/52's CRC: polynomial x^16 + x^15 + x^2 + 1, MSB first, start value 0 (crc.hip's header has the definition).  With fs the
// frame's size in 16-bit words and fs58 = (fs >> 1) + (fs >> 3) the encoder sums (ENC/ac3enc.cpp:1599-1638)
//     region 1 = bytes [0, 2 fs58) with bytes 0..3 read as zero (the sync word is outside the sum, the crc1 field zero while
//                summed); crc1 = that sum times x^-(16 fs58 - 16), which makes bytes [2, 2 fs58) sum to 0 with crc1 in place;
//     region 2 = bytes [2 fs58, 2 fs - 2); crc2 = that sum.
// The rule:
//   split   the 64 lanes are dealt n1 + n2 = 64 to the regions, every lane takes a chunk of C bytes (C a multiple of 4),
//           chunks are aligned to their region's END: bytes in front of the region read as zero, and a zero prefix does not
//           change a sum that starts at 0.  C is the smallest for which the chunks cover both regions.
//   sum     a lane reads its chunk as dwords of the staged frame (MSB-first dwords); a start that is only halfword-aligned
//           (2 fs58 and 2 fs - 2 are even, no more) is a funnel shift of consecutive dwords.  What lies in front of the region
//           is masked per dword.  The running value rides in the top half of a dword the data is XORed into, so a byte step is:
//           top byte, table read, shift, xor.
//   weigh   lane i of a region of n lanes multiplies its chunk sum by its OWN constant K = x^(8 C (n - 1 - i)) mod poly -
//           region 1's times x^-(16 fs58 - 16) as well - through the row t[j] = K x^j: sixteen select-and-xor steps.
//   reduce  an inclusive XOR scan over the lanes: crc1 = scan[n1 - 1], crc2 = scan[63] ^ scan[n1 - 1].
// Plain C++: compiles without HIP.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

constexpr uint32_t CRCL_POLY = 0x18005u;
constexpr uint32_t CRCL_X_INV = CRCL_POLY >> 1;     // x^-1 mod poly: x * (poly >> 1) = poly - 1 = 1
constexpr int CRCL_LANES = 64;
constexpr int CRCL_ROW = 16;                        // entries of a lane's row (uint16_t: 32 bytes a lane, 2 KB a frame size)
constexpr int CRCL_READ_AHEAD = 2;                  // dwords a lane reads behind its chunk's last: the funnel's, and one requested early

// GF(2)[x] / poly
__host__ __device__ inline uint32_t crcl_mul(uint32_t a, uint32_t b)
{
    uint32_t c = 0;
    for (; a; a >>= 1) {
        if (a & 1u) c ^= b;
        b <<= 1;
        if (b & 0x10000u) b ^= CRCL_POLY;
    }
    return c;
}
__host__ __device__ inline uint32_t crcl_pow(uint32_t a, uint32_t n)
{
    uint32_t r = 1;
    for (; n; n >>= 1, a = crcl_mul(a, a))
        if (n & 1u) r = crcl_mul(r, a);
    return r;
}

// the scalar reference: the sum after one more message byte, bit by bit; and of bytes [lo, end) of a frame
__host__ __device__ inline uint32_t crcl_byte(uint32_t crc, uint32_t byte)
{
    for (int k = 7; k >= 0; k--) {
        const uint32_t top = ((crc >> 15) ^ (byte >> k)) & 1u;
        crc = (crc << 1) & 0xffffu;
        if (top) crc ^= CRCL_POLY & 0xffffu;
    }
    return crc;
}
__host__ __device__ inline uint32_t crcl_ref_sum(const uint8_t *frame, int lo, int end)
{
    uint32_t crc = 0;
    for (int p = lo; p < end; p++) crc = crcl_byte(crc, frame[p]);
    return crc;
}
// ... and the two words of a frame of fs words by the definition (bytes 0..3 of `frame` are not read)
__host__ __device__ inline int crcl_end1(int fs) { return 2 * ((fs >> 1) + (fs >> 3)); }
__host__ __device__ inline int crcl_end2(int fs) { return 2 * fs - 2; }
__host__ __device__ inline uint32_t crcl_ref_crc1(const uint8_t *frame, int fs)
{
    return crcl_mul(crcl_ref_sum(frame, 4, crcl_end1(fs)), crcl_pow(CRCL_X_INV, 8u * (uint32_t)crcl_end1(fs) - 16u));
}
__host__ __device__ inline uint32_t crcl_ref_crc2(const uint8_t *frame, int fs) { return crcl_ref_sum(frame, crcl_end1(fs), crcl_end2(fs)); }

// ---- split ----
struct CrcSplit {
    int C;      // chunk bytes per lane, a multiple of 4
    int n1;     // lanes 0 .. n1 - 1 sum region 1, the other 64 - n1 region 2
};
__host__ __device__ inline CrcSplit crcl_split(int fs)
{
    const int len1 = crcl_end1(fs), len2 = crcl_end2(fs) - crcl_end1(fs);
    CrcSplit s{4, 0};
    while ((len1 + s.C - 1) / s.C + (len2 + s.C - 1) / s.C > CRCL_LANES) s.C += 4;
    s.n1 = (len1 + s.C - 1) / s.C;
    return s;
}

// ---- a lane's place ----
struct CrcLane {
    int begin;      // its chunk is bytes [begin, begin + C) of the frame; may be negative
    int lo;         // bytes below lo read as zero (4 in region 1, 2 fs58 in region 2)
    int weight;     // its chunk sum counts times x^(8 weight): the bytes of its region behind its chunk
};
__host__ __device__ inline CrcLane crcl_lane(CrcSplit s, int fs, int lane)
{
    const bool r2 = lane >= s.n1;
    const int end = r2 ? crcl_end2(fs) : crcl_end1(fs);
    const int behind = r2 ? CRCL_LANES - 1 - lane : s.n1 - 1 - lane;     // lanes of its region behind it
    return CrcLane{end - s.C * (behind + 1), r2 ? crcl_end1(fs) : 4, s.C * behind};
}
// its constant and the row of it
__host__ __device__ inline uint32_t crcl_lane_const(CrcSplit s, int fs, int lane)
{
    const uint32_t k = crcl_pow(2, 8u * (uint32_t)crcl_lane(s, fs, lane).weight);
    return lane < s.n1 ? crcl_mul(k, crcl_pow(CRCL_X_INV, 8u * (uint32_t)crcl_end1(fs) - 16u)) : k;
}
__host__ __device__ inline void crcl_row(uint32_t k, uint16_t *t)
{
    for (int j = 0; j < CRCL_ROW; j++) { t[j] = (uint16_t)k; k = crcl_mul(k, 2); }
}
// the table of a frame size: rows[lane][j]
inline void crcl_fill_rows(int fs, uint16_t (*rows)[CRCL_ROW])
{
    const CrcSplit s = crcl_split(fs);
    for (int lane = 0; lane < CRCL_LANES; lane++) crcl_row(crcl_lane_const(s, fs, lane), rows[lane]);
}

// ---- sum ----
// dword d of the staged frame with the bytes below `lo` zeroed; a dword in front of the frame is all zeros (lo >= 4 there)
template <class Fr>
__host__ __device__ inline uint32_t crcl_dword(const Fr &fr, int d, int lo)
{
    const int t = lo - 4 * d;                   // bytes of this dword in front of the region
    const uint32_t m = t <= 0 ? 0xffffffffu : t >= 4 ? 0u : 0xffffffffu >> (8 * t);
    return fr[d < 0 ? 0 : d] & m;
}
// the sum of bytes [begin, begin + C) (begin even): fr[d] = bytes 4 d .. 4 d + 3, MSB first; tab[b] = the sum of the one byte b.
// Reads dwords max(begin >> 2, 0) .. (begin >> 2) + C / 4 + CRCL_READ_AHEAD - 1
template <class Fr, class Tab>
__host__ __device__ inline uint32_t crcl_chunk_sum(const Fr &fr, const Tab &tab, int begin, int C, int lo)
{
    const int d0 = begin >> 2;                  // floor, also of a negative start
    const bool half = (begin & 2) != 0;
    uint32_t s = 0;                             // top half: the running sum, XORed into the data that is next
    uint32_t cur = crcl_dword(fr, d0, lo), nxt = crcl_dword(fr, d0 + 1, lo);
    for (int k = 0; k < C / 4; k++) {
        const uint32_t ahead = crcl_dword(fr, d0 + k + 2, lo);
        s ^= half ? (cur << 16) | (nxt >> 16) : cur;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 4; j++) s = (s << 8) ^ ((uint32_t)tab[s >> 24] << 16);
        cur = nxt;
        nxt = ahead;
    }
    return s >> 16;
}

// ---- weigh ----
// a * K for the row t[j] = K x^j, given as eight dwords (t[2 k] in the low half of r[k])
__host__ __device__ inline uint32_t crcl_mul_row(uint32_t a, const uint32_t *r)
{
    uint32_t e = 0, o = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < CRCL_ROW / 2; k++) {
        e ^= (uint32_t)((int32_t)(a << (31 - 2 * k)) >> 31) & r[k];
        o ^= (uint32_t)((int32_t)(a << (30 - 2 * k)) >> 31) & r[k];
    }
    return (e & 0xffffu) ^ (o >> 16);
}

}  // namespace ac3mi
