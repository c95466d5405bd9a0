// crc.hip — the two CRC-16 words of AC-3 frames, checked on gfx950 (ac3mi_crc_check_batch, ac3mi_set_decode_crc).
// liba52 never looks at them; A/52 defines them: polynomial x^16 + x^15 + x^2 + 1, MSB first, start value 0,
// crc1 makes bytes [2, 2 fs58) of the frame sum to 0, crc2 the rest, [2 fs58, 2 fs), summed from 0 again (fs = the frame's
// size in 16-bit words from its own header, fs58 = (fs >> 1) + (fs >> 3)).
//
// One wavefront per frame, four frames per workgroup, every frame of the call in one launch before the decoder's front
// end.  The header test and the frame's size (sync_rule.h's) run on wave-uniform values (the frame's first two dwords, a scalar read of their
// own); then the frame is read once into LDS (16-byte loads where base and stride allow, else dwords).  Each lane then sums
// a chunk of C bytes of a region through the 256-entry table (LDS), and six steps combine the 64 chunk sums: crc = left * x^(8 C 2^k) + crc in GF(2)[x] / poly, the scheme
// the encoder's packers had before the lane rule of crc_lanes.h.  Chunks are aligned to the region's END and the front is padded with zero bytes -
// a zero prefix does not change a sum that starts at 0 - so one C and one set of power tables per region and call, sized
// by the batch's largest frame, serve every frame size in the batch (44.1 kHz streams alternate between two).
// The verdict is one byte per frame, stored by lane 0 (a vector store): bit 0 crc1's region fails, bit 1 crc2's, bit 6
// the decoder is to treat the frame as refused (ac3mi_set_decode_crc 2), bit 7 not summed (no frame, or not this batch's).
#include "ac3mi_internal.h"
#include "sync_rule.h"
#include "wave_ops.h"

namespace ac3mi {

struct CrcParams {
    const uint8_t *frames;
    uint8_t *verdict;
    unsigned n_frames;
    int frame_stride, frame_bytes;
    int wide;               // base and stride are multiples of 16: 16-byte loads
    int acmod, lfeon;       // the decode call's coded configuration (other frames are not summed: the front end refuses them); -1: any
    int conceal;
    int c1, c2;             // chunk bytes per lane of the two regions
    uint16_t pw1[6][16], pw2[6][16];    // pw[k][i] = x^(8 c 2^k + i) mod poly
};

__device__ __forceinline__ uint32_t crc_rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// a * t[0] in GF(2)[x] / poly for a table t[i] = t[0] * x^i mod poly (wave-uniform, from the kernel arguments)
__device__ __forceinline__ uint32_t crc_mul_tab(uint32_t a, const uint16_t *t)
{
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) c ^= (uint32_t)__builtin_amdgcn_sbfe((int)a, i, 1) & (uint32_t)t[i];
    return c;
}

constexpr int CRC_WAVES = 4;

__global__ __launch_bounds__(64 * CRC_WAVES) void crc_kernel(const CrcParams P)
{
    __shared__ uint16_t tab[256];
    extern __shared__ uint4 crc_frames[];           // [CRC_WAVES][(frame_bytes + 15) / 16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = (int)crc_rfl((uint32_t)(tid >> 6));
    {
        uint32_t c = (uint32_t)tid << 8;
#pragma unroll
        for (int j = 0; j < 8; j++) c = (c & 0x8000u) ? (((c << 1) & 0xffffu) ^ 0x8005u) : (c << 1);
        tab[tid] = (uint16_t)c;
    }
    __syncthreads();
    const unsigned fidx = blockIdx.x * CRC_WAVES + (unsigned)wave;
    if (fidx >= P.n_frames) return;
    const uint8_t *src = P.frames + (size_t)fidx * P.frame_stride;

    // ---- the header rule (sync_rule.h) and the frame's size, on bytes 0-5; the decode call's acmod / lfeon on 6-7 ----
    // A frame the front ends refuse (decode_common.h: frame_own_bytes, then their acmod / lfeon tests) is not summed: both
    // sides call the one rule.  One refusal is out of reach here, a52_downmix_init_hd() < 0: it depends on the call's request only,
    // which ac3mi_decode_planes screens before any launch; the front ends also mask bits 10 / 11 of a frame they refused themselves.
    const uint32_t h0 = crc_rfl(reinterpret_cast<const uint32_t *>(src)[0]), h1 = crc_rfl(reinterpret_cast<const uint32_t *>(src)[1]);
    const int fbytes = sync_header_ok_le(h0, h1) ? (int)sync_frame_bytes(h1 & 0xffu) : 0;
    bool ok = fbytes != 0 && fbytes <= P.frame_bytes;
    if (ok && P.acmod >= 0) {
        const uint32_t w = ((h1 >> 8) & 0xff00u) | (h1 >> 24);          // bytes 6 and 7, MSB first
        const int acmod = (int)(w >> 13);
        const int lfeon = (int)((w >> (15 - sync_lfeon_pos(acmod))) & 1u);
        if (acmod != P.acmod || lfeon != P.lfeon) ok = false;
    }
    if (!ok) {
        if (lane == 0) P.verdict[fidx] = 0x80;
        return;
    }

    // ---- the frame into LDS, as it lies in memory ----
    uint8_t *fr = reinterpret_cast<uint8_t *>(crc_frames + (size_t)wave * ((P.frame_bytes + 15) >> 4));
    if (P.wide) {
        const int n16 = (fbytes + 15) >> 4;                             // <= stride / 16: the loads stay inside the frame's slot
        const uint4 *s16 = reinterpret_cast<const uint4 *>(src);
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {                                   // 4 x 64 x 16 bytes >= the largest frame (3840)
            const int i = lane + 64 * k;
            v[k] = i < n16 ? s16[i] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = lane + 64 * k;
            if (i < n16) reinterpret_cast<uint4 *>(fr)[i] = v[k];
        }
    } else {
        const int nw = (fbytes + 3) >> 2;                               // <= stride / 4
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
        for (int base = 0; base < nw; base += 512) {
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = base + lane + 64 * k;
                v[k] = i < nw ? s32[i] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = base + lane + 64 * k;
                if (i < nw) reinterpret_cast<uint32_t *>(fr)[i] = v[k];
            }
        }
    }
    wave_sync();

    // ---- per-lane chunk sums; bytes in front of a region count as 0 ----
    const int fs = fbytes >> 1, end1 = 2 * ((fs >> 1) + (fs >> 3)), end2 = 2 * fs;
    uint32_t s1 = 0, s2 = 0;
    {
        int p = end1 - 64 * P.c1 + lane * P.c1;
        for (int i = 0; i < P.c1; i++, p++) {
            const uint32_t byte = p >= 2 ? fr[p] : 0u;
            s1 = (tab[byte ^ (s1 >> 8)] ^ (s1 << 8)) & 0xffffu;
        }
    }
    {
        int p = end2 - 64 * P.c2 + lane * P.c2;
        for (int i = 0; i < P.c2; i++, p++) {
            const uint32_t byte = p >= end1 ? fr[p] : 0u;
            s2 = (tab[byte ^ (s2 >> 8)] ^ (s2 << 8)) & 0xffffu;
        }
    }
    // ---- combine: both regions in one register, one shuffle per step ----
    uint32_t crc = s1 | (s2 << 16);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int d = 1 << k;
        const uint32_t left = __shfl_up(crc, d, 64);
        if (((lane + 1) & (2 * d - 1)) == 0) crc ^= crc_mul_tab(left & 0xffffu, P.pw1[k]) | (crc_mul_tab(left >> 16, P.pw2[k]) << 16);
    }
    const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)crc, 63);
    uint32_t v = ((r & 0xffffu) ? 1u : 0u) | ((r >> 16) ? 2u : 0u);
    if (v && P.conceal) v |= 0x40u;
    if (lane == 0) P.verdict[fidx] = (uint8_t)v;
}

static uint32_t crc_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

static uint32_t crc_gf_pow(uint32_t a, unsigned n)
{
    uint32_t r = 1;
    for (; n; n >>= 1, a = crc_gf_mul(a, a))
        if (n & 1u) r = crc_gf_mul(r, a);
    return r;
}

hipError_t launch_crc(const CrcLaunch &L, hipStream_t stream)
{
    if (L.n_frames == 0) return hipSuccess;
    if (L.n_frames > 0x7fffffffu || L.frame_bytes < 8 || L.frame_bytes > 3840) return hipErrorInvalidValue;
    CrcParams P;
    P.frames = L.frames;
    P.verdict = L.verdict;
    P.n_frames = (unsigned)L.n_frames;
    P.frame_stride = L.frame_stride;
    P.frame_bytes = L.frame_bytes;
    P.wide = (((uintptr_t)L.frames | (uintptr_t)L.frame_stride) & 15) == 0;
    P.acmod = L.acmod;
    P.lfeon = L.lfeon;
    P.conceal = L.conceal ? 1 : 0;
    // the longest regions a frame of up to frame_bytes can have: 2 fs58 grows with fs; fs - fs58 <= (3 fs + 11) / 8
    const int fs = L.frame_bytes >> 1;
    const int len1 = 2 * ((fs >> 1) + (fs >> 3)), len2 = (3 * fs + 11) / 4 + 1;
    P.c1 = (len1 + 63) / 64;
    P.c2 = (len2 + 63) / 64;
    for (int k = 0; k < 6; k++) {
        uint32_t v1 = crc_gf_pow(2, 8u * P.c1 * (1u << k)), v2 = crc_gf_pow(2, 8u * P.c2 * (1u << k));
        for (int i = 0; i < 16; i++) {
            P.pw1[k][i] = (uint16_t)v1;
            P.pw2[k][i] = (uint16_t)v2;
            v1 = crc_gf_mul(v1, 2);
            v2 = crc_gf_mul(v2, 2);
        }
    }
    const size_t lds = (size_t)CRC_WAVES * ((L.frame_bytes + 15) >> 4) * 16;
    hipLaunchKernelGGL(crc_kernel, dim3((P.n_frames + CRC_WAVES - 1) / CRC_WAVES), dim3(64 * CRC_WAVES), lds, stream, P);
    return hipGetLastError();
}

}  // namespace ac3mi
