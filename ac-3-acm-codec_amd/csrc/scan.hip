// scan.hip — AC-3 frames found in device byte streams (ac3mi_frame_scan, ac3mi_frame_scan_batch, ac3mi_frame_gather_batch).
// The rule is stream_convert_ac3's resync rule (run_decode in stream.hip restates it for the byte-stream layer): test a
// header at p, hop over the frame if it is one, else move on by one byte - optionally (mode 1) with a candidate accepted only
// when both of its CRC regions sum to 0 (crc.hip's sums).  The header test is sync_rule.h's; scan_rule.h holds the walk's
// host twin.
//
// frame_scan_kernel: one wavefront per stream, four per workgroup.  The walk is serial per stream by design - the next
// position depends on this header - so the parallelism is across streams; inside a stream the wave works together where there
// is width to use:
//   hop     the header's 6 bytes come from two or three aligned dwords at the wave-uniform p, shifted into place; on a clean
//           stream that dependent read is the whole cost of a frame
//   search  where the test fails, each lane takes one aligned 16-byte load and tests its 16 positions against the following
//           bytes (the next lane's load), 63 x 16 positions a round; __ballot and find-first give the next candidate
//   CRC     (mode 1) the candidate is staged in LDS as it lies in memory (aligned 16-byte loads), each lane sums a chunk of each
//           region through the 256-entry table, six shuffle steps combine the 64 sums - crc_kernel's scheme: chunks aligned to
//           the region's END, zero bytes in front.  The chunk sizes and power tables come in four sets, for frames of up to
//           480 / 960 / 1920 / 3840 bytes, so that a short frame does not pay the longest frame's loop.
// No load is unaligned, none reaches the stream's stride, and no byte at or behind len enters a result.  Every loop moves
// its position forward and ends at len.
//
// frame_gather_kernel: one wavefront per slot of [n_streams][frames_per_stream]; aligned 16-byte loads (dwords when a base
// or a stride is not a multiple of 16), the bytes shifted into place in registers, 16-byte stores, the slot's tail zeroed
// in the same pass.
#include "scan_rule.h"

extern "C" int ac3mi_frame_scan(const uint8_t *buf, size_t len, int mode, int max_frames, ac3mi_frame_ref *refs,
                                ac3mi_scan_info *info)
{
    if (!buf || !refs || !info || (mode != 0 && mode != 1) || max_frames < 1 || (uint64_t)len > 0xffffffffull) return AC3MI_ERR_ARG;
    ac3mi::frame_scan_host(buf, len, mode, max_frames, refs, info);
    return AC3MI_OK;
}

#ifdef __HIPCC__
#include "ac3mi_internal.h"
#include "wave_ops.h"

namespace ac3mi {

constexpr int SCAN_WAVES = 4;
constexpr int SCAN_CLASSES = 4;                         // frames of up to 3840 >> (3 - class) bytes share a chunk size
constexpr int SCAN_STAGE_VECS = (3840 + 15 + 15) / 16;  // a 3840-byte frame from any byte offset, in 16-byte vectors

struct ScanParams {
    const uint8_t *bytes;
    const uint32_t *len;
    ac3mi_frame_ref *refs;
    ac3mi_scan_info *info;
    uint64_t stride;
    unsigned n_streams;
    int mode, max_frames;
    int c1[SCAN_CLASSES], c2[SCAN_CLASSES];             // chunk bytes per lane of the two regions
    uint16_t pw1[SCAN_CLASSES][6][16], pw2[SCAN_CLASSES][6][16];    // pw[class][k][i] = x^(8 c 2^k + i) mod poly
};

__device__ __forceinline__ uint32_t scan_rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// a * t[0] in GF(2)[x] / poly for a table t[i] = t[0] * x^i mod poly (crc.hip's crc_mul_tab)
__device__ __forceinline__ uint32_t scan_mul_tab(uint32_t a, const uint16_t *t)
{
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) c ^= (uint32_t)__builtin_amdgcn_sbfe((int)a, i, 1) & (uint32_t)t[i];
    return c;
}

// bytes [sh, sh + 4) of the 8 bytes lo, hi (sh = 0..3)
__device__ __forceinline__ uint32_t scan_align(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }

__global__ __launch_bounds__(64 * SCAN_WAVES) void frame_scan_kernel(const ScanParams P)
{
    __shared__ __attribute__((aligned(16))) uint4 stage[SCAN_WAVES][SCAN_STAGE_VECS];
    __shared__ uint16_t tab[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = (int)scan_rfl((uint32_t)(tid >> 6));
    {
        uint32_t c = (uint32_t)tid << 8;
#pragma unroll
        for (int j = 0; j < 8; j++) c = (c & 0x8000u) ? (((c << 1) & 0xffffu) ^ 0x8005u) : (c << 1);
        tab[tid] = (uint16_t)c;
    }
    __syncthreads();
    const unsigned sidx = blockIdx.x * SCAN_WAVES + (unsigned)wave;
    if (sidx >= P.n_streams) return;
    const uint8_t *src = P.bytes + (size_t)sidx * P.stride;
    const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
    const uint4 *src128 = reinterpret_cast<const uint4 *>(src);
    uint32_t len = scan_rfl(P.len[sidx]);
    if ((uint64_t)len > P.stride) len = (uint32_t)P.stride;        // (the contract is len <= stride: nothing behind the stride is read)
    ac3mi_frame_ref *refs = P.refs + (size_t)sidx * (size_t)P.max_frames;
    uint8_t *fr = reinterpret_cast<uint8_t *>(stage[wave]);

    uint32_t p = 0, n = 0, skipped = 0, rejected = 0, flags = 0;
    // p + 8 <= len, without wrapping
    while (len >= 8u && p <= len - 8u && n < (uint32_t)P.max_frames) {
        // ---- the header at p: bytes p .. p + 5 out of aligned dwords (the third one only where byte p + 5 lies in it) ----
        const uint32_t k = p >> 2, sh = p & 3u;
        const uint32_t d0 = src32[k], d1 = src32[k + 1];                // bytes up to 4 k + 7 <= p + 7 < len
        const uint32_t d2 = sh == 3u ? src32[k + 2] : 0u;               // starts at byte p + 5 < len <= stride: inside the stride; only byte p + 5 of it is used
        const uint32_t w0 = scan_rfl(scan_align(d1, d0, sh)), w1 = scan_rfl(scan_align(d2, d1, sh));
        const uint32_t fs = scan_header_size(w0, w1);
        if (fs) {
            if (fs > len - p) {                                         // the frame runs past len
                flags |= AC3MI_SCAN_INCOMPLETE;
                break;
            }
            bool take = true;
            if (P.mode) {
                // ---- the candidate into LDS as it lies in memory: byte i of the frame at fr[(p & 15) + i] ----
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t v0 = p >> 4, nv = ((p + fs + 15u) >> 4) - v0;    // <= SCAN_STAGE_VECS; the last vector ends at or before len rounded up to 16 <= stride
                uint4 v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t i = (uint32_t)lane + 64u * j;
                    v[j] = i < nv ? src128[(size_t)v0 + i] : make_uint4(0u, 0u, 0u, 0u);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t i = (uint32_t)lane + 64u * j;
                    if (i < nv) stage[wave][i] = v[j];
                }
                wave_sync();
                // ---- per-lane chunk sums; bytes in front of a region count as 0 ----
                const int cls = fs > 1920u ? 3 : fs > 960u ? 2 : fs > 480u ? 1 : 0;
                const int c1 = P.c1[cls], c2 = P.c2[cls];
                const int o = (int)(p & 15u), end1 = (int)scan_region1_end(fs), end2 = (int)(fs & ~1u);
                uint32_t s1 = 0, s2 = 0;
                {
                    int q = end1 - 64 * c1 + lane * c1;
                    for (int i = 0; i < c1; i++, q++) {
                        const uint32_t byte = q >= 2 ? fr[o + q] : 0u;
                        s1 = (tab[byte ^ (s1 >> 8)] ^ (s1 << 8)) & 0xffffu;
                    }
                }
                {
                    int q = end2 - 64 * c2 + lane * c2;
                    for (int i = 0; i < c2; i++, q++) {
                        const uint32_t byte = q >= end1 ? fr[o + q] : 0u;
                        s2 = (tab[byte ^ (s2 >> 8)] ^ (s2 << 8)) & 0xffffu;
                    }
                }
                // ---- combine: both regions in one register, one shuffle per step ----
                uint32_t crc = s1 | (s2 << 16);
#pragma unroll
                for (int kk = 0; kk < 6; kk++) {
                    const int d = 1 << kk;
                    const uint32_t left = __shfl_up(crc, d, 64);
                    if (((lane + 1) & (2 * d - 1)) == 0)
                        crc ^= scan_mul_tab(left & 0xffffu, P.pw1[cls][kk]) | (scan_mul_tab(left >> 16, P.pw2[cls][kk]) << 16);
                }
                take = (uint32_t)__builtin_amdgcn_readlane((int)crc, 63) == 0u;
            }
            if (take) {
                if (lane == 0) {
                    ac3mi_frame_ref r;
                    r.offset = p;
                    r.bytes = (uint16_t)fs;
                    r.sizecod = (uint8_t)(w1 & 0xffu);
                    r.reserved = 0;
                    refs[n] = r;
                }
                n++;
                p += fs;                                                // fs >= 128: forward, and p <= len still
                continue;
            }
            rejected++;
        }
        // ---- no frame at p: the next position in (p, len - 8] whose header passes, found by the whole wave ----
        // Lane l holds the aligned 16 bytes at a + 16 l and tests the 16 positions in them against its own bytes and the first 8
        // of lane l + 1; lane 63 only supplies lane 62, so a round covers 63 x 16 positions.  A position is tested only if it
        // lies in (p, len - 8]: every byte it looks at is then below len.
        const uint32_t last = len - 8u;                                 // the last position the walk may test
        uint32_t next = last + 1u;                                      // none found: the walk ends where p + 8 > len
        for (uint64_t a = (uint64_t)((p + 1u) & ~15u); a <= (uint64_t)last; a += 63u * 16u) {
            const uint64_t mine = a + 16u * (uint32_t)lane;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (mine < (uint64_t)len) v = src128[mine >> 4];            // a multiple of 16 below len <= stride, itself one: the 16 bytes lie inside the stride
            const uint32_t d[6] = {v.x, v.y, v.z, v.w, (uint32_t)__shfl_down(v.x, 1, 64), (uint32_t)__shfl_down(v.y, 1, 64)};
            uint32_t hits = 0;
            if (lane < 63) {
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint64_t x = mine + (uint32_t)j;
                    const uint32_t h0 = scan_align(d[(j >> 2) + 1], d[j >> 2], j & 3);
                    const uint32_t h1 = scan_align(d[(j >> 2) + 2], d[(j >> 2) + 1], j & 3);
                    if (x > (uint64_t)p && x <= (uint64_t)last && sync_header_ok_le(h0, h1)) hits |= 1u << j;
                }
            }
            const uint64_t any = __ballot(hits != 0u);
            if (any) {
                const int l = __builtin_ctzll(any);
                const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)hits, l);
                next = (uint32_t)(a + 16u * (uint32_t)l) + (uint32_t)__builtin_ctz(m);
                break;
            }
        }
        skipped += next - p;                                            // next > p
        p = next;
    }
    if (n == (uint32_t)P.max_frames && len >= 8u && p <= len - 8u) flags |= AC3MI_SCAN_CAPPED;
    if (lane == 0) {
        ac3mi_scan_info o;
        o.n_frames = n;
        o.consumed = p;
        o.skipped = skipped;
        o.rejected = rejected;
        o.flags = flags;
        o.reserved = 0;
        P.info[sidx] = o;
    }
}

struct GatherParams {
    const uint8_t *bytes;
    const ac3mi_frame_ref *refs;
    const ac3mi_scan_info *info;
    uint8_t *frames;
    uint64_t stride;
    unsigned n_slots;
    int max_frames, first_frame, frames_per_stream, frame_stride, frame_bytes;
};

// keeps bytes [0, keep) of the dword that starts `keep` bytes before the frame's end (keep <= 0: none, >= 4: all)
__device__ __forceinline__ uint32_t gather_keep(uint32_t v, int keep)
{
    return keep >= 4 ? v : keep <= 0 ? 0u : v & ((1u << (8 * keep)) - 1u);
}

// dwords DS .. DS + 4 of d, shifted left by bs bytes: 16 bytes from byte offset 4 DS + bs of the 32 in d
template <int DS>
__device__ __forceinline__ uint4 gather_shift(const uint32_t (&d)[8], uint32_t bs)
{
    return make_uint4(scan_align(d[DS + 1], d[DS], bs), scan_align(d[DS + 2], d[DS + 1], bs), scan_align(d[DS + 3], d[DS + 2], bs),
                      scan_align(d[DS + 4], d[DS + 3], bs));
}

// WIDE: the streams' base and stride and the slots' base and stride are multiples of 16
template <bool WIDE>
__global__ __launch_bounds__(64 * SCAN_WAVES) void frame_gather_kernel(const GatherParams P)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned slot = blockIdx.x * SCAN_WAVES + scan_rfl((uint32_t)(tid >> 6));
    if (slot >= P.n_slots) return;
    const unsigned s = slot / (unsigned)P.frames_per_stream, f = slot - s * (unsigned)P.frames_per_stream;
    const uint8_t *src = P.bytes + (size_t)s * P.stride;
    uint8_t *dst = P.frames + (size_t)slot * (size_t)P.frame_stride;
    // ---- the slot's frame: none (zeros) if the stream has no such frame, it is longer than frame_bytes, or its reference
    // does not lie inside the stream's stride (a list that did not come from the scan must not send a load outside) ----
    const uint32_t have = scan_rfl(P.info[s].n_frames);
    const uint64_t want = (uint64_t)(uint32_t)P.first_frame + f;
    uint32_t off = 0;
    int bytes = 0;
    if (want < (uint64_t)have && want < (uint64_t)(uint32_t)P.max_frames) {
        const uint32_t *r = reinterpret_cast<const uint32_t *>(P.refs + (size_t)s * (size_t)P.max_frames + (size_t)want);
        off = scan_rfl(r[0]);
        bytes = (int)(scan_rfl(r[1]) & 0xffffu);
        if (bytes > P.frame_bytes || (uint64_t)off + (uint32_t)bytes > P.stride) bytes = 0;
    }
    const uint64_t end = (uint64_t)off + (uint32_t)bytes;               // <= stride
    if constexpr (WIDE) {
        const uint4 *s128 = reinterpret_cast<const uint4 *>(src);
        uint4 *d128 = reinterpret_cast<uint4 *>(dst);
        const uint32_t ds = (off >> 2) & 3u, bs = off & 3u;
        const int nvec = P.frame_stride >> 4;
        for (int i = lane; i < nvec; i += 64) {
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (16 * i < bytes) {
                const uint64_t k = (uint64_t)(off >> 4) + (uint32_t)i;  // 16 k <= off + 16 i < end
                const uint4 lo = s128[k];
                const uint4 hi = (off & 15u) && 16 * (k + 1) < end ? s128[k + 1] : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                o = ds == 0u ? gather_shift<0>(d, bs) : ds == 1u ? gather_shift<1>(d, bs) : ds == 2u ? gather_shift<2>(d, bs) : gather_shift<3>(d, bs);
                const int keep = bytes - 16 * i;
                o.x = gather_keep(o.x, keep);
                o.y = gather_keep(o.y, keep - 4);
                o.z = gather_keep(o.z, keep - 8);
                o.w = gather_keep(o.w, keep - 12);
            }
            d128[i] = o;
        }
    } else {
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
        uint32_t *d32 = reinterpret_cast<uint32_t *>(dst);
        const uint32_t bs = off & 3u;
        const int ndw = P.frame_stride >> 2;
        for (int i = lane; i < ndw; i += 64) {
            uint32_t o = 0u;
            if (4 * i < bytes) {
                const uint64_t k = (uint64_t)(off >> 2) + (uint32_t)i;  // 4 k <= off + 4 i < end
                const uint32_t lo = s32[k];
                const uint32_t hi = bs && 4 * (k + 1) < end ? s32[k + 1] : 0u;
                o = gather_keep(scan_align(hi, lo, bs), bytes - 4 * i);
            }
            d32[i] = o;
        }
    }
}

static uint32_t scan_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

static uint32_t scan_gf_pow(uint32_t a, unsigned n)
{
    uint32_t r = 1;
    for (; n; n >>= 1, a = scan_gf_mul(a, a))
        if (n & 1u) r = scan_gf_mul(r, a);
    return r;
}

hipError_t launch_frame_scan(const ScanLaunch &L, hipStream_t stream)
{
    if (L.n_streams == 0) return hipSuccess;
    if (L.n_streams > 0x7fffffffu || L.stride > 0xffffffffull || (L.stride & 15) || ((uintptr_t)L.bytes & 15) || L.max_frames < 1 ||
        (L.mode != 0 && L.mode != 1))
        return hipErrorInvalidValue;
    ScanParams P;
    P.bytes = L.bytes;
    P.len = L.len;
    P.refs = L.refs;
    P.info = L.info;
    P.stride = L.stride;
    P.n_streams = (unsigned)L.n_streams;
    P.mode = L.mode;
    P.max_frames = L.max_frames;
    // per class, the longest regions any frame size of the class has (every fscod and frmsizecod the header test passes)
    for (int c = 0; c < SCAN_CLASSES; c++) {
        const uint32_t hi = 3840u >> (SCAN_CLASSES - 1 - c), lo = c ? 3840u >> (SCAN_CLASSES - c) : 0u;
        uint32_t len1 = 0, len2 = 0;
        for (uint32_t b4 = 0; b4 < 0xc0u; b4++) {
            const uint32_t fs = scan_header_size(0x770bu, b4);
            if (fs == 0 || fs <= lo || fs > hi) continue;
            const uint32_t e1 = scan_region1_end(fs);
            if (e1 > len1) len1 = e1;
            if ((fs & ~1u) - e1 > len2) len2 = (fs & ~1u) - e1;
        }
        P.c1[c] = (int)((len1 + 63) / 64);
        P.c2[c] = (int)((len2 + 63) / 64);
        for (int k = 0; k < 6; k++) {
            uint32_t v1 = scan_gf_pow(2, 8u * P.c1[c] * (1u << k)), v2 = scan_gf_pow(2, 8u * P.c2[c] * (1u << k));
            for (int i = 0; i < 16; i++) {
                P.pw1[c][k][i] = (uint16_t)v1;
                P.pw2[c][k][i] = (uint16_t)v2;
                v1 = scan_gf_mul(v1, 2);
                v2 = scan_gf_mul(v2, 2);
            }
        }
    }
    hipLaunchKernelGGL(frame_scan_kernel, dim3((P.n_streams + SCAN_WAVES - 1) / SCAN_WAVES), dim3(64 * SCAN_WAVES), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_frame_gather(const GatherLaunch &L, hipStream_t stream)
{
    const uint64_t slots = (uint64_t)L.n_streams * (uint64_t)(L.frames_per_stream > 0 ? L.frames_per_stream : 0);
    if (slots == 0) return hipSuccess;
    if (slots > 0x7fffffffu || L.stride > 0xffffffffull || (L.stride & 3) || ((uintptr_t)L.bytes & 3) || L.max_frames < 1 || L.first_frame < 0 ||
        L.frame_bytes < 8 || L.frame_bytes > 3840 || L.frame_stride < ((L.frame_bytes + 3) & ~3) || (L.frame_stride & 3) || ((uintptr_t)L.frames & 3))
        return hipErrorInvalidValue;
    GatherParams P;
    P.bytes = L.bytes;
    P.refs = L.refs;
    P.info = L.info;
    P.frames = L.frames;
    P.stride = L.stride;
    P.n_slots = (unsigned)slots;
    P.max_frames = L.max_frames;
    P.first_frame = L.first_frame;
    P.frames_per_stream = L.frames_per_stream;
    P.frame_stride = L.frame_stride;
    P.frame_bytes = L.frame_bytes;
    const bool wide = (((uintptr_t)L.bytes | (uintptr_t)L.stride | (uintptr_t)L.frames | (uintptr_t)L.frame_stride) & 15) == 0;
    const dim3 grid((P.n_slots + SCAN_WAVES - 1) / SCAN_WAVES);
    if (wide) hipLaunchKernelGGL(frame_gather_kernel<true>, grid, dim3(64 * SCAN_WAVES), 0, stream, P);
    else hipLaunchKernelGGL(frame_gather_kernel<false>, grid, dim3(64 * SCAN_WAVES), 0, stream, P);
    return hipGetLastError();
}

}  // namespace ac3mi
#endif  // __HIPCC__
