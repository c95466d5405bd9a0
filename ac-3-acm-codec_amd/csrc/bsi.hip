// bsi.hip — syncinfo and BSI of AC-3 frames, read without decoding them (ac3mi_bsi_read, ac3mi_bsi_read_batch,
// ac3mi_set_encode_metadata_source).  bsi_parse below is the product's one statement of that syntax (A/52 5.3.1 - 5.3.2; the
// header test and the frame's size are sync_rule.h's): the host entry point and the kernel both call it, each with its own
// way of fetching the frame's dwords.
//
// One lane per frame: the BSI is a serial chain of about 20 conditional fields, each of which decides where the next one
// lies, so a wavefront per frame would keep 63 lanes idle.  The loads are per-lane dword loads at the frame's stride - bytes
// 0-11 up front (three loads in flight together: they hold everything up to origbs unless the optional fields are present),
// further dwords only when a field reaches them.  Uncoalesced, and on purpose: frames lie frame_stride (hundreds of bytes)
// apart, so each frame's head is a cache line of its own whichever lane asks for it.  Staging 64 heads through LDS would fetch
// the same 64 lines; it would only turn the rare later dwords of a long BSI (timecodes, addbsi) from a second request on a
// line already in L2 into an LDS read, for an LDS buffer, a barrier and a guess at how many bytes to stage.
#include "ac3mi_internal.h"
#include "sync_rule.h"

namespace ac3mi {

// MSB-first reader over the frame's big-endian dwords: fetch(i) = bytes 4i .. 4i + 3.  A field that would end behind `end`
// (bits) reads as 0 and sets `over`; no dword that starts at or behind `end` is ever fetched.
template <class F>
struct BsiBits {
    F fetch;
    uint32_t pos, end;
    bool over;
    __host__ __device__ uint32_t get(int n)            // n = 1..16
    {
        if (pos + n > end) { over = true; pos += n; return 0; }
        const uint32_t i = pos >> 5, sh = pos & 31;
        uint64_t w = (uint64_t)fetch(i) << 32;
        if (sh + n > 32) w |= fetch(i + 1);             // (the field straddles: dword i + 1 starts below `end`)
        pos += n;
        return (uint32_t)((w << sh) >> (64 - n));
    }
};

// bytes 0-5 and the BSI of one frame.  avail: bytes that may be read (>= 0); max_frame: the largest frame the caller holds
// (ac3mi_bsi_read_batch's frame_bytes), <= 0: the frame's own size is not tested (ac3mi_bsi_read)
template <class F>
__host__ __device__ inline void bsi_parse(F fetch, int avail, int max_frame, ac3mi_bsi_info &o)
{
    o = ac3mi_bsi_info{};
    o.verdict = AC3MI_BSI_NOT_READ;
    if (avail < 6) return;
    const uint32_t w0 = fetch(0), w1 = fetch(1);
    const int b4 = w1 >> 24, b5 = (w1 >> 16) & 0xff;
    if (!sync_header_ok(w0 >> 16, b4, b5)) return;
    if (max_frame > 0 && (int)sync_frame_bytes(b4) > max_frame) return;
    o.verdict = 0;
    o.fscod = (uint8_t)(b4 >> 6);
    o.frmsizecod = (uint8_t)(b4 & 63);
    o.bsid = (uint8_t)(b5 >> 3);
    o.bsmod = (uint8_t)(b5 & 7);
    o.cmixlev = o.surmixlev = o.dsurmod = o.dialnorm2 = 0xff;
    BsiBits<F> rd{fetch, 48u, 8u * (uint32_t)avail, false};
    const int acmod = rd.get(3);
    o.acmod = (uint8_t)acmod;
    if ((acmod & 1) && acmod != 1) o.cmixlev = (uint8_t)rd.get(2);
    if (acmod & 4) o.surmixlev = (uint8_t)rd.get(2);
    if (acmod == 2) o.dsurmod = (uint8_t)rd.get(2);
    o.lfeon = (uint8_t)rd.get(1);
    uint32_t present = 0;
    o.dialnorm = (uint8_t)rd.get(5);
    if (rd.get(1)) { present |= AC3MI_BSI_COMPRE; o.compr = (uint8_t)rd.get(8); }
    if (rd.get(1)) { present |= AC3MI_BSI_LANGCODE; o.langcod = (uint8_t)rd.get(8); }
    if (rd.get(1)) { present |= AC3MI_BSI_AUDPRODIE; o.audprodi = (uint8_t)rd.get(7); }
    if (acmod == 0) {
        o.dialnorm2 = (uint8_t)rd.get(5);
        if (rd.get(1)) { present |= AC3MI_BSI_COMPR2E; o.compr2 = (uint8_t)rd.get(8); }
        if (rd.get(1)) { present |= AC3MI_BSI_LANGCOD2E; o.langcod2 = (uint8_t)rd.get(8); }
        if (rd.get(1)) { present |= AC3MI_BSI_AUDPRODI2E; o.audprodi2 = (uint8_t)rd.get(7); }
    }
    o.copyrightb = (uint8_t)rd.get(1);
    o.origbs = (uint8_t)rd.get(1);
    if (rd.get(1)) { present |= AC3MI_BSI_TIMECOD1E; o.timecod1 = (uint16_t)rd.get(14); }
    if (rd.get(1)) { present |= AC3MI_BSI_TIMECOD2E; o.timecod2 = (uint16_t)rd.get(14); }
    if (rd.get(1)) {
        present |= AC3MI_BSI_ADDBSIE;
        o.addbsil = (uint8_t)rd.get(6);
        rd.pos += 8u * (o.addbsil + 1u);                // addbsi itself is not read, only held against the end
        if (rd.pos > rd.end) rd.over = true;
    }
    o.present = (uint16_t)present;
    if (rd.over) o.verdict |= AC3MI_BSI_OVERRUN;
    else o.block0_bit = (uint16_t)rd.pos;
    o.word = bsi_sanitise(bsi_word(o.dialnorm, o.bsmod, o.cmixlev == 0xff ? 1 : o.cmixlev, o.surmixlev == 0xff ? 1 : o.surmixlev,
                                   o.dsurmod == 0xff ? 0 : o.dsurmod, o.copyrightb, o.origbs));
}

void bsi_read_host(const uint8_t *buf, int len, ac3mi_bsi_info *out)
{
    auto fetch = [=](uint32_t i) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++) w = (w << 8) | (4 * i + k < (uint32_t)len ? buf[4 * i + k] : 0u);
        return w;
    };
    bsi_parse(fetch, len, 0, *out);
}

struct BsiParams {
    const uint8_t *frames;
    ac3mi_bsi_info *info;
    uint32_t *words;
    const uint8_t *crc;
    unsigned n_frames;
    int frame_stride, frame_bytes;
    int acmod, lfeon;
    uint32_t ctx_word, coded_mask;      // coded_mask: the bits of cmixlev / surmixlev / dsurmod the coded acmod sends
};

// FOLLOW: a word per frame for the encoder (BsiLaunch::words); else the record (BsiLaunch::info)
template <bool FOLLOW>
__global__ __launch_bounds__(64) void bsi_kernel(const BsiParams P)
{
    const unsigned f = blockIdx.x * 64u + threadIdx.x;
    if (f >= P.n_frames) return;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(P.frames + (size_t)f * P.frame_stride);
    const uint32_t ndw = (uint32_t)(P.frame_bytes + 3) >> 2;       // >= 2: the dwords of the frame's slot that may be read
    const uint32_t h0 = src[0], h1 = src[1], h2 = ndw > 2 ? src[2] : 0u;
    auto fetch = [=](uint32_t i) {
        // (i < ndw whenever the reader asks: it never starts a dword at or behind 8 frame_bytes bits; the test keeps a slip from reading outside)
        const uint32_t v = i == 0 ? h0 : i == 1 ? h1 : i == 2 ? h2 : i < ndw ? src[i] : 0u;
        return __builtin_bswap32(v);
    };
    ac3mi_bsi_info o;
    bsi_parse(fetch, P.frame_bytes, P.frame_bytes, o);
    if constexpr (FOLLOW) {
        uint32_t w = P.ctx_word;
        const bool refused = o.verdict != 0 || o.acmod != P.acmod || o.lfeon != P.lfeon || (P.crc && (P.crc[f] & 0x40));
        if (!refused) {
            const uint32_t sent = (o.cmixlev != 0xff ? 0x300u : 0u) | (o.surmixlev != 0xff ? 0xc00u : 0u) | (o.dsurmod != 0xff ? 0x3000u : 0u);
            const uint32_t take = 0xc0ffu | (sent & P.coded_mask);  // dialnorm, bsmod, copyrightb, origbs always
            w = (o.word & take) | (w & ~take);
        }
        P.words[f] = w;
    } else {
        P.info[f] = o;
    }
}

hipError_t launch_bsi(const BsiLaunch &L, hipStream_t stream)
{
    if (L.n_frames == 0) return hipSuccess;
    if (L.n_frames > 0x7fffffffu || L.frame_bytes < 8 || L.frame_bytes > 3840 || (L.info == nullptr) == (L.words == nullptr))
        return hipErrorInvalidValue;
    BsiParams P;
    P.frames = L.frames;
    P.info = L.info;
    P.words = L.words;
    P.crc = L.crc;
    P.n_frames = (unsigned)L.n_frames;
    P.frame_stride = L.frame_stride;
    P.frame_bytes = L.frame_bytes;
    P.acmod = L.acmod;
    P.lfeon = L.lfeon;
    P.ctx_word = L.ctx_word;
    const int a = L.coded_acmod;
    P.coded_mask = (((a & 1) && a != 1) ? 0x300u : 0u) | ((a & 4) ? 0xc00u : 0u) | (a == 2 ? 0x3000u : 0u);
    const dim3 grid((P.n_frames + 63u) / 64u);
    if (L.words) hipLaunchKernelGGL(bsi_kernel<true>, grid, dim3(64), 0, stream, P);
    else hipLaunchKernelGGL(bsi_kernel<false>, grid, dim3(64), 0, stream, P);
    return hipGetLastError();
}

// ac3mi_set_encode_drc_source 1: the source's dynamic-range words as the encoder's arrays (DynSrcLaunch, ac3mi_internal.h; the
// rule is include/ac3mi.h's).  One lane per frame, as above and for the same reason: the frame's compr fields come from
// bsi_parse, the six blocks' raw words from the front end (24 bytes a frame, two 16-byte-aligned loads' worth), and the result
// is 16 bytes a frame.  Runs after the front end (its status words and raw words) and ahead of the encoder.
struct DynSrcParams {
    const uint8_t *frames;
    const uint32_t *src_dyn, *status;
    uint8_t *codes;
    uint16_t *compr;
    unsigned n_frames;
    int frame_stride, frame_bytes, prog;
};

__global__ __launch_bounds__(64) void enc_dynrng_source_kernel(const DynSrcParams P)
{
    const unsigned f = blockIdx.x * 64u + threadIdx.x;
    if (f >= P.n_frames) return;
    uint32_t code[2][6] = {{0u, 0u, 0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u, 0u, 0u}}, compr[2] = {0u, 0u};
    // a frame the decoder refused or concealed (bit 8) or one with a failed block (bits 0-5) carries nothing
    if (!(P.status[f] & 0x13fu)) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(P.frames + (size_t)f * P.frame_stride);
        const uint32_t ndw = (uint32_t)(P.frame_bytes + 3) >> 2;
        const uint32_t h0 = src[0], h1 = src[1], h2 = ndw > 2 ? src[2] : 0u;
        auto fetch = [=](uint32_t i) {
            const uint32_t v = i == 0 ? h0 : i == 1 ? h1 : i == 2 ? h2 : i < ndw ? src[i] : 0u;
            return __builtin_bswap32(v);
        };
        ac3mi_bsi_info o;
        bsi_parse(fetch, P.frame_bytes, P.frame_bytes, o);
        if (o.verdict == 0) {                           // (always: the front end read the same header)
            const bool dual = o.acmod == 0;
            uint32_t c[2], e[2] = {0u, 0u};
            c[0] = (o.present & AC3MI_BSI_COMPRE) ? 0x100u | o.compr : 0u;
            c[1] = dual && (o.present & AC3MI_BSI_COMPR2E) ? 0x100u | o.compr2 : 0u;
            const int p0 = P.prog < 0 ? 0 : dual ? P.prog : 0;     // the source programme that becomes programme 0
            compr[0] = c[p0];
            compr[1] = P.prog < 0 ? c[1] : 0u;
            const uint32_t *raw = P.src_dyn + (size_t)f * 6;
            for (int b = 0; b < 6; b++) {
                const uint32_t w = raw[b];
                if (w & 0x100u) e[0] = w & 0xffu;
                if (dual && (w & 0x1000000u)) e[1] = (w >> 16) & 0xffu;
                code[0][b] = e[p0];
                code[1][b] = P.prog < 0 ? e[1] : 0u;
            }
        }
    }
    uint32_t *out = reinterpret_cast<uint32_t *>(P.codes + (size_t)f * 12);
    for (int k = 0; k < 3; k++)                          // [6][2] bytes: blocks 2k and 2k + 1
        out[k] = code[0][2 * k] | code[1][2 * k] << 8 | code[0][2 * k + 1] << 16 | code[1][2 * k + 1] << 24;
    reinterpret_cast<uint32_t *>(P.compr)[f] = compr[0] | compr[1] << 16;
}

hipError_t launch_dynrng_source(const DynSrcLaunch &L, hipStream_t stream)
{
    if (L.n_frames == 0) return hipSuccess;
    if (L.n_frames > 0x7fffffffu || L.frame_bytes < 8 || L.frame_bytes > 3840 || !L.frames || !L.src_dyn || !L.status || !L.codes ||
        !L.compr || ((uintptr_t)L.codes & 3) || ((uintptr_t)L.compr & 3) || L.prog < -1 || L.prog > 1)
        return hipErrorInvalidValue;
    DynSrcParams P;
    P.frames = L.frames;
    P.src_dyn = L.src_dyn;
    P.status = L.status;
    P.codes = L.codes;
    P.compr = L.compr;
    P.n_frames = (unsigned)L.n_frames;
    P.frame_stride = L.frame_stride;
    P.frame_bytes = L.frame_bytes;
    P.prog = L.prog;
    hipLaunchKernelGGL(enc_dynrng_source_kernel, dim3((P.n_frames + 63u) / 64u), dim3(64), 0, stream, P);
    return hipGetLastError();
}

}  // namespace ac3mi
