// capi.hip — the C-ABI of libac3mi.so (include/ac3mi.h): context, device memory,
// table construction and the batched entry points.
#include "ac3mi_internal.h"
#include "a52_levels.h"
#include "spec_tables.h"
#include "sync_rule.h"
#include "resample_rule.h"
#include "pcm_lanes.h"
#include "crc_lanes.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

namespace ac3mi {

static std::string g_err;   // errors raised without a context


// ---------------------------------------------------------------------------
// tables (double precision on the host, rounded once to float)

static double bessel_i0(double x)
{
    // L52/imdct.c:347-356: 100-term series in Horner form
    double b = 1;
    for (int i = 100; i > 0; i--) b = b * x / (i * i) + 1;
    return b;
}

void build_host_tables(float *window, float2 *tw_long, float2 *tw_short)
{
    const double pi = 3.14159265358979323846;
    // KBD window, alpha = 5 (L52/imdct.c:364-372)
    double acc = 0, cum[256];
    for (int i = 0; i < 256; i++) {
        acc += bessel_i0(i * (256 - i) * (5 * pi / 256) * (5 * pi / 256));
        cum[i] = acc;
    }
    acc += 1;
    for (int i = 0; i < 256; i++) window[i] = (float)sqrt(cum[i] / acc);

    // merged lane twiddles (xform_core.h): lane n2, register k1
    //   long : (-1)^n2 e^{-j pi (n2+63.75)/256} . e^{-j 2 pi n2 k1/128} . e^{-j pi (k1+.5)/256}
    //   short: e^{-j pi (n-.25)/128} . e^{-j 2 pi n k1/64} . e^{-j pi (k1+.5)/128},  n = lane & 3
    for (int l = 0; l < 8; l++)
        for (int k = 0; k < 16; k++) {
            double a = -pi * (l + 63.75) / 256 - 2 * pi * l * k / 128 - pi * (k + 0.5) / 256 + (l & 1 ? pi : 0);
            tw_long[l * 16 + k] = make_float2((float)cos(a), (float)sin(a));
            int n = l & 3;
            double b = -pi * (n - 0.25) / 128 - 2 * pi * n * k / 64 - pi * (k + 0.5) / 128;
            tw_short[l * 16 + k] = make_float2((float)cos(b), (float)sin(b));
        }
}

// decoder tables: L52/bit_allocate.c:31-101, L52/tables.h:49-246
// descriptor of a row byte (same function as decode_common.h's mant_desc, host copy)
static uint32_t mant_desc_host(uint32_t b)
{
    const uint32_t k1 = b >> 5, nbp = b & 31u;
    const uint32_t qbase = k1 == 1 ? 0u : k1 == 2 ? 96u : k1 == 3 ? 480u : nbp == 3 ? 736u : nbp == 4 ? 744u : 0u;
    const uint32_t per = k1 == 3 ? 2u : k1 ? 3u : 0u, obits = k1 == 1 ? 5u : k1 ? 7u : 0u;
    const uint32_t coded = (k1 || nbp == 3 || nbp == 4) ? 1u : 0u;
    return qbase | (per << 10) | (obits << 12) | (coded << 15);
}

void build_dec_tables(DecTables *t, uint16_t *lfsr_seq, uint16_t *lfsr_idx)
{
    uint8_t la[256];
    build_logadd(la);
    for (int i = 0; i < 256; i++) t->la_neg[i] = (int8_t)-la[i];
    memcpy(t->hth, kHth, sizeof t->hth);
    memcpy(t->width, kWidth, sizeof t->width);
    memcpy(t->band_end, kBandEnd, sizeof t->band_end);
    for (int i = 0; i < 256; i++) {
        int b = i < 20 ? i : 20;
        while (i >= 20 && b < 49 && i >= kBandEnd[b - 20]) b++;
        t->band_of_bin[i] = (uint8_t)b;
    }
    // Q(x) = ROUND(32768 x) for the symmetric quantiser levels (L52/tables.h:49)
    auto q = [](int num, int den) {
        double x = 32768.0 * num / den;
        return (float)(int)(x + (x > 0 ? 0.5 : -0.5));
    };
    memset(t->qlev, 0, sizeof t->qlev);
    for (int i = 0; i < 3; i++) t->qlev[i] = q(2 * (i - 1), 3);
    for (int i = 0; i < 5; i++) t->qlev[3 + i] = q(2 * (i - 2), 5);
    for (int i = 0; i < 7; i++) t->qlev[8 + i] = q(2 * (i - 3), 7);
    for (int i = 0; i < 11; i++) t->qlev[16 + i] = q(2 * (i - 5), 11);
    for (int i = 0; i < 15; i++) t->qlev[27 + i] = q(2 * (i - 7), 15);
    memset(t->qtab, 0, sizeof t->qtab);
    for (int code = 0; code < 27; code++) {
        t->qtab[code * 3 + 0] = t->qlev[code / 9];
        t->qtab[code * 3 + 1] = t->qlev[(code / 3) % 3];
        t->qtab[code * 3 + 2] = t->qlev[code % 3];
    }
    for (int code = 0; code < 125; code++) {
        t->qtab[96 + code * 3 + 0] = t->qlev[3 + code / 25];
        t->qtab[96 + code * 3 + 1] = t->qlev[3 + (code / 5) % 5];
        t->qtab[96 + code * 3 + 2] = t->qlev[3 + code % 5];
    }
    for (int code = 0; code < 121; code++) {
        t->qtab[480 + code * 2 + 0] = t->qlev[16 + code / 11];
        t->qtab[480 + code * 2 + 1] = t->qlev[16 + code % 11];
    }
    for (int code = 0; code < 7; code++) t->qtab[736 + code] = t->qlev[8 + code];
    for (int code = 0; code < 15; code++) t->qtab[744 + code] = t->qlev[27 + code];
    for (int b = 0; b < 128; b++) t->desc[b] = mant_desc_host((uint32_t)b);
    // dither generator (L52/parse.c:310-319, table L52/tables.h:213-246): one call advances a
    // 16-bit Galois LFSR (feedback 0xa011) by 8 steps.  It is GF(2)-linear with period 65535,
    // so the sequence from state 1 plus its inverse index give O(1) access to any later draw.
    uint16_t step8[256];
    step8[0] = 0;
    for (int i = 1; i < 256; i <<= 1) {
        uint16_t v = (i == 1) ? 0xa011 : (uint16_t)((step8[i >> 1] << 1) ^ ((step8[i >> 1] & 0x8000) ? 0xa011 : 0));
        step8[i] = v;
        for (int k = 1; k < i; k++) step8[i + k] = (uint16_t)(v ^ step8[k]);
    }
    memset(lfsr_idx, 0, 65536 * sizeof(uint16_t));
    uint16_t s = 1;
    for (int i = 0; i < 65535; i++) {
        lfsr_seq[i] = s;
        lfsr_idx[s] = (uint16_t)i;
        s = (uint16_t)(step8[s >> 8] ^ (uint16_t)(s << 8));
    }
}

// encoder tables: ENC/ac3tab.h and AC3_encode_init (ENC/ac3enc.cpp:977-1016, 1094-1104)
static int16_t fix15(float a)                        // ENC/ac3enc.cpp:428-439
{
    int v = (int)(a * (float)(1 << 15));
    if (v < -32767) v = -32767; else if (v > 32767) v = 32767;
    return (int16_t)v;
}

void build_enc_tables(EncTables *t)
{
    const double pi = 3.14159265358979323846;
    // ac3_window (ENC/ac3tab.h:15-48) = floor(32768 * KBD alpha-5 window)
    double acc = 0, cum[256];
    for (int i = 0; i < 256; i++) {
        acc += bessel_i0(i * (256 - i) * (5 * pi / 256) * (5 * pi / 256));
        cum[i] = acc;
    }
    acc += 1;
    for (int i = 0; i < 256; i++) t->win[i] = (int16_t)floor(32768.0 * sqrt(cum[i] / acc));
    // fft_init(7): cos/sin of a float argument -> float overloads in the reference's C++ unit (:441-459)
    for (int i = 0; i < 64; i++) {
        float alpha = (float)(2 * pi * (float)i / (float)128);
        t->cos[i] = fix15(cosf(alpha));
        t->sin[i] = fix15(sinf(alpha));
    }
    for (int i = 0; i < 128; i++) {
        int m = 0;
        for (int j = 0; j < 7; j++) m |= ((i >> j) & 1) << (6 - j);
        t->bitrev[i] = (uint8_t)m;
        float alpha = (float)(2 * pi * (i + 1.0 / 8.0) / (float)512);      // :1098-1102
        t->xcos[i] = fix15(-cosf(alpha));
        t->xsin[i] = fix15(-sinf(alpha));
    }
    for (int i = 0; i < 64; i++) {                                          // the same at N = 256 (short transform pair)
        float alpha = (float)(2 * pi * (i + 1.0 / 8.0) / (float)256);
        t->xcos2[i] = fix15(-cosf(alpha));
        t->xsin2[i] = fix15(-sinf(alpha));
    }
    build_logadd(t->latab);
    for (int b = 0; b < 50; b++)
        for (int f = 0; f < 3; f++) t->hth[b][f] = (uint16_t)(0xc00 - kHth[f][b]);
    // baptab: address (psd - mask) >> 5 -> bap code; same table as the decoder's widths, as codes
    for (int a = 0; a < 64; a++) {
        const int w = kWidth[63 - a];
        int code;
        switch (w) {
        case 0: code = 0; break;
        case -1: code = 1; break;
        case -2: code = 2; break;
        case 3: code = 3; break;
        case -3: code = 4; break;
        case 4: code = 5; break;
        case 14: code = 14; break;
        case 16: code = 15; break;
        default: code = w + 1; break;       // widths 5..12 -> codes 6..13
        }
        t->baptab[a] = (uint8_t)code;
    }
    // band structure: bins 0..27 are 1-wide, then kBandEnd
    int start = 0, k = 0;
    for (int b = 0; b < 50; b++) {
        const int end = b < 20 ? b + 1 : kBandEnd[b - 20];
        t->band_start[b] = (uint8_t)start;
        t->band_size[b] = (uint8_t)(end - start);
        for (; k < end; k++) t->band_of_bin[k] = (uint8_t)b;
        start = end;
    }
    for (; k < 256; k++) t->band_of_bin[k] = 49;
    t->band_start[50] = 0;
    for (int n = 0; n < 256; n++) {                                          // ac3_crc_init :998-1016
        unsigned c = (unsigned)n << 8;
        for (int j = 0; j < 8; j++) c = (c & 0x8000) ? (((c << 1) & 0xffff) ^ 0x8005) : (c << 1);
        t->crc_tab[n] = (uint16_t)c;
    }
}

int enc_config(int freq, int bitrate, int channels, EncConfig *c, int acmod, int lfeon)
{
    static const uint8_t acmod_of[6] = {1, 2, 3, 6, 7, 7};
    const int *rates = kSampleRates;
    if (channels < 1 || channels > 6) return 0;
    c->nch = channels;
    if (acmod < 0) {
        c->acmod = acmod_of[channels - 1];
        c->lfe = channels == 6;
        c->nfbw = channels > 5 ? 5 : channels;
    } else {
        if (acmod > 7 || lfeon < 0 || lfeon > 1 || channels != sync_nfchans(acmod) + lfeon) return 0;
        c->acmod = acmod;
        c->lfe = lfeon;
        c->nfbw = sync_nfchans(acmod);
    }
    bool found = false;
    for (int i = 0; i < 3 && !found; i++)
        for (int j = 0; j < 3; j++)
            if ((rates[j] >> i) == freq) { c->halfrate = i; c->fscod = j; found = true; break; }
    if (!found) return 0;
    c->bsid = 8 + c->halfrate;
    bitrate /= 1000;
    int i;
    for (i = 0; i < 19; i++) if ((int)(sync_kbps(i) >> c->halfrate) == bitrate) break;
    if (i == 19) return 0;
    c->frmsizecod = i << 1;
    c->frame_words = (bitrate * 1000 * 1536) / (freq * 16);
    return c->frame_words * 2;
}

// ---------------------------------------------------------------------------
// a52_downmix() as a plane-mixing matrix (L52/downmix.c:480-619) and the set of
// outputs a52_downmix_init() can grant (L52/downmix.c:37-67)

int build_mix_plan(int acmod, int lfeon, int output, MixPlan *plan)
{
    // row = requested output, column = coded acmod
    static const uint8_t grant[11][8] = {
        {0, 10, 2, 2, 2, 2, 2, 2},  {1, 1, 1, 1, 1, 1, 1, 1},  {0, 10, 2, 2, 2, 2, 2, 2}, {0, 10, 2, 3, 2, 3, 2, 3},
        {0, 10, 2, 2, 4, 4, 4, 4},  {0, 10, 2, 2, 4, 5, 4, 5}, {0, 10, 2, 3, 6, 6, 6, 6}, {0, 10, 2, 3, 6, 7, 6, 7},
        {8, 1, 1, 1, 1, 1, 1, 1},   {9, 1, 1, 1, 1, 1, 1, 1},  {0, 10, 2, 10, 10, 10, 10, 10}};
    if (acmod < 0 || acmod > 7) return AC3MI_ERR_ARG;
    const int out = output & AC3MI_CHANNEL_MASK;
    if (out > AC3MI_DOLBY) return AC3MI_ERR_ARG;
    if (grant[out][acmod] != out) return AC3MI_ERR_ARG;
    if ((output & AC3MI_LFE) && !lfeon) return AC3MI_ERR_ARG;

    memset(plan, 0, sizeof *plan);
    plan->nfchans = sync_nfchans(acmod);
    plan->in_lfe = lfeon ? 1 : 0;
    plan->n_in = plan->nfchans + plan->in_lfe;
    const int out_lfe = (output & AC3MI_LFE) ? 1 : 0;
    const int nfo = sync_nfchans(out);
    plan->n_out = nfo + out_lfe;

    int8_t m[5][5];
    memset(m, 0, sizeof m);
    auto id = [&](int n) { for (int i = 0; i < n; i++) m[i][i] = 1; };
    auto fold_centre = [&]() { m[0][0] = 1; m[0][1] = 1; m[1][2] = 1; m[1][1] = 1; };   // mix3to2
    const int A = acmod;

    switch (out) {
    case AC3MI_CHANNEL:  case AC3MI_CHANNEL1:
        id(nfo);                                                    // (0,0) identity; CHANNEL1 keeps plane 0
        break;
    case AC3MI_CHANNEL2:
        m[0][1] = 1;                                                // downmix.c:485-487
        break;
    case AC3MI_MONO:
        for (int c = 0; c < plan->nfchans; c++) m[0][c] = 1;        // mix2to1..mix5to1
        break;
    case AC3MI_STEREO:
        switch (A) {
        case 2: id(2); break;
        case 3: fold_centre(); break;
        case 4: m[0][0] = 1; m[1][1] = 1; m[0][2] = 1; m[1][2] = 1; break;                     // mix21to2
        case 5: fold_centre(); m[0][3] = 1; m[1][3] = 1; break;                                // mix31to2
        case 6: m[0][0] = 1; m[0][2] = 1; m[1][1] = 1; m[1][3] = 1; break;                     // 2x mix2to1
        case 7: fold_centre(); m[0][3] = 1; m[1][4] = 1; break;                                // mix32to2
        default: return AC3MI_ERR_ARG;
        }
        break;
    case AC3MI_DOLBY:
        switch (A) {
        case 1: m[0][0] = 1; m[1][0] = 1; break;                                               // memcpy
        case 2: id(2); break;
        case 3: fold_centre(); break;
        case 4: m[0][0] = 1; m[1][1] = 1; m[0][2] = -1; m[1][2] = 1; break;                    // mix21toS
        case 5: fold_centre(); m[0][3] = -1; m[1][3] = 1; break;                               // mix31toS
        case 6: m[0][0] = 1; m[1][1] = 1; m[0][2] = m[0][3] = -1; m[1][2] = m[1][3] = 1; break; // mix22toS
        case 7: fold_centre(); m[0][3] = m[0][4] = -1; m[1][3] = m[1][4] = 1; break;           // mix32toS
        default: return AC3MI_ERR_ARG;
        }
        break;
    case AC3MI_3F:
        id(3);
        if (A == 5) { m[0][3] = 1; m[2][3] = 1; }                                              // mix21to2
        if (A == 7) { m[0][3] = 1; m[2][4] = 1; }
        break;
    case AC3MI_2F1R:
        if (A == 4) id(3);
        else if (A == 5) { fold_centre(); m[2][3] = 1; }
        else if (A == 6) { id(2); m[2][2] = 1; m[2][3] = 1; }
        else if (A == 7) { fold_centre(); m[2][3] = 1; m[2][4] = 1; }                          // move2to1
        else return AC3MI_ERR_ARG;
        break;
    case AC3MI_3F1R:
        id(4);
        if (A == 7) m[3][4] = 1;
        break;
    case AC3MI_2F2R:
        if (A == 6) id(4);
        else if (A == 4) { id(3); m[3][2] = 1; }
        else if (A == 5) { fold_centre(); m[2][3] = 1; m[3][3] = 1; }
        else if (A == 7) { fold_centre(); m[2][3] = 1; m[3][4] = 1; }
        else return AC3MI_ERR_ARG;
        break;
    case AC3MI_3F2R:
        if (A == 7) id(5);
        else if (A == 5) { id(4); m[4][3] = 1; }
        else return AC3MI_ERR_ARG;
        break;
    }
    for (int o = 0; o < nfo; o++)
        for (int c = 0; c < plan->nfchans; c++) plan->mix[o + out_lfe][c + plan->in_lfe] = m[o][c];
    if (out_lfe) plan->mix[0][0] = 1;
    // the outputs whose time-domain mixers test slev == 0 (downmix.c:494-583), from the acmods with surround channels
    if ((A & 4) && (out == AC3MI_MONO || out == AC3MI_STEREO || out == AC3MI_3F)) {
        const int nsurr = A >= 6 ? 2 : 1;
        for (int c = plan->nfchans - nsurr; c < plan->nfchans; c++) plan->surr_mask |= (uint8_t)(1u << (c + plan->in_lfe));
        if (out == AC3MI_STEREO && !(A & 1)) plan->nobias_mask = (uint8_t)(3u << out_lfe);             // 2/1, 2/2: L and R
        if (out == AC3MI_3F) plan->nobias_mask = (uint8_t)(5u << out_lfe);                             // 3/1, 3/2: L and R, not C
    }
    return AC3MI_OK;
}

}  // namespace ac3mi

using namespace ac3mi;

#define HIPCHK(ctx, call)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            std::string msg_ = std::string(#call) + ": " + hipGetErrorString(e_);      \
            if (ctx) (ctx)->err = msg_; else g_err = msg_;                             \
            return AC3MI_ERR_HIP;                                                      \
        }                                                                              \
    } while (0)

// an AC3MI_* status other than AC3MI_OK returns from the caller
#define TRY(call)                                                                      \
    do {                                                                               \
        const int r_ = (call);                                                         \
        if (r_ != AC3MI_OK) return r_;                                                 \
    } while (0)

// Measurement aid: what one SIMD sustains in plain 32-bit VALU instructions while the whole chip is busy with them
// (the issue ceiling the instruction-bound kernels are priced against; the clock under such a load is not the
// data-sheet peak).  Every wavefront executes iters x 32 v_add_u32 / v_xor_b32 on eight independent registers.
namespace ac3mi {
__global__ __launch_bounds__(256) void valu_probe_kernel(uint32_t *out, int iters)
{
    uint32_t a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    const uint32_t k = blockIdx.x | 1u;
    for (int i = 0; i < iters; i++) {
        asm volatile(
            "v_add_u32 %0, %0, %8\n v_xor_b32 %1, %1, %8\n v_add_u32 %2, %2, %8\n v_xor_b32 %3, %3, %8\n"
            "v_add_u32 %4, %4, %8\n v_xor_b32 %5, %5, %8\n v_add_u32 %6, %6, %8\n v_xor_b32 %7, %7, %8\n"
            "v_add_u32 %0, %0, %8\n v_xor_b32 %1, %1, %8\n v_add_u32 %2, %2, %8\n v_xor_b32 %3, %3, %8\n"
            "v_add_u32 %4, %4, %8\n v_xor_b32 %5, %5, %8\n v_add_u32 %6, %6, %8\n v_xor_b32 %7, %7, %8\n"
            "v_add_u32 %0, %0, %8\n v_xor_b32 %1, %1, %8\n v_add_u32 %2, %2, %8\n v_xor_b32 %3, %3, %8\n"
            "v_add_u32 %4, %4, %8\n v_xor_b32 %5, %5, %8\n v_add_u32 %6, %6, %8\n v_xor_b32 %7, %7, %8\n"
            "v_add_u32 %0, %0, %8\n v_xor_b32 %1, %1, %8\n v_add_u32 %2, %2, %8\n v_xor_b32 %3, %3, %8\n"
            "v_add_u32 %4, %4, %8\n v_xor_b32 %5, %5, %8\n v_add_u32 %6, %6, %8\n v_xor_b32 %7, %7, %8\n"
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
            : "v"(k));
    }
    const uint32_t r = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
    if (r == 0x12345678u) out[0] = r;               // keeps the chain alive; practically never taken
}
// the same for the scalar unit: iters x 32 s_add_u32 / s_xor_b32 on four independent registers per wavefront
__global__ __launch_bounds__(256) void salu_probe_kernel(uint32_t *out, int iters)
{
    uint32_t s0 = blockIdx.x, s1 = s0 + 1, s2 = s0 + 2, s3 = s0 + 3;
    for (int i = 0; i < iters; i++) {
        asm volatile(
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            "s_add_u32 %0, %0, 1\n s_xor_b32 %1, %1, 3\n s_add_u32 %2, %2, 5\n s_xor_b32 %3, %3, 7\n"
            : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
    }
    if ((s0 ^ s1 ^ s2 ^ s3) == 0x12345678u) out[0] = s0;
}
// both at once, three vector instructions to one scalar one (the encoder's and the front end's mix): iters x (24 + 8) per wavefront
__global__ __launch_bounds__(256) void mixed_probe_kernel(uint32_t *out, int iters)
{
    uint32_t a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5;
    uint32_t s0 = blockIdx.x, s1 = s0 + 1, s2 = s0 + 2, s3 = s0 + 3;
    const uint32_t k = blockIdx.x | 1u;
    for (int i = 0; i < iters; i++) {
#define AC3MI_MIX4 "v_add_u32 %0, %0, %10\n v_xor_b32 %1, %1, %10\n v_add_u32 %2, %2, %10\n s_add_u32 %6, %6, 1\n" \
                   "v_xor_b32 %3, %3, %10\n v_add_u32 %4, %4, %10\n v_xor_b32 %5, %5, %10\n s_xor_b32 %7, %7, 3\n" \
                   "v_add_u32 %0, %0, %10\n v_xor_b32 %1, %1, %10\n v_add_u32 %2, %2, %10\n s_add_u32 %8, %8, 5\n" \
                   "v_xor_b32 %3, %3, %10\n v_add_u32 %4, %4, %10\n v_xor_b32 %5, %5, %10\n s_xor_b32 %9, %9, 7\n"
        asm volatile(AC3MI_MIX4 AC3MI_MIX4
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3)
                     : "v"(k) : "scc");
#undef AC3MI_MIX4
    }
    if ((a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ s0 ^ s1 ^ s2 ^ s3) == 0x12345678u) out[0] = a0;
}
}  // namespace ac3mi

// A table in device memory, put there by the first call of a context that needs it (*slot; freed in ac3mi_destroy)
template <class T>
static int upload_table_once(ac3mi_ctx *ctx, const char *who, const T *h, size_t bytes, T **slot)
{
    if (*slot) return AC3MI_OK;
    T *d = nullptr;
    if (hipMalloc((void **)&d, bytes) != hipSuccess) { ctx->err = std::string(who) + ": out of memory"; return AC3MI_ERR_HIP; }
    hipError_t e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);       // h leaves scope
    if (e != hipSuccess) { (void)hipFree(d); ctx->err = std::string(who) + ": " + hipGetErrorString(e); return AC3MI_ERR_HIP; }
    *slot = d;
    return AC3MI_OK;
}

// The device read-out of a PCM tool: [n_streams] states -> [n_streams] records; launch() does what lies behind the checks
template <class F>
static int read_batch(ac3mi_ctx *ctx, const char *who, const void *d_state, int n_streams, const void *d_results, const F &launch)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!d_state || !d_results || n_streams < 0 || ((uintptr_t)d_state & 7) || ((uintptr_t)d_results & 7)) {
        ctx->err = std::string(who) + ": bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return launch();
}

extern "C" {

int ac3mi_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *ac3mi_last_error(const ac3mi_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

static int ctx_init(ac3mi_ctx *ctx)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIPCHK(ctx, hipEventCreate(&ctx->ev0));
    HIPCHK(ctx, hipEventCreate(&ctx->ev1));
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    std::vector<float> win(256);
    std::vector<float2> twl(128), tws(128);
    build_host_tables(win.data(), twl.data(), tws.data());
    HIPCHK(ctx, hipMalloc(&ctx->tab.window, 256 * sizeof(float)));
    HIPCHK(ctx, hipMalloc(&ctx->tab.tw_long, 128 * sizeof(float2)));
    HIPCHK(ctx, hipMalloc(&ctx->tab.tw_short, 128 * sizeof(float2)));
    HIPCHK(ctx, hipMemcpy(ctx->tab.window, win.data(), 256 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->tab.tw_long, twl.data(), 128 * sizeof(float2), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->tab.tw_short, tws.data(), 128 * sizeof(float2), hipMemcpyHostToDevice));
    {
        DecTables dt;
        // (the sequence runs on for LFSR_EXT entries past its period: mant_kernel indexes a block's draws without a modulo)
        constexpr int LFSR_EXT = 16384;
        std::vector<uint16_t> seq(65535 + LFSR_EXT), idx(65536);
        build_dec_tables(&dt, seq.data(), idx.data());
        for (int i = 0; i < LFSR_EXT; i++) seq[65535 + i] = seq[i];
        HIPCHK(ctx, hipMalloc(&ctx->tab.dec, sizeof dt));
        HIPCHK(ctx, hipMalloc(&ctx->tab.lfsr_seq, seq.size() * sizeof(uint16_t)));
        HIPCHK(ctx, hipMalloc(&ctx->tab.lfsr_idx, 65536 * sizeof(uint16_t)));
        HIPCHK(ctx, hipMemcpy(ctx->tab.dec, &dt, sizeof dt, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(ctx->tab.lfsr_seq, seq.data(), seq.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(ctx->tab.lfsr_idx, idx.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    {
        EncTables et;
        build_enc_tables(&et);
        HIPCHK(ctx, hipMalloc(&ctx->tab.enc, sizeof et));
        HIPCHK(ctx, hipMemcpy(ctx->tab.enc, &et, sizeof et, hipMemcpyHostToDevice));
    }
    return AC3MI_OK;
}

ac3mi_ctx *ac3mi_create(int device)
{
    int n = ac3mi_device_count();
    if (n <= 0) {
        g_err = "ac3mi_create: no HIP device visible (libac3mi has no CPU fallback)";
        return nullptr;
    }
    if (device < 0 || device >= n) {
        g_err = "ac3mi_create: device index out of range";
        return nullptr;
    }
    ac3mi_ctx *ctx = new ac3mi_ctx();
    ctx->device = device;
    if (const char *e = getenv("AC3MI_DECODE_MODE")) {          // test aid: default front-end variant (ac3mi_set_decode_mode)
        const int m = atoi(e);
        if (m >= 0 && m <= 6 && m != 2) ctx->decode_mode = m;
    }
    if (const char *e = getenv("AC3MI_ENCODE_MODE")) {          // test aid: default packer variant (ac3mi_set_encode_mode)
        const int m = atoi(e);
        if (m >= 0 && m <= 2) ctx->encode_mode = m;
    }
    if (ctx_init(ctx) != AC3MI_OK) {
        g_err = ctx->err;
        delete ctx;
        return nullptr;
    }
    return ctx;
}

void ac3mi_destroy(ac3mi_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(ctx->tab.window);
    (void)hipFree(ctx->tab.tw_long);
    (void)hipFree(ctx->tab.tw_short);
    (void)hipFree(ctx->tab.dec);
    (void)hipFree(ctx->tab.lfsr_seq);
    (void)hipFree(ctx->tab.lfsr_idx);
    for (DevBuf *b : ac3mi_ctx::workspaces(ctx)) (void)hipFree(b->p);
    (void)hipFree(ctx->tab.enc);
    (void)hipFree(ctx->loud_tab);
    for (uint32_t *t : ctx->resample_tab) (void)hipFree(t);
    for (const auto &e : ctx->crc_rows) (void)hipFree(e.second);
    (void)hipEventDestroy(ctx->ev0);
    (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

void *ac3mi_dev_alloc(ac3mi_ctx *ctx, size_t bytes)
{
    void *p = nullptr;
    if (!ctx) return nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) {
        ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return nullptr;
    }
    return p;
}

void ac3mi_dev_free(ac3mi_ctx *ctx, void *d_ptr)
{
    if (!ctx || !d_ptr) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_ptr);
}

int ac3mi_memcpy_h2d(ac3mi_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    if (!ctx) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return AC3MI_OK;
}

int ac3mi_memcpy_d2h(ac3mi_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    if (!ctx) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return AC3MI_OK;
}

int ac3mi_memset(ac3mi_ctx *ctx, void *d_dst, int byte, size_t bytes)
{
    if (!ctx) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipMemsetAsync(d_dst, byte, bytes, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_memcpy_d2d(ac3mi_ctx *ctx, void *d_dst, const void *d_src, size_t bytes)
{
    if (!ctx) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_sync(ac3mi_ctx *ctx)
{
    if (!ctx) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return AC3MI_OK;
}

int ac3mi_timer_start(ac3mi_ctx *ctx)
{
    if (!ctx) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_timer_stop(ac3mi_ctx *ctx, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return AC3MI_OK;
}

int ac3mi_probe_valu_rate(ac3mi_ctx *ctx, double *ginst_per_s_per_simd)
{
    if (!ctx || !ginst_per_s_per_simd) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const int cus = prop.multiProcessorCount, wg_per_cu = 8, iters = 8192;        // 8 wavefronts per SIMD
    uint32_t *d = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d, 64));
    hipLaunchKernelGGL(valu_probe_kernel, dim3(cus * wg_per_cu), dim3(256), 0, ctx->stream, d, 64);       // warm-up
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(valu_probe_kernel, dim3(cus * wg_per_cu), dim3(256), 0, ctx->stream, d, iters);
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    (void)hipFree(d);
    // per SIMD: wg_per_cu workgroups x 4 wavefronts / 4 SIMDs = wg_per_cu wavefronts, 32 instructions per iteration each
    *ginst_per_s_per_simd = (double)wg_per_cu * iters * 32.0 / (ms * 1e-3) / 1e9;
    return AC3MI_OK;
}

int ac3mi_probe_salu_rate(ac3mi_ctx *ctx, double *ginst_per_s_per_simd)
{
    if (!ctx || !ginst_per_s_per_simd) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const int cus = prop.multiProcessorCount, wg_per_cu = 8, iters = 4096;        // 8 wavefronts per SIMD
    uint32_t *d = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d, 64));
    hipLaunchKernelGGL(salu_probe_kernel, dim3(cus * wg_per_cu), dim3(256), 0, ctx->stream, d, 64);       // warm-up
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(salu_probe_kernel, dim3(cus * wg_per_cu), dim3(256), 0, ctx->stream, d, iters);
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    (void)hipFree(d);
    *ginst_per_s_per_simd = (double)wg_per_cu * iters * 32.0 / (ms * 1e-3) / 1e9;
    return AC3MI_OK;
}

int ac3mi_probe_mixed_rate(ac3mi_ctx *ctx, int waves_per_simd, double *valu_ginst_per_s_per_simd, double *salu_ginst_per_s_per_simd)
{
    if (!ctx || !valu_ginst_per_s_per_simd || !salu_ginst_per_s_per_simd || waves_per_simd < 1 || waves_per_simd > 8) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const int cus = prop.multiProcessorCount, wg_per_cu = waves_per_simd, iters = 8192;      // a 256-thread workgroup = one wavefront per SIMD
    uint32_t *d = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d, 64));
    hipLaunchKernelGGL(mixed_probe_kernel, dim3(cus * wg_per_cu), dim3(256), 0, ctx->stream, d, 64);      // warm-up
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(mixed_probe_kernel, dim3(cus * wg_per_cu), dim3(256), 0, ctx->stream, d, iters);
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    (void)hipFree(d);
    *valu_ginst_per_s_per_simd = (double)wg_per_cu * iters * 24.0 / (ms * 1e-3) / 1e9;
    *salu_ginst_per_s_per_simd = (double)wg_per_cu * iters * 8.0 / (ms * 1e-3) / 1e9;
    return AC3MI_OK;
}

// one float4 per lane and the workgroup ends: the copy the guide quotes (MI355X_MICROARCH.md, HBM) and the fastest one
// measured on this part (profiles/hbm_calibrate)
__global__ __launch_bounds__(256) void copy_probe_kernel(const float4 *__restrict__ a, float4 *__restrict__ b, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) b[i] = a[i];
}

int ac3mi_probe_copy_rate(ac3mi_ctx *ctx, size_t bytes, double *gbytes_per_s)
{
    if (!ctx || !gbytes_per_s || bytes < (1u << 20)) return AC3MI_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = bytes / 16;
    float4 *a = nullptr, *b = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&a, n * 16));
    if (hipMalloc((void **)&b, n * 16) != hipSuccess) { (void)hipFree(a); ctx->err = "ac3mi_probe_copy_rate: out of memory"; return AC3MI_ERR_HIP; }
    (void)hipMemsetAsync(a, 0, n * 16, ctx->stream);
    const unsigned grid = (unsigned)((n + 255) / 256);
    float best = 1e30f;
    for (int it = 0; it < 6; it++) {
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        hipLaunchKernelGGL(copy_probe_kernel, dim3(grid), dim3(256), 0, ctx->stream, a, b, n);
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        if (hipEventSynchronize(ctx->ev1) != hipSuccess) break;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess && it > 0 && ms < best) best = ms;
    }
    (void)hipFree(a);
    (void)hipFree(b);
    if (best > 1e29f) { ctx->err = "ac3mi_probe_copy_rate: timing failed"; return AC3MI_ERR_HIP; }
    *gbytes_per_s = 2.0 * (double)(n * 16) / (best * 1e-3) / 1e9;
    return AC3MI_OK;
}

int ac3mi_set_state_slots(ac3mi_ctx *ctx, const int32_t *d_slots)
{
    if (!ctx) return AC3MI_ERR_ARG;
    ctx->slots = d_slots;
    return AC3MI_OK;
}

int ac3mi_set_mix_state(ac3mi_ctx *ctx, float *d_pending, int32_t *d_flags)
{
    if (!ctx || ((d_pending == nullptr) != (d_flags == nullptr))) return AC3MI_ERR_ARG;
    ctx->mix_pending = d_pending;
    ctx->mix_flags = d_flags;
    return AC3MI_OK;
}

int ac3mi_set_decode_mode(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 6 || mode == 2) return AC3MI_ERR_ARG;       // (2: the one-kernel front end per frame, retired in round 4)
    ctx->decode_mode = mode;
    return AC3MI_OK;
}

int ac3mi_set_fixed_shape(ac3mi_ctx *ctx, int on)
{
    if (!ctx || on < 0 || on > 1) return AC3MI_ERR_ARG;
    ctx->fixed_shape = on;
    return AC3MI_OK;
}

int ac3mi_debug_search_curve(ac3mi_ctx *ctx, int32_t *d_curve)
{
    if (!ctx) return AC3MI_ERR_ARG;
    ctx->debug_search_curve = d_curve;
    return AC3MI_OK;
}

int ac3mi_debug_launch_log(ac3mi_ctx *ctx, uint32_t *h_log, int capacity)
{
    if (!ctx || (h_log && capacity < 1)) return AC3MI_ERR_ARG;
    ctx->launch_log.words = h_log;
    ctx->launch_log.capacity = h_log ? capacity : 0;
    if (h_log) h_log[0] = 0;
    return AC3MI_OK;
}

int ac3mi_set_decode_crc(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return AC3MI_ERR_ARG;
    ctx->decode_crc = mode;
    return AC3MI_OK;
}

int ac3mi_set_encode_mode(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return AC3MI_ERR_ARG;
    ctx->encode_mode = mode;
    return AC3MI_OK;
}

int ac3mi_set_encode_block_switch(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 1) return AC3MI_ERR_ARG;
    ctx->tools.block_switch = mode;
    return AC3MI_OK;
}

int ac3mi_set_encode_rematrix(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 1) return AC3MI_ERR_ARG;
    ctx->tools.rematrix = mode;
    return AC3MI_OK;
}

int ac3mi_set_encode_coupling(ac3mi_ctx *ctx, int mode, int begf)
{
    if (!ctx || mode < 0 || mode > 1 || begf < 0 || begf > 12) return AC3MI_ERR_ARG;
    ctx->tools.coupling = mode;
    ctx->tools.cpl_begf = begf;
    return AC3MI_OK;
}

int ac3mi_set_encode_bandwidth(ac3mi_ctx *ctx, int mode, int chbwcod)
{
    if (!ctx || mode < 0 || mode > 2 || (mode == 1 && (chbwcod < 0 || chbwcod > 50))) return AC3MI_ERR_ARG;
    ctx->tools.bw_mode = mode;
    ctx->tools.bw_chbwcod = mode == 1 ? chbwcod : 50;
    return AC3MI_OK;
}

// the chbwcod a call codes with (ac3mi_set_encode_bandwidth's rule, include/ac3mi.h); callers pass a descriptor enc_config
// accepted and the layout's number of full-bandwidth channels (a count outside 1..5 gets 50 here rather than a division by zero)
static int call_chbwcod(const ac3mi_ctx *ctx, const ac3mi_encode_desc *d, int nfbw)
{
    if (ctx->tools.bw_mode == 1) return ctx->tools.bw_chbwcod;
    if (ctx->tools.bw_mode != 2 || nfbw < 1 || nfbw > 5) return 50;
    const long long r = d->bit_rate / nfbw;
    if (r >= 96000) return 50;
    const long long fc = r >= 80000 ? 18000 : r >= 64000 ? 16000 : r >= 48000 ? 14000 : r >= 32000 ? 11000 : 8000;
    int c = 0;
    for (int k = 0; k <= 50; k++)
        if ((73LL + 3 * k) * d->sample_rate <= 512 * fc) c = k;
    return c;
}

int ac3mi_encode_metadata_word(const ac3mi_encode_metadata *md, uint32_t *word)
{
    if (!md || !word) return AC3MI_ERR_ARG;
    auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
    if (!in(md->dialnorm, 1, 31) || !in(md->bsmod, 0, 7) || !in(md->cmixlev, 0, 2) || !in(md->surmixlev, 0, 2) ||
        !in(md->dsurmod, 0, 2) || !in(md->copyrightb, 0, 1) || !in(md->origbs, 0, 1))
        return AC3MI_ERR_ARG;
    *word = ac3mi::bsi_word(md->dialnorm, md->bsmod, md->cmixlev, md->surmixlev, md->dsurmod, md->copyrightb, md->origbs);
    return AC3MI_OK;
}

int ac3mi_set_encode_metadata(ac3mi_ctx *ctx, const ac3mi_encode_metadata *md)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!md) {
        ctx->tools.bsi = ac3mi::BSI_DEFAULT;
        return AC3MI_OK;
    }
    if (ac3mi_encode_metadata_word(md, &ctx->tools.bsi) != AC3MI_OK) {
        ctx->err = "ac3mi_set_encode_metadata: field out of range";
        return AC3MI_ERR_ARG;
    }
    return AC3MI_OK;
}

int ac3mi_set_encode_metadata_frames(ac3mi_ctx *ctx, const uint32_t *d_words)
{
    if (!ctx || ((uintptr_t)d_words & 3)) return AC3MI_ERR_ARG;
    ctx->tools.bsi_words = d_words;
    return AC3MI_OK;
}

int ac3mi_set_encode_metadata_source(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 1) return AC3MI_ERR_ARG;
    ctx->tools.md_source = mode;
    return AC3MI_OK;
}

int ac3mi_set_encode_drc(ac3mi_ctx *ctx, int profile, int32_t *d_drc_state)
{
    if (!ctx || profile < 0 || profile > 5 || (profile != 0 && !d_drc_state)) return AC3MI_ERR_ARG;
    if (profile != 0 && ctx->tools.dyn_codes) {
        ctx->err = "ac3mi_set_encode_drc: the dynrng words are set by ac3mi_set_encode_dynrng_frames";
        return AC3MI_ERR_ARG;
    }
    ctx->tools.drc_profile = profile;
    ctx->tools.drc_state = profile ? d_drc_state : nullptr;
    return AC3MI_OK;
}

int ac3mi_set_encode_dynrng_frames(ac3mi_ctx *ctx, const uint8_t *d_dynrng, const uint16_t *d_compr)
{
    if (!ctx || ((uintptr_t)d_compr & 1)) return AC3MI_ERR_ARG;
    if (d_dynrng && ctx->tools.drc_profile) {
        ctx->err = "ac3mi_set_encode_dynrng_frames: the dynrng words are a profile's (ac3mi_set_encode_drc)";
        return AC3MI_ERR_ARG;
    }
    ctx->tools.dyn_codes = d_dynrng;
    ctx->tools.compr_words = d_compr;
    return AC3MI_OK;
}

int ac3mi_set_encode_drc_source(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 1) return AC3MI_ERR_ARG;
    ctx->tools.drc_source = mode;
    return AC3MI_OK;
}

int ac3mi_set_encode_exp_strategy(ac3mi_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 1) return AC3MI_ERR_ARG;
    ctx->tools.exp_strategy = mode;
    return AC3MI_OK;
}

int ac3mi_set_encode_layout(ac3mi_ctx *ctx, int mode, int acmod, int lfeon)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (mode < 0 || mode > 2 || (mode == 1 && (acmod < 0 || acmod > 7 || lfeon < 0 || lfeon > 1))) {
        ctx->err = "ac3mi_set_encode_layout: mode outside 0..2, or a mode-1 acmod / lfeon out of range";
        return AC3MI_ERR_ARG;
    }
    ctx->tools.layout_mode = mode;
    ctx->tools.layout_acmod = mode == 1 ? acmod : 0;
    ctx->tools.layout_lfeon = mode == 1 ? lfeon : 0;
    return AC3MI_OK;
}

// the layout an encode call codes (ac3mi_set_encode_layout): mode 1's, or -1 for the reference's table (mode 0; mode 2 on
// ac3mi_encode_batch, which has no source)
static int call_acmod(const ac3mi_ctx *ctx) { return ctx->tools.layout_mode == 1 ? ctx->tools.layout_acmod : -1; }

// mode 2 on a transcode: the coded layout of the decoder's granted output flags (CHANNEL1 / CHANNEL2: 1/0, DOLBY: 2/0)
static int granted_acmod(int out_flags)
{
    const int cfg = out_flags & AC3MI_CHANNEL_MASK;
    return cfg <= 7 ? cfg : cfg == AC3MI_DOLBY ? 2 : 1;
}

int ac3mi_set_tile_frames(ac3mi_ctx *ctx, long long frames)
{
    if (!ctx || frames < 0) return AC3MI_ERR_ARG;
    ctx->tile_frames = frames;
    return AC3MI_OK;
}

// Streams per tile when a batch of n_streams x frames_per_stream is above the workspace bound, else 0 (no tiling).
static int tile_streams(const ac3mi_ctx *ctx, int n_streams, int frames_per_stream)
{
    if (!ctx->tile_frames || n_streams < 2 || frames_per_stream < 1) return 0;
    if ((long long)n_streams * frames_per_stream <= ctx->tile_frames) return 0;
    const long long g = ctx->tile_frames / frames_per_stream;
    return (int)(g < 1 ? 1 : g);
}

// The context's per-stream pointers while a batch goes through in tiles: at(s0) points them at the tile's first stream s0
// (the state slots when set, else the mix state of mix_n_out chains a stream - 0: it stays - and with `drc` the encoder's
// DRC state; with `drc` also the per-frame metadata words and the per-frame dynrng / compr arrays, which go by the frame's
// position in the call, slots or not); the destructor puts them back.
struct TileState {
    ac3mi_ctx *ctx;
    int mix_n_out;
    bool drc;
    int frames_per_stream;
    const int32_t *slots;
    float *mix_pending;
    int32_t *mix_flags, *drc_state;
    const uint32_t *bsi_words;
    const uint8_t *dyn_codes;
    const uint16_t *compr_words;
    TileState(ac3mi_ctx *c, int mix_n_out, bool drc, int frames_per_stream)
        : ctx(c), mix_n_out(mix_n_out), drc(drc), frames_per_stream(frames_per_stream), slots(c->slots), mix_pending(c->mix_pending),
          mix_flags(c->mix_flags), drc_state(c->tools.drc_state), bsi_words(c->tools.bsi_words),
          dyn_codes(c->tools.dyn_codes), compr_words(c->tools.compr_words) {}
    void at(int s0)
    {
        if (drc && bsi_words) ctx->tools.bsi_words = bsi_words + (size_t)s0 * frames_per_stream;
        if (drc && dyn_codes) ctx->tools.dyn_codes = dyn_codes + (size_t)s0 * frames_per_stream * 12;
        if (drc && compr_words) ctx->tools.compr_words = compr_words + (size_t)s0 * frames_per_stream * 2;
        if (slots) { ctx->slots = slots + s0; return; }
        if (mix_n_out && mix_pending) {
            ctx->mix_pending = mix_pending + (size_t)s0 * mix_n_out * 128;
            ctx->mix_flags = mix_flags + (size_t)s0 * 6;
        }
        if (drc && drc_state) ctx->tools.drc_state = drc_state + s0;
    }
    ~TileState()
    {
        ctx->slots = slots;
        ctx->mix_pending = mix_pending;
        ctx->mix_flags = mix_flags;
        ctx->tools.drc_state = drc_state;
        ctx->tools.bsi_words = bsi_words;
        ctx->tools.dyn_codes = dyn_codes;
        ctx->tools.compr_words = compr_words;
    }
};

// Grows a workspace to `need` bytes if it holds fewer; its contents are not kept.  The context's stream is synchronised
// before the old buffer is freed.
static int ws_grow(ac3mi_ctx *ctx, DevBuf &b, size_t need)
{
    if (need <= b.bytes) return AC3MI_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    HIPCHK(ctx, hipMalloc(&b.p, need));
    b.bytes = need;
    return AC3MI_OK;
}

size_t ac3mi_workspace_bytes(const ac3mi_ctx *ctx)
{
    if (!ctx) return 0;
    size_t n = 0;
    for (const DevBuf *b : ac3mi_ctx::workspaces(ctx)) n += b->bytes;
    return n;
}

int ac3mi_fill_workspaces(ac3mi_ctx *ctx, int byte)
{
    if (!ctx || byte < 0 || byte > 255) return AC3MI_ERR_ARG;
    for (const DevBuf *b : ac3mi_ctx::workspaces(ctx))
        if (b->bytes) HIPCHK(ctx, hipMemsetAsync(b->p, byte, b->bytes, ctx->stream));
    return AC3MI_OK;
}

// the decoder's workspaces for nfr frames: coefficient planes (ws_coef), block-switch flags with the per-frame "surround
// level 0" flags after them at zs_off (ws_blksw), the frame-parallel front end's draw counts and LFSR states (ws_draws), the
// split front end's descriptors, generator positions, coupling coordinates and row sets (ws_split)
static size_t coef_bytes(size_t nfr, int n_in) { return nfr * 6 * n_in * 256 * sizeof(float); }
static size_t zs_off(size_t nfr, int nfchans) { return nfr * 6 * nfchans + 4; }
static size_t split_bytes(size_t nfr) { return nfr * (6 * BLKDESC_BYTES + 16 + 6 * 90 * 4 + 6 * 7 * 512) + 256; }

static int grow_front_ws(ac3mi_ctx *ctx, const DecChoice &fe, size_t nfr)
{
    if (fe.fp) TRY(ws_grow(ctx, ctx->ws_draws, nfr * 4 + nfr * 2 + 256));
    if (fe.split) TRY(ws_grow(ctx, ctx->ws_split, split_bytes(nfr)));
    return AC3MI_OK;
}

// ac3mi_set_decode_crc 1 / 2: the CRC kernel over the nfr frames of a call (or tile), ahead of its front end; *verdict is
// the array the front end reads (null in mode 0: nothing is launched)
static int crc_pass(ac3mi_ctx *ctx, const ac3mi_decode_desc *desc, const uint8_t *frames, int frame_stride, size_t nfr,
                    const uint8_t **verdict)
{
    *verdict = nullptr;
    if (!ctx->decode_crc || !nfr) return AC3MI_OK;
    TRY(ws_grow(ctx, ctx->ws_crc, nfr));
    CrcLaunch C;
    C.frames = frames;
    C.verdict = ctx->ws_crc.at<uint8_t>();
    C.n_frames = nfr;
    C.frame_stride = frame_stride;
    C.frame_bytes = desc->frame_bytes;
    C.acmod = desc->acmod;
    C.lfeon = desc->lfeon ? 1 : 0;
    C.conceal = ctx->decode_crc == 2;
    HIPCHK(ctx, launch_crc(C, ctx->stream));
    *verdict = C.verdict;
    return AC3MI_OK;
}

// The DecodeLaunch of a call: its frames, descriptor and state, and the front end's workspaces (grow_front_ws).  Coefficient
// planes, flags, taps and a fused transform are the caller's.
static DecodeLaunch decode_launch(const ac3mi_ctx *ctx, const DecChoice &fe, const ac3mi_decode_desc *desc, const uint8_t *frames,
                                  int frame_stride, int n_streams, int frames_per_stream, uint16_t *lfsr, uint32_t *status)
{
    const size_t nfr = (size_t)n_streams * frames_per_stream;
    DecodeLaunch D;
    D.frames = frames;
    D.frame_bytes = desc->frame_bytes;
    D.frame_stride = frame_stride;
    D.n_streams = n_streams;
    D.frames_per_stream = frames_per_stream;
    D.req_flags = desc->flags;
    D.acmod = desc->acmod;
    D.lfeon = desc->lfeon ? 1 : 0;
    D.dynrng_on = desc->dynrng ? 1 : 0;
    D.level = desc->level;
    D.coef = nullptr;
    D.blksw = nullptr;
    D.status = status;
    D.lfsr = lfsr;
    D.slot = ctx->slots;
    D.tap_exp = nullptr;
    D.tap_bap = nullptr;
    D.choice = fe;
    D.log = ctx->launch_log.words ? &ctx->launch_log : nullptr;
    D.frame_draws = fe.fp ? ctx->ws_draws.at<uint32_t>() : nullptr;
    D.frame_lfsr = fe.fp ? ctx->ws_draws.at<uint16_t>(nfr * 4) : nullptr;
    if (fe.split) {
        uint8_t *p = ctx->ws_split.at<uint8_t>();
        D.ws_desc = p;
        D.ws_fpos = (uint32_t *)(p + nfr * 6 * BLKDESC_BYTES);
        D.ws_cplco = (float *)(p + nfr * (6 * BLKDESC_BYTES + 16));
        D.ws_rows = p + nfr * (6 * BLKDESC_BYTES + 16 + 6 * 90 * 4);
    }
    return D;
}

// the encoder's workspace for `rows` channel-blocks (6 x channels per frame):
// mdct | raw exponents | encoded exponents | masking curves | exp_samples | strategies | exponent bits | search results | verdict tables
struct EncWs { size_t off_eexp, off_emask, off_shift, off_strat, off_ebits, off_snr, off_memo, need; };
static EncWs enc_ws_layout(size_t rows)
{
    EncWs w;
    const size_t rows_pad = (rows + 255) & ~(size_t)255;
    w.off_eexp = rows * 256 * 4 + rows * 256;
    w.off_emask = w.off_eexp + rows * 256;
    w.off_shift = w.off_emask + ((rows * 100 + 255) & ~(size_t)255);
    w.off_strat = w.off_shift + rows_pad;
    w.off_ebits = w.off_strat + rows_pad;
    w.off_snr = w.off_ebits + rows_pad * 4;
    w.off_memo = w.off_snr + rows_pad * 2;              // [S][F][2] int32 <= rows / 3 entries
    w.need = w.off_memo + rows_pad * 6 + 1024;          // [S][F][8] uint32
    return w;
}

// the transcode's s16 PCM between the transform and the encoder (ws_tc)
static size_t s16_ws_bytes(size_t nfr, int n_out) { return nfr * 1536 * n_out * 2 + 512; }

// The packers' CRC table of a frame size (crc_lanes.h): built and uploaded when the context first meets the size, kept by
// frame_words - a later call of that size finds it and adds no host work, no copy and no synchronisation
static int crc_rows_ready(ac3mi_ctx *ctx, int frame_words, const uint16_t **rows)
{
    for (const auto &e : ctx->crc_rows)
        if (e.first == frame_words) { *rows = e.second; return AC3MI_OK; }
    uint16_t h[CRCL_LANES][CRCL_ROW];
    crcl_fill_rows(frame_words, h);
    uint16_t *d = nullptr;
    if (int rc = upload_table_once(ctx, "ac3mi_encode_batch", &h[0][0], sizeof h, &d)) return rc;
    ctx->crc_rows.emplace_back(frame_words, d);
    *rows = d;
    return AC3MI_OK;
}

// The encoder's part of a call of nfr frames (E.cfg set): grows the encoder's and the tools' workspaces, and fills E's
// workspace arrays (the taps replace theirs), the tool settings and what else comes from the context.
static int encode_setup(ac3mi_ctx *ctx, EncodeLaunch &E, const ac3mi_encode_desc *desc, size_t nfr, const ac3mi_encode_taps *taps)
{
    const EncTools &t = ctx->tools;
    const size_t rows = nfr * 6 * E.cfg.nch;
    const EncWs W = enc_ws_layout(rows);
    TRY(ws_grow(ctx, ctx->ws_enc, W.need));
    TRY(crc_rows_ready(ctx, E.cfg.frame_words, &E.crc_rows));
    if (t.block_switch) {
        TRY(ws_grow(ctx, ctx->ws_bsw, rows));
        E.ws_bsw = ctx->ws_bsw.at<uint8_t>();
    }
    if (t.rematrix) {
        TRY(ws_grow(ctx, ctx->ws_remat, 6 * nfr));
        E.ws_remat = ctx->ws_remat.at<uint8_t>();
    }
    if (t.coupling) {
        TRY(ws_grow(ctx, ctx->ws_cpl, nfr * CPL_FRAME_BYTES + 256));
        E.cpl_begf = t.cpl_begf;
        E.ws_cpl = cpl_slices(ctx->ws_cpl.p, nfr);
        if (t.rematrix && E.cfg.acmod == 2) {       // the rows before rematrixing
            TRY(ws_grow(ctx, ctx->ws_cplr, nfr * cpl_remat_frame_bytes(E.cfg.nch) + 256));
            cpl_remat_slices(E.ws_cpl, ctx->ws_cplr.p, nfr, E.cfg.nch);
        }
    }
    E.bsi = t.bsi;
    E.bsi_words = t.bsi_words;
    E.dyn_codes = t.dyn_codes;
    E.compr_words = t.compr_words;
    E.drc_profile = t.drc_profile;
    if (t.drc_profile) {                            // [nfr][6] int16 gains, then [nfr][6] codes
        TRY(ws_grow(ctx, ctx->ws_drc, 18 * nfr));
        E.drc_state = t.drc_state;
        E.ws_drc_gain = ctx->ws_drc.at<int16_t>();
        E.ws_drc_code = ctx->ws_drc.at<uint8_t>(nfr * 12);
    }
    E.ws_mdct = ctx->ws_enc.at<int32_t>();
    E.ws_expo = nullptr;                                                   // raw exponents leave the MDCT kernel only as a tap
    E.ws_eexp = ctx->ws_enc.at<uint8_t>(W.off_eexp);
    E.ws_emask = ctx->ws_enc.at<int16_t>(W.off_emask);
    E.ws_shift = ctx->ws_enc.at<int8_t>(W.off_shift);
    E.ws_strat = ctx->ws_enc.at<uint8_t>(W.off_strat);
    E.ws_ebits = ctx->ws_enc.at<int32_t>(W.off_ebits);
    E.ws_snr = ctx->ws_enc.at<int32_t>(W.off_snr);
    E.ws_memo = ctx->ws_enc.at<uint32_t>(W.off_memo);
    if (taps && taps->d_mdct) { E.ws_mdct = taps->d_mdct; E.mdct_full_rows = true; }
    if (taps && taps->d_exponent) E.ws_expo = taps->d_exponent;
    if (taps && taps->d_exp_samples) E.ws_shift = taps->d_exp_samples;
    if (taps && taps->d_encoded_exp) E.ws_eexp = taps->d_encoded_exp;      // the exponent stage writes the tap directly
    E.tap_eexp = taps ? taps->d_encoded_exp : nullptr;
    E.tap_bap = taps ? taps->d_bap : nullptr;
    E.tap_strat = taps ? taps->d_exp_strategy : nullptr;
    E.tap_snr = taps ? taps->d_snroffst : nullptr;
    E.chbwcod = call_chbwcod(ctx, desc, E.cfg.nfbw);
    E.bw = t.bw_mode != 0;
    E.exp_strategy = t.exp_strategy;
    E.pack_mode = ctx->encode_mode;
    E.tap_curve = ctx->debug_search_curve;
    E.fixed_shape = ctx->fixed_shape != 0 && !ctx->debug_search_curve;    // (the tap is the generic search kernel's)
    E.slot = ctx->slots;
    E.log = ctx->launch_log.words ? &ctx->launch_log : nullptr;
    return AC3MI_OK;
}

size_t ac3mi_transcode_workspace_plan(size_t frames, int frames_per_stream, int n_in, int nfchans, int n_out)
{
    // what ac3mi_transcode_batch grows for a call (or tile) of `frames` frames in the default decode mode, with the
    // per-frame level flags and the split front end: the call's own expressions (n_in == n_out stands for identity routing)
    const bool mantx = dec_mantx(0, frames_per_stream, n_in == n_out, true);
    return (mantx ? 0 : coef_bytes(frames, n_in)) + (zs_off(frames, nfchans) + frames) + split_bytes(frames) +
           s16_ws_bytes(frames, n_out) + enc_ws_layout(frames * 6 * (size_t)n_out).need;
}

int ac3mi_xform_planes(const ac3mi_xform_desc *desc, int *n_in, int *n_out)
{
    MixPlan plan;
    if (!desc) return AC3MI_ERR_ARG;
    int r = build_mix_plan(desc->acmod, desc->lfeon, desc->output, &plan);
    if (r != AC3MI_OK) return r;
    if (n_in) *n_in = plan.n_in;
    if (n_out) *n_out = plan.n_out;
    return AC3MI_OK;
}

int ac3mi_imdct_batch(ac3mi_ctx *ctx, const ac3mi_xform_desc *desc, const float *d_coeffs,
                      const uint8_t *d_blksw, float *d_delay, float *d_pcm, int n_streams,
                      int frames_per_stream)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!desc || !d_coeffs || !d_delay || !d_pcm || n_streams < 0 || frames_per_stream < 0) {
        ctx->err = "ac3mi_imdct_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    XformLaunch L;
    int r = build_mix_plan(desc->acmod, desc->lfeon, desc->output, &L.plan);
    if (r != AC3MI_OK) {
        ctx->err = "ac3mi_imdct_batch: output configuration not reachable from acmod (a52_downmix_init)";
        return r;
    }
    if ((long long)n_streams * L.plan.n_out > 0x7fffffffLL) {
        ctx->err = "ac3mi_imdct_batch: too many chains for one launch";
        return AC3MI_ERR_ARG;
    }
    L.coef = d_coeffs;
    L.blksw = d_blksw;
    L.delay = d_delay;
    L.slot = ctx->slots;
    L.delay_stride = 6 * 128;
    L.pcm = d_pcm;
    L.n_streams = n_streams;
    L.frames = frames_per_stream;
    L.bias = desc->bias;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_xform(ctx->tab, L, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_syncinfo(const uint8_t *buf, int *flags, int *sample_rate, int *bit_rate)
{
    // a52_syncinfo's order (parse.c:86-129), outputs included: it writes *flags once the sync word and bsid pass, *bit_rate
    // once frmsizecod passes as well, *sample_rate with the size.  The partial tests are the one rule's on a byte 4 of 0
    // (which passes byte 4's part) and on frmsizecod alone (fscod 0)
    if (!buf || !ac3mi::sync_header_ok((uint32_t)buf[0] << 8 | buf[1], 0, buf[5])) return 0;
    const int half = ac3mi::sync_halfrate(buf[5] >> 3), acmod = buf[6] >> 5;
    const int lfebit = 0x80 >> ac3mi::sync_lfeon_pos(acmod);            // (always in byte 6)
    if (flags) *flags = (((buf[6] & 0xf8) == 0x50) ? AC3MI_DOLBY : acmod) | ((buf[6] & lfebit) ? AC3MI_LFE : 0);
    if (!ac3mi::sync_frame_bytes(buf[4] & 63)) return 0;
    if (bit_rate) *bit_rate = (int)(ac3mi::sync_kbps((buf[4] & 63) >> 1) * 1000) >> half;
    const int size = (int)ac3mi::sync_frame_bytes(buf[4]);
    if (size && sample_rate) *sample_rate = kSampleRates[buf[4] >> 6] >> half;
    return size;
}

int ac3mi_crc_check_batch(ac3mi_ctx *ctx, const uint8_t *d_frames, int frame_stride, int frame_bytes, size_t n_frames,
                          uint8_t *d_verdict)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!d_frames || !d_verdict || n_frames > 0x7fffffffu || frame_bytes < 8 || frame_bytes > 3840 ||
        frame_stride < ((frame_bytes + 3) & ~3) || (frame_stride & 3) || ((uintptr_t)d_frames & 3)) {
        ctx->err = "ac3mi_crc_check_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CrcLaunch C;
    C.frames = d_frames;
    C.verdict = d_verdict;
    C.n_frames = n_frames;
    C.frame_stride = frame_stride;
    C.frame_bytes = frame_bytes;
    HIPCHK(ctx, launch_crc(C, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_bsi_read(const uint8_t *buf, int len, ac3mi_bsi_info *out)
{
    if (!buf || !out || len < 0) return AC3MI_ERR_ARG;
    bsi_read_host(buf, len, out);
    return AC3MI_OK;
}

int ac3mi_bsi_read_batch(ac3mi_ctx *ctx, const uint8_t *d_frames, int frame_stride, int frame_bytes, size_t n_frames,
                         ac3mi_bsi_info *d_info)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!d_frames || !d_info || n_frames > 0x7fffffffu || frame_bytes < 8 || frame_bytes > 3840 ||
        frame_stride < ((frame_bytes + 3) & ~3) || (frame_stride & 3) || ((uintptr_t)d_frames & 3) || ((uintptr_t)d_info & 3)) {
        ctx->err = "ac3mi_bsi_read_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    BsiLaunch B;
    B.frames = d_frames;
    B.n_frames = n_frames;
    B.frame_stride = frame_stride;
    B.frame_bytes = frame_bytes;
    B.info = d_info;
    HIPCHK(ctx, launch_bsi(B, ctx->stream));
    return AC3MI_OK;
}

// (ac3mi_frame_scan, the host twin, lives in scan.hip beside the rule it shares with the kernel)
int ac3mi_frame_scan_batch(ac3mi_ctx *ctx, const uint8_t *d_bytes, size_t stream_stride, const uint32_t *d_len, int n_streams,
                           int mode, int max_frames, ac3mi_frame_ref *d_refs, ac3mi_scan_info *d_info)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!d_bytes || !d_len || !d_refs || !d_info || n_streams < 0 || (mode != 0 && mode != 1) || max_frames < 1 ||
        (uint64_t)stream_stride > 0xffffffffull || (stream_stride & 15) || ((uintptr_t)d_bytes & 15) || ((uintptr_t)d_len & 3) ||
        ((uintptr_t)d_refs & 3) || ((uintptr_t)d_info & 3)) {
        ctx->err = "ac3mi_frame_scan_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ScanLaunch S;
    S.bytes = d_bytes;
    S.stride = stream_stride;
    S.len = d_len;
    S.n_streams = (size_t)n_streams;
    S.mode = mode;
    S.max_frames = max_frames;
    S.refs = d_refs;
    S.info = d_info;
    HIPCHK(ctx, launch_frame_scan(S, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_frame_gather_batch(ac3mi_ctx *ctx, const uint8_t *d_bytes, size_t stream_stride, int n_streams,
                             const ac3mi_frame_ref *d_refs, const ac3mi_scan_info *d_info, int max_frames, int first_frame,
                             int frames_per_stream, uint8_t *d_frames, int frame_stride, int frame_bytes)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!d_bytes || !d_refs || !d_info || !d_frames || n_streams < 0 || max_frames < 1 || first_frame < 0 || frames_per_stream < 1 ||
        (uint64_t)n_streams * (uint64_t)frames_per_stream > 0x7fffffffu || (uint64_t)stream_stride > 0xffffffffull || (stream_stride & 3) ||
        ((uintptr_t)d_bytes & 3) || ((uintptr_t)d_refs & 3) || ((uintptr_t)d_info & 3) || frame_bytes < 8 || frame_bytes > 3840 ||
        frame_stride < ((frame_bytes + 3) & ~3) || (frame_stride & 3) || ((uintptr_t)d_frames & 3)) {
        ctx->err = "ac3mi_frame_gather_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    GatherLaunch G;
    G.bytes = d_bytes;
    G.stride = stream_stride;
    G.n_streams = (size_t)n_streams;
    G.refs = d_refs;
    G.info = d_info;
    G.max_frames = max_frames;
    G.first_frame = first_frame;
    G.frames_per_stream = frames_per_stream;
    G.frames = d_frames;
    G.frame_stride = frame_stride;
    G.frame_bytes = frame_bytes;
    HIPCHK(ctx, launch_frame_gather(G, ctx->stream));
    return AC3MI_OK;
}

// (ac3mi_loudness_state_bytes, _roles, _tables and _read, the host side, live in loudness.hip beside the rule)
static int loud_tab_ready(ac3mi_ctx *ctx, const char *who)
{
    if (ctx->loud_tab) return AC3MI_OK;
    double h[LOUD_TAB_DOUBLES];
    loud_fill_tab(h);
    return upload_table_once(ctx, who, h, sizeof h, &ctx->loud_tab);
}

// the plain meter (d_range_state nullptr, with_range false) and the one that meters the range beside it
static int loudness_batch(ac3mi_ctx *ctx, const char *who, const ac3mi_loudness_desc *desc, const int16_t *d_pcm, int n_streams,
                          int frames_per_stream, void *d_state, void *d_range_state, bool with_range)
{
    if (!ctx) return AC3MI_ERR_ARG;
    LoudnessLaunch L;
    L.pcm = d_pcm;
    L.sample_rate = desc ? desc->sample_rate : 0;
    L.channels = desc ? desc->channels : 0;
    pcm_copy_roles(L.role, desc ? desc->role : nullptr, L.channels);
    L.n_streams = n_streams;
    L.frames_per_stream = frames_per_stream;
    L.state = d_state;
    L.tab = nullptr;
    L.range_state = with_range ? d_range_state : nullptr;
    if ((with_range && !d_range_state) || !loudness_args_ok(L)) {
        ctx->err = std::string(who) + ": bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = loud_tab_ready(ctx, who)) return rc;
    L.tab = ctx->loud_tab;
    HIPCHK(ctx, launch_loudness(L, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_loudness_batch(ac3mi_ctx *ctx, const ac3mi_loudness_desc *desc, const int16_t *d_pcm, int n_streams,
                         int frames_per_stream, void *d_state)
{
    return loudness_batch(ctx, "ac3mi_loudness_batch", desc, d_pcm, n_streams, frames_per_stream, d_state, nullptr, false);
}

int ac3mi_loudness_range_batch(ac3mi_ctx *ctx, const ac3mi_loudness_desc *desc, const int16_t *d_pcm, int n_streams,
                               int frames_per_stream, void *d_state, void *d_range_state)
{
    return loudness_batch(ctx, "ac3mi_loudness_range_batch", desc, d_pcm, n_streams, frames_per_stream, d_state, d_range_state, true);
}

int ac3mi_loudness_range_read_batch(ac3mi_ctx *ctx, const void *d_range_state, int n_streams, ac3mi_loudness_range_result *d_results)
{
    return read_batch(ctx, "ac3mi_loudness_range_read_batch", d_range_state, n_streams, d_results, [&]() -> int {
        if (int rc = loud_tab_ready(ctx, "ac3mi_loudness_range_read_batch")) return rc;
        HIPCHK(ctx, launch_loudness_range_read(d_range_state, n_streams, ctx->loud_tab, d_results, ctx->stream));
        return AC3MI_OK;
    });
}

int ac3mi_loudness_read_batch(ac3mi_ctx *ctx, const void *d_state, int n_streams, ac3mi_loudness_result *d_results)
{
    return read_batch(ctx, "ac3mi_loudness_read_batch", d_state, n_streams, d_results, [&]() -> int {
        if (int rc = loud_tab_ready(ctx, "ac3mi_loudness_read_batch")) return rc;
        HIPCHK(ctx, launch_loudness_read(d_state, n_streams, ctx->loud_tab, d_results, ctx->stream));
        return AC3MI_OK;
    });
}

int ac3mi_loudness_words_batch(ac3mi_ctx *ctx, const ac3mi_loudness_result *d_results, int n_streams, int frames_per_stream,
                               uint32_t base_word, uint32_t *d_words)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!d_results || !d_words || n_streams < 0 || frames_per_stream < 1 || (uint64_t)n_streams * (uint64_t)frames_per_stream > 0x7fffffffu ||
        ((uintptr_t)d_results & 7) || ((uintptr_t)d_words & 3)) {
        ctx->err = "ac3mi_loudness_words_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_loudness_words(d_results, n_streams, frames_per_stream, base_word, d_words, ctx->stream));
    return AC3MI_OK;
}

// (ac3mi_truepeak_state_bytes, _tables, _ceiling, _read and _host, the host side, live in truepeak.hip beside the rule)
int ac3mi_truepeak_batch(ac3mi_ctx *ctx, int channels, const uint8_t *role, const int16_t *d_pcm, int n_streams,
                         int frames_per_stream, void *d_state)
{
    if (!ctx) return AC3MI_ERR_ARG;
    TruePeakLaunch L;
    L.pcm = d_pcm;
    L.channels = channels;
    pcm_copy_roles(L.role, role, channels);
    L.n_streams = n_streams;
    L.frames_per_stream = frames_per_stream;
    L.state = d_state;
    if (!role || !truepeak_args_ok(L)) {
        ctx->err = "ac3mi_truepeak_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_truepeak(L, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_truepeak_read_batch(ac3mi_ctx *ctx, const void *d_state, int n_streams, uint32_t ceiling_q28, ac3mi_truepeak_result *d_results)
{
    return read_batch(ctx, "ac3mi_truepeak_read_batch", d_state, n_streams, d_results, [&]() -> int {
        HIPCHK(ctx, launch_truepeak_read(d_state, n_streams, ceiling_q28, d_results, ctx->stream));
        return AC3MI_OK;
    });
}

// (ac3mi_limit_state_bytes, _release_step, _read and _host, the host side, live in limit.hip beside the rule)
int ac3mi_limit_batch(ac3mi_ctx *ctx, int channels, const uint8_t *role, uint32_t ceiling_q28, uint32_t release_step_q24,
                      const int16_t *d_pcm, int16_t *d_out, int n_streams, int frames_per_stream, void *d_state)
{
    if (!ctx) return AC3MI_ERR_ARG;
    LimitLaunch L;
    L.pcm = d_pcm;
    L.out = d_out;
    L.channels = channels;
    pcm_copy_roles(L.role, role, channels);
    L.ceiling_q28 = ceiling_q28;
    L.release_step_q24 = release_step_q24;
    L.n_streams = n_streams;
    L.frames_per_stream = frames_per_stream;
    L.state = d_state;
    if (!role || !limit_args_ok(L)) {
        ctx->err = "ac3mi_limit_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_limit(L, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_limit_read_batch(ac3mi_ctx *ctx, const void *d_state, int n_streams, ac3mi_limit_result *d_results)
{
    return read_batch(ctx, "ac3mi_limit_read_batch", d_state, n_streams, d_results, [&]() -> int {
        HIPCHK(ctx, launch_limit_read(d_state, n_streams, d_results, ctx->stream));
        return AC3MI_OK;
    });
}

// (ac3mi_resample_ratio, _tables, _state_bytes, _plan and _host, the host side, live in resample.hip beside the rule)
static int resample_tab_ready(ac3mi_ctx *ctx, int in_rate, int out_rate, const uint32_t **tab)
{
    uint32_t **slot = &ctx->resample_tab[rs_pair(in_rate, out_rate)];
    if (!*slot) {
        std::vector<uint32_t> h(resample_packed_table(in_rate, out_rate, nullptr));
        if (resample_packed_table(in_rate, out_rate, h.data()) == 0) {
            ctx->err = "ac3mi_resample_batch: the pair's table does not pass its bound check";
            return AC3MI_ERR_UNSUPPORTED;
        }
        if (int rc = upload_table_once(ctx, "ac3mi_resample_batch", h.data(), h.size() * 4, slot)) return rc;
    }
    *tab = *slot;
    return AC3MI_OK;
}

int ac3mi_resample_batch(ac3mi_ctx *ctx, const ac3mi_resample_desc *desc, const int16_t *d_pcm, int n_streams, int in_frames,
                         int16_t *d_out, int out_frames, void *d_state, uint32_t *d_status)
{
    if (!ctx) return AC3MI_ERR_ARG;
    ResampleLaunch L;
    L.in_rate = desc ? desc->in_rate : 0;
    L.out_rate = desc ? desc->out_rate : 0;
    L.channels = desc ? desc->channels : 0;
    L.pcm = d_pcm;
    L.out = d_out;
    L.n_streams = n_streams;
    L.in_frames = in_frames;
    L.out_frames = out_frames;
    L.state = d_state;
    L.status = d_status;
    L.tab = nullptr;
    if (!resample_args_ok(L)) {
        ctx->err = "ac3mi_resample_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    if (n_streams == 0) return AC3MI_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = resample_tab_ready(ctx, L.in_rate, L.out_rate, &L.tab)) return rc;
    HIPCHK(ctx, launch_resample(L, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_decode_planes(const ac3mi_decode_desc *desc, int *n_out, int *out_flags)
{
    if (!desc || desc->acmod < 0 || desc->acmod > 7) return AC3MI_ERR_ARG;
    const int out = a52_granted_output(desc->flags & AC3MI_CHANNEL_MASK, desc->acmod);
    if (out < 0) return AC3MI_ERR_ARG;
    const int lfe = (desc->lfeon && (desc->flags & AC3MI_LFE)) ? AC3MI_LFE : 0;
    if (n_out) *n_out = sync_nfchans(out) + (lfe ? 1 : 0);
    if (out_flags) *out_flags = out | lfe;
    return AC3MI_OK;
}

// d_pcm (float planes) or d_pcm16 (interleaved s16, written by the transform itself)
static int decode_impl(ac3mi_ctx *ctx, const ac3mi_decode_desc *desc, const uint8_t *d_frames,
                       int frame_stride, int n_streams, int frames_per_stream, float *d_delay,
                       uint16_t *d_lfsr, float *d_pcm, int16_t *d_pcm16, uint32_t *d_status, const ac3mi_decode_taps *taps)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!desc || !d_frames || !d_delay || !d_lfsr || (!d_pcm && !d_pcm16) || !d_status || n_streams < 0 ||
        frames_per_stream < 0 || desc->frame_bytes < 8 || desc->frame_bytes > 3840 ||
        frame_stride < ((desc->frame_bytes + 3) & ~3) || (frame_stride & 3) || ((uintptr_t)d_frames & 3)) {
        ctx->err = "ac3mi_decode_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    int n_out = 0, out_flags = 0;
    if (ac3mi_decode_planes(desc, &n_out, &out_flags) != AC3MI_OK) {
        ctx->err = "ac3mi_decode_batch: requested output not supported (a52_frame would return 1)";
        return AC3MI_ERR_ARG;
    }
    XformLaunch X;
    if (build_mix_plan(desc->acmod, desc->lfeon, out_flags, &X.plan) != AC3MI_OK) {
        ctx->err = "ac3mi_decode_batch: no mix plan for this acmod/output";
        return AC3MI_ERR_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the front end (launch_rule.h); the one-workgroup-per-stream kernel may also write planes for the transform kernel
    const DecChoice fe = dec_choice(ctx->decode_mode, n_streams, frames_per_stream, d_pcm16 != nullptr, taps != nullptr, true, mix_plan_identity(X.plan),
                                    ctx->mix_pending && X.plan.surr_mask, ctx->fixed_shape != 0, desc->acmod, desc->lfeon ? 1 : 0, false);
    if (const int g = (taps || fe.fused) ? 0 : tile_streams(ctx, n_streams, frames_per_stream)) {
        // bounded workspace: whole streams at a time (streams are independent; state arrays move with them)
        TileState tile(ctx, n_out, false, frames_per_stream);
        int rc = AC3MI_OK;
        for (int s0 = 0; s0 < n_streams && rc == AC3MI_OK; s0 += g) {
            const int ns = n_streams - s0 < g ? n_streams - s0 : g;
            const size_t f0 = (size_t)s0 * frames_per_stream;
            tile.at(s0);
            rc = decode_impl(ctx, desc, d_frames + f0 * frame_stride, frame_stride, ns, frames_per_stream,
                             tile.slots ? d_delay : d_delay + (size_t)s0 * n_out * 128, tile.slots ? d_lfsr : d_lfsr + s0,
                             d_pcm ? d_pcm + f0 * 6 * n_out * 256 : nullptr, d_pcm16 ? d_pcm16 + f0 * 6 * n_out * 256 : nullptr,
                             d_status + f0, nullptr);
        }
        return rc;
    }
    const size_t nfr = (size_t)n_streams * frames_per_stream;
    float *coef = taps && taps->d_coef ? taps->d_coef : nullptr;
    uint8_t *blksw = taps && taps->d_blksw ? taps->d_blksw : nullptr;
    uint8_t *zs = nullptr;
    if (!fe.fused) {
        const size_t zs_at = blksw ? 0 : zs_off(nfr, X.plan.nfchans);
        TRY(ws_grow(ctx, ctx->ws_coef, (coef || fe.mantx) ? 0 : coef_bytes(nfr, X.plan.n_in)));
        TRY(ws_grow(ctx, ctx->ws_blksw, zs_at + (fe.mixstate ? nfr : 0)));
        if (fe.mixstate) zs = ctx->ws_blksw.at<uint8_t>(zs_at);
        if (!coef) coef = ctx->ws_coef.at<float>();
        if (!blksw) blksw = ctx->ws_blksw.at<uint8_t>();
    }
    TRY(grow_front_ws(ctx, fe, nfr));
    DecodeLaunch D = decode_launch(ctx, fe, desc, d_frames, frame_stride, n_streams, frames_per_stream, d_lfsr, d_status);
    TRY(crc_pass(ctx, desc, d_frames, frame_stride, nfr, &D.crc));
    D.coef = fe.mantx ? nullptr : coef;
    D.blksw = blksw;
    D.zs = zs;
    D.tap_exp = taps ? taps->d_exp : nullptr;
    D.tap_bap = taps ? taps->d_bap : nullptr;
    D.dyn_out = taps ? taps->d_dynrng_out : nullptr;
    D.dyn_in = taps ? taps->d_dynrng_in : nullptr;
    X.coef = D.coef;
    X.blksw = blksw;
    X.zs = zs;
    X.mix_pending = fe.mixstate ? ctx->mix_pending : nullptr;
    X.mix_flags = fe.mixstate ? ctx->mix_flags : nullptr;
    X.delay = d_delay;
    X.slot = ctx->slots;
    X.delay_stride = 6 * 128;
    X.pcm = d_pcm;
    X.pcm16 = d_pcm16;
    X.s16_flags = out_flags;
    X.n_streams = n_streams;
    X.frames = frames_per_stream;
    X.bias = desc->bias;
    // One workgroup per stream, one wavefront per channel, the transform fused in when every
    // coded plane is an output plane (decode_wg.hip) - no coefficient planes in HBM.  Stage taps and mixing outputs
    // take the same front end with the planes written out, then the transform kernel.
    if (fe.wg) {
        HIPCHK(ctx, launch_decode_wg(ctx->tab, D, fe.fused ? &X : nullptr, 0, ctx->stream));
        if (!fe.fused) HIPCHK(ctx, launch_xform(ctx->tab, X, ctx->stream));
        return AC3MI_OK;
    }
    // One pass over the batch, kernels back to back on the context's stream.  Rounds 1-2 sent large batches through in two
    // chunks with the transform of chunk k on a second stream beside the front end of chunk k+1 (and round 3 tried the
    // mantissa kernel on a third): measured again with the split front end, 1 / 2 / 3 / 4 chunks = 3.545 / 3.549 / 3.572 /
    // 3.616 ms per 65 536 frames - a kernel of this size fills the chip, only the tails overlap - so the pipeline is gone.
    // (Also tried in round 3: the batch in 2 / 4 / 8 / 16 tiles, front end + transform per tile, so that a tile's coefficient
    // planes would still sit in the 256 MiB Infinity Cache when the transform reads them: 3.49 / 3.63 / 3.89 / 4.47 ms against
    // 3.48 ms in one piece - each kernel's tail costs more than the cache gives.)
    if (fe.mantx) D.fuse = &X;                              // the mantissa kernel transforms too (decode_mx.hip)
    HIPCHK(ctx, launch_decode(ctx->tab, D, ctx->stream));
    if (!fe.mantx) HIPCHK(ctx, launch_xform(ctx->tab, X, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_decode_batch(ac3mi_ctx *ctx, const ac3mi_decode_desc *desc, const uint8_t *d_frames,
                       int frame_stride, int n_streams, int frames_per_stream, float *d_delay,
                       uint16_t *d_lfsr, float *d_pcm, uint32_t *d_status, const ac3mi_decode_taps *taps)
{
    if (ctx && !d_pcm) {
        ctx->err = "ac3mi_decode_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    return decode_impl(ctx, desc, d_frames, frame_stride, n_streams, frames_per_stream, d_delay, d_lfsr, d_pcm, nullptr, d_status, taps);
}

int ac3mi_decode_s16_batch(ac3mi_ctx *ctx, const ac3mi_decode_desc *desc, const uint8_t *d_frames,
                           int frame_stride, int n_streams, int frames_per_stream, float *d_delay,
                           uint16_t *d_lfsr, int16_t *d_pcm16, uint32_t *d_status)
{
    if (!ctx) return AC3MI_ERR_ARG;
    if (!desc || !d_pcm16 || ((uintptr_t)d_pcm16 & 15)) {
        ctx->err = "ac3mi_decode_s16_batch: bad argument (d_pcm16 must be 16-byte aligned)";
        return AC3MI_ERR_ARG;
    }
    ac3mi_decode_desc dd = *desc;
    dd.level = 1.0f;                                    // what the reference's converters presuppose (src/AC3ACM.cpp:1553)
    dd.bias = 384.0f;
    return decode_impl(ctx, &dd, d_frames, frame_stride, n_streams, frames_per_stream, d_delay, d_lfsr, nullptr, d_pcm16, d_status, nullptr);
}

int ac3mi_encode_frame_bytes(const ac3mi_encode_desc *desc)
{
    EncConfig c;
    if (!desc) return 0;
    return enc_config(desc->sample_rate, desc->bit_rate, desc->channels, &c);
}

int ac3mi_encode_tables(int16_t *costab64, int16_t *sintab64, int16_t *xcos128, int16_t *xsin128, int16_t *window256)
{
    EncTables et;
    build_enc_tables(&et);
    if (costab64) memcpy(costab64, et.cos, sizeof et.cos);
    if (sintab64) memcpy(sintab64, et.sin, sizeof et.sin);
    if (xcos128) memcpy(xcos128, et.xcos, sizeof et.xcos);
    if (xsin128) memcpy(xsin128, et.xsin, sizeof et.xsin);
    if (window256) memcpy(window256, et.win, sizeof et.win);
    return AC3MI_OK;
}

int ac3mi_encode_spec_tables(int16_t *window256, uint8_t *latab256, uint16_t *hth50x3, uint8_t *baptab64, uint8_t *bndsz50,
                             uint16_t *sdecay4, uint16_t *fdecay4, uint16_t *sgain4, uint16_t *dbknee4, uint16_t *floor8,
                             uint16_t *fgain8, uint16_t *freqs3, uint16_t *bitrate19)
{
    EncTables et;
    build_enc_tables(&et);
    if (window256) memcpy(window256, et.win, sizeof et.win);
    if (latab256) memcpy(latab256, et.latab, sizeof et.latab);
    if (hth50x3) memcpy(hth50x3, et.hth, sizeof et.hth);
    if (baptab64) memcpy(baptab64, et.baptab, sizeof et.baptab);
    if (bndsz50) memcpy(bndsz50, et.band_size, sizeof et.band_size);
    for (int i = 0; i < 4; i++) {
        if (sdecay4) sdecay4[i] = (uint16_t)enc_sdecay(i);
        if (fdecay4) fdecay4[i] = (uint16_t)enc_fdecay(i);
        if (sgain4) sgain4[i] = (uint16_t)enc_sgain(i);
        if (dbknee4) dbknee4[i] = (uint16_t)enc_dbknee(i);
    }
    for (int i = 0; i < 8; i++) {
        if (floor8) floor8[i] = (uint16_t)enc_floor(i);
        if (fgain8) fgain8[i] = (uint16_t)enc_fgain(i);
    }
    for (int i = 0; i < 3; i++) if (freqs3) freqs3[i] = (uint16_t)kSampleRates[i];
    for (int i = 0; i < 19; i++) if (bitrate19) bitrate19[i] = (uint16_t)sync_kbps(i);
    return AC3MI_OK;
}

int ac3mi_encode_batch(ac3mi_ctx *ctx, const ac3mi_encode_desc *desc, const int16_t *d_pcm, const uint8_t *chmap,
                       int16_t *d_last, int32_t *d_csnroffst, uint8_t *d_frames, int frame_stride, int n_streams,
                       int frames_per_stream, const ac3mi_encode_taps *taps)
{
    if (!ctx) return AC3MI_ERR_ARG;
    EncodeLaunch E;
    if (!desc || !d_pcm || !chmap || !d_last || !d_csnroffst || !d_frames || n_streams < 0 || frames_per_stream < 0) {
        ctx->err = "ac3mi_encode_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    const int fb = enc_config(desc->sample_rate, desc->bit_rate, desc->channels, &E.cfg, call_acmod(ctx), ctx->tools.layout_lfeon);
    if (fb <= 0) {
        ctx->err = ctx->tools.layout_mode == 1 && ac3mi_encode_frame_bytes(desc) > 0
                       ? "ac3mi_encode_batch: channels is not nfchans(acmod) + lfeon of the layout set by ac3mi_set_encode_layout"
                       : "ac3mi_encode_batch: AC3_encode_init would return 0 for this rate/bitrate/channels";
        return AC3MI_ERR_ARG;
    }
    if (frame_stride < ((fb + 3) & ~3) || (frame_stride & 3) || ((uintptr_t)d_frames & 3) || ((uintptr_t)d_pcm & 1)) {
        ctx->err = "ac3mi_encode_batch: frame_stride must be a multiple of 4 and >= the frame size";
        return AC3MI_ERR_ARG;
    }
    for (int i = 0; i < 8; i++) E.chmap[i] = i < desc->channels ? chmap[i] : 0;
    for (int i = 0; i < desc->channels; i++)
        if (E.chmap[i] >= desc->channels) {
            ctx->err = "ac3mi_encode_batch: chmap entry out of range";
            return AC3MI_ERR_ARG;
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int g = taps ? 0 : tile_streams(ctx, n_streams, frames_per_stream)) {
        TileState tile(ctx, 0, true, frames_per_stream);
        int rc = AC3MI_OK;
        for (int s0 = 0; s0 < n_streams && rc == AC3MI_OK; s0 += g) {
            const int ns = n_streams - s0 < g ? n_streams - s0 : g;
            const size_t f0 = (size_t)s0 * frames_per_stream;
            tile.at(s0);
            rc = ac3mi_encode_batch(ctx, desc, d_pcm + f0 * 1536 * E.cfg.nch, chmap,
                                    tile.slots ? d_last : d_last + (size_t)s0 * E.cfg.nch * 256, tile.slots ? d_csnroffst : d_csnroffst + s0,
                                    d_frames + f0 * frame_stride, frame_stride, ns, frames_per_stream, nullptr);
        }
        return rc;
    }
    TRY(encode_setup(ctx, E, desc, (size_t)n_streams * frames_per_stream, taps));
    E.pcm = d_pcm;
    E.last = d_last;
    E.csnr = d_csnroffst;
    E.frames = d_frames;
    E.frame_stride = frame_stride;
    E.n_streams = n_streams;
    E.frames_per_stream = frames_per_stream;
    if ((E.tap_bap == nullptr) != (E.tap_eexp == nullptr)) {
        ctx->err = "ac3mi_encode_batch: d_bap and d_encoded_exp taps must be given together";
        return AC3MI_ERR_ARG;
    }
    HIPCHK(ctx, launch_encode(ctx->tab, E, ctx->stream));
    return AC3MI_OK;
}

int ac3mi_transcode_batch(ac3mi_ctx *ctx, const ac3mi_decode_desc *dec, const ac3mi_encode_desc *enc,
                          const uint8_t *d_frames_in, int in_stride, int n_streams, int frames_per_stream,
                          float *d_delay, uint16_t *d_lfsr, const uint8_t *chmap, int16_t *d_last,
                          int32_t *d_csnroffst, uint8_t *d_frames_out, int out_stride, uint32_t *d_status)
{
    if (!ctx) return AC3MI_ERR_ARG;
    const EncTools &t = ctx->tools;
    if (!dec || !enc || !d_frames_in || !d_delay || !d_lfsr || (!chmap && t.layout_mode != 2) || !d_last || !d_csnroffst || !d_frames_out || !d_status ||
        n_streams < 0 || frames_per_stream < 0 || dec->frame_bytes < 8 || dec->frame_bytes > 3840 ||
        in_stride < ((dec->frame_bytes + 3) & ~3) || (in_stride & 3) || ((uintptr_t)d_frames_in & 3)) {
        ctx->err = "ac3mi_transcode_batch: bad argument";
        return AC3MI_ERR_ARG;
    }
    if (t.drc_source == 1 && (dec->dynrng || t.drc_profile)) {
        ctx->err = dec->dynrng ? "ac3mi_transcode_batch: ac3mi_set_encode_drc_source 1 carries the source's dynrng words - a decode with dynrng != 0 "
                                 "would apply the gains twice"
                               : "ac3mi_transcode_batch: ac3mi_set_encode_drc_source 1 with a profile of ac3mi_set_encode_drc set";
        return AC3MI_ERR_ARG;
    }
    ac3mi_decode_desc dd = *dec;
    dd.level = 1.0f;                                    // the s16 converter reads the 16-bit value out of the float (bias 384)
    dd.bias = 384.0f;
    int n_out = 0, out_flags = 0;
    XformLaunch X;
    if (ac3mi_decode_planes(&dd, &n_out, &out_flags) != AC3MI_OK || build_mix_plan(dd.acmod, dd.lfeon, out_flags, &X.plan) != AC3MI_OK) {
        ctx->err = "ac3mi_transcode_batch: requested output not supported (a52_frame would return 1)";
        return AC3MI_ERR_ARG;
    }
    EncodeLaunch E;
    // ac3mi_set_encode_layout: 0 the reference's table, 1 the set layout, 2 the layout the decoder granted
    const int lay_acmod = t.layout_mode == 2 ? granted_acmod(out_flags) : call_acmod(ctx);
    const int lay_lfeon = t.layout_mode == 2 ? ((out_flags & AC3MI_LFE) ? 1 : 0) : t.layout_lfeon;
    const int fb = enc_config(enc->sample_rate, enc->bit_rate, enc->channels, &E.cfg, lay_acmod, lay_lfeon);
    if (fb <= 0 || enc->channels != n_out) {
        ctx->err = "ac3mi_transcode_batch: encoder configuration rejected (channels not those of the layout set by "
                   "ac3mi_set_encode_layout), or its channel count differs from the decoder's output";
        return AC3MI_ERR_ARG;
    }
    if (out_stride < ((fb + 3) & ~3) || (out_stride & 3) || ((uintptr_t)d_frames_out & 3)) {
        ctx->err = "ac3mi_transcode_batch: out_stride must be a multiple of 4 and >= the frame size";
        return AC3MI_ERR_ARG;
    }
    uint8_t follow[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t.layout_mode == 2) {
        // the map that inverts the s16 converter's WAVE interleave: coded full-bandwidth channel k is decoded plane lfe + k,
        // the LFE (coded last) plane 0; the converter puts plane map[w] into WAVE slot w
        int map[6];
        if (s16_channel_map(out_flags, map) != n_out) { ctx->err = "ac3mi_transcode_batch: no channel map for the granted output"; return AC3MI_ERR_ARG; }
        for (int k = 0; k < n_out; k++) {
            const int plane = k < E.cfg.nfbw ? E.cfg.lfe + k : 0;
            for (int w = 0; w < n_out; w++)
                if (map[w] == plane) follow[k] = (uint8_t)w;
        }
        chmap = follow;                                 // (each tile below builds it again)
    }
    for (int i = 0; i < 8; i++) E.chmap[i] = i < enc->channels ? chmap[i] : 0;
    for (int i = 0; i < enc->channels; i++)
        if (E.chmap[i] >= enc->channels) { ctx->err = "ac3mi_transcode_batch: chmap entry out of range"; return AC3MI_ERR_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (const int g = tile_streams(ctx, n_streams, frames_per_stream)) {
        TileState tile(ctx, n_out, true, frames_per_stream);
        int rc = AC3MI_OK;
        for (int s0 = 0; s0 < n_streams && rc == AC3MI_OK; s0 += g) {
            const int ns = n_streams - s0 < g ? n_streams - s0 : g;
            const size_t f0 = (size_t)s0 * frames_per_stream;
            tile.at(s0);
            rc = ac3mi_transcode_batch(ctx, dec, enc, d_frames_in + f0 * in_stride, in_stride, ns, frames_per_stream,
                                       tile.slots ? d_delay : d_delay + (size_t)s0 * n_out * 128, tile.slots ? d_lfsr : d_lfsr + s0, chmap,
                                       tile.slots ? d_last : d_last + (size_t)s0 * E.cfg.nch * 256, tile.slots ? d_csnroffst : d_csnroffst + s0,
                                       d_frames_out + f0 * out_stride, out_stride, d_status + f0);
        }
        return rc;
    }
    const size_t nfr = (size_t)n_streams * frames_per_stream;
    // workspaces: decoder planes, s16 PCM (the transform writes s16 itself: no float PCM in between), the front end's, the encoder's
    // the front end (launch_rule.h): s16 PCM itself, so the one-workgroup-per-stream kernel only with the transform fused in
    const DecChoice fe = dec_choice(ctx->decode_mode, n_streams, frames_per_stream, true, false, false, mix_plan_identity(X.plan),
                                    ctx->mix_pending && X.plan.surr_mask, ctx->fixed_shape != 0, dd.acmod, dd.lfeon ? 1 : 0, t.drc_source == 1 && nfr);
    TRY(ws_grow(ctx, ctx->ws_coef, fe.mantx ? 0 : coef_bytes(nfr, X.plan.n_in)));
    TRY(ws_grow(ctx, ctx->ws_blksw, zs_off(nfr, X.plan.nfchans) + (fe.mixstate ? nfr : 0)));
    TRY(ws_grow(ctx, ctx->ws_tc, s16_ws_bytes(nfr, n_out)));
    TRY(grow_front_ws(ctx, fe, nfr));
    TRY(encode_setup(ctx, E, enc, nfr, nullptr));
    if (t.md_source == 1) TRY(ws_grow(ctx, ctx->ws_bsi, nfr * sizeof(uint32_t)));
    if (t.drc_source == 1) TRY(ws_grow(ctx, ctx->ws_dyn, nfr * 40));      // raw words [nfr][6] u32 | codes [nfr][6][2] | compr [nfr][2] u16
    uint8_t *const zs = fe.mixstate ? ctx->ws_blksw.at<uint8_t>(zs_off(nfr, X.plan.nfchans)) : nullptr;
    int16_t *const ws_s16 = ctx->ws_tc.at<int16_t>();
    // Decoder front end, transform to s16, encoder: back to back on the context's stream.  (Until round 2 two chunks were
    // pipelined over two streams; profiles/transcode_overlap.py measured 12.20 ms with and 12.23 - 12.27 ms without it per
    // 65 536 cold frames, and the sum of the separate decode-to-s16 and encode calls at 12.1 - 12.2 ms: no overlap to keep.
    // Round 4 tried it for MID-SIZE calls, where the one-wavefront-per-stream kernels take their single-wavefront latency of
    // 90 - 140 us whatever the batch: chunks of 2 048 streams on two HIP streams, one chunk's encoder beside the next one's
    // decoder - 3 072 / 4 096 / 8 192 / 16 384 streams 0.561 / 0.644 / 1.265 / 2.175 ms against 0.537 / 0.639 / 1.142 / 2.110
    // in one piece: a kernel of 2 048 frames already occupies every CU (the six-wavefront-per-frame kernels) or is dispatched
    // whole before the other stream's (the others), so the chunks' latency floors add up instead of overlapping.)
    DecodeLaunch D = decode_launch(ctx, fe, &dd, d_frames_in, in_stride, n_streams, frames_per_stream, d_lfsr, d_status);
    TRY(crc_pass(ctx, &dd, d_frames_in, in_stride, nfr, &D.crc));
    if (t.md_source == 1 && nfr) {
        // ac3mi_set_encode_metadata_source 1: the BSI kernel over this call's (or tile's) input frames, after the CRC kernel whose
        // verdicts it reads, ahead of the encoder that codes from its words; an array of ac3mi_set_encode_metadata_frames is not read
        BsiLaunch B;
        B.frames = d_frames_in;
        B.n_frames = nfr;
        B.frame_stride = in_stride;
        B.frame_bytes = dd.frame_bytes;
        B.words = ctx->ws_bsi.at<uint32_t>();
        B.crc = D.crc;
        B.acmod = dd.acmod;
        B.lfeon = dd.lfeon ? 1 : 0;
        B.coded_acmod = E.cfg.acmod;
        B.ctx_word = t.bsi;
        HIPCHK(ctx, launch_bsi(B, ctx->stream));
        E.bsi_words = B.words;
    }
    if (t.drc_source == 1 && nfr) D.src_dyn = ctx->ws_dyn.at<uint32_t>();      // the SRC front ends
    D.coef = fe.mantx ? nullptr : ctx->ws_coef.at<float>();
    D.blksw = ctx->ws_blksw.at<uint8_t>();
    D.zs = zs;
    const bool fused = fe.fused || fe.mantx;            // the front end transforms too: no planes between the kernels
    X.coef = fused ? nullptr : ctx->ws_coef.at<float>();
    X.blksw = fused ? nullptr : ctx->ws_blksw.at<uint8_t>();
    X.zs = zs;
    X.mix_pending = fe.mixstate ? ctx->mix_pending : nullptr;
    X.mix_flags = fe.mixstate ? ctx->mix_flags : nullptr;
    X.delay = d_delay;
    X.slot = ctx->slots;
    X.delay_stride = 6 * 128;
    X.pcm = nullptr;
    X.pcm16 = ws_s16;
    X.s16_flags = out_flags;
    X.n_streams = n_streams;
    X.frames = frames_per_stream;
    X.bias = 384.0f;
    if (fe.fused) HIPCHK(ctx, launch_decode_wg(ctx->tab, D, &X, 0, ctx->stream));
    else {
        if (fe.mantx) D.fuse = &X;
        HIPCHK(ctx, launch_decode(ctx->tab, D, ctx->stream));
        if (!fe.mantx) HIPCHK(ctx, launch_xform(ctx->tab, X, ctx->stream));
    }
    if (D.src_dyn) {
        // ac3mi_set_encode_drc_source 1: the front end's raw words, the frames' status and their BSI resolved into the arrays the
        // encoder codes from, for this call (or tile); arrays of ac3mi_set_encode_dynrng_frames are not read
        DynSrcLaunch R;
        R.frames = d_frames_in;
        R.n_frames = nfr;
        R.frame_stride = in_stride;
        R.frame_bytes = dd.frame_bytes;
        R.src_dyn = D.src_dyn;
        R.status = d_status;
        R.codes = ctx->ws_dyn.at<uint8_t>(nfr * 24);
        R.compr = ctx->ws_dyn.at<uint16_t>(nfr * 36);
        // a dual-mono source coded as dual mono keeps both programmes; else the one the request names becomes programme 0
        R.prog = dd.acmod == 0 && E.cfg.acmod == 0 ? -1 : dd.acmod == 0 && (dd.flags & AC3MI_CHANNEL_MASK) == AC3MI_CHANNEL2 ? 1 : 0;
        HIPCHK(ctx, launch_dynrng_source(R, ctx->stream));
        E.dyn_codes = R.codes;
        E.compr_words = R.compr;
    }
    E.pcm = ws_s16;
    E.last = d_last;
    E.csnr = d_csnroffst;
    E.frames = d_frames_out;
    E.frame_stride = out_stride;
    E.n_streams = n_streams;
    E.frames_per_stream = frames_per_stream;
    if (fe.split) {                                     // block 0's descriptor of every frame carries the source's SNR offsets
        E.search_hint = reinterpret_cast<const uint32_t *>(D.ws_desc) + BLKDESC_SRC_SNR / 4;      // BlkDesc::src_snr
        E.search_hint_stride = 6 * BLKDESC_BYTES / 4;                                            // six descriptors per frame
    }
    HIPCHK(ctx, launch_encode(ctx->tab, E, ctx->stream));
    return AC3MI_OK;
}

}  // extern "C"
