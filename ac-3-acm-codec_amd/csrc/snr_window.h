// snr_window.h — the window rule of the SNR-offset search, stated once: how enc_search_kernel<1> (encode.hip) gets a frame's
// exact mantissa cost at SIXTEEN consecutive offsets g_lo .. g_lo + 15 (g = 16 csnroffst + fsnroffst) from one pass over the
// frame's run-start rows, and which window it costs next.  The kernel, the host program of tests/snr_window_c and (restated
// in Python) profiles/search_window_sim.py follow this file.
//
// A coefficient's bap table address at offset g is clamp(80 - k - 4 e, 0, 63): e its encoded exponent, k = max((m - so) >> 5, 0)
// of its BAND, m the row's band mask word, so = (g - 240) << 2 (ENC/ac3enc.cpp:393-420).  g enters through k alone, k belongs
// to the band and not to the bin, and with x = m - so(g_lo): k(g_lo + t) = max((x - 4 t) >> 5, 0) steps down by one at
// t1 = ((x & 31) >> 2) + 1 (1..8) and again at t1 + 8 - never below 0.  Over a window a band so takes at most three values
// k0, k0 - 1, k0 - 2 and all its bins step together: three look-ups per bin (addresses a0, a0 + 1, a0 + 2, each clamped), summed
// per band into W0, W1, W2, hold the frame's cost at all sixteen offsets - a block's packed totals at t are
// sum W0 + sum over bands with t1 <= t of (W1 - W0) + sum over bands with t2 <= t of (W2 - W1): a prefix sum over t of a histogram.
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

constexpr int WIN_N = 16;           // offsets of a window
constexpr int WIN_NEVER = 16;       // a step that does not happen inside the window (histogram slot 16 is never read)
constexpr int WIN_LO_MAX = 1008;    // the window's start lies in 0 .. 1008

// snroffset of offset g (:393-420 with floor folded into the mask words)
__host__ __device__ inline int win_snroffset(int g) { return (g - 240) * 4; }

// x = m - snroffset(g_lo) -> k at the window's start and the steps t1 < t2 at which it falls by one
__host__ __device__ inline void win_steps(int x, int &k0, int &t1, int &t2)
{
    const int k = x >> 5;
    k0 = k < 0 ? 0 : k;
    const int s = ((x & 31) >> 2) + 1;
    t1 = k >= 1 ? s : WIN_NEVER;
    t2 = k >= 2 ? s + 8 : WIN_NEVER;     // (9 .. 16: 16 is never too)
}
// steps taken at offset g_lo + t
__host__ __device__ inline int win_taken(int t, int t1, int t2) { return (t >= t1) + (t >= t2); }

// the band's term for its bins, four times the address as the cost table is indexed in bytes: a bin's address x 4 after j steps
// is clamp(term + 4 j - 16 e, 0, 252)
__host__ __device__ inline int win_term(int k0) { return 320 - 4 * k0; }
__host__ __device__ inline int win_addr(int k0, int j, int e)
{
    const int a = 80 - k0 + j - 4 * e;
    return a < 0 ? 0 : a > 63 ? 63 : a;
}

// The cost table's word of one coefficient: plain mantissa bits | 3-level << 9 | 5-level << 14 | 11-level << 19; a BAND's sum
// (<= 24 members, <= 384 bits) stays inside those fields.  A BLOCK's totals (<= 6 x 253 members: bits < 2^15, each count < 2^11)
// need two words: A = bits | 3-level << 15, B = 5-level | 11-level << 11.  Both maps are linear, so sums and differences may be
// formed modulo 2^32 on either side as long as the final total is a true (non-negative) one.
__host__ __device__ inline uint32_t win_wide_a(uint32_t w) { return (w & 0x1ffu) | ((w & 0x3e00u) << 6); }
__host__ __device__ inline uint32_t win_wide_b(uint32_t w) { return ((w >> 14) & 0x1fu) | ((w >> 8) & 0xf800u); }

// A block's mantissa bits from its two total words: the plain bits and the grouped codes' ceilings (:1194-1238 - a 5-bit code
// per three 3-level mantissas, 7 bits per three 5-level or two 11-level ones); extra6 = what the ceilings add beyond the
// nominal 5/3, 7/3 and 7/2 bits per mantissa, in sixths of a bit (<= 69: the search's monotone bounds)
__host__ __device__ inline uint32_t win_block_bits(uint32_t a, uint32_t b, uint32_t &extra6)
{
    const uint32_t n1 = a >> 15, n2 = b & 0x7ffu, n4 = b >> 11;
    const uint32_t t = 5u * (((n1 + 2u) * 0xaaabu) >> 17) + 7u * (((n2 + 2u) * 0xaaabu) >> 17) + 7u * ((n4 + 1u) >> 1);
    extra6 = 6u * t - (10u * n1 + 14u * n2 + 21u * n4);
    return (a & 0x7fffu) + t;
}

// ---- which window to cost ----
// Which offsets are costed never changes a result (the reference's sequence is replayed from exact verdicts); the rule only
// decides how many sweeps a frame takes.  profiles/search_window_sim.py runs it on the oracle's spare-bit curves.
__host__ __device__ inline int win_clamp_lo(int lo) { return lo < 0 ? 0 : lo > WIN_LO_MAX ? WIN_LO_MAX : lo; }

constexpr int WIN_HINT_BELOW = 5;   // a transcode's re-encode lands -5 .. +9 steps from its source's offsets: [hint - 5, hint + 11)
constexpr int WIN_COLD_LO = 176;    // a fresh stream (state 40/0, no hint): csnroffst 11, where 384 kbps 5.1 material lands
constexpr int WIN_WARM_BELOW = 6;   // a stream's next frame: around the last coded frame's offsets
constexpr int WIN_LINE_SWEEPS = 4;  // from this sweep on the bracket is halved, not interpolated: the bounded fallback
constexpr int WIN_ASK_SWEEPS = 7;   // from this sweep on the window is laid around the reference's open question itself

// first window of a frame: hint = the source frame's offsets (> 0) or 0, cold = the state AC3_encode_init leaves,
// g_prev = 16 csnroffst + fsnroffst of the stream's last coded frame
__host__ __device__ inline int win_first_lo(int hint, bool cold, int g_prev)
{
    return win_clamp_lo(hint > 0 ? hint - WIN_HINT_BELOW : cold ? WIN_COLD_LO : g_prev - WIN_WARM_BELOW);
}

// a later window.  sweeps = windows costed so far (>= 1); gl / gh = the largest costed offset that fits / the smallest that
// fails (-1: none) with their spare bits sl >= 0 > sh; slope15 = spare(lo) - spare(lo + 15) of the LAST window; cmin / cmax =
// the lowest and the highest offset costed so far; gq = the offset the reference asks about and no verdict answers.
__host__ __device__ inline int win_next_lo(int sweeps, int gl, int sl, int gh, int sh, int slope15, int cmin, int cmax, int gq)
{
    if (sweeps >= WIN_ASK_SWEEPS) return win_clamp_lo(gq - 8);
    // A question beside the boundary (the reference's ladder of csnroffst values below a frame that lands at the foot of its
    // window, say): the window next to what is costed, not the one around the question - offsets a step or two clear of the
    // boundary fit or fail by the margin that settles every offset beyond them (fit_hi / fail_lo), one sweep for the whole ladder
    const int around = win_clamp_lo(gq < cmin ? cmin - WIN_N : gq > cmax ? cmax + 1 : gq - 8);
    if (gl >= 0 && gh >= 0) {
        // the fit is not monotone here, or the boundary is pinned and the reference asks elsewhere
        if (gh <= gl + 1 || gq <= gl || gq >= gh) return around;
        const int w = gh - gl;
        if (w - 1 <= WIN_N) return win_clamp_lo(gl + 1);                // all that lies between
        int est = gl + (w >> 1);
        if (sweeps < WIN_LINE_SWEEPS) est = gl + (w * sl + ((sl - sh) >> 1)) / (sl - sh);    // where the line crosses zero
        int lo = est - 8;
        lo = lo < gl + 1 ? gl + 1 : lo;
        lo = lo > gh - WIN_N ? gh - WIN_N : lo;
        return win_clamp_lo(lo);
    }
    if (gh < 0 ? gq <= gl : gq >= gh) return around;                    // (one side known, the question on the other)
    if (gh < 0) {
        // everything costed fits: up along the window's own slope (a flat curve: to the top); halfway to the top as fallback
        int est = slope15 > 0 ? gl + (15 * sl) / slope15 : 1023;
        if (sweeps >= WIN_LINE_SWEEPS) est = gl + ((1024 - gl) >> 1);
        est = est > 1023 ? 1023 : est;
        const int lo = est - 8;
        return win_clamp_lo(lo < gl + 1 ? gl + 1 : lo);
    }
    // nothing costed fits: down
    int est = slope15 > 0 ? gh - (15 * -sh) / slope15 : 0;
    if (sweeps >= WIN_LINE_SWEEPS) est = gh >> 1;
    est = est < 0 ? 0 : est;
    const int lo = est - 7;
    return win_clamp_lo(lo > gh - WIN_N ? gh - WIN_N : lo);
}

}  // namespace ac3mi
