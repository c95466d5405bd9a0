// resample_rule.h — the parts of the sample-rate converter (ac3mi_resample_*, include/ac3mi.h) that need no GPU: the state's
// layout, the ratio / tap-count / plan arithmetic, the table's design (the only place with a float), the hi / lo split of a
// coefficient with the check that lets the sums run in 32 bits, one output instant as __host__ __device__ functions that
// resample_kernel (resample.hip) and the host twin ac3mi_resample_host both call, and the converter as the rule states it,
// output instant by output instant.  Integers decide every bit.
// Plain C++: compiles without HIP (a host-only build of resample.hip for the sanitiser program of tests/resample_c).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/ac3mi.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

constexpr int RS_HIST = 96;             // input samples kept per slot; the longest filter (96 taps) reads 95 of them
constexpr int RS_MAX_TAPS = 96, RS_MAX_L = 441;
constexpr int RS_PAIRS = 6;
constexpr int RS_MAX_FRAMES = 1 << 20;  // frames per call and stream, either side: an instant's place in a call fits a u32
constexpr int32_t RS_ONE = 1 << 23;     // coefficients are Q23
static_assert(RS_HIST >= RS_MAX_TAPS - 1 && RS_HIST % 2 == 0, "the history holds what the longest filter reads");
// |acc| <= 32768 * sum |C| < 2^41 for any table whose split passes rs_split (sum |C| <= 512 * 65535 + 65535)
static_assert(32768ll * (512ll * 65535 + 65535) < (1ll << 41), "acc fits the rule's bound");

// One stream's state (ac3mi_resample_state_bytes() = sizeof): all zeros is a new stream.  Slots >= channels stay 0, and so does
// every pend entry from the pending count on (the count is not stored: it follows from samples_in and frames_out)
struct ResampleState {
    uint64_t samples_in;                // input instants pushed
    uint64_t frames_out;                // output frames taken
    uint8_t tag;                        // 0 = new, else 1 + 6 * pair + (channels - 1)
    uint8_t zero[7];
    int16_t hist[6][RS_HIST];           // the last 96 input samples of every slot, oldest first
    int16_t pend[1536 * 6];             // the pending output instants, oldest first, interleaved [instant][channels]
};
static_assert(sizeof(ResampleState) == 19608 && sizeof(ResampleState) % 8 == 0 && offsetof(ResampleState, tag) == 16 &&
              offsetof(ResampleState, hist) == 24 && offsetof(ResampleState, pend) == 1176, "ResampleState layout");

// the pair's place in the header's table, -1 for anything the converter refuses
inline int rs_pair(int in_rate, int out_rate)
{
    static const int pairs[RS_PAIRS][2] = {{44100, 48000}, {48000, 44100}, {32000, 48000}, {48000, 32000}, {32000, 44100}, {44100, 32000}};
    for (int i = 0; i < RS_PAIRS; i++)
        if (pairs[i][0] == in_rate && pairs[i][1] == out_rate) return i;
    return -1;
}

inline bool rs_ratio(int in_rate, int out_rate, int *L, int *M, int *T)
{
    if (rs_pair(in_rate, out_rate) < 0) return false;
    int a = in_rate, b = out_rate;
    while (b) { const int t = a % b; a = b; b = t; }
    const int l = out_rate / a, m = in_rate / a;
    if (L) *L = l;
    if (M) *M = m;
    if (T) *T = l > m ? 64 : 8 * ((64 * m + 8 * l - 1) / (8 * l));
    return true;
}

__host__ __device__ inline uint8_t rs_tag(int pair, int channels) { return (uint8_t)(1 + 6 * pair + (channels - 1)); }

// output instants that exist after n input instants: ceil(n L / M)  (n < 2^52 here: rs_plan refuses older streams)
__host__ __device__ inline uint64_t rs_out_count(uint64_t n, uint32_t L, uint32_t M) { return (n * L + (M - 1)) / M; }

// The elastic buffer's arithmetic.  false: the stream cannot be that old (a state nobody's call left)
__host__ __device__ inline bool rs_plan(uint32_t L, uint32_t M, uint64_t samples_in, uint64_t frames_out, uint32_t in_frames, uint64_t *out_frames,
                                        uint32_t *pending_before, uint32_t *pending_after)
{
    if (samples_in >= (1ull << 52) || frames_out >= (1ull << 52)) return false;
    const uint64_t had = rs_out_count(samples_in, L, M), have = rs_out_count(samples_in + 1536ull * in_frames, L, M);
    if (had < 1536 * frames_out || had - 1536 * frames_out >= 1536) return false;
    const uint64_t total = have - 1536 * frames_out;
    *out_frames = total / 1536;
    *pending_before = (uint32_t)(had - 1536 * frames_out);
    *pending_after = (uint32_t)(total % 1536);
    return true;
}

// The table: C[L][T], Q23, in double in exactly the header's expression order
inline double rs_i0(double x)
{
    double s = 1.0, term = 1.0;
    for (int j = 1;; j++) {
        const double v = x / 2 / j;
        term *= v * v;
        s += term;
        if (term < 1e-21 * s) return s;
    }
}

inline void rs_build_table(int L, int M, int T, int32_t *C)
{
    const double pi = 3.14159265358979323846, beta = 9.2;
    const double r = (double)L / M < 1.0 ? (double)L / M : 1.0;
    const double i0b = rs_i0(beta);
    for (int p = 0; p < L; p++) {
        int32_t *row = C + (size_t)p * T;
        int64_t sum = 0;
        int top = 0;
        for (int k = 0; k < T; k++) {
            const double t = (k + (double)p / L) - T / 2;
            const double a = r * t;
            const double sinc = a == 0 ? 1.0 : sin(pi * a) / (pi * a);
            const double q = (2 * t) / T;
            const double u = 1 - q * q;
            const double w = rs_i0(beta * sqrt(u > 0.0 ? u : 0.0)) / i0b;
            const double h = (r * sinc) * w;
            row[k] = (int32_t)floor(8388608 * h + 0.5);
            sum += row[k];
            if (row[k] > row[top]) top = k;     // the first largest
        }
        row[top] += (int32_t)(RS_ONE - sum);
    }
}

// C = 512 hi + lo, lo in [-256, 255].  false unless every hi fits an int16 and both absolute phase sums stay at or under 65535:
// then |sum hi x| and |sum lo x| <= 65535 * 32768 < 2^31 for every s16 input
inline bool rs_split(const int32_t *C, int L, int T, int16_t *hi, int16_t *lo)
{
    for (int p = 0; p < L; p++) {
        int64_t ah = 0, al = 0;
        for (int k = 0; k < T; k++) {
            const int32_t c = C[(size_t)p * T + k], h = (c + 256) >> 9, l = c - 512 * h;
            if (h < -32768 || h > 32767) return false;
            hi[(size_t)p * T + k] = (int16_t)h;
            lo[(size_t)p * T + k] = (int16_t)l;
            ah += h < 0 ? -h : h;
            al += l < 0 ? -l : l;
        }
        if (ah > 65535 || al > 65535) return false;
    }
    return true;
}

// y from the two 32-bit sums A = sum hi x and B = sum lo x: acc = 512 A + B is the only 64-bit step
__host__ __device__ inline int32_t rs_round(int32_t A, int32_t B)
{
    const int64_t acc = 512 * (int64_t)A + B;
    const int64_t y = (acc + (1 << 22)) >> 23;
    return y < -32768 ? -32768 : y > 32767 ? 32767 : (int32_t)y;
}

// One output instant of one slot: hi and lo are the phase's rows, x(k) is x[i - k]
template <class X>
__host__ __device__ inline int32_t rs_output(const int16_t *hi, const int16_t *lo, int T, X x)
{
    int32_t A = 0, B = 0;
    for (int k = 0; k < T; k++) {
        const int32_t v = x(k);
        A += hi[k] * v;
        B += lo[k] * v;
    }
    return rs_round(A, B);
}

struct ResampleTable {
    int L, M, T, pair;
    const int16_t *hi, *lo;             // [L][T]
};

// The converter as the rule states it: in_frames frames of one stream in, out_frames out, on a state in host memory (any
// alignment).  Returns the stream's status; a refused stream's state is untouched and its output frames are zeros
inline uint32_t resample_host(const ResampleTable &tb, int channels, const int16_t *pcm, int in_frames, int16_t *out, int out_frames, void *h_state)
{
    ResampleState st, nw;
    memcpy(&st, h_state, sizeof st);
    const uint8_t tag = rs_tag(tb.pair, channels);
    uint32_t status = 0, before = 0, after = 0;
    uint64_t planned = 0;
    if (st.tag ? st.tag != tag : (st.samples_in | st.frames_out) != 0) status = AC3MI_RESAMPLE_STATE;
    else if (!rs_plan((uint32_t)tb.L, (uint32_t)tb.M, st.samples_in, st.frames_out, (uint32_t)in_frames, &planned, &before, &after) ||
             planned != (uint64_t)out_frames)
        status = AC3MI_RESAMPLE_FRAMES;
    if (status) {
        if (out_frames > 0) memset(out, 0, (size_t)out_frames * 3072u * (size_t)channels);
        return status;
    }
    nw = st;
    memset(nw.pend, 0, sizeof(int16_t) * 1536u * (size_t)channels);
    const uint64_t n = st.samples_in, cap = 1536ull * (uint64_t)out_frames, total = cap + after;
    for (uint64_t rel = 0; rel < total; rel++) {
        int16_t *dst = rel < cap ? out + rel * (uint64_t)channels : nw.pend + (rel - cap) * (uint64_t)channels;
        if (rel < before) {
            for (int c = 0; c < channels; c++) dst[c] = st.pend[rel * (uint64_t)channels + c];
            continue;
        }
        const uint64_t q = (1536 * st.frames_out + rel) * (uint64_t)tb.M;
        const int64_t i = (int64_t)(q / (uint64_t)tb.L - n);           // the newest input the instant reads, counted in the call: >= 0
        const size_t row = (size_t)(q % (uint64_t)tb.L) * (size_t)tb.T;
        for (int c = 0; c < channels; c++)
            dst[c] = (int16_t)rs_output(tb.hi + row, tb.lo + row, tb.T, [&](int k) -> int32_t {
                const int64_t at = i - k;
                return at >= 0 ? pcm[at * channels + c] : st.hist[c][RS_HIST + at];
            });
    }
    const int64_t n_new = 1536ll * in_frames;
    for (int c = 0; c < channels; c++)
        for (int j = 0; j < RS_HIST; j++) nw.hist[c][j] = pcm[(n_new - RS_HIST + j) * channels + c];
    nw.samples_in = n + (uint64_t)n_new;
    nw.frames_out = st.frames_out + (uint64_t)out_frames;
    nw.tag = tag;
    memcpy(h_state, &nw, sizeof nw);
    return 0;
}

}  // namespace ac3mi
