// truepeak_rule.h — the parts of the true-peak meter (ac3mi_truepeak_*, include/ac3mi.h) that need no GPU: the state's layout,
// the frozen interpolator of ITU-R BS.1770-4 Annex 2 as integers (its coefficients times 8192), the proof that a phase never
// leaves an int32, and the steps - an instant's four phases of the oversampled signal, the ordering of maxima, the
// saturating count, the read-out - as __host__ __device__ functions that truepeak_kernel / truepeak_read_kernel (truepeak.hip)
// and the host twins ac3mi_truepeak_host / ac3mi_truepeak_read both call.  Integers throughout: no float decides anything (dbtp and dbfs of the
// record are informative).
// Plain C++: compiles without HIP (a host-only build of truepeak.hip for the sanitiser program of tests/truepeak_c).
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

constexpr int TP_PHASES = 4, TP_TAPS = 12;
constexpr int TP_HIST = TP_TAPS - 1;    // the samples before an instant that its four phases read
constexpr int TP_SEG = 24;              // sample instants a lane owns in a frame: 64 x 24 = 1536

// One stream's state (ac3mi_truepeak_state_bytes() = sizeof): all zeros is a new stream.  An unmeasured slot's fields stay 0.
struct TruePeakState {
    uint64_t samples;                   // sample instants metered
    uint64_t index[6];                  // per slot: the smallest 4 n + p at which true_peak occurs
    uint32_t true_peak[6];              // ... max |y|, in 2^-28 of full scale
    uint32_t sample_peak[6];            // ... max |x|, 0..32768
    uint32_t full_scale[6];             // ... samples equal to -32768 or 32767, saturating
    int16_t hist[6][TP_HIST];           // ... the last 11 samples, oldest first
    uint8_t measured;                   // bit c: slot c has been metered (the read-out's "no slot was measured")
    uint8_t reserved[3];                // 0
};
static_assert(sizeof(TruePeakState) == 264 && sizeof(TruePeakState) % 8 == 0 && offsetof(TruePeakState, hist) == 128, "TruePeakState layout");
static_assert(sizeof(ac3mi_truepeak_result) == 96 && offsetof(ac3mi_truepeak_result, slot_true_peak) == 28 &&
              offsetof(ac3mi_truepeak_result, dbtp) == 76, "ac3mi_truepeak_result layout");

// H[p][k], frozen: Annex 2's 48-tap interpolator split into its four phases, times 8192 (every product is a whole number);
// phases 2 and 3 are phases 1 and 0 reversed
__host__ __device__ constexpr int tp_coef(int p, int k)
{
    constexpr int16_t h[2][TP_TAPS] = {{14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68},
                                       {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155}};
    return p < 2 ? h[p][k] : h[3 - p][TP_TAPS - 1 - k];
}

constexpr int64_t tp_abs_sum(int p)
{
    int64_t s = 0;
    for (int k = 0; k < TP_TAPS; k++) s += tp_coef(p, k) < 0 ? -tp_coef(p, k) : tp_coef(p, k);
    return s;
}
// |y| <= 32768 * (a phase's absolute sum): 542 998 528 for phases 1 and 2, so the int32 sum never wraps - and every partial sum
// is bounded alike - and |y| leaves two bits of a u32 free
static_assert(tp_abs_sum(0) == 11749 && tp_abs_sum(1) == 16571 && tp_abs_sum(2) == 16571 && tp_abs_sum(3) == 11749, "Annex 2 table");
static_assert(32768 * tp_abs_sum(1) == 542998528 && 32768 * tp_abs_sum(1) < (int64_t(1) << 30), "a phase fits an int32");

// y[4 n + p] = sum over k of H[p][k] x[n - k], p = 0..3, from the 12 samples x[n - 11] .. x[n] in time order (x12[11] is x[n]).
// The host twin runs this; truepeak_kernel forms the same int32 sums from pairs of samples with packed 16-bit dot products
// (tp_phases_packed, truepeak_packed.h) - integer sums that cannot wrap, so the same bits in any order of adding.
template <class X>
__host__ __device__ inline void tp_phases(const X *x12, int32_t y[TP_PHASES])
{
    for (int p = 0; p < TP_PHASES; p++) {
        int32_t a = 0;
        for (int k = 0; k < TP_TAPS; k++) a += tp_coef(p, k) * (int32_t)x12[TP_TAPS - 1 - k];
        y[p] = a;
    }
}

__host__ __device__ inline uint32_t tp_abs(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

// is -32768 or 32767
__host__ __device__ inline bool tp_full_scale(int32_t x) { return x == -32768 || x == 32767; }

// The ordering of maxima: (a, ia) goes before (b, ib) when it is larger, or as large and earlier.  Walking the instants in
// order, a new value replaces the old only when strictly greater; lanes, slots (lower slot first) and calls combine by this.
template <class I>
__host__ __device__ inline bool tp_before(uint32_t a, I ia, uint32_t b, I ib) { return a > b || (a == b && ia < ib); }

__host__ __device__ inline uint32_t tp_add_sat(uint32_t a, uint64_t b)
{
    const uint64_t s = (uint64_t)a + b;
    return s > 0xffffffffu || s < b ? 0xffffffffu : (uint32_t)s;
}

// The read-out of one state
__host__ __device__ inline void tp_result(const TruePeakState *st, uint32_t ceiling_q28, ac3mi_truepeak_result *out)
{
    ac3mi_truepeak_result r;
    r.true_peak_index = 0;
    r.samples = st->samples;
    r.true_peak = r.sample_peak = r.full_scale = 0;
    r.true_peak_slot = r.sample_peak_slot = 0;
    for (int c = 0; c < 6; c++) {
        r.slot_true_peak[c] = st->true_peak[c];
        r.slot_sample_peak[c] = st->sample_peak[c];
        if (c == 0 || tp_before(st->true_peak[c], st->index[c], r.true_peak, r.true_peak_index)) {
            r.true_peak = st->true_peak[c];
            r.true_peak_index = st->index[c];
            r.true_peak_slot = (uint8_t)c;
        }
        if (st->sample_peak[c] > r.sample_peak) {
            r.sample_peak = st->sample_peak[c];
            r.sample_peak_slot = (uint8_t)c;
        }
        r.full_scale = tp_add_sat(r.full_scale, st->full_scale[c]);
    }
    r.dbtp = r.true_peak ? (float)(20.0 * log10((double)r.true_peak / 268435456.0)) : -200.0f;
    r.dbfs = r.sample_peak ? (float)(20.0 * log10((double)r.sample_peak / 32768.0)) : -200.0f;
    r.flags = (uint8_t)(((st->samples == 0 || st->measured == 0) ? AC3MI_TRUEPEAK_EMPTY : 0) |
                        ((ceiling_q28 != 0 && r.true_peak > ceiling_q28) ? AC3MI_TRUEPEAK_OVER : 0));
    for (int i = 0; i < 9; i++) r.reserved[i] = 0;
    *out = r;
}

// floor(2^28 10^(dbtp / 20)) clamped to a u32 (not a number: 0)
inline uint32_t truepeak_ceiling_host(double dbtp)
{
    const double v = floor(268435456.0 * pow(10.0, dbtp / 20.0));
    return !(v >= 0.0) ? 0u : v >= 4294967295.0 ? 0xffffffffu : (uint32_t)v;
}

inline void truepeak_tables_host(int16_t *h48)
{
    for (int p = 0; p < TP_PHASES; p++)
        for (int k = 0; k < TP_TAPS; k++) h48[p * TP_TAPS + k] = (int16_t)tp_coef(p, k);
}

inline void truepeak_read_host(const void *h_state, uint32_t ceiling_q28, ac3mi_truepeak_result *out)
{
    TruePeakState st;
    memcpy(&st, h_state, sizeof st);
    tp_result(&st, ceiling_q28, out);
}

// The meter as the rule states it, sample by sample: `frames` frames of one stream, pcm [frames][1536][channels] interleaved,
// on a state in host memory (any alignment)
inline void truepeak_meter_host(int channels, const uint8_t *role, const int16_t *pcm, int frames, void *h_state)
{
    TruePeakState st;
    memcpy(&st, h_state, sizeof st);
    const uint64_t n_new = (uint64_t)frames * 1536u;
    for (int c = 0; c < channels; c++) {
        if (role[c] == 0) continue;
        int32_t x[TP_TAPS];                             // x[1 ..] the last 11 samples, then the window x[n - 11] .. x[n]
        x[0] = 0;
        for (int j = 0; j < TP_HIST; j++) x[j + 1] = st.hist[c][j];
        uint64_t count = 0;
        for (uint64_t i = 0; i < n_new; i++) {
            memmove(x, x + 1, TP_HIST * sizeof x[0]);
            const int32_t s = pcm[i * (uint64_t)channels + (uint64_t)c];
            x[TP_TAPS - 1] = s;
            int32_t y[TP_PHASES];
            tp_phases(x, y);
            for (int p = 0; p < TP_PHASES; p++) {
                const uint32_t a = tp_abs(y[p]);
                if (a > st.true_peak[c]) {              // in time order: only a strictly greater value replaces
                    st.true_peak[c] = a;
                    st.index[c] = 4 * (st.samples + i) + (uint64_t)p;
                }
            }
            const uint32_t m = tp_abs(s);
            if (m > st.sample_peak[c]) st.sample_peak[c] = m;
            count += tp_full_scale(s) ? 1 : 0;
        }
        st.full_scale[c] = tp_add_sat(st.full_scale[c], count);
        for (int j = 0; j < TP_HIST; j++) st.hist[c][j] = (int16_t)x[j + 1];
        st.measured |= (uint8_t)(1u << c);
    }
    st.samples += n_new;
    memcpy(h_state, &st, sizeof st);
}

}  // namespace ac3mi
