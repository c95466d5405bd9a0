// limit_rule.h — the parts of the true-peak limiter (ac3mi_limit_*, include/ac3mi.h) that need no GPU: the state's layout, the
// rule's steps - an instant's detector value, the exact quotient, the gain's application - as __host__ __device__ functions
// that limit_kernel / limit_read_kernel (limit.hip) and the host twins ac3mi_limit_host / ac3mi_limit_read both call, the
// read-out, and the limiter as the rule states it, sample by sample.  Integers throughout: no float decides anything (in_dbtp
// and reduction_db of the record are informative).  The interpolator is truepeak_rule.h's; nothing of it is restated here.
// Plain C++: compiles without HIP (a host-only build of limit.hip for the sanitiser program of tests/limit_c).
#pragma once
#include "truepeak_rule.h"

namespace ac3mi {

constexpr uint32_t LIM_ONE = 1u << 24;          // gains are Q24
constexpr int LIM_HOLD = 80;                    // W: m[n] = min q[n - 79 .. n]
constexpr int LIM_SMOOTH = 64;                  // B: g[n] = (sum r[n - 63 .. n]) >> 6
constexpr int LIM_DELAY = AC3MI_LIMIT_DELAY;    // D
constexpr int LIM_HIST = 80;                    // input samples kept per slot (the delay's 77 and the interpolator's 11 lie inside)
constexpr uint32_t LIM_MAX_CEILING = 1u << 28, LIM_MAX_STEP = 1u << 20;
static_assert(LIM_DELAY == 77 && LIM_DELAY <= LIM_HIST && TP_HIST <= LIM_HIST, "the history holds what the delay and the phases read");
// the 64 hold windows that g[n] averages all contain [n - 79, n - 63]: 17 instants, whose phases describe the times
// n - 84.875 .. n - 68.125, (n - 77) +- 8 around the sample that g[n] multiplies
static_assert(LIM_HOLD - LIM_SMOOTH == 16, "the look-ahead covers the delay");
// the min-plus scan of r stays inside an int32 over a frame: 1536 steps of at most 2^20 below -  and 24 above - a Q24 gain
static_assert(1536ll * LIM_MAX_STEP + LIM_ONE < (1ll << 31), "the scan of r fits an int32");
static_assert((uint64_t)LIM_SMOOTH * LIM_ONE < (1ull << 32), "the window sum of r fits a u32");

// One stream's state (ac3mi_limit_state_bytes() = sizeof): all zeros is a new stream, so gains are kept as reductions ONE - v
struct LimitState {
    uint64_t samples;                   // sample instants processed
    uint64_t reduced;                   // ... with g[n] < ONE
    uint32_t max_detect;                // max d[n]
    uint32_t max_reduction;             // ONE - min g[n]
    uint32_t q_red[LIM_HOLD];           // ONE - q of the last 80 instants, oldest first
    uint32_t r_red[LIM_SMOOTH];         // ONE - r of the last 64 instants, oldest first; the last is r[n - 1]
    int16_t hist[6][LIM_HIST];          // the last 80 input samples of every slot, oldest first; slots >= channels stay 0
};
static_assert(sizeof(LimitState) == 1560 && sizeof(LimitState) % 8 == 0 && offsetof(LimitState, max_detect) == 16 &&
              offsetof(LimitState, q_red) == 24 && offsetof(LimitState, r_red) == 344 && offsetof(LimitState, hist) == 600, "LimitState layout");
static_assert(sizeof(ac3mi_limit_result) == 40 && offsetof(ac3mi_limit_result, max_detect) == 16 && offsetof(ac3mi_limit_result, in_dbtp) == 24 &&
              offsetof(ac3mi_limit_result, flags) == 32, "ac3mi_limit_result layout");

// One slot's share of d[n] from the 12 samples x[n - 11] .. x[n] in time order: the four phases at instant n, and the two
// samples at n - 5 and n - 6 that lie beside them in time (phase p is the signal at n - 5.875 + p / 4), in the phases' unit
template <class X>
__host__ __device__ inline uint32_t lim_detect(const X *x12)
{
    int32_t y[TP_PHASES];
    tp_phases(x12, y);
    uint32_t a = tp_abs((int32_t)x12[TP_TAPS - 1 - 5]) << 13;
    const uint32_t b = tp_abs((int32_t)x12[TP_TAPS - 1 - 6]) << 13;
    a = b > a ? b : a;
    for (int p = 0; p < TP_PHASES; p++) a = tp_abs(y[p]) > a ? tp_abs(y[p]) : a;
    return a;
}

// q[n]: ONE where the detector is at or under the ceiling, else floor(C 2^24 / d) - exact, the numerator has up to 52 bits
__host__ __device__ inline uint32_t lim_quot(uint32_t ceiling_q28, uint32_t d)
{
    return d <= ceiling_q28 ? LIM_ONE : (uint32_t)(((uint64_t)ceiling_q28 << 24) / d);
}

// z = (x g + 2^23) >> 24, floor, for an s16 x and 0 <= g <= ONE, without a 64-bit product: with g = gh 2^12 + gl the sum is
// A 2^12 + B, A = x gh, B = x gl + 2^23, and floor((A 2^12 + B) / 2^24) = floor((A + floor(B / 2^12)) / 2^12) because A is whole.
// |A|, |B| < 2^28, and both factors of either product fit 24 bits (one full-rate multiply on the device).  g <= ONE gives
// |z| <= |x|: no clamp.
__host__ __device__ inline int32_t lim_apply(int32_t x, uint32_t g)
{
    const int32_t a = x * (int32_t)(g >> 12), b = x * (int32_t)(g & 0xfffu) + (1 << 23);
    return (a + (b >> 12)) >> 12;
}

// The read-out of one state
__host__ __device__ inline void lim_result(const LimitState *st, ac3mi_limit_result *out)
{
    ac3mi_limit_result r;
    r.samples = st->samples;
    r.reduced = st->reduced;
    r.max_detect = st->max_detect;
    r.min_gain_q24 = LIM_ONE - st->max_reduction;
    r.in_dbtp = st->max_detect ? (float)(20.0 * log10((double)st->max_detect / 268435456.0)) : -200.0f;
    r.reduction_db = st->max_reduction == 0 ? 0.0f : r.min_gain_q24 == 0 ? -200.0f : (float)(20.0 * log10((double)r.min_gain_q24 / 16777216.0));
    r.flags = (uint8_t)((st->samples == 0 ? AC3MI_LIMIT_EMPTY : 0) | (st->reduced > 0 ? AC3MI_LIMIT_ACTIVE : 0));
    for (int i = 0; i < 7; i++) r.reserved[i] = 0;
    *out = r;
}

// ceil(2^24 / (rate ms / 1000)) clamped to [1, 2^20]; not a number (or not positive): 1
inline uint32_t limit_release_step_host(int sample_rate, double full_recovery_ms)
{
    const double v = ceil(16777216.0 / ((double)sample_rate * full_recovery_ms / 1000.0));
    return !(v >= 1.0) ? 1u : v >= (double)LIM_MAX_STEP ? LIM_MAX_STEP : (uint32_t)v;
}

inline void limit_read_host(const void *h_state, ac3mi_limit_result *out)
{
    LimitState st;
    memcpy(&st, h_state, sizeof st);
    lim_result(&st, out);
}

// what both entry points refuse (the pointers apart)
inline bool limit_params_ok(int channels, uint32_t ceiling_q28, uint32_t release_step_q24, int frames)
{
    return channels >= 1 && channels <= 6 && ceiling_q28 >= 1 && ceiling_q28 <= LIM_MAX_CEILING && release_step_q24 >= 1 &&
           release_step_q24 <= LIM_MAX_STEP && frames >= 1;
}

// The limiter as the rule states it, sample by sample: `frames` frames of one stream, pcm and out [frames][1536][channels]
// interleaved (out == pcm: in place), on a state in host memory (any alignment)
inline void limit_host(int channels, const uint8_t *role, uint32_t C, uint32_t R, const int16_t *pcm, int16_t *out, int frames, void *h_state)
{
    LimitState st;
    memcpy(&st, h_state, sizeof st);
    const uint64_t n_new = (uint64_t)frames * 1536u;
    for (uint64_t i = 0; i < n_new; i++) {
        const int16_t *x = pcm + i * (uint64_t)channels;
        uint32_t d = 0;
        for (int c = 0; c < channels; c++) {
            if (role[c] == 0) continue;
            int32_t x12[TP_TAPS];
            for (int j = 0; j < TP_HIST; j++) x12[j] = st.hist[c][LIM_HIST - TP_HIST + j];
            x12[TP_TAPS - 1] = x[c];
            const uint32_t a = lim_detect(x12);
            d = a > d ? a : d;
        }
        const uint32_t q = lim_quot(C, d);
        uint32_t m = q;
        for (int j = 1; j < LIM_HOLD; j++) m = LIM_ONE - st.q_red[j] < m ? LIM_ONE - st.q_red[j] : m;
        const uint32_t up = LIM_ONE - st.r_red[LIM_SMOOTH - 1] + R;     // at most 2^24 + 2^20
        const uint32_t r = m < up ? m : up;
        uint32_t sum = r;
        for (int j = 1; j < LIM_SMOOTH; j++) sum += LIM_ONE - st.r_red[j];
        const uint32_t g = sum >> 6;
        int16_t *z = out + i * (uint64_t)channels;
        for (int c = 0; c < channels; c++) {
            const int16_t now = x[c];                   // read before z[c] is written: in place
            z[c] = (int16_t)lim_apply(st.hist[c][LIM_HIST - LIM_DELAY], g);
            memmove(&st.hist[c][0], &st.hist[c][1], (LIM_HIST - 1) * sizeof(int16_t));
            st.hist[c][LIM_HIST - 1] = now;
        }
        memmove(&st.q_red[0], &st.q_red[1], (LIM_HOLD - 1) * sizeof(uint32_t));
        st.q_red[LIM_HOLD - 1] = LIM_ONE - q;
        memmove(&st.r_red[0], &st.r_red[1], (LIM_SMOOTH - 1) * sizeof(uint32_t));
        st.r_red[LIM_SMOOTH - 1] = LIM_ONE - r;
        st.reduced += g < LIM_ONE ? 1 : 0;
        st.max_detect = d > st.max_detect ? d : st.max_detect;
        st.max_reduction = LIM_ONE - g > st.max_reduction ? LIM_ONE - g : st.max_reduction;
    }
    st.samples += n_new;
    memcpy(h_state, &st, sizeof st);
}

}  // namespace ac3mi
