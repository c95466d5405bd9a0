// truepeak.hip — true peak after ITU-R BS.1770-4 Annex 2, sample peak and full-scale count of s16 PCM in device memory
// (ac3mi_truepeak_*; the rule is include/ac3mi.h's, its steps and the state's layout are truepeak_rule.h's).
//
// truepeak_kernel: one wavefront per stream, four per workgroup, the stream's frames in order; int32 throughout.  A frame is
// 64 segments of 24 sample instants, one per lane (pcm_lanes.h):
//   load        pcm_load_segment
//   history     tp_pairs (truepeak_packed.h), per measured slot; the 12 instants it takes as carried are whole dwords for every
//               channel count, wave-uniform: lane 63's last 6 channels dwords, or at a call's first frame rebuilt from the
//               state's 11 samples per slot
//   phases      from the slot's 34 pairs the 4 x 24 phases with six packed 16-bit dot products each (v_dot2_i32_i16:
//               tp_phases' sums, the same int32), keeping the largest |y| with its first index in the frame, the largest |x|
//               and the full-scale count
//   combine     behind the last frame a butterfly with the rule's ordering (tp_before) gives every lane the call's maxima and
//               sums; lane 0 merges them into the state - strictly greater replaces - with plain stores
// The PCM is read once; nothing waits on another wavefront; every loop is bounded by the frame count or a constant; no LDS,
// no atomics.
//
// truepeak_read_kernel: one stream per lane (tp_result, the code ac3mi_truepeak_read runs).
#include "truepeak_rule.h"

namespace ac3mi {
// what the host meter and the device meter refuse alike of one call's shape (the roles apart: a pointer in both entries)
static inline bool truepeak_call_ok(int channels, const void *pcm, int frames, const void *state)
{
    return channels >= 1 && channels <= 6 && pcm && !((uintptr_t)pcm & 1) && frames >= 1 && state;
}
}  // namespace ac3mi

extern "C" size_t ac3mi_truepeak_state_bytes(void) { return sizeof(ac3mi::TruePeakState); }

extern "C" int ac3mi_truepeak_tables(int16_t *h48)
{
    if (!h48) return AC3MI_ERR_ARG;
    ac3mi::truepeak_tables_host(h48);
    return AC3MI_OK;
}

extern "C" uint32_t ac3mi_truepeak_ceiling(double dbtp) { return ac3mi::truepeak_ceiling_host(dbtp); }

extern "C" int ac3mi_truepeak_read(const void *h_state, uint32_t ceiling_q28, ac3mi_truepeak_result *out)
{
    if (!h_state || !out) return AC3MI_ERR_ARG;
    ac3mi::truepeak_read_host(h_state, ceiling_q28, out);
    return AC3MI_OK;
}

extern "C" int ac3mi_truepeak_host(int channels, const uint8_t *role, const int16_t *h_pcm, int frames, void *h_state)
{
    if (!role || !ac3mi::truepeak_call_ok(channels, h_pcm, frames, h_state)) return AC3MI_ERR_ARG;
    ac3mi::truepeak_meter_host(channels, role, h_pcm, frames, h_state);
    return AC3MI_OK;
}

#ifdef __HIPCC__
#include "ac3mi_internal.h"
#include "truepeak_packed.h"

namespace ac3mi {

bool truepeak_args_ok(const TruePeakLaunch &L)
{
    return truepeak_call_ok(L.channels, L.pcm, L.frames_per_stream, L.state) && L.n_streams >= 0 && !((uintptr_t)L.state & 7);
}

constexpr int TP_WAVES = 4;
// wavefronts per SIMD the meter kernel is compiled for.  The six-channel variant holds a frame's 72 dwords, 30 registers of
// per-slot maxima and a slot's 11 + 34 dwords of history and pairs.  Measured on 65 536 one-frame 5.1 streams with the
// multiply-add form of the phases: 2 (172 B of scratch) 1.39 ms, 3 (168 VGPRs, 532 B of scratch) 2.01 ms
constexpr int TP_MIN_WAVES = 2;

struct TruePeakParams {
    const int16_t *pcm;
    TruePeakState *state;
    unsigned n_streams;
    int frames;
    uint8_t role[8];
};

// what a lane keeps per slot over a call
struct TpLane {
    uint32_t best, best_at, best_frame; // the largest |y|, its first index in its frame, the frame
    uint32_t peak, full;                // the largest |x|; the full-scale samples (24 a frame: a u32 holds more frames than device memory)
};

// One slot of one frame in one lane (own, carry: tp_pairs')
template <int NCH, int C>
__device__ __forceinline__ void tp_slot(const uint32_t *own, const uint32_t *carry, uint32_t lane, uint32_t f, TpLane &L)
{
    uint32_t q[TP_HIST + TP_SEG - 1];
    tp_pairs<NCH, C>(own, carry, (int)lane, q);
    // |y| < 2^30 (truepeak_rule.h), so key = |y| << 2 | (3 - p) orders an instant's four phases by the rule - the larger value,
    // then the earlier phase - in one maximum; across instants only a strictly greater |y| replaces: key > (kept | 3)
    uint32_t key = 0, inst = 0, pk = 0, fs = 0;
#pragma unroll
    for (int i = 0; i < TP_SEG; i++) {
        int32_t y[TP_PHASES];
        tp_phases_packed(q + i, y);
        uint32_t k4 = 0;
#pragma unroll
        for (int p = 0; p < TP_PHASES; p++) {
            const uint32_t k = (tp_abs(y[p]) << 2) | (uint32_t)(3 - p);
            k4 = k > k4 ? k : k4;
        }
        const bool later = k4 > (key | 3u);
        inst = later ? (uint32_t)i : inst;
        key = later ? k4 : key;
        const uint32_t ax = tp_abs(pcm_sample<NCH>(own, i, C));
        pk = ax > pk ? ax : pk;
    }
    if (pk >= 32767u) {
#pragma unroll
        for (int i = 0; i < TP_SEG; i++) fs += tp_full_scale(pcm_sample<NCH>(own, i, C)) ? 1u : 0u;
    }
    const uint32_t m = key >> 2, at = 4 * inst + (3u - (key & 3u));
    const bool take = m > L.best;       // frames in order: only a strictly greater value replaces the lane's
    L.best = take ? m : L.best;
    L.best_at = take ? (uint32_t)(4 * TP_SEG) * lane + at : L.best_at;
    L.best_frame = take ? f : L.best_frame;
    L.peak = pk > L.peak ? pk : L.peak;
    L.full += fs;
}

template <int NCH, bool VEC>
__global__ __launch_bounds__(64 * TP_WAVES, TP_MIN_WAVES) void truepeak_kernel(const TruePeakParams P)
{
    constexpr int HW = 6 * NCH;         // dwords of 12 instants
    const int lane = threadIdx.x & 63;
    const unsigned s = pcm_wave_stream(TP_WAVES);
    if (s >= P.n_streams) return;
    TruePeakState *st = P.state + s;
    // the 12 instants before the frame, as dwords [12][NCH] (the same in every lane); instant 0 of them is never read
    uint32_t carry[HW];
#pragma unroll
    for (int k = 0; k < HW; k++) {
        uint32_t half[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int j = (2 * k + h) / NCH, c = (2 * k + h) % NCH;     // instant and slot of this int16
            half[h] = j >= 1 && P.role[c] != 0 ? (uint32_t)(uint16_t)st->hist[c][j - 1] : 0u;
        }
        carry[k] = half[0] | (half[1] << 16);
    }
    TpLane acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) acc[c] = TpLane{0, 0, 0, 0, 0};
    const int16_t *sp = P.pcm + (size_t)s * (size_t)P.frames * (1536 * NCH) + lane * (TP_SEG * NCH);

    for (int f = 0; f < P.frames; f++) {
        const int16_t *fp = sp + (size_t)f * (1536 * NCH);
        uint32_t w[12 * NCH];           // the lane's 24 NCH samples, two to a dword
        pcm_load_segment<NCH, VEC>(fp, w);
        pcm_for_each_slot<NCH>(P.role, [&](auto c) __attribute__((always_inline)) {
            tp_slot<NCH, decltype(c)::value>(w, carry, (uint32_t)lane, (uint32_t)f, acc[decltype(c)::value]);
        });
#pragma unroll
        for (int k = 0; k < HW; k++) carry[k] = (uint32_t)__builtin_amdgcn_readlane((int)w[HW + k], 63);
    }

    const uint64_t before = st->samples;
    uint8_t measured = st->measured;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        if (P.role[c] == 0) continue;
        uint32_t b = acc[c].best, pk = acc[c].peak;
        uint64_t at = (uint64_t)acc[c].best_frame * 6144u + acc[c].best_at, n = acc[c].full;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t b2 = __shfl_xor(b, o), pk2 = __shfl_xor(pk, o);
            const uint64_t at2 = __shfl_xor(at, o);
            n += __shfl_xor(n, o);
            const bool other = tp_before(b2, at2, b, at);
            b = other ? b2 : b;
            at = other ? at2 : at;
            pk = pk2 > pk ? pk2 : pk;
        }
        if (lane == 0) {
            if (b > st->true_peak[c]) {
                st->true_peak[c] = b;
                st->index[c] = 4 * before + at;
            }
            if (pk > st->sample_peak[c]) st->sample_peak[c] = pk;
            st->full_scale[c] = tp_add_sat(st->full_scale[c], n);
#pragma unroll
            for (int j = 0; j < TP_HIST; j++) st->hist[c][j] = (int16_t)pcm_sample<NCH>(carry, j + 1, c);
        }
        measured |= (uint8_t)(1u << c);
    }
    if (lane == 0) {
        st->samples = before + (uint64_t)P.frames * 1536u;
        st->measured = measured;
    }
}

__global__ __launch_bounds__(256) void truepeak_read_kernel(const TruePeakState *state, unsigned n_streams, uint32_t ceiling_q28,
                                                            ac3mi_truepeak_result *results)
{
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_streams) return;
    tp_result(state + s, ceiling_q28, results + s);
}

hipError_t launch_truepeak(const TruePeakLaunch &L, hipStream_t stream)
{
    if (!truepeak_args_ok(L)) return hipErrorInvalidValue;
    TruePeakParams P;
    P.pcm = L.pcm;
    P.state = (TruePeakState *)L.state;
    P.n_streams = (unsigned)L.n_streams;
    P.frames = L.frames_per_stream;
    pcm_copy_roles(P.role, L.role, L.channels);
    const bool vec = ((uintptr_t)L.pcm & 15) == 0;
    hipError_t e = hipSuccess;
    pcm_dispatch_channels(L.channels, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        e = pcm_launch_streams(vec ? truepeak_kernel<NCH, true> : truepeak_kernel<NCH, false>, L.n_streams, TP_WAVES, 64 * TP_WAVES, stream, P);
    });
    return e;
}

hipError_t launch_truepeak_read(const void *state, int n_streams, uint32_t ceiling_q28, ac3mi_truepeak_result *results, hipStream_t stream)
{
    return pcm_launch_streams(truepeak_read_kernel, n_streams, 256, 256, stream, (const TruePeakState *)state, (unsigned)n_streams, ceiling_q28,
                              results);
}

}  // namespace ac3mi
#endif  // __HIPCC__
