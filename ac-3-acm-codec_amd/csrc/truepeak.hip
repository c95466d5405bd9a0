// truepeak.hip — true peak after ITU-R BS.1770-4 Annex 2, sample peak and full-scale count of s16 PCM in device memory
// (ac3mi_truepeak_*; the rule is include/ac3mi.h's, its steps and the state's layout are truepeak_rule.h's).
//
// truepeak_kernel: one wavefront per stream, four per workgroup, the stream's frames in order; int32 throughout.  A frame is
// 64 segments of 24 sample instants, one per lane:
//   load        lane l's 24 instants are 48 channels contiguous bytes: 16-byte loads when the base is 16-byte aligned, else
//               16-bit loads into the same registers (same bits either way)
//   history     per measured slot the 11 instants before a lane's segment come from the left neighbour's registers, one lane
//               shift per dword; lane 0 takes them from the 12 instants carried from the frame before (whole dwords for
//               every channel count, wave-uniform: lane 63's last 6 channels dwords, or at a call's first frame rebuilt
//               from the state's 11 samples per slot).  No sample is read twice from memory
//   phases      the lane packs the slot's 35 samples into the 34 pairs of neighbours (v_perm_b32) and forms the 4 x 24
//               phases with six packed 16-bit dot products each (v_dot2_i32_i16: tp_phases' sums, the same int32), keeping
//               the largest |y| with its first index in the frame, the largest |x| and the full-scale count
//   combine     behind the last frame a butterfly with the rule's ordering (tp_before) gives every lane the call's maxima and
//               sums; lane 0 merges them into the state - strictly greater replaces - with plain stores
// The PCM is read once; nothing waits on another wavefront; every loop is bounded by the frame count or a constant; no LDS,
// no atomics.
//
// truepeak_read_kernel: one stream per lane (tp_result, the code ac3mi_truepeak_read runs).
#include "truepeak_rule.h"

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
    if (channels < 1 || channels > 6 || !role || !h_pcm || ((uintptr_t)h_pcm & 1) || frames < 1 || !h_state) return AC3MI_ERR_ARG;
    ac3mi::truepeak_meter_host(channels, role, h_pcm, frames, h_state);
    return AC3MI_OK;
}

#ifdef __HIPCC__
#include "ac3mi_internal.h"
#include "truepeak_packed.h"

namespace ac3mi {

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

// One slot of one frame in one lane.  own = the lane's 24 instants as dwords [24][NCH]; carry = the 12 instants before the
// frame, as dwords [12][NCH], the same in every lane.  The 11 instants before the segment come from the left neighbour's
// registers, one lane shift each (the dword that holds the sample; lane 0: the carried one)
template <int NCH, int C>
__device__ __forceinline__ void tp_slot(const uint32_t *own, const uint32_t *carry, uint32_t lane, uint32_t f, TpLane &L)
{
    constexpr int HW = 6 * NCH;
    uint32_t h[TP_HIST];                // the dwords with instants -11 .. -1 of this slot
#pragma unroll
    for (int j = 0; j < TP_HIST; j++) {
        const int k = ((j + 1) * NCH + C) >> 1;
        const uint32_t left = __shfl_up(own[HW + k], 1u);
        h[j] = lane == 0 ? carry[k] : left;
    }
    uint32_t q[TP_HIST + TP_SEG - 1];   // the pairs of instants (-11, -10) .. (22, 23)
#pragma unroll
    for (int j = 0; j < TP_HIST + TP_SEG - 1; j++) {
        const int a = (j + 1) * NCH + C, b = a + NCH;       // (in dwords that start 12 instants before the segment)
        const uint32_t wa = j < TP_HIST ? h[j] : own[(a >> 1) - HW], wb = j + 1 < TP_HIST ? h[j + 1] : own[(b >> 1) - HW];
        q[j] = tp_pack(wa, a & 1, wb, b & 1);
    }
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
        const uint32_t ax = tp_abs(tp_sample<NCH>(own, i, C));
        pk = ax > pk ? ax : pk;
    }
    if (pk >= 32767u) {
#pragma unroll
        for (int i = 0; i < TP_SEG; i++) fs += tp_full_scale(tp_sample<NCH>(own, i, C)) ? 1u : 0u;
    }
    const uint32_t m = key >> 2, at = 4 * inst + (3u - (key & 3u));
    const bool take = m > L.best;       // frames in order: only a strictly greater value replaces the lane's
    L.best = take ? m : L.best;
    L.best_at = take ? (uint32_t)(4 * TP_SEG) * lane + at : L.best_at;
    L.best_frame = take ? f : L.best_frame;
    L.peak = pk > L.peak ? pk : L.peak;
    L.full += fs;
}

// ... every measured slot (written as a recursion: the slot is a compile-time constant, so the dwords stay in registers)
template <int NCH, int C>
__device__ __forceinline__ void tp_slots(const uint8_t *role, const uint32_t *own, const uint32_t *carry, uint32_t lane, uint32_t f, TpLane *acc)
{
    if constexpr (C < NCH) {
        if (role[C] != 0) tp_slot<NCH, C>(own, carry, lane, f, acc[C]);
        tp_slots<NCH, C + 1>(role, own, carry, lane, f, acc);
    }
}

template <int NCH, bool VEC>
__global__ __launch_bounds__(64 * TP_WAVES, TP_MIN_WAVES) void truepeak_kernel(const TruePeakParams P)
{
    constexpr int HW = 6 * NCH;         // dwords of 12 instants
    const int lane = threadIdx.x & 63;
    const unsigned s = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * TP_WAVES + (threadIdx.x >> 6)));
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
        if constexpr (VEC) {
            const uint4 *v = reinterpret_cast<const uint4 *>(fp);
#pragma unroll
            for (int k = 0; k < 3 * NCH; k++) {
                const uint4 t = v[k];
                w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w;
            }
        } else {
            const uint16_t *h = reinterpret_cast<const uint16_t *>(fp);
#pragma unroll
            for (int k = 0; k < 12 * NCH; k++) w[k] = (uint32_t)h[2 * k] | ((uint32_t)h[2 * k + 1] << 16);
        }
        tp_slots<NCH, 0>(P.role, w, carry, (uint32_t)lane, (uint32_t)f, acc);
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
            for (int j = 0; j < TP_HIST; j++) st->hist[c][j] = (int16_t)tp_sample<NCH>(carry, j + 1, c);
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

template <int NCH>
static void tp_launch_nch(const TruePeakParams &P, bool vec, hipStream_t stream)
{
    const dim3 grid((P.n_streams + TP_WAVES - 1) / TP_WAVES), block(64 * TP_WAVES);
    if (vec) hipLaunchKernelGGL((truepeak_kernel<NCH, true>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((truepeak_kernel<NCH, false>), grid, block, 0, stream, P);
}

hipError_t launch_truepeak(const TruePeakLaunch &L, hipStream_t stream)
{
    if (L.channels < 1 || L.channels > 6 || L.frames_per_stream < 1 || !L.pcm || !L.state) return hipErrorInvalidValue;
    if (L.n_streams <= 0) return hipSuccess;
    TruePeakParams P;
    P.pcm = L.pcm;
    P.state = (TruePeakState *)L.state;
    P.n_streams = (unsigned)L.n_streams;
    P.frames = L.frames_per_stream;
    for (int c = 0; c < 8; c++) P.role[c] = c < L.channels ? L.role[c] : 0;
    const bool vec = ((uintptr_t)L.pcm & 15) == 0;      // every frame and every lane's segment then is: 3072 and 48 channels bytes apart
    switch (L.channels) {
    case 1: tp_launch_nch<1>(P, vec, stream); break;
    case 2: tp_launch_nch<2>(P, vec, stream); break;
    case 3: tp_launch_nch<3>(P, vec, stream); break;
    case 4: tp_launch_nch<4>(P, vec, stream); break;
    case 5: tp_launch_nch<5>(P, vec, stream); break;
    default: tp_launch_nch<6>(P, vec, stream); break;
    }
    return hipGetLastError();
}

hipError_t launch_truepeak_read(const void *state, int n_streams, uint32_t ceiling_q28, ac3mi_truepeak_result *results, hipStream_t stream)
{
    if (n_streams <= 0) return hipSuccess;
    hipLaunchKernelGGL(truepeak_read_kernel, dim3(((unsigned)n_streams + 255) / 256), dim3(256), 0, stream, (const TruePeakState *)state,
                       (unsigned)n_streams, ceiling_q28, results);
    return hipGetLastError();
}

}  // namespace ac3mi
#endif  // __HIPCC__
