// limit.hip — the look-ahead true-peak limiter of s16 PCM in device memory (ac3mi_limit_*; the rule is include/ac3mi.h's, its
// steps and the state's layout are limit_rule.h's, the interpolator truepeak_rule.h's).
//
// limit_kernel: one wavefront per stream, four per workgroup, the stream's frames in order; integers throughout.  A frame is 64
// segments of 24 sample instants, one per lane (pcm_lanes.h), as in truepeak_kernel:
//   load        pcm_load_segment, the 16-byte form when both bases are 16-byte aligned
//   detect      per detected slot tp_pairs and the four phases by packed 16-bit dot products (truepeak_packed.h); d[n] also
//               takes the two samples beside the phases, which are the halves of one of the pairs
//   q           d goes to the wavefront's q line in LDS (1536 entries behind the 79 carried ones); one loop that is not
//               unrolled replaces each by lim_quot - a single copy of the 64-bit division, which runs only where d > C
//   m           a lane-local pass over its 24 + 79 entries: the 57 that all its windows share, then suffix and prefix minima
//   r           the min-plus scan: a lane folds its 24 instants into an exit value, wave_incl_scan_min runs on
//               value - position * R (an int32 given R <= 2^20, limit_rule.h), the left neighbour's exit is the lane's entry
//   g           r goes to the r line (1536 behind the 63 carried); a sliding sum over 64 + 23 entries
//   apply       the delayed samples x[n - 77] are lanes l - 4 and l - 3's registers, one lane shift per dword (lanes 0..3:
//               the dwords lanes 60..63 left in LDS the frame before); lim_apply; pcm_store_segment: the lane stores the 24
//               instants it loaded, so an in-place call never reads what it has overwritten
// Both lines are padded by one entry in 24 (entry j at j + j / 24): lane l's entries start at 25 l, and a pass in which every
// lane reads its k-th entry meets no bank twice.  Nothing waits on another wavefront; every loop is bounded by the frame count
// or a constant; no atomics; plain vector stores.
//
// limit_read_kernel: one stream per lane (lim_result, the code ac3mi_limit_read runs).
#include "limit_rule.h"

namespace ac3mi {
// d_out may be exactly d_pcm or must not overlap it at all
static inline bool limit_buffers_ok(const void *pcm, const void *out, uint64_t bytes)
{
    const uintptr_t a = (uintptr_t)pcm, b = (uintptr_t)out;
    return a && b && !(a & 1) && !(b & 1) && (a == b || a + bytes <= b || b + bytes <= a);
}
}  // namespace ac3mi

extern "C" size_t ac3mi_limit_state_bytes(void) { return sizeof(ac3mi::LimitState); }

extern "C" uint32_t ac3mi_limit_release_step(int sample_rate, double full_recovery_ms)
{
    return ac3mi::limit_release_step_host(sample_rate, full_recovery_ms);
}

extern "C" int ac3mi_limit_read(const void *h_state, ac3mi_limit_result *out)
{
    if (!h_state || !out) return AC3MI_ERR_ARG;
    ac3mi::limit_read_host(h_state, out);
    return AC3MI_OK;
}

extern "C" int ac3mi_limit_host(int channels, const uint8_t *role, uint32_t ceiling_q28, uint32_t release_step_q24, const int16_t *h_pcm,
                                int16_t *h_out, int frames, void *h_state)
{
    if (!ac3mi::limit_params_ok(channels, ceiling_q28, release_step_q24, frames) || !role || !h_state ||
        !ac3mi::limit_buffers_ok(h_pcm, h_out, (uint64_t)frames * 3072u * (uint64_t)channels))
        return AC3MI_ERR_ARG;
    ac3mi::limit_host(channels, role, ceiling_q28, release_step_q24, h_pcm, h_out, frames, h_state);
    return AC3MI_OK;
}

#ifdef __HIPCC__
#include "ac3mi_internal.h"
#include "truepeak_packed.h"
#include "wave_ops.h"

namespace ac3mi {

bool limit_args_ok(const LimitLaunch &L)
{
    return limit_params_ok(L.channels, L.ceiling_q28, L.release_step_q24, L.frames_per_stream) && L.n_streams >= 0 && L.state &&
           !((uintptr_t)L.state & 7) &&
           limit_buffers_ok(L.pcm, L.out, (uint64_t)L.n_streams * (uint64_t)L.frames_per_stream * 3072u * (uint64_t)L.channels);
}

constexpr int LIM_WAVES = 4;
// wavefronts per SIMD the kernel is compiled for.  Measured on 65 536 one-frame 5.1 streams: 2 (256 VGPRs, 336 B of scratch in
// the six-channel variant) 1.607 ms, 1 (no scratch, 73 AGPRs) 1.669 ms
constexpr int LIM_MIN_WAVES = 2;

// a line's entry j lies at j + j / 24; lane l's k-th entry (entry 24 l + k) at 25 l + lim_pos(k)
__host__ __device__ constexpr int lim_pos(int j) { return j + j / 24; }
constexpr int LIM_Q_CARRY = LIM_HOLD - 1, LIM_R_CARRY = LIM_SMOOTH - 1;
constexpr int LIM_Q_WORDS = lim_pos(LIM_Q_CARRY + 1536 - 1) + 1, LIM_R_WORDS = lim_pos(LIM_R_CARRY + 1536 - 1) + 1;
static_assert(25 * 63 + lim_pos(LIM_Q_CARRY + TP_SEG - 1) == LIM_Q_WORDS - 1 && 25 * 63 + lim_pos(LIM_R_CARRY + TP_SEG - 1) == LIM_R_WORDS - 1,
              "lane 63's last entry is the line's last");

struct LimitParams {
    const int16_t *pcm;
    int16_t *out;
    LimitState *state;
    unsigned n_streams;
    int frames;
    uint32_t ceiling, step;
    uint8_t role[8];
};

// One detected slot of one frame in one lane: d[i] takes the slot's share (lim_detect's value, from packed pairs).  own, carry:
// tp_pairs', the carried dwords in LDS
template <int NCH, int C>
__device__ __forceinline__ void lim_slot(const uint32_t *own, const uint32_t *carry, int lane, uint32_t *d)
{
    uint32_t q[TP_HIST + TP_SEG - 1];
    tp_pairs<NCH, C>(own, carry, lane, q);
#pragma unroll
    for (int i = 0; i < TP_SEG; i++) {
        int32_t y[TP_PHASES];
        tp_phases_packed(q + i, y);
        const uint32_t pr = q[i + 5];   // (x[i - 6], x[i - 5])
        uint32_t a = tp_abs((int32_t)(int16_t)(pr & 0xffffu)), b = tp_abs((int32_t)(int16_t)(pr >> 16));
        a = (b > a ? b : a) << 13;
#pragma unroll
        for (int p = 0; p < TP_PHASES; p++) a = tp_abs(y[p]) > a ? tp_abs(y[p]) : a;
        d[i] = a > d[i] ? a : d[i];
    }
}

// dword j of the lane K to the left; for lanes 0 .. K - 1 of lanes 64 - K .. 63 of the frame before (kept [4][12 NCH])
template <int NCH, int K>
__device__ __forceinline__ uint32_t lim_from_left(uint32_t v, const uint32_t *kept, int lane, int j)
{
    const uint32_t t = __shfl_up(v, (unsigned)K);
    const uint32_t c = kept[((lane < K ? lane : 0) + 4 - K) * (12 * NCH) + j];
    return lane < K ? c : t;
}

template <int NCH, bool VEC>
__global__ __launch_bounds__(64 * LIM_WAVES, LIM_MIN_WAVES) void limit_kernel(const LimitParams P)
{
    constexpr int HW = 6 * NCH, NW = 12 * NCH;      // dwords of 12 instants, of a lane's 24
    __shared__ uint32_t s_q[LIM_WAVES][LIM_Q_WORDS], s_r[LIM_WAVES][LIM_R_WORDS], s_kept[LIM_WAVES][4 * NW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned s = pcm_wave_stream(LIM_WAVES);
    if (s >= P.n_streams) return;
    uint32_t *lq = s_q[wv], *lr = s_r[wv], *kept = s_kept[wv];
    LimitState *st = P.state + s;
    const int B = 25 * lane;
    const uint32_t C = P.ceiling;
    const int R = (int)P.step;

    // the carried entries: q of the 79 instants before the call, r of the 63, and the dwords of the last 96 instants as
    // lanes 60..63 would have left them (the state holds 80 of them; the first 16 are never read)
    for (int j = lane; j < LIM_Q_CARRY; j += 64) lq[lim_pos(j)] = LIM_ONE - st->q_red[j + 1];
    if (lane < LIM_R_CARRY) lr[lim_pos(lane)] = LIM_ONE - st->r_red[lane + 1];
    for (int k = lane; k < 4 * NW; k += 64) {
        uint32_t half[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int t = (2 * k + h) / NCH, c = (2 * k + h) % NCH;
            half[h] = t >= 96 - LIM_HIST ? (uint32_t)(uint16_t)st->hist[c][t - (96 - LIM_HIST)] : 0u;
        }
        kept[k] = half[0] | (half[1] << 16);
    }
    wave_sync();

    uint32_t n_red = 0, d_max = 0, g_min = LIM_ONE;
    uint32_t w[NW];                     // the lane's 24 NCH samples, two to a dword
    const size_t at = (size_t)s * (size_t)P.frames * (1536 * NCH) + lane * (TP_SEG * NCH);
    for (int f = 0; f < P.frames; f++) {
        const int16_t *fp = P.pcm + at + (size_t)f * (1536 * NCH);
        pcm_load_segment<NCH, VEC>(fp, w);

        // d, then q in place in the line
        {
            uint32_t d[TP_SEG];
#pragma unroll
            for (int i = 0; i < TP_SEG; i++) d[i] = 0;
            pcm_for_each_slot<NCH>(P.role, [&](auto c) __attribute__((always_inline)) {
                lim_slot<NCH, decltype(c)::value>(w, kept + 3 * NW + HW, lane, d);
            });
#pragma unroll
            for (int i = 0; i < TP_SEG; i++) {
                lq[B + lim_pos(LIM_Q_CARRY + i)] = d[i];
                d_max = d[i] > d_max ? d[i] : d_max;
            }
        }
#pragma unroll 1
        for (int i = 0; i < TP_SEG; i++) {
            const int k = B + lim_pos(LIM_Q_CARRY + i);
            lq[k] = lim_quot(C, lq[k]);
        }
        wave_sync();

        // m: the window of instant i is the lane's entries i .. i + 79
        int m[TP_SEG];
        {
            uint32_t core = lq[B + lim_pos(TP_SEG - 1)];
#pragma unroll
            for (int k = TP_SEG; k < LIM_HOLD; k++) {
                const uint32_t v = lq[B + lim_pos(k)];
                core = v < core ? v : core;
            }
            m[TP_SEG - 1] = (int)core;
#pragma unroll
            for (int i = TP_SEG - 2; i >= 0; i--) {
                const int v = (int)lq[B + lim_pos(i)];
                m[i] = v < m[i + 1] ? v : m[i + 1];
            }
            int pfx = (int)lq[B + lim_pos(LIM_HOLD)];
#pragma unroll
            for (int i = 1; i < TP_SEG; i++) {
                m[i] = pfx < m[i] ? pfx : m[i];
                if (i + 1 < TP_SEG) {
                    const int v = (int)lq[B + lim_pos(LIM_HOLD + i)];
                    pfx = v < pfx ? v : pfx;
                }
            }
        }

        // r = min(m, r[-1] + R) as a min-plus scan (m becomes the lane-local a, then r)
        const int r_prev = (int)lr[lim_pos(LIM_R_CARRY - 1)];
#pragma unroll
        for (int i = 1; i < TP_SEG; i++) m[i] = m[i] < m[i - 1] + R ? m[i] : m[i - 1] + R;
        const int ramp = TP_SEG * (lane + 1) * R;
        const int pm = wave_incl_scan_min(m[TP_SEG - 1] - ramp);
        const int exit_r = (pm < r_prev ? pm : r_prev) + ramp;
        const int left_r = __shfl_up(exit_r, 1u);
        const int entry = lane == 0 ? r_prev : left_r;
#pragma unroll
        for (int i = 0; i < TP_SEG; i++) {
            const int up = entry + (i + 1) * R;
            m[i] = m[i] < up ? m[i] : up;
            lr[B + lim_pos(LIM_R_CARRY + i)] = (uint32_t)m[i];
        }
        wave_sync();

        // g: the window of instant i is the lane's entries i .. i + 63 of the r line
        uint32_t g[TP_SEG];
        {
            uint32_t sum = 0;
#pragma unroll
            for (int k = 0; k < LIM_SMOOTH; k++) sum += lr[B + lim_pos(k)];
            g[0] = sum >> 6;
#pragma unroll
            for (int i = 1; i < TP_SEG; i++) {
                sum += (uint32_t)m[i] - lr[B + lim_pos(i - 1)];
                g[i] = sum >> 6;
            }
#pragma unroll
            for (int i = 0; i < TP_SEG; i++) {
                n_red += g[i] < LIM_ONE ? 1u : 0u;
                g_min = g[i] < g_min ? g[i] : g_min;
            }
        }

        // the delayed samples: the lane's element e (int16, [24][NCH]) is element e + 19 NCH of the lane four to the left for
        // e < 5 NCH, else element e - 5 NCH of the lane three to the left (77 = 3 * 24 + 5)
        uint32_t a4[NW], a3[NW];
#pragma unroll
        for (int j = 0; j < NW; j++) {
            a4[j] = j >= (19 * NCH) / 2 ? lim_from_left<NCH, 4>(w[j], kept, lane, j) : 0u;
            a3[j] = j <= (19 * NCH - 1) / 2 ? lim_from_left<NCH, 3>(w[j], kept, lane, j) : 0u;
        }
        uint32_t z[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) {
            uint32_t half[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int e = 2 * k + h;
                const int src = e < 5 * NCH ? e + 19 * NCH : e - 5 * NCH;
                const uint32_t dw = e < 5 * NCH ? a4[src >> 1] : a3[src >> 1];
                const int32_t x = (int32_t)(int16_t)(dw >> (16 * (src & 1)));
                half[h] = (uint32_t)lim_apply(x, g[e / NCH]) & 0xffffu;
            }
            z[k] = half[0] | (half[1] << 16);
        }
        pcm_store_segment<NCH, VEC>(P.out + at + (size_t)f * (1536 * NCH), z);

        // hand over: the lines' last 79 and 63 entries become the carried ones, lanes 60..63 leave their dwords
        const uint32_t q0 = lq[lim_pos(1536 + lane)], q1 = lane < LIM_Q_CARRY - 64 ? lq[lim_pos(1536 + 64 + lane)] : 0u;
        const uint32_t r0 = lane < LIM_R_CARRY ? lr[lim_pos(1536 + lane)] : 0u;
        wave_sync();
        lq[lim_pos(lane)] = q0;
        if (lane < LIM_Q_CARRY - 64) lq[lim_pos(64 + lane)] = q1;
        if (lane < LIM_R_CARRY) lr[lim_pos(lane)] = r0;
        if (lane >= 60) {
#pragma unroll
            for (int j = 0; j < NW; j++) kept[(lane - 60) * NW + j] = w[j];
        }
        wave_sync();
    }

    // the state: the lines still hold the last frame's entries behind the carried ones
    for (int j = lane; j < LIM_HOLD; j += 64) st->q_red[j] = LIM_ONE - lq[lim_pos(LIM_Q_CARRY + 1536 - LIM_HOLD + j)];
    st->r_red[lane] = LIM_ONE - lr[lim_pos(LIM_R_CARRY + 1536 - LIM_SMOOTH + lane)];
    if (lane >= 60) {
#pragma unroll
        for (int i = 0; i < TP_SEG; i++) {
            const int j = TP_SEG * (lane - 60) + i - (96 - LIM_HIST);
            if (j >= 0) {
#pragma unroll
                for (int c = 0; c < NCH; c++) st->hist[c][j] = (int16_t)pcm_sample<NCH>(w, i, c);
            }
        }
    }
    uint64_t n = n_red;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t d2 = __shfl_xor(d_max, o), g2 = __shfl_xor(g_min, o);
        n += __shfl_xor(n, o);
        d_max = d2 > d_max ? d2 : d_max;
        g_min = g2 < g_min ? g2 : g_min;
    }
    if (lane == 0) {
        st->samples += (uint64_t)P.frames * 1536u;
        st->reduced += n;
        if (d_max > st->max_detect) st->max_detect = d_max;
        if (LIM_ONE - g_min > st->max_reduction) st->max_reduction = LIM_ONE - g_min;
    }
}

__global__ __launch_bounds__(256) void limit_read_kernel(const LimitState *state, unsigned n_streams, ac3mi_limit_result *results)
{
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_streams) return;
    lim_result(state + s, results + s);
}

hipError_t launch_limit(const LimitLaunch &L, hipStream_t stream)
{
    if (!limit_args_ok(L)) return hipErrorInvalidValue;
    LimitParams P;
    P.pcm = L.pcm;
    P.out = L.out;
    P.state = (LimitState *)L.state;
    P.n_streams = (unsigned)L.n_streams;
    P.frames = L.frames_per_stream;
    P.ceiling = L.ceiling_q28;
    P.step = L.release_step_q24;
    pcm_copy_roles(P.role, L.role, L.channels);
    const bool vec = (((uintptr_t)L.pcm | (uintptr_t)L.out) & 15) == 0;
    hipError_t e = hipSuccess;
    pcm_dispatch_channels(L.channels, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        e = pcm_launch_streams(vec ? limit_kernel<NCH, true> : limit_kernel<NCH, false>, L.n_streams, LIM_WAVES, 64 * LIM_WAVES, stream, P);
    });
    return e;
}

hipError_t launch_limit_read(const void *state, int n_streams, ac3mi_limit_result *results, hipStream_t stream)
{
    return pcm_launch_streams(limit_read_kernel, n_streams, 256, 256, stream, (const LimitState *)state, (unsigned)n_streams, results);
}

}  // namespace ac3mi
#endif  // __HIPCC__
