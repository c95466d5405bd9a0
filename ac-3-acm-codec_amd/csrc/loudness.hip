// loudness.hip — programme loudness after ITU-R BS.1770-4 on s16 PCM in device memory and the dialnorm it implies
// (ac3mi_loudness_*; the rule is include/ac3mi.h's, its decisions and the state's layout are loudness_rule.h's).
//
// loudness_kernel: one wavefront per stream, four per workgroup, the stream's frames in order; float64 throughout (a float32
// recursion moves block energies by 1e-4 relative: the high-pass poles sit at radius 0.995).  A frame is 64 segments of 24
// sample instants, one per lane (pcm_lanes.h), and the two biquads are one linear system v' = A v + B x, y = C v + D x on four
// states:
//   load        pcm_load_segment
//   zero state  per measured slot the lane runs the cascade over its 24 samples from v = 0: 24 outputs and an end state
//   scan        the true end states follow from e[l] = A^24 e[l - 1] + (zero-state end of l): lane 0 adds A^24 (carried
//               state), then six steps e[l] += A^(24 2^k) e[l - 2^k] with the constant matrices from the kernel arguments
//   zero input  the lane's true start state (its left neighbour's end state; lane 0: the carried state) corrects the 24
//               outputs through the constant table C A^n
//   energy      w y^2 summed apart for the instants before and behind the frame's hop boundary (a frame holds at most one:
//               a hop is 3200 samples or more; at 44.1 and 32 kHz it falls inside a lane's segment), a butterfly gives
//               every lane the frame's two sums
//   state       the hop closes, the block forms and finds its bin (loud_bin) in every lane alike; lane 0 adds it to the bins
//               with plain loads and stores and, behind the last frame, writes the carried state back
// The PCM is read once; nothing waits on another wavefront; every loop is bounded by the frame count or a constant; no LDS.
// The fused multiply-adds are written out, so the result does not hang on the contraction setting.
//
// loudness_read_kernel: one wavefront per stream; lane l sums bins l, l + 64, ... (loud_total_part / loud_gated_part, the code
// the host twin runs with stride 1), butterflies combine them, lane 0 writes the record.
// loudness_words_kernel: one lane per frame.
//
// The loudness range meter (ac3mi_loudness_range_*, EBU Tech 3342) is loudness_kernel<.., RANGE = true>: where a hop closes, in
// the branch that is the same in every lane, lane 0 hands the hop's energy to range_push_hop (loudness_rule.h) - ring, ordered
// sum of 30, bin, counters, all in the range state in HBM with plain loads and stores; nothing of it is carried in registers
// across the frame's filter work, and the RANGE = false instantiations are the kernels they were.
// loudness_range_read_kernel: one wavefront per stream; lane l < 60 owns bins 15 l .. 15 l + 14 and reads them once, as what
// each adds to the blocks that pass the relative gate (range_counted); a prefix scan over the lanes gives each the blocks
// counted below its run, the lane whose run holds a rank finds its bin (range_bin_of_rank, the code the host twin runs over
// all 900), lane 0 writes the record.  Integer work once Gamma3 is fixed, and Gamma3 is one division of two values every lane
// reads alike: the record is the host twin's bit for bit.
#include "loudness_rule.h"

extern "C" size_t ac3mi_loudness_state_bytes(void) { return sizeof(ac3mi::LoudState); }

extern "C" int ac3mi_loudness_tables(int sample_rate, double *coef10, double *edges901, double *dialnorm30)
{
    const double *c = ac3mi::loud_coefs(sample_rate);
    if (!c) return AC3MI_ERR_ARG;
    if (coef10) memcpy(coef10, c, 10 * sizeof(double));
    if (edges901) ac3mi::loud_build_edges(edges901);
    if (dialnorm30) ac3mi::loud_build_dialnorm(dialnorm30);
    return AC3MI_OK;
}

extern "C" int ac3mi_loudness_read(const void *h_state, ac3mi_loudness_result *out)
{
    if (!h_state || !out) return AC3MI_ERR_ARG;
    ac3mi::loudness_read_host(h_state, out);
    return AC3MI_OK;
}

extern "C" size_t ac3mi_loudness_range_state_bytes(void) { return sizeof(ac3mi::RangeState); }

extern "C" int ac3mi_loudness_range_read(const void *h_range_state, ac3mi_loudness_range_result *out)
{
    if (!h_range_state || !out) return AC3MI_ERR_ARG;
    ac3mi::loudness_range_read_host(h_range_state, out);
    return AC3MI_OK;
}

#ifdef __HIPCC__
#include "ac3mi_internal.h"
#include "pcm_lanes.h"
#include "wave_ops.h"

// the roles of the slots the s16 converters write for these output flags (s16_channel_map, dropin.hip: slot -> plane; plane 0
// is the LFE when the flags carry it, the surround planes are the last one of 2F1R / 3F1R and the last two of 2F2R / 3F2R)
extern "C" int ac3mi_loudness_roles(int a52_flags, uint8_t role[6])
{
    if (!role) return AC3MI_ERR_ARG;
    int map[6];
    const int n = ac3mi::s16_channel_map(a52_flags, map);
    if (n <= 0) return AC3MI_ERR_ARG;
    const int cfg = a52_flags & 15, lfe = (a52_flags & 16) ? 1 : 0;
    const int n_sur = (cfg == 4 || cfg == 5) ? 1 : (cfg == 6 || cfg == 7) ? 2 : 0;
    for (int i = 0; i < 6; i++) role[i] = 0;
    for (int i = 0; i < n; i++) role[i] = (lfe && map[i] == 0) ? 0 : map[i] >= n - n_sur ? 2 : 1;
    return n;
}

namespace ac3mi {

static_assert(LOUD_SEG == PCM_SEG, "a lane's segment is the frame's");

// (a range state that is asked for and missing is the entry's to refuse: here nullptr means the plain meter)
bool loudness_args_ok(const LoudnessLaunch &L)
{
    bool ok = loud_coefs(L.sample_rate) && L.channels >= 1 && L.channels <= 6 && L.n_streams >= 0 && L.frames_per_stream >= 1 && L.pcm &&
              !((uintptr_t)L.pcm & 1) && L.state && !((uintptr_t)L.state & 7) && !((uintptr_t)L.range_state & 7);
    for (int c = 0; ok && c < L.channels; c++) ok = L.role[c] <= 2;
    return ok;
}

void loud_fill_tab(double *h_tab)
{
    loud_build_edges(h_tab);
    loud_build_dialnorm(h_tab + LOUD_BINS + 1);
}

constexpr int LOUD_WAVES = 4;
// wavefronts per SIMD the meter kernel is compiled for.  Measured on 65 536 one-frame 5.1 streams: 1 (255 VGPRs and more in
// AGPRs) 1.10 ms, 2 (36 B of scratch in the six-channel variant) 0.78 ms, 3 (168 VGPRs, 240 B of scratch) 0.86 ms
constexpr int LOUD_MIN_WAVES = 2;

struct LoudParams {
    const int16_t *pcm;
    LoudState *state;
    const double *edges;
    unsigned n_streams;
    int frames;
    uint32_t hop;
    uint8_t role[8];
    double w[6];                        // the slot's weight: 0, 1 or 1.41
    double b0, b1, b2, a1, a2, c1, c2;  // shelf b / 32768 (x = s / 32768 folded in: a power of two, so the same bits), a; high-pass a (its b is 1, -2, 1)
    double block_samples;               // 4 hop
    double M[6][16];                    // A^(24 2^k)
    double Z[LOUD_SEG][4];              // C A^n
    RangeState *range;                  // RANGE variants only (behind everything the others read: their arguments lie where they lay)
};

__device__ __forceinline__ double loud_readlane(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

template <int NCH, bool VEC, bool RANGE>
__global__ __launch_bounds__(64 * LOUD_WAVES, LOUD_MIN_WAVES) void loudness_kernel(const LoudParams P)
{
    const int lane = threadIdx.x & 63;
    const unsigned s = pcm_wave_stream(LOUD_WAVES);
    if (s >= P.n_streams) return;
    LoudState *st = P.state + s;
    double q[NCH][4];                   // the carried filter states, the same in every lane
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) q[c][r] = st->bq[c][r];
    double hop_sum = st->hop_sum, h0 = st->hops[0], h1 = st->hops[1], h2 = st->hops[2], max_block = st->max_block;
    uint32_t pos = st->pos, hop_count = st->hop_count, blocks = st->blocks, blocks_abs = st->blocks_abs;
    const int16_t *sp = P.pcm + (size_t)s * (size_t)P.frames * (1536 * NCH) + lane * (LOUD_SEG * NCH);

    for (int f = 0; f < P.frames; f++) {
        const int16_t *fp = sp + (size_t)f * (1536 * NCH);
        uint32_t w[12 * NCH];           // the lane's 24 NCH samples, two to a dword
        pcm_load_segment<NCH, VEC>(fp, w);
        // the hop closes behind sample nb - 1 of this frame if nb <= 1536 (a state that is not one: no boundary, nothing worse)
        const uint32_t nb = P.hop - pos;
        const int n0 = lane * LOUD_SEG;
        double e_before = 0.0, e_after = 0.0;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if (P.role[c] == 0) continue;
            double y[LOUD_SEG], s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int i = 0; i < LOUD_SEG; i++) {
                const double x = (double)pcm_sample<NCH>(w, i, c);
                const double y1 = __builtin_fma(P.b0, x, s1);
                s1 = __builtin_fma(-P.a1, y1, __builtin_fma(P.b1, x, s2));
                s2 = __builtin_fma(-P.a2, y1, P.b2 * x);
                const double yy = y1 + t1;
                t1 = __builtin_fma(-P.c1, yy, __builtin_fma(-2.0, y1, t2));
                t2 = __builtin_fma(-P.c2, yy, y1);
                y[i] = yy;
            }
            double e[4] = {s1, s2, t1, t2};
            {   // lane 0's segment starts from the carried state
                const double m = lane == 0 ? 1.0 : 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    double a = P.M[0][4 * r] * q[c][0];
#pragma unroll
                    for (int j = 1; j < 4; j++) a = __builtin_fma(P.M[0][4 * r + j], q[c][j], a);
                    e[r] = __builtin_fma(m, a, e[r]);
                }
            }
#pragma unroll
            for (int k = 0; k < 6; k++) {
                double u[4];
#pragma unroll
                for (int r = 0; r < 4; r++) u[r] = __shfl_up(e[r], 1u << k);
                const double m = lane >= (1 << k) ? 1.0 : 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    double a = P.M[k][4 * r] * u[0];
#pragma unroll
                    for (int j = 1; j < 4; j++) a = __builtin_fma(P.M[k][4 * r + j], u[j], a);
                    e[r] = __builtin_fma(m, a, e[r]);
                }
            }
            double v0[4];               // the lane's true start state
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double t = __shfl_up(e[r], 1u);
                v0[r] = lane == 0 ? q[c][r] : t;
            }
#pragma unroll
            for (int r = 0; r < 4; r++) q[c][r] = loud_readlane(e[r], 63);
            double cb = 0.0, ca = 0.0;
#pragma unroll
            for (int i = 0; i < LOUD_SEG; i++) {
                double yy = y[i];
#pragma unroll
                for (int r = 0; r < 4; r++) yy = __builtin_fma(P.Z[i][r], v0[r], yy);
                const double p = yy * yy;
                const bool before = (uint32_t)(n0 + i) < nb;
                cb += before ? p : 0.0;
                ca += before ? 0.0 : p;
            }
            e_before = __builtin_fma(P.w[c], cb, e_before);
            e_after = __builtin_fma(P.w[c], ca, e_after);
        }
        e_before = wave_all_sum_f64(e_before);
        e_after = wave_all_sum_f64(e_after);
        hop_sum += e_before;
        if (nb <= 1536u) {              // (the same in every lane)
            const double hn = hop_sum;
            if (hop_count != 0xffffffffu) hop_count++;
            if (hop_count >= 4) {
                const double z = (((h0 + h1) + h2) + hn) / P.block_samples;
                blocks++;
                max_block = z > max_block ? z : max_block;
                const int b = loud_bin(P.edges, z);
                if (b >= 0) {
                    blocks_abs++;
                    if (lane == 0) {
                        st->count[b] += 1;
                        st->sum[b] += z;
                    }
                }
            }
            if constexpr (RANGE) {
                if (lane == 0) range_push_hop(P.range + s, P.edges, hn, 7.5 * P.block_samples);
            }
            h0 = h1;
            h1 = h2;
            h2 = hn;
            hop_sum = e_after;
            pos = 1536u - nb;
        } else {
            pos += 1536u;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) st->bq[c][r] = q[c][r];
        st->hop_sum = hop_sum;
        st->hops[0] = h0;
        st->hops[1] = h1;
        st->hops[2] = h2;
        st->max_block = max_block;
        st->pos = pos;
        st->hop_count = hop_count;
        st->blocks = blocks;
        st->blocks_abs = blocks_abs;
    }
}

__global__ __launch_bounds__(64 * LOUD_WAVES) void loudness_read_kernel(const LoudState *state, unsigned n_streams, const double *tab,
                                                                       ac3mi_loudness_result *results)
{
    const int lane = threadIdx.x & 63;
    const unsigned s = pcm_wave_stream(LOUD_WAVES);
    if (s >= n_streams) return;
    const LoudState *st = state + s;
    double sum;
    uint32_t n;
    loud_total_part(st, lane, 64, &sum, &n);
    sum = wave_all_sum_f64(sum);
    n = wave_sum_u32(n);
    const double gamma = loud_gamma(sum, n);
    loud_gated_part(st, tab, gamma, lane, 64, &sum, &n);
    sum = wave_all_sum_f64(sum);
    n = wave_sum_u32(n);
    if (lane == 0) loud_result(st, tab + LOUD_BINS + 1, sum, n, results + s);
}

__global__ __launch_bounds__(64 * LOUD_WAVES) void loudness_range_read_kernel(const RangeState *state, unsigned n_streams, const double *edges,
                                                                             ac3mi_loudness_range_result *results)
{
    const int lane = threadIdx.x & 63;
    const unsigned s = pcm_wave_stream(LOUD_WAVES);
    if (s >= n_streams) return;
    const RangeState *rs = state + s;
    const double gamma = range_gamma(rs->sum_abs, rs->blocks_abs);
    const bool owner = lane < RANGE_LANES;              // lanes 60..63 own no bins
    const int first = owner ? lane * RANGE_RUN : 0;
    uint32_t c[RANGE_RUN];              // what each of this lane's bins adds to the counted blocks: the state is read once
#pragma unroll
    for (int k = 0; k < RANGE_RUN; k++) {
        const uint32_t v = range_counted(rs, edges, first + k, gamma);
        c[k] = owner ? v : 0;
    }
    const uint64_t part = range_counted_sum(c, RANGE_RUN);
    uint64_t incl = part;               // the blocks counted in this lane's bins and all below
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)incl, (unsigned)o);
        incl += lane >= o ? t : 0;
    }
    const uint64_t n = __shfl((unsigned long long)incl, 63);
    int lo = -1, hi = -1;               // one lane's run holds each rank
    if (n) {
        lo = range_bin_of_rank(c, first, RANGE_RUN, incl - part, range_rank(n, 10));
        hi = range_bin_of_rank(c, first, RANGE_RUN, incl - part, range_rank(n, 95));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
        lo = a > lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if (lane == 0) range_result(rs, n, lo, hi, results + s);
}

__global__ __launch_bounds__(256) void loudness_words_kernel(const ac3mi_loudness_result *results, unsigned n_frames, unsigned frames_per_stream,
                                                             uint32_t base_word, uint32_t *words)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames) return;
    const ac3mi_loudness_result *r = results + i / frames_per_stream;
    words[i] = (r->flags & AC3MI_LOUDNESS_EMPTY) ? base_word : ((base_word & ~31u) | (uint32_t)(r->dialnorm & 31u));
}

hipError_t launch_loudness(const LoudnessLaunch &L, hipStream_t stream)
{
    if (!loudness_args_ok(L) || !L.tab) return hipErrorInvalidValue;
    const double *coef = loud_coefs(L.sample_rate);
    LoudParams P;
    P.pcm = L.pcm;
    P.state = (LoudState *)L.state;
    P.range = (RangeState *)L.range_state;
    P.edges = L.tab;
    P.n_streams = (unsigned)L.n_streams;
    P.frames = L.frames_per_stream;
    P.hop = (uint32_t)(L.sample_rate / 10);
    pcm_copy_roles(P.role, L.role, L.channels);
    for (int c = 0; c < 6; c++) P.w[c] = P.role[c] == 2 ? 1.41 : P.role[c] == 1 ? 1.0 : 0.0;
    P.b0 = coef[0] / 32768.0; P.b1 = coef[1] / 32768.0; P.b2 = coef[2] / 32768.0; P.a1 = coef[3]; P.a2 = coef[4]; P.c1 = coef[8]; P.c2 = coef[9];
    P.block_samples = 4.0 * (double)P.hop;
    loud_build_segment(coef, P.M, P.Z);
    const bool vec = ((uintptr_t)L.pcm & 15) == 0;
    hipError_t e = hipSuccess;
    pcm_dispatch_channels(L.channels, [&](auto nch) {
        constexpr int NCH = decltype(nch)::value;
        const auto kernel = P.range ? (vec ? loudness_kernel<NCH, true, true> : loudness_kernel<NCH, false, true>)
                                    : (vec ? loudness_kernel<NCH, true, false> : loudness_kernel<NCH, false, false>);
        e = pcm_launch_streams(kernel, L.n_streams, LOUD_WAVES, 64 * LOUD_WAVES, stream, P);
    });
    return e;
}

hipError_t launch_loudness_read(const void *state, int n_streams, const double *tab, ac3mi_loudness_result *results, hipStream_t stream)
{
    return pcm_launch_streams(loudness_read_kernel, n_streams, LOUD_WAVES, 64 * LOUD_WAVES, stream, (const LoudState *)state, (unsigned)n_streams,
                              tab, results);
}

hipError_t launch_loudness_range_read(const void *range_state, int n_streams, const double *tab, ac3mi_loudness_range_result *results, hipStream_t stream)
{
    return pcm_launch_streams(loudness_range_read_kernel, n_streams, LOUD_WAVES, 64 * LOUD_WAVES, stream, (const RangeState *)range_state,
                              (unsigned)n_streams, tab, results);
}

hipError_t launch_loudness_words(const ac3mi_loudness_result *results, int n_streams, int frames_per_stream, uint32_t base_word,
                                 uint32_t *words, hipStream_t stream)
{
    const unsigned n = (unsigned)n_streams * (unsigned)frames_per_stream;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(loudness_words_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, results, n, (unsigned)frames_per_stream, base_word, words);
    return hipGetLastError();
}

}  // namespace ac3mi
#endif  // __HIPCC__
