// resample.hip — the sample-rate converter of s16 PCM in device memory between 32, 44.1 and 48 kHz (ac3mi_resample_*; the rule is
// include/ac3mi.h's, its steps and the state's layout are resample_rule.h's).
//
// resample_kernel: one workgroup of five wavefronts (seven for the 441 phases of 32 -> 44.1 kHz) per stream; integers
// throughout.  Output instants are independent given the input, so the only ordering is that of the state: everything a call
// reads of it (the counters, the history, the old pending instants) is read before the first barrier and everything it writes
// is written behind one.
//   check       every thread forms the stream's plan from the counters (rs_plan); a stream whose out_frames is not its own, or
//               whose state is another pair's, gets its status and zeros and leaves before any barrier (the whole workgroup)
//   pending     the instants the state held go to the head of the output (out_frames 0: they stay where they are)
//   per input frame
//     stage     the frame and the 96 instants before it (the state's history for the call's first frame, else the frame
//               before) go to LDS planar, one plane per slot, each plane twice: once from sample 0 and once from sample 1, so
//               that the dword with (x[i - 2 j - 1], x[i - 2 j]) is aligned whatever the parity of i.  16-byte loads between
//               the source's 16-byte boundaries, 16-bit loads outside them
//     convert   the first `active` threads - the largest multiple of L up to the workgroup's 320 (448 for L = 441) - own the
//               output instants m0 + tid + active n, which all have one phase: the phase's row - (hi, lo) pairs of packed
//               coefficients, time-reversed like the samples - is read once a frame into T registers, 16 bytes at a time,
//               and i advances by active M / L.  Per instant the row runs over every slot: two packed 16-bit dot products
//               (v_dot2_i32_i16) per sample pair and slot, A = sum hi x and B = sum lo x in 32 bits (rs_split's bound),
//               rs_round, and the instant's samples go to a second LDS area, interleaved.  i and the phase of the frame's
//               first instant take one 64-bit division per frame, wave-uniform
//     store     behind a barrier the frame's instants leave LDS for the output, those past out_frames for the state's pending
//               area: 16-byte stores between the destination's 16-byte boundaries, 16-bit stores outside them
//   state       behind the last barrier: the pending entries the call freed are zeroed, the last 96 input instants become the
//               history, thread 0 writes the counters, the tag and the status
// Every loop is bounded by an argument or a constant; no atomics; plain vector stores; every alignment gives the same bits.
#include "resample_rule.h"
#include <mutex>
#include <vector>

namespace ac3mi {

// a pair's table and its split, built once per process
struct ResampleHostTable {
    std::once_flag once;
    bool ok = false;
    int L = 0, M = 0, T = 0;
    std::vector<int32_t> C;
    std::vector<int16_t> hi, lo;
};

static const ResampleHostTable *resample_host_table(int in_rate, int out_rate)
{
    static ResampleHostTable tabs[RS_PAIRS];
    const int pair = rs_pair(in_rate, out_rate);
    if (pair < 0) return nullptr;
    ResampleHostTable &t = tabs[pair];
    std::call_once(t.once, [&] {
        rs_ratio(in_rate, out_rate, &t.L, &t.M, &t.T);
        const size_t n = (size_t)t.L * (size_t)t.T;
        t.C.resize(n);
        t.hi.resize(n);
        t.lo.resize(n);
        rs_build_table(t.L, t.M, t.T, t.C.data());
        t.ok = rs_split(t.C.data(), t.L, t.T, t.hi.data(), t.lo.data());
    });
    return &t;
}

// d_pcm and d_out must not overlap at all; out may be null when it has no bytes
static inline bool resample_buffers_ok(const void *pcm, uint64_t pcm_bytes, const void *out, uint64_t out_bytes)
{
    const uintptr_t a = (uintptr_t)pcm, b = (uintptr_t)out;
    if (!a || (a & 1) || (b & 1)) return false;
    if (out_bytes == 0) return true;
    return b && (a + pcm_bytes <= b || b + out_bytes <= a);
}

static inline bool resample_params_ok(int in_rate, int out_rate, int channels, int in_frames, int out_frames)
{
    return rs_pair(in_rate, out_rate) >= 0 && channels >= 1 && channels <= 6 && in_frames >= 1 && in_frames <= RS_MAX_FRAMES && out_frames >= 0 &&
           out_frames <= RS_MAX_FRAMES;
}

}  // namespace ac3mi

extern "C" int ac3mi_resample_ratio(int in_rate, int out_rate, int *L, int *M, int *taps)
{
    return ac3mi::rs_ratio(in_rate, out_rate, L, M, taps) ? AC3MI_OK : AC3MI_ERR_ARG;
}

extern "C" int ac3mi_resample_tables(int in_rate, int out_rate, int32_t *coef)
{
    const ac3mi::ResampleHostTable *t = ac3mi::resample_host_table(in_rate, out_rate);
    if (!t || !coef) return AC3MI_ERR_ARG;
    if (!t->ok) return AC3MI_ERR_UNSUPPORTED;
    memcpy(coef, t->C.data(), t->C.size() * sizeof(int32_t));
    return AC3MI_OK;
}

extern "C" size_t ac3mi_resample_state_bytes(void) { return sizeof(ac3mi::ResampleState); }

extern "C" int ac3mi_resample_plan(int in_rate, int out_rate, uint64_t samples_in, uint64_t frames_out, int in_frames, int *out_frames,
                                   int *pending_after)
{
    int L, M;
    if (!ac3mi::rs_ratio(in_rate, out_rate, &L, &M, nullptr) || in_frames < 1 || in_frames > ac3mi::RS_MAX_FRAMES) return AC3MI_ERR_ARG;
    uint64_t of;
    uint32_t before, after;
    if (!ac3mi::rs_plan((uint32_t)L, (uint32_t)M, samples_in, frames_out, (uint32_t)in_frames, &of, &before, &after)) return AC3MI_ERR_ARG;
    if (out_frames) *out_frames = (int)of;
    if (pending_after) *pending_after = (int)after;
    return AC3MI_OK;
}

extern "C" int ac3mi_resample_host(const ac3mi_resample_desc *desc, const int16_t *h_pcm, int in_frames, int16_t *h_out, int out_frames,
                                   void *h_state, uint32_t *status)
{
    if (!desc || !h_state || !status || !ac3mi::resample_params_ok(desc->in_rate, desc->out_rate, desc->channels, in_frames, out_frames) ||
        !ac3mi::resample_buffers_ok(h_pcm, (uint64_t)in_frames * 3072u * (uint64_t)desc->channels, h_out,
                                    (uint64_t)out_frames * 3072u * (uint64_t)desc->channels))
        return AC3MI_ERR_ARG;
    const ac3mi::ResampleHostTable *t = ac3mi::resample_host_table(desc->in_rate, desc->out_rate);
    if (!t->ok) return AC3MI_ERR_UNSUPPORTED;
    const ac3mi::ResampleTable tb = {t->L, t->M, t->T, ac3mi::rs_pair(desc->in_rate, desc->out_rate), t->hi.data(), t->lo.data()};
    *status = ac3mi::resample_host(tb, desc->channels, h_pcm, in_frames, h_out, out_frames, h_state);
    return AC3MI_OK;
}

#ifdef __HIPCC__
#include "ac3mi_internal.h"
#include "pcm_lanes.h"

namespace ac3mi {

bool resample_args_ok(const ResampleLaunch &L)
{
    return resample_params_ok(L.in_rate, L.out_rate, L.channels, L.in_frames, L.out_frames) && L.n_streams >= 0 && L.state &&
           !((uintptr_t)L.state & 7) && L.status && !((uintptr_t)L.status & 3) &&
           resample_buffers_ok(L.pcm, (uint64_t)L.n_streams * (uint64_t)L.in_frames * 3072u * (uint64_t)L.channels, L.out,
                               (uint64_t)L.n_streams * (uint64_t)L.out_frames * 3072u * (uint64_t)L.channels);
}

// [L][T / 2] pairs of dwords: ((hi[p][2 j + 1], hi[p][2 j]), (lo[p][2 j + 1], lo[p][2 j])), the later tap in the low half: what meets
// the dword (x[i - 2 j - 1], x[i - 2 j])
size_t resample_packed_table(int in_rate, int out_rate, uint32_t *h_tab)
{
    const ResampleHostTable *t = resample_host_table(in_rate, out_rate);
    if (!t || !t->ok) return 0;
    const size_t n = (size_t)t->L * (size_t)t->T;
    if (!h_tab) return n;
    for (size_t e = 0; e < n / 2; e++) {
        h_tab[2 * e] = (uint32_t)(uint16_t)t->hi[2 * e + 1] | ((uint32_t)(uint16_t)t->hi[2 * e] << 16);
        h_tab[2 * e + 1] = (uint32_t)(uint16_t)t->lo[2 * e + 1] | ((uint32_t)(uint16_t)t->lo[2 * e] << 16);
    }
    return n;
}

constexpr int RS_MAX_THREADS = 448;             // seven wavefronts: the 441 phases of 32 -> 44.1 kHz, one to a thread
constexpr int RS_STAGED = RS_HIST + 1536;       // sample instants of a slot in LDS
constexpr int RS_PLANE = RS_STAGED / 2;         // ... dwords
constexpr int RS_MAX_OUT = 2304;                // output instants of a frame at most: 1536 * 3 / 2

// threads of a workgroup, and how many of them convert: the largest multiple of L, so that a thread's output instants - `active`
// apart - all have one phase
inline uint32_t rs_threads(uint32_t L) { return L > 320 ? RS_MAX_THREADS : 320; }
inline uint32_t rs_active(uint32_t L) { return rs_threads(L) / L * L; }

struct ResampleParams {
    const int16_t *pcm;
    int16_t *out;
    ResampleState *state;
    uint32_t *status;
    const uint4 *tab;                   // two sample pairs' (hi, lo, hi, lo) to an entry
    uint32_t in_frames, out_frames;
    uint32_t L, M;
    uint32_t active, step;              // converting threads; input instants between two of a thread's outputs, active * M / L
    uint32_t tag;
};

typedef short rs_short2 __attribute__((ext_vector_type(2)));

// acc + a.lo * b.lo + a.hi * b.hi on signed 16-bit halves: v_dot2_i32_i16 (no clamp: the sums cannot wrap, rs_split)
__device__ __forceinline__ int32_t rs_dot2(uint32_t a, uint32_t b, int32_t acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(rs_short2, a), __builtin_bit_cast(rs_short2, b), acc, false);
}

// int16 elements before p's next 16-byte boundary, at most n
__device__ __forceinline__ uint32_t rs_head(const void *p, uint32_t n)
{
    const uint32_t h = (uint32_t)((16u - ((uintptr_t)p & 15u)) & 15u) >> 1;
    return h < n ? h : n;
}

// n int16 from LDS to global memory by the whole workgroup: 16-bit stores up to dst's first 16-byte boundary and behind its
// last, 16-byte stores between (16-bit accesses to global memory run at a tenth of the rate; the same bytes either way)
__device__ __forceinline__ void rs_flush(int16_t *dst, const int16_t *src, uint32_t n, uint32_t tid, uint32_t nt)
{
    const uint32_t head = rs_head(dst, n), vecs = (n - head) / 8, tail = head + 8 * vecs;
    for (uint32_t e = tid; e < head; e += nt) dst[e] = src[e];
    for (uint32_t q = tid; q < vecs; q += nt) {
        const uint16_t *h = reinterpret_cast<const uint16_t *>(src) + head + 8 * q;
        uint4 v;
        v.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
        v.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
        v.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16);
        v.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
        *reinterpret_cast<uint4 *>(dst + head + 8 * q) = v;
    }
    for (uint32_t e = tail + tid; e < n; e += nt) dst[e] = src[e];
}

// one staged sample: element e of [instant][NCH] from instant u0 of the planes on
template <int NCH>
__device__ __forceinline__ void rs_put(uint32_t (*x)[2][RS_PLANE], uint32_t u0, uint32_t e, uint32_t bits)
{
    const uint32_t u = u0 + e / NCH, c = e % NCH;
    reinterpret_cast<uint16_t *>(x[c][0])[u] = (uint16_t)bits;
    if (u > 0) reinterpret_cast<uint16_t *>(x[c][1])[u - 1] = (uint16_t)bits;
}

// n int16 [instant][NCH] from global memory to the planes, from instant u0 on: 16-byte loads between src's 16-byte boundaries
template <int NCH>
__device__ __forceinline__ void rs_stage(uint32_t (*x)[2][RS_PLANE], uint32_t u0, const int16_t *src, uint32_t n, uint32_t tid, uint32_t nt)
{
    const uint16_t *h = reinterpret_cast<const uint16_t *>(src);
    const uint32_t head = rs_head(src, n), vecs = (n - head) / 8, tail = head + 8 * vecs;
    for (uint32_t e = tid; e < head; e += nt) rs_put<NCH>(x, u0, e, h[e]);
    for (uint32_t q = tid; q < vecs; q += nt) {
        const uint4 v = *reinterpret_cast<const uint4 *>(h + head + 8 * q);
        const uint32_t e = head + 8 * q;
        rs_put<NCH>(x, u0, e, v.x);
        rs_put<NCH>(x, u0, e + 1, v.x >> 16);
        rs_put<NCH>(x, u0, e + 2, v.y);
        rs_put<NCH>(x, u0, e + 3, v.y >> 16);
        rs_put<NCH>(x, u0, e + 4, v.z);
        rs_put<NCH>(x, u0, e + 5, v.z >> 16);
        rs_put<NCH>(x, u0, e + 6, v.w);
        rs_put<NCH>(x, u0, e + 7, v.w >> 16);
    }
    for (uint32_t e = tail + tid; e < n; e += nt) rs_put<NCH>(x, u0, e, h[e]);
}

template <int NCH, int T>
__global__ __launch_bounds__(RS_MAX_THREADS) void resample_kernel(const ResampleParams P)
{
    // [slot][0]: dword d = samples (2 d, 2 d + 1); [slot][1]: dword d = samples (2 d + 1, 2 d + 2); sample u is input instant u - 96 of the frame
    __shared__ uint32_t s_x[NCH][2][RS_PLANE];
    __shared__ int16_t s_y[RS_MAX_OUT * NCH];       // a frame's output instants, interleaved, on their way to memory
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const size_t s = blockIdx.x;
    ResampleState *st = P.state + s;
    int16_t *op = P.out + s * (size_t)P.out_frames * (1536 * NCH);
    const int16_t *sp = P.pcm + s * (size_t)P.in_frames * (1536 * NCH);

    const uint64_t n = st->samples_in, f = st->frames_out;
    const uint32_t tag = st->tag;
    uint32_t status = 0, before = 0, after = 0;
    uint64_t planned = 0;
    if (tag ? tag != P.tag : (n | f) != 0) status = AC3MI_RESAMPLE_STATE;
    else if (!rs_plan(P.L, P.M, n, f, P.in_frames, &planned, &before, &after) || planned != P.out_frames) status = AC3MI_RESAMPLE_FRAMES;
    const uint32_t cap = P.out_frames * 1536u;      // instants of the call that go to the output; the rest stay pending
    if (status) {
        for (uint32_t e = tid; e < cap * NCH; e += nt) op[e] = 0;
        if (tid == 0) P.status[s] = status;
        return;
    }

    if (cap > 0) {
        // (8-byte copies where the output allows them; the state's records are 8-byte aligned)
        const uint32_t quads = ((uintptr_t)op & 7) == 0 ? before * NCH / 4 : 0;
        for (uint32_t q = tid; q < quads; q += nt) reinterpret_cast<uint2 *>(op)[q] = reinterpret_cast<const uint2 *>(st->pend)[q];
        for (uint32_t e = 4 * quads + tid; e < before * NCH; e += nt) op[e] = st->pend[e];
    }

    for (uint32_t fr = 0; fr < P.in_frames; fr++) {
        const int16_t *fp = sp + (size_t)fr * (1536 * NCH);
        if (fr == 0) {
            for (uint32_t e = tid; e < RS_HIST * NCH; e += nt) rs_put<NCH>(s_x, 0, e, (uint16_t)st->hist[e % NCH][e / NCH]);
            rs_stage<NCH>(s_x, RS_HIST, fp, 1536 * NCH, tid, nt);
        } else {
            rs_stage<NCH>(s_x, 0, fp - RS_HIST * NCH, RS_STAGED * NCH, tid, nt);
        }
        __syncthreads();

        // the frame's output instants m_lo .. m_hi - 1: those whose newest input lies in this frame
        const uint64_t n0 = n + 1536ull * fr;
        const uint64_t m_lo = rs_out_count(n0, P.L, P.M), m_hi = rs_out_count(n0 + 1536, P.L, P.M);
        const uint64_t q0 = m_lo * P.M;
        const uint32_t i0 = (uint32_t)(q0 / P.L - n0), p0 = (uint32_t)(q0 % P.L);
        const uint32_t rel0 = (uint32_t)(m_lo - 1536 * f), count = (uint32_t)(m_hi - m_lo);
        if (tid < P.active) {
            // the thread's instants m_lo + tid + active * a: one phase, its row read once, i advances by `step`
            const uint32_t v = p0 + tid * P.M;              // < 441 + 447 * 441
            uint32_t i = i0 + v / P.L;
            const uint4 *row = P.tab + (size_t)(v % P.L) * (T / 4);
            uint4 w[T / 4];
#pragma unroll
            for (int k = 0; k < T / 4; k++) w[k] = row[k];
            for (uint32_t j = tid; j < count; j += P.active, i += P.step) {
                const uint32_t top = i + RS_HIST - 1;       // the sample under the newest one: the low half of the first pair
                const uint32_t at = top >> 1, odd = top & 1;
                int32_t A[NCH], B[NCH];
#pragma unroll
                for (int c = 0; c < NCH; c++) A[c] = B[c] = 0;
                // two sample pairs of every slot per step; the next step's reads are issued ahead of this step's sums
                uint32_t x0[NCH], x1[NCH];
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    x0[c] = s_x[c][odd][at];
                    x1[c] = s_x[c][odd][at - 1];
                }
#pragma unroll
                for (int k = 0; k < T / 4; k++) {
                    uint32_t y0[NCH], y1[NCH];
                    if (k + 1 < T / 4) {
#pragma unroll
                        for (int c = 0; c < NCH; c++) {
                            y0[c] = s_x[c][odd][at - 2 * (k + 1)];
                            y1[c] = s_x[c][odd][at - 2 * (k + 1) - 1];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);      // (left to itself hipcc keeps two reads in flight and waits on each)
#pragma unroll
                    for (int c = 0; c < NCH; c++) {
                        A[c] = rs_dot2(w[k].x, x0[c], A[c]);
                        B[c] = rs_dot2(w[k].y, x0[c], B[c]);
                        A[c] = rs_dot2(w[k].z, x1[c], A[c]);
                        B[c] = rs_dot2(w[k].w, x1[c], B[c]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (k + 1 < T / 4) {
#pragma unroll
                        for (int c = 0; c < NCH; c++) {
                            x0[c] = y0[c];
                            x1[c] = y1[c];
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < NCH; c++) s_y[j * NCH + c] = (int16_t)rs_round(A[c], B[c]);
            }
        }
        __syncthreads();
        // the frame's instants rel0 .. rel0 + count - 1 of the call: those under cap to the output, the rest to the pending area
        const uint32_t to_out = rel0 >= cap ? 0 : cap - rel0 < count ? cap - rel0 : count;
        rs_flush(op + (size_t)rel0 * NCH, s_y, to_out * NCH, tid, nt);
        rs_flush(st->pend + (size_t)(rel0 + to_out - cap) * NCH, s_y + to_out * NCH, (count - to_out) * NCH, tid, nt);
    }

    if (cap > 0)
        for (uint32_t e = after * NCH + tid; e < before * NCH; e += nt) st->pend[e] = 0;
    const int16_t *tail = sp + ((size_t)P.in_frames * 1536 - RS_HIST) * NCH;
    for (uint32_t e = tid; e < RS_HIST * NCH; e += nt) st->hist[e % NCH][e / NCH] = tail[e];
    if (tid == 0) {
        st->samples_in = n + 1536ull * P.in_frames;
        st->frames_out = f + P.out_frames;
        st->tag = (uint8_t)P.tag;
        P.status[s] = 0;
    }
}

template <int NCH>
static void rs_launch_nch(const ResampleParams &P, int taps, dim3 grid, dim3 block, hipStream_t stream)
{
    switch (taps) {
    case 64: hipLaunchKernelGGL((resample_kernel<NCH, 64>), grid, block, 0, stream, P); break;
    case 72: hipLaunchKernelGGL((resample_kernel<NCH, 72>), grid, block, 0, stream, P); break;
    default: hipLaunchKernelGGL((resample_kernel<NCH, 96>), grid, block, 0, stream, P); break;
    }
}

hipError_t launch_resample(const ResampleLaunch &L, hipStream_t stream)
{
    if (!resample_args_ok(L) || !L.tab) return hipErrorInvalidValue;
    if (L.n_streams == 0) return hipSuccess;
    int l, m, t;
    rs_ratio(L.in_rate, L.out_rate, &l, &m, &t);
    ResampleParams P;
    P.pcm = L.pcm;
    P.out = L.out;
    P.state = (ResampleState *)L.state;
    P.status = L.status;
    P.tab = reinterpret_cast<const uint4 *>(L.tab);
    P.in_frames = (uint32_t)L.in_frames;
    P.out_frames = (uint32_t)L.out_frames;
    P.L = (uint32_t)l;
    P.M = (uint32_t)m;
    P.active = rs_active(P.L);
    P.step = P.active / P.L * P.M;
    P.tag = rs_tag(rs_pair(L.in_rate, L.out_rate), L.channels);
    const dim3 grid((unsigned)L.n_streams), block(rs_threads(P.L));
    pcm_dispatch_channels(L.channels, [&](auto nch) { rs_launch_nch<decltype(nch)::value>(P, t, grid, block, stream); });
    return hipGetLastError();
}

}  // namespace ac3mi
#endif  // __HIPCC__
