// decode_mx.hip — mantx_kernel: the mantissa half of the split front end with the synthesis transform fused in, for
// batches of one-frame streams whose coded planes are the output planes (no downmix).  Replaces mant_kernel + xform_kernel
// for those calls: the dequantised coefficient planes (L52/parse.c:813-879) never touch HBM - 36.9 KB written and read again
// per 5.1 frame otherwise - they go from the unpacking wavefront's LDS straight into a52_imdct_512 / a52_imdct_256
// (L52/imdct.c:258-345), window, overlap-add and, for the s16 variant, the reference's float -> s16 converter
// (src/AC3ASM.asm:174-318).
//
// A workgroup of six wavefronts takes one frame (as mant_kernel): wavefront b unpacks audio block b into six padded planes
// in its own LDS region (mant_block2, mant2.h - the same code, the planes' address is the only difference), then runs the
// transform of xform_core.h on them, one plane per 8-lane group - exactly the arithmetic of xform_kernel, so PCM and overlap
// state are bit-identical to the two-kernel path (tests/test_decode_gpu.py).  Block b's overlap tail goes to block b + 1
// through LDS, a flag per wavefront instead of a workgroup barrier; block 0 takes the stream's state from HBM, block 5 leaves the new state.
//
// LDS per wavefront (MX_WAVE = 7296 bytes, used in turn): planes 6 x 272 floats + the code ring of the mantissa stage |
// the six 8x16 transposes | tails (3 KB, read by the next wavefront) + the s16 tile (3 KB).
#include <stdlib.h>
#include "mant2.h"
#include "xform_core.h"
#include "ac3mi_internal.h"

namespace ac3mi {

constexpr int MX_PLANE = 256 + 16;              // floats from plane to plane: the six groups' loads fall on different banks
constexpr int MX_WAVE = 6 * EX_GROUP * 8;       // bytes per wavefront region
constexpr int MX_RING = 6 * MX_PLANE * 4;       // byte offset of the mantissa stage's code ring inside the region
constexpr int MX_TILE = 3072;                   // byte offset of the s16 tile (the tails come first)
static_assert(MX_RING + M2_LDS_WAVE <= MX_WAVE && MX_TILE + 256 * 6 * 2 <= MX_WAVE && 48 * 8 * 8 <= MX_TILE, "region layout");

struct MantxParams {
    MantParams m;
    const uint8_t *blksw;       // [frames][6][nfchans] from the parse kernel
    float *delay;               // overlap state, [streams or slots][delay_stride]
    const int32_t *slot;
    int delay_stride;
    float *pcm;                 // [frames][6][n_in][256], or
    int16_t *pcm16;             // [frames][6][256][n_in] interleaved, plane o in WAVE slot wslot[o]
    int8_t wslot[6];
    const float2 *tw_long, *tw_short;
    const float *window;
    float bias;
};

struct MantxLDS {
    uint4 dsc[M2_NDESC];
    float qtab[760];
    float2 tw[2][128];          // merged lane twiddles [long, short][lane][k]
    float win[256];
    uint8_t cplbnd[6][20];
    uint32_t ready[6];          // wavefront b's tails are in its region
    alignas(16) uint8_t wave[6][MX_WAVE];
};

#ifndef MANTX_LB
#define MANTX_LB 3
#endif
// Measurement aid (make EXTRA=-DMX_STAMPS, a separate library): lane 0 of every wavefront adds the s_memtime ticks of its
// sections to g_mx_cycles[block][section]: 0 staging up to the barrier, 1 mantissas, 2 transform, 3 waiting for the block
// before, 4 window + output.  ac3mi_debug_mx_cycles reads them (profiles/mx_stamps.py).
#ifdef MX_STAMPS
__device__ unsigned long long g_mx_cycles[6][8];
#define MX_T0() unsigned long long mx_t = __builtin_readcyclecounter()
#define MX_LAP(id) do { const unsigned long long t_ = __builtin_readcyclecounter(); if (lane == 0) atomicAdd(&g_mx_cycles[blk][id], t_ - mx_t); mx_t = t_; } while (0)
#else
#define MX_T0() do { } while (0)
#define MX_LAP(id) do { } while (0)
#endif
// FX (launch_decode's fixed-shape rule): 5.1 - six planes, five full-bandwidth channels, acmod 7 (no rematrixing) with the
// LFE, as constants instead of P's members; the WAVE slot of a plane comes out of one packed word instead of a chain of selects.
template <bool S16, bool FX = false>
__global__ __launch_bounds__(384, MANTX_LB) void mantx_kernel(const MantxParams Q)
{
    const MantParams &P = Q.m;
    const int n_in = FX ? 6 : P.n_in, nfchans = FX ? 5 : P.nfchans;
    __shared__ MantxLDS L;
    extern __shared__ uint32_t frw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int blk = __builtin_amdgcn_readfirstlane(tid >> 6);
    MX_T0();
    const unsigned fidx = xcd_remap(blockIdx.x, gridDim.x);     // consecutive frames on one XCD, as mant_kernel
    const size_t unit = (size_t)fidx * 6 + blk;
    const uint4 *dq = reinterpret_cast<const uint4 *>(P.desc + unit);
    const BlkWords D{{dq[0], dq[1], dq[2], dq[3], dq[4]}};
    const uint32_t fposv = P.frame_pos[fidx];
    const int nw = (P.frame_bytes + 3) >> 2;
    // Set-up.  Every load is issued before the first wait on any of them (a copy loop, or a load and its LDS store inside one
    // branch, was a round trip to memory each: profiles/EXPERIMENTS.md): the frame's words, which miss in cache, then the
    // chip-resident tables - two dequantiser words a thread, and ONE float2 of the twiddles and the window, which lie
    // back to back in LDS (wavefronts 0-1 the long twiddles, 2-3 the short ones, 4-5 the window as 128 pairs).  The first
    // use of any of it is the descriptor's, for the one dependent request - the first segment's rows - which then travels
    // while the LDS stores wait for the words requested before it, and on across the barrier.
    static_assert(offsetof(MantxLDS, win) == offsetof(MantxLDS, tw) + sizeof(float2) * 256, "tw and win are one 3-KB stretch");
    const auto fw = stage_frame_fetch<384>(P.frames + (size_t)fidx * P.frame_stride, P.frame_bytes, tid);
    const float q0 = P.tab->qtab[tid];
    float q1 = 0.f;
    if (tid < 760 - 384) q1 = P.tab->qtab[384 + tid];
    const float2 *twsrc = blk < 2 ? Q.tw_long + tid : blk < 4 ? Q.tw_short + (tid - 128) : reinterpret_cast<const float2 *>(Q.window) + (tid - 256);
    const float2 twv = *twsrc;
    uint8_t *const region = L.wave[blk];
    float *const planes = reinterpret_cast<float *>(region);
    MantBlk B;
    B.nf = nfchans; B.lfeon = FX ? 1 : P.lfeon; B.acmod = FX ? 7 : P.acmod; B.in_lfe = FX ? 1 : P.lfeon ? 1 : 0;
    const bool failed = D.head(B);
    // (a failed block's row indices read as 0: its request below then goes to the frame's own first row set and is never looked
    // at.  Behind a branch on `failed` the request would not cross the barrier - the waits for the words requested before it
    // have to assume the fewest loads in flight behind them - and it is the one load that should)
    const uint64_t rve = failed ? 0ull : D.rv_exp();
    const uint64_t rvb = failed ? 0ull : D.rv_bap();
    const uint8_t *const rowbase = P.rows + (size_t)fidx * 6 * ROWSET;
    const RowFetch fetch{rowbase, rve, rvb, lane};
    __builtin_assume(B.nf >= 1);                                // (every acmod has a channel: the first segment is slot 0's, and its request below sits behind no branch)
    const int slot0 = seg_slot(0, B.nf, B.chincpl, B.chincpl ? __builtin_ctz(B.chincpl) : 99);
    const uint2 first = fetch(slot0);
    {
        stage_frame_store<384>(frw, fw, P.frame_bytes, tid);
        // the slot's bytes behind a frame shorter than frame_bytes are not the frame's.  The parse kernel leaves such a frame's own
        // size in every block's descriptor (0: full size - every frame of a batch of one frame size); each thread clears what it staged
        if (const int own = D.own_bytes()) trim_staged_frame(frw, own, nw, tid, 384);
        if (tid < M2_NDESC) L.dsc[tid] = mant_desc2((uint32_t)tid);
        L.qtab[tid] = q0;
        if (tid < 760 - 384) L.qtab[384 + tid] = q1;
        reinterpret_cast<float2 *>(&L.tw[0][0])[tid] = twv;
        if (tid < 6) L.ready[tid] = 0u;
    }
    __syncthreads();
    MX_LAP(0);

    // ---- mantissas -> planes in LDS (a failed block leaves zero planes) ----
    if (failed) {
        for (int c = 0; c < n_in; c++)
            *reinterpret_cast<float4 *>(planes + c * MX_PLANE + 4 * lane) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        D.ranges(B);
        B.gainv = D.gainv(lane);
        if (B.chincpl && lane < 18) {                               // sub-band -> band (parse.c:448-456)
            const uint32_t below = D.cplbndstrc() & ((1u << lane) - 1u);
            L.cplbnd[blk][lane] = (uint8_t)(lane - __popc(below));
        }
        const uint32_t fpos = rfl(fposv);
        const bool lfsr_live = fpos != 0xffffffffu;
        const uint32_t i0 = lfsr_live ? (fpos + D.draw_off()) % 65535u : 0u;
        const float *cc = P.cplco + unit * 90;
        mant_block2<MX_PLANE, true>(B, fetch, first, [&](int c, int bnd) { return cc[c * 18 + bnd]; }, L.cplbnd[blk], L.dsc, region + MX_RING, frw,
                              (uint32_t)nw + 2u, L.qtab, reinterpret_cast<const int16_t *>(P.lfsr_seq) + 1 + i0, lfsr_live, planes, D.bitpos(), lane);
    }
    wave_sync();

    MX_LAP(1);
    // ---- transform: 8-lane group g takes plane g (left-over groups shadow plane 0 and store nothing) ----
    const int l8 = lane & 7, grp = lane >> 3;
    const bool own = grp < n_in;
    const int o = own ? grp : 0;
    const int fb = o - B.in_lfe;
    const bool sw = fb >= 0 && Q.blksw[unit * nfchans + fb] != 0;
    const size_t sidx = Q.slot ? (size_t)Q.slot[fidx] : (size_t)fidx;      // one frame per stream: stream = frame
    float *const dptr = Q.delay + sidx * Q.delay_stride + (size_t)o * 128;
    float2 dl[8];
    if (blk == 0) {                                                 // the stream's overlap state, in flight during the transform
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = ((j & 1) ? 15 - l8 : l8) + 16 * (j >> 1);
            dl[j] = *reinterpret_cast<const float2 *>(dptr + 2 * i);
        }
    }
    FirstTail ft;
#pragma unroll
    for (int j = 0; j < 8; j++) ft.f0[j] = ft.f1[j] = ft.t0[j] = ft.t1[j] = 0.f;
    {
        // the loads of xform.hip's load_long / load_short on the LDS plane; every group's loads come before any group's
        // transpose (the transposes overwrite the planes)
        const float *plane = planes + o * MX_PLANE;
        float xa[16], xb[16];
        if (!sw) {
            const float2 *p = reinterpret_cast<const float2 *>(plane) + l8;
            float2 v[16];
#pragma unroll
            for (int n = 0; n < 16; n++) v[n] = p[8 * n];
#pragma unroll
            for (int n = 0; n < 16; n++) {
                xa[n] = __builtin_fmaf(1.f, v[n].x, 0.f);
                xb[n] = __builtin_fmaf(1.f, mirror8(v[15 - n].y), 0.f);
            }
        } else {
            const int f = l8 >> 2, n2 = l8 & 3;
            const float *pa = plane + 4 * n2 + f;
            const float *pb = plane + 254 + f - 4 * n2;
#pragma unroll
            for (int n = 0; n < 16; n++) {
                xa[n] = __builtin_fmaf(1.f, pa[16 * n], 0.f);
                xb[n] = __builtin_fmaf(1.f, pb[-16 * n], 0.f);
            }
        }
        wave_sync();
        float2 *ex = reinterpret_cast<float2 *>(region) + o * EX_GROUP;
        const float2 *tw = &L.tw[sw ? 1 : 0][l8 * 16];
        cf r[16];
        imdct_first_half(xa, xb, tw, ex, l8, r);
        if (!sw) imdct_long_second_half(r, ft);
        else imdct_short_second_half(r, ft);
    }
    // ---- tails to the next block's wavefront ----
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (blk < 5 && lane < 48) {
        float2 *tl = reinterpret_cast<float2 *>(region);
#pragma unroll
        for (int j = 0; j < 8; j++) tl[j * 48 + lane] = make_float2(ft.t0[j], ft.t1[j]);
    }
    // Wavefront b waits for wavefront b - 1 only (a workgroup barrier here would hold all six until the slowest block is
    // unpacked and transformed).  The six are resident together and none leaves before it has published, so the wait ends;
    // the bound on the spin is a backstop, not an exit anyone takes.  Wavefront 0 publishes once the stream's old state has
    // ARRIVED in its registers; wavefront 5 stores the new one only after it has seen that flag as well.
    MX_LAP(2);
    if (blk == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the old state has arrived, not merely been requested)
    if (blk < 5) __hip_atomic_store(&L.ready[blk], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (blk > 0) {
        for (int spin = 0; spin < (1 << 20) && __hip_atomic_load(&L.ready[blk - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u; spin++)
            __builtin_amdgcn_s_sleep(1);
        const float2 *tl = reinterpret_cast<const float2 *>(L.wave[blk - 1]);
        const int ls = lane < 48 ? lane : l8;                       // (shadow groups read group 0's)
#pragma unroll
        for (int j = 0; j < 8; j++) dl[j] = tl[j * 48 + ls];
    }
    if (blk == 5) {
        for (int spin = 0; spin < (1 << 20) && __hip_atomic_load(&L.ready[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u; spin++)
            __builtin_amdgcn_s_sleep(1);
    }
    if (blk == 5 && own) {                                          // the last block's tails are the stream's new state
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = ((j & 1) ? 15 - l8 : l8) + 16 * (j >> 1);
            *reinterpret_cast<float2 *>(dptr + 2 * i) = make_float2(ft.t0[j], ft.t1[j]);
        }
    }

    MX_LAP(3);
    // ---- window + overlap-add + bias (xform.hip's output stage) ----
    int16_t *tile = reinterpret_cast<int16_t *>(region + MX_TILE);
    int wsl = 0;
    if constexpr (FX) {
        uint64_t w = 0;
#pragma unroll
        for (int oo = 0; oo < 6; oo++) w |= (uint64_t)(uint8_t)Q.wslot[oo] << (8 * oo);
        wsl = (int)((uint32_t)(w >> (8 * o)) & 0xffu);
    } else {
#pragma unroll
        for (int oo = 0; oo < 6; oo++) wsl = oo == o ? Q.wslot[oo] : wsl;
    }
    float *oblk = S16 ? nullptr : Q.pcm + (unit * n_in + o) * 256;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int i = ((j & 1) ? 15 - l8 : l8) + 16 * (j >> 1);
        const float2 wlo = *reinterpret_cast<const float2 *>(&L.win[2 * i]);
        const float2 whi = *reinterpret_cast<const float2 *>(&L.win[254 - 2 * i]);
        float2 lo, hi;
        window_pair(ft.f0[j], ft.f1[j], dl[j], wlo, whi, Q.bias, lo, hi);
        if (!S16 && own) {
            *reinterpret_cast<float2 *>(oblk + 2 * i) = lo;
            *reinterpret_cast<float2 *>(oblk + 254 - 2 * i) = hi;
        }
        if (S16 && own) {                                           // (24-bit multiplies: v_mul_lo_u32 runs at a quarter of the rate)
            const int at = wsl + (int)__umul24((uint32_t)(2 * i), (uint32_t)n_in), top = wsl + (int)__umul24(254u, (uint32_t)n_in) - (at - wsl);
            tile[at] = to_s16(lo.x);
            tile[at + n_in] = to_s16(lo.y);
            tile[top] = to_s16(hi.x);
            tile[top + n_in] = to_s16(hi.y);
        }
    }
    if (S16) {
        wave_sync();
        const int upb = 32 * n_in;                                // 16-byte units of the block
        int16_t *dst = Q.pcm16 + unit * 256 * n_in;
#pragma unroll
        for (int it = 0; it < 3; it++) {
            const int u = it * 64 + lane;
            if (u < upb) *reinterpret_cast<uint4 *>(dst + u * 8) = *reinterpret_cast<const uint4 *>(tile + u * 8);
        }
    }
    MX_LAP(4);
}

template <uint32_t V> struct MantxVariant { static constexpr auto fn = mantx_kernel<(V & V_S16) != 0, (V & V_FX) != 0>; };

// mant_kernel + xform_kernel in one launch (launch_decode calls this for the rule's K_MANTX launch; L.fuse is set)
hipError_t launch_mantx(const DeviceTables &tab, const DecodeLaunch &L, const MantParams &M, const KernelLaunch &k, hipStream_t stream)
{
    if (!L.fuse) return hipErrorInvalidValue;
    const XformLaunch &X = *L.fuse;
    if (L.frames_per_stream != 1 || X.plan.n_in != X.plan.n_out || M.n_in > 6) return hipErrorInvalidValue;
    MantxParams Q;
    Q.m = M;
    Q.m.coef = nullptr;
    Q.blksw = L.blksw;
    Q.delay = X.delay;
    Q.slot = X.slot;
    Q.delay_stride = X.slot ? X.delay_stride : X.plan.n_out * 128;
    Q.pcm = X.pcm;
    Q.pcm16 = X.pcm16;
    Q.tw_long = tab.tw_long;
    Q.tw_short = tab.tw_short;
    Q.window = tab.window;
    Q.bias = X.bias;
    for (int o = 0; o < 6; o++) Q.wslot[o] = 0;
    static const int lds_pad = getenv("AC3MI_MANTX_LDS_PAD") ? atoi(getenv("AC3MI_MANTX_LDS_PAD")) : 0;      // profiling aid: occupancy sweeps
    if (((k.variant & V_S16) != 0) != (X.pcm16 != nullptr)) return hipErrorInvalidValue;
    if (X.pcm16) {
        int map[6];
        if (s16_channel_map(X.s16_flags, map) != X.plan.n_out || ((uintptr_t)X.pcm16 & 15)) return hipErrorInvalidValue;
        for (int w = 0; w < X.plan.n_out; w++) Q.wslot[map[w]] = (int8_t)w;
    }
    const auto fn = variant_fn<MANTX_VARIANTS, MantxVariant>(k.variant);
    if (!fn) return hipErrorInvalidValue;
    log_launch(L.log, k);
    hipLaunchKernelGGL(fn, dim3(M.n_frames), dim3(k.block), staged_frame_lds(L.frame_bytes) + lds_pad, stream, Q);
    return hipGetLastError();
}

}  // namespace ac3mi

#ifdef MX_STAMPS
extern "C" __attribute__((visibility("default"))) int ac3mi_debug_mx_cycles(unsigned long long *out48, int reset)
{
    if (hipMemcpyFromSymbol(out48, HIP_SYMBOL(ac3mi::g_mx_cycles), sizeof(unsigned long long) * 48) != hipSuccess) return -1;
    if (reset) { unsigned long long z[48] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(ac3mi::g_mx_cycles), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif
