// wave_ops.h — wavefront (64-lane) prefix sums and reductions on the gfx950 DPP network.
// No LDS traffic: four row_shr steps inside each row of 16 lanes, then row_bcast:15 carries the
// totals of rows 0 and 2 into rows 1 and 3, then row_bcast:31 carries the lower half into the upper.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ac3mi {

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);    // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);    // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);    // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);    // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1,3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2,3
    return v;
}

// the same inside each row of 16 lanes (the four row_shr steps alone)
__device__ __forceinline__ uint32_t row_incl_scan_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    return v;
}

// the same with XOR for the sum (a lane without a source takes 0, XOR's identity too)
__device__ __forceinline__ uint32_t wave_incl_scan_xor_u32(uint32_t v)
{
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);    // row_shr:1
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);    // row_shr:2
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);    // row_shr:4
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);    // row_shr:8
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1,3
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2,3
    return v;
}

// lane 63's value as a wave-uniform scalar
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return wave_last(wave_incl_scan_u32(v)); }

// The sum of all lanes' values in every lane, by a butterfly that adds in this order and no other - the partner 32 lanes away
// first, the neighbour last: the loudness meter's bits depend on it
__device__ __forceinline__ double wave_all_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// What the lanes of a wavefront wrote to LDS or memory before this point, every lane of it reads behind it: release fence,
// wavefront barrier, acquire fence.  (A release and a barrier WITHOUT the acquire - a wavefront that only hands its stores on -
// is another fence and stays spelled out where it is used.)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Consecutive work items on one XCD (its L2 then serves what neighbours share once): workgroup `block` of `grid`, which the
// hardware deals to the eight XCDs in turn, takes the item that a contiguous eight-way split of the grid gives its XCD -
// the bijective remap of cdna_hip_programming.md T1 (the first grid % 8 XCDs hold one item more).
__device__ __forceinline__ unsigned xcd_remap(unsigned block, unsigned grid)
{
    const unsigned q = grid >> 3, r = grid & 7u, x = block & 7u, i = block >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// a * b on the low 24 bits of both, as v_mul_u32_u24 and nothing else: where only the low bits of `__umul24(x & 0xffff, w)`
// are used, hipcc drops the mask (the low bits of a product need only the low bits of the factors), then no longer knows the
// factor is short and emits v_mul_lo_u32 - a quarter of the rate.
__device__ __forceinline__ uint32_t mul24_asm(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Prefix minimum / maximum.  One `v_max_i32_dpp v, v, v` per step: a lane whose source lies outside its row (or whose row is
// masked out) is left unwritten, which IS the identity - no identity register, no separate move.  hipcc does not form this
// from __builtin_amdgcn_update_dpp + max (it emits v_mov_b32 identity, s_nop, v_mov_b32_dpp, v_max: four instructions per
// step), so the steps are spelled out; `s_nop 1` = the two wait states a DPP read needs behind the VALU write of its source
// (gfx9 data hazard), which the compiler cannot place inside an asm block - nor behind it, hence the trailing one.
#define AC3MI_DPP6(op) \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t" \
    "s_nop 1\n\t" op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t" \
    "s_nop 1"
// two independent scans interleaved: each fills one of the other's wait states
#define AC3MI_DPP6x2(op) \
    "s_nop 1\n\t" \
    op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t" op " %1, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 0\n\t" \
    op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t" op " %1, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 0\n\t" \
    op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t" op " %1, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 0\n\t" \
    op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t" op " %1, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 0\n\t" \
    op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t" op " %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 0\n\t" \
    op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t" op " %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"

__device__ __forceinline__ int wave_incl_scan_min(int v)
{
    asm volatile(AC3MI_DPP6("v_min_i32_dpp") : "+v"(v));
    return v;
}
__device__ __forceinline__ int wave_incl_scan_max(int v)
{
    asm volatile(AC3MI_DPP6("v_max_i32_dpp") : "+v"(v));
    return v;
}
__device__ __forceinline__ void wave_incl_scan_min2(int &a, int &b)
{
    asm volatile(AC3MI_DPP6x2("v_min_i32_dpp") : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void wave_incl_scan_max2(int &a, int &b)
{
    asm volatile(AC3MI_DPP6x2("v_max_i32_dpp") : "+v"(a), "+v"(b));
}

// A butterfly network's trade inside the quads, D = 1 or 2 lanes apart: a lane with (lane & D) == 0 keeps p and takes its
// partner's p for q, the partner keeps q and takes this lane's q for p - for two components at once.  v_cndmask_b32_dpp reads
// its first source through the quad permutation and selects with VCC, so each result is one instruction: VCC = the lower
// lanes gives p' = lower ? p : partner's q, its complement q' = upper ? q : partner's p.  hipcc does not form this from
// __builtin_amdgcn_update_dpp + select (two selects, two zero moves, two DPP moves and four selects per trade); the block
// carries its own wait states, as the scans above do.  Every lane of the wavefront must be active.
template <int D>
__device__ __forceinline__ void quad_trade2(int &pr, int &pi, int &qr, int &qi)
{
    static_assert(D == 1 || D == 2, "inside a quad");
    constexpr uint64_t lower = D == 1 ? 0x5555555555555555ull : 0x3333333333333333ull;
    int npr, npi, nqr, nqi;
    if constexpr (D == 1)
        asm volatile("s_mov_b64 vcc, %8\n\ts_nop 1\n\t"
                     "v_cndmask_b32_dpp %0, %6, %4, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %1, %7, %5, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                     "s_not_b64 vcc, vcc\n\t"
                     "v_cndmask_b32_dpp %2, %4, %6, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %3, %5, %7, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1"
                     : "=&v"(npr), "=&v"(npi), "=&v"(nqr), "=&v"(nqi) : "v"(pr), "v"(pi), "v"(qr), "v"(qi), "s"(lower) : "vcc", "scc");
    else
        asm volatile("s_mov_b64 vcc, %8\n\ts_nop 1\n\t"
                     "v_cndmask_b32_dpp %0, %6, %4, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %1, %7, %5, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "s_not_b64 vcc, vcc\n\t"
                     "v_cndmask_b32_dpp %2, %4, %6, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %3, %5, %7, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "s_nop 1"
                     : "=&v"(npr), "=&v"(npi), "=&v"(nqr), "=&v"(nqi) : "v"(pr), "v"(pi), "v"(qr), "v"(qi), "s"(lower) : "vcc", "scc");
    pr = npr; pi = npi; qr = nqr; qi = nqi;
}

// maximum of all lanes' non-negative values, wave-uniform
__device__ __forceinline__ int wave_max_nonneg(int v) { return __builtin_amdgcn_readlane(wave_incl_scan_max(v), 63); }

// suffix minimum: lane i gets min over lanes i..63 (row_shl inside the rows, the row totals through scalars)
__device__ __forceinline__ int wave_suffix_scan_min(int v, int lane)
{
    constexpr int ID = 0x3fffffff;
    asm volatile("s_nop 1\n\tv_min_i32_dpp %0, %0, %0 row_shl:1 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_min_i32_dpp %0, %0, %0 row_shl:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_min_i32_dpp %0, %0, %0 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_min_i32_dpp %0, %0, %0 row_shl:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1" : "+v"(v));
    const int t1 = __builtin_amdgcn_readlane(v, 16), t2 = __builtin_amdgcn_readlane(v, 32), t3 = __builtin_amdgcn_readlane(v, 48);
    const int a2 = t2 < t3 ? t2 : t3, a1 = t1 < a2 ? t1 : a2;
    const int r = lane >> 4;
    const int extra = r == 0 ? a1 : r == 1 ? a2 : r == 2 ? t3 : ID;
    return extra < v ? extra : v;
}

}  // namespace ac3mi
