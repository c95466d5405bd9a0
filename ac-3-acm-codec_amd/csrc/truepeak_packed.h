// truepeak_packed.h — the device form of truepeak_rule.h's interpolator that truepeak_kernel (truepeak.hip) and limit_kernel
// (limit.hip) share, on pcm_lanes.h's frame: samples two to a dword, a slot's history from the left neighbour, pairs of
// neighbours by v_perm_b32, an instant's four phases as six packed 16-bit dot products each.  Integer sums that cannot wrap
// (truepeak_rule.h), so tp_phases' bits in any order of adding.
#pragma once
#include "pcm_lanes.h"
#include "truepeak_rule.h"

namespace ac3mi {

static_assert(TP_SEG == PCM_SEG, "a lane's segment is the frame's");

// two int16 (dword a's half ha below dword b's half hb) as one dword: one v_perm_b32
__device__ __forceinline__ uint32_t tp_pack(uint32_t a, int ha, uint32_t b, int hb)
{
    const uint32_t sel = (uint32_t)(2 * ha) | ((uint32_t)(2 * ha + 1) << 8) | ((uint32_t)(4 + 2 * hb) << 16) | ((uint32_t)(5 + 2 * hb) << 24);
    return __builtin_amdgcn_perm(b, a, sel);
}

// The interpolator's input for slot C of one frame in one lane: q = the pairs of instants (-11, -10) .. (22, 23) of the lane's
// segment.  own = the lane's 24 instants as dwords [24][NCH]; carry = the 12 instants before the frame as dwords [12][NCH],
// the same in every lane.  The 11 instants before the segment come from the left neighbour's registers, one lane shift each
// (the dword that holds the sample; lane 0: the carried one)
template <int NCH, int C>
__device__ __forceinline__ void tp_pairs(const uint32_t *own, const uint32_t *carry, int lane, uint32_t q[TP_HIST + TP_SEG - 1])
{
    constexpr int HW = 6 * NCH;
    uint32_t h[TP_HIST];                // the dwords with instants -11 .. -1 of this slot
#pragma unroll
    for (int j = 0; j < TP_HIST; j++) {
        const int k = ((j + 1) * NCH + C) >> 1;
        const uint32_t left = __shfl_up(own[HW + k], 1u);
        h[j] = lane == 0 ? carry[k] : left;
    }
#pragma unroll
    for (int j = 0; j < TP_HIST + TP_SEG - 1; j++) {
        const int a = (j + 1) * NCH + C, b = a + NCH;       // (in dwords that start 12 instants before the segment)
        const uint32_t wa = j < TP_HIST ? h[j] : own[(a >> 1) - HW], wb = j + 1 < TP_HIST ? h[j + 1] : own[(b >> 1) - HW];
        q[j] = tp_pack(wa, a & 1, wb, b & 1);
    }
}

// (H[p][2 m + 1], H[p][2 m]) as the two halves of a dword: what meets the pair (x[n - 2 m - 1], x[n - 2 m])
constexpr int tp_coef2(int p, int m)
{
    return (int)((uint32_t)(uint16_t)tp_coef(p, 2 * m + 1) | ((uint32_t)(uint16_t)tp_coef(p, 2 * m) << 16));
}

// The four phases of instant n (tp_phases' sums, the same int32) from the 11 pairs (x[n - 11], x[n - 10]) .. (x[n - 1], x[n]),
// the earlier sample in the low half: six packed 16-bit dot products a phase, spelled as the instruction with the four phases
// of a pair side by side, and in order.  Left to itself hipcc starts a segment's 96 sums at once and spills their registers.
__device__ __forceinline__ void tp_phases_packed(const uint32_t *q11, int32_t y[TP_PHASES])
{
    int32_t y0, y1, y2, y3;
    asm volatile("v_dot2_i32_i16 %0, %4, %5, 0\n\tv_dot2_i32_i16 %1, %4, %6, 0\n\tv_dot2_i32_i16 %2, %4, %7, 0\n\tv_dot2_i32_i16 %3, %4, %8, 0"
                 : "=&v"(y0), "=&v"(y1), "=&v"(y2), "=&v"(y3)
                 : "v"(q11[10]), "s"(tp_coef2(0, 0)), "s"(tp_coef2(1, 0)), "s"(tp_coef2(2, 0)), "s"(tp_coef2(3, 0)));
#pragma unroll
    for (int m = 1; m < TP_TAPS / 2; m++)
        asm volatile("v_dot2_i32_i16 %0, %4, %5, %0\n\tv_dot2_i32_i16 %1, %4, %6, %1\n\tv_dot2_i32_i16 %2, %4, %7, %2\n\tv_dot2_i32_i16 %3, %4, %8, %3"
                     : "+v"(y0), "+v"(y1), "+v"(y2), "+v"(y3)
                     : "v"(q11[10 - 2 * m]), "s"(tp_coef2(0, m)), "s"(tp_coef2(1, m)), "s"(tp_coef2(2, m)), "s"(tp_coef2(3, m)));
    y[0] = y0; y[1] = y1; y[2] = y2; y[3] = y3;
}

}  // namespace ac3mi
