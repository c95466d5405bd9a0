// mdct_rule.h — the scalar rules of enc_mdct_kernel's block loop, stated once and without branches: the largest magnitude of a
// lane's windowed samples, a coefficient's raw exponent, and the twiddle that stands for "no multiply".  Plain C++: the kernel
// includes it, and tests/mdct_rule_c/main.cpp holds each rule to the expression it replaced on the host.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

__host__ __device__ inline int mdct_max_i32(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline int mdct_min_i32(int a, int b) { return a < b ? a : b; }

// max |w[k]| over eight values as max(max w, -min w): a chain of three-operand maxima, one of minima, one negation (the
// larger of the two is never negative: where every w is negative, -min w is positive).  |w| <= 2^31 - 1 is the caller's.
__host__ __device__ inline int mdct_mag8(const int (&w)[8])
{
    int hi = mdct_max_i32(mdct_max_i32(w[0], w[1]), w[2]), lo = mdct_min_i32(mdct_min_i32(w[0], w[1]), w[2]);
    hi = mdct_max_i32(mdct_max_i32(hi, w[3]), w[4]); lo = mdct_min_i32(mdct_min_i32(lo, w[3]), w[4]);
    hi = mdct_max_i32(mdct_max_i32(hi, w[5]), w[6]); lo = mdct_min_i32(mdct_min_i32(lo, w[5]), w[6]);
    lo = mdct_min_i32(lo, w[7]);
    return mdct_max_i32(mdct_max_i32(hi, w[7]), -lo);
}

// The raw exponent of coefficient c of a row normalised by `shift` (= v - 9, v = 0 .. 14; the reference's :1707-1722):
// 23 - log2|c| + shift = clz|c| + shift - 8, and 24 with the coefficient zeroed where that reaches 24 or c is 0.  The count of
// a zero is taken as 41, so that 41 + shift - 8 >= 24 for every shift >= -9 and the zero needs no case of its own; on the GPU
// the count is the bare v_ffbh_u32, which gives 0xffffffff for 0.  The exponent stays signed (a coefficient of 2^16 under shift -9 gives -2).
__host__ __device__ inline int mdct_raw_exp(int &c, int shift)
{
    const unsigned a = (unsigned)mdct_max_i32(c, -c);
#ifdef __HIP_DEVICE_COMPILE__
    unsigned t;                 // (spelled out: from the expression below hipcc makes the count, a compare and a select)
    asm("v_ffbh_u32 %0, %1" : "=v"(t) : "v"(a));
#else
    unsigned t = a ? (unsigned)__builtin_clz(a) : 0xffffffffu;
#endif
    t = t < 41u ? t : 41u;
    const int e = mdct_min_i32((int)t + shift - 8, 24);
    c = e == 24 ? 0 : c;
    return e;
}

// The twiddle of a group's first butterfly.  The reference skips the multiply there; cos[0] is 32767 after the Q15 clamp, so
// multiplying by the table's entry would not.  (32768, 0) does: (32768 q + 0 r) >> 15 == q for every 16-bit q and r, and
// 32768 fits the 24-bit multiplier.
constexpr int MDCT_TW_ONE_RE = 32768, MDCT_TW_ONE_IM = 0;

}  // namespace ac3mi
