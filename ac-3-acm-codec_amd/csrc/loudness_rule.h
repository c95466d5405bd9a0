// loudness_rule.h — the parts of the BS.1770 meter (ac3mi_loudness_*, include/ac3mi.h) that need no GPU: the state's layout,
// the frozen K-weighting coefficients, the bin-edge and dialnorm tables, and the three decisions - a block's bin, the gated
// read-out of the bins, the dialnorm word - as __host__ __device__ functions that loudness_kernel / loudness_read_kernel
// (loudness.hip) and the host twin ac3mi_loudness_read both call.  No decision uses a logarithm: blocks and means are
// compared as energies against tables built once on the host in double.
// Plain C++: compiles without HIP (a host-only build of loudness.hip for the sanitiser program of tests/loudness_c).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/ac3mi.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

constexpr int LOUD_BINS = 900;          // 0.1 LU each over [-70, +20) LKFS
constexpr int LOUD_SEG = 24;            // sample instants a lane owns in a frame: 64 x 24 = 1536

// One stream's state (ac3mi_loudness_state_bytes() = sizeof): all zeros is a new stream.
struct LoudState {
    double bq[6][4];                    // per input slot: shelf s1, s2, high-pass s1, s2 (transposed direct form II)
    double hop_sum;                     // the open hop's energy so far
    double hops[3];                     // the last three closed hops, oldest first
    double max_block;                   // the largest block energy z seen
    uint32_t pos;                       // samples in the open hop
    uint32_t hop_count;                 // closed hops (a block per hop from the fourth on)
    uint32_t blocks, blocks_abs;        // blocks formed, and those at or above the absolute gate
    uint32_t count[LOUD_BINS];          // per bin: the blocks in it
    double sum[LOUD_BINS];              // ... and their energies, added in time order
};
static_assert(sizeof(LoudState) == 11048 && offsetof(LoudState, sum) % 8 == 0, "LoudState layout");

// K-weighting, frozen: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (a0 = 1) from the bilinear design of include/ac3mi.h,
// evaluated in double; the 48 kHz row is BS.1770's table to its printed digits.  nullptr: not a rate the meter takes
inline const double *loud_coefs(int sample_rate)
{
    static const double C48[10] = {1.5351248595869702, -2.6916961894063807, 1.19839281085285, -1.6906592931824103, 0.7324807742158501,
                                   1.0, -2.0, 1.0, -1.9900474548339797, 0.9900722503662099};
    static const double C44[10] = {1.5308412300503478, -2.6509799951547297, 1.169079079921587, -1.6636551132560204, 0.7125954280732254,
                                   1.0, -2.0, 1.0, -1.989169673629796, 0.9891990357870393};
    static const double C32[10] = {1.5111778995687646, -2.464889413360141, 1.0416332735222955, -1.5390450962506403, 0.626966855981559,
                                   1.0, -2.0, 1.0, -1.9850896689886883, 0.9851453206695515};
    return sample_rate == 48000 ? C48 : sample_rate == 44100 ? C44 : sample_rate == 32000 ? C32 : nullptr;
}

// E_b = 10^((-70 + 0.1 b + 0.691) / 10), b = 0..900: bin b holds the blocks with E_b <= z < E_(b+1)
inline void loud_build_edges(double *edges901)
{
    for (int b = 0; b <= LOUD_BINS; b++) edges901[b] = pow(10.0, (-70.0 + 0.1 * b + 0.691) / 10.0);
}

// T_d = 10^((-d - 0.5 + 0.691) / 10) at [d - 1], d = 1..30: a mean below T_d is quieter than -(d + 0.5) LKFS
inline void loud_build_dialnorm(double *thr30)
{
    for (int d = 1; d <= 30; d++) thr30[d - 1] = pow(10.0, (-d - 0.5 + 0.691) / 10.0);
}

// The cascade as a linear system on v = (s1, s2, t1, t2): v' = A v + B x, y = C v + D x with
//   y1 = b0 x + s1, s1' = b1 x - a1 y1 + s2, s2' = b2 x - a2 y1;  y = y1 + t1, t1' = -2 y1 - c1 y + t2, t2' = y1 - c2 y.
// For the segmented kernel: M[k] = A^(24 2^k) (row-major 4 x 4, k = 0..5) and Z[n] = C A^n (n = 0..23), the zero-input response.
inline void loud_build_segment(const double *coef, double M[6][16], double Z[LOUD_SEG][4])
{
    const double a1 = coef[3], a2 = coef[4], c1 = coef[8], c2 = coef[9];
    const double A[16] = {-a1, 1, 0, 0, -a2, 0, 0, 0, -2 - c1, 0, -c1, 1, 1 - c2, 0, -c2, 0};
    auto mul = [](const double *x, const double *y, double *o) {
        double t[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) t[4 * r + c] = x[4 * r] * y[c] + x[4 * r + 1] * y[4 + c] + x[4 * r + 2] * y[8 + c] + x[4 * r + 3] * y[12 + c];
        memcpy(o, t, sizeof t);
    };
    double P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};      // A^n
    for (int n = 0; n < LOUD_SEG; n++) {
        for (int c = 0; c < 4; c++) Z[n][c] = P[c] + P[8 + c];              // C = (1, 0, 1, 0)
        mul(A, P, P);
    }
    memcpy(M[0], P, sizeof P);
    for (int k = 1; k < 6; k++) mul(M[k - 1], M[k - 1], M[k]);
}

// A block's bin: -1 below the absolute gate (z < E_0, or not a number), else the b with E_b <= z < E_(b+1), 899 from E_900 on
__host__ __device__ inline int loud_bin(const double *edges, double z)
{
    if (!(z >= edges[0])) return -1;
    int lo = 0, hi = LOUD_BINS;                         // edges[lo] <= z, and the answer is below hi
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (z >= edges[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Read-out, first pass: the sums and counts of bins first, first + stride, ... (the host: 0 and 1; a lane: itself and 64)
__host__ __device__ inline void loud_total_part(const LoudState *st, int first, int stride, double *sum, uint32_t *count)
{
    double s = 0;
    uint32_t n = 0;
    for (int b = first; b < LOUD_BINS; b += stride) {
        s += st->sum[b];
        n += st->count[b];
    }
    *sum = s;
    *count = n;
}

// The relative gate: -10 LU under the mean of everything above the absolute gate (no such block: 0, and no bin has blocks)
__host__ __device__ inline double loud_gamma(double sum, uint32_t count) { return count ? 0.1 * (sum / (double)count) : 0.0; }

// ... a bin counts whole if its lower edge is at or above the gate; the one bin the gate cuts counts whole iff its own mean
// is at or above the gate; every other bin is out
__host__ __device__ inline bool loud_bin_included(const LoudState *st, const double *edges, int b, double gamma)
{
    const uint32_t n = st->count[b];
    if (!n) return false;
    if (edges[b] >= gamma) return true;
    if (edges[b + 1] > gamma) return st->sum[b] / (double)n >= gamma;
    return false;
}

// ... second pass: the same walk over the bins that count
__host__ __device__ inline void loud_gated_part(const LoudState *st, const double *edges, double gamma, int first, int stride,
                                                double *sum, uint32_t *count)
{
    double s = 0;
    uint32_t n = 0;
    for (int b = first; b < LOUD_BINS; b += stride)
        if (loud_bin_included(st, edges, b, gamma)) {
            s += st->sum[b];
            n += st->count[b];
        }
    *sum = s;
    *count = n;
}

// round-half-up of -lkfs, clamped to 1..31, decided on energies: 1 + the number of d in 1..30 with mean < T_d
__host__ __device__ inline int loud_dialnorm(const double *thr30, double mean_energy)
{
    int dn = 1;
    for (int d = 0; d < 30; d++) dn += mean_energy < thr30[d] ? 1 : 0;
    return dn;
}

// ... and the record, from the gated totals and the state's counters
__host__ __device__ inline void loud_result(const LoudState *st, const double *thr30, double sum, uint32_t count, ac3mi_loudness_result *out)
{
    ac3mi_loudness_result r;
    r.max_block_energy = st->max_block;
    r.blocks = st->blocks;
    r.blocks_abs = st->blocks_abs;
    r.blocks_rel = count;
    for (int i = 0; i < 6; i++) r.reserved[i] = 0;
    if (count) {
        r.mean_energy = sum / (double)count;
        r.lkfs = (float)(-0.691 + 10.0 * log10(r.mean_energy));
        r.dialnorm = (uint8_t)loud_dialnorm(thr30, r.mean_energy);
        r.flags = 0;
    } else {
        r.mean_energy = 0.0;
        r.lkfs = -70.0f;
        r.dialnorm = 31;
        r.flags = AC3MI_LOUDNESS_EMPTY;
    }
    *out = r;
}

// The whole read-out on a state in host memory (any alignment)
inline void loudness_read_host(const void *h_state, ac3mi_loudness_result *out)
{
    static const struct Tables {
        double edges[LOUD_BINS + 1], thr[30];
        Tables() { loud_build_edges(edges); loud_build_dialnorm(thr); }
    } T;
    LoudState *st = new LoudState;
    memcpy(st, h_state, sizeof *st);
    double s;
    uint32_t n;
    loud_total_part(st, 0, 1, &s, &n);
    const double gamma = loud_gamma(s, n);
    loud_gated_part(st, T.edges, gamma, 0, 1, &s, &n);
    loud_result(st, T.thr, s, n, out);
    delete st;
}

}  // namespace ac3mi
