/* csrc/mdct_rule.h on the host, for tests/test_mdct_rule_cpu.py: built without HIP, with -fsanitize=address,undefined, and run
 * on its own (never loaded into Python).
 *   exponent   mdct_raw_exp against the expression it replaced in enc_mdct_kernel (|c|, the zero's case, 23 - log2 + shift, the
 *              clamp to 24 that zeroes the coefficient), restated here: every c with |c| < 2^18, both signs, every v in 0..14
 *              (shift = v - 9) - the exponent as a signed value, its low byte as the row stores it, and the coefficient left
 *   magnitude  mdct_mag8 against the loop of maxima of |w| it replaced: random 8-tuples of 16-bit and of 31-bit values, tuples
 *              of one sign, and every tuple over the extremes {-32768, -32767, -1, 0, 1, 32767}
 *   twiddle    (32768 q) >> 15 == q and (32768 q + 0 r) >> 15 == q, (32768 q - 0 r) >> 15 == q for every 16-bit q (r drawn), with
 *              the products taken as the 24-bit multiplier takes them
 *   mdct_rule SEED */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "mdct_rule.h"

using namespace ac3mi;

static uint64_t g_rng;
static uint32_t rnd()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// av_log2 as the kernel's ilog2u states it
static int ilog2u(unsigned v) { return v ? 31 - __builtin_clz(v) : 0; }

// the block loop's exponent of one coefficient before the rule: returns e, rewrites c
static int old_exp(int &c, int shift)
{
    const int a = c < 0 ? -c : c;
    int e;
    if (a == 0) e = 24;
    else {
        e = 23 - ilog2u((unsigned)a) + shift;
        if (e >= 24) { e = 24; c = 0; }
    }
    return e;
}

static long check_exponent()
{
    long n = 0, zeroed = 0, negative = 0;
    for (int v = 0; v <= 14; v++)
        for (int c = -(1 << 18) + 1; c < (1 << 18); c++) {
            int c0 = c, c1 = c;
            const int e0 = old_exp(c0, v - 9), e1 = mdct_raw_exp(c1, v - 9);
            CHECK(e0 == e1 && (e0 & 0xff) == (e1 & 0xff) && c0 == c1, "exponent: c=%d v=%d: %d / %d, coefficient %d / %d", c, v, e0, e1, c0, c1);
            CHECK(e1 <= 24 && (e1 == 24) == (c1 == 0), "exponent: c=%d v=%d: e=%d with coefficient %d", c, v, e1, c1);
            zeroed += c != 0 && c1 == 0;
            negative += e1 < 0;
            n++;
        }
    CHECK(zeroed > 0 && negative > 0, "exponent: the range holds no zeroed coefficient or no negative exponent");
    return n;
}

static int old_mag8(const int (&w)[8])
{
    int acc = 0;
    for (int k = 0; k < 8; k++) {
        const int m = w[k] > -w[k] ? w[k] : -w[k];
        acc = acc > m ? acc : m;
    }
    return acc;
}

static long check_magnitude()
{
    long n = 0;
    int w[8];
    for (int i = 0; i < 200000; i++) {
        const int kind = i % 5;
        for (int k = 0; k < 8; k++) {
            const int r16 = (int)(int16_t)rnd(), r31 = (int)(rnd() & 0x7fffffffu) * ((rnd() & 1) ? 1 : -1);
            w[k] = kind == 0 ? r16 : kind == 1 ? r31 : kind == 2 ? -(r16 < 0 ? -r16 : r16) - 1 : kind == 3 ? (r16 < 0 ? -r16 : r16) : r16 >> (rnd() % 16);
        }
        CHECK(mdct_mag8(w) == old_mag8(w), "magnitude: drawn tuple %d", i);
        n++;
    }
    static const int ext[6] = {-32768, -32767, -1, 0, 1, 32767};
    for (int code = 0; code < 6 * 6 * 6 * 6 * 6 * 6 * 6 * 6; code++) {
        int c = code;
        for (int k = 0; k < 8; k++) { w[k] = ext[c % 6]; c /= 6; }
        CHECK(mdct_mag8(w) == old_mag8(w), "magnitude: extreme tuple %d", code);
        n++;
    }
    return n;
}

// a product as v_mul_i32_i24 forms it: both factors sign-extended from their low 24 bits, the low 32 bits of the product
static int mul24(int a, int b)
{
    const int64_t x = (int64_t)((int32_t)((uint32_t)a << 8) >> 8), y = (int64_t)((int32_t)((uint32_t)b << 8) >> 8);
    return (int)(uint32_t)(uint64_t)(x * y);
}

static long check_twiddle()
{
    long n = 0;
    for (int q = -32768; q <= 32767; q++) {
        const int r = (int)(int16_t)rnd();
        const int c = MDCT_TW_ONE_RE, s = MDCT_TW_ONE_IM;
        CHECK(mul24(c, q) >> 15 == q, "twiddle: 32768 * %d", q);
        CHECK((mul24(c, q) - mul24(s, r)) >> 15 == q && (mul24(c, q) + mul24(r, s)) >> 15 == q, "twiddle: q=%d r=%d", q, r);
        n++;
    }
    return n;
}

int main(int argc, char **argv)
{
    g_rng = argc > 1 ? (uint64_t)atoll(argv[1]) : 1;
    printf("exponent ok checked=%ld\n", check_exponent());
    printf("magnitude ok checked=%ld\n", check_magnitude());
    printf("twiddle ok checked=%ld\n", check_twiddle());
    return 0;
}
