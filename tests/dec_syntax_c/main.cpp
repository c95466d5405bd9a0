/* csrc/dec_syntax.h on the host, for tests/test_dec_syntax_cpu.py: built without HIP, with -fsanitize=address,undefined, and run
 * on its own (never loaded into Python).  The decoder's field lists - dsyn_frame, dsyn_block_a, dsyn_block_b, dsyn_skip_field -
 * over a reader of a byte buffer (bits past its end read as zeros, as the kernels' padding does), a plain-struct state whose
 * setters abort on a value that would not fit the field St (decode_common.h) packs it into or on a slot outside its array,
 * and a sink that records what the kernels' sinks are handed.  It cannot skip mantissas: it reads a block where it is told to.
 *   dec_syntax FILE      one frame per line of FILE:
 *     F lfeon flags hex s0 s1 s2 s3 s4 s5    the header (expected lfeon, requested output flags), then the six blocks from
 *                                            bit positions s0..s5
 *     D lfeon flags hex                      the header and block 0 where the header ends (damaged frames)
 *   Output, name=value: a line `hdr` per frame (out: the granted output or -1, at: the bit behind the BSI), then a line per
 *   block read:
 *     err    0: read to the end, else the exit the lists took: 1 acmod < 2 coupled, 2 cplendf + 3 - cplbegf < 0, 3 chbwcod > 60,
 *            4 a deltba segment that reaches band 50               end     the bit behind the skip field (-1 with err)
 *     blksw dith chincpl (bit ch)  phs cplstrt cplend ncplbnd strc (cplbndstrc)  remat  the state behind the block
 *     exps   slot:strategy:groups:absexp:bit position of the first group, per exponent field in bitstream order
 *     endm bai csnr cbai fleak sleak deltbae                     the state; cbai by slot 0..6, deltbae by slot 0..5 (5: coupling)
 *     deltba the six rows of 50 bands, a hex digit delta + 8 per band
 *     dyn    code:programme per dynamic-range word read         co      ch:band:exponent:mantissa:master per coordinate
 *     flips  coupling bands whose phase flag was set            reuse0  the block-0 flag */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "dec_syntax.h"

using namespace ac3mi;

[[noreturn]] static void die(const char *what, long a, long b)
{
    fprintf(stderr, "dec_syntax: %s (%ld, %ld)\n", what, a, b);
    abort();
}

struct HostRd {
    const uint8_t *p;
    uint32_t nbits, at;
    int last_n;             // the last field read: its width and value
    uint32_t last_v;
    uint32_t get(int n)
    {
        if (n < 0 || n > 32) die("a field's width", n, at);
        uint32_t v = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t b = at + (uint32_t)i;
            v = (v << 1) | (b < nbits ? (uint32_t)(p[b >> 3] >> (7 - (b & 7u))) & 1u : 0u);
        }
        at += (uint32_t)n;
        last_n = n;
        last_v = v;
        return v;
    }
    int32_t sget(int n)
    {
        const uint32_t v = get(n);
        return ((int32_t)(v << (32 - n))) >> (32 - n);
    }
    uint32_t pos() const { return at; }
    void skip(uint32_t n) { at += n; }
};

// St's accessor names over plain members; `bits`: the width St packs the field into (0: a plain member there)
struct HostState {
#define HS_FIELD(type, name, bits) \
    type name##_ = 0; \
    type name() const { return name##_; } \
    void set_##name(type v) { if (bits && ((long)v < 0 || (long)v >= (1l << bits))) die("a value too wide for St's " #name, (long)v, bits); name##_ = v; }
    HS_FIELD(int, lfeon, 0) HS_FIELD(int, nf, 0) HS_FIELD(int, output, 0) HS_FIELD(int, chincpl, 0) HS_FIELD(int, cplstrtmant, 0)
    HS_FIELD(uint32_t, cplbndstrc, 0) HS_FIELD(float, clev, 0) HS_FIELD(float, slev, 0) HS_FIELD(float, level, 0) HS_FIELD(float, dynrng, 0)
    HS_FIELD(int, phsflginu, 1) HS_FIELD(int, ncplbnd, 5) HS_FIELD(int, cplstrtbnd, 6) HS_FIELD(int, cplfleak, 4) HS_FIELD(int, cplsleak, 4)
    HS_FIELD(int, rematflg, 4) HS_FIELD(int, dynrnge, 1) HS_FIELD(int, bai, 11) HS_FIELD(int, csnroffst, 6)
#undef HS_FIELD
#define HS_SLOTS(name, n, bits) \
    int name##_[n] = {}; \
    int name(int k) const { if (k < 0 || k >= n) die("slot of " #name, k, n); return name##_[k]; } \
    void set_##name(int k, int v) { if (k < 0 || k >= n) die("slot of " #name, k, n); if (v < 0 || v >= (1 << bits)) die("a value too wide for St's " #name, v, bits); name##_[k] = v; }
    HS_SLOTS(endm, 7, 8) HS_SLOTS(cbai, 7, 7) HS_SLOTS(deltbae, 6, 2)
#undef HS_SLOTS
    void reset_deltbae() { for (int i = 0; i < 6; i++) deltbae_[i] = 2; }
};

struct HostSink {
    int8_t deltba[6][50];
    std::string exps, dyn, co;
    int flips = 0;
    HostSink() { memset(deltba, 0, sizeof deltba); }
    void begin_block() { exps.clear(); dyn.clear(); co.clear(); flips = 0; }
    static void add(std::string &s, const char *fmt, int a, int b, int c = 0, int d = 0, int e = 0)
    {
        char t[96];
        snprintf(t, sizeof t, fmt, a, b, c, d, e);
        if (!s.empty()) s += ';';
        s += t;
    }
    float dynrng(int code, int word, bool apply)
    {
        if (code < -128 || code > 127 || word < 0 || word > 1) die("a dynamic-range word", code, word);
        add(dyn, "%d:%d", code & 0xff, word);
        // parse.c:587-595
        return apply ? ldexpf((float)(((code & 0x1f) | 0x20) << 13), -(15 + 3 - (code >> 5))) : 0.f;
    }
    void cplco(int ch, int bnd, int ex, int ma, int master)
    {
        if (ch < 0 || ch >= 5 || bnd < 0 || bnd >= 18 || ex < 0 || ex > 15 || ma < 0 || ma > 15 || master < 0 || master > 9) die("a coupling coordinate", ch, bnd);
        add(co, "%d:%d:%d:%d:%d", ch, bnd, ex, ma, master);
    }
    void cplco_flip(int bnd)
    {
        if (bnd < 0 || bnd >= 18) die("a phase flag's band", bnd, 0);
        flips++;
    }
    int exponents(int slot, int es, int ngrp, int e0, int start, uint32_t pos)
    {
        // (the rows hold 256 bins: read_exponents writes 3 ngrp values, each 1, 2 or 4 times, from `start` or from bin 1)
        if (slot < 0 || slot > 6 || es < 1 || es > 3 || ngrp < 0 || (slot == 6 ? start : 1) + 3 * ngrp * (1 << (es - 1)) > 256) die("an exponent field", slot, ngrp);
        add(exps, "%d:%d:%d:%d:%d", slot, es, ngrp, e0, (int)pos);
        return 0;
    }
    void deltba_clear(int slot)
    {
        if (slot < 0 || slot >= 6) die("a deltba row", slot, 0);
        memset(deltba[slot], 0, 50);
    }
    void deltba_seg(int slot, int band, int len, int d)
    {
        if (slot < 0 || slot >= 6 || band < 0 || len < 1 || band + len > 50 || d < -4 || d > 4 || d == 0) die("a deltba segment", band, len);
        for (int i = 0; i < len; i++) deltba[slot][band + i] = (int8_t)d;
    }
    void lap(int point) { if (point < 0 || point > 2) die("a lap", point, 0); }
};

static std::vector<uint8_t> unhex(const char *h)
{
    std::vector<uint8_t> v;
    for (; h[0] && h[1]; h += 2) {
        unsigned x;
        if (sscanf(h, "%2x", &x) != 1) die("hex", 0, 0);
        v.push_back((uint8_t)x);
    }
    return v;
}

// one block from rd's position
static int read_block(HostRd &rd, HostState &st, HostSink &k, int blk, int acmod)
{
    DsynBlock b;
    k.begin_block();
    const int nf = st.nf(), lfeon = st.lfeon();
    int err = dsyn_block_a(rd, st, k, b, blk, acmod, nf, lfeon);
    if (!err) err = dsyn_block_b(rd, st, k, b, blk, nf, lfeon);
    if (!err) dsyn_skip_field(rd);
    // which of the lists' four exits a refusal took, by the last field read: chbwcod (6 bits, above 60), a deltba segment's delta
    // (3 bits), cplendf (4 bits), chincpl (nf = 1 or 2 bits: acmod < 2).  (This sink reports no exponent errors.)
    if (err) err = rd.last_n == 6 ? 3 : rd.last_n == 3 ? 4 : rd.last_n == 4 ? 2 : 1;
    if ((err == 3 && rd.last_v <= 60) || (err == 1 && (acmod >= 2 || rd.last_n != nf))) die("a refusal behind an unexpected field", rd.last_n, rd.last_v);
    printf("blk=%d err=%d end=%d blksw=%d dith=%d chincpl=%d phs=%d cplstrt=%d cplend=%d ncplbnd=%d strc=%u remat=%d", blk, err,
           err ? -1 : (int)rd.pos(), b.blkswm, b.dithmask, st.chincpl(), st.phsflginu(), st.cplstrtmant(), st.endm(6), st.ncplbnd(), st.cplbndstrc(), st.rematflg());
    printf(" exps=%s endm=%d,%d,%d,%d,%d bai=%d csnr=%d cbai=%d,%d,%d,%d,%d,%d,%d fleak=%d sleak=%d deltbae=%d,%d,%d,%d,%d,%d deltba=", k.exps.c_str(),
           st.endm(0), st.endm(1), st.endm(2), st.endm(3), st.endm(4), st.bai(), st.csnroffst(), st.cbai(0), st.cbai(1), st.cbai(2), st.cbai(3),
           st.cbai(4), st.cbai(5), st.cbai(6), st.cplfleak(), st.cplsleak(), st.deltbae(0), st.deltbae(1), st.deltbae(2), st.deltbae(3),
           st.deltbae(4), st.deltbae(5));
    for (int s = 0; s < 6; s++) {
        for (int i = 0; i < 50; i++) printf("%x", k.deltba[s][i] + 8);
        if (s < 5) printf(",");
    }
    printf(" dyn=%s co=%s flips=%d reuse0=%d redo=%d\n", k.dyn.c_str(), k.co.c_str(), k.flips, b.reuse0, b.redo);
    return err;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    static char line[16384];
    while (fgets(line, sizeof line, f)) {
        char kind = 0;
        int lfeon = 0, flags = 0, used = 0;
        static char hex[8192];
        if (sscanf(line, " %c %d %d %8191s%n", &kind, &lfeon, &flags, hex, &used) != 4) die("a line of the input", 0, 0);
        const std::vector<uint8_t> bytes = unhex(hex);
        if (bytes.size() < 8) die("a frame of fewer than 8 bytes", (long)bytes.size(), 0);
        HostRd rd{bytes.data(), (uint32_t)(8 * bytes.size()), 6 * 8 + 3, 0, 0};
        HostState st;
        HostSink k;
        st.set_dynrnge(1);
        const int acmod = (bytes[6] >> 5) & 7;
        const DsynRequest q{lfeon, flags, 1.0f, 1};
        const int out = dsyn_frame(rd, st, acmod, q);
        printf("hdr out=%d at=%d acmod=%d nf=%d lfeon=%d clev=%.9g slev=%.9g level=%.9g\n", out, (int)rd.pos(), acmod, st.nf(), st.lfeon(), st.clev(),
               st.slev(), st.level());
        if (out < 0) continue;
        if (kind == 'F') {
            const char *p = line + used;
            for (int blk = 0; blk < 6; blk++) {
                int at = 0, n = 0;
                if (sscanf(p, " %d%n", &at, &n) != 1) die("a block's start", blk, 0);
                p += n;
                rd.at = (uint32_t)at;
                read_block(rd, st, k, blk, acmod);
            }
        } else read_block(rd, st, k, 0, acmod);
    }
    fclose(f);
    return 0;
}
