/* csrc/enc_syntax.h on the host, for tests/test_enc_syntax_cpu.py: built without HIP, with -fsanitize=address,undefined, and run
 * on its own (never loaded into Python).  Walks the shapes the encoder can be asked for - every acmod with and without the
 * LFE; the reference's BSI, a metadata word, compr words absent or present per programme; block switching; dynrng words in
 * none, some or all blocks per programme; rematrixing absent or with flags in any subset of blocks 1..5; coupling off or at
 * cplbegf 0, 2, 3 with cplendf 12 or 7; exponent strategies all D15, block 0 only, and DRAWS seeded draws per row - and writes
 * each as a frame of side information alone: exponents of zeros, offsets of zero, no mantissas.  The writing sink is
 * SynWriter over a byte buffer; it aborts where a field would take the accumulator past 64 pending bits.
 * One line per case, name=value: what was put in, then
 *     hdr=written,counted,closed   the header's bits: the sink's position, SynCounter, syn_header_bits
 *     blk=..  cnt=..  closed=..    the same for the six blocks (closed: syn_block_bits, -1 for a coupled frame)
 *     fixed=                       the search's sum for the case: syn_priced_fixed (+ syn_priced_cpl) and the frame's own terms
 *     expbits=                     4 + 7 groups over the channels' exponent sets (what the search adds from exp_stage)
 *     hex=                         the frame up to the last bit written (cases of the first STRATS_READ strategy patterns)
 *   enc_syntax SEED DRAWS STRATS_READ
 *   enc_syntax groups              the exponent group counts instead (print_groups) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "launch_rule.h"
#include "enc_syntax.h"

using namespace ac3mi;

static long g_case = 0;

struct HostSink : SynWriter<HostSink> {
    uint8_t buf[4096];
    HostSink() { memset(buf, 0, sizeof buf); }
    void put(int n, uint32_t v)
    {
        if (n < 0 || n > 32 || nacc + n > 64 || (n < 32 && (v >> n) != 0)) {
            fprintf(stderr, "case %ld: a field of %d bits, value %u, at bit %u with %d bits pending\n", g_case, n, v, pos + (uint32_t)nacc, nacc);
            abort();
        }
        SynWriter<HostSink>::put(n, v);
    }
    void store(uint32_t at, int n, uint32_t v)
    {
        for (int i = 0; i < n; i++) {
            const uint32_t p = at + (uint32_t)i;
            if (p >= 8 * sizeof buf) { fprintf(stderr, "case %ld: bit %u beyond the buffer\n", g_case, p); abort(); }
            buf[p >> 3] |= (uint8_t)(((v >> (n - 1 - i)) & 1u) << (7 - (p & 7u)));
        }
    }
    // exponents of zeros: absolute exponent 0, every differential 0 -> group code (2 * 5 + 2) * 5 + 2.  The sequence put(4) -
    // flush - groups is PackSink::exponents' (encode.hip): the bound proved here is the device's while the two keep the same flush
    void exponents(int, int, int ng)
    {
        put(4, 0);
        flush();
        for (int g = 0; g < ng; g++) store(pos + 7u * (uint32_t)g, 7, 62);
        pos += 7u * (uint32_t)ng;
    }
};

struct Case {
    int acmod, lfe, nfbw, nch;
    uint32_t m, compr[2];
    uint32_t bsw[6];            // bit ch: blksw
    uint32_t dyn[6][2];         // bit 8: sent
    int remat_on;               // the rematrixing tool (2/0)
    uint32_t remat[6];
    uint32_t cplw;
    int begf, endf;
    uint32_t co[5][16], cstrat[6];
    uint32_t strat[6][6];
    uint32_t chbwcod, csnr, fsnr, fscod, frmsizecod;
};

static uint32_t g_lcg;
static uint32_t rnd(uint32_t n) { g_lcg = g_lcg * 1664525u + 1013904223u; return (g_lcg >> 8) % n; }

template <class K> static void emit_header(K &k, const Case &c)
{
    syn_header(k, c.fscod, c.frmsizecod, 8, c.acmod, c.lfe != 0, c.acmod == 0, c.m, c.compr[0], c.compr[1]);
}
template <class K> static void emit_block(K &k, const Case &c, int b)
{
    const SynShape s{c.acmod, c.nfbw, c.nch, c.lfe != 0, c.acmod == 0, 73 + 3 * (int)c.chbwcod, c.chbwcod};
    syn_block(k, s, SynCpl{c.cplw, c.begf, c.endf, c.cstrat[b]}, b, [&](int ch) { return (c.bsw[b] >> ch) & 1u; },
              [&](int p) { return c.dyn[b][p]; }, c.remat_on ? c.remat[b] : b == 0 ? 0x10u : 0u, [&](int ch) { return c.strat[b][ch]; },
              [&](int ch, int bd) { return c.co[ch][bd]; }, c.csnr, c.fsnr);
}

static void run(const Case &c, bool with_hex)
{
    HostSink w;
    SynCounter hc;
    emit_header(w, c);
    emit_header(hc, c);
    if (w.nacc != 0) { fprintf(stderr, "case %ld: the header leaves %d bits pending\n", g_case, w.nacc); abort(); }
    const uint32_t hdr = w.pos;
    uint32_t blk[6];
    int cnt[6], closed[6], exp_rows = 0, dyn_words = 0, remat_blocks = 0, cpl_ebits = 0, expbits = 0;
    const bool cplf = (c.cplw & 1u) != 0;
    const int nbc = 73 + 3 * (int)c.chbwcod, cs = 37 + 12 * c.begf, ce = 73 + 12 * c.endf;
    for (int b = 0; b < 6; b++) {
        const uint32_t at = w.pos;
        SynCounter sc;
        emit_block(w, c, b);
        emit_block(sc, c, b);
        if (w.nacc != 0) { fprintf(stderr, "case %ld: block %d leaves %d bits pending\n", g_case, b, w.nacc); abort(); }
        blk[b] = w.pos - at;
        cnt[b] = sc.bits;
        const SynShape s{c.acmod, c.nfbw, c.nch, c.lfe != 0, c.acmod == 0, nbc, c.chbwcod};
        closed[b] = cplf ? -1 : syn_block_bits(s, b, c.dyn[b][0], c.acmod == 0 ? c.dyn[b][1] : 0u, c.remat_on ? c.remat[b] : b == 0 ? 0x10u : 0u,
                                               [&](int ch) { return c.strat[b][ch]; });
        // the integers enc_search_kernel forms from its ballots and arrays
        for (int ch = 0; ch < c.nch; ch++) {
            const int st = (int)c.strat[b][ch];
            if (!st) continue;
            const bool is_lfe = c.lfe && ch == c.nch - 1;
            if (!is_lfe) exp_rows++;
            expbits += 4 + 7 * syn_exp_groups(is_lfe ? 7 : cplf ? cs : nbc, st);
        }
        for (int p = 0; p < (c.acmod == 0 ? 2 : 1); p++) dyn_words += (c.dyn[b][p] & 0x100u) ? 1 : 0;
        if (b > 0 && c.remat_on && (c.remat[b] & 0x10u)) remat_blocks++;
        if (cplf && c.cstrat[b]) cpl_ebits += 4 + 7 * syn_cpl_exp_groups(cs, ce, (int)c.cstrat[b]);
    }
    const int compr_words = ((c.compr[0] & 0x100u) ? 1 : 0) + ((c.compr[1] & 0x100u) ? 1 : 0);
    // the search's sum, formed as enc_search_kernel forms it: the layout's part, then what the frame adds
    int fixed = syn_priced_fixed(c.acmod, c.lfe != 0, c.nfbw, c.nch) + 8 * exp_rows + 8 * (dyn_words + compr_words) + 4 * remat_blocks;
    if (cplf) fixed += syn_priced_cpl(c.acmod, c.nfbw, 3 + c.endf - c.begf) + cpl_ebits - 6 * exp_rows - (4 - syn_cpl_nrem(c.begf)) * remat_blocks;
    printf("acmod=%d lfe=%d m=%u compr=%u,%u chbwcod=%u csnr=%u fsnr=%u fscod=%u frmsizecod=%u remat_on=%d cplw=%u begf=%d endf=%d", c.acmod, c.lfe, c.m,
           c.compr[0], c.compr[1], c.chbwcod, c.csnr, c.fsnr, c.fscod, c.frmsizecod, c.remat_on, c.cplw, c.begf, c.endf);
    printf(" bsw=");
    for (int b = 0; b < 6; b++) printf("%u%s", c.bsw[b], b < 5 ? "," : "");
    printf(" dyn=");
    for (int b = 0; b < 6; b++) printf("%u,%u%s", c.dyn[b][0], c.dyn[b][1], b < 5 ? "," : "");
    printf(" remat=");
    for (int b = 0; b < 6; b++) printf("%u%s", c.remat[b], b < 5 ? "," : "");
    printf(" cstrat=");
    for (int b = 0; b < 6; b++) printf("%u%s", c.cstrat[b], b < 5 ? "," : "");
    printf(" strat=");
    for (int b = 0; b < 6; b++)
        for (int ch = 0; ch < c.nch; ch++) printf("%u", c.strat[b][ch]);
    printf(" co=");
    for (int ch = 0; ch < 5; ch++)
        for (int bd = 0; bd < 16; bd++) printf("%02x", c.co[ch][bd]);
    printf(" hdr=%u,%d,%d blk=", hdr, hc.bits, syn_header_bits(c.acmod, c.compr[0], c.compr[1]));
    for (int b = 0; b < 6; b++) printf("%u%s", blk[b], b < 5 ? "," : "");
    printf(" cnt=");
    for (int b = 0; b < 6; b++) printf("%d%s", cnt[b], b < 5 ? "," : "");
    printf(" closed=");
    for (int b = 0; b < 6; b++) printf("%d%s", closed[b], b < 5 ? "," : "");
    printf(" fixed=%d expbits=%d end=%u hex=", fixed, expbits, w.pos);
    if (with_hex)
        for (uint32_t i = 0; i < (w.pos + 7) / 8; i++) printf("%02x", w.buf[i]);
    printf("\n");
    g_case++;
}

// syn_exp_groups for every n a row can have and syn_cpl_exp_groups for every range ac3mi_set_encode_coupling / _bandwidth can
// produce, per strategy: "ch n strat groups" and "cpl cs ce strat groups" lines
static int print_groups()
{
    for (int n = 1; n <= 253; n++)
        for (int s = 1; s <= 3; s++) printf("ch %d %d %d\n", n, s, syn_exp_groups(n, s));
    for (int begf = 0; begf <= 12; begf++)
        for (int endf = 0; endf <= 12; endf++) {
            const int cs = 37 + 12 * begf, ce = 73 + 12 * endf;
            if (cs >= ce) continue;
            for (int s = 1; s <= 3; s++) printf("cpl %d %d %d %d\n", cs, ce, s, syn_cpl_exp_groups(cs, ce, s));
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "groups")) return print_groups();
    if (argc != 4) return 2;
    g_lcg = (uint32_t)strtoul(argv[1], nullptr, 10);
    const int draws = atoi(argv[2]), strats_read = atoi(argv[3]);
    static const int nf[8] = {2, 1, 2, 3, 3, 4, 4, 5};
    static const int cpl_at[7][2] = {{-1, 12}, {0, 12}, {2, 12}, {3, 12}, {0, 7}, {2, 7}, {3, 7}};
    for (int acmod = 0; acmod < 8; acmod++)
        for (int lfe = 0; lfe < 2; lfe++) {
            const bool dual = acmod == 0;
            const int np = dual ? 2 : 1;
            // metadata: the reference's word; a drawn word; then compr words present in every non-empty set of programmes
            for (int meta = 0; meta < 2 + (dual ? 3 : 1); meta++)
                for (int bswon = 0; bswon < 2; bswon++)
                    for (int dynpat = 0; dynpat < (dual ? 9 : 3); dynpat++)
                        // rematrixing (2/0): absent, then rematstr in every subset of blocks 1..5.  Only absent / none / all are
                        // crossed with everything else; the other subsets take one combination of the other tools each
                        for (int rem = 0; rem < (acmod == 2 ? 33 : 1); rem++)
                            for (int cp = 0; cp < (acmod >= 2 ? 7 : 1); cp++) {
                                const bool corner = rem == 0 || rem == 1 || rem == 32;
                                if (!corner && (meta != rem % 3 || bswon != rem % 2 || dynpat != rem % 3)) continue;
                                for (int sp = 0; sp < 2 + draws; sp++) {
                                    Case c;
                                    memset(&c, 0, sizeof c);
                                    c.acmod = acmod; c.lfe = lfe; c.nfbw = nf[acmod]; c.nch = c.nfbw + lfe;
                                    c.fscod = (uint32_t)(g_case % 3); c.frmsizecod = 30 + (uint32_t)(g_case % 8);
                                    c.m = meta == 0 ? BSI_DEFAULT : bsi_word(1 + (int)rnd(31), (int)rnd(8), (int)rnd(3), (int)rnd(3), (int)rnd(3), (int)rnd(2), (int)rnd(2));
                                    if (meta >= 2) {
                                        const int set = dual ? meta - 1 : 1;        // bit p: programme p sends compr
                                        for (int p = 0; p < np; p++) c.compr[p] = ((set >> p) & 1) ? 0x100u | rnd(256) : 0u;
                                    }
                                    for (int b = 0; b < 6; b++) {
                                        c.bsw[b] = bswon ? rnd(1u << c.nfbw) : 0u;
                                        for (int p = 0; p < np; p++) {
                                            const int how = p ? dynpat / 3 : dynpat % 3;    // none, some (blocks 0, 2, 5), all
                                            const bool sends = how == 2 || (how == 1 && (b == 0 || b == 2 || b == 5));
                                            c.dyn[b][p] = sends ? 0x100u | rnd(256) : 0u;
                                        }
                                    }
                                    c.remat_on = acmod == 2 && rem > 0;
                                    for (int b = 0; b < 6; b++) {
                                        const bool str = b == 0 || (((rem - 1) >> (b - 1)) & 1);
                                        c.remat[b] = c.remat_on ? (str ? 0x10u : 0u) | rnd(16) : 0u;
                                    }
                                    c.begf = cpl_at[cp][0] < 0 ? 0 : cpl_at[cp][0];
                                    c.endf = cpl_at[cp][1];
                                    // (the bandwidth tool: chbwcod 30 ends a channel at bin 163 and coupling at cplendf 30 >> 2 = 7)
                                    static const uint32_t bw[4] = {50u, 30u, 0u, 60u};
                                    c.chbwcod = cp ? (c.endf == 12 ? 50u : 30u) : bw[g_case % 4];
                                    if (cp) {
                                        c.cplw = 1u;
                                        for (int ch = 0; ch < c.nfbw; ch++) {
                                            c.cplw |= rnd(4) << (8 + 2 * ch);
                                            for (int bd = 0; bd < 3 + c.endf - c.begf; bd++) c.co[ch][bd] = rnd(256);
                                        }
                                    }
                                    // strategies: D15 everywhere; block 0 only; drawn (the LFE's is one bit; block 0 sends)
                                    for (int b = 0; b < 6; b++) {
                                        for (int ch = 0; ch < c.nch; ch++) {
                                            const bool is_lfe = lfe && ch == c.nch - 1;
                                            c.strat[b][ch] = sp == 0 ? 1u : sp == 1 ? (b == 0 ? 1u : 0u) : is_lfe ? (b == 0 ? 1u : rnd(2)) : b == 0 ? 1u + rnd(3) : rnd(4);
                                        }
                                        c.cstrat[b] = !cp ? 0u : sp == 0 ? 1u : sp == 1 ? (b == 0 ? 1u : 0u) : b == 0 ? 1u + rnd(3) : rnd(4);
                                    }
                                    run(c, sp < strats_read);
                                }
                            }
        }
    return 0;
}
