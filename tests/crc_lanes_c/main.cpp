/* csrc/crc_lanes.h on the host, for tests/test_crc_lanes_cpu.py: built without HIP, with -fsanitize=address,undefined, and run
 * on its own (never loaded into Python).
 * Every frame size enc_config can return - 19 bit rates x 3 sample rates x 3 half-rate shifts, by its own expression - and for each
 *   split    n1 in 1..63 (n1 + n2 = 64), C a multiple of 4 and the smallest that covers both regions; a region's chunks lie end to
 *            end, finish at the region's end and start at or in front of its first byte; no lane's bytes leave [-(64 C), 2 fs)
 *   reads    a lane's dword reads of the staged frame, counted by the accessor it reads through, stay inside the frame's dwords
 *            plus three of headroom (which hold noise here: nothing of them may reach a sum)
 *   words    the lane rule's two words - split, chunk sums through the 256-entry table, each lane's own row, the XOR scan -
 *            equal the bit-by-bit definition (A/52: x^16 + x^15 + x^2 + 1, MSB first, from 0; written out below, not taken from
 *            the header), and equal the header's scalar reference; with the two words stored, bytes [2, 2 fs58) and
 *            [2 fs58, 2 fs) both sum to 0
 *   frames   all zeros, all ones, SEEDED random ones (64 a size); every single set bit of a 128-byte frame
 * A few frames are printed as `vec FS CRC1 CRC2 HEX` for the Python model (tests/crc_model.py) to check.
 *   crc_lanes SEED */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <vector>
#include "crc_lanes.h"

using namespace ac3mi;

static uint64_t g_rng;
static uint32_t rnd()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// the definition, one message bit per step
static uint32_t def_crc(const uint8_t *p, int n)
{
    uint32_t crc = 0;
    for (int i = 0; i < n; i++)
        for (int k = 7; k >= 0; k--) {
            const uint32_t top = ((crc >> 15) & 1u) ^ ((p[i] >> k) & 1u);
            crc = (crc << 1) & 0xffffu;
            if (top) crc ^= 0x8005u;
        }
    return crc;
}

// the staged frame: MSB-first dwords and three dwords of headroom; every read is checked and recorded
struct Staged {
    std::vector<uint32_t> w;
    mutable int lo_read = 1 << 30, hi_read = -1;
    Staged(const uint8_t *frame, int fs) : w((size_t)(2 * fs + 3) / 4 + 3)
    {
        for (size_t d = 0; d < w.size(); d++) w[d] = rnd() * 2654435761u + 0x9e3779b9u;     // headroom, and the tail of an odd frame's last dword
        for (int p = 0; p < 2 * fs; p++) {
            uint32_t &x = w[(size_t)p >> 2];
            const int sh = 24 - 8 * (p & 3);
            x = (x & ~(0xffu << sh)) | ((uint32_t)frame[p] << sh);
        }
    }
    uint32_t operator[](int d) const
    {
        CHECK(d >= 0 && d < (int)w.size(), "staged read of dword %d outside 0..%d", d, (int)w.size() - 1);
        if (d < lo_read) lo_read = d;
        if (d > hi_read) hi_read = d;
        return w[(size_t)d];
    }
};

struct SizeTables {
    int fs;
    CrcSplit sp;
    uint16_t rows[CRCL_LANES][CRCL_ROW];
};
static uint16_t g_tab[256];

// the two words the lane rule gives: crc1 | crc2 << 16
static uint32_t lane_rule(const SizeTables &T, const uint8_t *frame)
{
    const int fs = T.fs;
    const Staged fr(frame, fs);
    uint32_t scan[CRCL_LANES], acc = 0;
    for (int lane = 0; lane < CRCL_LANES; lane++) {
        const CrcLane ln = crcl_lane(T.sp, fs, lane);
        fr.lo_read = 1 << 30;
        fr.hi_read = -1;
        const uint32_t sum = crcl_chunk_sum(fr, g_tab, ln.begin, T.sp.C, ln.lo);
        CHECK(sum <= 0xffffu, "fs %d lane %d: a sum of more than 16 bits", fs, lane);
        const int first = ln.begin >> 2;
        const int last = first + T.sp.C / 4 + CRCL_READ_AHEAD - 1;
        CHECK(fr.lo_read == (first < 0 ? 0 : first) && fr.hi_read == (last < 0 ? 0 : last), "fs %d lane %d: reads %d..%d", fs, lane, fr.lo_read, fr.hi_read);
        uint32_t r[CRCL_ROW / 2];
        for (int k = 0; k < CRCL_ROW / 2; k++) r[k] = (uint32_t)T.rows[lane][2 * k] | ((uint32_t)T.rows[lane][2 * k + 1] << 16);   // as the device reads the table
        acc ^= crcl_mul_row(sum, r);
        scan[lane] = acc;
    }
    const uint32_t crc1 = scan[T.sp.n1 - 1];
    return crc1 | ((scan[CRCL_LANES - 1] ^ crc1) << 16);
}

static void check_split(const SizeTables &T)
{
    const int fs = T.fs, C = T.sp.C, n1 = T.sp.n1, e1 = crcl_end1(fs), e2 = crcl_end2(fs);
    CHECK(C > 0 && C % 4 == 0, "fs %d: C = %d", fs, C);
    CHECK(n1 >= 1 && n1 <= CRCL_LANES - 1, "fs %d: n1 = %d", fs, n1);
    if (C > 4) CHECK((e1 + C - 5) / (C - 4) + (e2 - e1 + C - 5) / (C - 4) > CRCL_LANES, "fs %d: C = %d is not the smallest", fs, C);
    for (int lane = 0; lane < CRCL_LANES; lane++) {
        const CrcLane ln = crcl_lane(T.sp, fs, lane);
        const bool r2 = lane >= n1;
        CHECK(ln.begin >= -(CRCL_LANES * C) && ln.begin + C <= 2 * fs && (ln.begin & 1) == 0, "fs %d lane %d: bytes %d..", fs, lane, ln.begin);
        CHECK(ln.lo == (r2 ? e1 : 4), "fs %d lane %d: lo %d", fs, lane, ln.lo);
        const bool first = lane == 0 || lane == n1, last = lane == n1 - 1 || lane == CRCL_LANES - 1;
        if (first) CHECK(ln.begin <= (r2 ? e1 : 0), "fs %d lane %d: the region's first bytes are not covered", fs, lane);
        else CHECK(ln.begin == crcl_lane(T.sp, fs, lane - 1).begin + C, "fs %d lane %d: chunks not end to end", fs, lane);
        if (last) CHECK(ln.begin + C == (r2 ? e2 : e1) && ln.weight == 0, "fs %d lane %d: does not finish at the region's end", fs, lane);
        CHECK(ln.weight == (r2 ? e2 : e1) - (ln.begin + C), "fs %d lane %d: weight %d", fs, lane, ln.weight);
        // the lane's constant from the definition: the byte 1 and n - 2 zero bytes behind it sum to x^(8 n) (n >= 2)
        std::vector<uint8_t> one((size_t)(ln.weight > e1 ? ln.weight : e1), 0);
        one[0] = 1;
        const uint32_t k = ln.weight ? def_crc(one.data(), ln.weight - 1) : 1u;
        const uint32_t got = r2 ? T.rows[lane][0] : crcl_mul(T.rows[lane][0], def_crc(one.data(), e1 - 3));      // region 1's times x^(8 e1 - 16) again
        CHECK(got == k, "fs %d lane %d: constant %04x, x^(8 * %d) = %04x", fs, lane, got, ln.weight, k);
        for (int j = 1; j < CRCL_ROW; j++) CHECK(T.rows[lane][j] == crcl_mul(T.rows[lane][j - 1], 2), "fs %d lane %d: row entry %d", fs, lane, j);
    }
}

static long g_frames;
static void check_frame(const SizeTables &T, std::vector<uint8_t> &f, bool print)
{
    const int fs = T.fs, e1 = crcl_end1(fs);
    const uint32_t words = lane_rule(T, f.data()), crc1 = words & 0xffffu, crc2 = words >> 16;
    CHECK(crc1 == crcl_ref_crc1(f.data(), fs) && crc2 == crcl_ref_crc2(f.data(), fs), "fs %d: the lane rule gives %04x %04x, the scalar reference %04x %04x", fs,
          crc1, crc2, crcl_ref_crc1(f.data(), fs), crcl_ref_crc2(f.data(), fs));
    CHECK(crc2 == def_crc(f.data() + e1, 2 * fs - 2 - e1), "fs %d: crc2 %04x is not the definition's", fs, crc2);
    std::vector<uint8_t> g(f);
    g[2] = (uint8_t)(crc1 >> 8); g[3] = (uint8_t)crc1;
    g[(size_t)2 * fs - 2] = (uint8_t)(crc2 >> 8); g[(size_t)2 * fs - 1] = (uint8_t)crc2;
    CHECK(def_crc(g.data() + 2, e1 - 2) == 0, "fs %d: region 1 does not sum to 0 with crc1 = %04x", fs, crc1);
    CHECK(def_crc(g.data() + e1, 2 * fs - e1) == 0, "fs %d: region 2 does not sum to 0 with crc2 = %04x", fs, crc2);
    // what the fields held while summed does not count (crc1's reads as zero, crc2's is outside the region)
    g[0] ^= 0x5a; g[1] ^= 0xc3;
    CHECK(lane_rule(T, g.data()) == words, "fs %d: the words depend on bytes 0..3 or on the crc2 field", fs);
    g_frames++;
    if (print) {
        printf("vec %d %u %u ", fs, crc1, crc2);
        for (int p = 0; p < 2 * fs; p++) printf("%02x", f[(size_t)p]);
        printf("\n");
    }
}

int main(int argc, char **argv)
{
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    for (int b = 0; b < 256; b++) {
        const uint8_t byte = (uint8_t)b;
        g_tab[b] = (uint16_t)def_crc(&byte, 1);
    }
    CHECK(crcl_mul(2, CRCL_X_INV) == 1, "x^-1");

    // enc_config's frame sizes (capi.hip): the rates, the bit rates of A/52 table 5.18 shifted by the half-rate code
    static const int kRates[3] = {48000, 44100, 32000};
    static const int kKbps[19] = {32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 448, 512, 576, 640};
    std::set<int> sizes;
    int configs = 0;
    for (int h = 0; h < 3; h++)
        for (int j = 0; j < 3; j++)
            for (int i = 0; i < 19; i++) {
                const int freq = kRates[j] >> h, bitrate = kKbps[i] >> h;
                sizes.insert((bitrate * 1000 * 1536) / (freq * 16));
                configs++;
            }
    CHECK(configs == 171 && *sizes.begin() == 64 && *sizes.rbegin() == 1920, "frame sizes %d..%d", *sizes.begin(), *sizes.rbegin());

    int c_max = 0;
    for (int fs : sizes) {
        SizeTables T;
        T.fs = fs;
        T.sp = crcl_split(fs);
        crcl_fill_rows(fs, T.rows);
        check_split(T);
        if (T.sp.C > c_max) c_max = T.sp.C;
        std::vector<uint8_t> f((size_t)2 * fs, 0);
        check_frame(T, f, false);
        memset(f.data(), 0xff, f.size());
        check_frame(T, f, false);
        for (int n = 0; n < 64; n++) {
            for (auto &b : f) b = (uint8_t)(rnd() >> 7);
            check_frame(T, f, n == 0 && (fs == 64 || fs == 768 || fs == 835 || fs == 1920));
        }
        if (fs == 64)
            for (int bit = 0; bit < 1024; bit++) {
                memset(f.data(), 0, f.size());
                f[(size_t)bit >> 3] = (uint8_t)(0x80 >> (bit & 7));
                check_frame(T, f, false);
            }
    }
    const CrcSplit bench = crcl_split(768);
    CHECK(bench.C == 24 && bench.n1 == 40, "the 384 kbps 48 kHz frame splits %d + %d lanes at C = %d", bench.n1, CRCL_LANES - bench.n1, bench.C);
    printf("crc_lanes ok sizes=%d frames=%ld c_max=%d\n", (int)sizes.size(), g_frames, c_max);
    return 0;
}
