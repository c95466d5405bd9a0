// The launch rule of csrc/launch_rule.h on the rows of grid.h, one canonical line a row, for tests/test_launch_rule_cpu.py:
//   main enc | dec     the reduced grids
//   main lists         every listed variant, by its kernel's name
//   main words         "family word name" of every listed variant: the one table that ties a word of the launch log
//                      (ac3mi_debug_launch_log; written here by log_launch itself) to a kernel's name
//   main pairs         a row on either side of every threshold
//   main plan          dec_choice's mantx answer for the calls ac3mi_transcode_workspace_plan describes
// Built with the host compiler under -fsanitize=address,undefined; nothing here but the header under test and grid.h.
#include <string.h>
#include "launch_rule.h"
#include "grid.h"

using namespace ac3mi;

static const char *B(uint32_t v, uint32_t bit) { return (v & bit) ? "true" : "false"; }

// the kernel a (family, word) names, spelled as its symbol demangles
static std::string kernel_name(int family, uint32_t v)
{
    char b[128];
    const int n = (int)(v & V_NUM);
    switch (family) {
    case K_DECODE: snprintf(b, sizeof b, "decode_kernel<%d, %s, %s>", n, B(v, V_FX), B(v, V_SRC)); break;
    case K_DECODE_WG: snprintf(b, sizeof b, "decode_wg_kernel<%d, %s>", n, B(v, V_SRC)); break;
    case K_LFSR_PREFIX: snprintf(b, sizeof b, "lfsr_prefix_kernel"); break;
    case K_MANT: snprintf(b, sizeof b, "mant_kernel"); break;
    case K_MANTX: snprintf(b, sizeof b, "mantx_kernel<%s, %s>", B(v, V_S16), B(v, V_FX)); break;
    case K_ENC_MDCT:
        snprintf(b, sizeof b, "enc_mdct_kernel<%s, %s, %s, %s, %s, %s>", B(v, V_BSW), B(v, V_REMAT), B(v, V_BW), B(v, V_XS), B(v, V_LFEROW), B(v, V_FX));
        break;
    case K_ENC_CPL: snprintf(b, sizeof b, "enc_cpl_kernel<%s, %s, %s>", B(v, V_BW), B(v, V_XS), B(v, V_R3)); break;
    case K_ENC_SEARCH:
        snprintf(b, sizeof b, "enc_search_kernel<%d, %s, %s, %s, %s, %s>", n, B(v, V_CPL), B(v, V_BW), B(v, V_DRC), B(v, V_FX), B(v, V_DW));
        break;
    case K_ENC_PACKF:
        snprintf(b, sizeof b, "enc_packf_kernel<%s, %s, %s, %s, %s, %s>", B(v, V_FX), B(v, V_CPL), B(v, V_BW), B(v, V_MD), B(v, V_DUAL), B(v, V_DW));
        break;
    case K_ENC_PACKB: snprintf(b, sizeof b, "enc_packb_kernel<%s, %s>", B(v, V_MD), B(v, V_DW)); break;
    default: snprintf(b, sizeof b, "?");
    }
    return b;
}

static grid::Launched launched(const KernelLaunch &k, int streams, int frames, int nch)
{
    return {kernel_name(k.family, k.variant), grid_size(k, streams, frames, nch), k.block};
}

// an encoder call as enc_choice reads one: EncodeLaunch's members by name, the arrays as "is set"
struct Call {
    struct { int acmod, lfe, nch, nfbw; } cfg;
    int n_streams, frames_per_stream, pack_mode, chbwcod, cpl_begf, drc_profile;
    uint32_t bsi;
    bool bw, ws_bsw, ws_remat, dyn_codes, compr_words, bsi_words, exp_strategy, fixed_shape, mdct_full_rows, ws_expo, tap_strat, tap_snr, ws_memo;
};

static std::string enc_line(const grid::EncRow &r)
{
    Call in;
    in.cfg = {r.acmod, r.lfe, r.nch(), r.nfbw()};
    in.n_streams = r.streams; in.frames_per_stream = r.frames; in.pack_mode = r.pack_mode;
    in.chbwcod = r.chbwcod; in.bw = r.bw; in.ws_bsw = r.bsw; in.ws_remat = r.remat; in.cpl_begf = r.begf;
    in.drc_profile = r.drc; in.dyn_codes = r.dyn; in.compr_words = r.compr; in.bsi_words = r.bsi_words; in.bsi = r.bsi_default ? BSI_DEFAULT : BSI_DEFAULT ^ 32u;
    in.exp_strategy = r.xs; in.fixed_shape = r.fixed; in.mdct_full_rows = r.full_rows;
    in.ws_expo = r.expo; in.tap_strat = r.tap_strat; in.tap_snr = r.tap_snr; in.ws_memo = true;
    const EncChoice c = enc_choice(in);
    std::vector<grid::Launched> l;
    for (const KernelLaunch &k : c.stage)
        if (k.family != K_NONE) l.push_back(launched(k, r.streams, r.frames, r.nch()));
    return grid::enc_line(r, c.err, l, c.history);
}

static std::string dec_line(const grid::DecRow &r)
{
    const DecChoice c = dec_choice(r.mode, r.streams, r.frames, r.s16, r.taps, !r.transcode, r.identity, r.mix_state, r.fixed, r.acmod, r.lfe, r.src);
    const char flags[8] = {(char)('0' + c.identity), (char)('0' + c.mixstate), (char)('0' + c.wg), (char)('0' + c.fused), (char)('0' + c.split),
                           (char)('0' + c.mantx), (char)('0' + c.fp), 0};
    std::vector<grid::Launched> l;
    for (int i = 0; i < c.n; i++) l.push_back(launched(c.launch[i], r.streams, r.frames, 1));
    return grid::dec_line(r, flags, c.err, l);
}

template <size_t N> static void list(int family, const uint32_t (&v)[N])
{
    for (uint32_t w : v) puts(kernel_name(family, w).c_str());
}

// the listed variants through log_launch, as the launchers log them: family, variant word and name of each logged word
template <size_t N> static void words(KernelFamily family, const uint32_t (&v)[N])
{
    uint32_t h[2 + N] = {};
    const LaunchLog log = {h, (int)(1 + N)};        // (one word short of the array: the last slot must stay as it is)
    h[1 + N] = 0xa5a5a5a5u;
    for (uint32_t w : v) log_launch(&log, kernel_launch(family, w, G_STREAM, 64));
    log_launch(&log, kernel_launch(family, v[0], G_STREAM, 64));       // no longer fits: counted, not stored
    log_launch(nullptr, kernel_launch(family, v[0], G_STREAM, 64));
    if (h[0] != N + 1 || h[1 + N] != 0xa5a5a5a5u) abort();
    for (size_t i = 1; i <= N; i++) printf("%u %u %s\n", h[i] >> 24, h[i] & 0xffffffu, kernel_name((int)(h[i] >> 24), h[i] & 0xffffffu).c_str());
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "enc")) grid::enc_reduced([](const grid::EncRow &r) { puts(enc_line(r).c_str()); });
    else if (!strcmp(what, "dec")) grid::dec_reduced([](const grid::DecRow &r) { puts(dec_line(r).c_str()); });
    else if (!strcmp(what, "lists")) {
        list(K_DECODE, DECODE_VARIANTS);
        list(K_DECODE_WG, DECODE_WG_VARIANTS);
        list(K_LFSR_PREFIX, PLAIN_VARIANT);
        list(K_MANT, PLAIN_VARIANT);
        list(K_MANTX, MANTX_VARIANTS);
        list(K_ENC_MDCT, ENC_MDCT_VARIANTS);
        list(K_ENC_CPL, ENC_CPL_VARIANTS);
        list(K_ENC_SEARCH, ENC_SEARCH_VARIANTS);
        list(K_ENC_PACKF, ENC_PACKF_VARIANTS);
        list(K_ENC_PACKB, ENC_PACKB_VARIANTS);
    } else if (!strcmp(what, "words")) {
        words(K_DECODE, DECODE_VARIANTS);
        words(K_DECODE_WG, DECODE_WG_VARIANTS);
        words(K_LFSR_PREFIX, PLAIN_VARIANT);
        words(K_MANT, PLAIN_VARIANT);
        words(K_MANTX, MANTX_VARIANTS);
        words(K_ENC_MDCT, ENC_MDCT_VARIANTS);
        words(K_ENC_CPL, ENC_CPL_VARIANTS);
        words(K_ENC_SEARCH, ENC_SEARCH_VARIANTS);
        words(K_ENC_PACKF, ENC_PACKF_VARIANTS);
        words(K_ENC_PACKB, ENC_PACKB_VARIANTS);
    } else if (!strcmp(what, "pairs")) {
        // decoder, 5.1 to s16, auto: 512 | 513 streams of one frame; four | five frames at 512 streams; 5 119 | 5 120 streams of two
        grid::DecRow d = {0, 512, 1, 1, 0, 0, 1, 0, 1, 7, 1, 0};
        for (int s : {512, 513}) { d.streams = s; puts(dec_line(d).c_str()); }
        d.streams = 512;
        for (int f : {4, 5}) { d.frames = f; puts(dec_line(d).c_str()); }
        d.frames = 2;
        for (int s : {5119, 5120}) { d.streams = s; puts(dec_line(d).c_str()); }
        // encoder, 5.1 with no tool: 1 024 | 1 025 one-frame streams; 2 047 | 2 048 and 5 119 | 5 120 streams of two frames
        grid::EncRow e = grid::enc_row(0);
        e.acmod = 7; e.lfe = 1;
        for (int s : {1024, 1025}) { e.streams = s; puts(enc_line(e).c_str()); }
        e.frames = 2;
        for (int s : {2047, 2048, 5119, 5120}) { e.streams = s; puts(enc_line(e).c_str()); }
    } else if (!strcmp(what, "plan")) {
        // the default decode mode, to s16, no taps, a batch too large for the one-workgroup-per-stream kernel
        for (int frames = 1; frames <= 2; frames++)
            for (int identity = 0; identity <= 1; identity++)
                printf("%d %d %d\n", frames, identity, (int)dec_choice(0, 65536 / frames, frames, true, false, false, identity, false, true, 7, 1, false).mantx);
    } else return 2;
    return 0;
}
