// Tile tables of the window-classifier CNN's tuned convolutions and their
// lookups: which instantiation serves a (precision, kernel, C_in, pool) shape
// and how many output channels its block covers.  Read by the planner
// (aa_cnn_plan.h: stage classification, cout_pad, workspace) and by the
// launchers (aa_cnn.hip: one instantiation per row).  Included by aa_cnn.hip
// after the precision tags (bf16, fp8, bf16x3); holds tables and constexpr /
// host lookups only, no kernel.
#pragma once

namespace aa {

// Tile configuration of every conv_mfma instantiation, one line per
// (dtype, kernel, C_in, pool): waves (WM x WN), 16x16 fragments per wave
// (MF x NF), output tile TH x TW, bf16 epilogue tile.  BN = WN * NF * 16
// output channels per block.  The f32 rows are the parity mode (smaller
// tiles: the same LDS budget holds half the elements).
#define AA_CONV_CFGS(X)                                     \
    X(bf16, 3, 3, 32, 3, 4, 1, 6, 2, 18, 21, true, 0)          \
    X(bf16, 3, 3, 32, 1, 2, 2, 4, 2, 8, 16, true, 0)           \
    X(bf16, 3, 3, 64, 1, 2, 2, 4, 2, 8, 16, true, 0)           \
    X(bf16, 9, 3, 64, 3, 4, 2, 6, 4, 39, 9, true, 0)           \
    X(bf16, 1, 3, 128, 1, 2, 4, 5, 2, 7, 20, false, 0)         \
    X(fp8, 3, 3, 32, 3, 4, 1, 6, 2, 12, 30, true, 0)           \
    X(fp8, 3, 3, 32, 1, 2, 2, 4, 2, 8, 16, true, 0)            \
    X(fp8, 3, 3, 64, 1, 4, 1, 3, 4, 12, 16, true, 0)           \
    X(fp8, 9, 3, 64, 3, 4, 2, 6, 4, 21, 18, true, 0)           \
    X(fp8, 1, 3, 128, 1, 2, 4, 5, 2, 7, 20, true, 0)           \
    X(float, 3, 3, 32, 3, 2, 2, 9, 1, 6, 48, false, 0)         \
    X(float, 3, 3, 32, 1, 1, 4, 9, 1, 6, 24, false, 0)         \
    X(float, 3, 3, 64, 1, 1, 4, 9, 1, 6, 24, false, 0)         \
    X(float, 9, 3, 64, 3, 1, 4, 7, 1, 3, 33, false, 0)         \
    X(float, 1, 3, 128, 1, 2, 2, 5, 1, 6, 24, false, 0)

// conv_x3 (split-bf16) instantiations: (kernel, C_in, pool) -> waves (WM x
// WN), fragments per wave (MF x NF), output tile TH x TW, weight ring in LDS
// (1) or per-wave B fragments from global (0), A fragments just in time (1)
// or a whole step ahead (0), pinned waves per SIMD (0: free); picked by
// tools/conv_bench_x3.hip sweeps
#ifdef AA_X3_ALT  // tools/ab_build.py: an alternative tile table for in-pipeline A/B runs
#define AA_X3_CFGS(X) AA_X3_ALT(X)
#else
#define AA_X3_CFGS(X)                                 \
    X(3, 3, 32, 3, 4, 1, 4, 2, 12, 21, 0, 1, 0)       \
    X(3, 3, 32, 1, 4, 2, 3, 2, 10, 18, 1, 0, 4)       \
    X(3, 3, 64, 1, 2, 2, 3, 2, 12, 8, 1, 1, 0)        \
    X(9, 3, 64, 3, 2, 2, 4, 2, 21, 6, 0, 1, 4)        \
    X(1, 3, 128, 1, 2, 2, 3, 2, 7, 12, 1, 1, 0)
#endif

// conv_wg (split-bf16, Winograd F(WO,3) along W) instantiations: (kh, C_in,
// pool) of kernel-width-3 convs -> waves (WM x WN), fragments per wave (MF x
// NF, each with WO + 2 accumulator sets), output tile TH x TW (TW a multiple
// of WO), pinned waves per SIMD (0: free), outputs per group WO, staging
// passes NPASS, B fragment sets in flight BD, A fragments sliding in registers
// (SLIDE, aa_conv_wg.h: 0 reads them from LDS at every kernel row, S every S
// rows).  Preferred over conv_x3 where a row exists (the
// fused first-layer stage always runs conv_x3).  In-pipeline A/B (tools/ab.sh,
// same box): the 9x3 layer 187 -> 160 us, step 180k -> 193k audio-s/s; the
// small 3x3 / 1x3 layers lose on it (their transform-heavy staging outweighs
// the saved MFMAs: 3x3/32 36 -> 55 us, 3x3/64 52 -> 76 us, 1x3 22 -> 28 us).
#ifdef AA_WG_ALT
#define AA_WG_CFGS(X) AA_WG_ALT(X)
#else
// F(6,3) for the 9x3 layer (in-pipeline A/B, 3 rounds on one box: 9x3 131 ->
// 122 us, step 260k -> 264k; F(4,3) on 39x12 tiles 140 us, F(3,3) spills):
// 8 planes of the 39 x 6 tile's single column group, 4 waves of 16 output
// channels each, 96 accumulator VGPRs.  SLIDE 9 and 4 B sets (harness, bit-
// identical outputs: 113.9 -> 105.1 us sliding, -> 103.9 us with the deeper B
// ring; serial trace 110.4 -> ~104 us; profiles/r07/conv_wg_slide.txt)
#define AA_WG_CFGS(X) X(9, 64, 3, 1, 4, 3, 1, 39, 6, 0, 6, 1, 4, 9)
#endif

// The fused tail (aa_conv_tail.h: the 1x3/128 -> 256 conv and the 1x1 head in
// one launch): conv output tile TAIL_TH x TAIL_TW per block, for the launch
// and for the workspace that holds its per-tile label maxima.
#ifndef AA_TAIL_TW  // (A/B knobs: tile width and pixel fragments per wave)
#define AA_TAIL_TW 5
#define AA_TAIL_MF 5
#endif
constexpr int TAIL_TH = 13, TAIL_TW = AA_TAIL_TW;

static int wg_bn(int kh, int kw, int cin, int pool) {
#define AA_WBN(KH, CIN, POOL, WM, WN, MF, NF, TH, TW, OCC, WO, NPASS, BD, SLIDE) \
    if (kw == 3 && kh == KH && cin == CIN && pool == POOL) return WN * NF * 16;
    AA_WG_CFGS(AA_WBN)
#undef AA_WBN
    return 0;
}
// (WO, NPASS) of the Winograd instantiation serving a stage
static void wg_form(int kh, int cin, int pool, int* wo, int* npass) {
#define AA_WFORM(KH, CIN, POOL, WM, WN, MF, NF, TH, TW, OCC, WO, NPASS, BD, SLIDE) \
    if (kh == KH && cin == CIN && pool == POOL) { *wo = WO; *npass = NPASS; return; }
    AA_WG_CFGS(AA_WFORM)
#undef AA_WFORM
    *wo = 0;
    *npass = 1;
}

template <typename T>
constexpr int prec_of() {
    return is_split<T>() ? AA_PREC_BF16X3 : sizeof(T) == 1 ? AA_PREC_FP8 : sizeof(T) == 2 ? AA_PREC_BF16 : AA_PREC_F32;
}

// output channels per block of the instantiation serving this stage (0: none)
static int mfma_bn(int prec, int kh, int kw, int cin, int pool) {
    if (prec == AA_PREC_BF16X3 && wg_bn(kh, kw, cin, pool)) return wg_bn(kh, kw, cin, pool);
#define AA_BN(T_, KH, KW, CIN, POOL, WM, WN, MF, NF, TH, TW, EB, OCC)                                       \
    if (prec_of<T_>() == prec && kh == KH && kw == KW && cin == CIN && pool == POOL) \
        return WN * NF * 16;
    AA_CONV_CFGS(AA_BN)
#undef AA_BN
#define AA_BN3(KH, KW, CIN, POOL, WM, WN, MF, NF, TH, TW, RING, AJIT, OCC)                                               \
    if (prec == AA_PREC_BF16X3 && kh == KH && kw == KW && cin == CIN && pool == POOL) return WN * NF * 16;
    AA_X3_CFGS(AA_BN3)
#undef AA_BN3
    return 0;
}

}  // namespace aa
