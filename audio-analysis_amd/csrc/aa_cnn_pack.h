// Host-side weight layouts of the CNN kernels: number-format conversions and
// one pure function per byte layout a kernel reads.  Plain C++ (no HIP call,
// no device code), so every layout can be checked on a machine without a GPU.
//
// The packers take the folded weights (BatchNorm scale multiplied in) as a
// compact f32 image -- [tap][cout_pad][cin] (tap = kh * KW + kw, rows past
// cout zero) or [cout][K] -- and return the bytes the kernel's weight pointer
// is loaded with, row padding and trailing slack included.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace aa {

static inline uint16_t f2bf(float f) {  // round to nearest even
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    u += 0x7fff + ((u >> 16) & 1);
    return (uint16_t)(u >> 16);
}
static inline float bf2f(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// f32 -> OCP e4m3fn byte, round to nearest even, saturated to +-448 (the
// device's v_cvt_pk_fp8_f32 conversion of the same value)
static inline uint8_t f2fp8(float f) {
    const uint8_t sgn = std::signbit(f) ? 0x80 : 0;
    double a = std::fabs((double)f);
    if (std::isnan(f)) return 0x7f;
    if (a >= 448.0) return sgn | 0x7e;
    if (a < std::ldexp(1.0, -6)) {  // subnormal: multiples of 2^-9
        const int q = (int)std::nearbyint(a * 512.0);
        return sgn | (uint8_t)q;  // q == 8 is the smallest normal's encoding
    }
    int ex;
    std::frexp(a, &ex);  // a = m 2^ex, m in [0.5, 1)
    const int e = ex - 1;
    double q = std::nearbyint(std::ldexp(a, 3 - e));  // 8 .. 16
    int ee = e;
    if (q >= 16.0) { q = 8.0; ++ee; }
    if (ee > 8 || (ee == 8 && q > 14.0)) return sgn | 0x7e;
    return sgn | (uint8_t)(((ee + 7) << 3) | ((int)q - 8));
}

// The per-lane constants of the fused first conv in the split-bf16 kernel
// (aa_conv_x3.h, FUSED): what a lane of a wave holds while it computes the
// first layer with two v_mfma_f32_32x32x16_bf16, built once per model instead
// of once per wave.  [part][lane 0..63][16 B]: part 0 the lane's A operand of
// MFMA 1 (8 bf16), part 1 that of MFMA 2, parts 2..5 its 16 accumulator start
// values (the bias, f32).  w: the folded first-layer weights [32][9], b: [32].
// MFMA row m = lane & 31 computes first-layer channel
// 16 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3); k-group kg = lane >> 5.  The 27
// split products of a pixel sit in the 32 k-slots of the two MFMAs: MFMA 1 =
// wh.xh (k-group 0) and wh.xl (k-group 1) over taps 0-7, so both k-groups
// hold the weights' hi halves; MFMA 2 = wl.xh over taps 0-7 (k-group 0) and
// wh8.xh8, wh8.xl8, wl8.xh8, then zeros (k-group 1).  D register r of a
// k-group kg lane holds channel 16 kg + r.
constexpr int F1_LANE_PARTS = 6;
constexpr size_t F1_LANE_IMAGE_BYTES = (size_t)F1_LANE_PARTS * 64 * 16;
static inline std::vector<uint8_t> pack_first_lanes(const float* w, const float* b) {
    std::vector<uint8_t> img(F1_LANE_IMAGE_BYTES);
    auto lo = [](float x) { return f2bf(x - bf2f(f2bf(x))); };
    for (int lane = 0; lane < 64; ++lane) {
        const int l32 = lane & 31, kg = lane >> 5;
        const float* w9 = w + (16 * ((l32 >> 2) & 1) + 4 * (l32 >> 3) + (l32 & 3)) * 9;
        uint16_t wa[8], wal[8];
        for (int j = 0; j < 8; ++j) {
            wa[j] = f2bf(w9[j]);
            wal[j] = kg == 0 ? lo(w9[j]) : j < 2 ? f2bf(w9[8]) : j == 2 ? lo(w9[8]) : (uint16_t)0;
        }
        memcpy(&img[(0 * 64 + lane) * 16], wa, 16);
        memcpy(&img[(1 * 64 + lane) * 16], wal, 16);
        for (int q = 0; q < 4; ++q) memcpy(&img[((2 + q) * 64 + lane) * 16], b + 16 * kg + 4 * q, 16);
    }
    return img;
}

template <typename E>
static inline std::vector<uint8_t> as_bytes(const std::vector<E>& v) {
    std::vector<uint8_t> b(v.size() * sizeof(E));
    if (!b.empty()) memcpy(b.data(), v.data(), b.size());
    return b;
}

// conv_small / conv_generic / pool_dense: the f32 image as it is
static inline std::vector<uint8_t> pack_rowmajor_f32(const std::vector<float>& w) { return as_bytes(w); }

// [tap][cout_pad][cstr] in the element type of `cvt` (rows padded from cin to
// cstr with zeros) plus `slack` zero elements: one tap's slice of a block is
// one contiguous [BN][cstr] block, byte-identical to its LDS image, and the
// slack covers the last slice's rounding up to whole global_load_lds
// instructions.  The 1x1 head reads [cout_pad][cin] (cstr = cin, no slack).
template <typename E, typename Cvt>
static inline std::vector<uint8_t> pack_tap(const std::vector<float>& w, int ntap, int cout_pad, int cin, int cstr,
                                            size_t slack, Cvt cvt) {
    std::vector<E> h((size_t)ntap * cout_pad * cstr + slack, cvt(0.f));
    for (size_t r = 0; r < (size_t)ntap * cout_pad; ++r)
        for (int c = 0; c < cin; ++c) h[r * cstr + c] = cvt(w[r * cin + c]);
    return as_bytes(h);
}
static inline std::vector<uint8_t> pack_tap_f32(const std::vector<float>& w, int ntap, int cout_pad, int cin,
                                                int cstr, size_t slack) {
    return pack_tap<float>(w, ntap, cout_pad, cin, cstr, slack, [](float v) { return v; });
}
static inline std::vector<uint8_t> pack_bf16(const std::vector<float>& w, int ntap, int cout_pad, int cin, int cstr,
                                             size_t slack) {
    return pack_tap<uint16_t>(w, ntap, cout_pad, cin, cstr, slack, f2bf);
}

// fp8 (e4m3fn), quantised per output channel: the largest |w| maps to 240
// (e4m3fn tops out at 448) and the kernel's epilogue multiplies by amax / 240,
// stored in scales[0 .. cout_pad) (1 for an all-zero channel).
// bstr128 == 0: [tap][cout_pad][cstr] as pack_tap (conv_mfma's K = 32 loop,
// the head).  bstr128 > 0 (conv_mfma's K = 128 loop): super-steps of four
// 32-channel chunks (chunk k = tap k / (cin/32), channels 32 (k % (cin/32))
// ..), each [cout_pad][bstr128] with chunk k % 4 at byte 32 (k % 4) of the
// row; chunks past the last tap stay zero; 1 KiB of slack.
static inline std::vector<uint8_t> pack_fp8(const std::vector<float>& w, int ntap, int cout_pad, int cin, int cstr,
                                            size_t slack, int bstr128, float* scales) {
    const int cpc = cin / 32, nch = ntap * cpc, nss = (nch + 3) / 4;
    std::vector<uint8_t> h(bstr128 ? (size_t)nss * cout_pad * bstr128 + 1024 : (size_t)ntap * cout_pad * cstr + slack, 0);
    for (int o = 0; o < cout_pad; ++o) {
        float amax = 0.f;
        for (int t = 0; t < ntap; ++t)
            for (int c = 0; c < cin; ++c) amax = std::max(amax, std::fabs(w[((size_t)t * cout_pad + o) * cin + c]));
        const float sc = amax > 0.f ? 240.f / amax : 1.f;
        scales[o] = 1.f / sc;
        for (int t = 0; t < ntap; ++t)
            for (int c = 0; c < cin; ++c) {
                const uint8_t q = f2fp8(w[((size_t)t * cout_pad + o) * cin + c] * sc);
                const int k = t * cpc + c / 32;
                if (bstr128)
                    h[((size_t)(k / 4) * cout_pad + o) * bstr128 + 32 * (k % 4) + c % 32] = q;
                else
                    h[((size_t)t * cout_pad + o) * cstr + c] = q;
            }
    }
    return h;
}

// One 64-element weight row of a split-bf16 step (aa_conv_x3.h): 8 units of 8
// bf16, units 0-3 hi = rn_bf16(w) of the row's 32 channels, units 4-7 lo =
// rn_bf16(w - hi), unit u of output channel o stored in slot (u + o) & 7.
// Writes channel c (0..31) of row o.
static inline void put_split(uint16_t* row, int o, int c, float w) {
    const uint16_t hi = f2bf(w);
    const int u = c / 8;
    row[((u + o) & 7) * 8 + c % 8] = hi;
    row[((u + 4 + o) & 7) * 8 + c % 8] = f2bf(w - bf2f(hi));
}

// conv_x3 steps (32-channel group g, tap t) in order g * ntap + t, each
// [cout_pad] rows of put_split; 2 KiB of slack
static inline std::vector<uint8_t> pack_x3(const std::vector<float>& w, int ntap, int cout_pad, int cin) {
    std::vector<uint16_t> h(2 * ((size_t)ntap * cout_pad * cin + 512), 0);
    for (int g = 0; g < cin / 32; ++g)
        for (int t = 0; t < ntap; ++t)
            for (int o = 0; o < cout_pad; ++o)
                for (int c = 0; c < 32; ++c)
                    put_split(&h[((size_t)(g * ntap + t) * cout_pad + o) * 64], o, c,
                              w[((size_t)t * cout_pad + o) * cin + 32 * g + c]);
    return as_bytes(h);
}

// conv_wg steps (group g, pass p, row kh, plane slot el) in order
// ((g * npass + p) * KH + kh) * pps + el, each [cout_pad] rows of put_split
// holding the transformed weights v_e = sum_k G[e][k] w_k of plane e = p * pps
// + el (w_k = the folded kernel at (kh, k); F(2,3): v0 = w0, v1 = (w0 + w1 +
// w2) / 2, v2 = (w0 - w1 + w2) / 2, v3 = w2).  Computed in double from the
// raw kernel [kh][3][cin][cout] and the BatchNorm scale, rounded to f32 once;
// G is the [wo + 2][3] transform (wg_g, aa_conv_wg.h); 2 KiB of slack.
static inline std::vector<uint8_t> pack_wg(const float* kern, const std::vector<double>& scale, int kh_n, int cin,
                                           int cout, int cout_pad, int wo, int npass, const std::vector<double>& G) {
    const int A = wo + 2, pps = A / npass, ng = cin / 32;
    std::vector<uint16_t> h((size_t)ng * kh_n * A * cout_pad * 64 * 2 + 1024, 0);
    for (int g = 0; g < ng; ++g)
        for (int kh = 0; kh < kh_n; ++kh)
            for (int o = 0; o < cout_pad; ++o)
                for (int c = 0; c < 32; ++c) {
                    double w3[3];
                    for (int kw = 0; kw < 3; ++kw)
                        w3[kw] = o < cout ? (double)kern[((size_t)(kh * 3 + kw) * cin + 32 * g + c) * cout + o] * scale[o] : 0.0;
                    for (int e = 0; e < A; ++e) {
                        const double v = G[e * 3] * w3[0] + G[e * 3 + 1] * w3[1] + G[e * 3 + 2] * w3[2];
                        const int p = e / pps, el = e % pps;
                        put_split(&h[((size_t)(((g * npass + p) * kh_n + kh) * pps + el) * cout_pad + o) * 64], o, c, (float)v);
                    }
                }
    return as_bytes(h);
}

// conv_tail_x3's head weights from the f32 head image [cout_pad][cin = 32 nw]:
// per (wave w, label fragment lf, hi / lo, lane l) 8 bf16: label 16 lf +
// (l & 15), k-slot e <-> channel 32 w + (e < 4 ? 4 (l >> 4) + e : 16 +
// 4 (l >> 4) + e - 4); labels past cout zero
static inline std::vector<uint8_t> pack_tail_head(const std::vector<float>& hw, int cout, int cin, int nw) {
    std::vector<uint16_t> pk((size_t)nw * 2 * 2 * 64 * 8, 0);
    for (int w = 0; w < nw; ++w)
        for (int lf = 0; lf < 2; ++lf)
            for (int l = 0; l < 64; ++l)
                for (int k = 0; k < 8; ++k) {
                    const int lab = lf * 16 + (l & 15), qq = l >> 4;
                    const int co = 32 * w + (k < 4 ? 4 * qq + k : 16 + 4 * qq + k - 4);
                    const float v = lab < cout ? hw[(size_t)lab * cin + co] : 0.f;
                    const uint16_t hi = f2bf(v);
                    pk[((((size_t)w * 2 + lf) * 2 + 0) * 64 + l) * 8 + k] = hi;
                    pk[((((size_t)w * 2 + lf) * 2 + 1) * 64 + l) * 8 + k] = f2bf(v - bf2f(hi));
                }
    return as_bytes(pk);
}

// gconv_x3 (aa_gconv.h) from a compact f32 [tap][cout][cin] image (BN already
// folded): [tap][cin_pad/32][cout_pad][32 hi | 32 lo]
static inline std::vector<uint16_t> gconv_pack_x3(const std::vector<float>& w_tco, int ntap, int cout, int cin,
                                                  int cout_pad, int cin_pad) {
    const int ncc = cin_pad / 32;
    std::vector<uint16_t> h((size_t)ntap * ncc * cout_pad * 64, 0);
    for (int t = 0; t < ntap; ++t)
        for (int o = 0; o < cout; ++o)
            for (int c = 0; c < cin; ++c) {
                const float w = w_tco[((size_t)t * cout + o) * cin + c];
                const uint16_t hi = f2bf(w);
                const size_t row = ((size_t)(t * ncc + c / 32) * cout_pad + o) * 64;
                h[row + c % 32] = hi;
                h[row + 32 + c % 32] = f2bf(w - bf2f(hi));
            }
    return h;
}

// The graph's images (aa_graph_plan.h) of a Keras kernel k = [K][cout], K =
// tap * cin + c (HWIO flattened), no folding:
// [tap][cout][cin], what gconv_pack_x3 takes
static inline std::vector<float> keras_to_tco(const float* k, int ntap, int cin, int cout) {
    std::vector<float> w((size_t)ntap * cout * cin);
    for (int t = 0; t < ntap; ++t)
        for (int o = 0; o < cout; ++o)
            for (int c = 0; c < cin; ++c) w[((size_t)t * cout + o) * cin + c] = k[((size_t)t * cin + c) * cout + o];
    return w;
}

// [cout][K]: gconv_f32 / gconv_f32_lds, gmatvec (1x1 convs on 1x1 maps, Dense)
static inline std::vector<float> keras_to_ok(const float* k, int K, int cout) {
    std::vector<float> w((size_t)cout * K);
    for (int o = 0; o < cout; ++o)
        for (int kk = 0; kk < K; ++kk) w[(size_t)o * K + kk] = k[(size_t)kk * cout + o];
    return w;
}

// [K][cout], the Keras order as it is: gmatvec_t (one thread per output)
static inline std::vector<float> keras_as_is(const float* k, int K, int cout) {
    return std::vector<float>(k, k + (size_t)K * cout);
}

// [ceil(cout / 32)][K][32], channels past cout zero: gconv_f32_s (the f32
// stem's weights through the scalar cache)
static inline std::vector<float> pack_stem_f32(const float* k, int K, int cout) {
    std::vector<float> w((size_t)((cout + 31) / 32) * K * 32, 0.f);
    for (int o = 0; o < cout; ++o)
        for (int kk = 0; kk < K; ++kk) w[((size_t)(o / 32) * K + kk) * 32 + o % 32] = k[(size_t)kk * cout + o];
    return w;
}

}  // namespace aa
