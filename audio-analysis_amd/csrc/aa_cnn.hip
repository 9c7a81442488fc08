// Window-classifier CNN for gfx950: MFMA implicit-GEMM convolutions.
//
// Replaces model.predict(np.array(d)) (reference src/identify_tracks.py:544,
// Keras on TF-CPU) for the layer family the build defines:
//   [MagTransform] conv-BN-act [maxpool] ... conv1x1 globalmax sigmoid
// Four precisions (aa.h): f32 parity, bf16, fp8 (e4m3fn, per-channel weight
// scales) and split-bf16 (f32 activations, bf16 hi + lo operands: the default).
//
// This file holds, in order:
//   * the precision tags, MFMA fragment helpers and the kernels every
//     precision shares: conv_small (C_in = 1 first conv, VALU), conv_mfma
//     (tuned implicit-GEMM conv for f32 / bf16 / fp8: patch staged once in
//     LDS, weight slices streamed through an LDS ring by global_load_lds,
//     K = 128 super-steps for fp8 at C_in >= 64, optional fused first conv,
//     max-pool + bias + activation epilogue), conv_head + head_final (1x1
//     conv, global max, sigmoid), conv_generic / pool_dense (f32 VALU
//     fallbacks for any other shape), track_mean, stage_decode;
//   * the split-bf16 kernel families, each in its own header: aa_conv_x3.h
//     (direct; it also holds the fragment helpers -- x3_mfma3, x3_frag_pixel,
//     x3_bofs, x3_read_b, x3_stage_split, x3_step_jit -- and the epilogue
//     x3_store that the next three share), aa_conv_pair.h (the 3x3 32 -> 64
//     and 64 -> 64 convs in one launch), aa_conv_wg.h (Winograd along W),
//     aa_conv_tail.h (last conv + head in one launch), aa_gconv.h
//     (runtime-shaped; also built into aa_graph.hip, so it keeps its own);
//   * aa_cnn_plan.h: Stage, Model and the host-only planner (layer list ->
//     stages with packed weight images), over aa_cnn_tiles.h (tile tables)
//     and aa_cnn_pack.h (weight layouts);
//   * the launchers (one shared prologue for the tuned convs, launch_stage
//     choosing the instantiation from the tile tables), upload_model,
//     run_stages (the one stage loop behind aa_model_forward and
//     aa_model_forward_prefix) and the aa_model_* entry points.
#include "aa_common.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

namespace aa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __bf16 bf16;
// OCP e4m3fn byte (gfx950's fp8; not the MI300 fnuz encoding)
struct fp8 {
    uint8_t v;
};
// Split-bf16 precision tag (AA_PREC_BF16X3): activations stay f32 in HBM; at
// LDS staging every value x becomes bf16 hi = rn(x) and lo = rn(x - hi)
// (x - hi is exact in f32), weights likewise on the host, and each product
// is hi*hi + hi*lo + lo*hi on three bf16 MFMAs with f32 accumulation.  The
// representation error is <= 2^-18 |x| per operand and the dropped lo*lo
// term <= 2^-18 |x w|, so a MAC carries ~17 significant bits instead of
// bf16's 8 -- enough for the 1e-3 logit gate at 3/16 of the f32-MFMA cost.
struct bf16x3 {};

// Storage types of a precision: L = LDS / fragment element, G = HBM
// activation element.
template <typename T>
struct Prec {
    using L = T;
    using G = T;
};
template <>
struct Prec<bf16x3> {
    using L = bf16;
    using G = float;
};
template <typename T>
constexpr bool is_split() { return std::is_same<T, bf16x3>::value; }
template <typename T>
constexpr bool is_fp8() { return std::is_same<T, fp8>::value; }

// bf16 hi + lo of an f32 (round to nearest even both times)
__device__ __forceinline__ bf16 bf_hi(float x) { return (bf16)x; }
__device__ __forceinline__ bf16 bf_lo(float x) { return (bf16)(x - (float)(bf16)x); }

// 4 / 8 floats -> e4m3fn bytes, round to nearest even, saturated to +-448
__device__ __forceinline__ uint32_t pack4_fp8(float a, float b, float c, float d) {
    const float M = 448.f;
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(a, -M), M), fminf(fmaxf(b, -M), M), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(c, -M), M), fminf(fmaxf(d, -M), M), w, true);
    return (uint32_t)w;
}

// ---- 8-element fragments and the MFMA step over one 32-deep K chunk -------
template <typename T>
struct Frag;
template <>
struct Frag<bf16> {
    bf16x8 v;
    __device__ __forceinline__ void load(const bf16* p) { v = *reinterpret_cast<const bf16x8*>(p); }
};
template <>
struct Frag<fp8> {
    long v;
    __device__ __forceinline__ void load(const fp8* p) { v = *reinterpret_cast<const long*>(p); }
};
template <>
struct Frag<float> {
    float v[8];
    __device__ __forceinline__ void load(const float* p) {
        const float4 a = reinterpret_cast<const float4*>(p)[0];
        const float4 b = reinterpret_cast<const float4*>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
};

// Lane l holds A[row l&15][k0 + 8(l>>4) + j] and B[k0 + 8(l>>4) + j][col l&15].
__device__ __forceinline__ f32x4 mfma_chunk(const Frag<bf16>& a, const Frag<bf16>& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
}
// fp8: the same lane layout with 8 bytes per lane (non-scaled form: the bf16 rate,
// half the staging and fragment bytes)
__device__ __forceinline__ f32x4 mfma_chunk(const Frag<fp8>& a, const Frag<fp8>& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a.v, b.v, c, 0, 0, 0);
}
// f32: sub-step s feeds k = 8(l>>4) + s into the instruction's k slot (l>>4),
// identically for A and B, so the 8 instructions cover the 32-chunk exactly.
__device__ __forceinline__ f32x4 mfma_chunk(const Frag<float>& a, const Frag<float>& b, f32x4 c) {
#pragma unroll
    for (int s = 0; s < 8; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[s], b.v[s], c, 0, 0, 0);
    return c;
}

template <typename T>
__device__ __forceinline__ T to_t(float x);
template <>
__device__ __forceinline__ float to_t<float>(float x) { return x; }
template <>
__device__ __forceinline__ bf16 to_t<bf16>(float x) { return (bf16)x; }
template <>
__device__ __forceinline__ fp8 to_t<fp8>(float x) { return fp8{(uint8_t)(pack4_fp8(x, 0.f, 0.f, 0.f) & 0xff)}; }

enum { ACT_NONE = 0, ACT_LEAKY = 1, ACT_RELU = 2 };
__device__ __forceinline__ float apply_act(float v, int act, float alpha) {
    if (act == ACT_LEAKY) return v >= 0.f ? v : v * alpha;
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    return v;
}

// ---------------------------------------------------------------------------
// conv_small: C_in == 1, VALU.  One thread per output pixel, all COUT channels.
// ---------------------------------------------------------------------------
template <typename TO, int KH, int KW, int COUT>
__global__ __launch_bounds__(256) void conv_small(const float* __restrict__ in, int Hin, int Win,
                                                  const float* __restrict__ wt /*[COUT][KH*KW]*/,
                                                  const float* __restrict__ bias, int has_mag,
                                                  float mag_exp, TO* __restrict__ out, int Hc, int Wc,
                                                  int act, float alpha) {
    __shared__ float sw[COUT * KH * KW];
    __shared__ float sb[COUT];
    for (int i = threadIdx.x; i < COUT * KH * KW; i += blockDim.x) sw[i] = wt[i];
    for (int i = threadIdx.x; i < COUT; i += blockDim.x) sb[i] = bias[i];
    __syncthreads();
    const int n = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= Hc * Wc) return;
    const int h = p / Wc, w = p - (p / Wc) * Wc;
    float x[KH * KW];
    const float* src = in + (size_t)n * Hin * Win;
#pragma unroll
    for (int i = 0; i < KH; ++i)
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            float v = src[(h + i) * Win + w + j];
            if (has_mag) v = powf(v, mag_exp);
            x[i * KW + j] = v;
        }
    TO* o = out + ((size_t)n * Hc * Wc + p) * COUT;
#pragma unroll
    for (int c0 = 0; c0 < COUT; c0 += 8) {
        float r[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < KH * KW; ++t) s = fmaf(x[t], sw[(c0 + c) * KH * KW + t], s);
            r[c] = apply_act(s + sb[c0 + c], act, alpha);
        }
        if constexpr (sizeof(TO) == 1) {
            *reinterpret_cast<uint2*>(o + c0) =
                make_uint2(pack4_fp8(r[0], r[1], r[2], r[3]), pack4_fp8(r[4], r[5], r[6], r[7]));
        } else if constexpr (sizeof(TO) == 2) {
            bf16x8 v;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (bf16)r[c];
            *reinterpret_cast<bf16x8*>(o + c0) = v;
        } else {
            reinterpret_cast<float4*>(o + c0)[0] = make_float4(r[0], r[1], r[2], r[3]);
            reinterpret_cast<float4*>(o + c0)[1] = make_float4(r[4], r[5], r[6], r[7]);
        }
    }
}

// ---------------------------------------------------------------------------
// conv_mfma: implicit-GEMM conv, C_in % 32 == 0, fused pool/bias/act.
// Block = 4 waves = WM (pixel) x WN (channel); wave = MF x NF 16x16 tiles.
// ---------------------------------------------------------------------------
// Padded row length (elements) of the staged patch and of the weight slices:
// bf16 rows padded by 32 B (stride = 2 mod 4 16-B units, which makes every
// ds_read_b128 lane group of the fragment reads conflict-free); fp8 rows
// padded by 16 B (48 / 80 / 144-B strides put the 16 rows of a ds_read_b64
// half-wave on distinct 4-bank groups); f32 (parity mode) keeps a 16-B pad.
template <typename T>
__host__ __device__ constexpr int conv_cstr(int cin) {
    return cin + (sizeof(T) == 1 ? 16 : sizeof(T) == 2 ? 16 : 4);
}

// LDS of one conv_mfma block: [staged patch][f32 log-mel patch if FUSED]
// [2 x weight slice], and afterwards the epilogue tile reusing it from 0.
template <typename T, int KH, int KW, int CIN, int TH, int TW, bool FUSED>
__host__ __device__ constexpr size_t conv_b_offset() {
    constexpr int CSTR = conv_cstr<T>(CIN);
    size_t off = ((size_t)(TH + KH - 1) * (TW + KW - 1) * CSTR * sizeof(typename Prec<T>::L) + 15) & ~(size_t)15;
    if (FUSED) off += ((sizeof(float) * (TH + KH + 1) * (TW + KW + 1)) + 15) & ~(size_t)15;
    return off;
}

// fp8 runs the block-scaled K = 128 MFMA (v_mfma_f32_16x16x128_f8f6f4, the
// scale operands literal 0 = unscaled, 2x the non-scaled fp8 rate): its K
// loop walks "super-steps" of four 32-deep chunks (chunk k = tap * C_in/32 +
// channel chunk), and its weights are packed per super-step as rows of
// 4 x 32 B (+16 B pad) instead of per tap.
// C_in = 32 layers keep the non-scaled K = 32 form: 9 taps are 9 chunks, and
// packed into K = 128 they would waste a quarter of the MFMA work (measured
// in the pipeline: fused first conv 64 -> 75 us, 3x3/32 19 -> 22 us).
constexpr int F8_BSTR = 144;  // bytes of one packed fp8 weight row (128 + pad)
template <typename T>
__host__ __device__ constexpr bool conv_k128(int cin) {
    return is_fp8<T>() && cin >= 64;
}
template <typename T>
__host__ __device__ constexpr int conv_bstr(int cin) {  // weight-row stride (elements) of one step's slice
    return conv_k128<T>(cin) ? F8_BSTR : conv_cstr<T>(cin);
}
template <typename T>
__host__ __device__ constexpr int conv_nstep(int ntap, int cin) {  // K-loop steps (= weight slices)
    return conv_k128<T>(cin) ? (ntap * (cin / 32) + 3) / 4 : ntap;
}

// One step's weight slice [BN][BSTR] in LDS, rounded up to whole 1-KiB
// wave-instructions of global_load_lds (the tail lanes land in the rounding).
template <typename T, int CIN, int BN>
__host__ __device__ constexpr int conv_slice_lds_bytes() {
    return (BN * conv_bstr<T>(CIN) * (int)sizeof(typename Prec<T>::L) + 1023) / 1024 * 1024;
}

template <typename T, int KH, int KW, int CIN, int BN, int TH, int TW, bool FUSED, bool EBF16>
constexpr size_t conv_lds_bytes_nb(int nb) {
    const size_t main = conv_b_offset<T, KH, KW, CIN, TH, TW, FUSED>() + (size_t)nb * conv_slice_lds_bytes<T, CIN, BN>();
    const size_t epi = (size_t)TH * TW * (BN + (EBF16 ? 8 : 4)) * (EBF16 ? 2 : 4);
    return main > epi ? main : epi;
}

// Depth of the LDS ring of weight slices: as many buffers (up to 8, at most
// one per tap) as fit without lowering the blocks per CU that a 2-deep ring
// allows.  Slices in flight = ring - 1.
template <typename T, int KH, int KW, int CIN, int BN, int TH, int TW, bool FUSED, bool EBF16>
constexpr int conv_ring() {
    constexpr size_t cap = 160 * 1024;
    // fp8: the loop reads slice s+1 while s+NB-1 is issued (one-step software pipeline): >= 3
    constexpr int NB0 = conv_k128<T>(CIN) ? 3 : 2;
    const size_t base = conv_lds_bytes_nb<T, KH, KW, CIN, BN, TH, TW, FUSED, EBF16>(NB0);
    const size_t blocks = cap / base;
    int nb = NB0;
    while (nb < 8 && nb < conv_nstep<T>(KH * KW, CIN) &&
           blocks * conv_lds_bytes_nb<T, KH, KW, CIN, BN, TH, TW, FUSED, EBF16>(nb + 1) <= cap)
        ++nb;
    return nb;
}

template <typename T, int KH, int KW, int CIN, int BN, int TH, int TW, bool FUSED, bool EBF16>
constexpr size_t conv_lds_bytes() {
    return conv_lds_bytes_nb<T, KH, KW, CIN, BN, TH, TW, FUSED, EBF16>(
        conv_ring<T, KH, KW, CIN, BN, TH, TW, FUSED, EBF16>());
}

// s_waitcnt vmcnt(N) with N = PER * k for a runtime k in [0, 7] (the
// immediate must be a literal), lgkmcnt(0) alongside.
template <int PER>
__device__ __forceinline__ void wait_vm_lgkm(int k) {
#define AA_W(K) case K: asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PER * K) : "memory"); break;
    switch (k) { AA_W(0) AA_W(1) AA_W(2) AA_W(3) AA_W(4) AA_W(5) AA_W(6) default: AA_W(7) }
#undef AA_W
}

// s_waitcnt vmcnt(N) alone (LDS reads stay in flight), N = PER * k
template <int PER>
__device__ __forceinline__ void wait_vm(int k) {
#define AA_W(K) case K: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER * K) : "memory"); break;
    switch (k) { AA_W(0) AA_W(1) AA_W(2) AA_W(3) AA_W(4) AA_W(5) AA_W(6) default: AA_W(7) }
#undef AA_W
}

// First layer fused into the next conv's patch staging (FUSED = true): the
// log-mel patch is staged in LDS and the C_in = 1, 3x3 conv (f32 VALU, folded
// BN, activation, optional MagTransform prologue) writes the activations the
// MFMA loop consumes straight into the LDS patch -- the first layer's output
// never reaches HBM.
struct FirstConv {
    const float* w;  // [32][9] folded
    const float* b;  // [32]
    int act;
    float alpha;
    int has_mag;
    float mag_exp;
    int H0, W0;      // log-mel image
    int lm_f16;      // log-mel stored as float16 (aa_model_set_input_f16)
    const void* img; // conv_x3: the per-lane image of w and b (aa_cnn_pack.h pack_first_lanes)
};

// one log-mel value of the fused first conv's input (f32, or f16 when lm_f16)
__device__ __forceinline__ float load_lm(const void* in, size_t i, int lm_f16) {
    return lm_f16 ? (float)reinterpret_cast<const _Float16*>(in)[i] : reinterpret_cast<const float*>(in)[i];
}

// DIAG (diagnostic builds only, tools/conv_bench.hip): bit 0 skips the patch
// staging, bit 1 the MFMA loop, bit 2 the epilogue stores, bit 3 makes every
// lane read pixel 0 (no LDS bank conflicts), bit 4 re-reads chunk 0's weights
// (L1-resident, no L2 stream), bit 5 skips the weight loads in the loop, bit 7
// skips the fragment reads after the first (MFMA issue alone), bit 6 the
// fused first conv's compute, bit 9 its log-mel patch load.
// Waves per SIMD a conv_mfma block shape reaches (LDS-limited), told to the
// compiler so it schedules for latency at that occupancy instead of trimming
// registers for an occupancy the LDS footprint never allows.
template <typename T, int KH, int KW, int CIN, int WM, int WN, int NF, int TH, int TW, bool FUSED, bool EBF16>
constexpr int conv_waves_per_simd() {
    constexpr size_t lds = conv_lds_bytes<T, KH, KW, CIN, WN * NF * 16, TH, TW, FUSED, EBF16>();
    constexpr int blocks = (int)((160 * 1024) / lds);
    constexpr int w = blocks * WM * WN / 4;
    return w < 1 ? 1 : (w > 8 ? 8 : w);
}

template <typename T, int KH, int KW, int CIN, int WM, int WN, int MF, int NF, int POOL, int TH, int TW,
          bool FUSED = false, int DIAG = 0, bool EBF16 = false, int OCC = 0>
__global__ __launch_bounds__(WM * WN * 64)
__attribute__((amdgpu_waves_per_eu(OCC ? OCC : conv_waves_per_simd<T, KH, KW, CIN, WM, WN, NF, TH, TW, FUSED, EBF16>(),
                                    OCC ? OCC : conv_waves_per_simd<T, KH, KW, CIN, WM, WN, NF, TH, TW, FUSED, EBF16>())))
void conv_mfma(const typename Prec<T>::G* __restrict__ in, int Hin, int Win,
                                                 const typename Prec<T>::L* __restrict__ wt, const float* __restrict__ bias,
                                                 typename Prec<T>::G* __restrict__ out, int Hout, int Wout, int cout_store,
                                                 int tiles_w, int act, float alpha, FirstConv fc) {
    using LT = typename Prec<T>::L;  // LDS / fragment element
    using GT = typename Prec<T>::G;  // HBM activation element
    constexpr bool F8 = is_fp8<T>();
    static_assert(!is_split<T>(), "split-bf16 runs conv_x3 (aa_conv_x3.h)");
    static_assert(TH % POOL == 0 && TW % POOL == 0, "pool-aligned tile");
    static_assert(TH * TW <= WM * MF * 16, "tile covered by the waves' fragments");
    constexpr int NTHR = WM * WN * 64;
    static_assert(CIN % 32 == 0, "C_in multiple of 32");
    constexpr int BN = WN * NF * 16;
    constexpr int VEC = 16 / sizeof(LT);
    constexpr int CSTR = conv_cstr<T>(CIN);  // padded pixel / weight-row stride
    // epilogue tile: f32, or bf16 with the bias already added (rounding is
    // monotone, so max-pooling the rounded values equals rounding the max)
    using ET = typename std::conditional<EBF16, bf16, float>::type;
    constexpr int ESTR = BN + (EBF16 ? 8 : 4);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LT* patch = reinterpret_cast<LT*>(smem);

    const int n = blockIdx.z;
    const int th = blockIdx.x / tiles_w, tw = blockIdx.x - (blockIdx.x / tiles_w) * tiles_w;
    const int oh0 = th * TH, ow0 = tw * TW;
    constexpr int PH = TH + KH - 1, PW = TW + KW - 1;

    // The first NB - 1 weight slices of the K loop's LDS ring (described
    // there) are issued before the patch is staged, so their L2 round trip
    // overlaps the staging instead of following it.
    const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int NTAP = KH * KW;
    constexpr int CPC = CIN / 32;
    constexpr int NW = WM * WN;
    constexpr int NB = conv_ring<T, KH, KW, CIN, BN, TH, TW, FUSED, EBF16>();
    constexpr int NSTEP = conv_nstep<T>(NTAP, CIN);                // K-loop steps / weight slices
    constexpr int SLICE = BN * conv_bstr<T>(CIN);                  // elements
    constexpr int SLICE_LDS = conv_slice_lds_bytes<T, CIN, BN>();  // bytes
    constexpr int GPS = SLICE_LDS / 1024;                          // wave-instructions per slice
    constexpr int GHI = (GPS + NW - 1) / NW, GLO = GPS / NW;       // this wave's share: GHI if wave < GPS % NW
    char* Bs = smem + conv_b_offset<T, KH, KW, CIN, TH, TW, FUSED>();
    const size_t tap_stride = (size_t)gridDim.y * SLICE;
    const LT* wsl = wt + (size_t)blockIdx.y * SLICE + (threadIdx.x & 63) * VEC;
#define AA_GLDS(t)                                                                                       \
    _Pragma("unroll") for (int u_ = 0; u_ < GHI; ++u_) {                                               \
        const int g_ = u_ * NW + wave0;                                                                  \
        if (GPS % NW == 0 || g_ < GPS)                                                                  \
            __builtin_amdgcn_global_load_lds(                                                           \
                (const __attribute__((address_space(1))) void*)(wsl + (size_t)(t) * tap_stride + g_ * (1024 / sizeof(LT))), \
                (__attribute__((address_space(3))) void*)(Bs + ((t) % NB) * SLICE_LDS + g_ * 1024), 16, 0, 0); \
    }
    if constexpr (!(DIAG & 32)) {
#pragma unroll
        for (int t = 0; t < NB - 1; ++t)
            if (t < NSTEP) { AA_GLDS(t) }
    }

    // ---- stage the input patch ----
    if constexpr (DIAG & 1) {
    } else if constexpr (!FUSED) {
        // batched, unconditional 16-B loads from clamped addresses (a
        // load-or-zero branch would serialise them); out-of-image pixels only
        // feed discarded outputs but are zeroed anyway
        constexpr int VPP = CIN / VEC;  // 16-B vectors per pixel
        constexpr int U = 4;
        const int total = PH * PW * VPP;
        const GT* src = in + (size_t)n * Hin * Win * CIN;
        for (int i0 = 0; i0 < total; i0 += U * NTHR) {
            uint4 v[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + u * NTHR + threadIdx.x;
                const int pix = idx / VPP, cv = idx - pix * VPP;
                const int r = pix / PW, c = pix - r * PW;
                const int gh = oh0 + r, gw = ow0 + c;
                ok[u] = idx < total && gh < Hin && gw < Win;
                const int ch = min(gh, Hin - 1), cw = min(gw, Win - 1);
                v[u] = *reinterpret_cast<const uint4*>(src + ((size_t)ch * Win + cw) * CIN + cv * VEC);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + u * NTHR + threadIdx.x;
                if (idx < total) {
                    const int pix = idx / VPP, cv = idx - pix * VPP;
                    *reinterpret_cast<uint4*>(patch + pix * CSTR + cv * VEC) = ok[u] ? v[u] : make_uint4(0, 0, 0, 0);
                }
            }
        }
    } else {
        static_assert(CIN == 32, "fused first layer produces 32 channels");
        // (a) log-mel patch (PH+2) x (PW+2), f32, after the activation patch
        constexpr int XW = PW + 2, XN = (PH + 2) * XW;
        const size_t pbytes = ((size_t)PH * PW * CSTR * sizeof(LT) + 15) & ~(size_t)15;
        float* X = reinterpret_cast<float*>(smem + pbytes);
        const size_t lmo = (size_t)n * fc.H0 * fc.W0;
        for (int i0 = 0; i0 < ((DIAG & 512) ? 0 : XN); i0 += 4 * NTHR) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = min(i0 + u * NTHR + (int)threadIdx.x, XN - 1);
                const int r = idx / XW, c = idx - r * XW;
                v[u] = load_lm(in, lmo + (size_t)min(oh0 + r, fc.H0 - 1) * fc.W0 + min(ow0 + c, fc.W0 - 1), fc.lm_f16);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = i0 + u * NTHR + threadIdx.x;
                if (idx < XN) X[idx] = fc.has_mag ? powf(v[u], fc.mag_exp) : v[u];
            }
        }
        if constexpr (sizeof(LT) <= 2) {
            // (b) first conv on the matrix cores: per 32 patch pixels one
            // v_mfma_f32_32x32x16_bf16, D[32 ch][32 px] = W[32 ch][16 k] X[16 k][32 px]
            // with the 9 taps in k (0..8; weights 0 for k = 9..15, so those
            // B entries may hold any finite value), the bias as the C input,
            // then the activation, bf16, and 8-byte stores of 4 channels into
            // the patch.  Lane l: pixel l % 32, k-group / channel quad l / 32.
            const int wave1 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
            const int l32 = threadIdx.x & 31, kg = (threadIdx.x >> 5) & 1;
            bf16x8 wa;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int tap = 8 * kg + j;
                wa[j] = tap < 9 ? (bf16)fc.w[l32 * 9 + tap] : (bf16)0.f;
            }
            f32x16 cb;  // D row (channel) of register r: 8 (r / 4) + 4 kg + r % 4
#pragma unroll
            for (int r = 0; r < 16; ++r) cb[r] = fc.b[8 * (r >> 2) + 4 * kg + (r & 3)];
            const float ae = fc.alpha;  // host: act folded to a slope in [0, 1]
            // tap offsets into X: k = 8 kg + j; k-group 1 only needs tap 8 (j = 0)
            const int off0 = kg ? 2 * XW + 2 : 0;
            __syncthreads();
            constexpr int NPX = PH * PW;
            // bf16: two pixel groups per iteration, so independent MFMA chains
            // (and their LDS reads) interleave instead of waiting out each
            // chain's latency (in-pipeline A/B: +0.7 % bench; fp8 -0.7 %, so one)
            constexpr int NG = (NPX + 31) / 32;
            constexpr int UG = std::is_same<T, bf16>::value ? 2 : 1;
            for (int g0 = wave1; g0 < ((DIAG & 64) ? 0 : NG); g0 += 4 * UG) {
                bf16x8 xh[UG], xl[UG];
                int pix[UG];
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    pix[u] = min((g0 + 4 * u) * 32 + l32, NPX - 1);
                    const int r = pix[u] / PW, c = pix[u] - r * PW;
                    const float* xp = X + r * XW + c;
                    float xv[8];
                    xv[0] = xp[off0];
#pragma unroll
                    for (int j = 1; j < 8; ++j) xv[j] = xp[(j / 3) * XW + j % 3];
                    // the log-mel as bf16 hi + lo (x - hi, exact in f32): two MFMAs
                    // keep ~16 significant bits of the input
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        xh[u][j] = (bf16)xv[j];
                        xl[u][j] = (bf16)(xv[j] - (float)xh[u][j]);
                    }
                }
                f32x16 d[UG];
#pragma unroll
                for (int u = 0; u < UG; ++u) d[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, xh[u], cb, 0, 0, 0);
#pragma unroll
                for (int u = 0; u < UG; ++u) d[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, xl[u], d[u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    if ((g0 + 4 * u) * 32 + l32 < NPX) {
                        LT* dst = patch + pix[u] * CSTR + 4 * kg;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if constexpr (F8) {
                                float o[4];
#pragma unroll
                                for (int e = 0; e < 4; ++e) o[e] = fmaxf(d[u][4 * q + e], d[u][4 * q + e] * ae);
                                *reinterpret_cast<uint32_t*>(dst + 8 * q) = pack4_fp8(o[0], o[1], o[2], o[3]);
                            } else {
                                typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
                                bf16x4 o;
#pragma unroll
                                for (int e = 0; e < 4; ++e) o[e] = (bf16)fmaxf(d[u][4 * q + e], d[u][4 * q + e] * ae);
                                *reinterpret_cast<bf16x4*>(dst + 8 * q) = o;
                            }
                        }
                    }
                }
            }
        } else {
            // (b) first conv: wave -> 8 output channels (wave-uniform, so its 72
            // weights and 8 biases are scalar loads), lane -> one patch column; the
            // lane slides the 3x3 window down its column (3 new LDS reads per
            // output row) and computes channel pairs with packed FMAs, each f32
            // chain started at the bias (only the bf16 path fuses; the f32 parity
            // mode runs conv_small).  Activation as max(v, a v): the planner
            // fuses only when the activation has 0 <= a <= 1 (none: 1, relu: 0).
            static_assert(NTHR == 256 && PW <= 64, "fused first layer: 4 waves, patch width <= 64");
            const int cg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
            const int col = threadIdx.x & 63;
            f32x2 w1[9][4];
            f32x2 b1[4];
    #pragma unroll
            for (int k = 0; k < 4; ++k) {
                b1[k] = f32x2{fc.b[cg * 8 + 2 * k], fc.b[cg * 8 + 2 * k + 1]};
    #pragma unroll
                for (int t = 0; t < 9; ++t)
                    w1[t][k] = f32x2{fc.w[(cg * 8 + 2 * k) * 9 + t], fc.w[(cg * 8 + 2 * k + 1) * 9 + t]};
            }
            const float ae = fc.alpha;  // host: act folded to a slope in [0, 1]
            __syncthreads();
            if (col < PW) {
                float xr[3][3];
    #pragma unroll
                for (int i = 0; i < 2; ++i)
    #pragma unroll
                    for (int j = 0; j < 3; ++j) xr[i][j] = X[i * XW + col + j];
    #pragma unroll
                for (int r = 0; r < PH; ++r) {
    #pragma unroll
                    for (int j = 0; j < 3; ++j) xr[(r + 2) % 3][j] = X[(r + 2) * XW + col + j];
                    f32x2 acc[4];  // the bias starts the chain (bf16 path only: f32 parity runs conv_small)
    #pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = b1[k];
    #pragma unroll
                    for (int i = 0; i < 3; ++i)
    #pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            const float xv = xr[(r + i) % 3][j];
    #pragma unroll
                            for (int k = 0; k < 4; ++k)
                                acc[k] = __builtin_elementwise_fma(f32x2{xv, xv}, w1[i * 3 + j][k], acc[k]);
                        }
                    float o[8];
    #pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const f32x2 v = acc[k];
                        const f32x2 sv = v * ae;
                        o[2 * k] = fmaxf(v.x, sv.x);
                        o[2 * k + 1] = fmaxf(v.y, sv.y);
                    }
                    LT* dst = patch + (r * PW + col) * CSTR + cg * 8;
                    if constexpr (sizeof(LT) == 2) {
                        bf16x8 v;
    #pragma unroll
                        for (int ch = 0; ch < 8; ++ch) v[ch] = (bf16)o[ch];
                        *reinterpret_cast<bf16x8*>(dst) = v;
                    } else {
                        reinterpret_cast<float4*>(dst)[0] = make_float4(o[0], o[1], o[2], o[3]);
                        reinterpret_cast<float4*>(dst)[1] = make_float4(o[4], o[5], o[6], o[7]);
                    }
                }
            }
        }
        }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int wm = wave % WM, wn = wave / WM;
    const int q8 = 8 * (lane >> 4);
    constexpr int TP = TH * TW;
    int abase[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        int p = (wm * MF + i) * 16 + (lane & 15);
        if (p >= TP || (DIAG & 8)) p = 0;  // padding rows: computed, never stored
        const int r = p / TW, c = p - (p / TW) * TW;
        abase[i] = (r * PW + c) * CSTR + q8;
    }
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- K loop, one tap (kh, kw) at a time.  Weights are packed tap-major
    // with padded rows, [tap][cout_pad][CSTR], so a block's slice of one tap
    // is one contiguous [BN][CSTR] block whose bytes are exactly its LDS
    // image.  global_load_lds streams the slices through a ring of NB LDS
    // buffers, NB - 1 taps ahead of the one computing (an L2 round trip of
    // a slice outlasts one tap's MFMAs): at the top of tap t each wave waits
    // for its own loads of slice t with a counted vmcnt (later slices stay in
    // flight), one barrier publishes slice t to every wave and retires all
    // reads of the buffer slice t + NB - 1 will overwrite, then that slice is
    // issued.  A fragments come from the staged patch. ----
    const int brow = (wn * NF * 16 + (lane & 15)) * CSTR + q8;
    const bool hi_share = (GPS % NW == 0) || wave < GPS % NW;
    // Fragments are double-buffered in registers: while chunk q's MFMAs run,
    // chunk q+1's fragments are in flight.  Across a tap boundary only the A
    // fragments (from the static patch) can run ahead; the next slice's B
    // fragments follow the barrier that publishes it.
    Frag<LT> fa[MF], fb[NF], na[MF], nb[NF];
#define AA_LOAD_A(dst, tap, cc_)                                                             \
    if (!(DIAG & 128) || (tap) == 0)                                                         \
    {                                                                                        \
        const int kh_ = (tap) / KW, kw_ = (tap) - ((tap) / KW) * KW;                         \
        const int at_ = (kh_ * PW + kw_) * CSTR + (cc_) * 32;                                \
        _Pragma("unroll") for (int i = 0; i < MF; ++i) dst[i].load(patch + abase[i] + at_); \
    }
#define AA_LOAD_B(dst, buf, cc_)                                                             \
    if (!(DIAG & 128) || (buf) < 0)                                                          \
    {                                                                                        \
        const LT* bt_ = reinterpret_cast<const LT*>(Bs + (buf) * SLICE_LDS) + brow + (cc_) * 32; \
        _Pragma("unroll") for (int j = 0; j < NF; ++j) dst[j].load(bt_ + j * 16 * CSTR);   \
    }
    // f32 (parity mode) fragments are twice as wide: single-buffered there
    constexpr bool DB = !std::is_same<T, float>::value;
    if constexpr (conv_k128<T>(CIN)) {
        // ---- fp8, C_in >= 64: K = 128 per MFMA.  Super-step s covers chunks 4s .. 4s+3
        // (chunk k: tap k / CPC, channel chunk k % CPC); lane group q's 32
        // fragment bytes are its 8 bytes (channels 8q .. 8q+7) of each of the
        // four chunks, read as four ds_read_b64 from the patch (A, pixels)
        // and from the super-step's weight slice (B, rows of 4 x 32 B), in the
        // same order for both operands -- the instruction's k order is the
        // same permutation for A and B (tools/mfma_scale_probe.hip), so the
        // product is the sum over the four chunks.  Chunks past the last tap
        // have zero weights (their A reads re-read chunk 0: finite values).
        // Software-pipelined by one step: the barrier at the top of step s
        // publishes slice s+1, whose B fragments are read while step s's
        // MFMAs run; A fragments are read just in time, two in flight. ----
        typedef __attribute__((ext_vector_type(8))) int i32x8;
        typedef __attribute__((ext_vector_type(2))) int i32x2;
        constexpr int NCH = NTAP * CPC;
        const int browf = (wn * NF * 16 + (lane & 15)) * F8_BSTR + q8;
        auto choff = [&](int k) {
            k = k < NCH ? k : 0;
            const int t = k / CPC, cc = k - (k / CPC) * CPC;
            const int kh = t / KW, kw = t - (t / KW) * KW;
            return (kh * PW + kw) * CSTR + cc * 32;
        };
        auto rd4 = [](i32x8& v, const char* p0, const char* p1, const char* p2, const char* p3) {
            const i32x2 x0 = *reinterpret_cast<const i32x2*>(p0), x1 = *reinterpret_cast<const i32x2*>(p1);
            const i32x2 x2 = *reinterpret_cast<const i32x2*>(p2), x3 = *reinterpret_cast<const i32x2*>(p3);
            v = i32x8{x0[0], x0[1], x1[0], x1[1], x2[0], x2[1], x3[0], x3[1]};
        };
        auto read_b8 = [&](i32x8* b, int st) {
            const char* bt = Bs + (st % NB) * SLICE_LDS + browf;
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const char* r = bt + j * 16 * F8_BSTR;
                rd4(b[j], r, r + 32, r + 64, r + 96);
            }
        };
        const char* pb = reinterpret_cast<const char*>(patch);
        auto f8step = [&](i32x8* bc, i32x8* bn, int st) {
            if (st + 1 < NSTEP && !(DIAG & 32)) {
                // own share of slice st+1 landed (st+2 .. st+NB-2 may stay in
                // flight); this wave's reads of slice st-1 (whose buffer the
                // next issue overwrites) were consumed by step st-1's MFMAs
                const int ahead = min(NB - 3, NSTEP - 2 - st);
                if (hi_share) wait_vm<GHI>(ahead);
                else wait_vm<GLO>(ahead);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                if (st + NB - 1 < NSTEP) { AA_GLDS(st + NB - 1) }  // into the buffer slice st-1 was read from
            }
            const int o0 = choff(4 * st), o1 = choff(4 * st + 1), o2 = choff(4 * st + 2), o3 = choff(4 * st + 3);
            // A fragments three deep (fragment i+2 in flight under fragment
            // i's MFMAs), the next step's B fragments issued after the first
            // two A reads so the first MFMAs do not wait behind them (LDS
            // reads retire in order)
            i32x8 a3[3];
            auto rda = [&](int i, int k) {
                if ((DIAG & 128) && st > 0) return;
                const char* a = pb + abase[i];
                rd4(a3[k], a + o0, a + o1, a + o2, a + o3);
            };
            rda(0, 0);
            if (MF > 1) rda(1, 1);
            if (st + 1 < NSTEP && !((DIAG & 128) && st > 0)) read_b8(bn, st + 1);
#pragma unroll
            for (int i = 0; i < MF; ++i) {
                if (i + 2 < MF) rda(i + 2, (i + 2) % 3);
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bc[j], a3[i % 3], acc[i][j], 0, 0, 0, 0,
                                                                                 0, 0);
            }
        };
        i32x8 B0[NF], B1[NF];
        {  // slice 0: own share landed (later slices stay in flight), one barrier publishes it
            const int ahead = min(NB - 2, NSTEP - 1);
            if (hi_share) wait_vm_lgkm<GHI>(ahead);
            else wait_vm_lgkm<GLO>(ahead);
            __builtin_amdgcn_s_barrier();
            read_b8(B0, 0);
        }
        for (int st = 0; st < NSTEP; st += 2) {
            f8step(B0, B1, st);
            if (st + 1 < NSTEP) f8step(B1, B0, st + 1);
        }
    } else {
    if constexpr (DB) AA_LOAD_A(fa, 0, 0)
    for (int t = 0; t < ((DIAG & 2) ? 0 : NTAP); ++t) {
        // slices t+1 .. min(t+NB-2, NTAP-1) may stay in flight
        const int ahead = min(NB - 2, NTAP - 1 - t);
        if (DIAG & 32) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        } else if (hi_share) {
            wait_vm_lgkm<GHI>(ahead);
        } else {
            wait_vm_lgkm<GLO>(ahead);
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!(DIAG & 32)) {
            if (t + NB - 1 < NTAP) { AA_GLDS(t + NB - 1) }
        }
        const int buf = (DIAG & 16) ? 0 : (t % NB);
        if constexpr (!DB) {
#pragma unroll
            for (int cc = 0; cc < CPC; ++cc) {
                AA_LOAD_A(fa, t, cc)
                AA_LOAD_B(fb, buf, cc)
#pragma unroll
                for (int i = 0; i < MF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j) acc[i][j] = mfma_chunk(fb[j], fa[i], acc[i][j]);
            }
            continue;
        }
        AA_LOAD_B(fb, buf, 0)
#pragma unroll
        for (int cc = 0; cc < CPC; ++cc) {
            if (cc + 1 < CPC) {
                AA_LOAD_A(na, t, cc + 1)
                AA_LOAD_B(nb, buf, cc + 1)
            } else if (t + 1 < NTAP) {
                AA_LOAD_A(na, t + 1, 0)
            }
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = mfma_chunk(fb[j], fa[i], acc[i][j]);
#pragma unroll
            for (int i = 0; i < MF; ++i) fa[i] = na[i];
            if (cc + 1 < CPC) {
#pragma unroll
                for (int j = 0; j < NF; ++j) fb[j] = nb[j];
            }
        }
    }
    }  // !K128
#undef AA_LOAD_A
#undef AA_LOAD_B
#undef AA_GLDS
    __syncthreads();  // patch no longer needed: reuse LDS for the f32 tile

    // The MFMAs compute D = W X^T (weights as the A operand): lane holds
    // output channels c0 .. c0 + 3 of pixel p, stored as one 8-byte (bf16) /
    // 16-byte (f32) vector per fragment
    ET* E = reinterpret_cast<ET*>(smem);
    // fp8: per-output-channel dequantisation scales follow the bias (both padded to cout_pad)
    const float* wscale = bias + gridDim.y * BN;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int c0 = wn * NF * 16 + j * 16 + 4 * (lane >> 4);
        float bj[4], sj[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bj[r] = EBF16 ? bias[blockIdx.y * BN + c0 + r] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) sj[r] = (EBF16 && F8) ? wscale[blockIdx.y * BN + c0 + r] : 1.f;
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int p = (wm * MF + i) * 16 + (lane & 15);
            if (p < TP) {
                ET* e = E + p * ESTR + c0;
                if constexpr (EBF16) {
                    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
                    bf16x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = (bf16)(F8 ? fmaf(acc[i][j][r], sj[r], bj[r]) : acc[i][j][r] + bj[r]);
                    *reinterpret_cast<bf16x4*>(e) = v;
                } else {
                    *reinterpret_cast<float4*>(e) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                }
            }
        }
    }
    __syncthreads();

    // pooled outputs: each thread owns one 8-channel group (bias in registers)
    // and writes 16-B (bf16) / 32-B (f32) vectors
    constexpr int PHo = TH / POOL, PWo = TW / POOL;
    constexpr int G = BN / 8;
    static_assert(NTHR % G == 0, "fixed channel group per thread");
    const int oh0s = oh0 / POOL, ow0s = ow0 / POOL;
    const int col = (threadIdx.x % G) * 8;
    const int ch0 = blockIdx.y * BN + col;
    float bv[8], sv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) bv[c] = EBF16 ? 0.f : bias[ch0 + c];  // bias is padded to cout_pad
#pragma unroll
    for (int c = 0; c < 8; ++c) sv[c] = (!EBF16 && F8) ? wscale[ch0 + c] : 1.f;
    GT* dst = out + (size_t)n * Hout * Wout * cout_store;
    for (int q = threadIdx.x / G; q < PHo * PWo; q += NTHR / G) {
        const int pr = q / PWo, pc = q - (q / PWo) * PWo;
        const int gh = oh0s + pr, gw = ow0s + pc;
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < POOL; ++dy)
#pragma unroll
            for (int dx = 0; dx < POOL; ++dx) {
                const ET* e = E + ((pr * POOL + dy) * TW + pc * POOL + dx) * ESTR + col;
                if constexpr (EBF16) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(e);
#pragma unroll
                    for (int c = 0; c < 8; ++c) v[c] = fmaxf(v[c], (float)a[c]);
                } else {
                    const float4 a = reinterpret_cast<const float4*>(e)[0], b = reinterpret_cast<const float4*>(e)[1];
                    v[0] = fmaxf(v[0], a.x); v[1] = fmaxf(v[1], a.y); v[2] = fmaxf(v[2], a.z); v[3] = fmaxf(v[3], a.w);
                    v[4] = fmaxf(v[4], b.x); v[5] = fmaxf(v[5], b.y); v[6] = fmaxf(v[6], b.z); v[7] = fmaxf(v[7], b.w);
                }
            }
        if (gh >= Hout || gw >= Wout) continue;
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = apply_act((!EBF16 && F8) ? fmaf(v[c], sv[c], bv[c]) : v[c] + bv[c], act, alpha);
        if constexpr ((DIAG & 4) != 0) {
            if (v[0] != 12345.f) continue;  // keep the values live, store (almost) never
        }
        GT* o = dst + ((size_t)gh * Wout + gw) * cout_store + ch0;
        if (ch0 + 8 <= cout_store) {
            if constexpr (F8) {
                *reinterpret_cast<uint2*>(o) = make_uint2(pack4_fp8(v[0], v[1], v[2], v[3]), pack4_fp8(v[4], v[5], v[6], v[7]));
            } else if constexpr (sizeof(GT) == 2) {
                bf16x8 pk;
#pragma unroll
                for (int c = 0; c < 8; ++c) pk[c] = (bf16)v[c];
                *reinterpret_cast<bf16x8*>(o) = pk;
            } else {
                reinterpret_cast<float4*>(o)[0] = make_float4(v[0], v[1], v[2], v[3]);
                reinterpret_cast<float4*>(o)[1] = make_float4(v[4], v[5], v[6], v[7]);
            }
        } else {
            for (int c = 0; c < 8 && ch0 + c < cout_store; ++c) o[c] = to_t<GT>(v[c]);
        }
    }
}

// ---------------------------------------------------------------------------
// conv_head: 1x1 conv (C_in % 32 == 0) + global max + sigmoid.  Pixel ranges
// of 64 per block (blockIdx.y), 32 labels per block (blockIdx.z: label group);
// 4 waves along pixels, MF tiles each per chunk, NF = 2 label tiles.
// ---------------------------------------------------------------------------
template <typename T, int MF, int NF>
__global__ __launch_bounds__(256) void conv_head(const T* __restrict__ in, int HW, int cin,
                                                 const T* __restrict__ wt, const float* __restrict__ bias,
                                                 int L, int act, float alpha, int sigmoid,
                                                 float* __restrict__ logits, float* __restrict__ probs,
                                                 float* __restrict__ part, const float* __restrict__ wscale) {
    const int n = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q8 = 8 * (lane >> 4);
    const int lg = blockIdx.z * 16 * NF;  // first label of this block's group
    const T* src = in + (size_t)n * HW * cin;
    const T* bptr[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) bptr[j] = wt + (size_t)(lg + j * 16 + (lane & 15)) * cin + q8;
    float rmax[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) rmax[j] = -INFINITY;
    constexpr int CHUNK = 4 * MF * 16;
    for (int p0 = blockIdx.y * CHUNK; p0 < HW; p0 += CHUNK * gridDim.y) {
        f32x4 acc[MF][NF];
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        int arow[MF];
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int p = p0 + (wave * MF + i) * 16 + (lane & 15);
            arow[i] = (p < HW ? p : 0) * cin + q8;
        }
#pragma unroll 2
        for (int k0 = 0; k0 < cin; k0 += 32) {
            Frag<T> b[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) b[j].load(bptr[j] + k0);
#pragma unroll
            for (int i = 0; i < MF; ++i) {
                Frag<T> a;
                a.load(src + arow[i] + k0);
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = mfma_chunk(a, b[j], acc[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int prow = p0 + (wave * MF + i) * 16 + 4 * (lane >> 4);
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (prow + r < HW) rmax[j] = fmaxf(rmax[j], acc[i][j][r]);
        }
    }
    __shared__ float red[4][16 * NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        float v = rmax[j];
        v = fmaxf(v, __shfl_xor(v, 16, 64));
        v = fmaxf(v, __shfl_xor(v, 32, 64));
        if (lane < 16) red[wave][j * 16 + lane] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16 * NF) {  // one of gridDim.y pixel ranges: its column maxima, finished by head_final
        const int lp = gridDim.z * 16 * NF;  // cout_pad
        part[((size_t)n * gridDim.y + blockIdx.y) * lp + lg + threadIdx.x] =
            fmaxf(fmaxf(red[0][threadIdx.x], red[1][threadIdx.x]), fmaxf(red[2][threadIdx.x], red[3][threadIdx.x]));
    }
}

// global max over the head's pixel ranges, bias, activation, sigmoid
__global__ __launch_bounds__(256) void head_final(const float* __restrict__ part, int nparts, int width,
                                                  const float* __restrict__ bias, int L, int act, float alpha,
                                                  int sigmoid, float* __restrict__ logits,
                                                  float* __restrict__ probs, const float* __restrict__ wscale) {
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < L; c += blockDim.x) {
        const float* p = part + (size_t)n * nparts * width + c;
        float v = p[0];
        for (int k = 1; k < nparts; ++k) v = fmaxf(v, p[(size_t)k * width]);
        v = apply_act(wscale ? fmaf(v, wscale[c], bias[c]) : v + bias[c], act, alpha);
        logits[(size_t)n * L + c] = v;
        if (probs) probs[(size_t)n * L + c] = sigmoid ? 1.f / (1.f + expf(-v)) : v;
    }
}

// ---------------------------------------------------------------------------
// Generic stages for layer shapes no tuned kernel covers (the planner's
// fallback, exact f32 arithmetic on the VALU): any kernel size, any C_in,
// any max-pool window, optional MagTransform prologue.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(bf16 x) { return (float)x; }
__device__ __forceinline__ float to_f(fp8 x) {  // OCP e4m3fn
    const int s = x.v >> 7, e = (x.v >> 3) & 15, m = x.v & 7;
    float v = e ? ldexpf(1.f + m / 8.f, e - 7) : ldexpf(m / 8.f, -6);
    if (e == 15 && m == 7) v = NAN;
    return s ? -v : v;
}

// one thread = one (pooled) output pixel x 8 output channels; weights
// [cout][kh][kw][cin] f32 (BN folded), bias f32
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void conv_generic(const TI* __restrict__ in, int Hin, int Win, int cin,
                                                    const float* __restrict__ w, const float* __restrict__ bias,
                                                    int kh, int kw, int cout, int ph, int pw, int Hout, int Wout,
                                                    int act, float alpha, int has_mag, float mag_exp,
                                                    TO* __restrict__ out) {
    const int n = blockIdx.z;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = blockIdx.y * 8;
    if (p >= Hout * Wout) return;
    const int oh = p / Wout, ow = p - (p / Wout) * Wout;
    const int K = kh * kw * cin;
    const int nc = min(8, cout - c0);
    float best[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) best[o] = -INFINITY;
    const TI* img = in + (size_t)n * Hin * Win * cin;
    for (int dy = 0; dy < ph; ++dy)
        for (int dx = 0; dx < pw; ++dx) {
            const int h = oh * ph + dy, x = ow * pw + dx;
            float acc[8];
#pragma unroll
            for (int o = 0; o < 8; ++o) acc[o] = 0.f;
            for (int i = 0; i < kh; ++i)
                for (int j = 0; j < kw; ++j) {
                    const TI* src = img + ((size_t)(h + i) * Win + x + j) * cin;
                    const float* wk = w + (size_t)c0 * K + (i * kw + j) * cin;
                    for (int c = 0; c < cin; ++c) {
                        float v = to_f(src[c]);
                        if (has_mag) v = powf(v, mag_exp);
#pragma unroll
                        for (int o = 0; o < 8; ++o)
                            if (o < nc) acc[o] = fmaf(v, wk[(size_t)o * K + c], acc[o]);
                    }
                }
#pragma unroll
            for (int o = 0; o < 8; ++o)
                if (o < nc) best[o] = fmaxf(best[o], apply_act(acc[o] + bias[c0 + o], act, alpha));
        }
    TO* dst = out + ((size_t)(n * Hout + oh) * Wout + ow) * cout + c0;
    for (int o = 0; o < nc; ++o) dst[o] = to_t<TO>(best[o]);
}

// GlobalMaxPool2D over a stage's output, then an optional Dense layer
// (weights [C][U] f32, bias [U]) and sigmoid; one block per window
template <typename TI>
__global__ __launch_bounds__(256) void pool_dense(const TI* __restrict__ in, int HW, int C,
                                                  const float* __restrict__ w, const float* __restrict__ b, int U,
                                                  int sigmoid, float* __restrict__ logits, float* __restrict__ probs) {
    extern __shared__ float mx[];
    const int n = blockIdx.x;
    const TI* src = in + (size_t)n * HW * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float m = -INFINITY;
        for (int p = 0; p < HW; ++p) m = fmaxf(m, to_f(src[(size_t)p * C + c]));
        mx[c] = m;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < U; u += blockDim.x) {
        float v;
        if (w) {
            v = 0.f;
            for (int c = 0; c < C; ++c) v = fmaf(mx[c], w[(size_t)c * U + u], v);
            v += b[u];
        } else {
            v = mx[u];
        }
        logits[(size_t)n * U + u] = v;
        if (probs) probs[(size_t)n * U + u] = sigmoid ? 1.f / (1.f + expf(-v)) : v;
    }
}

// ---------------------------------------------------------------------------
// track mean: mean over models, then over the track's windows (f32,
// sequential, src/identify_tracks.py:547-551)
// ---------------------------------------------------------------------------
__global__ void track_mean(const float* __restrict__ probs, int n_models, long long model_stride, int L,
                           const int* __restrict__ wb, const int* __restrict__ wc,
                           float* __restrict__ out) {
    const int t = blockIdx.x;
    const int c = threadIdx.x;
    if (c >= L) return;
    constexpr int U = 40;  // loads in flight (a 60 s track has 39 windows); the adds stay in numpy's order
    float acc = 0.f;
    const int n = wc[t];
    const float* base = probs + (size_t)wb[t] * L + c;
    for (int w0 = 0; w0 < n; w0 += U) {
        float m[U];  // per window: ((0 + p_0) + p_1) + ..., numpy's axis-0 sum over models
#pragma unroll
        for (int u = 0; u < U; ++u) m[u] = 0.f;
        for (int k = 0; k < n_models; ++k) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = base[k * model_stride + (size_t)min(w0 + u, n - 1) * L];
#pragma unroll
            for (int u = 0; u < U; ++u) m[u] = __fadd_rn(m[u], v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (w0 + u < n) acc = __fadd_rn(acc, __fdiv_rn(m[u], (float)n_models));
    }
    out[(size_t)t * L + c] = n > 0 ? __fdiv_rn(acc, (float)n) : NAN;
}

}  // namespace aa

#include "aa_conv_x3.h"
#include "aa_conv_pair.h"
#include "aa_conv_wg.h"
#include "aa_gconv.h"
#include "aa_conv_tail.h"

namespace aa {

// ---------------------------------------------------------------------------
// Stage read-out (aa_model_forward_prefix): whatever a stage stored, as plain
// f32 NHWC.  MODE 0: f32 copied; 1: bf16 -> f32; 2: e4m3fn -> f32 (exact, bit
// arithmetic); 3: the grouped-split layout (aa_conv_x3.h: per pixel and
// 32-channel group 64 B of bf16 hi, then 64 B of bf16 lo) -> hi + lo, which
// is exact in f32 (lo is a multiple of the split value's f32 ulp).
// ---------------------------------------------------------------------------
template <int MODE>
__global__ void stage_decode(const void* __restrict__ src, float* __restrict__ dst, size_t total, int cout) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float v;
        if (MODE == 0) {
            v = static_cast<const float*>(src)[i];
        } else if (MODE == 1) {
            v = __uint_as_float((uint32_t) static_cast<const uint16_t*>(src)[i] << 16);
        } else if (MODE == 2) {
            const uint32_t b = static_cast<const uint8_t*>(src)[i];
            const int e = (b >> 3) & 15, m = b & 7;
            const float a = (e == 15 && m == 7) ? __uint_as_float(0x7fc00000u)
                            : e == 0            ? ldexpf((float)m, -9)
                                                : ldexpf((float)(8 + m), e - 10);
            v = (b & 0x80) ? -a : a;
        } else {
            const size_t pix = i / (size_t)cout;
            const int c = (int)(i - pix * (size_t)cout);
            const uint16_t* h = static_cast<const uint16_t*>(src) + pix * (size_t)cout * 2 + (size_t)(c >> 5) * 64 + (c & 31);
            v = __uint_as_float((uint32_t)h[0] << 16) + __uint_as_float((uint32_t)h[32] << 16);
        }
        dst[i] = v;
    }
}

}  // namespace aa

#include "aa_cnn_plan.h"

namespace aa {

// ---------------------------------------------------------------------------
// host: launchers, upload, forward, timing
// ---------------------------------------------------------------------------
// What the tuned conv launchers (conv_mfma, conv_x3, conv_wg) share: the fused
// first conv's arguments (`first` non-null), the kernel's LDS limit, and the
// grid of POOL-aligned TH x TW tiles x BN-channel blocks x windows.  window32:
// the kernel addresses one window's activations through buffer resources
// based at the window (64-bit) with 32-bit offsets inside it.  Then
// launch(grid, tiles_w, fc) starts the kernel.
template <typename Launch>
static int launch_tuned(const Stage& s, const Stage* first, int n, const void* kernel, size_t lds, bool window32,
                        int pool, int th, int tw, int bn, Launch&& launch) {
    if (window32)
        AA_CHECK((double)s.Hin * s.Win * s.cin * 4 < 2147483647.0, AA_ERR_UNSUPPORTED,
                 "conv %s: one window's activations exceed 2 GiB", s.name.c_str());
    FirstConv fc{};
    if (first) {
        const float slope = first->act == ACT_LEAKY ? first->alpha : first->act == ACT_RELU ? 0.f : 1.f;
        fc = FirstConv{(const float*)first->d_w, first->d_b, first->act, slope, first->has_mag,
                       first->mag_exp, first->Hin, first->Win, s.lm_f16, s.d_f1};
    }
    AA_CHECK(lds <= 160 * 1024, AA_ERR_UNSUPPORTED, "conv %s: %zu B LDS", s.name.c_str(), lds);
    AA_DYN_LDS(kernel, lds);
    const int tiles_h = (s.Hout * pool + th - 1) / th;
    const int tiles_w = (s.Wout * pool + tw - 1) / tw;
    launch(dim3(tiles_h * tiles_w, s.cout_pad / bn, n), tiles_w, fc);
    AA_LAUNCH_CHECK();
    return AA_OK;
}

template <typename T, int KH, int KW, int CIN, int WM, int WN, int MF, int NF, int POOL, int TH, int TW,
          bool FUSED = false, bool EBF16 = false, int OCC = 0>
static int launch_mfma(const Stage& s, const void* in, void* out, int n, hipStream_t st,
                       const Stage* first = nullptr) {
    auto k = conv_mfma<T, KH, KW, CIN, WM, WN, MF, NF, POOL, TH, TW, FUSED, 0, EBF16, OCC>;
    constexpr int BN = WN * NF * 16;
    const size_t lds = conv_lds_bytes<T, KH, KW, CIN, BN, TH, TW, FUSED, EBF16>();
    using GT = typename Prec<T>::G;
    using LT = typename Prec<T>::L;
    return launch_tuned(s, FUSED ? first : nullptr, n, (const void*)k, lds, false, POOL, TH, TW, BN,
                        [&](dim3 grid, int tiles_w, const FirstConv& fc) {
        hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, st, (const GT*)in, s.Hin, s.Win, (const LT*)s.d_w, s.d_b,
                           (GT*)out, s.Hout, s.Wout, s.cout, tiles_w, s.act, s.alpha, fc);
    });
}

template <int KH, int KW, int CIN, int WM, int WN, int MF, int NF, int POOL, int TH, int TW, bool RING, bool AJIT,
          int OCC, bool FUSED, bool IN_SPLIT, bool OUT_SPLIT, int LM = 0>
static int launch_x3(const Stage& s, const void* in, void* out, int n, hipStream_t st, const Stage* first) {
    // a fused first conv (launch_stage: pool 3 only): the instantiation for
    // its log-mel form (conv_x3's LM)
    if constexpr (FUSED && LM == 0 && POOL == 3) {
        const int lm = (s.lm_f16 ? 1 : 0) | (first && first->has_mag ? 2 : 0);
#define AA_X3_LM(V)                                                                                              \
        if (lm == V)                                                                                             \
            return launch_x3<KH, KW, CIN, WM, WN, MF, NF, POOL, TH, TW, RING, AJIT, OCC, FUSED, IN_SPLIT, OUT_SPLIT, V>( \
                s, in, out, n, st, first);
        AA_X3_LM(1) AA_X3_LM(2) AA_X3_LM(3)
#undef AA_X3_LM
    }
    if constexpr (FUSED)
        AA_CHECK(s.d_f1, AA_ERR_INVALID, "conv %s: no first-layer lane image", s.name.c_str());
    auto k = conv_x3<KH, KW, CIN, WM, WN, MF, NF, POOL, TH, TW, FUSED, 0, RING, AJIT, OCC, IN_SPLIT, OUT_SPLIT, LM>;
    constexpr int BN = WN * NF * 16;
    const size_t lds = x3_lds_bytes<KH, KW, CIN, BN, TH, TW, FUSED, RING>();
    return launch_tuned(s, FUSED ? first : nullptr, n, (const void*)k, lds, true, POOL, TH, TW, BN,
                        [&](dim3 grid, int tiles_w, const FirstConv& fc) {
        hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, st, (const float*)in, s.Hin, s.Win, (const bf16*)s.d_w,
                           s.d_b, (float*)out, s.Hout, s.Wout, s.cout, tiles_w, s.act, s.alpha, fc);
    });
}

template <int KH, int CIN, int WM, int WN, int MF, int NF, int POOL, int TH, int TW, int OCC, int WO, int NPASS,
          int BD, int SLIDE, bool IN_SPLIT, bool OUT_SPLIT>
static int launch_wg(const Stage& s, const void* in, void* out, int n, hipStream_t st) {
    auto k = conv_wg<KH, CIN, WM, WN, MF, NF, POOL, TH, TW, OCC, IN_SPLIT, OUT_SPLIT, 0, WO, NPASS, BD, SLIDE>;
    constexpr int BN = WN * NF * 16;
    const size_t lds = wg_lds_bytes<KH, BN, TH, TW, WO, NPASS, WN>();
    return launch_tuned(s, nullptr, n, (const void*)k, lds, true, POOL, TH, TW, BN,
                        [&](dim3 grid, int tiles_w, const FirstConv&) {
        hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, st, (const float*)in, s.Hin, s.Win, (const bf16*)s.d_w,
                           s.d_b, (float*)out, s.Hout, s.Wout, s.cout, tiles_w, s.act, s.alpha);
    });
}

// Stages a and b (3x3 32 -> 64, 3x3 64 -> 64; aa_cnn_plan.h mark_pairs) in one
// launch: reads a's input, writes b's output
static int launch_pair(const Stage& a, const Stage& b, const void* in, void* out, int n, hipStream_t st) {
    AA_CHECK((double)a.Hin * a.Win * a.cin * 4 < 2147483647.0, AA_ERR_UNSUPPORTED,
             "conv %s: one window's activations exceed 2 GiB", a.name.c_str());
    constexpr size_t lds = pair_lds_bytes<PAIR_TH, PAIR_TW, true>();
    auto go = [&](auto is) {
        auto k = conv_x3_pair<PAIR_TH, PAIR_TW, 2, true, true, 3, true, decltype(is)::value>;
        return launch_tuned(b, nullptr, n, (const void*)k, lds, true, 1, PAIR_TH, PAIR_TW, 64,
                            [&](dim3 grid, int tiles_w, const FirstConv&) {
            hipLaunchKernelGGL(k, grid, dim3(256), lds, st, (const float*)in, a.Hin, a.Win, (const bf16*)a.d_w, a.d_b,
                               a.act, a.alpha, (const bf16*)b.d_w, b.d_b, (float*)out, b.Hout, b.Wout, b.cout, tiles_w,
                               b.act, b.alpha);
        });
    };
    return a.in_split ? go(std::true_type{}) : go(std::false_type{});
}

// A split-bf16 stage's runtime (fused_first, in_split, out_split) as template
// arguments: f(fused, in_split, out_split) with std::true_type / false_type.
// A fused first conv reads the f32 log-mel, never the split layout, and only
// a kernel shape that CAN_FUSE is instantiated with it.
template <bool CAN_FUSE, typename F>
static int dispatch_split(const Stage& s, F&& f) {
    using Y = std::true_type;
    using N = std::false_type;
    if constexpr (CAN_FUSE) {
        if (s.fused_first) return s.out_split ? f(Y{}, N{}, Y{}) : f(Y{}, N{}, N{});
    }
    if (s.in_split) return s.out_split ? f(N{}, Y{}, Y{}) : f(N{}, Y{}, N{});
    return s.out_split ? f(N{}, N{}, Y{}) : f(N{}, N{}, N{});
}

template <typename T>
static int launch_stage(const Model& m, const Stage& s, const void* in, void* out, float* logits,
                        float* probs, int n, hipStream_t st, const Stage* first, float* tmp) {
    using GT = typename Prec<T>::G;
    if (s.kind == ST_SMALL) {
        dim3 grid((s.Hc * s.Wc + 255) / 256, n);
        hipLaunchKernelGGL((conv_small<GT, 3, 3, 32>), grid, dim3(256), 0, st, (const float*)in, s.Hin,
                           s.Win, (const float*)s.d_w, s.d_b, s.has_mag, s.mag_exp, (GT*)out, s.Hc, s.Wc,
                           s.act, s.alpha);
        AA_LAUNCH_CHECK();
        return AA_OK;
    }
    if (s.kind == ST_GCONV) {
        if constexpr (!is_split<T>()) {
            set_error("%s: the runtime-shaped MFMA conv is split-bf16 only", s.name.c_str());
            return AA_ERR_UNSUPPORTED;
        } else {
            const ConvGeom g{s.Hin, s.Win, s.cin, s.Hc, s.Wc, s.cout, s.kh, s.kw, 1, 1, 0, 0, s.cin_pad};
            const bool pooled = s.ph > 1 || s.pw > 1;
            float* conv_out = pooled ? tmp : static_cast<float*>(out);
            const int gact_ = s.act == ACT_LEAKY ? GACT_LEAKY : s.act == ACT_RELU ? GACT_RELU : GACT_NONE;
            hipLaunchKernelGGL((gconv_x3t<2, 2, 2, 2>), dim3((s.Hc * s.Wc + 63) / 64, s.cout_pad / 64, n), dim3(256), 0, st,
                               (const float*)in, (const uint16_t*)s.d_w, s.d_b, conv_out, g, s.cout_pad, gact_,
                               s.alpha, nullptr, nullptr);
            AA_LAUNCH_CHECK();
            if (pooled) {  // max pool after the (monotonic) activation: the pool of the activated values
                const size_t items = (size_t)s.Hout * s.Wout * s.cout;
                hipLaunchKernelGGL(gpool2d, dim3((unsigned)((items + 255) / 256), n), dim3(256), 0, st, tmp,
                                   (float*)out, s.Hc, s.Wc, s.cout, s.Hout, s.Wout, s.ph, s.pw, s.ph, s.pw, 0, 0, 0,
                                   GACT_NONE, 0.f);
                AA_LAUNCH_CHECK();
            }
            return AA_OK;
        }
    }
    if (s.kind == ST_GENERIC) {
        if constexpr (is_fp8<T>()) {
            set_error("%s: no fp8 kernel for this shape", s.name.c_str());
            return AA_ERR_UNSUPPORTED;
        } else {
            dim3 grid((s.Hout * s.Wout + 255) / 256, (s.cout + 7) / 8, n);
            if (s.is_first) {  // reads the f32 model input (log-mel)
                hipLaunchKernelGGL((conv_generic<float, GT>), grid, dim3(256), 0, st, (const float*)in, s.Hin,
                                   s.Win, s.cin, (const float*)s.d_w, s.d_b, s.kh, s.kw, s.cout, s.ph, s.pw, s.Hout,
                                   s.Wout, s.act, s.alpha, s.has_mag, s.mag_exp, (GT*)out);
            } else {
                hipLaunchKernelGGL((conv_generic<GT, GT>), grid, dim3(256), 0, st, (const GT*)in, s.Hin, s.Win,
                                   s.cin, (const float*)s.d_w, s.d_b, s.kh, s.kw, s.cout, s.ph, s.pw, s.Hout,
                                   s.Wout, s.act, s.alpha, 0, 1.f, (GT*)out);
            }
            AA_LAUNCH_CHECK();
            return AA_OK;
        }
    }
    if (s.kind == ST_POOLDENSE) {
        hipLaunchKernelGGL((pool_dense<GT>), dim3(n), dim3(256), (size_t)s.cin * sizeof(float), st, (const GT*)in,
                           s.Hin * s.Win, s.cin, (const float*)s.d_w, s.d_b, s.cout, s.sigmoid, logits, probs);
        AA_LAUNCH_CHECK();
        return AA_OK;
    }
    if (s.kind == ST_HEAD && s.tail) {
        if constexpr (is_split<T>()) {
            // the last conv stage and the head in one launch (aa_conv_tail.h):
            // per-tile label maxima into `out`, then head_final over the tiles
            const Stage& c = *first;
            const int tiles_h = (c.Hc + TAIL_TH - 1) / TAIL_TH, tiles_w = (c.Wc + TAIL_TW - 1) / TAIL_TW;
            auto k = conv_tail_x3<1, 3, 128, AA_TAIL_MF, TAIL_TH, TAIL_TW>;
            constexpr size_t lds = tail_lds_bytes<1, 3, 128, TAIL_TH, TAIL_TW>();
            AA_DYN_LDS(k, lds);
            float* part = static_cast<float*>(out);
            hipLaunchKernelGGL(k, dim3(tiles_h * tiles_w, 1, n), dim3(TAIL_NW * 64), lds, st, (const float*)in, c.Hin,
                               c.Win, (const bf16*)c.d_w, c.d_b, c.Hc, c.Wc, tiles_w, c.act, c.alpha,
                               (const bf16*)s.d_tw, part);
            AA_LAUNCH_CHECK();
            hipLaunchKernelGGL(head_final, dim3(n), dim3(64), 0, st, part, tiles_h * tiles_w, 32, s.d_b, s.cout, s.act,
                               s.alpha, s.sigmoid, logits, probs, (const float*)nullptr);
            AA_LAUNCH_CHECK();
            return AA_OK;
        } else {
            set_error("%s: the fused tail is split-bf16 only", s.name.c_str());
            return AA_ERR_UNSUPPORTED;
        }
    }
    if (s.kind == ST_HEAD) {
        // pixel ranges of 64 spread over blocks (a window alone is too little
        // work for one block's dependent load chain), 32 labels per block;
        // their column maxima go to the free ping-pong buffer `out` and
        // head_final reduces them
        const int HW = s.Hin * s.Win, parts = (HW + 63) / 64;
        float* part = static_cast<float*>(out);
        const float* hsc = is_fp8<T>() ? s.d_b + s.cout_pad : nullptr;  // fp8 dequantisation scales
        // split-bf16: the head reads f32 activations and runs the exact f32
        // MFMA (its 1x1 contraction is <1 % of the network's FLOPs)
        hipLaunchKernelGGL((conv_head<GT, 1, 2>), dim3(n, parts, s.cout_pad / 32), dim3(256), 0, st, (const GT*)in,
                           HW, s.cin, (const GT*)s.d_w, s.d_b, s.cout, s.act, s.alpha, s.sigmoid, logits, probs, part,
                           hsc);
        AA_LAUNCH_CHECK();
        hipLaunchKernelGGL(head_final, dim3(n), dim3(s.cout <= 64 ? 64 : 256), 0, st, part, parts, s.cout_pad, s.d_b,
                           s.cout, s.act, s.alpha, s.sigmoid, logits, probs, hsc);
        AA_LAUNCH_CHECK();
        return AA_OK;
    }
    if (s.fused_first) {
        AA_CHECK(s.kh == 3 && s.kw == 3 && s.cin == 32 && s.pool == 3, AA_ERR_UNSUPPORTED,
                 "no fused first-layer kernel for %s", s.name.c_str());
    }
    if constexpr (is_split<T>()) {
        if (s.wg) {
#define AA_LAUNCHW(KH, CIN, POOL, WM, WN, MF, NF, TH, TW, OCC, WO, NPASS, BD, SLIDE)                             \
            if (s.kh == KH && s.cin == CIN && s.pool == POOL)                                                    \
                return dispatch_split<false>(s, [&](auto, auto is, auto os) {                                    \
                    return launch_wg<KH, CIN, WM, WN, MF, NF, POOL, TH, TW, OCC, WO, NPASS, BD, SLIDE,           \
                                     decltype(is)::value, decltype(os)::value>(s, in, out, n, st);               \
                });
            AA_WG_CFGS(AA_LAUNCHW)
#undef AA_LAUNCHW
            set_error("conv %dx%d cin %d pool %d: no Winograd kernel instantiation", s.kh, s.kw, s.cin, s.pool);
            return AA_ERR_UNSUPPORTED;
        }
        // (only the 3x3/32 rows have a fused-first form: launch_stage checked the shape above)
#define AA_LAUNCH3(KH, KW, CIN, POOL, WM, WN, MF, NF, TH, TW, RING, AJIT, OCC)                                   \
        if (s.kh == KH && s.kw == KW && s.cin == CIN && s.pool == POOL)                                          \
            return dispatch_split<CIN == 32 && KH == 3 && KW == 3>(s, [&](auto fu, auto is, auto os) {           \
                return launch_x3<KH, KW, CIN, WM, WN, MF, NF, POOL, TH, TW, RING, AJIT, OCC, decltype(fu)::value, \
                                 decltype(is)::value, decltype(os)::value>(s, in, out, n, st, first);            \
            });
        AA_X3_CFGS(AA_LAUNCH3)
#undef AA_LAUNCH3
        set_error("conv %dx%d cin %d pool %d: no split-bf16 kernel instantiation", s.kh, s.kw, s.cin, s.pool);
        return AA_ERR_UNSUPPORTED;
    }
#define AA_LAUNCH(T_, KH, KW, CIN, POOL, WM, WN, MF, NF, TH, TW, EB, OCC)                                        \
    if constexpr (std::is_same<T, T_>::value) {                                                          \
        if (s.kh == KH && s.kw == KW && s.cin == CIN && s.pool == POOL) {                                \
            if (s.fused_first) {                                                                         \
                if constexpr (CIN == 32 && KH == 3 && KW == 3)                                           \
                    return launch_mfma<T, KH, KW, CIN, WM, WN, MF, NF, POOL, TH, TW, true, EB, OCC>(s, in, out, \
                                                                                              n, st, first); \
            } else {                                                                                     \
                return launch_mfma<T, KH, KW, CIN, WM, WN, MF, NF, POOL, TH, TW, false, EB, OCC>(s, in, out, n, st); \
            }                                                                                            \
        }                                                                                                \
    }
    AA_CONV_CFGS(AA_LAUNCH)
#undef AA_LAUNCH
    set_error("conv %dx%d cin %d pool %d: no kernel instantiation", s.kh, s.kw, s.cin, s.pool);
    return AA_ERR_UNSUPPORTED;
}

static void free_model(Model* m) {
    if (!m) return;
    m->timer.release();
    if (m->uploaded)
        for (auto& s : m->st) {
            (void)hipFree(s.d_w);
            (void)hipFree(s.d_b);
            (void)hipFree(s.d_tw);
            (void)hipFree(s.d_f1);
        }
    delete m;
}

// Copies every stage's host images to the device and releases them.
static int upload_model(Model* m) {
    m->uploaded = true;  // from here on the stages may own device memory
    auto put = [](void** d, const void* h, size_t bytes) {
        hipError_t e = hipMalloc(d, bytes ? bytes : 4);
        if (e == hipSuccess && bytes) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
        return e;
    };
    for (Stage& s : m->st) {
        hipError_t e = s.h_w.empty() ? hipSuccess : put(&s.d_w, s.h_w.data(), s.h_w.size());
        if (e == hipSuccess) e = put((void**)&s.d_b, s.h_b.data(), sizeof(float) * s.h_b.size());
        AA_CHECK(e == hipSuccess, AA_ERR_HIP, "aa_model_create: layer %d: %s", s.layer_end, hipGetErrorString(e));
        if (!s.h_tw.empty()) e = put(&s.d_tw, s.h_tw.data(), s.h_tw.size());
        if (e == hipSuccess && !s.h_f1.empty()) e = put(&s.d_f1, s.h_f1.data(), s.h_f1.size());
        AA_CHECK(e == hipSuccess, AA_ERR_HIP, "aa_model_create: %s", hipGetErrorString(e));
        std::vector<uint8_t>().swap(s.h_w);
        std::vector<uint8_t>().swap(s.h_tw);
        std::vector<uint8_t>().swap(s.h_f1);
        std::vector<float>().swap(s.h_b);
    }
    return AA_OK;
}

// Stages 0 .. last_stage on n <= 32768 windows: the workspace carved into the
// two ping-pong buffers and the ST_GCONV scratch, one launch_stage per stored
// stage.  *last_out (optional): where stage last_stage wrote.
template <typename T>
static int run_stages_t(Model* m, const void* x, int n, int last_stage, float* logits, float* probs, void* workspace,
                        hipStream_t st, bool timed, const void** last_out) {
    const size_t es = prec_bytes(m->prec);
    char* buf[2] = {static_cast<char*>(workspace),
                    static_cast<char*>(workspace) + align_up(m->act_elems[0] * es * n, 256)};
    float* tmp = reinterpret_cast<float*>(buf[1] + align_up(m->act_elems[1] * es * n, 256));
    const void* in = x;
    int flip = 0;  // after a pair the later stages write the buffer of the other parity (mark_pairs)
    for (int k = 0; k <= last_stage; ++k) {
        const Stage& s = m->st[k];
        if (s.skipped) continue;  // computed inside stage k + 1 (reads x directly)
        if (k + 1 <= last_stage && m->st[k + 1].pair) continue;  // computed inside stage k + 1 (conv_x3_pair)
        // (a fused tail writes its per-tile maxima into the skipped conv stage's
        // buffer: its own would be the one its input lives in; so does a pair,
        // whose own buffer holds the previous stage's input)
        void* out = buf[((s.tail || s.pair ? k - 1 : k) % 2) ^ flip];
        const Stage* first = (s.fused_first || s.tail) ? &m->st[k - 1] : nullptr;
        hipEvent_t e0 = nullptr;
        int rc = timed ? m->timer.begin(k, st, &e0) : AA_OK;
        if (rc != AA_OK) return rc;
        if (s.pair) {
            if constexpr (is_split<T>()) {
                rc = launch_pair(m->st[k - 1], s, in, out, n, st);
                flip ^= 1;
            } else {
                set_error("%s: the fused conv pair is split-bf16 only", s.name.c_str());
                rc = AA_ERR_UNSUPPORTED;
            }
        } else {
            rc = launch_stage<T>(*m, s, in, out, logits, probs, n, st, first, tmp);
        }
        if (rc != AA_OK) return rc;
        rc = m->timer.end(k, st, e0);
        if (rc != AA_OK) return rc;
        in = out;
    }
    if (last_out) *last_out = in;
    return AA_OK;
}

static int run_stages(Model* m, const void* x, int n, int last_stage, float* logits, float* probs, void* workspace,
                      hipStream_t st, bool timed, const void** last_out = nullptr) {
    switch (m->prec) {
        case AA_PREC_BF16: return run_stages_t<bf16>(m, x, n, last_stage, logits, probs, workspace, st, timed, last_out);
        case AA_PREC_FP8: return run_stages_t<fp8>(m, x, n, last_stage, logits, probs, workspace, st, timed, last_out);
        case AA_PREC_BF16X3: return run_stages_t<bf16x3>(m, x, n, last_stage, logits, probs, workspace, st, timed, last_out);
        default: return run_stages_t<float>(m, x, n, last_stage, logits, probs, workspace, st, timed, last_out);
    }
}

}  // namespace aa

using namespace aa;

extern "C" int aa_model_plan(const aa_layer* layers, int32_t n_layers, const float* blob, int64_t blob_len,
                             int32_t in_h, int32_t in_w, int32_t in_c, int32_t precision, void** model) {
    AA_CHECK(model, AA_ERR_INVALID, "aa_model_create: null argument");
    Model* m = nullptr;
    const int rc = plan_model(layers, n_layers, blob, blob_len, in_h, in_w, in_c, precision, &m);
    if (rc == AA_OK) *model = m;
    return rc;
}

extern "C" int aa_model_create(const aa_layer* layers, int32_t n_layers, const float* blob, int64_t blob_len,
                               int32_t in_h, int32_t in_w, int32_t in_c, int32_t precision, void** model) {
    void* m = nullptr;
    int rc = aa_model_plan(layers, n_layers, blob, blob_len, in_h, in_w, in_c, precision, model ? &m : nullptr);
    if (rc != AA_OK) return rc;
    rc = upload_model(static_cast<Model*>(m));
    if (rc != AA_OK) {
        free_model(static_cast<Model*>(m));
        return rc;
    }
    *model = m;
    return AA_OK;
}

extern "C" int aa_model_first_lane_image(const void* model, void* buf, size_t cap, size_t* len) {
    const Model* m = static_cast<const Model*>(model);
    AA_CHECK(m && len, AA_ERR_INVALID, "aa_model_first_lane_image: bad argument");
    AA_CHECK(!m->uploaded, AA_ERR_UNSUPPORTED,
             "aa_model_first_lane_image: the host images are released once a model is created; plan it (aa_model_plan)");
    static const std::vector<uint8_t> none;
    const std::vector<uint8_t>& img = m->st.size() >= 2 ? m->st[1].h_f1 : none;
    *len = img.size();
    if (!buf) return AA_OK;  // a size query
    AA_CHECK(cap >= *len, AA_ERR_INVALID, "aa_model_first_lane_image: buffer %zu < %zu", cap, *len);
    if (*len) memcpy(buf, img.data(), *len);
    return AA_OK;
}

extern "C" int aa_model_stage_image(const void* model, int32_t stage, int32_t which, void* buf, size_t cap,
                                    size_t* len) {
    const Model* m = static_cast<const Model*>(model);
    AA_CHECK(m && len && stage >= 0 && stage < (int)m->st.size() && which >= 0 && which <= 2, AA_ERR_INVALID,
             "aa_model_stage_image: bad argument");
    AA_CHECK(!m->uploaded, AA_ERR_UNSUPPORTED,
             "aa_model_stage_image: the host images are released once a model is created; plan it (aa_model_plan)");
    const Stage& s = m->st[stage];
    const void* src = which == 0 ? (const void*)s.h_w.data() : which == 1 ? (const void*)s.h_b.data() : s.h_tw.data();
    *len = which == 0 ? s.h_w.size() : which == 1 ? s.h_b.size() * sizeof(float) : s.h_tw.size();
    if (!buf) return AA_OK;  // a size query
    AA_CHECK(cap >= *len, AA_ERR_INVALID, "aa_model_stage_image: buffer %zu < %zu", cap, *len);
    if (*len) memcpy(buf, src, *len);
    return AA_OK;
}

extern "C" int aa_model_destroy(void* model) {
    free_model(static_cast<Model*>(model));
    return AA_OK;
}

extern "C" int aa_model_n_outputs(const void* model) {
    return model ? static_cast<const Model*>(model)->L : -1;
}

extern "C" size_t aa_model_workspace_bytes(const void* model, int32_t max_batch) {
    if (!model || max_batch < 0) return 0;
    const Model* m = static_cast<const Model*>(model);
    const size_t es = prec_bytes(m->prec);
    return align_up(m->act_elems[0] * es * max_batch, 256) + align_up(m->act_elems[1] * es * max_batch, 256) +
           align_up(m->tmp_elems * 4 * max_batch, 256);
}

extern "C" int aa_model_set_input_f16(void* model, int32_t f16) {
    Model* m = static_cast<Model*>(model);
    AA_CHECK(m && (f16 == 0 || f16 == 1), AA_ERR_INVALID, "aa_model_set_input_f16: bad argument");
    AA_CHECK(m->uploaded, AA_ERR_INVALID, "aa_model_set_input_f16: the model is a plan (aa_model_plan), not created");
    AA_CHECK(!f16 || (m->st.size() >= 2 && m->st[1].fused_first), AA_ERR_UNSUPPORTED,
             "aa_model_set_input_f16: float16 input needs the fused first conv (3x3 C_in=1 -> 32 before a "
             "pooled 3x3/32 conv)");
    if (m->st.size() >= 2) m->st[1].lm_f16 = f16;
    return AA_OK;
}

extern "C" int aa_model_forward(void* model, const void* x, int32_t n, float* logits, float* probs,
                                void* workspace, size_t workspace_bytes, void* stream) {
    Model* m = static_cast<Model*>(model);
    AA_CHECK(m && x && logits, AA_ERR_INVALID, "aa_model_forward: null argument");
    AA_CHECK(m->uploaded, AA_ERR_INVALID, "aa_model_forward: the model is a plan (aa_model_plan), not created");
    if (n <= 0) return AA_OK;
    const size_t need = aa_model_workspace_bytes(m, n);
    AA_CHECK(workspace && workspace_bytes >= need, AA_ERR_WORKSPACE, "aa_model_forward: workspace %zu < %zu",
             workspace_bytes, need);
    // launch grids carry the window index in blockIdx.z (at most 65,535):
    // larger batches run as consecutive chunks through the same workspace
    constexpr int32_t CHUNK = 32768;
    if (n > CHUNK) {
        const size_t in_bytes = (size_t)m->in_h * m->in_w * m->in_c *
                                (m->st.size() >= 2 && m->st[1].lm_f16 ? 2 : 4);
        for (int32_t c0 = 0; c0 < n; c0 += CHUNK) {
            const int32_t nc = std::min(CHUNK, n - c0);
            const int rc = aa_model_forward(model, static_cast<const char*>(x) + (size_t)c0 * in_bytes, nc,
                                            logits + (size_t)c0 * m->L, probs ? probs + (size_t)c0 * m->L : nullptr,
                                            workspace, workspace_bytes, stream);
            if (rc != AA_OK) return rc;
        }
        return AA_OK;
    }
    return run_stages(m, x, n, (int)m->st.size() - 1, logits, probs, workspace, static_cast<hipStream_t>(stream), true);
}

extern "C" int aa_model_n_stages(const void* model) {
    return model ? (int)static_cast<const Model*>(model)->st.size() : -1;
}

extern "C" int aa_model_stage_info(const void* model, int32_t stage, char* name, int32_t name_len,
                                   double* flops_per_item, double* bytes_per_item) {
    const Model* m = static_cast<const Model*>(model);
    AA_CHECK(m && stage >= 0 && stage < (int)m->st.size(), AA_ERR_INVALID, "aa_model_stage_info: bad stage");
    const Stage& s = m->st[stage];
    if (name && name_len > 0) snprintf(name, name_len, "%s", s.name.c_str());
    if (flops_per_item) *flops_per_item = s.flops;
    if (bytes_per_item) *bytes_per_item = s.bytes;
    return AA_OK;
}

extern "C" int aa_model_set_timing(void* model, uint32_t stage_mask) {
    Model* m = static_cast<Model*>(model);
    AA_CHECK(m, AA_ERR_INVALID, "aa_model_set_timing: null model");
    m->timer.mask = stage_mask;
    return AA_OK;
}

extern "C" int aa_model_stage_time(void* model, int32_t stage, double* total_ms, int64_t* count) {
    Model* m = static_cast<Model*>(model);
    AA_CHECK(m && stage >= 0 && stage < (int)m->st.size(), AA_ERR_INVALID, "aa_model_stage_time: bad stage");
    return m->timer.collect(stage, total_ms, count);
}

extern "C" int aa_model_stage_shape(const void* model, int32_t stage, int32_t* h, int32_t* w, int32_t* c) {
    const Model* m = static_cast<const Model*>(model);
    AA_CHECK(m && stage >= 0 && stage < (int)m->st.size(), AA_ERR_INVALID, "aa_model_stage_shape: bad stage");
    const Stage& s = m->st[stage];
    // stages whose output never reaches memory as activations: a first conv
    // computed inside the next stage, the conv inside the fused tail, the logits
    AA_CHECK(!s.skipped, AA_ERR_UNSUPPORTED, "aa_model_stage_shape: stage %d (%s) is computed inside stage %d and never stored",
             stage, s.name.c_str(), stage + 1);
    AA_CHECK(s.kind != ST_POOLDENSE && s.kind != ST_HEAD, AA_ERR_UNSUPPORTED,
             "aa_model_stage_shape: stage %d (%s) writes the logits, not activations", stage, s.name.c_str());
    if (h) *h = s.Hout;
    if (w) *w = s.Wout;
    if (c) *c = s.cout;
    return AA_OK;
}

extern "C" int aa_model_forward_prefix(void* model, const void* x, int32_t n, int32_t stage, float* act,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    Model* m = static_cast<Model*>(model);
    AA_CHECK(m && x && act, AA_ERR_INVALID, "aa_model_forward_prefix: null argument");
    AA_CHECK(m->uploaded, AA_ERR_INVALID, "aa_model_forward_prefix: the model is a plan (aa_model_plan), not created");
    int32_t sh, sw, sc;
    const int src = aa_model_stage_shape(model, stage, &sh, &sw, &sc);
    if (src != AA_OK) return src;
    AA_CHECK(n >= 0 && n <= 32768, AA_ERR_INVALID, "aa_model_forward_prefix: n %d outside 0..32768", n);
    if (n == 0) return AA_OK;
    const size_t need = aa_model_workspace_bytes(m, n);
    AA_CHECK(workspace && workspace_bytes >= need, AA_ERR_WORKSPACE, "aa_model_forward_prefix: workspace %zu < %zu",
             workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const void* in = nullptr;
    const int rc = run_stages(m, x, n, stage, nullptr, nullptr, workspace, st, false, &in);
    if (rc != AA_OK) return rc;
    const size_t total = (size_t)n * sh * sw * sc;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    // ST_SMALL / ST_GENERIC / ST_GCONV store the mode's plain activation type;
    // only a conv_x3 / conv_wg stage with out_split writes the grouped split
    if (m->st[stage].out_split)
        hipLaunchKernelGGL(stage_decode<3>, dim3(blocks), dim3(256), 0, st, in, act, total, sc);
    else if (m->prec == AA_PREC_BF16)
        hipLaunchKernelGGL(stage_decode<1>, dim3(blocks), dim3(256), 0, st, in, act, total, sc);
    else if (m->prec == AA_PREC_FP8)
        hipLaunchKernelGGL(stage_decode<2>, dim3(blocks), dim3(256), 0, st, in, act, total, sc);
    else
        hipLaunchKernelGGL(stage_decode<0>, dim3(blocks), dim3(256), 0, st, in, act, total, sc);
    AA_LAUNCH_CHECK();
    return AA_OK;
}

extern "C" int aa_track_mean(const float* probs, int32_t n_models, int64_t model_stride, int32_t n_labels,
                             const int32_t* win_begin, const int32_t* win_count, int32_t n_tracks, float* out,
                             void* stream) {
    AA_CHECK(probs && win_begin && win_count && out, AA_ERR_INVALID, "aa_track_mean: null argument");
    AA_CHECK(n_models >= 1 && n_labels >= 1 && n_labels <= 1024, AA_ERR_INVALID, "aa_track_mean: bad sizes");
    if (n_tracks <= 0) return AA_OK;
    const int threads = (n_labels + 63) / 64 * 64;
    hipLaunchKernelGGL(track_mean, dim3(n_tracks), dim3(threads), 0, static_cast<hipStream_t>(stream), probs,
                       n_models, (long long)model_stride, n_labels, win_begin, win_count, out);
    AA_LAUNCH_CHECK();
    return AA_OK;
}
