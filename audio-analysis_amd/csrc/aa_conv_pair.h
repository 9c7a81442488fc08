// Two stacked 3x3 split-bf16 convs in one launch (AA_PREC_BF16X3): layer A
// (C_in 32 -> 64, bias + activation, grouped-split output) and layer B (64 ->
// 64, bias + activation, f32 NHWC output) without the round trip of layer A's
// activations through global memory.  Included by aa_cnn.hip after
// aa_conv_x3.h (shares its swizzle, weight packing, x3_stage_split, x3_read_b,
// x3_step_jit, x3_mfma3 and x3_store).
//
// One block of 4 waves (WM 2 x WN 2, NF 2: a wave owns 32 output channels of
// both layers) per (window, TH x TW tile of layer B's output):
//
//  * the (TH + 4) x (TW + 4) x 32-channel input patch is staged from the
//    grouped-split layout by global_load_lds (IN_SPLIT) or split from f32 as
//    conv_x3 does, swizzled for layer A's reads (rows of TW + 2 intermediate
//    pixels);
//  * layer A runs its 9 steps for all (TH + 2) x (TW + 2) intermediate pixels
//    the tile needs -- the tile's halo is recomputed, 140 instead of 96 pixels
//    for 12 x 8 -- as MFA pixel fragments per wave;
//  * bias, activation and the hi / lo split are applied to the accumulators
//    with the functions x3_store uses (apply_act, split2), and the result is
//    written into two swizzled 32-channel group images in LDS: what
//    x3_stage_split would have staged from layer A's stored output.
//    Intermediate pixels past layer A's output come from clamped (finite)
//    input pixels and only feed outputs the store discards;
//  * after a barrier layer B runs its 18 steps from those images, then its
//    f32 tile goes through LDS to x3_store.
//
// LDS: the group images (35 KiB for 12 x 8) either lie beside the input patch
// and the f32 tile, which share 24 KiB (59 KiB: two blocks per CU, three
// barriers), or share their LDS too (ALIAS: 35 KiB, four blocks per CU by LDS,
// a barrier more before the images are written and one before the f32 tile
// is).  Measured (tools/conv_bench_x3.hip mode 40, profiles/r10/conv_pair.txt)
// the aliased form at three waves per SIMD wins.
//
// Weights: every wave loads its own B fragments from the packed weights in
// global memory (L2-resident) BD - 1 steps ahead; a 3-slice LDS ring beside
// the unaliased images would put the block past 80 KiB.  No inter-block
// synchronisation.
//
// Every accumulator sums (group, tap) ascending through x3_mfma3 over the
// same fragments as conv_x3, so the output equals that of the two conv_x3
// launches word for word.
#pragma once

namespace aa {

// the tile of layer B's output a block computes (the 3x3/64 row of AA_X3_CFGS)
constexpr int PAIR_TH = 12, PAIR_TW = 8;

// ALIAS: the group images share the input patch's (and the f32 tile's) LDS,
// at the price of a barrier before they are written and one before the f32
// tile is: 35 KiB instead of 59 KiB for 12 x 8, four blocks per CU instead of two
template <int TH, int TW, bool ALIAS>
__host__ __device__ constexpr size_t pair_lds_bytes() {
    const size_t patch = (size_t)(TH + 4) * (TW + 4) * 128;
    const size_t epi = (size_t)TH * TW * 64 * 4;
    const size_t mid = (size_t)2 * (TH + 2) * (TW + 2) * 128;
    const size_t pe = patch > epi ? patch : epi;
    return ALIAS ? (pe > mid ? pe : mid) : pe + mid;
}

// NSTEP steps of one layer: step s reads tap s % 9 of group image s / 9.
// Bq holds the B sets of steps 0 .. BD - 2 on entry.  AJIT: A fragments just
// in time (x3_step_jit) or the whole next step's set read one step ahead.
template <int MF, int NSTEP, int PW, int TW, int GIMG, int BD, bool AJIT, bool PIN>
__device__ __forceinline__ void pair_steps(f32x4 (&acc)[MF][2], const char* img, const int (&abase)[MF],
                                           const int (&aph)[MF], __amdgpu_buffer_rsrc_t wrs, const int (&bofs)[2],
                                           X3BSet<2> (&Bq)[BD]) {
    constexpr int SLICE_B = 64 * 128;  // bytes of one step's weights
    auto addr = [&](int i, int s) {
        const int g = s / 9, t = s - g * 9;
        const int kh = t / 3, kw = t - kh * 3;
        return abase[i] + g * GIMG + (kh * PW + kw) * 128 + (((aph[i] + kh * TW + kw) & 7) << 4);
    };
    bf16x8 ah[2][AJIT ? 1 : MF], al[2][AJIT ? 1 : MF];
    if constexpr (!AJIT) {
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int a = addr(i, 0);
            ah[0][i] = *reinterpret_cast<const bf16x8*>(img + a);
            al[0][i] = *reinterpret_cast<const bf16x8*>(img + (a ^ 64));
        }
    }
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
        if (s + BD - 1 < NSTEP)
            x3_read_b(Bq[(s + BD - 1) % BD], wrs, bofs, __builtin_amdgcn_readfirstlane((s + BD - 1) * SLICE_B));
        if constexpr (AJIT) {
            x3_step_jit<MF, 2, PIN>(acc, Bq[s % BD], [&](int i, int k) {
                return *reinterpret_cast<const bf16x8*>(img + (addr(i, s) ^ (64 * k)));
            });
        } else {
            if (s + 1 < NSTEP) {
#pragma unroll
                for (int i = 0; i < MF; ++i) {
                    const int a = addr(i, s + 1);
                    ah[(s + 1) & 1][i] = *reinterpret_cast<const bf16x8*>(img + a);
                    al[(s + 1) & 1][i] = *reinterpret_cast<const bf16x8*>(img + (a ^ 64));
                }
            }
            if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    x3_mfma3(acc[i][j], Bq[s % BD].h[j], Bq[s % BD].l[j], ah[s & 1][i], al[s & 1][i]);
        }
    }
}

template <int TH, int TW, int BD = 2, bool AJIT = true, bool PIN = true, int OCC = 0, bool ALIAS = false,
          bool IN_SPLIT = true>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OCC ? OCC : 1, OCC ? OCC : (ALIAS ? 4 : 2))))
void conv_x3_pair(const float* __restrict__ in, int Hin, int Win, const bf16* __restrict__ wtA,
                  const float* __restrict__ biasA, int actA, float alphaA, const bf16* __restrict__ wtB,
                  const float* __restrict__ biasB, float* __restrict__ out, int Hout, int Wout, int cout_store,
                  int tiles_w, int actB, float alphaB) {
    constexpr int WM = 2, NW = 4, NTHR = 256, BN = 64;
    constexpr int IH = TH + 2, IW = TW + 2, IP = IH * IW;  // intermediate (layer A output) pixels
    constexpr int PH = TH + 4, PW = TW + 4;                // input patch
    constexpr int TP = TH * TW;
    constexpr int MFA = ((IP + 15) / 16 + WM - 1) / WM, MFB = ((TP + 15) / 16 + WM - 1) / WM;
    constexpr int GIMG = IP * 128;  // bytes of one intermediate group image
    constexpr size_t PATCH = ALIAS ? 0 : pair_lds_bytes<TH, TW, false>() - 2 * GIMG;
    static_assert(BD >= 2, "a B set in use and one in flight");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;
    char* mid = smem + PATCH;

    const BlockPos bp = x3_block();
    const int n = bp.n;
    const int th = bp.tile / tiles_w, tw = bp.tile - (bp.tile / tiles_w) * tiles_w;
    const int oh0 = th * TH, ow0 = tw * TW;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, q = lane >> 4;
    const int wm = wave % WM, wn = wave / WM;

    // ---- the input patch, swizzled by layer A's row width IW ----
    if constexpr (IN_SPLIT) {
        x3_stage_split<1, 32, PH, PW, IW, NW>(patch, in, n, Hin, Win, oh0, ow0, 0, wave, lane);
    } else {
        // f32 NHWC input: (pixel, channel quad) items split as conv_x3 splits them
        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
        const float* src = in + (size_t)n * Hin * Win * 32;
#pragma unroll 2
        for (int idx = threadIdx.x; idx < PH * PW * 8; idx += NTHR) {
            const int pix = idx >> 3, cq = idx & 7;
            const int R = pix / PW, C = pix - R * PW;
            const int gh = min(oh0 + R, Hin - 1), gw = min(ow0 + C, Win - 1);
            const float4 x = *reinterpret_cast<const float4*>(src + ((size_t)gh * Win + gw) * 32 + cq * 4);
            bf16x4 h, l;
            h[0] = bf_hi(x.x); l[0] = bf_lo(x.x);
            h[1] = bf_hi(x.y); l[1] = bf_lo(x.y);
            h[2] = bf_hi(x.z); l[2] = bf_lo(x.z);
            h[3] = bf_hi(x.w); l[3] = bf_lo(x.w);
            const int a = x3_addr(R, C, cq >> 1, PW, IW) + (cq & 1) * 8;
            *reinterpret_cast<bf16x4*>(patch + a) = h;
            *reinterpret_cast<bf16x4*>(patch + (a ^ 64)) = l;
        }
    }

    int bofs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bofs[j] = x3_bofs(wn * 32 + j * 16 + (lane & 15), q);
    const __amdgpu_buffer_rsrc_t wrsA = x3_wrsrc(wtA), wrsB = x3_wrsrc(wtB);
    X3BSet<2> Bq[BD];
#pragma unroll
    for (int s = 0; s < BD - 1; ++s) x3_read_b(Bq[s], wrsA, bofs, s * (64 * 128));
    // layer A's bias quads of this lane's channels (32 wn + 16 j + 4 q + e)
    float4 bvA[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bvA[j] = *reinterpret_cast<const float4*>(biasA + wn * 32 + j * 16 + q * 4);

    // ---- layer A: intermediate pixel fragments wm * MFA + i ----
    {
        int abase[MFA], aph[MFA];
#pragma unroll
        for (int i = 0; i < MFA; ++i) {
            const int p = x3_frag_pixel((wm * MFA + i) * 16 + (lane & 15), IP);
            const int r = p / IW, c = p - (p / IW) * IW;
            abase[i] = (r * PW + c) * 128;
            aph[i] = p + q;
        }
        f32x4 acc[MFA][2];
#pragma unroll
        for (int i = 0; i < MFA; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's patch pieces (and the first B sets) landed
        __syncthreads();
        pair_steps<MFA, 9, PW, IW, 0, BD, AJIT, PIN>(acc, patch, abase, aph, wrsA, bofs, Bq);

        // layer B's first B sets: their latency hides behind the epilogue below
#pragma unroll
        for (int s = 0; s < BD - 1; ++s) x3_read_b(Bq[s], wrsB, bofs, s * (64 * 128));

        if constexpr (ALIAS) __syncthreads();  // every wave is done with the input patch
        // bias, activation, split; the lane's 4 channels of fragment j are half
        // (q & 1) of unit 2 j + (q >> 1) of group wn's image, swizzled by layer
        // B's row width TW
#pragma unroll
        for (int i = 0; i < MFA; ++i) {
            const int p = (wm * MFA + i) * 16 + (lane & 15);
            if (p < IP) {
                const int r = p / IW, c = p - (p / IW) * IW;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    uint32_t h0, l0, h1, l1;
                    split2(apply_act(acc[i][j][0] + bvA[j].x, actA, alphaA),
                           apply_act(acc[i][j][1] + bvA[j].y, actA, alphaA), h0, l0);
                    split2(apply_act(acc[i][j][2] + bvA[j].z, actA, alphaA),
                           apply_act(acc[i][j][3] + bvA[j].w, actA, alphaA), h1, l1);
                    const int a = wn * GIMG + x3_addr(r, c, 2 * j + (q >> 1), IW, TW) + (q & 1) * 8;
                    *reinterpret_cast<uint2*>(mid + a) = make_uint2(h0, h1);
                    *reinterpret_cast<uint2*>(mid + (a ^ 64)) = make_uint2(l0, l1);
                }
            }
        }
    }
    __syncthreads();  // the group images are complete; the input patch is free

    // ---- layer B: tile pixel fragments wm * MFB + i ----
    int abase[MFB], aph[MFB];
#pragma unroll
    for (int i = 0; i < MFB; ++i) {
        const int p = x3_frag_pixel((wm * MFB + i) * 16 + (lane & 15), TP);
        const int r = p / TW, c = p - (p / TW) * TW;
        abase[i] = (r * IW + c) * 128;
        aph[i] = p + q;
    }
    f32x4 acc[MFB][2];
#pragma unroll
    for (int i = 0; i < MFB; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    pair_steps<MFB, 18, IW, TW, GIMG, BD, AJIT, PIN>(acc, mid, abase, aph, wrsB, bofs, Bq);

    // ---- epilogue: f32 tile (x3_store's swizzled layout) over the input patch ----
    if constexpr (ALIAS) __syncthreads();  // every wave is done with the group images
    float* E = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int u = wn * 8 + j * 4 + q;
#pragma unroll
        for (int i = 0; i < MFB; ++i) {
            const int p = (wm * MFB + i) * 16 + (lane & 15);
            if (p < TP)
                *reinterpret_cast<float4*>(E + x3_eoff<BN, 0>(p, u)) =
                    make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
    }
    __syncthreads();
    x3_store<TH, TW, 1, BN, NTHR, false, false, 0>(E, biasB, out, n, 0, oh0, ow0, Hout, Wout, cout_store, actB, alphaB);
}

}  // namespace aa
