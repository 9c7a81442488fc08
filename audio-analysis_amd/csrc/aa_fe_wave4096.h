// ---------------------------------------------------------------------------
// fe_stft_mel_4096: the n_fft = 4096 path, one WAVE per frame, waves
// independent of each other (no block-level synchronisation after the
// prologue).
//
// normalize_data folded into the transform.  It is affine: inside the window
// y = a (x + beta) with a = 2 / scale, beta = scale (1e-6 - 0.5) - lo
// (src/identify_tracks.py:203-208), and the centre padding is y = 0.  The
// transform is linear, so a frame's spectrum is a * FFT(z) with z = x + beta on
// window samples and 0 on the padding, and |.|^p scales by a^p, applied to the
// mel sums.  In a frame without centre padding beta * 1 only reaches bin 0 of
// the unwindowed transform, i.e. bins -1..1 after the Hann convolution (step
// 7), so interior frames take z = x outright (the host keeps kmin >= 2); edge
// frames add beta and zero their padding.  The reference rounds y to f32
// before its f64 STFT; the two agree to f32 rounding (parity tolerance).
//
// z[n] = x[2n] + i x[2n+1] (2048 complex points) is loaded straight into
// registers: lane c holds n = c + 64 r, r = 0..31 (samples 2c + 128 r and +1),
// through a buffer resource spanning the window's view [src, src + n_valid),
// so np.pad zeros, centre padding and the ends of the recording all read as 0
// by the hardware range check (a negative offset wraps past num_records).
//   1. DFT-32 over r in registers                   -> Y[k1][c]
//   2. Y[k1][c] *= W2048^(c k1)                     (ladder from two table entries)
//   3. transpose through the wave's LDS buffer (two half passes, rows padded
//      to 66 float2 so the row writes and the strided reads are
//      conflict-free): lane L = 2 k1 + h gets Y[k1][h + 2m], m = 0..31
//   4. DFT-32 over m in registers -> E_h[k2']
//   5. radix-2 across the lane pair (DPP quad_perm swap):
//      Z[k1 + 32 k2'] = E0 + W64^k2' E1, Z[k1 + 32 (k2' + 32)] = E0 - W64^k2' E1
//   6. real split X[k] = E + W4096^k O from Z[k], conj Z[2048 - k] (both lanes
//      of a pair, 16 bins each), with
//      W4096^(k1 + 32 j) = W4096^k1 W128^j (one table entry per lane)
//   7. |X|^power into the wave's LDS buffer (the periodic Hann was applied to
//      the samples before step 1, by angle addition from two table values)
//   8. sparse mel rows (CSR in LDS, shared by the block), times a^p ->
//      melF[w][t][:] (frame-major: one contiguous row per frame) and the frame
//      maximum -> pmax[w][t]
// Block = 8 waves sharing one CSR image, 2 blocks per CU (16 waves: VGPRs
// capped at 128).  Each XCD (block b runs on XCD b % 8) owns a contiguous
// eighth of the frames -- neighbouring frames overlap by 4096 - hop samples
// and one L2 then serves the overlap -- and its waves take them round-robin,
// wave-major over its blocks, so the last partial round lands on every SIMD
// (block-major over the whole grid left that round to the first XCDs: 16 frames
// on their SIMDs against 12 elsewhere; 69.6 -> 64.0 us alone).
// ---------------------------------------------------------------------------
#pragma once

#include "aa_fe_stft.h"

namespace aa {

constexpr int kMelG = 2;  // mel rows: float4 groups whose loads are issued together
constexpr int kMelP = 1;  // mel rows: slots (rounds of 64) whose first groups load together

// DIAG (tools/fe_bench.hip only): 1 skip the PCM loads, 4 the FFT (steps 1-5),
// 8 the real split, 16 Hann and power, 32 the mel rows, 64 the output stores.
// DIAG & 128 (tools/fe_bench.hip): per-wave s_memtime totals of the frame's
// phases into fe_stamps[global wave][phase][lane] (every lane stores: vector
// stores only) -- 0 loads + Hann, 1 DFT-32 #1, 2 twiddles, 3 transpose,
// 4 DFT-32 #2, 5 radix-2, 6 split + power, 7 mel rows
constexpr int kFeStampPh = 8;
__device__ unsigned long long* fe_stamps = nullptr;
#define FE_STAMP(k)                                                              \
    if constexpr ((DIAG & 128) != 0) {                                           \
        const unsigned long long tn = __builtin_amdgcn_s_memtime();              \
        st_acc[k] += tn - st_prev;                                               \
        st_prev = tn;                                                            \
    }
template <int PM, int DIAG = 0>
__global__ __launch_bounds__(64 * kWpb) __attribute__((amdgpu_waves_per_eu(kWpb / 2, kWpb / 2))) void fe_stft_mel_4096(
    const float* __restrict__ pcm, const aa_window* __restrict__ wins, const float4* __restrict__ stats,
    const float2* __restrict__ tw, const float2* __restrict__ tw4096, const char* __restrict__ cimg,
    int cimg_bytes, int win_len, int hop, int T, int n_mels, int kmin, int kmax, int normalize, float power,
    int n_frames, float* __restrict__ melF, float* __restrict__ pmax) {
    constexpr int NC = 2048;
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    char* cl = reinterpret_cast<char*>(lds);
    const int4* srows = reinterpret_cast<const int4*>(cl);  // CSR image (fe_cimg4096): rows | values
    const float* svals = reinterpret_cast<const float*>(srows + fe_mel_slots(n_mels));
    float2* wb = reinterpret_cast<float2*>(cl + cimg_bytes) + wave * kHalf;  // this wave's buffer

    for (int g = wave; g < cimg_bytes / 1024; g += kWpb)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cimg + g * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void*)(cl + g * 1024), 16, 0, 0);
    const int k1 = lane >> 1, h = lane & 1;
    float2 t1 = tw[lane];                // W2048^c
    float2 t8 = tw[(8 * lane) & (NC - 1)];  // W2048^(8c)
    const float2 wk1 = tw4096[k1];       // W4096^k1
    // (cos, sin) of 2 pi n / 4096 at the lane's first even / odd sample n = 2c, 2c + 1
    const float2 te = tw4096[2 * lane], to = tw4096[2 * lane + 1];
    const float2 hwe = make_float2(te.x, -te.y), hwo = make_float2(to.x, -to.y);
    __syncthreads();                     // vmcnt(0): the CSR image has landed
    unsigned long long st_acc[kFeStampPh] = {}, st_prev = 0;
    // the PCM samples of frame fl into yy (step 0): lane c gets z[c + 64 r]
    auto load_frame = [&](int fl, float2 (&yy)[32]) {
        const int wl = fl / T;
        const aa_window dl = wins[wl];
        const int i0l = (fl - wl * T) * hop - 2048;
        // per-lane sample index, opaque to the optimiser: otherwise it hoists the
        // 64 loop-invariant load offsets and edge masks out of the frame loop
        // and spills them
        int l2l = 2 * lane;
        __asm__ volatile("" : "+v"(l2l));
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(pcm + dl.src), 0, dl.n_valid * 4, 0x00020000);
        // even and odd samples through two address registers: the backend
        // must not fuse a pair into one 8-byte load, whose range check would
        // not zero the two samples independently
        const int offe = i0l - dl.pad_left + l2l;
        const int v0 = i0l - dl.pad_left;  // the frame's first sample in the view
        if (v0 >= 0 && v0 + 4096 <= dl.n_valid) {
            // frame inside the view (wave-uniform): no sample is range checked,
            // so a lane's pair comes in one 8-byte load (32 fully used 512-B
            // wave-instructions instead of 64 half-used)
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const uint2 v = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rs, (offe + 128 * r) * 4, 0, 0));
                yy[r] = make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
            }
        } else {
            int offo = offe + 1;
            __asm__ volatile("" : "+v"(offo));
#pragma unroll
            for (int r = 0; r < 32; ++r) yy[r] = make_float2(load_view(rs, offe + 128 * r), load_view(rs, offo + 128 * r));
        }
    };

    // XCD x (block b runs on XCD b % 8) owns frames [x n / 8, (x + 1) n / 8);
    // its waves take them round-robin, wave-major over its blocks, so the last,
    // partial round is spread over every XCD, CU and SIMD (a block's waves w
    // and w + 4 share a SIMD) instead of filling the first XCDs only
    const int nbx = gridDim.x >> 3;  // blocks per XCD (grid a multiple of 8)
    const int xcd = blockIdx.x & 7;
    const int f_end = (int)((long long)(xcd + 1) * n_frames / 8);
    const int G = nbx * kWpb;
    const int f_first = (int)((long long)xcd * n_frames / 8) + wave * nbx + (blockIdx.x >> 3);
    for (int fi = f_first; fi < f_end; fi += G) {
        const int w = fi / T;
        const int t = fi - w * T;
        if constexpr ((DIAG & 128) != 0) st_prev = __builtin_amdgcn_s_memtime();
        float apow = 1.f, beta = 0.f;
        if (normalize) {
            float lo = INFINITY, hi = -INFINITY;
#pragma unroll
            for (int s = 0; s < kStatSplit; ++s) {
                const float4 st = stats[w * kStatSplit + s];
                lo = fminf(lo, st.x);
                hi = fmaxf(hi, st.y);
            }
            const float scale = __fsub_rn(hi, lo);  // == max(x - min) (monotone rounding)
            const float a = __fdiv_rn(2.f, scale);
            apow = PM == PM_SQUARE ? a * a : PM == PM_ABS ? a : powf(a, power);
            beta = fmaf(scale, 0.000001f - 0.5f, -lo);
        }
        const int i0 = t * hop - 2048;  // window index of the frame's first sample
        // per-lane sample index, opaque to the optimiser: otherwise it hoists the
        // 64 loop-invariant load offsets and edge masks out of the frame loop
        // and spills them
        int l2 = 2 * lane;
        __asm__ volatile("" : "+v"(l2));
        float2 wk = wk1;  // per frame, or W4096^k1 W128^j gets hoisted as 32 live twiddles
        __asm__ volatile("" : "+v"(wk.x), "+v"(wk.y));
        float2 u[32];
        {
            // ---- load (steps 0) ----
            float2 y[32];
            if constexpr ((DIAG & 1) != 0) {
#pragma unroll
                for (int r = 0; r < 32; ++r) y[r] = make_float2((float)(lane + r), (float)(t - r));
            } else {
                load_frame(fi, y);
            }
            if (normalize && (i0 < 0 || i0 + 4096 > win_len)) {  // edge frame: + beta, centre padding 0
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    const int i = i0 + l2 + 128 * r;
                    y[r].x = (i >= 0 && i < win_len) ? y[r].x + beta : 0.f;
                    y[r].y = (i + 1 >= 0 && i + 1 < win_len) ? y[r].y + beta : 0.f;
                }
            }
            // periodic Hann, w[n] = 1/2 - cos(2 pi n / 4096) / 2 at n = 2c + 128 r
            // (+1): cos(a + 2 pi r / 32) by angle addition from the lane's
            // cos/sin of a (table values; opaque per frame so the 64 products
            // are not hoisted into live registers)
            // The upper half-wave's (-1)^r input modulation of step 1 is folded
            // in as the sign of the odd-r weights: +-1/2 per lane.
            float2 he = hwe, ho = hwo;
            float hs = lane >= 32 ? -0.5f : 0.5f;
            __asm__ volatile("" : "+v"(he.x), "+v"(he.y), "+v"(ho.x), "+v"(ho.y), "+v"(hs));
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const float cr = kW32[r][0], sr = -kW32[r][1];  // cos, sin of 2 pi r / 32
                const float ce = fmaf(he.x, cr, -he.y * sr), co = fmaf(ho.x, cr, -ho.y * sr);
                const float a = (r & 1) ? hs : 0.5f;  // w = a (1 - cos)
                y[r].x *= fmaf(-a, ce, a);
                y[r].y *= fmaf(-a, co, a);
            }
            FE_STAMP(0)
            if constexpr ((DIAG & 4) != 0) {
#pragma unroll
                for (int j = 0; j < 32; ++j) u[j] = y[j];
            } else {
                // (the same steps as aa_wavefft.h's wave_hann + wave_fft_core,
                // kept inline here: called as functions, the register
                // allocation of this kernel spills 11 VGPRs)
                // The transpose (step 3) runs in two passes of 16 registers per
                // lane, each pass freeing 16 registers before it fills 16, so the
                // data never occupies more than 64 VGPRs.  For that, the upper
                // half-wave (columns c >= 32) works with its rows rotated by 16:
                // (-1)^r on the input gives DFT output X[(k + 16) % 32] in
                // register k (step 1), its twiddle ladder is rotated to match
                // (step 2), it reads its columns rotated by 16 (step 3), and
                // undoes that rotation of the second DFT by (-1)^k on the odd
                // outputs (step 4).
                const unsigned up = lane >= 32 ? 0x80000000u : 0u;  // sign mask of the upper half
                auto flip = [up](float2 v) {
                    return make_float2(__uint_as_float(__float_as_uint(v.x) ^ up),
                                       __uint_as_float(__float_as_uint(v.y) ^ up));
                };
                // ---- 1. DFT-32 over r ----
                // (the (-1)^r of the upper half rides on its Hann weights, above)
                dft32(y);
                FE_STAMP(1)
                // ---- 2. twiddle W2048^(c row) = (W^8c)^(row/8) (W^c)^(row%8),
                // row = k (+16 mod 32 in the upper half); ladders rebuilt per frame
                // (<= 4 roundings per twiddle; not kept live across the loop) ----
                __asm__ volatile("" : "+v"(t1.x), "+v"(t1.y), "+v"(t8.x), "+v"(t8.y));
                float2 p1[8], p8[4];
                p1[0] = make_float2(1.f, 0.f);
                p1[1] = t1;
#pragma unroll
                for (int i = 2; i < 8; ++i) p1[i] = cmul(p1[i - 1], t1);
                {
                    const float2 q1 = t8, q2 = cmul(t8, t8), q3 = cmul(q2, t8);
                    const bool hi = lane >= 32;
                    p8[0] = hi ? q2 : make_float2(1.f, 0.f);
                    p8[1] = hi ? q3 : q1;
                    p8[2] = hi ? make_float2(1.f, 0.f) : q2;
                    p8[3] = hi ? q1 : q3;
                }
#pragma unroll
                for (int k = 0; k < 32; ++k) {
                    const float2 tk = (k & 7) == 0 ? p8[k >> 3] : cmul(p8[k >> 3], p1[k & 7]);
                    y[dperm(k)] = cmul(y[dperm(k)], tk);
                }
                FE_STAMP(2)
                // ---- 3. transpose in two passes: pass p moves registers
                // 16p..16p+15 (rows (16p + 16 [c >= 32]) % 32 + 0..15 of column
                // c) and lane (k1, h) takes columns h + 2m, m in the 16-range
                // 16 ((k1 / 16) ^ p) of row k1, into u[16p ..] ----
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) wb[k * kRow + lane] = y[dperm(16 * pass + k)];
                    wave_sync();
                    const float2* src = wb + (k1 & 15) * kRow + h + 32 * (((k1 >> 4) ^ pass) & 1);
#pragma unroll
                    for (int i = 0; i < 16; ++i) u[16 * pass + i] = src[2 * i];
                    wave_sync();
                }
                FE_STAMP(3)
                // ---- 4. DFT-32 over m (input rotated by 16 in the upper half:
                // output k times (-1)^k) ----
                dft32(u);
#pragma unroll
                for (int k = 1; k < 32; k += 2) u[dperm(k)] = flip(u[dperm(k)]);
                FE_STAMP(4)
                // ---- 5. radix-2 across the lane pair: lane h = 1 sends
                // W64^j E1, lane h = 0 sends E0; then Z = E0 + W E1 (h = 0) and
                // E0 - W E1 (h = 1) are recv +- own ----
                const float sg = h ? -1.f : 1.f;
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    const float2 e = u[dperm(j)];
                    const float2 wj = wconst64(j);
                    const float2 g = h ? cmul(wj, e) : e;
                    const float2 rv = make_float2(swap_pair(g.x), swap_pair(g.y));
                    u[dperm(j)] = make_float2(fmaf(sg, g.x, rv.x), fmaf(sg, g.y, rv.y));
                }
                FE_STAMP(5)
            }
        }
        // lane holds Z[k1 + 32 (32 h + j)] in u[dperm(j)]
        // ---- 6. real split and |X|^power ----
        if (h && !(DIAG & 8)) {
#pragma unroll
            for (int j = 0; j < 32; ++j) wb[k1 + 32 * j] = u[dperm(j)];  // Z[1024 + k1 + 32 j]
        }
        wave_sync();
        // Both lanes of a pair split: lane h takes the bins k = k1 + 32 (16 h +
        // i), i < 16 (all 1024 bins below NC/2 over the 64 lanes; bands above
        // take the generic kernel, see choose_kernel).  Z[k] is the h = 0 lane's
        // u[dperm(16 h + i)] (the h = 1 lane swaps it over from its partner),
        // its mirror Z[2048 - k] the h = 1 lanes' LDS copy.  |X|^p is stored
        // reversed from the top of the wave's buffer (bin k at float Pt[-k],
        // Pt = float 2 kHalf - 1), where it overlaps mirrors that later
        // iterations still read, so the 16 values wait in registers until the
        // loop is done.
        float* Pt = reinterpret_cast<float*>(wb) + (2 * kHalf - 1);
        if (!(DIAG & 8)) {
            // mirror of bin k1 + 32 (16 h + i) at wb[1024 - k] = mb[32 (31 - i)]
            // (one base register, non-negative immediates; wb[1024], read for
            // k = 0, is in the buffer and unused)
            const float2* mb = wb + (32 - k1) - 512 * h;
            float* pk = Pt - k1 - 512 * h - 32 * 15;  // bin k at pk[32 (15 - i)] = Pt[-k]
            // W4096^k = W4096^k1 (W4096^512)^h W128^i, W4096^512 = (r, -r)
            const float r2 = 0.70710678118654752440f;
            const float2 wkh = h ? make_float2(r2 * (wk.x + wk.y), r2 * (wk.y - wk.x)) : wk;
            float pw[16];
            float2 zm[16];  // mirrors, read 8 ahead of their use
#pragma unroll
            for (int i = 0; i < 8; ++i) zm[i] = mb[32 * (31 - i)];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i % 8 == 0 && i + 8 < 16) {
#pragma unroll
                    for (int k = i + 8; k < i + 16; ++k) zm[k] = mb[32 * (31 - k)];
                }
                const float2 hiv = u[dperm(16 + i)];
                const float2 oth = make_float2(swap_pair(hiv.x), swap_pair(hiv.y));
                const float2 a = h ? oth : u[dperm(i)];
                const float2 zb = zm[i];
                const float2 b = (i == 0 && k1 == 0 && !h) ? a : zb;  // Z[NC - k]; Z[0] for k = 0
                const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
                const float2 O = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
                float2 wj = cmul(wkh, wconst128(i));  // W4096^k
                __asm__ volatile("" : "+v"(wj.x), "+v"(wj.y));  // formed here, not hoisted
                const float2 X = cadd(E, cmul(wj, O));
                pw[i] = pow_mag<PM>(X.x, X.y, power);
            }
            if (!(DIAG & 16)) {
#pragma unroll
                for (int i = 0; i < 16; ++i) pk[32 * (15 - i)] = pw[i];
            }
        }
        wave_sync();
        FE_STAMP(6)
        // ---- 8. mel rows ----
        // rows of the CSR image are zero-padded to whole float4s (value
        // offsets 16-B aligned); the padding adds exact zeros
        float fmx = 0.f;
        float* orow = melF + (size_t)fi * n_mels;  // fi = w T + t
        const int nslot = fe_mel_slots(n_mels);
        // the slot index opaque per frame: the rows' descriptors and value
        // addresses are frame-invariant, and hoisted out of the frame loop they
        // would stay live through the FFT (spills)
        int si0 = lane;
        __asm__ volatile("" : "+v"(si0));
        // slot si holds band rw.w (-1: empty, length 0) covering bins [x, x +
        // L): its values are stored reversed and front-padded to L4 = roundup(L,
        // 4) (fe_cimg4096), so with P reversed the row is an ascending run
        // pv[0 .. L4)
        // P slots per trip, the first G float4 groups of each: every load issued
        // before the first FMA (one LDS round trip for P x G groups instead of
        // one per group), then each row's FMA chain in the order of a plain
        // loop over the row (identical sums; fe_bench's hash,
        // profiles/r06/fe_mel_groups.txt)
        constexpr int G = kMelG, NP = kMelP;
        for (int si = si0; si < ((DIAG & 32) ? 0 : nslot); si += 64 * NP) {
            int4 rw[NP];
            const float4* wv[NP];
            const float* pv[NP];
            float4 wa[NP][G];
            float pa[NP][G][4];
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int sq = si + 64 * q;
                // a slot past the last round is an empty row (its loads stay
                // inside the wave's power buffer, as fe_cimg4096's empty slots)
                rw[q] = sq < nslot ? srows[sq] : make_int4(kmin + 3, 0, 0, -1);
                wv[q] = reinterpret_cast<const float4*>(svals + rw[q].z);
                pv[q] = Pt - rw[q].x - (rw[q].y - 1);  // bins x + L4 - 1 down to x
                // (groups past the row re-read its last group: in range, unused)
                const int glast = max((rw[q].y >> 2) - 1, 0);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int gi = min(g, glast);
                    wa[q][g] = wv[q][gi];
#pragma unroll
                    for (int e = 0; e < 4; ++e) pa[q][g][e] = pv[q][4 * gi + e];
                }
            }
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                float s = 0.f;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (4 * g < rw[q].y) {
                        s = fmaf(wa[q][g].x, pa[q][g][0], s);
                        s = fmaf(wa[q][g].y, pa[q][g][1], s);
                        s = fmaf(wa[q][g].z, pa[q][g][2], s);
                        s = fmaf(wa[q][g].w, pa[q][g][3], s);
                    }
                }
                for (int i = 4 * G; i < rw[q].y; i += 4) {
                    const float4 a = wv[q][i >> 2];
                    s = fmaf(a.x, pv[q][i], s);
                    s = fmaf(a.y, pv[q][i + 1], s);
                    s = fmaf(a.z, pv[q][i + 2], s);
                    s = fmaf(a.w, pv[q][i + 3], s);
                }
                s *= apow;
                if (!(DIAG & 64) && rw[q].w >= 0) orow[rw[q].w] = s;
                fmx = fmaxf(fmx, s);
            }
        }
        fmx = wave_max(fmx);
        if (lane == 0 && !(DIAG & 64)) pmax[fi] = fmx;
        wave_sync();  // the buffer is rewritten by the next frame
        FE_STAMP(7)
    }
    if constexpr ((DIAG & 128) != 0) {
        const size_t gw = (size_t)blockIdx.x * kWpb + wave;
#pragma unroll
        for (int k = 0; k < kFeStampPh; ++k) fe_stamps[(gw * kFeStampPh + k) * 64 + lane] = st_acc[k];
    }
}

}  // namespace aa
