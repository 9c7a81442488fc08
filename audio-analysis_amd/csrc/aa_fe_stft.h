// The three LDS Stockham STFT + mel kernels of the front end, fe_stft_mel (n_fft
// 2048..8192), fe_stft_mel_small (256..1024) and fe_stft_mel_mixed (the sizes
// that are no powers of two), and the device helpers they share.  Included by
// aa_frontend.hip; LDS layouts and constants: aa_fe_plan.h.
#pragma once

#include "aa_fe_plan.h"

namespace aa {

// LDS index of complex point i: one float2 of padding per 8 keeps the radix-8
// scatter of pass 1 (stride 8) and the NS = 8 scatter of pass 2 conflict-free.
__device__ __forceinline__ int pidx(int i) { return i + (i >> 3); }

// One Stockham pass of radix R over NC points held in LDS (src -> dst), for
// sub-transform size NS >= 8 (product of the earlier radices), by the NL lanes
// that share the transform: lane l of them handles butterflies j = l + b*NL.
// Its twiddles depend only on (j, NS), so they are loaded once per block into
// registers (load) and reused for every frame.
template <int NC, int R, int NL, int NS>
struct Pass {
    static constexpr int NB = NC / R;
    static constexpr int PER = NB / NL;
    static_assert(NB % NL == 0 && NB % 8 == 0 && NS % 8 == 0, "whole butterflies per lane, strides of whole pads");
    float2 t[PER][R - 1];
    __device__ __forceinline__ void load(const float2* __restrict__ tw, int l) {
#pragma unroll
        for (int b = 0; b < PER; ++b) {
            const int k = (l + b * NL) % NS;
#pragma unroll
            for (int r = 1; r < R; ++r)  // unconditional loads: all in flight together
                t[b][r - 1] = tw[(r * k * (NC / (NS * R))) & (NC - 1)];
        }
    }
    __device__ __forceinline__ void run(const float2* __restrict__ src, float2* __restrict__ dst, int l) const {
#pragma unroll
        for (int b = 0; b < PER; ++b) {
            const int j = l + b * NL;
            // NB and NS are multiples of 8, so pidx(i + 8c) = pidx(i) + 9c: one
            // address per butterfly side, the rest immediate offsets
            const float2* s0 = src + pidx(j);
            float2 v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = s0[r * (NB + NB / 8)];
#pragma unroll
            for (int r = 1; r < R; ++r) v[r] = cmul(v[r], t[b][r - 1]);
            if constexpr (R == 8) dft8(v);
            if constexpr (R == 4) dft4(v[0], v[1], v[2], v[3]);
            if constexpr (R == 2) dft2(v[0], v[1]);
            const int k = j % NS;
            float2* d0 = dst + pidx((j / NS) * NS * R + k);
#pragma unroll
            for (int r = 0; r < R; ++r) d0[r * (NS + NS / 8)] = v[r];
        }
    }
};

// fe_stft_mel's pass: Pass's twiddle registers and load() for a block of NT
// threads, with a run() of its own that computes one LDS address per point.
// Pass::run is valid here too (the static_assert) but is other code for that
// kernel (22 to 27 fewer VGPRs, another occupancy), which was to stay as it was.
template <int NC, int R, int NT, int NS>
struct BlockPass : Pass<NC, R, NT, NS> {
    using P = Pass<NC, R, NT, NS>;  // (whose static_assert holds: no partial round of butterflies, NS >= 8)
    __device__ __forceinline__ void run(const float2* __restrict__ src, float2* __restrict__ dst) const {
#pragma unroll
        for (int b = 0; b < P::PER; ++b) {
            const int j = threadIdx.x + b * NT;
            float2 v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = src[pidx(j + r * P::NB)];
#pragma unroll
            for (int r = 1; r < R; ++r) v[r] = cmul(v[r], P::t[b][r - 1]);
            if constexpr (R == 8) dft8(v);
            if constexpr (R == 4) dft4(v[0], v[1], v[2], v[3]);
            if constexpr (R == 2) dft2(v[0], v[1]);
            const int k = j % NS;
            const int o = (j / NS) * NS * R + k;
#pragma unroll
            for (int r = 0; r < R; ++r) dst[pidx(o + r * NS)] = v[r];
        }
    }
};

// Correctly rounded (x - lo) / scale as three instructions: with
// y = RN(1/scale), q0 = RN(a y) is within an ulp of a/scale, the residual
// a - q0 scale is exact in one fma, and RN(q0 + r y) is the correctly rounded
// quotient (Markstein's theorem; tools/div_check.hip compares it with
// __fdiv_rn on 3.4e10 operand pairs: no mismatch).  Then normalize_data's
// remaining steps in reference order (src/identify_tracks.py:205-208).
__device__ __forceinline__ float normalize_sample(float x, float lo, float scale, float inv) {
    const float a = __fsub_rn(x, lo);
    const float q0 = __fmul_rn(a, inv);
    const float r = fmaf(-q0, scale, a);
    float y = fmaf(r, inv, q0);
    y = __fadd_rn(y, 0.000001f);
    y = __fsub_rn(y, 0.5f);
    return __fmul_rn(y, 2.0f);
}

// complex64 -> np.abs -> ** power.  The power mode is a template parameter:
// a runtime select between the three forms would make every bin pay for the
// inlined powf.  |X|^2 is formed directly (the reference squares a rounded
// hypot: the two differ by an ulp, far inside the f32-FFT tolerance), and the
// other modes use the hardware square root (v_sqrt_f32, 1 ulp) rather than the
// correctly rounded expansion.
enum { PM_GENERAL = 0, PM_ABS = 1, PM_SQUARE = 2 };
template <int PM>
__device__ __forceinline__ float pow_mag(float re, float im, float power) {
    const float m2 = fmaf(re, re, im * im);
    if constexpr (PM == PM_SQUARE) return m2;
    const float mag = __builtin_amdgcn_sqrtf(m2);
    if constexpr (PM == PM_ABS) return mag;
    else return powf(mag, power);
}

// (The stats fold, the view predicate and the real split stay written out in each
// kernel: shared, they are other code for fe_stft_mel -- ~110 more instructions, or
// its split's products paired into other FMAs (-ffp-contract=fast): other bits.)

// One CSR mel row: sum of wv[i] pv[i], i < len, in index order, as predicated
// W-wide chunks: all LDS reads of a chunk in flight at once.
template <int W>
__device__ __forceinline__ float mel_row_dot(const float* wv, const float* pv, int len) {
    float s = 0.f;
    for (int i0 = 0; i0 < len; i0 += W) {
        float a[W], b[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const int ii = min(i0 + i, len - 1);  // unconditional LDS reads
            a[i] = (i0 + i < len) ? wv[ii] : 0.f;
            b[i] = pv[ii];
        }
#pragma unroll
        for (int i = 0; i < W; ++i) s = fmaf(a[i], b[i], s);
    }
    return s;
}

// ---------------------------------------------------------------------------
// fe_stft_mel
// Transform plan for NC = NFFT/2 complex points with NT = NC/8 threads:
//   pass 1  radix 8, NS = 1   (input read from the windowed PCM segment)
//   pass 2  radix 8, NS = 8
//   pass 3  radix 8, NS = 64
//   pass 4  radix NC/512, NS = 512   (NC = 1024: 2, 2048: 4, 4096: 8)
// ---------------------------------------------------------------------------
template <int NFFT, int PM>
__global__ __launch_bounds__(NFFT / 16) void fe_stft_mel(
    const float* __restrict__ pcm, const aa_window* __restrict__ wins, const float4* __restrict__ stats,
    const float* __restrict__ hann, const float2* __restrict__ tw, const float2* __restrict__ tw2,
    const int4* __restrict__ rows, const float* __restrict__ vals, int nnz, int win_len, int hop, int T,
    int n_mels, int kmin, int kmax, int normalize, float power, int nblk, int n_items,
    float* __restrict__ melS, float* __restrict__ blkmax) {
    constexpr int NC = NFFT / 2;
    constexpr int NT = NC / 8;
    constexpr int R4 = NC / 512;
    static_assert(NC >= 1024 && NC <= 4096, "NFFT 2048..8192");
    constexpr int KREG = 4;  // post-processing bins per thread with register twiddles
    extern __shared__ float lds[];
    const FeLdsGeneric L(NFFT, hop, n_mels, nnz);
    float* seg = lds;
    float2* bufA = reinterpret_cast<float2*>(seg + L.seg);
    float2* bufB = bufA + L.buf;
    float* melT = reinterpret_cast<float*>(bufB + L.buf);  // [n_mels][kFpb] staging
    int4* srows = reinterpret_cast<int4*>(melT + L.melT);
    float* svals = reinterpret_cast<float*>(srows + L.rows);

    // --- per-thread constants, loaded once per block ---
    const int tid = threadIdx.x;
    float hw[8][2];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = tid + r * (NC / 8);
        const float2 h = reinterpret_cast<const float2*>(hann)[n];
        hw[r][0] = h.x;
        hw[r][1] = h.y;
    }
    BlockPass<NC, 8, NT, 8> p2;
    BlockPass<NC, 8, NT, 64> p3;
    BlockPass<NC, R4, NT, 512> p4;
    p2.load(tw, tid);
    p3.load(tw, tid);
    p4.load(tw, tid);
    float2 w2r[KREG];
#pragma unroll
    for (int i = 0; i < KREG; ++i) {
        w2r[i] = tw2[min(kmin + tid + i * NT, kmax)];
    }
    for (int i = tid; i < n_mels; i += NT) srows[i] = rows[i];
    for (int i = tid; i < nnz; i += NT) svals[i] = vals[i];

    __syncthreads();
    // persistent loop over (window, frame block) items
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int w = item / nblk;
    const int fb = item - w * nblk;
    const int f0 = fb * kFpb;
    const int nf = min(kFpb, T - f0);
    const int seg_len = (nf - 1) * hop + NFFT;
    // --- normalisation constants (normalize_data, :203-208) ---
    const aa_window d = wins[w];
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int s = 0; s < kStatSplit; ++s) {
        float4 st = stats[w * kStatSplit + s];
        lo = fminf(lo, st.x);
        hi = fmaxf(hi, st.y);
    }
    const float scale = __fsub_rn(hi, lo);  // == max(x - min) (monotone rounding)
    const float inv = __fdiv_rn(1.f, scale);

    // --- overlapped segment -> LDS, normalised; loads issued in batches of
    // SEGU per thread before any is consumed ---
    const int base = f0 * hop - NFFT / 2;  // window index of seg[0]
    constexpr int SEGU = 8;
    const long long safe = d.n_valid > 0 ? d.src : 0;  // any in-bounds sample
    for (int q0 = 0; q0 < seg_len; q0 += SEGU * NT) {
        float raw[SEGU];
        bool ok[SEGU];
#pragma unroll
        for (int u = 0; u < SEGU; ++u) {  // unconditional loads from clamped addresses
            const int q = q0 + u * NT + tid;
            const int i = base + q;
            const int rel = i - d.pad_left;
            ok[u] = q < seg_len && i >= 0 && i < win_len && rel >= 0 && rel < d.n_valid;
            raw[u] = pcm[ok[u] ? d.src + rel : safe];
        }
#pragma unroll
        for (int u = 0; u < SEGU; ++u) {
            const int q = q0 + u * NT + tid;
            const int i = base + q;
            if (q < seg_len) {
                float v = 0.f;
                if (i >= 0 && i < win_len) {
                    v = ok[u] ? raw[u] : 0.f;
                    if (normalize) v = normalize_sample(v, lo, scale, inv);
                }
                seg[q] = v;
            }
        }
    }
    __syncthreads();

    float bmax = 0.f;
    for (int f = 0; f < nf; ++f) {
        // pass 1 (NS = 1) straight from the segment: z[n] = xw[2n] + i xw[2n+1]
        {
            const float* x = seg + f * hop;
            float2 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int n = tid + r * NT;
                v[r] = make_float2(x[2 * n] * hw[r][0], x[2 * n + 1] * hw[r][1]);
            }
            dft8(v);
#pragma unroll
            for (int r = 0; r < 8; ++r) bufA[pidx(tid * 8 + r)] = v[r];
        }
        __syncthreads();
        p2.run(bufA, bufB);
        __syncthreads();
        p3.run(bufB, bufA);
        __syncthreads();
        p4.run(bufA, bufB);
        __syncthreads();
        const float2* Z = bufB;             // natural order
        float* Pf = reinterpret_cast<float*>(bufA);  // free scratch for |X|^p
        for (int i = 0; kmin + tid + i * NT <= kmax; ++i) {
            const int k = kmin + tid + i * NT;
            float re, im;
            if (k == 0 || k == NC) {
                const float2 z0 = Z[0];  // pidx(0) == 0
                re = (k == 0) ? z0.x + z0.y : z0.x - z0.y;
                im = 0.f;
            } else {
                const float2 a = Z[pidx(k)];
                const float2 b = Z[pidx(NC - k)];  // conj taken below
                // E = (a + conj b)/2 ; O = -i (a - conj b)/2 ; X = E + W^k O
                const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
                const float2 O = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
                float2 wk;
                if (i < KREG) {
                    wk = w2r[0];
#pragma unroll
                    for (int q = 1; q < KREG; ++q) if (i == q) wk = w2r[q];
                } else {
                    wk = tw2[k];
                }
                const float2 X = cadd(E, cmul(wk, O));
                re = X.x;
                im = X.y;
            }
            Pf[k - kmin] = pow_mag<PM>(re, im, power);
        }
        __syncthreads();
        for (int m = tid; m < n_mels; m += NT) {
            const int4 rw = srows[m];
            const float s = mel_row_dot<16>(svals + rw.z, Pf + (rw.x - kmin), rw.y);
            melT[m * kFpb + f] = s;
            bmax = fmaxf(bmax, s);
        }
        __syncthreads();  // P / buffers reused by the next frame
    }
    // staged [n_mels][nf] tile -> melS[w][m][f0 .. f0 + nf)
    const float inv_nm = 1.0f / (float)n_mels;  // exact row below 2^21 (as in fe_db)
    for (int idx = tid; idx < nf * n_mels; idx += NT) {  // frame-major rows
        const int f = (int)(((float)idx + 0.5f) * inv_nm), m = idx - f * n_mels;
        melS[((size_t)w * T + f0 + f) * n_mels + m] = melT[m * kFpb + f];
    }
    // item max -> blkmax[w][fb]
    __shared__ float red[NT / 64];
    bmax = wave_max(bmax);
    if ((tid & 63) == 0) red[tid >> 6] = bmax;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < NT / 64; ++k) bmax = fmaxf(bmax, red[k]);
        blkmax[w * nblk + fb] = bmax;
    }
    }  // item loop
}

// ---------------------------------------------------------------------------
// fe_stft_mel_small: n_fft 256, 512 and 1024 -- the same contract as
// fe_stft_mel (window views, normalize_sample, centre padding, periodic Hann,
// f32, pow_mag, CSR mel rows, melS[w][t][m]), shaped for short transforms at
// short hops: a frame belongs to a GROUP of G = NC/8 lanes (64, 32 or 16), so
// a wave carries 64/G = 1, 2 or 4 frames and a frame never spans waves.  The
// transform is three Stockham passes, radix 8 (NS = 1, from the samples),
// radix 8 (NS = 8) and radix NC/64 = 8, 4 or 2 (NS = 64), ping-ponging
// between the group's two LDS buffers with wave_sync() between passes; the
// block-wide barriers are the two around the staging of the PCM span.
//
// Block = 4 waves on fe_small_fpb() consecutive frames of one window (8 at
// 1024, 16 below: 2, 2 or 1 rounds of 4, 8 or 16 frames).  Their overlapped
// PCM span is loaded and normalised once into LDS when (fpb - 1) hop + n_fft
// fits kSmallSeg samples; otherwise (hop well above n_fft) every lane loads
// and normalises its own 16 samples from global memory.  Each wave writes one
// partial maximum per item: blkmax[w][fb][wave].  The span budget and the
// register bound (3 waves per SIMD) are set so that three blocks share a CU
// at the usual filterbanks (48 KiB + CSR <= 53 KiB of LDS each).
//
// LDS banks (ds_read_b32 / stores: word mod 32 per half-wave or 16-lane
// store group; ds_read_b64: word mod 64 per half-wave):
//   span      even samples in segE, odd samples in segO = segE + kSmallHalf,
//             kSmallHalf = 16 mod 32: the staging stores (lane q -> word q/2
//             of either half) and the pass-1 reads (lane n -> word n of each
//             half, whatever the parity of the frame's start) are
//             conflict-free; the interleaved layout of fe_stft_mel reads at
//             stride 2, 2-way.
//   passes    pidx() pads one float2 per 8.  The scatters of pass 1 (float2
//             stride 9) and pass 2 (rows of 8 at stride 72) are conflict-free;
//             pass 3 stores runs of consecutive points, where the pad makes 1
//             or 2 of 16 lanes wrap onto a used bank: 2-way, inside the store's
//             own issue time.  The gathers of passes 2 and 3 and the real
//             split read 32 consecutive points per half-wave across 4 pads
//             (36 float2 slots over 32): 3 or 4 lanes share a bank 2-way, so
//             such a ds_read_b64 takes 2 LDS cycles per half-wave instead of
//             1.  At n_fft 256 the two groups of a half-wave sit 144 float2
//             apart (16 mod 32) and overlap by 2 slots the same way.
//   mel rows  a lane per band: the rows' offsets and lengths set the banks
//             (neighbouring triangles overlap by half), as in fe_stft_mel.
// ---------------------------------------------------------------------------
template <int NFFT, int PM>
__global__ __launch_bounds__(64 * kSmallWaves, 3) void fe_stft_mel_small(
    const float* __restrict__ pcm, const aa_window* __restrict__ wins, const float4* __restrict__ stats,
    const float* __restrict__ hann, const float2* __restrict__ tw, const float2* __restrict__ tw2,
    const int4* __restrict__ rows, const float* __restrict__ vals, int nnz, int win_len, int hop, int T,
    int n_mels, int kmin, int kmax, int normalize, float power, int nblk, int n_items,
    float* __restrict__ melS, float* __restrict__ blkmax) {
    constexpr int NC = NFFT / 2;
    constexpr int G = NC / 8;             // lanes per frame
    constexpr int FPW = 64 / G;           // frames per wave
    constexpr int FPR = kSmallWaves * FPW;  // frames per round of the block
    constexpr int FPB = fe_small_fpb(NFFT);
    constexpr int NCP = NC + NC / 8;      // padded group buffer (float2); FPW * NCP == kSmallBuf
    constexpr int KB = 9;                 // bins per lane: NC + 1 over G lanes
    static_assert(NC == 128 || NC == 256 || NC == 512, "NFFT 256..1024");
    static_assert(FPB % FPR == 0 && FPW * NCP == kSmallBuf, "rounds of whole waves");
    extern __shared__ float lds[];
    const FeLdsSmall L(n_mels, nnz);
    float* segE = lds;                    // even samples of the span
    float* segO = segE + L.half;          // odd samples
    float2* bufs = reinterpret_cast<float2*>(segO + L.half);
    int4* srows = reinterpret_cast<int4*>(bufs + L.bufs);
    float* svals = reinterpret_cast<float*>(srows + L.rows);

    const int tid = threadIdx.x;
    const int wv = tid >> 6, lane = tid & 63;
    const int g = lane / G, gl = lane % G;
    float2* bufA = bufs + wv * 2 * kSmallBuf + g * NCP;
    float2* bufB = bufA + kSmallBuf;

    // --- per-thread constants, loaded once per block ---
    float hw[8][2];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float2 h = reinterpret_cast<const float2*>(hann)[gl + r * G];
        hw[r][0] = h.x;
        hw[r][1] = h.y;
    }
    Pass<NC, 8, G, 8> p2;
    Pass<NC, NC / 64, G, 64> p3;
    p2.load(tw, gl);
    p3.load(tw, gl);
    float2 w2r[KB];
#pragma unroll
    for (int i = 0; i < KB; ++i) w2r[i] = tw2[min(kmin + gl + i * G, kmax)];
    for (int i = tid; i < n_mels; i += 64 * kSmallWaves) srows[i] = rows[i];
    for (int i = tid; i < nnz; i += 64 * kSmallWaves) svals[i] = vals[i];
    const bool shared = fe_small_shared(NFFT, hop);  // the span fits: stage it once
    __syncthreads();

    // persistent loop over (window, frame block) items
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int w = item / nblk;
        const int fb = item - w * nblk;
        const int f0 = fb * FPB;
        const int nf = min(FPB, T - f0);
        // --- normalisation constants (normalize_data, :203-208) ---
        const aa_window d = wins[w];
        float lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int s = 0; s < kStatSplit; ++s) {
            const float4 st = stats[w * kStatSplit + s];
            lo = fminf(lo, st.x);
            hi = fmaxf(hi, st.y);
        }
        const float scale = __fsub_rn(hi, lo);  // == max(x - min) (monotone rounding)
        const float inv = __fdiv_rn(1.f, scale);
        const long long safe = d.n_valid > 0 ? d.src : 0;  // any in-bounds sample
        // sample i of the centre-padded window: np.pad zeros outside the view,
        // normalised inside the window, 0 on the centre padding
        auto in_view = [&](int i) {
            const int rel = i - d.pad_left;
            return i >= 0 && i < win_len && rel >= 0 && rel < d.n_valid;
        };
        auto finish = [&](int i, bool ok, float raw) {
            float v = 0.f;
            if (i >= 0 && i < win_len) {
                v = ok ? raw : 0.f;
                if (normalize) v = normalize_sample(v, lo, scale, inv);
            }
            return v;
        };

        if (shared) {
            __syncthreads();  // the previous item's frames have read their span
            const int seg_len = (nf - 1) * hop + NFFT;
            const int base = f0 * hop - NFFT / 2;  // window index of the span's first sample
            constexpr int SEGU = 4;
            for (int q0 = 0; q0 < seg_len; q0 += SEGU * 64 * kSmallWaves) {
                float raw[SEGU];
                bool ok[SEGU];
#pragma unroll
                for (int u = 0; u < SEGU; ++u) {  // unconditional loads from clamped addresses
                    const int q = q0 + u * 64 * kSmallWaves + tid;
                    ok[u] = q < seg_len && in_view(base + q);
                    raw[u] = pcm[ok[u] ? d.src + (base + q - d.pad_left) : safe];
                }
#pragma unroll
                for (int u = 0; u < SEGU; ++u) {
                    const int q = q0 + u * 64 * kSmallWaves + tid;
                    if (q < seg_len) ((q & 1) ? segO : segE)[q >> 1] = finish(base + q, ok[u], raw[u]);
                }
            }
            __syncthreads();
        }

        float bmax = 0.f;
#pragma unroll 1
        for (int rd = 0; rd < FPB / FPR; ++rd) {
            const int fw = rd * FPR + wv * FPW;  // the wave's first frame of this round
            if (fw >= nf) break;                 // wave-uniform: no frame left for this wave
            // a group past the last frame repeats it (uniform control flow) and stores nothing
            const bool live = fw + g < nf;
            const int fr = min(fw + g, nf - 1);
            // pass 1 (NS = 1) straight from the samples: z[n] = xw[2n] + i xw[2n+1]
            {
                float2 v[8];
                if (shared) {
                    const int s = fr * hop;  // span index of the frame's first sample
                    const float* pe = (s & 1) ? segO + (s >> 1) : segE + (s >> 1);      // x[2n]
                    const float* po = (s & 1) ? segE + ((s + 1) >> 1) : segO + (s >> 1);  // x[2n+1]
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int n = gl + r * G;
                        v[r] = make_float2(pe[n] * hw[r][0], po[n] * hw[r][1]);
                    }
                } else {
                    const int i0 = (f0 + fr) * hop - NFFT / 2 + 2 * gl;
                    float raw[8][2];
                    bool ok[8][2];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int i = i0 + 2 * r * G + e;
                            ok[r][e] = in_view(i);
                            raw[r][e] = pcm[ok[r][e] ? d.src + (i - d.pad_left) : safe];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int i = i0 + 2 * r * G;
                        v[r] = make_float2(finish(i, ok[r][0], raw[r][0]) * hw[r][0],
                                           finish(i + 1, ok[r][1], raw[r][1]) * hw[r][1]);
                    }
                }
                dft8(v);
#pragma unroll
                for (int r = 0; r < 8; ++r) bufA[pidx(gl * 8 + r)] = v[r];
            }
            wave_sync();
            p2.run(bufA, bufB, gl);
            wave_sync();
            p3.run(bufB, bufA, gl);
            wave_sync();
            const float2* Z = bufA;                        // natural order
            const float2* zk = Z + pidx(kmin + gl);        // Z[k] of the lane's first bin
            const float2* zm = Z + pidx(NC - kmin - gl);   // its mirror (read only while k <= kmax <= NC)
            float* Pf = reinterpret_cast<float*>(bufB);    // free buffer: |X|^p of bins kmin..kmax
#pragma unroll
            for (int i = 0; i < KB; ++i) {
                const int k = kmin + gl + i * G;
                if (k <= kmax) {
                    float re, im;
                    if (k == 0 || k == NC) {
                        const float2 z0 = Z[0];  // pidx(0) == 0
                        re = (k == 0) ? z0.x + z0.y : z0.x - z0.y;
                        im = 0.f;
                    } else {
                        // (G is a multiple of 8: pidx(k) = pidx(kmin + gl) + 9 i G / 8)
                        const float2 a = zk[i * (G + G / 8)];
                        const float2 b = zm[-i * (G + G / 8)];  // Z[NC - k]; conj taken below
                        // E = (a + conj b)/2 ; O = -i (a - conj b)/2 ; X = E + W^k O
                        const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
                        const float2 O = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
                        const float2 X = cadd(E, cmul(w2r[i], O));
                        re = X.x;
                        im = X.y;
                    }
                    Pf[k - kmin] = pow_mag<PM>(re, im, power);
                }
            }
            wave_sync();
            // mel rows: a lane per band, one contiguous row of melS per frame
            float* orow = melS + ((size_t)w * T + f0 + fr) * n_mels;
            for (int m = gl; m < n_mels; m += G) {
                const int4 rw = srows[m];
                const float s = mel_row_dot<8>(svals + rw.z, Pf + (rw.x - kmin), rw.y);
                if (live) orow[m] = s;
                bmax = fmaxf(bmax, s);  // (a repeated frame repeats its values)
            }
            // the next round writes bufA first (read last before the wave_sync
            // above) and bufB only after its own first wave_sync
        }
        bmax = wave_max(bmax);
        if (lane == 0) blkmax[(size_t)w * nblk * kSmallWaves + fb * kSmallWaves + wv] = bmax;
    }  // item loop
}

// ---------------------------------------------------------------------------
// fe_stft_mel_mixed: every accepted n_fft that is not a power of two (a
// multiple of 16 with n_fft / 16 = 2^a 3^b 5^c: 400 .. 7776) -- fe_stft_mel's
// contract, arguments, item loop, staging, real split and mel rows, with the
// transform's passes taken from the plan (fe_mixed_schedule, aa_fe_plan.h)
// instead of from the template: `sched` holds the radices, 4 bits each, first
// pass lowest, 0 past the last.  Pass 1 is the radix 8 from the windowed
// samples; every later pass is MixedPass<R>::run, picked by a switch on the
// radix that is uniform over the block.
//
// NC and the passes' NB differ per size and are no multiples of the block, so
//   * the block is fe_mixed_threads() = NC/8 rounded up to whole waves (64 ..
//     512); the threads past NC/8 take no butterfly of pass 1,
//   * every pass loops j = tid; j < NB; j += NT, and every thread reaches
//     every __syncthreads().
// Twiddles: the schedule is a runtime value, so there are no per-size register
// sets; pass twiddles are read per butterfly from the tw table, whose entries
// are correctly rounded (no products of twiddles).  TWL: the block copies tw
// into LDS once (plan_fe: whenever the layout with the copy keeps the 150 KB
// bound); otherwise the reads go to global memory (L1/L2: the table is at most
// 31 KB and shared by every block).
//
// LDS banks, NB and NS being multiples of 8 but not powers of two (r = 3, 5):
//   reads   lane j reads pidx(j) + q (NB + NB/8): for one q the 32 lanes of a
//           half-wave read 32 consecutive points across 4 pads, 36 float2
//           slots over 32 (ds_read_b64: slot mod 32 per half-wave): 4 lanes
//           share a bank 2-way, whatever NB is.
//   writes  16-lane groups, slot mod 16.  NS a multiple of 16: one run of 16
//           consecutive points across 2 pads, 2 lanes 2-way.  NS = 8 mod 16
//           (8, 24, 40, 120, ...): two runs of 8, the second 9 (NS r - NS)/8
//           + 9 slots on: the runs overlap in 8 - (9 NS r / 8 mod 16) banks at
//           most, 2-way (r = 8 at NS = 8: 72 = 8 mod 16, conflict-free; r = 5:
//           45 -> 5 lanes; r = 3: 27 -> 3 lanes).  Nothing is worse than 2-way.
//   tw      (TWL) lane k reads entry q k NC/(NS r): stride 1 in the last pass,
//           the product of the later radices before; the odd factors sit late
//           in the schedule, so the early strides are odd multiples of a small
//           power of two (4800: 60, 12, 3, 1) and spread over the banks.
// None of this has been measured with counters.
// ---------------------------------------------------------------------------
template <int R>
struct MixedPass {
    // Pass::run's indexing with runtime NC, NS: butterfly j < NB = NC/R reads src[pidx(j + q NB)],
    // multiplies by tw[q k NC/(NS R)], k = j % NS, and writes dst[pidx((j / NS) NS R + k + q NS)].
    // The exponent q k NC/(NS R) <= (R - 1)(NS - 1) NB/NS < NC needs no reduction mod NC (the
    // power-of-two kernels' & (NC - 1) never acts either).
    __device__ __forceinline__ static void run(const float2* __restrict__ src, float2* __restrict__ dst,
                                               const float2* __restrict__ twp, int NC, int NS, int tid, int NT) {
        const int NB = NC / R;
        const int ts = NB / NS;                  // twiddle stride NC / (NS R)
        const float inv_ns = 1.0f / (float)NS;   // j / NS as a float product: exact below 2^21
        for (int j = tid; j < NB; j += NT) {
            const int blk = (int)(((float)j + 0.5f) * inv_ns), k = j - blk * NS;
            // NB and NS are multiples of 8: pidx(i + 8c) = pidx(i) + 9c
            const float2* s0 = src + pidx(j);
            float2 v[R], t[R - 1];
#pragma unroll
            for (int q = 1; q < R; ++q) t[q - 1] = twp[q * k * ts];
#pragma unroll
            for (int q = 0; q < R; ++q) v[q] = s0[q * (NB + NB / 8)];
#pragma unroll
            for (int q = 1; q < R; ++q) v[q] = cmul(v[q], t[q - 1]);
            if constexpr (R == 8) dft8(v);
            if constexpr (R == 5) dft5(v);
            if constexpr (R == 4) dft4(v[0], v[1], v[2], v[3]);
            if constexpr (R == 3) dft3(v[0], v[1], v[2]);
            if constexpr (R == 2) dft2(v[0], v[1]);
            float2* d0 = dst + pidx(blk * NS * R + k);
#pragma unroll
            for (int q = 0; q < R; ++q) d0[q * (NS + NS / 8)] = v[q];
        }
    }
};

template <int PM, bool TWL>
__global__ __launch_bounds__(512) void fe_stft_mel_mixed(
    const float* __restrict__ pcm, const aa_window* __restrict__ wins, const float4* __restrict__ stats,
    const float* __restrict__ hann, const float2* __restrict__ tw, const float2* __restrict__ tw2,
    const int4* __restrict__ rows, const float* __restrict__ vals, int nnz, int win_len, int hop, int T,
    int n_mels, int kmin, int kmax, int normalize, float power, int nblk, int n_items,
    float* __restrict__ melS, float* __restrict__ blkmax, int n_fft, unsigned sched) {
    const int NC = n_fft / 2;
    const int N8 = NC / 8;                 // butterflies of pass 1
    const int NT = blockDim.x;             // fe_mixed_threads(n_fft) >= N8
    constexpr int KREG = 4;  // post-processing bins per thread with register twiddles
    extern __shared__ float lds[];
    const FeLdsGeneric L(n_fft, hop, n_mels, nnz, TWL ? NC : 0);
    float* seg = lds;
    float2* bufA = reinterpret_cast<float2*>(seg + L.seg);
    float2* bufB = bufA + L.buf;
    float2* stw = bufB + L.buf;            // the block's copy of tw (TWL)
    float* melT = reinterpret_cast<float*>(stw + L.tw);  // [n_mels][kFpb] staging
    int4* srows = reinterpret_cast<int4*>(melT + L.melT);
    float* svals = reinterpret_cast<float*>(srows + L.rows);

    // --- per-thread constants, loaded once per block ---
    const int tid = threadIdx.x;
    const bool p1 = tid < N8;              // the thread has a butterfly in pass 1
    float hw[8][2];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = min(tid, N8 - 1) + r * N8;
        const float2 h = reinterpret_cast<const float2*>(hann)[n];
        hw[r][0] = h.x;
        hw[r][1] = h.y;
    }
    float2 w2r[KREG];
#pragma unroll
    for (int i = 0; i < KREG; ++i) {
        w2r[i] = tw2[min(kmin + tid + i * NT, kmax)];
    }
    if constexpr (TWL)
        for (int i = tid; i < NC; i += NT) stw[i] = tw[i];
    const float2* twp = TWL ? stw : tw;
    for (int i = tid; i < n_mels; i += NT) srows[i] = rows[i];
    for (int i = tid; i < nnz; i += NT) svals[i] = vals[i];

    __syncthreads();
    // persistent loop over (window, frame block) items
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int w = item / nblk;
    const int fb = item - w * nblk;
    const int f0 = fb * kFpb;
    const int nf = min(kFpb, T - f0);
    const int seg_len = (nf - 1) * hop + n_fft;
    // --- normalisation constants (normalize_data, :203-208) ---
    const aa_window d = wins[w];
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int s = 0; s < kStatSplit; ++s) {
        float4 st = stats[w * kStatSplit + s];
        lo = fminf(lo, st.x);
        hi = fmaxf(hi, st.y);
    }
    const float scale = __fsub_rn(hi, lo);  // == max(x - min) (monotone rounding)
    const float inv = __fdiv_rn(1.f, scale);

    // --- overlapped segment -> LDS, normalised; loads issued in batches of
    // SEGU per thread before any is consumed ---
    const int base = f0 * hop - n_fft / 2;  // window index of seg[0]
    constexpr int SEGU = 8;
    const long long safe = d.n_valid > 0 ? d.src : 0;  // any in-bounds sample
    for (int q0 = 0; q0 < seg_len; q0 += SEGU * NT) {
        float raw[SEGU];
        bool ok[SEGU];
#pragma unroll
        for (int u = 0; u < SEGU; ++u) {  // unconditional loads from clamped addresses
            const int q = q0 + u * NT + tid;
            const int i = base + q;
            const int rel = i - d.pad_left;
            ok[u] = q < seg_len && i >= 0 && i < win_len && rel >= 0 && rel < d.n_valid;
            raw[u] = pcm[ok[u] ? d.src + rel : safe];
        }
#pragma unroll
        for (int u = 0; u < SEGU; ++u) {
            const int q = q0 + u * NT + tid;
            const int i = base + q;
            if (q < seg_len) {
                float v = 0.f;
                if (i >= 0 && i < win_len) {
                    v = ok[u] ? raw[u] : 0.f;
                    if (normalize) v = normalize_sample(v, lo, scale, inv);
                }
                seg[q] = v;
            }
        }
    }
    __syncthreads();

    float bmax = 0.f;
    for (int f = 0; f < nf; ++f) {
        // pass 1 (NS = 1) straight from the segment: z[n] = xw[2n] + i xw[2n+1]
        if (p1) {
            const float* x = seg + f * hop;
            float2 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int n = tid + r * N8;
                v[r] = make_float2(x[2 * n] * hw[r][0], x[2 * n + 1] * hw[r][1]);
            }
            dft8(v);
#pragma unroll
            for (int r = 0; r < 8; ++r) bufA[pidx(tid * 8 + r)] = v[r];
        }
        __syncthreads();
        // the scheduled passes, ping-pong; the result ends in `src`
        float2 *src = bufA, *dst = bufB;
        int NS = 8;
        for (unsigned sc = sched >> 4; sc != 0; sc >>= 4) {
            const int R = sc & 15;
            switch (R) {  // uniform over the block
                case 8: MixedPass<8>::run(src, dst, twp, NC, NS, tid, NT); break;
                case 5: MixedPass<5>::run(src, dst, twp, NC, NS, tid, NT); break;
                case 4: MixedPass<4>::run(src, dst, twp, NC, NS, tid, NT); break;
                case 3: MixedPass<3>::run(src, dst, twp, NC, NS, tid, NT); break;
                default: MixedPass<2>::run(src, dst, twp, NC, NS, tid, NT); break;
            }
            NS *= R;
            float2* t = src; src = dst; dst = t;
            __syncthreads();
        }
        const float2* Z = src;             // natural order
        float* Pf = reinterpret_cast<float*>(dst);  // free scratch for |X|^p
        for (int i = 0; kmin + tid + i * NT <= kmax; ++i) {
            const int k = kmin + tid + i * NT;
            float re, im;
            if (k == 0 || k == NC) {
                const float2 z0 = Z[0];  // pidx(0) == 0
                re = (k == 0) ? z0.x + z0.y : z0.x - z0.y;
                im = 0.f;
            } else {
                const float2 a = Z[pidx(k)];
                const float2 b = Z[pidx(NC - k)];  // conj taken below
                // E = (a + conj b)/2 ; O = -i (a - conj b)/2 ; X = E + W^k O
                const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
                const float2 O = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
                float2 wk;
                if (i < KREG) {
                    wk = w2r[0];
#pragma unroll
                    for (int q = 1; q < KREG; ++q) if (i == q) wk = w2r[q];
                } else {
                    wk = tw2[k];
                }
                const float2 X = cadd(E, cmul(wk, O));
                re = X.x;
                im = X.y;
            }
            Pf[k - kmin] = pow_mag<PM>(re, im, power);
        }
        __syncthreads();
        for (int m = tid; m < n_mels; m += NT) {
            const int4 rw = srows[m];
            const float s = mel_row_dot<16>(svals + rw.z, Pf + (rw.x - kmin), rw.y);
            melT[m * kFpb + f] = s;
            bmax = fmaxf(bmax, s);
        }
        __syncthreads();  // P / buffers reused by the next frame
    }
    // staged [n_mels][nf] tile -> melS[w][m][f0 .. f0 + nf)
    const float inv_nm = 1.0f / (float)n_mels;  // exact row below 2^21 (as in fe_db)
    for (int idx = tid; idx < nf * n_mels; idx += NT) {  // frame-major rows
        const int f = (int)(((float)idx + 0.5f) * inv_nm), m = idx - f * n_mels;
        melS[((size_t)w * T + f0 + f) * n_mels + m] = melT[m * kFpb + f];
    }
    // item max -> blkmax[w][fb]
    __shared__ float red[512 / 64];
    bmax = wave_max(bmax);
    if ((tid & 63) == 0) red[tid >> 6] = bmax;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < NT / 64; ++k) bmax = fmaxf(bmax, red[k]);
        blkmax[w * nblk + fb] = bmax;
    }
    }  // item loop
}

}  // namespace aa
