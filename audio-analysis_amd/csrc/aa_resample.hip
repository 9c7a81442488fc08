// Rational polyphase resampling to the 48 kHz the reference analyses at.
//
// load_recording (reference src/identify_tracks.py:49-62) resamples any other
// rate with librosa.resample(res_type="soxr_hq"): libsoxr's high-quality
// recipe -- linear phase, 20-bit precision (stop band >= 126 dB down), pass
// band flat to 0.913 and stop band from 1.0 of the lower rate's Nyquist.
// libsoxr is not in this image; aa_amd/resample.py designs a filter to that
// published specification (Kaiser-windowed sinc on the L-times upsampled
// grid) and this kernel applies it.  Output sample m sits at time m / fs_out,
// i.e. grid index m M; with the filter's centre tap at half:
//   q = m M + half,  k0 = floor(q / L),  r = q - k0 L,
//   y[m] = sum_t bank[r][t] x[k0 - t]     (bank[r][t] = h[r + t L], x = 0 outside)
// One thread per output sample; the L x taps bank and the input window a
// block needs are served from L1/L2 (the kernel is FMA-bound: ~190 taps per
// output at 44.1 -> 48 kHz).
#include "aa_common.h"

namespace aa {

__global__ __launch_bounds__(256) void resample_poly(const float* __restrict__ x, long long n_in,
                                                     const float* __restrict__ bank, int L, int M, int taps,
                                                     int half, float* __restrict__ y, long long n_out) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_out) return;
    const long long q = m * M + half;
    const long long k0 = q / L;
    const int r = (int)(q - k0 * L);
    const float* h = bank + (size_t)r * taps;
    float acc = 0.f;
    if (k0 - (taps - 1) >= 0 && k0 < n_in) {  // interior: no bounds checks
        const float* xp = x + k0;
        for (int t = 0; t < taps; ++t) acc = fmaf(h[t], xp[-t], acc);
    } else {
        for (int t = 0; t < taps; ++t) {
            const long long k = k0 - t;
            if (k >= 0 && k < n_in) acc = fmaf(h[t], x[k], acc);
        }
    }
    y[m] = acc;
}

// ---- a batch of recordings in one launch ----------------------------------
// The batched index path (aa_amd/ci_batch.py) brings every recording of a
// batch that shares an input rate to 16 kHz with one launch.  Block
// (blockIdx.y, blockIdx.x) is output tile blockIdx.x (RS_TILE outputs) of
// segment blockIdx.y; the grid is as wide as the longest segment and a block
// past its segment's end leaves at once.  The arithmetic per output is
// resample_poly's, term by term (one accumulator, fmaf in tap order), so the
// words are its words; what changes is where the operands come from:
//   * the tile's input span [k0(first) - taps + 1, k0(last)] -- at most
//     ceil((RS_TILE - 1) M / L) + taps samples -- is staged once in LDS, an
//     int16 source widened and downmixed on the way (pcm_s16_frame_to_f32, the
//     expression of aa_pcm_s16_to_f32), so the f32 signal at the file's rate
//     never exists in memory.  The span is zero-filled outside [0, n_in).
//     For samples that come from int16 (never -0.0) a zero-filled term
//     fmaf(h, +0, acc) leaves every acc unchanged (acc starts +0 and an exact
//     zero sum rounds to +0), so the edges could run the plain loop; an f32
//     source may hold -0.0 or products that underflow to it, and then acc can
//     be -0.0, which fmaf(h, +0, -0.0) would turn into +0.0.  So an output
//     whose taps leave [0, n_in) skips those terms exactly as resample_poly
//     does -- only the first and last tiles of a segment hold such outputs;
//   * L == 1 (48, 96 kHz -> 16 kHz): every lane uses row 0, tap t is wave
//     uniform and comes through the scalar cache;
//   * L taps <= RS_BANK_LDS floats (L = 2: 8, 32, 24 kHz): the bank is staged
//     in LDS too; lanes of one phase read one word (broadcast);
//   * otherwise (the 160- and 320-row banks of 44.1 / 22.05 / 88.2 kHz): row
//     r per thread from global memory (L2: the 335 KB bank is shared by all
//     blocks).
// LDS reads of the span: lane j reads word floor(((m0 + j) M + half) / L) - t,
// a stride of M / L words across lanes.  ds_read_b32 banks are word mod 32
// within each 32-lane half.  Counting the distinct words per bank of every
// half-wave of a tile: M / L = 3 (48 kHz) and 1/2 (8 kHz, lane pairs share a
// word) are conflict-free; 6 (96 kHz), 2 (32 kHz), 441/160 (44.1 kHz) and
// 441/320 (22.05 kHz) are 2-way (lanes j and j + 16 meet where the stride is
// even; the 441 ratios advance about 88 words per half-wave over 32 banks).
// A padded index would cost an add and a shift per tap in a loop that is one
// ds_read and one fmaf; the 2-way ratios are left as they are.
constexpr int RS_TILE = 256;
constexpr int RS_BANK_LDS = 4096;        // floats of bank kept in LDS (16 KiB)
constexpr size_t RS_LDS_MAX = 64 * 1024;  // static + dynamic LDS a launch may take without an attribute

template <int BANK>  // 0: L == 1, uniform taps; 1: bank in LDS; 2: bank rows from global memory
__global__ __launch_bounds__(RS_TILE) void resample_batch(const short* __restrict__ s16, long long n_s16,
                                                          const float* __restrict__ f32, long long n_f32,
                                                          const aa_rs_segment* __restrict__ segs,
                                                          const float* __restrict__ bank, int L, int M, int taps,
                                                          int half, int span_max, float* __restrict__ y,
                                                          long long n_y) {
    extern __shared__ float lds[];
    float* xs = lds;                 // [span_max]
    float* hs = lds + span_max;      // [L * taps] when BANK == 1
    const aa_rs_segment sg = segs[blockIdx.y];
    const long long m0 = (long long)blockIdx.x * RS_TILE;
    if (m0 >= sg.n_out) return;
    // a segment that leaves its buffers is skipped whole (nothing read or
    // written): the table is device memory the host call cannot check
    const bool is16 = sg.kind == AA_RS_S16;
    const long long ch = is16 ? sg.channels : 1;
    if ((!is16 && sg.kind != AA_RS_F32) || ch < 1 || ch > 8 || sg.n_in < 0 || sg.src_off < 0 || sg.dst_off < 0 ||
        sg.n_in > (1LL << 40) || sg.n_out > (1LL << 40))
        return;
    if (sg.src_off + sg.n_in * ch > (is16 ? n_s16 : n_f32) || sg.dst_off + sg.n_out > n_y) return;
    const long long m_last = min(m0 + RS_TILE - 1, sg.n_out - 1);
    const long long base = (m0 * M + half) / L - (taps - 1);
    const int span = (int)((m_last * M + half) / L - base) + 1;
    if (span > span_max) return;  // (cannot happen: span_max is the bound of this very expression)
    if (is16) {
        const short* src = s16 + sg.src_off;
        for (int i = threadIdx.x; i < span; i += RS_TILE) {
            const long long k = base + i;
            xs[i] = (k >= 0 && k < sg.n_in) ? pcm_s16_frame_to_f32(src + k * ch, (int)ch) : 0.f;
        }
    } else {
        const float* src = f32 + sg.src_off;
        for (int i = threadIdx.x; i < span; i += RS_TILE) {
            const long long k = base + i;
            xs[i] = (k >= 0 && k < sg.n_in) ? src[k] : 0.f;
        }
    }
    if (BANK == 1)
        for (int i = threadIdx.x; i < L * taps; i += RS_TILE) hs[i] = bank[i];
    __syncthreads();
    const long long m = m0 + threadIdx.x;
    if (m >= sg.n_out) return;
    const long long q = m * M + half;
    const long long k0 = q / L;
    const int r = (int)(q - k0 * L);
    const float* h = BANK == 0 ? bank : (BANK == 1 ? hs : bank) + (size_t)r * taps;
    const float* xp = xs + (k0 - base);  // xp[-t] = x[k0 - t]
    float acc = 0.f;
    if (k0 - (taps - 1) >= 0 && k0 < sg.n_in) {  // interior: every tap inside the recording
#pragma unroll 8
        for (int t = 0; t < taps; ++t) acc = fmaf(h[t], xp[-t], acc);
    } else {
        for (int t = 0; t < taps; ++t) {
            const long long k = k0 - t;
            if (k >= 0 && k < sg.n_in) acc = fmaf(h[t], xp[-t], acc);
        }
    }
    y[sg.dst_off + m] = acc;
}

}  // namespace aa

extern "C" int aa_resample_poly(const float* x, int64_t n_in, const float* bank, int32_t L, int32_t M, int32_t taps,
                                int32_t half, float* y, int64_t n_out, void* stream) {
    AA_CHECK(x && bank && y, AA_ERR_INVALID, "aa_resample_poly: null argument");
    AA_CHECK(n_in >= 0 && n_out >= 0 && L >= 1 && M >= 1 && taps >= 1 && half >= 0 && half < (int64_t)L * taps,
             AA_ERR_INVALID, "aa_resample_poly: bad sizes");
    if (n_out == 0) return AA_OK;
    hipLaunchKernelGGL(aa::resample_poly, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, (long long)n_in, bank, L, M, taps, half, y,
                       (long long)n_out);
    AA_LAUNCH_CHECK();
    return AA_OK;
}

extern "C" int aa_resample_batch(const int16_t* src_s16, int64_t n_s16, const float* src_f32, int64_t n_f32,
                                 const aa_rs_segment* segs_dev, int32_t n_seg, int64_t max_n_out, const float* bank,
                                 int32_t L, int32_t M, int32_t taps, int32_t half, float* y, int64_t n_y,
                                 void* stream) {
    AA_CHECK(segs_dev, AA_ERR_INVALID, "aa_resample_batch: segs_dev is null");
    AA_CHECK(bank, AA_ERR_INVALID, "aa_resample_batch: bank is null");
    AA_CHECK(y, AA_ERR_INVALID, "aa_resample_batch: y is null");
    AA_CHECK(n_s16 >= 0 && (src_s16 || n_s16 == 0), AA_ERR_INVALID,
             "aa_resample_batch: src_s16 is null or n_s16 negative (%lld)", (long long)n_s16);
    AA_CHECK(n_f32 >= 0 && (src_f32 || n_f32 == 0), AA_ERR_INVALID,
             "aa_resample_batch: src_f32 is null or n_f32 negative (%lld)", (long long)n_f32);
    AA_CHECK(n_y >= 0, AA_ERR_INVALID, "aa_resample_batch: n_y negative (%lld)", (long long)n_y);
    AA_CHECK(n_seg >= 0 && n_seg <= AA_CI_MAX_REC, AA_ERR_INVALID, "aa_resample_batch: n_seg %d outside 0..%d",
             n_seg, AA_CI_MAX_REC);
    AA_CHECK(max_n_out >= 0 && max_n_out <= n_y, AA_ERR_INVALID,
             "aa_resample_batch: max_n_out %lld outside 0..n_y", (long long)max_n_out);
    AA_CHECK(L >= 1 && M >= 1 && taps >= 1 && L <= 65536 && M <= 65536, AA_ERR_INVALID,
             "aa_resample_batch: L %d, M %d (1..65536), taps %d (>= 1)", L, M, taps);
    AA_CHECK(half >= 0 && half < (int64_t)L * taps, AA_ERR_INVALID, "aa_resample_batch: half %d outside 0..L taps",
             half);
    const int64_t span_max = ((int64_t)(aa::RS_TILE - 1) * M + L - 1) / L + taps;
    const int variant = L == 1 ? 0 : ((int64_t)L * taps <= aa::RS_BANK_LDS ? 1 : 2);
    const size_t lds = (size_t)(span_max + (variant == 1 ? (int64_t)L * taps : 0)) * sizeof(float);
    AA_CHECK(lds <= aa::RS_LDS_MAX, AA_ERR_INVALID, "aa_resample_batch: taps %d, M / L %d / %d need %zu bytes of LDS",
             taps, M, L, lds);
    const int64_t tiles = (max_n_out + aa::RS_TILE - 1) / aa::RS_TILE;
    AA_CHECK(tiles <= 0x7fffffffLL, AA_ERR_INVALID, "aa_resample_batch: max_n_out %lld too large",
             (long long)max_n_out);
    if (n_seg == 0 || max_n_out == 0) return AA_OK;
    const dim3 grid((unsigned)tiles, (unsigned)n_seg);
    const auto st = static_cast<hipStream_t>(stream);
    const short* s16 = reinterpret_cast<const short*>(src_s16);
#define AA_RS_LAUNCH(V)                                                                                        \
    hipLaunchKernelGGL(aa::resample_batch<V>, grid, dim3(aa::RS_TILE), lds, st, s16, (long long)n_s16, src_f32, \
                       (long long)n_f32, segs_dev, bank, L, M, taps, half, (int)span_max, y, (long long)n_y)
    if (variant == 0)
        AA_RS_LAUNCH(0);
    else if (variant == 1)
        AA_RS_LAUNCH(1);
    else
        AA_RS_LAUNCH(2);
#undef AA_RS_LAUNCH
    AA_LAUNCH_CHECK();
    return AA_OK;
}
