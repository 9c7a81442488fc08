// Planner of the log-mel front end: aa_fe_config + dense filterbank -> every
// number and host image the launches need, host only (no HIP call), so a plan
// can be made and inspected on a machine without a GPU (aa_fe_plan /
// aa_fe_plan_info / aa_fe_plan_image).  aa_fe_create uploads the images and
// releases them; aa_fe_run launches what was chosen here.
// The LDS layouts of fe_stft_mel, fe_stft_mel_mixed and fe_stft_mel_small are
// stated here once (FeLdsGeneric, FeLdsSmall): the kernel steps its pointers
// through the regions, the planner adds them up.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "aa_wavefft.h"

namespace aa {

constexpr int kStatSplit = 16;  // stats blocks per window
constexpr int kFpb = 6;         // frames per fe_stft_mel block

// fe_stft_mel_small (aa_fe_stft.h)
constexpr int kSmallWaves = 4;                    // waves per block
constexpr int kSmallSeg = 3072;                   // shared PCM span, samples
constexpr int kSmallHalf = kSmallSeg / 2 + 16;    // words per parity half (16 mod 32)
constexpr int kSmallBuf = 64 * 9;                 // float2 per wave buffer: 512 points + pidx padding
__host__ __device__ constexpr int fe_small_fpb(int n_fft) { return n_fft == 1024 ? 8 : 16; }
__host__ __device__ constexpr bool fe_small_shared(int n_fft, int hop) {
    return (long long)(fe_small_fpb(n_fft) - 1) * hop + n_fft <= kSmallSeg;
}

// fe_stft_mel_4096 (aa_fe_wave4096.h)
constexpr int kWpb = 8;  // waves per block (2 blocks per CU)
// band slots of the wave-per-frame kernel's CSR image: whole rounds of 64 lanes
__host__ __device__ constexpr int fe_mel_slots(int n_mels) { return (n_mels + 63) / 64 * 64; }

// ---- LDS layouts: the regions of the dynamic LDS in order, each with its length in its
// own element type.  The kernel steps its pointers through them, bytes() adds them up. ----
// fe_stft_mel: segment (float) | bufA, bufB (float2) | melT [n_mels][kFpb] (float) | CSR rows (int4) | values (float)
// fe_stft_mel_mixed: the same, with its copy of the tw table (float2, n_fft/2 entries, or none) after bufB
struct FeLdsGeneric {
    int seg, buf, tw, melT, rows, vals;
    __host__ __device__ FeLdsGeneric(int n_fft, int hop, int n_mels, int nnz, int tw_entries = 0)
        : seg(((kFpb - 1) * hop + n_fft + 3) & ~3), buf(n_fft / 2 + n_fft / 16), tw(tw_entries),
          melT((n_mels * kFpb + 3) & ~3), rows(n_mels), vals(nnz > 1 ? nnz : 1) {}
    size_t bytes() const {
        return 4 * ((size_t)seg + 4 * (size_t)buf + 2 * (size_t)tw + melT + 4 * (size_t)rows + vals);
    }
};
// fe_stft_mel_small (no term in the hop): even, odd samples (float) | wave buffers (float2) | CSR rows (int4) | values
struct FeLdsSmall {
    int half = kSmallHalf, bufs = kSmallWaves * 2 * kSmallBuf, rows, vals;
    __host__ __device__ FeLdsSmall(int n_mels, int nnz) : rows(n_mels), vals(nnz > 1 ? nnz : 1) {}
    size_t bytes() const { return 4 * (2 * (size_t)half + 2 * (size_t)bufs + 4 * (size_t)rows + vals); }
};
// fe_stft_mel_4096, in bytes: CSR image (rows | values, as uploaded) | a kHalf-float2 buffer per wave
static inline size_t fe_lds_bytes4096(int cimg_bytes) { return (size_t)cimg_bytes + sizeof(float2) * (size_t)kWpb * kHalf; }

enum FeKernel {
    FE_K_SMALL = AA_FE_K_SMALL, FE_K_WAVE4096 = AA_FE_K_WAVE4096, FE_K_GENERIC = AA_FE_K_GENERIC,
    FE_K_MIXED = AA_FE_K_MIXED
};

constexpr int kMaxPasses = 8;  // Stockham passes of a schedule (7 at n_fft 7776 = 2 * 8 * 2 * 3^5)

// threads of an fe_stft_mel_mixed block: a thread per radix-8 butterfly of pass 1, in whole waves
__host__ __device__ constexpr int fe_mixed_threads(int n_fft) { return (n_fft / 16 + 63) / 64 * 64; }

// n_fft of fe_stft_mel_mixed: a multiple of 16 whose sixteenth has no prime factor but 2, 3 and 5
static bool fe_smooth16(int n) {
    if (n <= 0 || n % 16) return false;
    int m = n / 16;
    for (int f : {2, 3, 5})
        while (m % f == 0) m /= f;
    return m == 1;
}

// Pass schedule of the NC = n_fft/2 point transform of fe_stft_mel_mixed: radices r_1 .. r_P with
// product NC, in this fixed order: the radix 8 of pass 1 (from the samples), every further 8, the
// 5s, one 4, the 3s, one 2 (NC/8 = 2^a 3^b 5^c: a/3 eights, a 4 when a % 3 == 2, a 2 when
// a % 3 == 1).  The sub-transform size before a pass, NS = the product of the earlier radices, is
// a multiple of 8 from pass 2 on.  Returns P (<= kMaxPasses inside 256..8192).
static int fe_mixed_schedule(int n_fft, int* radix) {
    int m = n_fft / 16, a = 0, b = 0, c = 0, n = 0;
    while (m % 2 == 0) { m /= 2; ++a; }
    while (m % 3 == 0) { m /= 3; ++b; }
    while (m % 5 == 0) { m /= 5; ++c; }
    radix[n++] = 8;
    for (int i = 0; i < a / 3; ++i) radix[n++] = 8;
    for (int i = 0; i < c; ++i) radix[n++] = 5;
    if (a % 3 == 2) radix[n++] = 4;
    for (int i = 0; i < b; ++i) radix[n++] = 3;
    if (a % 3 == 1) radix[n++] = 2;
    return n;
}

struct FePlan {
    aa_fe_config cfg;
    int T = 0;         // frames per window
    int kmin = 0, kmax = 0;  // first and last filterbank bin with a nonzero weight
    int nnz = 0;
    FeKernel kernel = FE_K_GENERIC;
    int nblk = 0;      // FE_K_SMALL / FE_K_GENERIC: frame blocks (grid items) per window
    int nparts = 0;    // per-window partial maxima that fe_db reads
    int per_cu = 1;    // blocks resident together on a CU
    size_t lds_bytes = 0;  // dynamic LDS of the chosen kernel
    int n_pass = 0;    // Stockham passes of the chosen kernel and their radices (aa_fe_plan_passes);
    int radix[kMaxPasses] = {};  // FE_K_MIXED runs this schedule, the others have it built in
    bool tw_lds = false;  // FE_K_MIXED: the block keeps a copy of tw in LDS (it fits the bound)
    // host images, released once aa_fe_create has uploaded them
    std::vector<float> h_win;    // periodic Hann, f32 [n_fft]
    std::vector<float2> h_tw;    // exp(-2 pi i m / Nc), m < Nc
    std::vector<float2> h_tw2;   // exp(-2 pi i k / n_fft), k <= Nc
    std::vector<int4> h_rows;    // per band: (first bin, count, value offset, 0)
    std::vector<float> h_vals;   // CSR values
    std::vector<char> h_cimg;    // fe_stft_mel_4096 CSR image (rows | values), 1-KiB padded
    bool uploaded = false;
    float *d_win = nullptr, *d_vals = nullptr;  // their device copies
    float2 *d_tw = nullptr, *d_tw2 = nullptr;
    int4* d_rows = nullptr;
    char* d_cimg = nullptr; int cimg_bytes = 0;
    StageTimer timer;  // HIP events around the launches in timer.mask

    // persistent grid of the stft launch: the blocks resident together on 256
    // CUs; the wave-per-frame kernel takes a multiple of 8 (its XCD renumbering)
    int grid(int n_win) const {
        if (kernel == FE_K_WAVE4096) return (std::min((T * n_win + kWpb - 1) / kWpb, 256 * per_cu) + 7) & ~7;
        return std::min(nblk * n_win, 256 * per_cu);
    }
};

// The one kernel choice.  n_fft 256, 512 and 1024 run fe_stft_mel_small; the wave-per-frame
// kernel covers n_fft 4096 whenever the kept band fits the per-wave buffer (15 bins per lane):
// inside X[2..1022] (Hann neighbours in range and clear of the bins -1..1 that the folded
// normalisation offset touches), padded rows (+3 bins) inside the 15 x 64 power slots.
// Every accepted n_fft that is not a power of two runs fe_stft_mel_mixed.
static FeKernel choose_kernel(int n_fft, int kmin, int kmax) {
    if (n_fft & (n_fft - 1)) return FE_K_MIXED;
    if (n_fft <= 1024) return FE_K_SMALL;
    const bool wave = n_fft == 4096 && kmin >= 2 && kmax <= 1022 && kmin + 64 * (kHalf / 64 - 1) < kHalf &&
                      kmax - kmin + 1 + 3 <= (kHalf / 64 - 1) * 64;
    return wave ? FE_K_WAVE4096 : FE_K_GENERIC;
}

static const char* fe_kernel_name(FeKernel k) {
    return k == FE_K_SMALL ? "fe_stft_mel_small" : k == FE_K_WAVE4096 ? "fe_stft_mel_4096"
           : k == FE_K_MIXED ? "fe_stft_mel_mixed" : "fe_stft_mel";
}

// CSR image of the wave-per-frame kernel, byte-identical to its LDS
// region: rows (first bin, padded length, value offset) | values, each
// row zero-padded to whole float4s (value offsets 16-B aligned)
// Rows sit in fe_mel_slots() slots, slot i served by lane i % 64 (the
// .w field names the band): the longest row first goes to the
// least-loaded lane with a free slot, so the lanes' loop trip counts
// stay close (round-robin rows gave lane 31 the 3 widest-spaced rows:
// 52 bins against a mean of 32).  Empty slots have length 0.
static std::vector<char> fe_cimg4096(const std::vector<int4>& rows, const std::vector<float>& vals, int kmin) {
    const int nslot = fe_mel_slots((int)rows.size());
    // (an empty slot's first bin: kmin + 3, so that the grouped loads of an
    // empty row, kMelG, read inside the wave's power buffer)
    std::vector<int4> prow(nslot, make_int4(kmin + 3, 0, 0, -1));
    std::vector<float> pval;
    std::vector<int> order(rows.size());
    for (size_t m = 0; m < rows.size(); ++m) order[m] = (int)m;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rows[a].y > rows[b].y; });
    std::vector<int> load(64, 0), used(64, 0);
    for (int m : order) {
        int best = -1;
        for (int l = 0; l < 64; ++l)
            if (used[l] < nslot / 64 && (best < 0 || load[l] < load[best])) best = l;
        const int len = (rows[m].y + 3) & ~3, pad = len - rows[m].y;
        // (the kernel keeps the band power reversed: values are stored last
        // bin first, zero-padded at the front, so a row reads one ascending run)
        prow[best + 64 * used[best]] = make_int4(rows[m].x, len, (int)pval.size(), m);
        load[best] += len;
        ++used[best];
        for (int i = 0; i < len; ++i) pval.push_back(i < pad ? 0.f : vals[rows[m].z + rows[m].y - 1 - (i - pad)]);
    }
    const size_t raw = sizeof(int4) * prow.size() + sizeof(float) * pval.size();
    std::vector<char> img((raw + 1023) / 1024 * 1024, 0);
    memcpy(img.data(), prow.data(), sizeof(int4) * prow.size());
    if (!pval.empty()) memcpy(img.data() + sizeof(int4) * prow.size(), pval.data(), sizeof(float) * pval.size());
    return img;
}

// The whole plan; every refusal of aa_fe_create / aa_fe_plan is decided here.
static int plan_fe(const aa_fe_config* cfg, const float* melfb, FePlan* p) {
    AA_CHECK(cfg && melfb && p, AA_ERR_INVALID, "aa_fe_create: null argument");
    const int n = cfg->n_fft;
    AA_CHECK(n >= 256 && n <= 8192 && ((n & (n - 1)) == 0 || fe_smooth16(n)), AA_ERR_UNSUPPORTED,
             "aa_fe_create: n_fft %d not supported (power of two, or a multiple of 16 with factors 2, 3, 5, 256..8192)",
             n);
    AA_CHECK(cfg->hop > 0 && cfg->win_len > 0 && cfg->n_mels > 0 && cfg->channels >= 1 &&
                 (cfg->out_f16 == 0 || cfg->out_f16 == 1),
             AA_ERR_INVALID, "aa_fe_create: bad sizes");
    p->cfg = *cfg;
    p->T = 1 + cfg->win_len / cfg->hop;

    const int nbins = n / 2 + 1;
    // CSR of the dense filterbank (rows are contiguous triangles; keep
    // [first nonzero, last nonzero] per row)
    std::vector<int4>& rows = p->h_rows;
    std::vector<float>& vals = p->h_vals;
    rows.resize(cfg->n_mels);
    int kmin = nbins, kmax = 0;
    for (int m = 0; m < cfg->n_mels; ++m) {
        const float* r = melfb + (size_t)m * nbins;
        int a = -1, b = -1;
        for (int k = 0; k < nbins; ++k)
            if (r[k] != 0.f) { if (a < 0) a = k; b = k; }
        if (a < 0) { a = 0; b = -1; }
        rows[m] = make_int4(a, b - a + 1, (int)vals.size(), 0);
        for (int k = a; k <= b; ++k) vals.push_back(r[k]);
        if (b >= a) { kmin = std::min(kmin, a); kmax = std::max(kmax, b); }
    }
    if (kmax < kmin) { kmin = 0; kmax = 0; }
    for (auto& r : rows) if (r.y == 0) r.x = kmin;
    p->kmin = kmin;
    p->kmax = kmax;
    p->nnz = (int)vals.size();
    if (vals.empty()) vals.push_back(0.f);

    p->kernel = choose_kernel(n, kmin, kmax);
    // (from 2048 up the hop is held to fe_stft_mel's segment whichever kernel runs; fe_stft_mel_small
    // takes any hop: past its shared span, frames load their own samples.  FE_K_WAVE4096's own bytes are
    // not bounded here: a dense filterbank can pass this and be refused at launch, launch_stft.)
    size_t lds_generic = FeLdsGeneric(n, cfg->hop, cfg->n_mels, p->nnz).bytes();
    const size_t lds_small = FeLdsSmall(cfg->n_mels, p->nnz).bytes();
    if (p->kernel == FE_K_MIXED) {
        // fe_stft_mel_mixed reads its pass twiddles from the tw table: from a copy in LDS when the
        // layout with it stays inside the bound, from global memory otherwise (the long transforms
        // at long hops: 7680 / 1024 / 160 bands is 141 KB without the 30 KB copy)
        const size_t with_tw = FeLdsGeneric(n, cfg->hop, cfg->n_mels, p->nnz, n / 2).bytes();
        p->tw_lds = with_tw <= 150 * 1024;
        if (p->tw_lds) lds_generic = with_tw;
    }
    if (p->kernel == FE_K_SMALL)
        AA_CHECK(lds_small <= 160 * 1024, AA_ERR_UNSUPPORTED,
                 "aa_fe_create: filterbank (%d bands, %d weights) too large for the LDS", cfg->n_mels, p->nnz);
    else
        AA_CHECK(lds_generic <= 150 * 1024, AA_ERR_UNSUPPORTED, "aa_fe_create: hop %d too large for the LDS segment",
                 cfg->hop);
    if (n == 4096) {  // (built and uploaded whichever 4096 kernel runs)
        p->h_cimg = fe_cimg4096(rows, vals, kmin);
        p->cimg_bytes = (int)p->h_cimg.size();
    }
    const bool small = p->kernel == FE_K_SMALL, wave = p->kernel == FE_K_WAVE4096;
    const int fpb = small ? fe_small_fpb(n) : kFpb;
    p->nblk = (p->T + fpb - 1) / fpb;
    // partial maxima: one per frame, per wave of each frame block, or per frame block
    p->nparts = wave ? p->T : small ? p->nblk * kSmallWaves : p->nblk;
    p->lds_bytes = wave ? fe_lds_bytes4096(p->cimg_bytes) : small ? lds_small : lds_generic;
    // blocks per CU by LDS (static LDS comes on top); the wave-per-frame kernel
    // at most 2 (1 measured -1.5 % on the two-stream step, profiles/r05/ab_fe_per_cu.txt)
    p->per_cu = std::max(1, wave ? std::min(2, (int)((160 * 1024) / p->lds_bytes))
                                 : (int)((160 * 1024) / (p->lds_bytes + 256)));

    // the passes: fe_stft_mel_mixed's schedule; the built-in ones of the other kernels (fe_stft_mel_4096:
    // its two register DFT-32s as 8 x 4 each, then the radix 2 across the lane pair)
    if (p->kernel == FE_K_MIXED) p->n_pass = fe_mixed_schedule(n, p->radix);
    else if (wave) { const int r[5] = {8, 4, 8, 4, 2}; std::copy(r, r + 5, p->radix); p->n_pass = 5; }
    else if (small) { const int r[3] = {8, 8, n / 128}; std::copy(r, r + 3, p->radix); p->n_pass = 3; }
    else { const int r[4] = {8, 8, 8, n / 1024}; std::copy(r, r + 4, p->radix); p->n_pass = 4; }

    const int nc = n / 2;
    p->h_win.resize(n);
    for (int i = 0; i < n; ++i) p->h_win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / n));
    p->h_tw.resize(nc);
    p->h_tw2.resize(nc + 1);
    for (int m = 0; m < nc; ++m) {
        const double a = -2.0 * M_PI * m / nc;
        p->h_tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    for (int k = 0; k <= nc; ++k) {
        const double a = -2.0 * M_PI * k / n;
        p->h_tw2[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return AA_OK;
}

}  // namespace aa
