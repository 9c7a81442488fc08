// Per-window log-mel front end for gfx950.
//
// Replaces, per analysis window (reference /root/reference):
//   normalize_data                      src/identify_tracks.py:202-209
//   np.abs(librosa.stft(x, n_fft, hop))  src/identify_tracks.py:243
//   custommel.mel_spec (|S|**p, mel_f.)  src/custommel.py:59-63
//   librosa.power_to_db(ref=np.max)     src/identify_tracks.py:266
//   expand_dims / mean_sub / channels   src/identify_tracks.py:267-288
//
// Three launches per batch of windows (all on the caller's stream):
//   fe_stats    min/max/finite partials of every window (HBM stream of the PCM)
//   fe_stft_mel a block owns FPB consecutive frames of one window: the
//               overlapped PCM segment is loaded once (coalesced) and normalised
//               into LDS, each frame is windowed and transformed by an N/2-point
//               complex Stockham FFT (radix 8, LDS ping-pong, table twiddles),
//               split into the N-point real spectrum, |X|**power, and projected
//               on the sparse mel filterbank (CSR rows, contiguous bins).
//   fe_db       per-window max -> power_to_db, clamp, mean_sub, layout/channels.
// The plan is made on the host (aa_fe_plan.h); the stft kernels live in
// aa_fe_stft.h (fe_stft_mel, fe_stft_mel_small, and fe_stft_mel_mixed for the
// n_fft that are not powers of two) and aa_fe_wave4096.h.
#include "aa_fe_wave4096.h"

namespace aa {

enum { FE_STAGE_STATS = 0, FE_STAGE_STFT = 1, FE_STAGE_DB = 2, FE_N_STAGES = 3 };

// ---------------------------------------------------------------------------
// fe_stats: min / max / non-finite over each virtual window (zeros outside the
// valid view, exactly like np.pad before normalize_data).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fe_stats(const float* __restrict__ pcm,
                                                const aa_window* __restrict__ wins,
                                                int win_len, float4* __restrict__ stats) {
    const int w = blockIdx.y;
    const aa_window d = wins[w];
    const int chunk = (win_len + kStatSplit - 1) / kStatSplit;
    const int i0 = blockIdx.x * chunk;
    const int i1 = min(win_len, i0 + chunk);
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    // valid part of this chunk, in window coordinates; the rest is np.pad zeros
    const int v0 = max(i0, d.pad_left);
    const int v1 = min(i1, d.pad_left + d.n_valid);
    if (i0 < i1 && !(v0 == i0 && v1 >= i1)) { mn = 0.f; mx = 0.f; }
    if (v0 < v1) {
        const float* p = pcm + d.src + (v0 - d.pad_left);
        const int n = v1 - v0;
        // scalar head up to 16-byte alignment, float4 body, scalar tail
        const int head = min(n, (int)((16 - ((uintptr_t)p & 15)) & 15) / 4);
        for (int i = threadIdx.x; i < head; i += blockDim.x) {
            float x = p[i];
            bad |= !isfinite(x);
            mn = fminf(mn, x);
            mx = fmaxf(mx, x);
        }
        const int nb = (n - head) / 4;
        const float4* q = reinterpret_cast<const float4*>(p + head);
        // four independent loads in flight per thread before any is consumed
        // (past the end a lane re-reads the last float4: min / max / the
        // non-finite flag do not change under duplicates)
        constexpr int U = 4;
        for (int i = threadIdx.x; i < nb; i += U * blockDim.x) {
            float4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = q[min(i + u * (int)blockDim.x, nb - 1)];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bad |= !isfinite(x[u].x) | !isfinite(x[u].y) | !isfinite(x[u].z) | !isfinite(x[u].w);
                mn = fminf(fminf(mn, x[u].x), fminf(x[u].y, fminf(x[u].z, x[u].w)));
                mx = fmaxf(fmaxf(mx, x[u].x), fmaxf(x[u].y, fmaxf(x[u].z, x[u].w)));
            }
        }
        for (int i = head + nb * 4 + threadIdx.x; i < n; i += blockDim.x) {
            float x = p[i];
            bad |= !isfinite(x);
            mn = fminf(mn, x);
            mx = fmaxf(mx, x);
        }
    }
    __shared__ float smn[4], smx[4];
    __shared__ int sbad[4];
    mn = wave_min(mn);
    mx = wave_max(mx);
    bad = wave_or(bad);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smn[wv] = mn; smx[wv] = mx; sbad[wv] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) {
            mn = fminf(mn, smn[k]);
            mx = fmaxf(mx, smx[k]);
            bad |= sbad[k];
        }
        stats[w * kStatSplit + blockIdx.x] = make_float4(mn, mx, (float)bad, 0.f);
    }
}

// ---------------------------------------------------------------------------
// fe_db: power_to_db(ref=max), clamp at -top_db, mean_sub, channel repeat,
// and the frame-major -> band-major transpose of the stft kernels' output.
// Block = (tile of `tile_t` frames, window): coalesced rows of melF in,
// dB in registers, transpose through LDS, contiguous band rows out.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float db_value(float v, float ref_db, int db_scale, float amin, float top_db) {
    if (db_scale) {
        v = __fsub_rn(__fmul_rn(10.0f, log10f(fmaxf(amin, v))), ref_db);
        v = fmaxf(v, -top_db);  // log_spec.max() == 0 exactly
    }
    return v;
}

// block-wide max of the window's partial maxima -> 10 log10(max(amin, S.max()))
__device__ __forceinline__ float window_ref_db(const float* __restrict__ pmax, int nparts, float amin, float* red) {
    float mx = 0.f;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) mx = fmaxf(mx, pmax[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) mx = fmaxf(mx, red[k]);
    return __fmul_rn(10.0f, log10f(fmaxf(amin, mx)));
}

constexpr int kDbU = 8;     // fe_db: loads in flight per thread
constexpr int kDbTile = 8;  // fe_db: frames per block (a power of two: the tile is indexed by shifts)
static_assert((kDbTile & (kDbTile - 1)) == 0, "fe_db indexes its tile by shifts");

// TO: float, or _Float16 for the fp16 log-mel of aa_fe_config.out_f16
template <typename TO>
__global__ __launch_bounds__(256) void fe_db(const float* __restrict__ melF, const float* __restrict__ pmax,
                                             int nparts, const float4* __restrict__ stats,
                                             const float* __restrict__ band_mean, int n_mels, int T, int tile_t,
                                             int db_scale, float amin, float top_db, int channels, int normalize,
                                             TO* __restrict__ out, int* __restrict__ status) {
    extern __shared__ float tile[];  // [tile_t][n_mels + 1]
    __shared__ float red[4];
    const int w = blockIdx.y;
    const int t0 = blockIdx.x * tile_t;
    const int nt = min(tile_t, T - t0);
    const int ld = n_mels + 1;
    const float* src = melF + ((size_t)w * T + t0) * n_mels;  // nt contiguous frame rows
    const int total = nt * n_mels;
    // row of element idx as a float product: exact while idx < 2^21 (the tile
    // holds at most 2^14 elements), ~35 VALU cheaper than an integer divide
    const float inv_nm = 1.0f / (float)n_mels;
    const int tsh = __builtin_ctz(tile_t);  // tile_t is a power of two (host)
    constexpr int U = kDbU;  // loads in flight per thread before any is consumed
    // the first batch of rows is issued before the window's reference max
    // (independent loads: their latencies overlap instead of adding up)
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[min(u * 256 + (int)threadIdx.x, total - 1)];
    const float ref_db = window_ref_db(pmax + (size_t)w * nparts, nparts, amin, red);
    if (blockIdx.x == 0 && threadIdx.x == 0 && status) {
        float lo = INFINITY, hi = -INFINITY;
        int bad = 0;
        for (int s = 0; s < kStatSplit; ++s) {
            const float4 st = stats[w * kStatSplit + s];
            lo = fminf(lo, st.x);
            hi = fmaxf(hi, st.y);
            bad |= st.z != 0.f;
        }
        // normalize_data divides by max(x - min): 0 -> NaN -> librosa raises
        if (normalize && !(hi - lo > 0.f)) bad = 1;
        status[w] = bad ? AA_WIN_NONFINITE : AA_WIN_OK;
    }
    for (int i0 = 0; i0 < total; i0 += U * 256) {
        if (i0 > 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = src[min(i0 + u * 256 + (int)threadIdx.x, total - 1)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = i0 + u * 256 + threadIdx.x;
            if (idx < total) {
                const int tt = (int)(((float)idx + 0.5f) * inv_nm), m = idx - tt * n_mels;
                tile[tt * ld + m] = db_value(v[u], ref_db, db_scale, amin, top_db);
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * tile_t; idx += 256) {
        const int m = idx >> tsh, tt = idx & (tile_t - 1);
        if (tt < nt) {
            float v = tile[tt * ld + m];
            if (band_mean) v -= band_mean[(size_t)w * n_mels + m];
            TO* o = out + (((size_t)w * n_mels + m) * T + t0 + tt) * channels;
            for (int c = 0; c < channels; ++c) o[c] = (TO)v;
        }
    }
}

// mean_sub: per-band mean over time of the dB values, one block per window
__global__ __launch_bounds__(256) void fe_band_mean(const float* __restrict__ melF, const float* __restrict__ pmax,
                                                    int nparts, int n_mels, int T, int db_scale, float amin,
                                                    float top_db, float* __restrict__ band_mean) {
    __shared__ float red[4];
    const int w = blockIdx.x;
    const float ref_db = window_ref_db(pmax + (size_t)w * nparts, nparts, amin, red);
    const float* src = melF + (size_t)w * T * n_mels;
    for (int m = threadIdx.x; m < n_mels; m += 256) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += db_value(src[(size_t)t * n_mels + m], ref_db, db_scale, amin, top_db);
        band_mean[(size_t)w * n_mels + m] = s / (float)T;
    }
}

// ---- host side: the plan (aa_fe_plan.h) says which kernel, grid and LDS bytes ----
// the stft launch of the plan's kernel and n_fft at power mode PM
template <int PM>
static int launch_stft(const FePlan& p, const float* pcm, const aa_window* wins, int n_win, const float4* stats,
                       float* melS, float* blkmax, hipStream_t st) {
    // fe_stft_mel and fe_stft_mel_small take the same arguments
    auto lds = [&](auto kernel, int threads) -> int {
        AA_DYN_LDS(kernel, p.lds_bytes);  // dynamic LDS opt-in (static LDS comes on top)
        hipLaunchKernelGGL(kernel, dim3(p.grid(n_win)), dim3(threads), p.lds_bytes, st, pcm, wins, stats, p.d_win,
                           p.d_tw, p.d_tw2, p.d_rows, p.d_vals, p.nnz, p.cfg.win_len, p.cfg.hop, p.T, p.cfg.n_mels,
                           p.kmin, p.kmax, p.cfg.normalize, p.cfg.power, p.nblk, p.nblk * n_win, melS, blkmax);
        AA_LAUNCH_CHECK();
        return AA_OK;
    };
    switch (p.kernel) {
        case FE_K_WAVE4096:
            // (not implied by plan_fe's segment bound: a dense filterbank can pass that and not fit here)
            AA_CHECK(p.lds_bytes <= 160 * 1024, AA_ERR_UNSUPPORTED, "fe4096: %zu B of LDS", p.lds_bytes);
            AA_DYN_LDS(fe_stft_mel_4096<PM>, p.lds_bytes);
            hipLaunchKernelGGL(fe_stft_mel_4096<PM>, dim3(p.grid(n_win)), dim3(64 * kWpb), p.lds_bytes, st, pcm, wins,
                               stats, p.d_tw, p.d_tw2, p.d_cimg, p.cimg_bytes, p.cfg.win_len, p.cfg.hop, p.T,
                               p.cfg.n_mels, p.kmin, p.kmax, p.cfg.normalize, p.cfg.power, p.T * n_win, melS, blkmax);
            AA_LAUNCH_CHECK();
            return AA_OK;
        case FE_K_MIXED: {
            // fe_stft_mel's arguments, then n_fft and the schedule, 4 bits per radix
            unsigned sched = 0;
            for (int i = 0; i < p.n_pass; ++i) sched |= (unsigned)p.radix[i] << (4 * i);
            auto mixed = [&](auto kernel) -> int {
                AA_DYN_LDS(kernel, p.lds_bytes);
                hipLaunchKernelGGL(kernel, dim3(p.grid(n_win)), dim3(fe_mixed_threads(p.cfg.n_fft)), p.lds_bytes, st,
                                   pcm, wins, stats, p.d_win, p.d_tw, p.d_tw2, p.d_rows, p.d_vals, p.nnz,
                                   p.cfg.win_len, p.cfg.hop, p.T, p.cfg.n_mels, p.kmin, p.kmax, p.cfg.normalize,
                                   p.cfg.power, p.nblk, p.nblk * n_win, melS, blkmax, p.cfg.n_fft, sched);
                AA_LAUNCH_CHECK();
                return AA_OK;
            };
            return p.tw_lds ? mixed(fe_stft_mel_mixed<PM, true>) : mixed(fe_stft_mel_mixed<PM, false>);
        }
        case FE_K_SMALL:
            return p.cfg.n_fft == 256   ? lds(fe_stft_mel_small<256, PM>, 64 * kSmallWaves)
                   : p.cfg.n_fft == 512 ? lds(fe_stft_mel_small<512, PM>, 64 * kSmallWaves)
                                        : lds(fe_stft_mel_small<1024, PM>, 64 * kSmallWaves);
        default:
            return p.cfg.n_fft == 2048   ? lds(fe_stft_mel<2048, PM>, 2048 / 16)
                   : p.cfg.n_fft == 4096 ? lds(fe_stft_mel<4096, PM>, 4096 / 16)
                                         : lds(fe_stft_mel<8192, PM>, 8192 / 16);
    }
}

struct FeWs {
    float4* stats;
    float* melS;       // frame-major mel power [n_win][T][n_mels]
    float* blkmax;     // partial maxima [n_win][nparts]
    float* band_mean;  // mean_sub: [n_win][n_mels]
    size_t bytes;
};

static FeWs fe_ws_layout(const FePlan& p, int n_win, char* base) {
    FeWs w{};
    size_t off = 0;
    w.stats = reinterpret_cast<float4*>(base + off);
    off = align_up(off + sizeof(float4) * (size_t)n_win * kStatSplit, 256);
    w.melS = reinterpret_cast<float*>(base + off);
    off = align_up(off + sizeof(float) * (size_t)n_win * p.cfg.n_mels * p.T, 256);
    w.blkmax = reinterpret_cast<float*>(base + off);
    off = align_up(off + sizeof(float) * (size_t)n_win * p.nparts, 256);
    w.band_mean = reinterpret_cast<float*>(base + off);
    if (p.cfg.mean_sub) off = align_up(off + sizeof(float) * (size_t)n_win * p.cfg.n_mels, 256);
    w.bytes = off;
    return w;
}

// device copies of the plan's images, which are then released
static hipError_t upload_fe(FePlan* p) {
    auto up = [](auto** d, auto& h) -> hipError_t {
        const size_t b = h.size() * sizeof(h[0]);
        hipError_t e = hipMalloc((void**)d, b);
        if (e == hipSuccess) e = hipMemcpy(*d, h.data(), b, hipMemcpyHostToDevice);
        h.clear();
        h.shrink_to_fit();
        return e;
    };
    hipError_t e = up(&p->d_win, p->h_win);
    if (e == hipSuccess) e = up(&p->d_tw, p->h_tw);
    if (e == hipSuccess) e = up(&p->d_tw2, p->h_tw2);
    if (e == hipSuccess) e = up(&p->d_rows, p->h_rows);
    if (e == hipSuccess) e = up(&p->d_vals, p->h_vals);
    if (e == hipSuccess && p->cimg_bytes) e = up(&p->d_cimg, p->h_cimg);
    p->uploaded = true;
    return e;
}

}  // namespace aa

using namespace aa;

extern "C" int aa_fe_plan(const aa_fe_config* cfg, const float* melfb, void** plan) {
    AA_CHECK(plan, AA_ERR_INVALID, "aa_fe_create: null argument");
    FePlan* p = new FePlan();
    const int rc = plan_fe(cfg, melfb, p);
    if (rc != AA_OK) {
        delete p;
        return rc;
    }
    *plan = p;
    return AA_OK;
}

extern "C" int aa_fe_create(const aa_fe_config* cfg, const float* melfb, void** plan) {
    void* h = nullptr;
    const int rc = aa_fe_plan(cfg, melfb, plan ? &h : nullptr);
    if (rc != AA_OK) return rc;
    const hipError_t e = upload_fe(static_cast<FePlan*>(h));
    if (e != hipSuccess) {
        set_error("aa_fe_create: %s", hipGetErrorString(e));
        aa_fe_destroy(h);
        return AA_ERR_HIP;
    }
    *plan = h;
    return AA_OK;
}

extern "C" int aa_fe_plan_info(const void* plan, int32_t n_win, aa_fe_info* out) {
    const FePlan* p = static_cast<const FePlan*>(plan);
    AA_CHECK(p && out && n_win >= 0, AA_ERR_INVALID, "aa_fe_plan_info: bad argument");
    *out = aa_fe_info{(int32_t)p->kernel, p->T, p->kmin, p->kmax, p->nnz, p->nparts, (int64_t)p->lds_bytes,
                             p->grid(n_win)};
    return AA_OK;
}

extern "C" int aa_fe_plan_image(const void* plan, int32_t which, void* buf, size_t cap, size_t* len) {
    const FePlan* p = static_cast<const FePlan*>(plan);
    AA_CHECK(p && len && which >= 0 && which <= 5, AA_ERR_INVALID, "aa_fe_plan_image: bad argument");
    AA_CHECK(!p->uploaded, AA_ERR_UNSUPPORTED,
             "aa_fe_plan_image: the host images are released once a plan is created; plan it (aa_fe_plan)");
    const void* src[6] = {p->h_win.data(), p->h_tw.data(), p->h_tw2.data(), p->h_rows.data(), p->h_vals.data(), p->h_cimg.data()};
    const size_t n[6] = {sizeof(float) * p->h_win.size(), sizeof(float2) * p->h_tw.size(), sizeof(float2) * p->h_tw2.size(),
                         sizeof(int4) * p->h_rows.size(), sizeof(float) * p->h_vals.size(), p->h_cimg.size()};
    *len = n[which];
    if (!buf) return AA_OK;  // a size query
    AA_CHECK(cap >= *len, AA_ERR_INVALID, "aa_fe_plan_image: buffer %zu < %zu", cap, *len);
    if (*len) memcpy(buf, src[which], *len);
    return AA_OK;
}

extern "C" int aa_fe_plan_passes(const void* plan, int32_t* radices, int32_t cap, int32_t* n) {
    const FePlan* p = static_cast<const FePlan*>(plan);
    AA_CHECK(p && n && cap >= 0 && (radices || cap == 0), AA_ERR_INVALID, "aa_fe_plan_passes: bad argument");
    *n = p->n_pass;
    if (!radices) return AA_OK;  // a count query
    AA_CHECK(cap >= p->n_pass, AA_ERR_INVALID, "aa_fe_plan_passes: room for %d radices < %d", cap, p->n_pass);
    for (int i = 0; i < p->n_pass; ++i) radices[i] = p->radix[i];
    return AA_OK;
}

extern "C" int aa_fe_destroy(void* plan) {
    FePlan* p = static_cast<FePlan*>(plan);
    if (!p) return AA_OK;
    if (p->uploaded) {
        for (void* d : {(void*)p->d_win, (void*)p->d_tw, (void*)p->d_tw2, (void*)p->d_rows, (void*)p->d_vals, (void*)p->d_cimg})
            (void)hipFree(d);
        p->timer.release();
    }
    delete p;
    return AA_OK;
}

extern "C" int aa_fe_n_frames(const void* plan) { return plan ? static_cast<const FePlan*>(plan)->T : -1; }

extern "C" size_t aa_fe_workspace_bytes(const void* plan, int32_t max_windows) {
    if (!plan || max_windows < 0) return 0;
    return fe_ws_layout(*static_cast<const FePlan*>(plan), max_windows, nullptr).bytes;
}

extern "C" int aa_fe_run(void* plan, const float* pcm, int64_t pcm_len, const aa_window* windows,
                         int32_t n_win, void* out, int32_t* win_status, void* workspace,
                         size_t workspace_bytes, void* stream) {
    FePlan* p = static_cast<FePlan*>(plan);
    AA_CHECK(p && pcm && windows && out, AA_ERR_INVALID, "aa_fe_run: null argument");
    AA_CHECK(p->uploaded, AA_ERR_INVALID, "aa_fe_run: the plan is planned only (aa_fe_plan), not created");
    AA_CHECK(n_win >= 0, AA_ERR_INVALID, "aa_fe_run: n_win < 0");
    (void)pcm_len;  // window views are validated by the host against pcm_len
    if (n_win == 0) return AA_OK;
    // the per-window grids carry the window in blockIdx.y (at most 65,535):
    // larger batches run as consecutive chunks through the same workspace
    constexpr int32_t CHUNK = 32768;
    if (n_win > CHUNK) {
        const size_t ob = (size_t)p->cfg.n_mels * p->T * p->cfg.channels * (p->cfg.out_f16 ? 2 : 4);
        for (int32_t c0 = 0; c0 < n_win; c0 += CHUNK) {
            const int32_t nc = std::min(CHUNK, n_win - c0);
            const int rc = aa_fe_run(plan, pcm, pcm_len, windows + c0, nc, static_cast<char*>(out) + c0 * ob,
                                     win_status ? win_status + c0 : nullptr, workspace, workspace_bytes, stream);
            if (rc != AA_OK) return rc;
        }
        return AA_OK;
    }
    FeWs ws = fe_ws_layout(*p, n_win, static_cast<char*>(workspace));
    AA_CHECK(workspace && workspace_bytes >= ws.bytes, AA_ERR_WORKSPACE,
             "aa_fe_run: workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0;
    int rc = p->timer.begin(FE_STAGE_STATS, st, &e0);
    if (rc != AA_OK) return rc;
    hipLaunchKernelGGL(fe_stats, dim3(kStatSplit, n_win), dim3(256), 0, st, pcm, windows,
                       p->cfg.win_len, ws.stats);
    AA_LAUNCH_CHECK();
    if ((rc = p->timer.end(FE_STAGE_STATS, st, e0)) != AA_OK) return rc;
    if ((rc = p->timer.begin(FE_STAGE_STFT, st, &e0)) != AA_OK) return rc;
    rc = p->cfg.power == 2.f   ? launch_stft<PM_SQUARE>(*p, pcm, windows, n_win, ws.stats, ws.melS, ws.blkmax, st)
         : p->cfg.power == 1.f ? launch_stft<PM_ABS>(*p, pcm, windows, n_win, ws.stats, ws.melS, ws.blkmax, st)
                               : launch_stft<PM_GENERAL>(*p, pcm, windows, n_win, ws.stats, ws.melS, ws.blkmax, st);
    if (rc != AA_OK) return rc;
    if ((rc = p->timer.end(FE_STAGE_STFT, st, e0)) != AA_OK) return rc;
    if ((rc = p->timer.begin(FE_STAGE_DB, st, &e0)) != AA_OK) return rc;
    if (p->cfg.mean_sub) {
        hipLaunchKernelGGL(fe_band_mean, dim3(n_win), dim3(256), 0, st, ws.melS, ws.blkmax, p->nparts,
                           p->cfg.n_mels, p->T, p->cfg.db_scale, p->cfg.amin, p->cfg.top_db, ws.band_mean);
        AA_LAUNCH_CHECK();
    }
    int tile_t = kDbTile;  // frames per fe_db block (the [tile_t][n_mels + 1] tile within 64 KiB)
    while (tile_t > 1 && (size_t)tile_t * (p->cfg.n_mels + 1) * 4 > 65536) tile_t >>= 1;
    auto db = [&](auto* o) {
        hipLaunchKernelGGL(fe_db<std::remove_pointer_t<decltype(o)>>, dim3((p->T + tile_t - 1) / tile_t, n_win),
                           dim3(256), (size_t)tile_t * (p->cfg.n_mels + 1) * 4, st, ws.melS, ws.blkmax, p->nparts, ws.stats,
                           p->cfg.mean_sub ? ws.band_mean : nullptr, p->cfg.n_mels, p->T, tile_t, p->cfg.db_scale,
                           p->cfg.amin, p->cfg.top_db, p->cfg.channels, p->cfg.normalize, o, win_status);
    };
    if (p->cfg.out_f16) db((_Float16*)out);
    else db((float*)out);
    AA_LAUNCH_CHECK();
    return p->timer.end(FE_STAGE_DB, st, e0);
}

extern "C" int aa_fe_n_stages(const void* plan) { return plan ? FE_N_STAGES : -1; }

// Algorithmic work of one window through each launch:
//   stft_mel flops = T (2.5 N log2 N + N + 3 (N/2 + 1) + 2 nnz) + 5 L
//   (real FFT as an N/2 complex FFT + split, window, |.|^p, mel rows; the
//   normalisation pass), bytes = L f32 PCM in + n_mels T f32 mel power out.
//   fe_stft_mel_mixed: the 2.5 N log2 N term is counted from the plan's
//   schedule instead: per pass N/2 / r butterflies of 6 (r - 1) twiddle flops
//   (none in pass 1) plus the radix's own adds and multiplies (2: 4, 3: 16,
//   4: 16, 5: 44, 8: 56), and 5 N for the real split.
extern "C" int aa_fe_stage_info(const void* plan, int32_t stage, char* name, int32_t name_len,
                                double* flops_per_item, double* bytes_per_item) {
    const FePlan* p = static_cast<const FePlan*>(plan);
    AA_CHECK(p && stage >= 0 && stage < FE_N_STAGES, AA_ERR_INVALID, "aa_fe_stage_info: bad stage");
    const double N = p->cfg.n_fft, L = p->cfg.win_len, T = p->T, M = p->cfg.n_mels;
    double fl = 0, by = 0;
    const char* nm = "";
    switch (stage) {
        case FE_STAGE_STATS: nm = "fe_stats"; fl = 2 * L; by = 4 * L; break;
        case FE_STAGE_STFT:
            nm = fe_kernel_name(p->kernel);
            if (p->kernel == FE_K_MIXED) {
                double fft = 5 * N;  // the real split
                for (int i = 0; i < p->n_pass; ++i) {
                    const int r = p->radix[i];
                    const double own = r == 2 ? 4 : r == 3 ? 16 : r == 4 ? 16 : r == 5 ? 44 : 56;
                    fft += N / 2 / r * ((i ? 6.0 * (r - 1) : 0.0) + own);
                }
                fl = T * (fft + N + 3 * (N / 2 + 1) + 2.0 * p->nnz) + 5 * L;
            } else
            fl = T * (2.5 * N * std::log2(N) + N + 3 * (N / 2 + 1) + 2.0 * p->nnz) + 5 * L;
            by = 4 * L + 4 * M * T;
            break;
        default: nm = "fe_db"; fl = 3 * M * T; by = M * T * (4 + (p->cfg.out_f16 ? 2 : 4) * p->cfg.channels); break;
    }
    if (name && name_len > 0) snprintf(name, name_len, "%s", nm);
    if (flops_per_item) *flops_per_item = fl;
    if (bytes_per_item) *bytes_per_item = by;
    return AA_OK;
}

extern "C" int aa_fe_set_timing(void* plan, uint32_t stage_mask) {
    FePlan* p = static_cast<FePlan*>(plan);
    AA_CHECK(p, AA_ERR_INVALID, "aa_fe_set_timing: null plan");
    AA_CHECK(p->uploaded, AA_ERR_INVALID, "aa_fe_set_timing: the plan is planned only (aa_fe_plan), not created");
    p->timer.mask = stage_mask;
    return AA_OK;
}

extern "C" int aa_fe_stage_time(void* plan, int32_t stage, double* total_ms, int64_t* count) {
    FePlan* p = static_cast<FePlan*>(plan);
    AA_CHECK(p && stage >= 0 && stage < FE_N_STAGES, AA_ERR_INVALID, "aa_fe_stage_time: bad stage");
    AA_CHECK(p->uploaded, AA_ERR_INVALID, "aa_fe_stage_time: the plan is planned only (aa_fe_plan), not created");
    return p->timer.collect(stage, total_ms, count);
}
