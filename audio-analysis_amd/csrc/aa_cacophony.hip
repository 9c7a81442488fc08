// The old cacophony index's frame loop for gfx950 (reference
// src/cacophony_index.py:53-97): per 2048-sample frame of the 16 kHz
// recording the float64 Hann window, scipy.fftpack.dct (the unnormalised
// DCT-II) and the energy of ten log-spaced bands; per pair of neighbouring
// frames the bands that more than halved or more than doubled.
//
//   ci_bands   one workgroup (one wave) per frame, all recordings of the
//              batch in one launch.  s[n] = w[n] x[n] (f64 window times the
//              f32 sample, one rounding: numpy's product).  Makhoul's
//              reordering v[n] = s[2n], v[2047 - n] = s[2n + 1] makes the
//              DCT-II the real DFT V of v: y[k] = 2 Re(V[k] e^(-i pi k / 4096)).
//              V comes from the 1024-point complex FFT Z of z[m] = v[2m] +
//              i v[2m + 1] and the real split.  Sample 4m' + r of the frame
//              lands in z[m'] (r = 0: re, r = 2: im) or z[1023 - m'] (r = 3:
//              re, r = 1: im), so the reordering is the LDS address of the
//              windowed sample.  The FFT is 16 x 8 x 8 in registers with two
//              LDS transposes (n = 64 n1 + 8 n2 + n3, k = k1 + 16 k2 + 128 k3,
//              m = k1 + 16 k2):
//                1. lane (n2, n3): DFT-16 over n1, twiddle W128^(n2 k1)
//                2. lane (k1, n3), two k1 per lane: DFT-8 over n2, twiddle
//                   W1024^(n3 m)
//                3. lane's columns m and m + 64: DFT-8 over n3 -> Z[m + 128 k3]
//              Z goes back to LDS in natural order; lane t takes the pairs
//              (Z[k], Z[1024 - k]), k = 1 + t + 64 i, through the split
//              (V[k] = E + W2048^k O, V[1024 - k] = conj(E - W2048^k O)) and
//              the DCT's rotation into y[k], y[2048 - k], y[1024 - k],
//              y[1024 + k]; lane 0 adds y[0] and y[1024] from Z[0].  Every twiddle is a
//              table value rounded from long double (the rotation of
//              1024 - k excepted: two operations on that of k).  The band sums run over
//              y in LDS: lane t adds y[k]^2 for k = e_b + t, e_b + t + 64, ...
//              and a xor-butterfly of shuffles adds the 64 partial sums -- a
//              fixed order, no atomics, so a run is bit-reproducible.
//   ci_points  one lane per frame row: the ten comparisons against the row
//              before it, unless the row is its recording's first.
//
// The transform may contract into fused multiply-adds (the file is built
// with the compiler's default); only the window product names its rounding.
// Digital silence gives exactly 0.0 in every band either way.
#include <cmath>
#include <vector>

#include "aa_common.h"
#include "aa_fft64.h"

namespace aa {

constexpr int CI_N = AA_CI_N;
constexpr int CI_HOP = AA_CI_HOP;
constexpr int CI_NB = AA_CI_BANDS;
constexpr int CI_T = 64;     // lanes per frame
constexpr int CI_M = 1024;   // complex FFT points
constexpr int CI_BUF = CI_M;  // double2; each exchange in turn, then y: 16 KiB, 10 workgroups per CU
static_assert(CI_N == 2 * CI_M && CI_HOP * 2 == CI_N, "geometry");
// The two transposes are swizzled instead of padded (a ds_*_b128 serves 16
// lanes = 256 B of banks per pass):
//   step-1 row k1 holds its lane t at slot (t + 8 k1) mod 64: written as a
//   rotated contiguous row; read by lanes (k1a, n3) as two 128-B runs per
//   pass, rows k1a and k1a + 1, which the rotation puts 128 B apart mod 256
//   step-2 column m holds its n3 at slot (n3 + m / 2) mod 8 of its 128-B
//   block: even and odd m take the two bank halves, the eight even (odd) m of
//   a pass eight different slots
__device__ __forceinline__ int ci_row(int k1, int col) { return k1 * 64 + ((col + 8 * k1) & 63); }
__device__ __forceinline__ int ci_col(int m, int n3) { return m * 8 + ((n3 + (m >> 1)) & 7); }

// tables (double2): tw1 [16][8] W128^(n2 k1) | tw2 [8][128] W1024^(n3 m) |
// twS [513] W2048^k | rot [513] (cos, sin)(pi k / 4096)
constexpr int kCiTw1 = 0, kCiTw2 = kCiTw1 + 16 * 8, kCiTwS = kCiTw2 + 8 * 128, kCiRot = kCiTwS + 513,
              kCiTabN = kCiRot + 513;

// One recording of a batch; the batch travels by value as a kernel argument.
struct CiJob {
    long long off;  // first sample in the PCM buffer
    int frames;     // aa_ci_n_frames
    int row0;       // its first row of bins
    int pt0;        // its first point
    int pad;
};
struct CiBatch {
    int n;
    int rows;
    int edges[CI_NB + 1];
    int pad;
    CiJob job[AA_CI_MAX_REC];
};
static_assert(sizeof(CiBatch) <= 2048, "kernel argument size");

struct CiPlan {
    double window[CI_N];
    int edges[CI_NB + 1];
    double* d_window = nullptr;
    double2* d_tab = nullptr;
};

// The recording that owns bins row `row` (< B.rows): the last job whose row0
// is <= row.  A recording without frames shares its row0 with the one after
// it, so the last of equal row0s is the one that has the row; a bisection,
// since every workgroup pays for it before its first load.
__device__ __forceinline__ int ci_job_of(const CiBatch& B, int row) {
    int lo = 0, hi = B.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (B.job[mid].row0 <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

// 16 KiB of LDS lets 10 workgroups share a CU: keep the registers to three waves per SIMD
__global__ __launch_bounds__(CI_T) __attribute__((amdgpu_waves_per_eu(3))) void ci_bands(
    const float* __restrict__ pcm, const CiBatch B, const double* __restrict__ win, const double2* __restrict__ tab,
    double* __restrict__ bins) {
    __shared__ double2 buf[CI_BUF];
    const int t = threadIdx.x;
    const int row = blockIdx.x;
    if (row >= B.rows) return;
    const int j = ci_job_of(B, row);  // uniform
    const int f = row - B.job[j].row0;
    const float* __restrict__ x = pcm + B.job[j].off + (long long)CI_HOP * (f + 1);

    // ---- window and reordering: sample n = 4 m' + r -> z[m'] or z[1023 - m'] ----
    double* zd = reinterpret_cast<double*>(buf);
#pragma unroll
    for (int i = 0; i < CI_N / CI_T; ++i) {
        const int n = t + CI_T * i;
        const double s = __dmul_rn(win[n], (double)x[n]);
        const int mq = n >> 2, r = n & 3;
        const int m = (r & 1) ? CI_M - 1 - mq : mq;         // r = 1, 3: the reversed odd samples
        const int im = (r == 2 || r == 1) ? 1 : 0;
        zd[2 * m + im] = s;
    }
    // Every table value is loaded a step before its use (the loads of a step
    // would otherwise start after the barrier in front of it: the frame's
    // time is a chain of memory round trips, not arithmetic).
    double2 w1[16];  // W128^(n2 k1), n2 = t >> 3
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) w1[k1] = tab[kCiTw1 + k1 * 8 + (t >> 3)];
    __syncthreads();

    // ---- 1. DFT-16 over n1, twiddle W128^(n2 k1), rows k1 ----
    double2 v[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) v[n1] = buf[t + CI_T * n1];
    __syncthreads();
    ddft16(v);
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) v[dp16(k1)] = dmul(v[dp16(k1)], w1[k1]);
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) buf[ci_row(k1, t)] = v[dp16(k1)];
    const int k1a = t >> 3, n3 = t & 7;
    double2 wa[8], wb[8];  // W1024^(n3 m) of the lane's columns m = k1a + 16 k2 and m + 8
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
        wa[k2] = tab[kCiTw2 + n3 * 128 + k1a + 16 * k2];
        wb[k2] = tab[kCiTw2 + n3 * 128 + k1a + 16 * k2 + 8];
    }
    __syncthreads();

    // ---- 2. DFT-8 over n2 of the lane's (k1, n3) and (k1 + 8, n3), twiddle W1024^(n3 m) ----
    double2 a[8], b[8];
#pragma unroll
    for (int n2 = 0; n2 < 8; ++n2) {
        a[n2] = buf[ci_row(k1a, 8 * n2 + n3)];
        b[n2] = buf[ci_row(k1a + 8, 8 * n2 + n3)];
    }
    __syncthreads();
    ddft8(a);
    ddft8(b);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
        const int ma = k1a + 16 * k2, mb = ma + 8;
        buf[ci_col(ma, n3)] = dmul(a[k2], wa[k2]);
        buf[ci_col(mb, n3)] = dmul(b[k2], wb[k2]);
    }
    double2 ws[8], rk[8];  // the split's W2048^k and the rotation (c_k, s_k), k = 1 + t + 64 i
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = 1 + t + CI_T * i;
        ws[i] = tab[kCiTwS + k];
        rk[i] = tab[kCiRot + k];
    }
    __syncthreads();

    // ---- 3. DFT-8 over n3 of columns t and t + 64: Z[m + 128 k3], natural order ----
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        a[q] = buf[ci_col(t, q)];
        b[q] = buf[ci_col(t + 64, q)];
    }
    __syncthreads();
    ddft8(a);
    ddft8(b);
#pragma unroll
    for (int k3 = 0; k3 < 8; ++k3) {
        buf[t + 128 * k3] = a[k3];
        buf[t + 64 + 128 * k3] = b[k3];
    }
    __syncthreads();

    // ---- real split and the DCT's rotation: Z is the transform of z
    // unhalved, so E and O below are twice the split's and carry the DCT's
    // factor 2 ----
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = buf[1 + t + CI_T * i];
        b[i] = buf[CI_M - 1 - t - CI_T * i];
    }
    const double2 z0 = buf[0];
    __syncthreads();
    double* y = reinterpret_cast<double*>(buf);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = 1 + t + CI_T * i;  // 1..512 (k = 512 pairs with itself and writes its two bins twice)
        const double2 E = make_double2(a[i].x + b[i].x, a[i].y - b[i].y);
        const double2 O = make_double2(a[i].y + b[i].y, b[i].x - a[i].x);
        const double2 q = dmul(ws[i], O);
        const double2 Vk = make_double2(E.x + q.x, E.y + q.y);    // 2 V[k]
        const double2 Vm = make_double2(E.x - q.x, q.y - E.y);    // 2 V[1024 - k]
        // the rotation of 1024 - k, (cos, sin)(pi / 4 - pi k / 4096), from that of k
        // (two more roundings of 2^-53 in a coefficient: far inside the gate)
        const double2 rm = make_double2(kRt2 * (rk[i].x + rk[i].y), kRt2 * (rk[i].x - rk[i].y));
        y[k] = Vk.x * rk[i].x + Vk.y * rk[i].y;
        y[CI_N - k] = Vk.x * rk[i].y - Vk.y * rk[i].x;
        y[CI_M - k] = Vm.x * rm.x + Vm.y * rm.y;
        y[CI_M + k] = Vm.x * rm.y - Vm.y * rm.x;
    }
    if (t == 0) {  // V[0] = Re Z[0] + Im Z[0], V[1024] = Re Z[0] - Im Z[0]: real
        y[0] = 2.0 * (z0.x + z0.y);
        y[CI_M] = 2.0 * (z0.x - z0.y) * kRt2;
    }
    __syncthreads();

    // ---- band energies, fixed order: the ten bands' lane sums first, then
    // their ten butterflies side by side (independent shuffles) ----
    double acc[CI_NB];
#pragma unroll
    for (int bnd = 0; bnd < CI_NB; ++bnd) {
        const int hi = B.edges[bnd + 1];
        double s = 0.0;
        for (int k = B.edges[bnd] + t; k < hi; k += CI_T) s += y[k] * y[k];
        acc[bnd] = s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int bnd = 0; bnd < CI_NB; ++bnd) acc[bnd] += __shfl_xor(acc[bnd], o, 64);
    }
    if (t < CI_NB) {
        double r = acc[0];
#pragma unroll
        for (int bnd = 1; bnd < CI_NB; ++bnd) r = t == bnd ? acc[bnd] : r;
        bins[(size_t)row * CI_NB + t] = r;  // every lane holds every sum: lane b stores band b
    }
}

__global__ __launch_bounds__(256) void ci_points(const double* __restrict__ bins, const CiBatch B,
                                                 int* __restrict__ points) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= B.rows) return;
    const int j = ci_job_of(B, row);
    const int f = row - B.job[j].row0;
    if (f < 1) return;  // a recording's first frame has no predecessor
    const double* cur = bins + (size_t)row * CI_NB;
    const double* prev = cur - CI_NB;
    int c = 0;
#pragma unroll
    for (int bnd = 0; bnd < CI_NB; ++bnd) {
        const double p = prev[bnd], q = cur[bnd];
        c += (q * 2.0 < p) + (q > p * 2.0);
    }
    points[B.job[j].pt0 + f - 1] = c;
}

static int ci_plan_host(const double* window, const int32_t* edges, CiPlan** out, const char* who) {
    AA_CHECK(window && edges && out, AA_ERR_INVALID, "%s: null argument", who);
    for (int b = 0; b <= CI_NB; ++b) {
        AA_CHECK(edges[b] >= 0 && edges[b] <= CI_N, AA_ERR_INVALID, "%s: edge %d is %d, outside 0..%d", who, b,
                 edges[b], CI_N);
        AA_CHECK(b == 0 || edges[b] >= edges[b - 1], AA_ERR_INVALID, "%s: edges decrease at %d (%d after %d)", who, b,
                 edges[b], edges[b - 1]);
    }
    for (int n = 0; n < CI_N; ++n)
        AA_CHECK(std::isfinite(window[n]), AA_ERR_INVALID, "%s: window[%d] is not finite", who, n);
    CiPlan* p = new CiPlan();
    for (int n = 0; n < CI_N; ++n) p->window[n] = window[n];
    for (int b = 0; b <= CI_NB; ++b) p->edges[b] = edges[b];
    *out = p;
    return AA_OK;
}

static int64_t ci_frames(int64_t n) { return n <= 2 * CI_N ? 0 : (n - 2 * CI_N + CI_HOP - 1) / CI_HOP; }

// rows of a batch, or -1 when a length is out of range
static int64_t ci_rows(const int64_t* lengths, int32_t n_rec) {
    int64_t rows = 0;
    for (int32_t k = 0; k < n_rec; ++k) {
        if (lengths[k] < 0 || lengths[k] > AA_CI_MAX_SAMPLES) return -1;
        rows += ci_frames(lengths[k]);
    }
    return rows;
}

}  // namespace aa

extern "C" int64_t aa_ci_n_frames(int64_t n_samples) { return aa::ci_frames(n_samples); }

extern "C" int aa_ci_plan(const double* window, const int32_t* edges, void** plan) {
    aa::CiPlan* p = nullptr;
    const int rc = aa::ci_plan_host(window, edges, plan ? &p : nullptr, "aa_ci_plan");
    if (rc == AA_OK) *plan = p;
    return rc;
}

extern "C" int aa_ci_create(const double* window, const int32_t* edges, void** plan) {
    using namespace aa;
    CiPlan* p = nullptr;
    const int rc = ci_plan_host(window, edges, plan ? &p : nullptr, "aa_ci_create");
    if (rc != AA_OK) return rc;
    // twiddles rounded from long double
    auto wexp = [](long long e, long long m) {  // exp(-2 pi i e / m)
        const long double a = -2.0L * 3.141592653589793238462643383279502884L * (long double)(e % m) / (long double)m;
        return make_double2((double)cosl(a), (double)sinl(a));
    };
    std::vector<double2> tab(kCiTabN);
    for (int k1 = 0; k1 < 16; ++k1)
        for (int n2 = 0; n2 < 8; ++n2) tab[kCiTw1 + k1 * 8 + n2] = wexp((long long)n2 * k1, 128);
    for (int n3 = 0; n3 < 8; ++n3)
        for (int m = 0; m < 128; ++m) tab[kCiTw2 + n3 * 128 + m] = wexp((long long)n3 * m, 1024);
    for (int k = 0; k <= 512; ++k) tab[kCiTwS + k] = wexp(k, 2048);
    for (int k = 0; k <= 512; ++k) {
        const long double a = 3.141592653589793238462643383279502884L * (long double)k / 4096.0L;
        tab[kCiRot + k] = make_double2((double)cosl(a), (double)sinl(a));
    }
    hipError_t e = hipMalloc((void**)&p->d_tab, sizeof(double2) * tab.size());
    if (e == hipSuccess) e = hipMemcpy(p->d_tab, tab.data(), sizeof(double2) * tab.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_window, sizeof(double) * CI_N);
    if (e == hipSuccess) e = hipMemcpy(p->d_window, p->window, sizeof(double) * CI_N, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("aa_ci_create: %s", hipGetErrorString(e));
        if (p->d_tab) (void)hipFree(p->d_tab);
        if (p->d_window) (void)hipFree(p->d_window);
        delete p;
        return AA_ERR_HIP;
    }
    *plan = p;
    return AA_OK;
}

extern "C" int aa_ci_destroy(void* plan) {
    aa::CiPlan* p = static_cast<aa::CiPlan*>(plan);
    if (!p) return AA_OK;
    if (p->d_tab) (void)hipFree(p->d_tab);
    if (p->d_window) (void)hipFree(p->d_window);
    delete p;
    return AA_OK;
}

extern "C" size_t aa_ci_workspace_bytes(const int64_t* lengths, int32_t n_rec) {
    if (!lengths || n_rec <= 0) return 0;
    const int64_t rows = aa::ci_rows(lengths, n_rec);
    return rows <= 0 ? 0 : (size_t)rows * AA_CI_BANDS * sizeof(double);
}

extern "C" int aa_ci_run(void* plan, const float* pcm16k, const int64_t* offsets, const int64_t* lengths,
                         int32_t n_rec, void* workspace, size_t workspace_bytes, double* bins_out,
                         int32_t* points_out, void* stream) {
    using namespace aa;
    CiPlan* p = static_cast<CiPlan*>(plan);
    AA_CHECK(p && pcm16k && offsets && lengths && points_out, AA_ERR_INVALID, "aa_ci_run: null argument");
    AA_CHECK(n_rec >= 0 && n_rec <= AA_CI_MAX_REC, AA_ERR_INVALID, "aa_ci_run: %d recordings (0..%d)", n_rec,
             AA_CI_MAX_REC);
    CiBatch B = {};
    B.n = n_rec;
    for (int b = 0; b <= CI_NB; ++b) B.edges[b] = p->edges[b];
    int64_t rows = 0, pts = 0;
    for (int32_t k = 0; k < n_rec; ++k) {
        AA_CHECK(offsets[k] >= 0, AA_ERR_INVALID, "aa_ci_run: recording %d starts at %lld", k, (long long)offsets[k]);
        AA_CHECK(lengths[k] >= 0 && lengths[k] <= AA_CI_MAX_SAMPLES, AA_ERR_INVALID,
                 "aa_ci_run: recording %d has %lld samples (0..%lld)", k, (long long)lengths[k],
                 (long long)AA_CI_MAX_SAMPLES);
        const int64_t F = ci_frames(lengths[k]);
        B.job[k].off = offsets[k];
        B.job[k].frames = (int)F;
        B.job[k].row0 = (int)rows;
        B.job[k].pt0 = (int)pts;
        rows += F;
        pts += F > 0 ? F - 1 : 0;
    }
    AA_CHECK(rows <= (int64_t)1 << 27, AA_ERR_INVALID, "aa_ci_run: %lld frames in one run (at most 2^27)",
             (long long)rows);
    B.rows = (int)rows;
    const size_t need = (size_t)rows * CI_NB * sizeof(double);
    double* bins = bins_out;
    if (!bins && rows > 0) {
        AA_CHECK(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, AA_ERR_WORKSPACE,
                 "aa_ci_run: workspace null or not 8-byte aligned");
        AA_CHECK(workspace_bytes >= need, AA_ERR_WORKSPACE, "aa_ci_run: workspace %zu < %zu bytes", workspace_bytes,
                 need);
        bins = static_cast<double*>(workspace);
    }
    AA_CHECK(p->d_tab && p->d_window, AA_ERR_INVALID, "aa_ci_run: a planned handle (aa_ci_plan) cannot run");
    if (rows == 0) return AA_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ci_bands, dim3((unsigned)rows), dim3(CI_T), 0, st, pcm16k, B, p->d_window, p->d_tab, bins);
    AA_LAUNCH_CHECK();
    if (pts > 0) {
        hipLaunchKernelGGL(ci_points, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, bins, B, points_out);
        AA_LAUNCH_CHECK();
    }
    return AA_OK;
}
