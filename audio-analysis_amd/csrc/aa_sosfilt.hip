// Band-pass filtering of track spans on the device: scipy.signal.sosfilt as a
// chunked float64 scan (reference src/identify_tracks.py:152-162, :1036-1056).
//
// The cascade of second-order sections is a linear recurrence with the
// 4-vector state s = (z0, z1 of section 0, z0, z1 of section 1); a step with
// zero input is s <- P s.  One lane owns a chunk of L = AA_SOS_CHUNK samples,
// one workgroup 256 chunks (AA_SOS_BLOCK samples, staged through LDS):
//   sos_local   every lane runs its chunk from zero state and keeps the end
//               state e_c; the workgroup's inclusive scan of e (Kogge-Stone
//               over its 256 lanes, v_i += P^(L d) v_(i-d)) leaves the
//               workgroup's aggregate.
//   sos_carry   one workgroup per job scans the aggregates with P^(B 2^k)
//               into each workgroup's start state, 256 aggregates per round,
//               the last state of a round entering the next one's first lane.
//   sos_output  the scan of (start state, e_0, ..., e_254) is each chunk's
//               true start state; every lane reruns its chunk from it and
//               the f32 result leaves through LDS.
// Cross-workgroup values only ever pass between launches.
//
// The per-sample arithmetic is scipy's (_sosfilt.pyx), operation by
// operation, in round-to-nearest f64 without contraction (__dmul_rn /
// __dadd_rn), so a chunk run from the exact start state equals scipy bit for
// bit; the scans may fuse (they carry the rounding of the state hand-over
// either way).  A NaN enters every later chunk's start state through the
// scans (NaN * 0 is NaN) and none before it: lanes only ever read lower lanes.
#include <cmath>

#include "aa_common.h"

namespace aa {

constexpr int SOS_L = AA_SOS_CHUNK;
constexpr int SOS_T = 256;           // lanes (chunks) per workgroup
constexpr int SOS_B = AA_SOS_BLOCK;  // samples per workgroup
constexpr int SOS_ROW = SOS_L + 1;   // LDS row stride: lane t walks words t * 33 + i, bank (t + i) mod 32
constexpr int SOS_BLOCK_LEVEL = 8;   // pw level of P^B: B = L * 2^8
static_assert(SOS_B == SOS_L * SOS_T && SOS_T == 1 << SOS_BLOCK_LEVEL, "block span");
static_assert(SOS_BLOCK_LEVEL + 8 <= AA_SOS_LEVELS, "sos_carry scans 256 aggregates per round");
static_assert(SOS_T * SOS_ROW * sizeof(float) >= 8 * SOS_T * sizeof(double), "the scan reuses the sample tile");

// per job: e [blocks_max][256][4], aggregates [blocks_max][4], carries [blocks_max][4] (doubles)
__host__ __device__ static inline size_t sos_ws_doubles(long long n_jobs, long long blocks_max) {
    return (size_t)n_jobs * (size_t)blocks_max * (size_t)(SOS_T * 4 + 8);
}

__device__ __forceinline__ bool sos_job_ok(const aa_sos_job& J, long long n_pcm, long long max_n) {
    return J.n > 0 && J.n <= max_n && J.src >= 0 && J.dst >= 0 && J.src <= n_pcm - J.n && J.dst <= n_pcm - J.n &&
           (J.n_sections == 1 || J.n_sections == 2);
}

__device__ __forceinline__ int sos_idx(int i) { return i + i / SOS_L; }

// samples g[0, cnt) -> the padded tile; 16-byte loads from the first
// 16-B-aligned ADDRESS (a span starts at any sample), zeros to the end of the
// last chunk
__device__ __forceinline__ void sos_stage_in(const float* __restrict__ g, int cnt, float* xs) {
    const int tid = threadIdx.x;
    int head = (4 - (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3;
    if (head > cnt) head = cnt;
    const int n4 = (cnt - head) >> 2;
    if (tid < head) xs[sos_idx(tid)] = g[tid];
    const float4* q = reinterpret_cast<const float4*>(g + head);
    for (int v = tid; v < n4; v += SOS_T) {
        const float4 x = q[v];
        const int i = head + 4 * v;
        xs[sos_idx(i)] = x.x;
        xs[sos_idx(i + 1)] = x.y;
        xs[sos_idx(i + 2)] = x.z;
        xs[sos_idx(i + 3)] = x.w;
    }
    for (int i = head + 4 * n4 + tid; i < cnt; i += SOS_T) xs[sos_idx(i)] = g[i];
    const int end = (cnt + SOS_L - 1) / SOS_L * SOS_L;
    for (int i = cnt + tid; i < end; i += SOS_T) xs[sos_idx(i)] = 0.f;
}

__device__ __forceinline__ void sos_stage_out(float* __restrict__ g, int cnt, const float* xs) {
    const int tid = threadIdx.x;
    int head = (4 - (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3;
    if (head > cnt) head = cnt;
    const int n4 = (cnt - head) >> 2;
    if (tid < head) g[tid] = xs[sos_idx(tid)];
    float4* q = reinterpret_cast<float4*>(g + head);
    for (int v = tid; v < n4; v += SOS_T) {
        const int i = head + 4 * v;
        q[v] = make_float4(xs[sos_idx(i)], xs[sos_idx(i + 1)], xs[sos_idx(i + 2)], xs[sos_idx(i + 3)]);
    }
    for (int i = head + 4 * n4 + tid; i < cnt; i += SOS_T) g[i] = xs[sos_idx(i)];
}

// scipy's step (_sosfilt.pyx), sample outer, section inner; c = b0 b1 b2 -a1 -a2
// (x - a y == x + (-a) y exactly: negation commutes with rounding)
template <int NS>
__device__ __forceinline__ double sos_step(const double (&c)[NS][5], double (&z)[NS][2], double x) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const double y = __dadd_rn(__dmul_rn(c[s][0], x), z[s][0]);
        z[s][0] = __dadd_rn(__dadd_rn(__dmul_rn(c[s][1], x), __dmul_rn(c[s][3], y)), z[s][1]);
        z[s][1] = __dadd_rn(__dmul_rn(c[s][2], x), __dmul_rn(c[s][4], y));
        x = y;
    }
    return x;
}

template <int NS>
__device__ __forceinline__ void sos_coeffs(const aa_sos_job& J, double (&c)[NS][5]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        c[s][0] = J.sos[6 * s];
        c[s][1] = J.sos[6 * s + 1];
        c[s][2] = J.sos[6 * s + 2];
        c[s][3] = -J.sos[6 * s + 4];
        c[s][4] = -J.sos[6 * s + 5];
    }
}

// lane's chunk from state v (in: start state, out: end state); STORE: the f32
// output replaces the samples in the tile
template <int NS, bool STORE>
__device__ __forceinline__ void sos_chunk(const aa_sos_job& J, float* row, double (&v)[4]) {
    double c[NS][5], z[NS][2];
    sos_coeffs<NS>(J, c);
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s][0] = v[2 * s], z[s][1] = v[2 * s + 1];
#pragma unroll 8
    for (int i = 0; i < SOS_L; ++i) {
        const double y = sos_step<NS>(c, z, (double)row[i]);
        if (STORE) row[i] = (float)y;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) v[2 * s] = z[s][0], v[2 * s + 1] = z[s][1];
}

// v += M u (M row-major 4 x 4, workgroup-uniform)
__device__ __forceinline__ void sos_mac(double (&v)[4], const double* __restrict__ M, const double (&u)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double a = v[r];
#pragma unroll
        for (int k = 0; k < 4; ++k) a = fma(M[4 * r + k], u[k], a);
        v[r] = a;
    }
}

// Inclusive scan over the workgroup's lanes: v_i = sum_{j <= i} (M_0)^(i - j) v_j,
// Kogge-Stone over all 256 lanes with the levels M_k = (M_0)^(2^k) at
// pw + 16 k.  Every level passes through LDS (lane i - d may sit in another
// wave); sc holds two buffers of 4 * 256 doubles used in turn, so one barrier
// per level orders both the reads after the writes and the next writes to the
// same buffer (two levels on) after the reads.  Only lanes < count matter, so
// levels of distance >= count are skipped.  Ends on a barrier.
__device__ __forceinline__ void sos_scan(double (&v)[4], const double* __restrict__ pw, double* sc, int count) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < SOS_BLOCK_LEVEL; ++k) {
        const int d = 1 << k;
        if (d >= count) break;
        double* b = sc + (k & 1) * 4 * SOS_T;
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j * SOS_T + tid] = v[j];
        __syncthreads();
        if (tid >= d) {
            double u[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = b[j * SOS_T + tid - d];
            sos_mac(v, pw + 16 * k, u);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(SOS_T) void sos_local(const float* __restrict__ pcm, long long n_pcm,
                                                   const aa_sos_job* __restrict__ jobs, long long max_n,
                                                   int blocks_max, double* __restrict__ ws_e,
                                                   double* __restrict__ ws_agg) {
    __shared__ __align__(16) float xs[SOS_T * SOS_ROW];
    const aa_sos_job& J = jobs[blockIdx.y];
    if (!sos_job_ok(J, n_pcm, max_n)) return;
    const long long b0 = (long long)blockIdx.x * SOS_B;
    if (b0 >= J.n) return;
    const int cnt = (int)(J.n - b0 < SOS_B ? J.n - b0 : SOS_B);
    const int tid = threadIdx.x;
    sos_stage_in(pcm + J.src + b0, cnt, xs);
    __syncthreads();
    double v[4] = {0., 0., 0., 0.};
    if (tid * SOS_L < cnt) {  // a chunk of zeros from zero state ends in zero state
        if (J.n_sections == 2) sos_chunk<2, false>(J, xs + tid * SOS_ROW, v);
        else sos_chunk<1, false>(J, xs + tid * SOS_ROW, v);
    }
    const size_t blk = (size_t)blockIdx.y * blocks_max + blockIdx.x;
    double2* e = reinterpret_cast<double2*>(ws_e + (blk * SOS_T + tid) * 4);
    e[0] = make_double2(v[0], v[1]);
    e[1] = make_double2(v[2], v[3]);
    if (b0 + SOS_B >= J.n) return;  // the last workgroup's aggregate has no reader
    __syncthreads();                // the tile becomes the scan's exchange buffer
    sos_scan(v, J.pw, reinterpret_cast<double*>(xs), SOS_T);
    if (tid == SOS_T - 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ws_agg[blk * 4 + j] = v[j];
    }
}

// start state of workgroup b: S_b = P^B S_(b-1) + A_(b-1), S_0 = 0
__global__ __launch_bounds__(SOS_T) void sos_carry(const aa_sos_job* __restrict__ jobs, long long n_pcm,
                                                   long long max_n, int blocks_max,
                                                   const double* __restrict__ ws_agg, double* __restrict__ ws_carry) {
    __shared__ double sc[8 * SOS_T];
    __shared__ double last[4];
    const aa_sos_job& J = jobs[blockIdx.x];
    if (!sos_job_ok(J, n_pcm, max_n)) return;
    const int nb = (int)((J.n + SOS_B - 1) / SOS_B);
    const int tid = threadIdx.x;
    const double* pw = J.pw + 16 * SOS_BLOCK_LEVEL;
    const size_t base = (size_t)blockIdx.x * blocks_max;
    double prev[4] = {0., 0., 0., 0.};
    for (int t0 = 0; t0 < nb; t0 += SOS_T) {
        const int i = t0 + tid;
        double w[4] = {0., 0., 0., 0.};
        if (i >= 1 && i < nb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = ws_agg[(base + i - 1) * 4 + j];
        }
        if (tid == 0 && t0 > 0) sos_mac(w, pw, prev);
        sos_scan(w, pw, sc, nb - t0 < SOS_T ? nb - t0 : SOS_T);
        if (i < nb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ws_carry[(base + i) * 4 + j] = w[j];
        }
        if (tid == SOS_T - 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) last[j] = w[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) prev[j] = last[j];
    }
}

__global__ __launch_bounds__(SOS_T) void sos_output(float* __restrict__ pcm, long long n_pcm,
                                                    const aa_sos_job* __restrict__ jobs, long long max_n,
                                                    int blocks_max, const double* __restrict__ ws_e,
                                                    const double* __restrict__ ws_carry) {
    __shared__ __align__(16) float xs[SOS_T * SOS_ROW];
    const aa_sos_job& J = jobs[blockIdx.y];
    if (!sos_job_ok(J, n_pcm, max_n)) return;
    const long long b0 = (long long)blockIdx.x * SOS_B;
    if (b0 >= J.n) return;
    const int cnt = (int)(J.n - b0 < SOS_B ? J.n - b0 : SOS_B);
    const int tid = threadIdx.x;
    const size_t blk = (size_t)blockIdx.y * blocks_max + blockIdx.x;
    // s_i = P^L s_(i-1) + e_(i-1): the inclusive scan of (S_b, e_0, ..., e_254)
    double v[4] = {0., 0., 0., 0.};
    if (tid > 0) {
        const double2* e = reinterpret_cast<const double2*>(ws_e + (blk * SOS_T + tid - 1) * 4);
        const double2 a = e[0], b = e[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else if (blockIdx.x > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ws_carry[blk * 4 + j];
    }
    sos_scan(v, J.pw, reinterpret_cast<double*>(xs), (cnt + SOS_L - 1) / SOS_L);
    sos_stage_in(pcm + J.src + b0, cnt, xs);
    __syncthreads();
    if (tid * SOS_L < cnt) {
        if (J.n_sections == 2) sos_chunk<2, true>(J, xs + tid * SOS_ROW, v);
        else sos_chunk<1, true>(J, xs + tid * SOS_ROW, v);
    }
    __syncthreads();
    sos_stage_out(pcm + J.dst + b0, cnt, xs);
}

// one step of the state with zero input, in the kernel's arithmetic (this
// file is built without contraction)
static void sos_host_zero_step(const double* sos, int ns, double* s) {
    double x = 0.;
    for (int k = 0; k < ns; ++k) {
        const double* c = sos + 6 * k;
        const double y = c[0] * x + s[2 * k];
        s[2 * k] = (c[1] * x - c[4] * y) + s[2 * k + 1];
        s[2 * k + 1] = c[2] * x - c[5] * y;
        x = y;
    }
}

static void sos_square(long double* a) {
    long double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            long double t = 0;
            for (int k = 0; k < 4; ++k) t += a[4 * i + k] * a[4 * k + j];
            r[4 * i + j] = t;
        }
    for (int i = 0; i < 16; ++i) a[i] = r[i];
}

}  // namespace aa

extern "C" int aa_sosfilt_plan(const double* sos, int32_t n_sections, int64_t src, int64_t n, int64_t dst,
                               aa_sos_job* job) {
    AA_CHECK(sos && job, AA_ERR_INVALID, "aa_sosfilt_plan: null argument");
    AA_CHECK(n_sections >= 1 && n_sections <= AA_SOS_MAX_SECTIONS, AA_ERR_INVALID,
             "aa_sosfilt_plan: n_sections %d not in 1..%d", n_sections, AA_SOS_MAX_SECTIONS);
    AA_CHECK(n >= 0 && n <= AA_SOS_MAX_N, AA_ERR_INVALID, "aa_sosfilt_plan: n %lld not in 0..%lld", (long long)n,
             (long long)AA_SOS_MAX_N);
    AA_CHECK(src >= 0 && dst >= 0, AA_ERR_INVALID, "aa_sosfilt_plan: negative offset");
    for (int i = 0; i < 6 * n_sections; ++i)
        AA_CHECK(std::isfinite(sos[i]), AA_ERR_INVALID, "aa_sosfilt_plan: coefficient %d of section %d is not finite",
                 i % 6, i / 6);
    for (int s = 0; s < n_sections; ++s)
        AA_CHECK(sos[6 * s + 3] == 1.0, AA_ERR_INVALID, "aa_sosfilt_plan: a0 of section %d is %g, not 1", s,
                 sos[6 * s + 3]);
    aa_sos_job J = {};
    J.src = src, J.n = n, J.dst = dst;
    J.n_sections = n_sections, J.n_levels = AA_SOS_LEVELS;
    for (int i = 0; i < 6 * n_sections; ++i) J.sos[i] = sos[i];
    long double a[16];
    for (int j = 0; j < 4; ++j) {  // column j: the unit state e_j after one step
        double s[4] = {0., 0., 0., 0.};
        s[j] = 1.;
        if (j < 2 * n_sections) aa::sos_host_zero_step(sos, n_sections, s);
        else s[j] = 0.;  // no such section: its state stays zero
        for (int i = 0; i < 4; ++i) J.p[4 * i + j] = s[i], a[4 * i + j] = s[i];
    }
    for (int l = 1; l < AA_SOS_CHUNK; l *= 2) aa::sos_square(a);  // P^L
    for (int k = 0; k < AA_SOS_LEVELS; ++k) {
        for (int i = 0; i < 16; ++i) {
            const double d = (double)a[i];
            AA_CHECK(std::isfinite(d), AA_ERR_INVALID, "aa_sosfilt_plan: unstable filter (P^(%d 2^%d) overflows)",
                     AA_SOS_CHUNK, k);
            J.pw[16 * k + i] = d;
        }
        aa::sos_square(a);
    }
    *job = J;
    return AA_OK;
}

extern "C" size_t aa_sosfilt_workspace_bytes(const aa_sos_job* jobs_host, int32_t n_jobs) {
    if (!jobs_host || n_jobs <= 0) return 0;
    int64_t max_n = 0;
    for (int32_t i = 0; i < n_jobs; ++i)
        if (jobs_host[i].n > max_n) max_n = jobs_host[i].n;
    if (max_n > AA_SOS_MAX_N) max_n = AA_SOS_MAX_N;
    return aa::sos_ws_doubles(n_jobs, (max_n + aa::SOS_B - 1) / aa::SOS_B) * sizeof(double);
}

extern "C" int aa_sosfilt_run(float* pcm, int64_t n_pcm, const aa_sos_job* jobs_dev, int32_t n_jobs, int64_t max_n,
                              void* workspace, size_t workspace_bytes, void* stream) {
    AA_CHECK(pcm && jobs_dev, AA_ERR_INVALID, "aa_sosfilt_run: null argument");
    AA_CHECK(n_jobs >= 0 && n_jobs <= 65535, AA_ERR_INVALID, "aa_sosfilt_run: n_jobs %d not in 0..65535", n_jobs);
    AA_CHECK(n_pcm >= 0 && max_n >= 0, AA_ERR_INVALID, "aa_sosfilt_run: negative size");
    if (n_jobs == 0 || max_n == 0) return AA_OK;
    AA_CHECK(max_n <= AA_SOS_MAX_N, AA_ERR_INVALID, "aa_sosfilt_run: max_n %lld > %lld", (long long)max_n,
             (long long)AA_SOS_MAX_N);
    AA_CHECK(max_n <= n_pcm, AA_ERR_INVALID, "aa_sosfilt_run: a job of %lld samples is outside the %lld of pcm",
             (long long)max_n, (long long)n_pcm);
    const int blocks_max = (int)((max_n + aa::SOS_B - 1) / aa::SOS_B);
    const size_t need = aa::sos_ws_doubles(n_jobs, blocks_max) * sizeof(double);
    AA_CHECK(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, AA_ERR_INVALID,
             "aa_sosfilt_run: workspace null or not 16-byte aligned");
    AA_CHECK(workspace_bytes >= need, AA_ERR_WORKSPACE, "aa_sosfilt_run: workspace %zu < %zu bytes", workspace_bytes,
             need);
    double* ws_e = static_cast<double*>(workspace);
    double* ws_agg = ws_e + (size_t)n_jobs * blocks_max * aa::SOS_T * 4;
    double* ws_carry = ws_agg + (size_t)n_jobs * blocks_max * 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks_max, (unsigned)n_jobs);
    hipLaunchKernelGGL(aa::sos_local, grid, dim3(aa::SOS_T), 0, st, pcm, (long long)n_pcm, jobs_dev, (long long)max_n,
                       blocks_max, ws_e, ws_agg);
    AA_LAUNCH_CHECK();
    if (blocks_max > 1) {
        hipLaunchKernelGGL(aa::sos_carry, dim3((unsigned)n_jobs), dim3(aa::SOS_T), 0, st, jobs_dev, (long long)n_pcm,
                           (long long)max_n, blocks_max, ws_agg, ws_carry);
        AA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(aa::sos_output, grid, dim3(aa::SOS_T), 0, st, pcm, (long long)n_pcm, jobs_dev,
                       (long long)max_n, blocks_max, ws_e, ws_carry);
    AA_LAUNCH_CHECK();
    return AA_OK;
}
