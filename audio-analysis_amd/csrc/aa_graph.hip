// CNN graphs: Keras Functional models that are not one conv chain --
// residual Add, squeeze-and-excite Multiply, DepthwiseConv2D, strided and
// "same"-padded convs, global average pooling -- i.e. the layer set of the
// EfficientNet route of classify() (reference src/identify_tracks.py:539-540;
// the CLI's default models /models/*/audioModel.keras, src/analyse.py:414-418,
// are whatever Keras graph the AI-Model release holds).
//
// Execution: the node list (include/aa.h aa_node, topological order) runs
// node by node over a batch of windows, each node's output an NHWC f32
// tensor in a workspace region reused once its last consumer has run
// (first-fit over the freed intervals).  Kernels:
//   conv (C_in >= 16, split-bf16)  gconv_x3t / gconv_x3p (aa_gconv.h, MFMA; split K: + gsplit_reduce)
//   conv (C_in < 16, or f32 mode)  gconv_f32_s / gconv_f32_lds / gconv_f32 (exact f32 FMA chains)
//   1x1 conv on a 1x1 map, dense   gmatvec / gmatvec_t
//   depthwise conv                 gdwconv (one lane per output pixel and 4 channels);
//                                  gdwconv_pool4 / gdwconv_pool with the global average pool that reads it
//   max / avg pool, global pools   gpool2d / ggpool4 / ggpool
//   add, broadcast multiply        gbinary
//   affine / activation / pow      gaffine / gpow
// every one with its activation fused.
//
// This file: the kernels, upload_graph, graph_run_node (a switch over the
// planned launch) and the entry points.  The plan itself -- shapes, weight
// images, fusions, launch variants, workspace offsets -- is made on the host
// by aa_graph_plan.h.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>

#include "aa_common.h"
#include "aa_gconv.h"
#include "aa_graph_plan.h"

namespace aa {

// depthwise conv: one lane per (output pixel, 4 channels) when C % 4 == 0
// (float4 taps and weights), else per (pixel, channel)
template <int V>
__global__ __launch_bounds__(256) void gdwconv(const float* __restrict__ in, const float* __restrict__ w,
                                               const float* __restrict__ bias, float* __restrict__ out, int Hin,
                                               int Win, int C, int Hout, int Wout, int kh, int kw, int sh, int sw,
                                               int pt, int pl, int act, float alpha) {
    typedef __attribute__((ext_vector_type(V))) float fv;
    const int CV = C / V;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (i >= (size_t)Hout * Wout * CV) return;
    const int c = (int)(i % CV) * V;
    const int P = (int)(i / CV);
    const int oy = P / Wout, ox = P - (P / Wout) * Wout;
    const float* img = in + (size_t)n * Hin * Win * C;
    fv acc;
    for (int e = 0; e < V; ++e) acc[e] = bias ? bias[c + e] : 0.f;
    for (int ky = 0; ky < kh; ++ky) {
        const int iy = oy * sh - pt + ky;
        if (iy < 0 || iy >= Hin) continue;
        for (int kx = 0; kx < kw; ++kx) {
            const int ix = ox * sw - pl + kx;
            if (ix < 0 || ix >= Win) continue;
            const fv wv = *reinterpret_cast<const fv*>(w + (ky * kw + kx) * C + c);
            const fv xv = *reinterpret_cast<const fv*>(img + ((size_t)iy * Win + ix) * C + c);
            for (int e = 0; e < V; ++e) acc[e] = fmaf(wv[e], xv[e], acc[e]);
        }
    }
    fv o;
    for (int e = 0; e < V; ++e) o[e] = gact(acc[e], act, alpha);
    *reinterpret_cast<fv*>(out + (size_t)n * Hout * Wout * C + (size_t)P * C + c) = o;
}

// global pool over H x W: a block per (window, 64 channels), 16 pixel
// stripes of 64 lanes (coalesced channel reads), each stripe summed in pixel
// order, the stripes combined by a fixed tree (deterministic: the same sums
// whatever the batch; gdwconv_pool reproduces this order exactly)
constexpr int GP_STRIPES = 16;
__device__ __forceinline__ float gpool_combine(float (*part)[64], int lane, int avg) {
    float v[GP_STRIPES];
#pragma unroll
    for (int i = 0; i < GP_STRIPES; ++i) v[i] = part[i][lane];
#pragma unroll
    for (int w = GP_STRIPES / 2; w >= 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) v[i] = avg ? v[i] + v[i + w] : fmaxf(v[i], v[i + w]);
    return v[0];
}

__global__ __launch_bounds__(64 * GP_STRIPES) void ggpool(const float* __restrict__ in, float* __restrict__ out,
                                                          int HW, int C, int avg, int act, float alpha) {
    __shared__ float part[GP_STRIPES][64];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int n = blockIdx.y;
    float m = avg ? 0.f : -INFINITY;
    if (c < C) {
        const float* p = in + (size_t)n * HW * C + c;
        for (int i = s; i < HW; i += GP_STRIPES) m = avg ? m + p[(size_t)i * C] : fmaxf(m, p[(size_t)i * C]);
    }
    part[s][lane] = m;
    __syncthreads();
    if (s == 0 && c < C) {
        float r = gpool_combine(part, lane, avg);
        if (avg) r = r / (float)HW;
        out[(size_t)n * C + c] = gact(r, act, alpha);
    }
}

// depthwise conv fused with the global average pool that reads it (the
// squeeze of squeeze-and-excite): ggpool's block shape, each lane computing
// its stripe's output pixels of one channel (exactly gdwconv's chain), storing
// them and summing them in ggpool's order -- the map and the pooled vector
// equal the unfused pair bit for bit.
__global__ __launch_bounds__(64 * GP_STRIPES) void gdwconv_pool(
    const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
    float* __restrict__ pooled, int Hin, int Win, int C, int Hout, int Wout, int kh, int kw, int sh, int sw, int pt,
    int pl, int act, float alpha, int pact, float palpha) {
    __shared__ float part[GP_STRIPES][64];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int n = blockIdx.y;
    const int HW = Hout * Wout;
    float m = 0.f;
    if (c < C) {
        const float* img = in + (size_t)n * Hin * Win * C + c;
        float* o = out + (size_t)n * HW * C + c;
        const float b = bias ? bias[c] : 0.f;
        for (int P = s; P < HW; P += GP_STRIPES) {
            const int oy = P / Wout, ox = P - (P / Wout) * Wout;
            float acc = b;
            for (int ky = 0; ky < kh; ++ky) {
                const int iy = oy * sh - pt + ky;
                if (iy < 0 || iy >= Hin) continue;
                for (int kx = 0; kx < kw; ++kx) {
                    const int ix = ox * sw - pl + kx;
                    if (ix < 0 || ix >= Win) continue;
                    acc = fmaf(w[(ky * kw + kx) * C + c], img[((size_t)iy * Win + ix) * C], acc);
                }
            }
            const float y = gact(acc, act, alpha);
            o[(size_t)P * C] = y;
            m += y;
        }
    }
    part[s][lane] = m;
    __syncthreads();
    if (s == 0 && c < C) pooled[(size_t)n * C + c] = gact(gpool_combine(part, lane, 1) / (float)HW, pact, palpha);
}

constexpr int GP4_STRIPES = 32;
// The same two kernels 4 channels per lane (C % 4 == 0): thread t of a block
// owns channel quad t % Q of the block's 4 Q channels and stripe t / Q
// (GP4_STRIPES stripes: twice the scalar kernels', for twice the waves on
// the small maps of a network's last stages).  Per channel the sum order is
// fixed (pixel order within a stripe, a fixed combine tree), the same in the
// pool and in the fused dwconv + pool: float4 loads give 16 lanes 256
// contiguous bytes per pixel.
// Stripe s sums the pixels p = s, s + GP4_STRIPES, ... of the map in row-major
// order (the order gdwconv_pool4 produces its pixels in, so a fused depthwise
// conv + pool and the two separate nodes give the same bits; every stripe
// gets HW / GP4_STRIPES pixels within one, whatever the map's width).
template <int Q>
__global__ __launch_bounds__(Q * GP4_STRIPES) void ggpool4(const float* __restrict__ in, float* __restrict__ out,
                                                         int H, int W, int C, int avg, int act, float alpha) {
    __shared__ float part[GP4_STRIPES][4 * Q];
    const int cq = threadIdx.x % Q, s = threadIdx.x / Q;
    const int c = blockIdx.x * 4 * Q + 4 * cq;
    const int n = blockIdx.y;
    const int HW = H * W;
    float4 m = avg ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (c < C) {
        const float* p = in + (size_t)n * HW * C + c;
        for (int px = s; px < HW; px += GP4_STRIPES) {
            const float4 v = *reinterpret_cast<const float4*>(p + (size_t)px * C);
            if (avg) { m.x += v.x; m.y += v.y; m.z += v.z; m.w += v.w; }
            else { m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w); }
        }
    }
    part[s][4 * cq] = m.x; part[s][4 * cq + 1] = m.y; part[s][4 * cq + 2] = m.z; part[s][4 * cq + 3] = m.w;
    __syncthreads();
    const int k = threadIdx.x;  // one channel of the block per thread
    if (k < 4 * Q && blockIdx.x * 4 * Q + k < C) {
        float v[GP4_STRIPES];
#pragma unroll
        for (int i = 0; i < GP4_STRIPES; ++i) v[i] = part[i][k];
#pragma unroll
        for (int w = GP4_STRIPES / 2; w >= 1; w >>= 1)
#pragma unroll
            for (int i = 0; i < w; ++i) v[i] = avg ? v[i] + v[i + w] : fmaxf(v[i], v[i + w]);
        float r = v[0];
        if (avg) r = r / (float)HW;
        out[(size_t)n * C + blockIdx.x * 4 * Q + k] = gact(r, act, alpha);
    }
}

// KS = 3: a 3x3 kernel, the taps unrolled and their weights held in
// registers for every pixel; KS = 0: any kernel, weights re-read per tap.
// Thread = (channel quad, stripe s): it computes the pixels p = s, s +
// GP4_STRIPES, ... in row-major order, so every stripe has HW / GP4_STRIPES
// pixels within one.  S = 1 or 2 (KS = 3, both strides S): R of the thread's
// pixels at a time, their 9 R taps loaded unconditionally from clamped
// addresses and zeroed by a value select (R = 1 by default: the fewest
// registers).  Round 5's column walk with a sliding 3 x 3 window was
// latency-bound -- one round trip per output row, 0.69-0.86 of the wave
// cycles parked on loads, its padding zeros read through flat loads from
// scratch, and on a 33-column map stripe 0 walked two columns while the
// others walked one (profiles/r05/pmc_ev2_top.txt).
template <int Q, int KS, int S = 0, int R = 1>
__global__ __launch_bounds__(Q * GP4_STRIPES) void gdwconv_pool4(
    const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
    float* __restrict__ pooled, int Hin, int Win, int C, int Hout, int Wout, int kh, int kw, int sh, int sw, int pt,
    int pl, int act, float alpha, int pact, float palpha) {
    static_assert(S == 0 || KS == 3, "chunked rows: 3x3 kernels");
    __shared__ float part[GP4_STRIPES][4 * Q];
    const int cq = threadIdx.x % Q, s = threadIdx.x / Q;
    const int c = blockIdx.x * 4 * Q + 4 * cq;
    const int n = blockIdx.y;
    const int HW = Hout * Wout;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) with_act(act, [&](auto actc) {
        constexpr int AV = decltype(actc)::value;
        const float* img = in + (size_t)n * Hin * Win * C + c;
        float* o = out + (size_t)n * HW * C + c;
        const float4 b = bias ? *reinterpret_cast<const float4*>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        constexpr int NW = KS ? KS * KS : 1;
        float4 wr[NW];  // the taps' weights of this lane's channels, held for every pixel
        if constexpr (KS > 0) {
#pragma unroll
            for (int t = 0; t < NW; ++t) wr[t] = *reinterpret_cast<const float4*>(w + t * C + c);
        }
        const int KH = KS ? KS : kh, KW = KS ? KS : kw;
        auto fma4 = [](float4& acc, const float4& wv, const float4& x) {
            acc.x = fmaf(wv.x, x.x, acc.x);
            acc.y = fmaf(wv.y, x.y, acc.y);
            acc.z = fmaf(wv.z, x.z, acc.z);
            acc.w = fmaf(wv.w, x.w, acc.w);
        };
        auto emit = [&](int oy, int ox, const float4& acc) {
            // no contraction of the activation's last product into the pool's
            // add: the pool sums the stored (rounded) outputs, as the unfused
            // ggpool4 does (with the activation a constant the compiler would
            // otherwise fuse swish's v * logistic(v) into an FMA with m)
#pragma clang fp contract(off)
            const float4 y = make_float4(gact(acc.x, AV, alpha), gact(acc.y, AV, alpha), gact(acc.z, AV, alpha),
                                         gact(acc.w, AV, alpha));
            *reinterpret_cast<float4*>(o + ((size_t)oy * Wout + ox) * C) = y;
            m.x += y.x; m.y += y.y; m.z += y.z; m.w += y.w;
        };
        if constexpr (S > 0) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float* imgw = in + (size_t)n * Hin * Win * C;
            for (int p0 = s; p0 < HW; p0 += GP4_STRIPES * R) {
                float4 x[R][9];
                int oyv[R], oxv[R];
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    const int p = p0 + u * GP4_STRIPES;
                    const bool pv = p < HW;
                    oyv[u] = pv ? p / Wout : 0;
                    oxv[u] = pv ? p - oyv[u] * Wout : 0;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            // a load from the clamped pixel, zeroed outside the image: a
                            // value select (a `cond ? *p : z` becomes a select of
                            // pointers -- flat loads, z in scratch)
                            const int iy = oyv[u] * S - pt + ky, ix = oxv[u] * S - pl + kx;
                            const int iyc = min(max(iy, 0), Hin - 1), ixc = min(max(ix, 0), Win - 1);
                            // (a 32-bit offset from the window's base: one VGPR per address)
                            const float4 t = *reinterpret_cast<const float4*>(
                                imgw + (uint32_t)((iyc * Win + ixc) * C + c));
                            x[u][ky * 3 + kx] = (pv && iy == iyc && ix == ixc) ? t : z;
                        }
                }
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    if (p0 + u * GP4_STRIPES >= HW) break;
                    float4 acc = b;
                    // padding taps add +0 * w: the same sum unless w is inf / nan
#pragma unroll
                    for (int t = 0; t < 9; ++t) fma4(acc, wr[t], x[u][t]);
                    emit(oyv[u], oxv[u], acc);
                }
            }
        } else {
            for (int p = s; p < HW; p += GP4_STRIPES) {
                const int oy = p / Wout, ox = p - oy * Wout;
                float4 acc = b;
                // (KS > 0: constant trip counts, unrolled by the compiler)
                for (int ky = 0; ky < KH; ++ky) {
                    const int iy = oy * sh - pt + ky;
                    if (iy < 0 || iy >= Hin) continue;
                    for (int kx = 0; kx < KW; ++kx) {
                        const int ix = ox * sw - pl + kx;
                        if (ix < 0 || ix >= Win) continue;
                        float4 wv;
                        if constexpr (KS > 0) wv = wr[ky * KS + kx];
                        else wv = *reinterpret_cast<const float4*>(w + (ky * kw + kx) * C + c);
                        fma4(acc, wv, *reinterpret_cast<const float4*>(img + ((size_t)iy * Win + ix) * C));
                    }
                }
                emit(oy, ox, acc);
            }
        }
    });
    part[s][4 * cq] = m.x; part[s][4 * cq + 1] = m.y; part[s][4 * cq + 2] = m.z; part[s][4 * cq + 3] = m.w;
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 4 * Q && blockIdx.x * 4 * Q + k < C) {
        float v[GP4_STRIPES];
#pragma unroll
        for (int i = 0; i < GP4_STRIPES; ++i) v[i] = part[i][k];
#pragma unroll
        for (int ww = GP4_STRIPES / 2; ww >= 1; ww >>= 1)
#pragma unroll
            for (int i = 0; i < ww; ++i) v[i] = v[i] + v[i + ww];
        pooled[(size_t)n * C + blockIdx.x * 4 * Q + k] = gact(v[0] / (float)HW, pact, palpha);
    }
}

// [n][K] x W[Cout][K] + bias: one wave per (window, output), lanes striding
// K by float4s, a fixed-order butterfly reduction (deterministic).  Dense
// layers, and 1x1 convs on 1x1 maps (the squeeze-and-excite reduce / expand).
__global__ __launch_bounds__(256) void gmatvec(const float* __restrict__ in, const float* __restrict__ w,
                                               const float* __restrict__ bias, float* __restrict__ out, int K,
                                               int Cout, int act, float alpha) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.y;
    if (o >= Cout) return;  // wave-uniform
    const float* x = in + (size_t)n * K;
    const float* wr = w + (size_t)o * K;
    float acc = 0.f;
    if ((K & 3) == 0) {
#pragma unroll 4
        for (int k = 4 * lane; k < K; k += 256) {
            const float4 a = *reinterpret_cast<const float4*>(x + k);
            const float4 b = *reinterpret_cast<const float4*>(wr + k);
            acc = fmaf(a.x, b.x, acc);
            acc = fmaf(a.y, b.y, acc);
            acc = fmaf(a.z, b.z, acc);
            acc = fmaf(a.w, b.w, acc);
        }
    } else {
        for (int k = lane; k < K; k += 64) acc = fmaf(x[k], wr[k], acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) {
        if (bias) acc += bias[o];
        out[(size_t)n * Cout + o] = gact(acc, act, alpha);
    }
}

// a (+|*) b; b_bcast: b is [n][C] broadcast over the pixels
__global__ __launch_bounds__(256) void gbinary(const float* __restrict__ a, const float* __restrict__ b,
                                               float* __restrict__ out, size_t per_win, int C, int mul,
                                               int b_bcast, int act, float alpha) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (i >= per_win) return;
    const size_t o = (size_t)n * per_win + i;
    const float y = b_bcast ? b[(size_t)n * C + (int)(i % C)] : b[o];
    out[o] = gact(mul ? a[o] * y : a[o] + y, act, alpha);
}

__global__ __launch_bounds__(256) void gaffine(const float* __restrict__ in, const float* __restrict__ scale,
                                               const float* __restrict__ shift, float* __restrict__ out,
                                               size_t total, int C, int act, float alpha) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    float v = in[i];
    if (scale) v = fmaf(v, scale[c], shift ? shift[c] : 0.f);
    else if (shift) v += shift[c];
    out[i] = gact(v, act, alpha);
}

__global__ __launch_bounds__(256) void gpow(const float* __restrict__ in, float* __restrict__ out, size_t total,
                                            float e) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out[i] = powf(in[i], e);
}

// [n][K] x W[K][Cout] + bias for short K: one thread per (window, output),
// lanes along the outputs (coalesced weight rows), the K products summed in
// order
__global__ __launch_bounds__(256) void gmatvec_t(const float* __restrict__ in, const float* __restrict__ w,
                                                 const float* __restrict__ bias, float* __restrict__ out, int K,
                                                 int Cout, int act, float alpha) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (o >= Cout) return;
    const float* x = in + (size_t)n * K;
    float acc = 0.f;
    // 16 products per round: all 32 loads issued (clamped indices, no
    // branches between them) before the round's FMAs -- one memory round trip
    // per 16 products instead of per 8; the same ordered chain
    for (int k0 = 0; k0 < K; k0 += 16) {
        float xv[16], wv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = min(k0 + u, K - 1);
            xv[u] = x[k];
            wv[u] = w[(size_t)k * Cout + o];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (k0 + u < K) acc = fmaf(xv[u], wv[u], acc);
    }
    if (bias) acc += bias[o];
    out[(size_t)n * Cout + o] = gact(acc, act, alpha);
}

__global__ __launch_bounds__(256) void gfinal(const float* __restrict__ x, float* __restrict__ logits,
                                              float* __restrict__ probs, size_t total, int sigmoid) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float v = x[i];
    logits[i] = v;
    if (probs) probs[i] = sigmoid ? 1.f / (1.f + expf(-v)) : v;
}

constexpr size_t AA_GRAPH_CAPTURES = 16;  // captured forwards kept per graph

// an instantiated forward that may still be executing from its last launch:
// wait for that launch before the executable goes
static void release_captured(Graph::Captured& c) {
    if (c.done) {
        (void)hipEventSynchronize(c.done);
        (void)hipEventDestroy(c.done);
    }
    if (c.exec) (void)hipGraphExecDestroy(c.exec);
    c.done = nullptr;
    c.exec = nullptr;
}

static void free_graph(Graph* g) {
    if (!g) return;
    for (auto& c : g->captured) release_captured(c);
    g->timer.release();
    if (g->uploaded)
        for (auto& nd : g->nodes) {
            (void)hipFree(nd.d_w);
            (void)hipFree(nd.d_b);
            (void)hipFree(nd.d_b2);
            (void)hipFree(nd.d_ws);
        }
    delete g;
}

// Copies every node's host images to the device and releases them (an empty
// image: the pointer stays null, which the kernels read as "absent").
static int upload_graph(Graph* G) {
    G->uploaded = true;  // from here on the nodes may own device memory
    auto put = [](auto** d, auto& h) -> int {
        const size_t bytes = h.size() * sizeof(h[0]);
        if (!bytes) return AA_OK;
        AA_HIP(hipMalloc((void**)d, bytes));
        AA_HIP(hipMemcpy(*d, h.data(), bytes, hipMemcpyHostToDevice));
        std::remove_reference_t<decltype(h)>().swap(h);
        return AA_OK;
    };
    for (GNode& N : G->nodes) {
        int rc = put(&N.d_w, N.h_w);
        if (rc == AA_OK) rc = put(&N.d_ws, N.h_ws);
        if (rc == AA_OK) rc = put(&N.d_b, N.h_b);
        if (rc == AA_OK) rc = put(&N.d_b2, N.h_b2);
        if (rc != AA_OK) return rc;
    }
    return AA_OK;
}

// What every launch of a node needs: its input a (of shape Hin x Win x Cin),
// its output, and the activation (the output node's sigmoid is applied by
// gfinal: logits before it).
struct NodeRun {
    const Graph& G;
    const GNode& N;
    const float* x;
    float* ws;
    int n;
    hipStream_t st;
    const float* a;
    float* out;
    int Hin, Win, Cin;
    int act;
    const float* buf(int k) const { return k < 0 ? x : ws + G.nodes[k].off * (size_t)n; }
};

// the split-bf16 MFMA convs: gconv_x3p and the gconv_x3t tile shapes
static int run_conv_mfma(const NodeRun& r) {
    const GNode& N = r.N;
    const aa_node& d = N.d;
    const int n = r.n, act = r.act;
    ConvGeom g = N.g;
    int nz = n, scale_hw = 0;
    if (is_pointwise(d)) {
        // pointwise: the n windows' pixels are one [1][n H W] image
        // (NHWC is [n][H][W][C] either way), so small maps fill whole
        // tiles; a squeeze-and-excite scale is looked up per pixel's window
        g.Hin = g.Hout = 1;
        g.Win = g.Wout = N.H * N.W * n;
        nz = 1;
        scale_hw = N.H * N.W;
    }
    constexpr int xo = 1;  // XCD-aware block order (aa_gconv.h xcd_order)
    const float* scl = N.scale_src >= 0 ? r.buf(N.scale_src) : nullptr;
    const float* res = N.res_src >= 0 ? r.buf(N.res_src) : nullptr;
    const int HWo = g.Hout * g.Wout;
    auto x3t = [&](auto kern, dim3 grid, int cslice, float* part) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, r.st, r.a, (const uint16_t*)N.d_w, N.d_b, r.out, g, N.cout_pad,
                           act, d.alpha, scl, res, scale_hw, cslice, part, xo);
    };
    const dim3 g64((HWo + 63) / 64, N.cout_pad / 64, nz);
    switch (N.kernel) {
        case AA_GK_X3P: {
            constexpr int TH = kPatchTH, TW = kPatchTW;
            const int tiles_w = (N.W + TW - 1) / TW, tiles_h = (N.H + TH - 1) / TH;
            const size_t lds = (size_t)((TH - 1) * d.sh + d.kh) * ((TW - 1) * d.sw + d.kw) * GX_ROW * 4;
            const dim3 grid((unsigned)(tiles_w * tiles_h), N.cout_pad / N.bn, n);
            hipLaunchKernelGGL((gconv_x3p<4, 1, 4, 1, 16>), grid, dim3(256), lds, r.st, r.a, (const uint16_t*)N.d_w,
                               N.d_b, r.out, g, N.cout_pad, act, d.alpha, TW, tiles_w, scl, res, xo);
            break;
        }
        case AA_GK_X3T_256x16:
            x3t(gconv_x3t<4, 1, 4, 1, 1, 1>, dim3((HWo + 255) / 256, N.cout_pad / 16, nz), 0, nullptr);
            break;
        case AA_GK_X3T_128x32:
            x3t(gconv_x3t<4, 1, 2, 2, 1, 1>, dim3((HWo + 127) / 128, N.cout_pad / 32, nz), 0, nullptr);
            break;
        case AA_GK_X3T_64x128:
            x3t(gconv_x3t<2, 2, 2, 4, 1, 1>, dim3((HWo + 63) / 64, N.cout_pad / 128, nz), 0, nullptr);
            break;
        case AA_GK_X3T_SPLIT_KC2:
        case AA_GK_X3T_SPLIT_KC1: {
            float* part = r.ws + r.G.part_off * (size_t)n;
            const dim3 grid((HWo + 63) / 64, N.cout_pad / 64, N.split);
            if (N.kernel == AA_GK_X3T_SPLIT_KC2) x3t(gconv_x3t<2, 2, 2, 2, 2, 1>, grid, N.cslice, part);
            else x3t(gconv_x3t<2, 2, 2, 2, 1, 1>, grid, N.cslice, part);
            AA_LAUNCH_CHECK();
            const size_t total = (size_t)HWo * N.C;
            hipLaunchKernelGGL(gsplit_reduce, dim3((unsigned)((total / 4 + 255) / 256 + 1)), dim3(256), 0, r.st, part,
                               N.split, total, N.C, N.d_b, res, r.out, act, d.alpha);
            break;
        }
        case AA_GK_X3T_64x64_KC2: x3t(gconv_x3t<2, 2, 2, 2, 2, 1>, g64, 0, nullptr); break;
        case AA_GK_X3T_64x64_PD2: x3t(gconv_x3t<2, 2, 2, 2, 1, 2>, g64, 0, nullptr); break;
        case AA_GK_X3T_64x64: x3t(gconv_x3t<2, 2, 2, 2, 1, 1>, g64, 0, nullptr); break;
        default: return AA_ERR_UNSUPPORTED;
    }
    return AA_OK;
}

// exact f32: matrix-vector products and the gconv_f32 family
static int run_conv_f32(const NodeRun& r) {
    const GNode& N = r.N;
    const aa_node& d = N.d;
    const int n = r.n;
    auto matvec = [&](auto kern, dim3 grid) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, r.st, r.a, (const float*)N.d_w, N.d_b, r.out, r.Cin, N.C, r.act,
                           d.alpha);
    };
    auto conv = [&](auto kern, const float* w, int cpb) {  // cpb: output channels per block
        hipLaunchKernelGGL(kern, dim3((N.H * N.W + 255) / 256, (N.C + cpb - 1) / cpb, n), dim3(256), 0, r.st, r.a, w,
                           N.d_b, r.out, N.g, r.act, d.alpha);
    };
    switch (N.kernel) {
        case AA_GK_MATVEC_T: matvec(gmatvec_t, dim3((N.C + 255) / 256, n)); break;
        case AA_GK_MATVEC: matvec(gmatvec, dim3((N.C + 3) / 4, n)); break;
        case AA_GK_F32_S: conv(gconv_f32_s<3, 3, 3>, N.d_ws, 32); break;
        case AA_GK_F32_LDS_3x3x3: conv(gconv_f32_lds<3, 3, 3>, (const float*)N.d_w, 32); break;
        case AA_GK_F32_LDS_3x3x1: conv(gconv_f32_lds<3, 3, 1>, (const float*)N.d_w, 32); break;
        case AA_GK_F32_LDS: conv(gconv_f32_lds<>, (const float*)N.d_w, 32); break;
        case AA_GK_F32: conv(gconv_f32, (const float*)N.d_w, 8); break;
        default: return AA_ERR_UNSUPPORTED;
    }
    return AA_OK;
}

static int run_dwconv(const NodeRun& r) {
    const GNode& N = r.N;
    const aa_node& d = N.d;
    const int n = r.n, Cin = r.Cin;
    const size_t per = (size_t)N.H * N.W * N.C;
    auto plain = [&](auto kern, int v) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((per / v + 255) / 256), n), dim3(256), 0, r.st, r.a,
                           (const float*)N.d_w, N.d_b, r.out, r.Hin, r.Win, Cin, N.H, N.W, d.kh, d.kw, d.sh, d.sw, d.pt,
                           d.pl, r.act, d.alpha);
    };
    // + the global average pool node it also writes; cpb: channels per block
    auto pooled = [&](auto kern, int cpb, int threads) {
        const GNode& P = r.G.nodes[N.pool_into];
        hipLaunchKernelGGL(kern, dim3((Cin + cpb - 1) / cpb, n), dim3(threads), 0, r.st, r.a, (const float*)N.d_w,
                           N.d_b, r.out, r.ws + P.off * (size_t)n, r.Hin, r.Win, Cin, N.H, N.W, d.kh, d.kw, d.sh, d.sw,
                           d.pt, d.pl, r.act, d.alpha, P.d.act, P.d.alpha);
    };
    constexpr int Q = 8;  // channel quads per gdwconv_pool4 block
    switch (N.kernel) {
        case AA_GK_DWPOOL4_S1: pooled(gdwconv_pool4<Q, 3, 1, 1>, 4 * Q, Q * GP4_STRIPES); break;
        case AA_GK_DWPOOL4_S2: pooled(gdwconv_pool4<Q, 3, 2, 1>, 4 * Q, Q * GP4_STRIPES); break;
        case AA_GK_DWPOOL4_K3: pooled(gdwconv_pool4<Q, 3, 0, 1>, 4 * Q, Q * GP4_STRIPES); break;
        case AA_GK_DWPOOL4: pooled(gdwconv_pool4<Q, 0, 0, 1>, 4 * Q, Q * GP4_STRIPES); break;
        case AA_GK_DWPOOL: pooled(gdwconv_pool, 64, 64 * GP_STRIPES); break;
        case AA_GK_DW4: plain(gdwconv<4>, 4); break;
        case AA_GK_DW1: plain(gdwconv<1>, 1); break;
        default: return AA_ERR_UNSUPPORTED;
    }
    return AA_OK;
}

// The launch planned for node N (aa_graph_plan.h choose_kernel): grids and
// arguments only.
static int graph_run_node(const Graph& G, const GNode& N, const float* x, float* ws, int n, hipStream_t st) {
    const aa_node& d = N.d;
    const GShape in = out_shape(G, d.in0);
    const bool last = &N == &G.nodes.back();
    NodeRun r{G, N, x, ws, n, st, nullptr, ws + N.off * (size_t)n, in.H, in.W, in.C,
              last && G.sigmoid_out ? AA_GACT_NONE : d.act};
    r.a = r.buf(d.in0);
    const float* a = r.a;
    float* out = r.out;
    const int Hin = in.H, Win = in.W, Cin = in.C, act = r.act;
    const size_t per = (size_t)N.H * N.W * N.C;
    int rc = AA_OK;
    switch (N.kernel) {
        case AA_GK_X3P:
        case AA_GK_X3T_256x16:
        case AA_GK_X3T_128x32:
        case AA_GK_X3T_64x128:
        case AA_GK_X3T_SPLIT_KC2:
        case AA_GK_X3T_SPLIT_KC1:
        case AA_GK_X3T_64x64_KC2:
        case AA_GK_X3T_64x64_PD2:
        case AA_GK_X3T_64x64: rc = run_conv_mfma(r); break;
        case AA_GK_MATVEC:
        case AA_GK_MATVEC_T:
        case AA_GK_F32_S:
        case AA_GK_F32_LDS_3x3x3:
        case AA_GK_F32_LDS_3x3x1:
        case AA_GK_F32_LDS:
        case AA_GK_F32: rc = run_conv_f32(r); break;
        case AA_GK_DWPOOL4_S1:
        case AA_GK_DWPOOL4_S2:
        case AA_GK_DWPOOL4_K3:
        case AA_GK_DWPOOL4:
        case AA_GK_DWPOOL:
        case AA_GK_DW4:
        case AA_GK_DW1: rc = run_dwconv(r); break;
        case AA_GK_POOL2D:
            hipLaunchKernelGGL(gpool2d, dim3((unsigned)((per + 255) / 256), n), dim3(256), 0, st, a, out, Hin, Win, Cin,
                               N.H, N.W, d.kh, d.kw, d.sh, d.sw, d.pt, d.pl, d.op == AA_G_AVGPOOL ? 1 : 0, act,
                               d.alpha);
            break;
        case AA_GK_GPOOL4:
            hipLaunchKernelGGL((ggpool4<16>), dim3((Cin + 63) / 64, n), dim3(16 * GP4_STRIPES), 0, st, a, out, Hin,
                               Win, Cin, d.op == AA_G_GAVGPOOL ? 1 : 0, act, d.alpha);
            break;
        case AA_GK_GPOOL:
            hipLaunchKernelGGL(ggpool, dim3((Cin + 63) / 64, n), dim3(64 * GP_STRIPES), 0, st, a, out, Hin * Win, Cin,
                               d.op == AA_G_GAVGPOOL ? 1 : 0, act, d.alpha);
            break;
        case AA_GK_BINARY: {
            const GNode* B = d.in1 >= 0 ? &G.nodes[d.in1] : nullptr;
            const int bc = B ? (B->H == 1 && B->W == 1 && (N.H != 1 || N.W != 1)) : 0;
            hipLaunchKernelGGL(gbinary, dim3((unsigned)((per + 255) / 256), n), dim3(256), 0, st, a, r.buf(d.in1), out,
                               per, N.C, d.op == AA_G_MUL ? 1 : 0, bc, act, d.alpha);
            break;
        }
        case AA_GK_AFFINE:
            hipLaunchKernelGGL(gaffine, dim3((unsigned)((per * n + 255) / 256)), dim3(256), 0, st, a, N.d_b, N.d_b2,
                               out, per * n, N.C, act, d.alpha);
            break;
        case AA_GK_POW:
            hipLaunchKernelGGL(gpow, dim3((unsigned)((per * n + 255) / 256)), dim3(256), 0, st, a, out, per * n,
                               d.alpha);
            break;
        case AA_GK_DENSE:
            hipLaunchKernelGGL(gmatvec, dim3((N.C + 3) / 4, n), dim3(256), 0, st, a, (const float*)N.d_w, N.d_b, out,
                               Hin * Win * Cin, N.C, act, d.alpha);
            break;
        default:
            return AA_ERR_UNSUPPORTED;
    }
    if (rc != AA_OK) return rc;
    AA_LAUNCH_CHECK();
    return AA_OK;
}

}  // namespace aa

using namespace aa;

extern "C" int aa_graph_create(const aa_node* nodes, int32_t n_nodes, const float* blob, int64_t blob_len,
                               int32_t in_h, int32_t in_w, int32_t in_c, int32_t precision, void** graph) {
    Graph* G = nullptr;
    int rc = plan_graph(nodes, n_nodes, blob, blob_len, in_h, in_w, in_c, precision, graph ? &G : nullptr);
    if (rc != AA_OK) return rc;
    rc = upload_graph(G);
    if (rc != AA_OK) {
        free_graph(G);
        return rc;
    }
    *graph = G;
    return AA_OK;
}

extern "C" int aa_graph_plan(const aa_node* nodes, int32_t n_nodes, const float* blob, int64_t blob_len, int32_t in_h,
                             int32_t in_w, int32_t in_c, int32_t precision, void** graph) {
    Graph* G = nullptr;
    const int rc = plan_graph(nodes, n_nodes, blob, blob_len, in_h, in_w, in_c, precision, graph ? &G : nullptr);
    if (rc == AA_OK) *graph = G;
    return rc;
}

extern "C" int aa_graph_node_plan(const void* graph, int32_t node, aa_node_plan* out) {
    const Graph* G = static_cast<const Graph*>(graph);
    AA_CHECK(G && out && node >= 0 && node < (int)G->nodes.size(), AA_ERR_INVALID, "aa_graph_node_plan: bad argument");
    const GNode& N = G->nodes[node];
    *out = aa_node_plan{N.H, N.W, N.C, N.kernel, N.bn, N.cout_pad, N.g.cin_pad, N.split, N.cslice, N.skip, N.nolaunch,
                        N.scale_src, N.res_src, N.pool_into, N.d.in0, N.d.in1, N.d.act, N.d.alpha, N.last_use,
                        (int64_t)N.off};
    return AA_OK;
}

extern "C" int aa_graph_plan_layout(const void* graph, aa_graph_layout* out) {
    const Graph* G = static_cast<const Graph*>(graph);
    AA_CHECK(G && out, AA_ERR_INVALID, "aa_graph_plan_layout: null argument");
    *out = aa_graph_layout{(int64_t)G->per_win, (int64_t)G->part_off, G->L, G->sigmoid_out};
    return AA_OK;
}

extern "C" int aa_graph_node_image(const void* graph, int32_t node, int32_t which, void* buf, size_t cap,
                                   size_t* len) {
    const Graph* G = static_cast<const Graph*>(graph);
    AA_CHECK(G && len && node >= 0 && node < (int)G->nodes.size() && which >= 0 && which <= 3, AA_ERR_INVALID,
             "aa_graph_node_image: bad argument");
    AA_CHECK(!G->uploaded, AA_ERR_UNSUPPORTED,
             "aa_graph_node_image: the host images are released once a graph is created; plan it (aa_graph_plan)");
    const GNode& N = G->nodes[node];
    const std::vector<float>& f = which == 1 ? N.h_b : which == 2 ? N.h_b2 : N.h_ws;
    const void* src = which == 0 ? (const void*)N.h_w.data() : (const void*)f.data();
    *len = which == 0 ? N.h_w.size() : f.size() * sizeof(float);
    if (!buf) return AA_OK;  // a size query
    AA_CHECK(cap >= *len, AA_ERR_INVALID, "aa_graph_node_image: buffer %zu < %zu", cap, *len);
    if (*len) memcpy(buf, src, *len);
    return AA_OK;
}

extern "C" int aa_graph_destroy(void* graph) {
    free_graph(static_cast<Graph*>(graph));
    return AA_OK;
}

extern "C" int aa_graph_n_outputs(const void* graph) { return graph ? static_cast<const Graph*>(graph)->L : -1; }

extern "C" size_t aa_graph_workspace_bytes(const void* graph, int32_t max_batch) {
    if (!graph || max_batch < 0) return 0;
    const Graph* G = static_cast<const Graph*>(graph);
    return align_up(G->per_win * 4 * (size_t)std::min<int32_t>(max_batch, 32768), 256);
}

// the forward's launches for n windows (<= 32768) on stream st
static int graph_enqueue(Graph* G, const float* x, int32_t n, float* logits, float* probs, float* ws,
                         hipStream_t st) {
    G->timer.mask = 0xFFFFFFFFu;  // the node filter is time_stage (graphs exceed 32 stages)
    for (size_t i = 0; i < G->nodes.size(); ++i) {
        if (G->nodes[i].skip || G->nodes[i].nolaunch) continue;
        const bool timed = G->time_stage == -1 || G->time_stage == (int)i;
        hipEvent_t e0 = nullptr;
        if (timed) {
            const int rc = G->timer.begin(0, st, &e0);
            if (rc != AA_OK) return rc;
        }
        const int rc = graph_run_node(*G, G->nodes[i], x, ws, n, st);
        if (rc != AA_OK) return rc;
        if (timed) {
            const int rc2 = G->timer.end((int)i, st, e0);
            if (rc2 != AA_OK) return rc2;
        }
    }
    const GNode& O = G->nodes.back();
    const size_t total = (size_t)G->L * n;
    hipLaunchKernelGGL(gfinal, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws + O.off * (size_t)n, logits,
                       probs, total, G->sigmoid_out);
    AA_LAUNCH_CHECK();
    return AA_OK;
}

extern "C" int aa_graph_forward(void* graph, const float* x, int32_t n, float* logits, float* probs, void* workspace,
                                size_t workspace_bytes, void* stream) {
    Graph* G = static_cast<Graph*>(graph);
    AA_CHECK(G && x && logits, AA_ERR_INVALID, "aa_graph_forward: null argument");
    AA_CHECK(G->uploaded, AA_ERR_INVALID, "aa_graph_forward: the graph is a plan (aa_graph_plan), not created");
    if (n <= 0) return AA_OK;
    constexpr int32_t CHUNK = 32768;  // grids carry the window in blockIdx.y / z
    const int32_t nc0 = std::min(n, CHUNK);
    AA_CHECK(workspace && workspace_bytes >= aa_graph_workspace_bytes(G, nc0), AA_ERR_WORKSPACE,
             "aa_graph_forward: workspace %zu < %zu", workspace_bytes, aa_graph_workspace_bytes(G, nc0));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const size_t in_per = (size_t)G->in_h * G->in_w * G->in_c;
    // replay a captured forward (not while timing nodes: the events would be
    // baked into the capture; not on the legacy null stream, which cannot capture)
    if (n <= CHUNK && G->time_stage == -2 && st != nullptr) {
        std::lock_guard<std::mutex> lk(G->cap_mu);
        auto same = [&](const Graph::Captured& c) {
            return c.x == x && c.n == n && c.ws == workspace && c.logits == logits && c.probs == probs && c.st == st;
        };
        for (const auto& c : G->captured)
            if (same(c)) {
                AA_HIP(hipGraphLaunch(c.exec, st));
                AA_HIP(hipEventRecord(c.done, st));
                return AA_OK;
            }
        bool again = false;
        for (auto it = G->seen.begin(); it != G->seen.end(); ++it)
            if (same(*it)) {
                again = true;
                G->seen.erase(it);
                break;
            }
        if (!again) {
            if (G->seen.size() >= AA_GRAPH_CAPTURES) G->seen.erase(G->seen.begin());
            G->seen.push_back(Graph::Captured{x, n, workspace, logits, probs, st, nullptr, nullptr});
            return graph_enqueue(G, x, n, logits, probs, ws, st);
        }
        // capture; if the stream cannot be captured (the runtime refuses, or the
        // caller's stream is itself capturing), launch node by node instead
        hipGraph_t hg = nullptr;
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            return graph_enqueue(G, x, n, logits, probs, ws, st);
        }
        const int rc = graph_enqueue(G, x, n, logits, probs, ws, st);
        const hipError_t ec = hipStreamEndCapture(st, &hg);
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = (rc == AA_OK && ec == hipSuccess) ? hipGraphInstantiate(&exec, hg, nullptr, nullptr, 0)
                                                                : hipErrorUnknown;
        if (hg) (void)hipGraphDestroy(hg);
        if (rc != AA_OK) return rc;  // a launch-configuration error: report it
        if (ei != hipSuccess) {
            (void)hipGetLastError();
            // (nothing ran during the capture attempt)
            return graph_enqueue(G, x, n, logits, probs, ws, st);
        }
        hipEvent_t done = nullptr;
        if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipGraphExecDestroy(exec);
            return graph_enqueue(G, x, n, logits, probs, ws, st);
        }
        if (G->captured.size() >= AA_GRAPH_CAPTURES) {  // bounded: the oldest goes
            release_captured(G->captured.front());
            G->captured.erase(G->captured.begin());
        }
        G->captured.push_back(Graph::Captured{x, n, workspace, logits, probs, st, exec, done});
        AA_HIP(hipGraphLaunch(exec, st));
        AA_HIP(hipEventRecord(done, st));
        return AA_OK;
    }
    for (int32_t c0 = 0; c0 < n; c0 += CHUNK) {
        const int32_t nc = std::min(CHUNK, n - c0);
        const int rc = graph_enqueue(G, x + (size_t)c0 * in_per, nc, logits + (size_t)c0 * G->L,
                                     probs ? probs + (size_t)c0 * G->L : nullptr, ws, st);
        if (rc != AA_OK) return rc;
    }
    return AA_OK;
}

extern "C" int aa_graph_n_stages(const void* graph) {
    return graph ? (int)static_cast<const Graph*>(graph)->nodes.size() : -1;
}

extern "C" int aa_graph_stage_info(const void* graph, int32_t stage, char* name, int32_t name_len,
                                   double* flops_per_item, double* bytes_per_item) {
    const Graph* G = static_cast<const Graph*>(graph);
    AA_CHECK(G && stage >= 0 && stage < (int)G->nodes.size(), AA_ERR_INVALID, "aa_graph_stage_info: bad stage");
    const GNode& N = G->nodes[stage];
    if (name && name_len > 0) snprintf(name, name_len, "%s", N.name.c_str());
    if (flops_per_item) *flops_per_item = N.flops;
    if (bytes_per_item) *bytes_per_item = N.bytes;
    return AA_OK;
}

// Node timing (the aa_model_stage_* contract, per node; a graph has more nodes
// than a 32-bit stage mask holds): set_timing(mask != 0) times every node,
// time_stage(k) only node k (-1 every node, -2 none).
extern "C" int aa_graph_set_timing(void* graph, uint32_t stage_mask) {
    Graph* G = static_cast<Graph*>(graph);
    AA_CHECK(G, AA_ERR_INVALID, "aa_graph_set_timing: null graph");
    G->time_stage = stage_mask ? -1 : -2;
    return AA_OK;
}

extern "C" int aa_graph_time_stage(void* graph, int32_t stage) {
    Graph* G = static_cast<Graph*>(graph);
    AA_CHECK(G && stage >= -2 && stage < (int)G->nodes.size(), AA_ERR_INVALID, "aa_graph_time_stage: bad stage");
    G->time_stage = stage;
    return AA_OK;
}

extern "C" int aa_graph_stage_time(void* graph, int32_t stage, double* total_ms, int64_t* count) {
    Graph* G = static_cast<Graph*>(graph);
    AA_CHECK(G && stage >= 0 && stage < (int)G->nodes.size(), AA_ERR_INVALID, "aa_graph_stage_time: bad stage");
    return G->timer.collect(stage, total_ms, count);
}
