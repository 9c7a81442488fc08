// Planner of the graph models: the aa_node list -> nodes with their shapes,
// packed weight images, fusions, launch variants and workspace offsets, host
// only (no HIP call), so a graph can be planned and inspected on a machine
// without a GPU (aa_graph_plan / aa_graph_node_plan / aa_graph_node_image).
// Included by aa_graph.hip after aa_gconv.h: it reads that header's ConvGeom
// and limits (gconv_bn, gconv_x3p_fits, GF32_KMAX) and packs with
// aa_cnn_pack.h.
//
// plan_graph runs, in this order: plan_node per node (validation, shape
// inference, weight images, name / flops / bytes), graph_fuse (three passes),
// choose_kernel per node, assign_workspace.  upload_graph and graph_run_node
// (aa_graph.hip) only copy the images and launch what was chosen here.
#pragma once

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "aa_cnn_pack.h"

namespace aa {

struct GNode {
    aa_node d;
    int H = 0, W = 0, C = 0;  // output shape
    int kernel = 0;           // aa_gkernel: the launch of this node (choose_kernel)
    int mfma = 0;             // conv on the split-bf16 MFMA kernels
    int matvec = 0;           // 1x1 conv on a 1x1 map, or Dense: 1 gmatvec on W[Cout][K], 2 gmatvec_t on W[K][Cout]
    int bn = 64;              // its tile's output channels (16, 32, 64)
    int split = 1, cslice = 0;  // pointwise conv on a small map: K split into `split` slices of cslice chunks
    ConvGeom g{};
    int cout_pad = 0;
    // host images (plan_node), released once upload_graph has copied them; an
    // empty image leaves its device pointer null (no bias, no affine scale ..)
    std::vector<uint8_t> h_w;
    std::vector<float> h_b;   // bias; affine: scale
    std::vector<float> h_b2;  // affine shift
    std::vector<float> h_ws;  // f32 stem: weights [C_out / 32][K][32] for the scalar path (gconv_f32_s)
    void* d_w = nullptr;
    float* d_b = nullptr;
    float* d_b2 = nullptr;
    float* d_ws = nullptr;
    size_t off = 0;           // workspace offset (f32 elements per window)
    // fusions (graph_fuse): a skipped node launches nothing; a conv may read
    // a squeeze-and-excite scale [n][Cin] (the Multiply it replaces) and add a
    // residual map (the Add it replaces) in its epilogue
    bool skip = false;        // fused into a consumer: no launch, no buffer
    bool nolaunch = false;    // written by its producer's launch (a pool fused into a dwconv)
    int scale_src = -2, res_src = -2;
    int pool_into = -2;       // dwconv: the global average pool node it also writes
    int last_use = 0;
    std::string name;
    double flops = 0, bytes = 0;
};

struct Graph {
    int prec = AA_PREC_BF16X3;
    int in_h = 0, in_w = 0, in_c = 0;
    bool uploaded = false;  // false: a plan (aa_graph_plan), host images and no device memory
    std::vector<GNode> nodes;
    size_t per_win = 0;  // workspace f32 elements per window
    size_t part_off = 0; // split-K partial sums (per window, after the node buffers)
    int L = 0;
    int sigmoid_out = 0;
    // HIP events around node launches (aa_graph_set_timing / aa_graph_time_stage):
    // time_stage -1 every node, >= 0 that node only, -2 none
    int time_stage = -2;
    StageTimer timer;
    // the forward's launches captured into HIP graphs, one per (input,
    // batch, workspace, outputs, stream): a graph model issues one launch per
    // node (~180 for an EfficientNetV2-B0), which from the host costs about
    // as much as the kernels take on the device; a replay is one launch
    struct Captured {
        const float* x;
        int n;
        void* ws;
        float* logits;
        float* probs;
        hipStream_t st;
        hipGraphExec_t exec;
        hipEvent_t done;  // recorded after every launch of exec: it may still run when evicted
    };
    std::vector<Captured> captured;
    std::vector<Captured> seen;  // keys met once (captured the second time: a caller
                                 // that allocates its outputs per call never pays a capture)
    std::mutex cap_mu;
};

struct GShape {
    int H, W, C;
};

static GShape out_shape(const Graph& G, int k) {
    if (k < 0) return {G.in_h, G.in_w, G.in_c};
    return {G.nodes[k].H, G.nodes[k].W, G.nodes[k].C};
}

// the weight blob: n floats at off, or null when they lie outside it
struct GBlob {
    const float* p;
    int64_t len;
    const float* get(int64_t off, int64_t n) const {
        if (off < 0 || n < 0 || off + n > len) return nullptr;
        return p + off;
    }
};

static const char* gop_name(int op) {
    switch (op) {
        case AA_G_CONV: return "conv";
        case AA_G_DWCONV: return "dwconv";
        case AA_G_MAXPOOL: return "maxpool";
        case AA_G_AVGPOOL: return "avgpool";
        case AA_G_GMAXPOOL: return "gmaxpool";
        case AA_G_GAVGPOOL: return "gavgpool";
        case AA_G_ADD: return "add";
        case AA_G_MUL: return "mul";
        case AA_G_AFFINE: return "affine";
        case AA_G_DENSE: return "dense";
        case AA_G_POW: return "pow";
        default: return "?";
    }
}

// a 1x1 stride-1 unpadded conv: the n windows' pixels run as one [1][n H W]
// image (graph_run_node), and on a small map its K may be split
static bool is_pointwise(const aa_node& d) {
    return d.kh == 1 && d.kw == 1 && d.sh == 1 && d.sw == 1 && d.pt == 0 && d.pl == 0;
}

// a pointwise conv over >= 384 channels on a small map (<= kSplitHW pixels
// per window) is a short grid of long K loops: its K is split over blocks
// (a shape-only choice: the sums do not depend on n)
constexpr int kSplitHW = 128;
static void choose_split(GNode& N) {
    if (!(N.mfma && is_pointwise(N.d) && N.H * N.W <= kSplitHW)) return;
    const int ncc = N.g.cin_pad / 32;
    for (int cs : {6, 7, 4, 5, 8, 9})
        if (ncc >= 12 && ncc % cs == 0) {
            N.split = ncc / cs;
            N.cslice = cs;
            break;
        }
}

static std::string gname(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static std::string gname(const char* fmt, ...) {
    char nm[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(nm, sizeof nm, fmt, ap);
    va_end(ap);
    return nm;
}

static void set_bias(std::vector<float>& h, size_t len, const float* b, int n) {
    h.assign(len, 0.f);
    if (b) std::copy(b, b + n, h.begin());
}

static int plan_conv(int prec, int i, GNode& N, GShape in, const GBlob& blob) {
    const aa_node& d = N.d;
    const int C = in.C;
    AA_CHECK(d.filters >= 1, AA_ERR_INVALID, "node %d: filters", i);
    N.C = d.filters;
    const int ntap = d.kh * d.kw, K = ntap * C;
    const float* k = blob.get(d.off[0], (int64_t)K * d.filters);
    AA_CHECK(k, AA_ERR_INVALID, "node %d: conv kernel outside the blob", i);
    const float* b = d.off[1] >= 0 ? blob.get(d.off[1], d.filters) : nullptr;
    AA_CHECK(d.off[1] < 0 || b, AA_ERR_INVALID, "node %d: bias outside the blob", i);
    N.g = ConvGeom{in.H, in.W, C, N.H, N.W, N.C, d.kh, d.kw, d.sh, d.sw, d.pt, d.pl, (C + 31) / 32 * 32};
    // a 1x1 conv on a 1x1 map is a matrix-vector product per window
    // (squeeze-and-excite): exact f32 on gmatvec, not a 64-pixel MFMA tile
    N.matvec = in.H == 1 && in.W == 1 && d.kh == 1 && d.kw == 1 && d.pt == 0 && d.pl == 0;
    N.mfma = prec == AA_PREC_BF16X3 && C >= 16 && !N.matvec;
    if (N.mfma) {
        N.bn = gconv_bn(N.C);
        N.cout_pad = (N.C + N.bn - 1) / N.bn * N.bn;
        N.h_w = as_bytes(gconv_pack_x3(keras_to_tco(k, ntap, C, N.C), ntap, N.C, C, N.cout_pad, N.g.cin_pad));
        set_bias(N.h_b, N.cout_pad, b, N.C);
    } else {
        // [Cout][K]; a matrix-vector product with K <= 64 keeps the
        // Keras [K][Cout] order (gmatvec_t: one thread per output)
        if (N.matvec && K <= 64) N.matvec = 2;
        N.h_w = as_bytes(N.matvec == 2 ? keras_as_is(k, K, N.C) : keras_to_ok(k, K, N.C));
        if (d.kh == 3 && d.kw == 3 && C == 3) N.h_ws = pack_stem_f32(k, K, N.C);  // the scalar-path stem layout
        set_bias(N.h_b, N.C, b, N.C);
    }
    N.flops = 2.0 * N.H * N.W * K * N.C;
    N.bytes = 4.0 * (in.H * in.W * C + N.H * N.W * N.C);
    choose_split(N);
    N.name = gname("%s_%dx%d_s%d_%d_%d", N.mfma ? "conv_gx3" : N.matvec ? "matvec" : "conv_gf32", d.kh, d.kw, d.sh, C,
                   N.C);
    return AA_OK;
}

static int plan_dwconv(int i, GNode& N, GShape in, const GBlob& blob) {
    const aa_node& d = N.d;
    const int C = in.C;
    N.C = C;
    const float* k = blob.get(d.off[0], (int64_t)d.kh * d.kw * C);
    AA_CHECK(k, AA_ERR_INVALID, "node %d: depthwise kernel outside the blob", i);
    const float* b = d.off[1] >= 0 ? blob.get(d.off[1], C) : nullptr;
    AA_CHECK(d.off[1] < 0 || b, AA_ERR_INVALID, "node %d: bias outside the blob", i);
    N.h_w = as_bytes(std::vector<float>(k, k + (size_t)d.kh * d.kw * C));
    if (b) N.h_b.assign(b, b + C);
    N.flops = 2.0 * N.H * N.W * d.kh * d.kw * C;
    N.bytes = 4.0 * (in.H * in.W * C + N.H * N.W * N.C);
    N.name = gname("dwconv_%dx%d_s%d_%d", d.kh, d.kw, d.sh, C);
    return AA_OK;
}

static int plan_affine(int i, GNode& N, GShape in, const GBlob& blob) {
    const aa_node& d = N.d;
    const int C = in.C;
    N.H = in.H; N.W = in.W; N.C = C;
    if (d.off[0] >= 0) {
        const float* sc = blob.get(d.off[0], C);
        AA_CHECK(sc, AA_ERR_INVALID, "node %d: scale outside the blob", i);
        N.h_b.assign(sc, sc + C);
    }
    if (d.off[1] >= 0) {
        const float* sh = blob.get(d.off[1], C);
        AA_CHECK(sh, AA_ERR_INVALID, "node %d: shift outside the blob", i);
        N.h_b2.assign(sh, sh + C);
    }
    N.bytes = 8.0 * in.H * in.W * C;
    N.name = gname("affine_%d", C);
    return AA_OK;
}

static int plan_dense(int i, GNode& N, GShape in, const GBlob& blob) {
    const aa_node& d = N.d;
    AA_CHECK(d.filters >= 1, AA_ERR_INVALID, "node %d: units", i);
    const int K = in.H * in.W * in.C;
    const float* k = blob.get(d.off[0], (int64_t)K * d.filters);
    AA_CHECK(k, AA_ERR_INVALID, "node %d: dense kernel outside the blob", i);
    const float* b = d.off[1] >= 0 ? blob.get(d.off[1], d.filters) : nullptr;
    AA_CHECK(d.off[1] < 0 || b, AA_ERR_INVALID, "node %d: bias outside the blob", i);
    N.h_w = as_bytes(keras_to_ok(k, K, d.filters));  // [Cout][K] for gmatvec
    if (b) N.h_b.assign(b, b + d.filters);
    N.matvec = 1;
    N.H = N.W = 1;
    N.C = d.filters;
    N.flops = 2.0 * K * d.filters;
    N.bytes = 4.0 * (K + (double)K * d.filters + d.filters);
    N.name = gname("dense_%d_%d", K, d.filters);
    return AA_OK;
}

// Node i of the table: validation, output shape, weight images, name and the
// algorithmic flops / bytes per window.
static int plan_node(Graph& G, int i, const GBlob& blob) {
    GNode& N = G.nodes[i];
    const aa_node& d = N.d;
    AA_CHECK(d.in0 >= -1 && d.in0 < i && d.in1 >= -1 && d.in1 < i, AA_ERR_INVALID,
             "aa_graph_create: node %d reads a later node", i);
    AA_CHECK(d.act >= AA_GACT_NONE && d.act <= AA_GACT_SWISH, AA_ERR_INVALID, "node %d: activation %d", i, d.act);
    const GShape in = out_shape(G, d.in0);
    const int H = in.H, W = in.W, C = in.C;
    const bool windowed = d.op == AA_G_CONV || d.op == AA_G_DWCONV || d.op == AA_G_MAXPOOL || d.op == AA_G_AVGPOOL;
    if (windowed) {
        AA_CHECK(d.kh >= 1 && d.kw >= 1 && d.sh >= 1 && d.sw >= 1 && d.pt >= 0 && d.pb >= 0 && d.pl >= 0 &&
                     d.pr >= 0, AA_ERR_INVALID, "node %d: window / strides / pads", i);
        N.H = (H + d.pt + d.pb - d.kh) / d.sh + 1;
        N.W = (W + d.pl + d.pr - d.kw) / d.sw + 1;
        AA_CHECK(H + d.pt + d.pb >= d.kh && W + d.pl + d.pr >= d.kw, AA_ERR_INVALID,
                 "node %d: input %dx%d smaller than the window", i, H, W);
    }
    int rc = AA_OK;
    switch (d.op) {
        case AA_G_CONV: rc = plan_conv(G.prec, i, N, in, blob); break;
        case AA_G_DWCONV: rc = plan_dwconv(i, N, in, blob); break;
        case AA_G_MAXPOOL:
        case AA_G_AVGPOOL:
            N.C = C;
            N.bytes = 4.0 * (H * W * C + N.H * N.W * N.C);
            N.name = gname("%s_%dx%d_s%d_%d", gop_name(d.op), d.kh, d.kw, d.sh, C);
            break;
        case AA_G_GMAXPOOL:
        case AA_G_GAVGPOOL:
            N.H = N.W = 1;
            N.C = C;
            N.bytes = 4.0 * (H * W * C + C);
            N.name = gname("%s_%d", gop_name(d.op), C);
            break;
        case AA_G_ADD:
        case AA_G_MUL: {
            const GShape b = out_shape(G, d.in1);
            const bool same = b.H == H && b.W == W && b.C == C;
            const bool bc = d.op == AA_G_MUL && b.H == 1 && b.W == 1 && b.C == C;
            AA_CHECK(same || bc, AA_ERR_UNSUPPORTED, "node %d: %s of %dx%dx%d and %dx%dx%d", i, gop_name(d.op), H, W,
                     C, b.H, b.W, b.C);
            N.H = H; N.W = W; N.C = C;
            N.bytes = 4.0 * (2 * H * W * C + H * W * C);
            N.name = gname("%s_%d", gop_name(d.op), C);
            break;
        }
        case AA_G_AFFINE: rc = plan_affine(i, N, in, blob); break;
        case AA_G_POW:
            N.H = H; N.W = W; N.C = C;
            N.bytes = 8.0 * H * W * C;
            N.name = gname("pow_%d", C);
            break;
        case AA_G_DENSE: rc = plan_dense(i, N, in, blob); break;
        default:
            AA_CHECK(false, AA_ERR_UNSUPPORTED, "node %d: op %d", i, d.op);
    }
    if (rc != AA_OK) return rc;
    AA_CHECK(N.H >= 1 && N.W >= 1 && N.C >= 1, AA_ERR_INVALID, "node %d: empty output", i);
    return AA_OK;
}

// ---- fusions (bit-identical to the unfused graph: the fused kernel computes
// the same f32 products and sums in the same order) -------------------------
// uses[k]: the readers of node k in the table as given (not updated between
// the passes).

// Multiply(x [H][W][C], s [1][1][C]) whose only consumer is an MFMA conv: the
// conv scales its input channels while staging (squeeze-and-excite)
static void fuse_se_scale(std::vector<GNode>& nodes, const std::vector<int>& uses) {
    const int n = (int)nodes.size();
    for (int i = 0; i < n - 1; ++i) {
        GNode& M = nodes[i];
        if (M.d.op != AA_G_MUL || M.d.act != AA_GACT_NONE || uses[i] != 1 || M.d.in1 < 0) continue;
        const GNode& S = nodes[M.d.in1];
        if (!(S.H == 1 && S.W == 1 && (M.H != 1 || M.W != 1))) continue;
        for (int j = i + 1; j < n; ++j) {
            GNode& K = nodes[j];
            if (K.d.in0 != i && K.d.in1 != i) continue;
            if (K.d.op == AA_G_CONV && K.mfma && K.d.in0 == i && K.scale_src == -2) {
                K.d.in0 = M.d.in0;
                K.scale_src = M.d.in1;
                M.skip = true;
            }
            break;
        }
    }
}

// Add(conv, r) where the conv has no activation and no other consumer and r
// is computed before the conv: the conv adds r in its epilogue and applies
// the add's activation (the residual of an inverted-bottleneck block)
static void fuse_residual_add(Graph& G, const std::vector<int>& uses) {
    std::vector<GNode>& nodes = G.nodes;
    const int n = (int)nodes.size();
    for (int i = 0; i < n - 1; ++i) {
        GNode& A = nodes[i];
        if (A.d.op != AA_G_ADD || A.d.in1 < 0) continue;
        for (int side = 0; side < 2; ++side) {
            const int x = side ? A.d.in1 : A.d.in0, r = side ? A.d.in0 : A.d.in1;
            if (x < 0) continue;
            GNode& X = nodes[x];
            if (X.d.op != AA_G_CONV || !X.mfma || X.skip || X.d.act != AA_GACT_NONE || uses[x] != 1 ||
                X.res_src != -2 || r >= x)
                continue;
            const GShape R = out_shape(G, r);
            // (the graph input is not a workspace buffer)
            if (!(R.H == X.H && R.W == X.W && R.C == X.C) || r < 0) continue;
            X.res_src = r;
            X.d.act = A.d.act;
            X.d.alpha = A.d.alpha;
            X.bytes += 4.0 * X.H * X.W * X.C;
            X.name += "+add";
            A.skip = true;
            for (GNode& N : nodes) {  // the add's readers read the conv
                if (N.d.in0 == i) N.d.in0 = x;
                if (N.d.in1 == i) N.d.in1 = x;
            }
            break;
        }
    }
}

// a depthwise conv followed at once by the global average pool of its output
// (the squeeze of squeeze-and-excite): one launch writes both
static void fuse_dw_pool(std::vector<GNode>& nodes) {
    const int n = (int)nodes.size();
    for (int i = 0; i + 1 < n; ++i) {
        GNode& D = nodes[i];
        GNode& P = nodes[i + 1];
        if (D.d.op == AA_G_DWCONV && P.d.op == AA_G_GAVGPOOL && P.d.in0 == i && i + 1 != n - 1) {
            D.pool_into = i + 1;
            P.nolaunch = true;
            D.name += "+gap";
        }
    }
}

static void graph_fuse(Graph& G) {
    std::vector<int> uses(G.nodes.size(), 0);
    for (const GNode& N : G.nodes)
        for (int k : {N.d.in0, N.d.in1})
            if (k >= 0) ++uses[k];
    fuse_se_scale(G.nodes, uses);
    fuse_residual_add(G, uses);
    fuse_dw_pool(G.nodes);
    for (GNode& N : G.nodes) {
        if (N.scale_src >= 0) N.name += "+se";
        for (bool fused : {N.nolaunch, N.skip})
            if (fused) {
                N.name += "(fused)";
                N.flops = N.bytes = 0;
            }
    }
}

// ---- kernel variants --------------------------------------------------------
// Tile and kernel choices of the graph's convs, fixed from in-pipeline A/B
// runs (rounds 4-5; the rejected alternatives are no longer built):
//  * 64 x 128 gconv_x3t tiles for short-K convs with C_out a multiple of 128,
//    1x1 and larger kernels (42.3k -> 43.2k audio-s/s on the EfficientNetV2
//    graph; 3x3 32->128 160 -> 147 us, profiles/r04/graph_ab_xcd.txt);
//    128 x 64 tiles measured slower;
//  * KC <= 2 chunks per K step (KC = 4 halves the blocks per CU);
//  * two K steps in flight in the one-chunk 64 x 64 launches over >= 8 chunks
//    (the 672 -> 112 project convs 46 -> 42 us; 3 steps and 64 / 128 x 224 /
//    192 / 112 pointwise tiles slower, profiles/r05/graph_ab_pw.txt);
//  * the depthwise conv + pool at 8 channel quads per 256-thread block and one
//    pixel's taps per load batch (dwconv stages 526 -> 363 us against round
//    5's column walk; 2 / 3 pixels 390 / 436 us, profiles/r05/graph_ab_dw.txt);
//  * XCD-aware block order (stage sum 3016 -> 2923 us, graph_ab_xcd.txt);
//  * gconv_x3p (patch-staged) for kernels > 1x1 at C_out <= 16 on 256-pixel
//    tiles (3x3/32->16 212 -> 149 us); 128-pixel tiles and the stride-1
//    patch + weight-ring kernel at 64 channels measured slower.

// gconv_x3p's output tile (256 pixels)
constexpr int kPatchTH = 16, kPatchTW = 16;

static int conv_kernel(const GNode& N, int Cin) {
    const aa_node& d = N.d;
    if (N.matvec) return N.matvec == 2 ? AA_GK_MATVEC_T : AA_GK_MATVEC;
    if (!N.mfma) {
        if (d.kh * d.kw * Cin > GF32_KMAX) return AA_GK_F32;
        if (!N.h_ws.empty()) return AA_GK_F32_S;  // an RGB-style stem, weights through the scalar cache
        if (d.kh == 3 && d.kw == 3 && Cin == 3) return AA_GK_F32_LDS_3x3x3;
        if (d.kh == 3 && d.kw == 3 && Cin == 1) return AA_GK_F32_LDS_3x3x1;
        return AA_GK_F32_LDS;
    }
    // kernels larger than 1x1 with C_out <= 16: the patch-staged kernel when
    // every patch pixel is staged (GX_P_STG items per thread) and its patch
    // fits 64 KiB (two blocks per CU at least); otherwise gconv_x3t.
    // (Measured on the EfficientNetV2 graph: 3x3/32->16 212 -> 149 us; at 64
    // channels per block it lost -- 3x3/32->128 161 -> 178, 3x3/2 16->64 97 ->
    // 176 us -- its per-tap B loads from L2 stall the short tap loop:
    // gconv_x3t keeps those.)
    if (N.bn == 16)
        return d.kh * d.kw > 1 && gconv_x3p_fits((kPatchTH - 1) * d.sh + d.kh, (kPatchTW - 1) * d.sw + d.kw)
                   ? AA_GK_X3P
                   : AA_GK_X3T_256x16;
    if (N.bn == 32) return AA_GK_X3T_128x32;
    // 64 x 128 tiles: half the re-reads of the pixel tile
    if (N.C >= 128 && N.g.cin_pad <= 256 && N.cout_pad % 128 == 0) return AA_GK_X3T_64x128;
    // split K: slices of cslice chunks on blockIdx.z, then the ordered sum
    if (N.split > 1) return N.cslice % 2 == 0 ? AA_GK_X3T_SPLIT_KC2 : AA_GK_X3T_SPLIT_KC1;
    // 64 x 64 tiles, KC 32-channel chunks per K step (the same products
    // summed in the same order whatever KC is)
    const int ncc = N.g.cin_pad / 32;
    if (ncc % 2 == 0) return AA_GK_X3T_64x64_KC2;
    return ncc >= 8 ? AA_GK_X3T_64x64_PD2 : AA_GK_X3T_64x64;
}

static int dwconv_kernel(const GNode& N, int Cin) {
    const aa_node& d = N.d;
    const bool quad = (Cin & 3) == 0;
    if (N.pool_into < 0) return quad ? AA_GK_DW4 : AA_GK_DW1;
    if (!quad) return AA_GK_DWPOOL;
    const bool k3 = d.kh == 3 && d.kw == 3;
    if (k3 && d.sh == d.sw && d.sh == 1) return AA_GK_DWPOOL4_S1;
    if (k3 && d.sh == d.sw && d.sh == 2) return AA_GK_DWPOOL4_S2;
    return k3 ? AA_GK_DWPOOL4_K3 : AA_GK_DWPOOL4;
}

// the launch of a node, from its shape alone (after the fusions: a depthwise
// conv's depends on pool_into)
static int choose_kernel(const Graph& G, const GNode& N) {
    const int Cin = out_shape(G, N.d.in0).C;
    switch (N.d.op) {
        case AA_G_CONV: return conv_kernel(N, Cin);
        case AA_G_DWCONV: return dwconv_kernel(N, Cin);
        case AA_G_MAXPOOL:
        case AA_G_AVGPOOL: return AA_GK_POOL2D;
        case AA_G_GMAXPOOL:
        case AA_G_GAVGPOOL: return (Cin & 3) == 0 ? AA_GK_GPOOL4 : AA_GK_GPOOL;
        case AA_G_ADD:
        case AA_G_MUL: return AA_GK_BINARY;
        case AA_G_AFFINE: return AA_GK_AFFINE;
        case AA_G_POW: return AA_GK_POW;
        default: return AA_GK_DENSE;  // (plan_node refused every other op)
    }
}

// ---- workspace ----------------------------------------------------------------
// per-window size rounded up to 16 floats: every buffer starts 64-B aligned,
// so the float4 loads / stores of the kernels never straddle
static size_t node_elems(const GNode& N) { return align_up((size_t)N.H * N.W * N.C, 16); }

typedef std::vector<std::pair<size_t, size_t>> GIntervals;  // [begin, end) of buffers in use

static size_t first_fit(GIntervals& live, size_t sz) {
    std::sort(live.begin(), live.end());
    size_t at = 0;
    for (auto& iv : live) {
        if (iv.first >= at + sz) break;
        at = std::max(at, iv.second);
    }
    live.emplace_back(at, at + sz);
    return at;
}

static void release(GIntervals& live, const GNode& N) {
    auto it = std::find(live.begin(), live.end(), std::make_pair(N.off, N.off + node_elems(N)));
    if (it != live.end()) live.erase(it);
}

// Liveness (a node's buffer is free after its last reader; the output
// survives the forward) and first-fit offsets; then the split-K partial sums
// after the node buffers.  Fused-away nodes own no buffer; a pool written by
// its depthwise conv is allocated with that conv.
static void assign_workspace(std::vector<GNode>& nodes, size_t* part_off, size_t* per_win) {
    const int n = (int)nodes.size(), last = n - 1;
    auto inputs = [](const GNode& N) { return std::array<int, 4>{N.d.in0, N.d.in1, N.scale_src, N.res_src}; };
    for (int i = 0; i < n; ++i) nodes[i].last_use = i;
    for (int i = 0; i < n; ++i) {
        if (nodes[i].skip || nodes[i].nolaunch) continue;
        for (int k : inputs(nodes[i]))
            if (k >= 0) nodes[k].last_use = std::max(nodes[k].last_use, i);
    }
    nodes[last].last_use = n;
    GIntervals live;
    size_t peak = 0;
    for (int i = 0; i < n; ++i) {
        GNode& N = nodes[i];
        if (N.skip || N.nolaunch) continue;
        N.off = first_fit(live, node_elems(N));
        peak = std::max(peak, N.off + node_elems(N));
        if (N.pool_into >= 0) {
            GNode& P = nodes[N.pool_into];
            P.off = first_fit(live, node_elems(P));
            peak = std::max(peak, P.off + node_elems(P));
        }
        for (int k : inputs(N))  // release the inputs whose last use is this node
            if (k >= 0 && nodes[k].last_use == i) release(live, nodes[k]);
        if (N.last_use == i && i != last) release(live, N);  // a node nobody reads (a dangling branch)
    }
    *part_off = (peak + 63) / 64 * 64;
    size_t part = 0;
    for (const GNode& N : nodes)
        if (N.split > 1 && !N.skip) part = std::max(part, (size_t)N.split * N.H * N.W * N.C);
    *per_win = *part_off + (part + 63) / 64 * 64;
}

// The arguments of aa_graph_create -> a Graph whose nodes hold their host
// images (no device memory).  On failure *out is untouched and the reason is
// in aa_last_error.
static int plan_graph(const aa_node* nodes, int32_t n_nodes, const float* blob, int64_t blob_len, int32_t in_h,
                      int32_t in_w, int32_t in_c, int32_t precision, Graph** out) {
    AA_CHECK(nodes && blob && out && n_nodes > 0, AA_ERR_INVALID, "aa_graph_create: null argument");
    AA_CHECK(precision == AA_PREC_BF16X3 || precision == AA_PREC_F32, AA_ERR_UNSUPPORTED,
             "aa_graph_create: graphs run in split-bf16 or f32 (precision %d)", precision);
    AA_CHECK(in_h >= 1 && in_w >= 1 && in_c >= 1, AA_ERR_INVALID, "aa_graph_create: input shape");
    Graph* G = new Graph();
    G->prec = precision;
    G->in_h = in_h;
    G->in_w = in_w;
    G->in_c = in_c;
    G->nodes.resize(n_nodes);
    for (int i = 0; i < n_nodes; ++i) {
        G->nodes[i].d = nodes[i];
        const int rc = plan_node(*G, i, GBlob{blob, blob_len});
        if (rc != AA_OK) {
            delete G;
            return rc;
        }
    }
    if (getenv("AA_GRAPH_NOFUSE") == nullptr) graph_fuse(*G);
    for (GNode& N : G->nodes) N.kernel = choose_kernel(*G, N);
    assign_workspace(G->nodes, &G->part_off, &G->per_win);
    const GNode& O = G->nodes.back();
    G->L = O.H * O.W * O.C;
    G->sigmoid_out = O.d.act == AA_GACT_SIGMOID;
    *out = G;
    return AA_OK;
}

}  // namespace aa
