// Planner of the window-classifier CNN: the Keras-style layer list -> stages
// with their packed weight images, host only (no HIP call), so a plan can be
// made and inspected on a machine without a GPU (aa_model_plan /
// aa_model_stage_image).  Included by aa_cnn.hip after the kernel headers: it
// reads their layout constants (conv_cstr, conv_k128, F8_BSTR, wg_g, TAIL_NW)
// and the tile tables (aa_cnn_tiles.h), and packs with aa_cnn_pack.h.
//
// plan_model folds each BatchNormalization into the preceding conv, fuses the
// activation and a following max-pool into the conv's epilogue, and the final
// 1x1 conv + GlobalMaxPool2D + sigmoid into one head stage; then the fusion
// passes (first conv, split hand-off, tail) run over the stage vector, the
// ping-pong workspace is sized, and the 3x3 conv pairs that run as one launch
// within that workspace are marked (mark_pairs).
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "aa_cnn_pack.h"
#include "aa_cnn_tiles.h"

namespace aa {

// ST_SMALL: C_in = 1 3x3 -> 32 first conv (VALU, fusable into the next
// stage); ST_MFMA: tuned matrix-core conv; ST_HEAD: 1x1 conv + global max;
// ST_GENERIC: any other conv shape / pool window (f32 VALU fallback);
// ST_POOLDENSE: GlobalMaxPool2D [+ Dense] [+ sigmoid] after a conv stage;
// ST_GCONV: split-bf16 mode, a conv with C_in >= 16 and no tuned tile: the
// runtime-shaped MFMA kernel gconv_x3 (aa_gconv.h) [+ gpool2d for the max pool]
enum StageKind { ST_SMALL = 0, ST_MFMA = 1, ST_HEAD = 2, ST_GENERIC = 3, ST_POOLDENSE = 4, ST_GCONV = 5 };

struct Stage {
    int kind = ST_MFMA;
    int kh = 1, kw = 1, cin = 0, cout = 0, cout_pad = 0;
    int pool = 1;        // square pool window of the tuned kernels (1 or 3), 0 otherwise
    int ph = 1, pw = 1;  // max-pool window (= strides)
    int act = ACT_NONE;
    float alpha = 0.f;
    int has_mag = 0;
    float mag_exp = 1.f;
    int sigmoid = 0;
    int Hin = 0, Win = 0, Hc = 0, Wc = 0, Hout = 0, Wout = 0;
    // host images (plan_model), released once upload_model has copied them:
    // packed weights (empty: pool_dense without a Dense reads a null pointer),
    // bias [+ fp8 dequantisation scales], the fused tail's head weights
    std::vector<uint8_t> h_w, h_tw;
    std::vector<uint8_t> h_f1;  // split-bf16 fused_first: the first conv's per-lane image (pack_first_lanes)
    std::vector<float> h_b;
    int layer_end = 0;  // index of the first layer after this stage's group
    void* d_w = nullptr;
    float* d_b = nullptr;
    double flops = 0, bytes = 0;  // algorithmic per window
    std::string name;
    int skipped = 0;    // first layer computed inside the next stage
    int is_first = 0;   // reads the model input (f32 log-mel)
    int fused_first = 0;  // this stage computes the previous (first) layer itself
    int lm_f16 = 0;       // fused_first: the model input is float16
    int in_split = 0;     // split-bf16: input / output in the grouped-split layout (aa_conv_x3.h)
    int out_split = 0;
    int wg = 0;           // split-bf16 Winograd F(wg, 3)-along-W kernel (aa_conv_wg.h, wg = WO) and its weight packing
    int wg_npass = 1;     // its staging passes (planes per pass = (wg + 2) / wg_npass)
    int cin_pad = 0;      // ST_GCONV: C_in rounded up to 32
    int tail = 0;         // ST_HEAD, split-bf16: computes the previous conv stage itself (aa_conv_tail.h)
    void* d_f1 = nullptr;
    void* d_tw = nullptr;  // tail: head weights packed per wave / label fragment, hi then lo
    int pair = 0;         // split-bf16: a full forward computes the previous stage inside this one (aa_conv_pair.h)
};

struct Model {
    int prec = AA_PREC_BF16;
    int in_h = 0, in_w = 0, in_c = 0;
    int L = 0;
    bool uploaded = false;  // false: a plan (aa_model_plan), host images and no device memory
    std::vector<Stage> st;
    size_t act_elems[2] = {0, 0};  // per-window elements of the ping-pong buffers
    size_t tmp_elems = 0;          // per-window f32 elements of an ST_GCONV stage's unpooled output
    StageTimer timer;  // HIP events around the stages in timer.mask
};

// bytes of one stored activation (split-bf16 keeps f32 activations)
static size_t prec_bytes(int prec) { return prec == AA_PREC_FP8 ? 1 : prec == AA_PREC_BF16 ? 2 : 4; }

// The layer list being consumed: cursor, running activation shape, and a
// MagTransform waiting for the first conv.
struct LayerCursor {
    const aa_layer* layers;
    int n_layers;
    const float* blob;
    int64_t blob_len;
    int prec;
    int i = 0;
    int H = 0, W = 0, C = 0;
    int has_mag = 0;
    float mag_exp = 1.f;

    const float* get(int64_t off, int64_t n) const {
        if (off < 0 || off + n > blob_len) return nullptr;
        return blob + off;
    }
    bool at(int op) const { return i < n_layers && layers[i].op == op; }
    int fail(int code, const char* msg) const {
        set_error("aa_model_create: layer %d: %s", i, msg);
        return code;
    }
};

// a conv's raw kernel [kh][kw][cin][cout] and the per-channel affine that
// follows it (bias and folded BatchNorm): y = scale * conv + shift
struct Fold {
    const float* kern = nullptr;
    std::vector<double> scale, shift;
};

static std::string pool_suffix(const Stage& s) {
    char pl[24] = "";
    if (s.ph > 1 || s.pw > 1) snprintf(pl, sizeof pl, s.ph == s.pw ? "_pool%d" : "_pool%dx%d", s.ph, s.pw);
    return pl;
}

// GlobalMaxPool2D [+ Dense] [+ sigmoid] after a conv stage: one pool_dense
// launch (the 1x1-conv head pattern is folded by classify_conv)
static int plan_pooldense(LayerCursor& p, Stage& s) {
    const int C = p.C;
    s.kind = ST_POOLDENSE;
    s.Hin = p.H;
    s.Win = p.W;
    s.cin = C;
    s.cout = C;
    ++p.i;
    std::vector<float> wd;
    if (p.at(AA_OP_DENSE)) {
        const aa_layer& d = p.layers[p.i];
        s.cout = d.filters;
        const float* k = p.get(d.off[0], (int64_t)C * d.filters);
        if (!k || d.filters <= 0) return p.fail(AA_ERR_INVALID, "dense kernel outside the blob");
        wd.assign(k, k + (size_t)C * d.filters);
        s.h_b.assign(d.filters, 0.f);
        if (d.off[1] >= 0) {
            const float* bb = p.get(d.off[1], d.filters);
            if (!bb) return p.fail(AA_ERR_INVALID, "dense bias outside the blob");
            s.h_b.assign(bb, bb + d.filters);
        }
        ++p.i;
    }
    if (p.at(AA_OP_SIGMOID)) {
        s.sigmoid = 1;
        ++p.i;
    }
    if (p.i != p.n_layers) return p.fail(AA_ERR_UNSUPPORTED, "layers after the global pooling / dense");
    s.cout_pad = s.cout;
    s.h_w = pack_rowmajor_f32(wd);
    s.flops = 2.0 * C * (wd.empty() ? 0 : s.cout);
    s.bytes = (double)prec_bytes(p.prec) * p.H * p.W * C + 4.0 * s.cout;
    char nm[96];
    snprintf(nm, sizeof nm, "globalmax%s_%d_%d", wd.empty() ? "" : "_dense", C, s.cout);
    s.name = nm;
    return AA_OK;
}

// Conv2D [+ BatchNormalization] [+ LeakyReLU / ReLU] [+ MaxPool2D]
static int parse_conv(LayerCursor& p, bool first, Stage& s, Fold& f) {
    const aa_layer& ly = p.layers[p.i];
    s.kh = ly.kh;
    s.kw = ly.kw;
    s.cin = p.C;
    s.cout = ly.filters;
    s.Hin = p.H;
    s.Win = p.W;
    s.Hc = p.H - ly.kh + 1;
    s.Wc = p.W - ly.kw + 1;
    s.is_first = first;
    if (s.Hc <= 0 || s.Wc <= 0) return p.fail(AA_ERR_INVALID, "input smaller than the kernel");
    const int K = s.kh * s.kw * s.cin;
    f.kern = p.get(ly.off[0], (int64_t)K * s.cout);
    if (!f.kern) return p.fail(AA_ERR_INVALID, "conv kernel outside the blob");
    f.scale.assign(s.cout, 1.0);
    f.shift.assign(s.cout, 0.0);
    if (ly.off[1] >= 0) {
        const float* b = p.get(ly.off[1], s.cout);
        if (!b) return p.fail(AA_ERR_INVALID, "bias outside the blob");
        for (int c = 0; c < s.cout; ++c) f.shift[c] = b[c];
    }
    ++p.i;
    if (p.at(AA_OP_BATCHNORM)) {
        const aa_layer& bn = p.layers[p.i];
        const float *g = p.get(bn.off[0], s.cout), *be = p.get(bn.off[1], s.cout), *mu = p.get(bn.off[2], s.cout),
                    *var = p.get(bn.off[3], s.cout);
        if (!g || !be || !mu || !var) return p.fail(AA_ERR_INVALID, "batchnorm params outside the blob");
        for (int c = 0; c < s.cout; ++c) {
            const double sc = (double)g[c] / std::sqrt((double)var[c] + (double)bn.eps);
            f.shift[c] = (f.shift[c] - mu[c]) * sc + be[c];
            f.scale[c] = sc;
        }
        ++p.i;
    }
    if (p.at(AA_OP_LEAKYRELU) || p.at(AA_OP_RELU)) {
        s.act = p.layers[p.i].op == AA_OP_LEAKYRELU ? ACT_LEAKY : ACT_RELU;
        s.alpha = p.layers[p.i].alpha;
        if (s.act == ACT_LEAKY && s.alpha < 0.f) return p.fail(AA_ERR_UNSUPPORTED, "LeakyReLU with a negative slope");
        ++p.i;
    }
    if (p.at(AA_OP_MAXPOOL2D)) {
        if (p.layers[p.i].kh <= 0 || p.layers[p.i].kw <= 0) return p.fail(AA_ERR_INVALID, "max-pool window");
        s.ph = p.layers[p.i].kh;
        s.pw = p.layers[p.i].kw;
        ++p.i;
    }
    s.pool = (s.ph == s.pw && (s.ph == 1 || s.ph == 3)) ? s.ph : 0;
    s.Hout = s.Hc / s.ph;
    s.Wout = s.Wc / s.pw;
    if (s.Hout <= 0 || s.Wout <= 0) return p.fail(AA_ERR_INVALID, "pool window larger than the conv output");
    return AA_OK;
}

// The kernel family of a parsed conv stage (a head consumes its
// GlobalMaxPool2D [+ sigmoid]), its cout_pad and Winograd form.
static int classify_conv(LayerCursor& p, Stage& s) {
    const bool gpool = p.at(AA_OP_GLOBALMAXPOOL2D);
    const bool dense_next = gpool && p.i + 1 < p.n_layers && p.layers[p.i + 1].op == AA_OP_DENSE;
    // (the first stage reads the f32 model input: only ST_SMALL / ST_GENERIC do)
    if (!s.is_first && gpool && !dense_next && s.kh == 1 && s.kw == 1 && s.ph == 1 && s.pw == 1 &&
        s.cin % 32 == 0 && s.cout <= 1024) {
        // the reference family's head: 1x1 conv, global max, sigmoid
        s.kind = ST_HEAD;
        ++p.i;
        if (p.at(AA_OP_SIGMOID)) {
            s.sigmoid = 1;
            ++p.i;
        }
        if (p.i != p.n_layers) return p.fail(AA_ERR_UNSUPPORTED, "layers after the 1x1 head");
    } else if (s.cin == 1 && s.kh == 3 && s.kw == 3 && s.cout == 32 && s.pool == 1) {
        s.kind = ST_SMALL;
    } else if (!s.is_first && s.pool && mfma_bn(p.prec, s.kh, s.kw, s.cin, s.pool)) {
        s.kind = ST_MFMA;
    } else if (p.prec == AA_PREC_BF16X3 && !s.is_first && s.cin >= 16) {
        s.kind = ST_GCONV;  // any other shape with a real contraction: the runtime-shaped MFMA kernel
    } else {
        s.kind = ST_GENERIC;
        if (p.prec == AA_PREC_FP8)
            return p.fail(AA_ERR_UNSUPPORTED, "no fp8 kernel for this conv shape (the f32 / bf16x3 / bf16 modes have one)");
    }
    if (s.is_first) {
        s.has_mag = p.has_mag;
        s.mag_exp = p.mag_exp;
        if (p.has_mag && s.kind != ST_SMALL && s.kind != ST_GENERIC)
            return p.fail(AA_ERR_UNSUPPORTED, "MagTransform needs a C_in=1 first conv");
    }
    if (s.kind == ST_GCONV) {
        s.cout_pad = (s.cout + 63) / 64 * 64;
        s.cin_pad = (s.cin + 31) / 32 * 32;
    } else if (s.kind == ST_SMALL || s.kind == ST_GENERIC) {
        s.cout_pad = s.cout;
    } else {
        const int bn_tile = s.kind == ST_MFMA ? mfma_bn(p.prec, s.kh, s.kw, s.cin, s.pool) : 32;
        s.cout_pad = (s.cout + bn_tile - 1) / bn_tile * bn_tile;
    }
    if (p.prec == AA_PREC_BF16X3 && s.kind == ST_MFMA && wg_bn(s.kh, s.kw, s.cin, s.pool) > 0)
        wg_form(s.kh, s.cin, s.pool, &s.wg, &s.wg_npass);
    return AA_OK;
}

// Weights with the BN scale folded in, in the layout of the stage's kernel
// (aa_cnn_pack.h), and the bias (fp8: [bias | dequantisation scale], both
// cout_pad long); flops, bytes and name.
static void pack_conv(Stage& s, const Fold& f, int prec) {
    const int ntap = s.kh * s.kw, K = ntap * s.cin;
    const bool mfma = s.kind == ST_MFMA;
    const bool tapmajor = mfma || s.kind == ST_HEAD;
    s.h_b.assign(prec == AA_PREC_FP8 && tapmajor ? 2 * s.cout_pad : s.cout_pad, 0.f);
    for (int o = 0; o < s.cout; ++o) s.h_b[o] = (float)f.shift[o];
    if (s.kind == ST_GCONV) {
        std::vector<float> w_tco((size_t)ntap * s.cout * s.cin);
        for (int t = 0; t < ntap; ++t)
            for (int o = 0; o < s.cout; ++o)
                for (int c = 0; c < s.cin; ++c)
                    w_tco[((size_t)t * s.cout + o) * s.cin + c] =
                        (float)(f.kern[((size_t)t * s.cin + c) * s.cout + o] * f.scale[o]);
        s.h_w = as_bytes(gconv_pack_x3(w_tco, ntap, s.cout, s.cin, s.cout_pad, s.cin_pad));
    } else if (!tapmajor) {  // conv_small / conv_generic: [cout][K]
        std::vector<float> w((size_t)s.cout * K);
        for (int o = 0; o < s.cout; ++o)
            for (int k = 0; k < K; ++k) w[(size_t)o * K + k] = (float)(f.kern[(size_t)k * s.cout + o] * f.scale[o]);
        s.h_w = pack_rowmajor_f32(w);
    } else if (s.wg) {
        std::vector<double> G((size_t)(s.wg + 2) * 3);
        for (size_t e = 0; e < G.size(); ++e) G[e] = wg_g(s.wg, (int)e / 3, (int)e % 3);
        s.h_w = pack_wg(f.kern, f.scale, s.kh, s.cin, s.cout, s.cout_pad, s.wg, s.wg_npass, G);
    } else {
        std::vector<float> w((size_t)ntap * s.cout_pad * s.cin, 0.f);  // [tap][cout_pad][cin]
        for (int o = 0; o < s.cout; ++o)
            for (int k = 0; k < K; ++k)
                w[((size_t)(k / s.cin) * s.cout_pad + o) * s.cin + k % s.cin] =
                    (float)(f.kern[(size_t)k * s.cout + o] * f.scale[o]);
        // MFMA stages pad their rows and carry 1 KiB of slack; the head reads [cout_pad][cin]
        const size_t slack = mfma ? 1024 : 0;
        if (prec == AA_PREC_BF16) {
            s.h_w = pack_bf16(w, ntap, s.cout_pad, s.cin, mfma ? conv_cstr<bf16>(s.cin) : s.cin, slack / 2);
        } else if (prec == AA_PREC_FP8) {
            s.h_w = pack_fp8(w, ntap, s.cout_pad, s.cin, mfma ? conv_cstr<fp8>(s.cin) : s.cin, slack,
                             mfma && conv_k128<fp8>(s.cin) ? F8_BSTR : 0, &s.h_b[s.cout_pad]);
        } else if (prec == AA_PREC_BF16X3 && mfma) {
            s.h_w = pack_x3(w, ntap, s.cout_pad, s.cin);
        } else {  // f32, and the split-bf16 head (f32 MFMA)
            s.h_w = pack_tap_f32(w, ntap, s.cout_pad, s.cin, mfma ? conv_cstr<float>(s.cin) : s.cin, slack / 4);
        }
    }
    s.flops = 2.0 * s.Hc * s.Wc * K * s.cout;
    const double es = (double)prec_bytes(prec);
    s.bytes = (s.is_first ? 4.0 : es) * s.Hin * s.Win * s.cin +
              (s.kind == ST_HEAD ? 4.0 * s.cout : es * s.Hout * s.Wout * s.cout);
    char nm[96];
    snprintf(nm, sizeof nm, "%s%dx%d_%d_%d%s",
             s.kind == ST_SMALL ? "conv_small_" : s.kind == ST_HEAD ? "head_" : s.kind == ST_GENERIC ? "conv_generic_"
             : s.kind == ST_GCONV ? "conv_gx3_" : "conv_",
             s.kh, s.kw, s.cin, s.cout, pool_suffix(s).c_str());
    s.name = nm;
}

// a C_in = 1 first conv (3x3 -> 32) the next 3x3/32 pooled MFMA stage computes itself
static bool fusable_first(const Stage& a, const Stage& b) {
    return a.kind == ST_SMALL && a.kh == 3 && a.kw == 3 && a.cin == 1 && a.cout == 32 && b.kind == ST_MFMA &&
           b.cin == 32 && b.kh == 3 && b.kw == 3 && b.pool == 3 &&
           (a.act != ACT_LEAKY || (a.alpha >= 0.f && a.alpha <= 1.f));
}

// fuse a C_in = 1 first conv (3x3 -> 32) into the following 3x3/32 pooled conv
static void fuse_first_conv(std::vector<Stage>& st, int prec) {
    if (st.size() < 2 || !fusable_first(st[0], st[1])) return;
    st[0].skipped = 1;
    st[1].fused_first = 1;
    st[1].flops += st[0].flops;
    // the fused pair reads the first conv's f32 input and writes the
    // second's output; the first conv's activations never reach HBM
    const double es1 = (double)prec_bytes(prec);
    st[1].bytes = 4.0 * st[0].Hin * st[0].Win * st[0].cin + (st[1].bytes - es1 * st[1].Hin * st[1].Win * st[1].cin);
    st[1].name = st[0].name + "+" + st[1].name;
    // (the skipped first conv keeps its f32 images: [32][9] weights, 32 biases)
    if (prec == AA_PREC_BF16X3) {
        std::vector<float> w1(32 * 9);
        memcpy(w1.data(), st[0].h_w.data(), w1.size() * sizeof(float));
        st[1].h_f1 = pack_first_lanes(w1.data(), st[0].h_b.data());
    }
}

// split-bf16: a conv_x3 stage whose consumer is another conv_x3 stage
// writes the grouped-split layout, and that consumer stages it by
// global_load_lds alone (aa_conv_x3.h); heads / generic stages keep f32
static void split_handoff(std::vector<Stage>& st) {
    for (size_t k = 0; k + 1 < st.size(); ++k) {
        Stage& a = st[k];
        Stage& b = st[k + 1];
        if (a.skipped || a.kind != ST_MFMA || b.kind != ST_MFMA || b.fused_first) continue;
        if (a.cout % 32 != 0 || b.cin != a.cout) continue;
        // a Winograd consumer transforms f32 values before it splits them: it
        // reads plain f32 (one 16-B load per 4 channels, not two 8-B loads and
        // a hi + lo sum); the split layout only pays for global_load_lds staging
        if (b.wg) continue;
        a.out_split = 1;
        b.in_split = 1;
    }
}

// split-bf16: the 1x3/128 -> 256 conv before a 1x1 head (<= 32 labels) and
// the head in one kernel (aa_conv_tail.h); the conv's 13 x 20 x 256
// activations never reach HBM.
static void fuse_tail(std::vector<Stage>& st) {
    if (st.size() < 2) return;
    Stage& h = st.back();
    Stage& c = st[st.size() - 2];
    if (!(h.kind == ST_HEAD && h.cout <= 32 && h.cout_pad == 32 && h.cin == 256 && c.kind == ST_MFMA && !c.skipped &&
          !c.fused_first && !c.wg && c.in_split && !c.out_split && c.kh == 1 && c.kw == 3 && c.cin == 128 &&
          c.cout == 256 && c.cout_pad == 256 && c.pool == 1 && c.ph == 1 && c.pw == 1))
        return;
    std::vector<float> hwf((size_t)h.cout_pad * h.cin);  // the head's f32 image [cout_pad][256]
    memcpy(hwf.data(), h.h_w.data(), hwf.size() * 4);
    h.h_tw = pack_tail_head(hwf, h.cout, h.cin, TAIL_NW);
    c.skipped = 1;
    h.tail = 1;
    h.flops += c.flops;
    h.bytes = 4.0 * c.Hin * c.Win * c.cin + 4.0 * h.cout;
    h.name = c.name + "+" + h.name;
}

// ping-pong activation buffers (stage s writes buffer s % 2), the head's
// partial maxima, and an ST_GCONV stage's unpooled f32 output
static void size_workspace(Model& m) {
    const size_t es = prec_bytes(m.prec);
    for (size_t k = 0; k < m.st.size(); ++k) {
        const Stage& s = m.st[k];
        if (s.kind == ST_GCONV && (s.ph > 1 || s.pw > 1)) m.tmp_elems = std::max(m.tmp_elems, (size_t)s.Hc * s.Wc * s.cout);
        if (k + 1 == m.st.size() || s.skipped || s.kind == ST_POOLDENSE) continue;
        m.act_elems[k % 2] = std::max(m.act_elems[k % 2], (size_t)s.Hout * s.Wout * s.cout);
    }
    if (m.st.back().kind != ST_HEAD) return;
    const Stage& h = m.st.back();  // the head's partial maxima use its free buffer
    const size_t parts = ((size_t)h.Hin * h.Win + 63) / 64;
    const size_t k = m.st.size() - 1;
    m.act_elems[k % 2] = std::max(m.act_elems[k % 2], (parts * h.cout_pad * sizeof(float) + es - 1) / es);
    if (h.tail) {  // the fused tail's per-tile maxima go to the skipped conv stage's buffer
        const Stage& c = m.st[k - 1];
        const size_t tiles = (size_t)((c.Hc + TAIL_TH - 1) / TAIL_TH) * ((c.Wc + TAIL_TW - 1) / TAIL_TW);
        m.act_elems[(k - 1) % 2] = std::max(m.act_elems[(k - 1) % 2], (tiles * 32 * sizeof(float) + es - 1) / es);
    }
}

// per-window elements stage k writes into its activation buffer (what
// size_workspace reserved for it)
static size_t stage_out_elems(const Model& m, size_t k) {
    const size_t es = prec_bytes(m.prec);
    const Stage& s = m.st[k];
    if (k + 1 == m.st.size()) {
        if (s.kind != ST_HEAD) return 0;
        if (s.tail) {
            const Stage& c = m.st[k - 1];
            const size_t tiles = (size_t)((c.Hc + TAIL_TH - 1) / TAIL_TH) * ((c.Wc + TAIL_TW - 1) / TAIL_TW);
            return (tiles * 32 * sizeof(float) + es - 1) / es;
        }
        return ((((size_t)s.Hin * s.Win + 63) / 64) * s.cout_pad * sizeof(float) + es - 1) / es;
    }
    if (s.skipped || s.kind == ST_POOLDENSE) return 0;
    return (size_t)s.Hout * s.Wout * s.cout;
}

// split-bf16: a 3x3 32 -> 64 conv_x3 stage that hands its output to a 3x3
// 64 -> 64 conv_x3 stage in the split layout, neither pooled: a full forward
// runs both in one launch (conv_x3_pair) and stage k's activations never
// reach HBM.  Only the consumer is marked: the stage vector, names, flops,
// bytes, split flags and workspace stay as planned, and a prefix that ends at
// stage k still runs its own kernel.
//
// Buffers: stage k + 1's ping-pong buffer is the one stage k's input lives
// in, so the pair writes stage k's buffer instead (stage k + 1's output is
// the smaller), and every later stage then writes the buffer of the other
// parity.  The pair is marked only where each of those outputs fits the
// buffer it lands in.  AA_X3_PAIR=0 at create time keeps the two launches.
static void mark_pairs(Model& m) {
    const char* e = getenv("AA_X3_PAIR");
    if (e && e[0] == '0') return;
    int flip = 0;  // later stages write the other buffer
    for (size_t k = 0; k + 1 < m.st.size(); ++k) {
        const Stage& a = m.st[k];
        Stage& b = m.st[k + 1];
        if (a.skipped || a.fused_first || a.pair || a.kind != ST_MFMA || b.kind != ST_MFMA) continue;
        if (!(a.kh == 3 && a.kw == 3 && a.cin == 32 && a.cout == 64 && a.cout_pad == 64 && a.pool == 1 && !a.wg &&
              a.out_split && b.kh == 3 && b.kw == 3 && b.cin == 64 && b.cout_pad == 64 && b.pool == 1 && !b.wg &&
              b.in_split && !b.out_split))
            continue;
        bool fits = stage_out_elems(m, k + 1) <= m.act_elems[(k % 2) ^ flip];
        for (size_t j = k + 2; fits && j < m.st.size(); ++j) {
            const size_t dst = (m.st[j].tail ? j - 1 : j) % 2;
            fits = stage_out_elems(m, j) <= m.act_elems[dst ^ flip ^ 1];
        }
        if (!fits) continue;
        b.pair = 1;
        flip ^= 1;
    }
}

// The arguments of aa_model_create -> a Model whose stages hold their host
// images (no device memory).  On failure *out is untouched and the reason is
// in aa_last_error.
static int plan_model(const aa_layer* layers, int32_t n_layers, const float* blob, int64_t blob_len, int32_t in_h,
                      int32_t in_w, int32_t in_c, int32_t precision, Model** out) {
    AA_CHECK(layers && blob && out && n_layers > 0, AA_ERR_INVALID, "aa_model_create: null argument");
    AA_CHECK(precision == AA_PREC_F32 || precision == AA_PREC_BF16 || precision == AA_PREC_FP8 ||
                 precision == AA_PREC_BF16X3, AA_ERR_INVALID,
             "aa_model_create: precision %d", precision);
    std::vector<Stage> st;
    LayerCursor p{layers, n_layers, blob, blob_len, precision};
    p.H = in_h, p.W = in_w, p.C = in_c;
    while (p.i < n_layers) {
        const int op = layers[p.i].op;
        if (op == AA_OP_MAGTRANSFORM) {
            const float* a = p.get(layers[p.i].off[0], 1);
            if (!a || !st.empty()) return p.fail(AA_ERR_UNSUPPORTED, "MagTransform must precede the first conv");
            p.has_mag = 1;
            p.mag_exp = 1.f / (1.f + expf(-a[0]));  // sigmoid(a) in f32 like tf.math.sigmoid
            ++p.i;
            continue;
        }
        Stage s;
        if (op == AA_OP_GLOBALMAXPOOL2D) {
            if (st.empty()) return p.fail(AA_ERR_UNSUPPORTED, "GlobalMaxPool2D before any conv");
            const int rc = plan_pooldense(p, s);
            if (rc != AA_OK) return rc;
        } else if (op == AA_OP_CONV2D) {
            Fold f;
            int rc = parse_conv(p, st.empty(), s, f);
            if (rc == AA_OK) rc = classify_conv(p, s);
            if (rc != AA_OK) return rc;
            pack_conv(s, f, precision);
            p.H = s.Hout;
            p.W = s.Wout;
            p.C = s.cout;
        } else {
            return p.fail(AA_ERR_UNSUPPORTED, "expected Conv2D");
        }
        s.layer_end = p.i;
        st.push_back(std::move(s));
    }
    AA_CHECK(!st.empty() && (st.back().kind == ST_HEAD || st.back().kind == ST_POOLDENSE), AA_ERR_UNSUPPORTED,
             "aa_model_create: the model must end with GlobalMaxPool2D (after a 1x1 conv or before a Dense)");
    fuse_first_conv(st, precision);
    if (precision == AA_PREC_BF16X3) {
        split_handoff(st);
        fuse_tail(st);
    }
    Model* m = new Model();
    m->prec = precision;
    m->in_h = in_h;
    m->in_w = in_w;
    m->in_c = in_c;
    m->L = st.back().cout;
    m->st = std::move(st);
    size_workspace(*m);
    if (precision == AA_PREC_BF16X3) mark_pairs(*m);
    *out = m;
    return AA_OK;
}

}  // namespace aa
