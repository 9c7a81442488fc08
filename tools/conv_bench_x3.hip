// Diagnostic harness: time split-bf16 (bf16x3) conv_x3 tilings of model1's
// layers at T = 226 on random f32 activations, 64 windows per launch.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include
//   tools/conv_bench_x3.hip audio-analysis_amd/csrc/aa_api.cpp -o tools/conv_bench_x3 ; run on the GPU box.
#include "../audio-analysis_amd/csrc/aa_cnn.hip"
#include "conv_wgp.h"  // the rejected plane-split Winograd conv (profiles/r06/wgp_rejected.txt)

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace aa;

template <int KH, int KW, int CIN, int WM, int WN, int MF, int NF, int POOL, int TH, int TW, bool FUSED,
          int DIAG = 0, bool RING = true, bool AJIT = false, int OCC = 0, bool IS = false, bool OS = false>
static void time_one(const char* tag, int n, int Hin, int Win, int cout, const void* in, const void* w,
                     const float* b, void* out, FirstConv fc, int iters) {
    auto k = conv_x3<KH, KW, CIN, WM, WN, MF, NF, POOL, TH, TW, FUSED, DIAG, RING, AJIT, OCC, IS, OS>;
    constexpr int BN = WN * NF * 16;
    const size_t lds = x3_lds_bytes<KH, KW, CIN, BN, TH, TW, FUSED, RING>();
    if (lds > 160 * 1024) {
        printf("%-8s %dx%d cin %3d WM%d WN%d MF%2d NF%d %2dx%2d  LDS %zu: skip\n", tag, KH, KW, CIN, WM, WN, MF, NF,
               TH, TW, lds);
        return;
    }
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int Hc = Hin - KH + 1, Wc = Win - KW + 1;
    const int Hout = Hc / POOL, Wout = Wc / POOL;
    const int tiles_h = (Hout * POOL + TH - 1) / TH, tiles_w = (Wout * POOL + TW - 1) / TW;
    dim3 grid(tiles_h * tiles_w, cout / BN, n);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (int i = 0; i < 3; ++i)
        hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, 0, (const float*)in, Hin, Win, (const bf16*)w, b,
                           (float*)out, Hout, Wout, cout, tiles_w, 1, 0.3f, fc);
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, 0, (const float*)in, Hin, Win, (const bf16*)w, b,
                           (float*)out, Hout, Wout, cout, tiles_w, 1, 0.3f, fc);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const float us = 1e3f * ms / iters;
    double fl = 2.0 * n * Hc * Wc * KH * KW * CIN * cout;
    if (FUSED) fl += 2.0 * n * (Hin) * (Win) * 9 * 32;
    printf("%-8s%s%s%s%d %dx%d cin %3d WM%d WN%d MF%2d NF%d %2dx%2d  LDS %6zu  grid %6d  %7.1f us  %6.1f TF (%.3f of 833)\n",
           tag, IS ? "S" : "", RING ? "" : "G", AJIT ? "J" : "", OCC, KH, KW, CIN, WM, WN, MF, NF, TH, TW, lds, grid.x * grid.y * grid.z, us, fl / us * 1e-6,
           fl / us * 1e-6 / 833.3);
}

template <int KH, int CIN, int WM, int WN, int MF, int NF, int POOL, int TH, int TW, int OCC, bool IS, bool OS,
          int DIAG = 0, int WO = 2, int NPASS = 1>
static void time_wg(const char* tag, int n, int Hin, int Win, int cout, const void* in, const void* w, const float* b,
                    void* out, int iters) {
    auto k = conv_wg<KH, CIN, WM, WN, MF, NF, POOL, TH, TW, OCC, IS, OS, DIAG, WO, NPASS>;
    constexpr int BN = WN * NF * 16;
    const size_t lds = wg_lds_bytes<KH, BN, TH, TW, WO, NPASS, WN>();
    if (lds > 160 * 1024) { printf("%s LDS %zu: skip\n", tag, lds); return; }
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int Hc = Hin - KH + 1, Wc = Win - 3 + 1;
    const int Hout = Hc / POOL, Wout = Wc / POOL;
    const int tiles_h = (Hout * POOL + TH - 1) / TH, tiles_w = (Wout * POOL + TW - 1) / TW;
    dim3 grid(tiles_h * tiles_w, cout / BN, n);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (int i = 0; i < 3; ++i)
        hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, 0, (const float*)in, Hin, Win, (const bf16*)w, b,
                           (float*)out, Hout, Wout, cout, tiles_w, 1, 0.3f);
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, 0, (const float*)in, Hin, Win, (const bf16*)w, b,
                           (float*)out, Hout, Wout, cout, tiles_w, 1, 0.3f);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const float us = 1e3f * ms / iters;
    const double fl = 2.0 * n * Hc * Wc * KH * 3 * CIN * cout;
    printf("%-6s wg%d d%d %dx3 cin %3d WM%d WN%d MF%d NF%d %2dx%2d occ%d LDS %6zu grid %6d  %7.1f us  %6.1f TF (%.3f of 833)\n",
           tag, WO, DIAG, KH, CIN, WM, WN, MF, NF, TH, TW, OCC, lds, grid.x * grid.y * grid.z, us, fl / us * 1e-6,
           fl / us * 1e-6 / 833.3);
}

int main(int argc, char** argv) {
    const int n = 64, it = 20;
    std::vector<float> h(100u << 20);  // 400 MB of f32 activations: larger than every layer's input
    for (auto& x : h) x = 1.f + (rand() & 0xffff) / 65536.f;
    std::vector<uint16_t> hw(4u << 20);
    for (auto& x : hw) x = 0x3c00 + (rand() & 0x3ff);  // bf16 ~0.0078..0.0156
    void *in, *w, *out;
    float* b;
    (void)hipMalloc(&in, h.size() * 4);
    (void)hipMalloc(&w, hw.size() * 2);
    (void)hipMalloc(&out, 400u << 20);
    (void)hipMalloc(&b, 8192);
    (void)hipMemcpy(in, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemset(b, 0, 8192);
    FirstConv fc{};
    float *w1, *b1;
    (void)hipMalloc(&w1, 32 * 9 * 4);
    (void)hipMalloc(&b1, 32 * 4);
    std::vector<float> hw1(32 * 9, 0.05f), hb1(32, 0.01f);
    (void)hipMemcpy(w1, hw1.data(), hw1.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(b1, hb1.data(), hb1.size() * 4, hipMemcpyHostToDevice);
    FirstConv f1{w1, b1, 1, 0.3f, 0, 1.f, 160, 226};
    {  // conv_x3 reads the first layer's weights and bias as the per-lane image
        const std::vector<uint8_t> li = pack_first_lanes(hw1.data(), hb1.data());
        void* dli;
        (void)hipMalloc(&dli, li.size());
        (void)hipMemcpy(dli, li.data(), li.size(), hipMemcpyHostToDevice);
        f1.img = dli;
    }
    const int which = argc > 1 ? atoi(argv[1]) : 0;  // 0: all layers, 9: ablations
    if (which == 9) {
        // DIAG bits (aa_cnn.hip): 1 no staging, 4 no stores, 32 no weight stream,
        // 128 no fragment reads after the first, 2 no MFMA loop
#define ABL5(D) time_one<9, 3, 64, 4, 2, 4, 4, 3, 39, 6, false, D, false, true, 2>("c5 d" #D, n, 48, 70, 128, in, w, b, out, fc, it);
#define ABL2(D) time_one<3, 3, 32, 4, 1, 4, 2, 3, 12, 21, true, D, false, true, 0>("c2 d" #D, n, 158, 224, 32, in, w, b, out, f1, it);
#define ABL4(D) time_one<3, 3, 64, 4, 2, 3, 2, 1, 12, 14, false, D, true, true, 4>("c4 d" #D, n, 50, 72, 64, in, w, b, out, fc, it);
#define ABL3(D) time_one<3, 3, 32, 4, 2, 3, 2, 1, 10, 18, false, D, true, false, 0>("c3 d" #D, n, 52, 74, 64, in, w, b, out, fc, it);
        ABL5(0) ABL5(1) ABL5(2) ABL5(4) ABL5(5) ABL5(33) ABL5(161) ABL5(165) ABL5(37)
        ABL2(0) ABL2(2) ABL2(64) ABL2(512) ABL2(576) ABL2(4) ABL2(1) ABL2(5)
        ABL4(0) ABL4(1) ABL4(2) ABL4(4) ABL4(5) ABL4(33) ABL4(161) ABL4(165)
        ABL3(0) ABL3(1) ABL3(2) ABL3(5) ABL3(165)
        return 0;
    }
    // model1 at T = 226: (Hin, Win) of each conv's input
#define C2(WM, WN, MF, NF, TH, TW) time_one<3, 3, 32, WM, WN, MF, NF, 3, TH, TW, true>("c1+c2", n, 158, 224, 32, in, w, b, out, f1, it);
#define C3(WM, WN, MF, NF, TH, TW) time_one<3, 3, 32, WM, WN, MF, NF, 1, TH, TW, false>("c3", n, 52, 74, 64, in, w, b, out, fc, it);
#define C4(WM, WN, MF, NF, TH, TW) time_one<3, 3, 64, WM, WN, MF, NF, 1, TH, TW, false>("c4", n, 50, 72, 64, in, w, b, out, fc, it);
#define C5(WM, WN, MF, NF, TH, TW) time_one<9, 3, 64, WM, WN, MF, NF, 3, TH, TW, false>("c5", n, 48, 70, 128, in, w, b, out, fc, it);
#define G2(WM, WN, MF, NF, TH, TW) time_one<3, 3, 32, WM, WN, MF, NF, 3, TH, TW, true, 0, false>("c1+c2", n, 158, 224, 32, in, w, b, out, f1, it);
#define G3(WM, WN, MF, NF, TH, TW) time_one<3, 3, 32, WM, WN, MF, NF, 1, TH, TW, false, 0, false>("c3", n, 52, 74, 64, in, w, b, out, fc, it);
#define G4(WM, WN, MF, NF, TH, TW) time_one<3, 3, 64, WM, WN, MF, NF, 1, TH, TW, false, 0, false>("c4", n, 50, 72, 64, in, w, b, out, fc, it);
#define G5(WM, WN, MF, NF, TH, TW) time_one<9, 3, 64, WM, WN, MF, NF, 3, TH, TW, false, 0, false>("c5", n, 48, 70, 128, in, w, b, out, fc, it);
#define G6(WM, WN, MF, NF, TH, TW) time_one<1, 3, 128, WM, WN, MF, NF, 1, TH, TW, false, 0, false>("c6", n, 13, 22, 256, in, w, b, out, fc, it);
#define J2(WM, WN, MF, NF, TH, TW, R, O) time_one<3, 3, 32, WM, WN, MF, NF, 3, TH, TW, true, 0, R, true, O>("c1+c2", n, 158, 224, 32, in, w, b, out, f1, it);
#define J3(WM, WN, MF, NF, TH, TW, R, O) time_one<3, 3, 32, WM, WN, MF, NF, 1, TH, TW, false, 0, R, true, O>("c3", n, 52, 74, 64, in, w, b, out, fc, it);
#define J4(WM, WN, MF, NF, TH, TW, R, O) time_one<3, 3, 64, WM, WN, MF, NF, 1, TH, TW, false, 0, R, true, O>("c4", n, 50, 72, 64, in, w, b, out, fc, it);
#define J5(WM, WN, MF, NF, TH, TW, R, O) time_one<9, 3, 64, WM, WN, MF, NF, 3, TH, TW, false, 0, R, true, O>("c5", n, 48, 70, 128, in, w, b, out, fc, it);
#define J6(WM, WN, MF, NF, TH, TW, R, O) time_one<1, 3, 128, WM, WN, MF, NF, 1, TH, TW, false, 0, R, true, O>("c6", n, 13, 22, 256, in, w, b, out, fc, it);
#define C6(WM, WN, MF, NF, TH, TW) time_one<1, 3, 128, WM, WN, MF, NF, 1, TH, TW, false>("c6", n, 13, 22, 256, in, w, b, out, fc, it);
    // pre-split input / output (IN_SPLIT, OUT_SPLIT): the shipped pipeline's c3..c6
#define S3(WM, WN, MF, NF, TH, TW, R, J, O) time_one<3, 3, 32, WM, WN, MF, NF, 1, TH, TW, false, 0, R, J, O, true, true>("c3", n, 52, 74, 64, in, w, b, out, fc, it);
#define S4(WM, WN, MF, NF, TH, TW, R, J, O) time_one<3, 3, 64, WM, WN, MF, NF, 1, TH, TW, false, 0, R, J, O, true, true>("c4", n, 50, 72, 64, in, w, b, out, fc, it);
#define S5(WM, WN, MF, NF, TH, TW, R, J, O) time_one<9, 3, 64, WM, WN, MF, NF, 3, TH, TW, false, 0, R, J, O, true, true>("c5", n, 48, 70, 128, in, w, b, out, fc, it);
#define S6(WM, WN, MF, NF, TH, TW, R, J, O) time_one<1, 3, 128, WM, WN, MF, NF, 1, TH, TW, false, 0, R, J, O, true, false>("c6", n, 13, 22, 256, in, w, b, out, fc, it);
    if (which == 11) {
        S5(4, 2, 4, 4, 39, 6, false, true, 2) S5(4, 1, 4, 4, 39, 6, false, true, 2) S5(4, 1, 4, 4, 39, 6, false, true, 0)
        S5(4, 1, 4, 4, 39, 6, true, true, 2) S5(4, 2, 4, 4, 39, 6, true, true, 2) S5(4, 2, 4, 2, 39, 6, false, true, 4)
        S5(4, 2, 4, 2, 39, 6, true, true, 4) S5(4, 1, 4, 2, 39, 6, false, true, 4) S5(2, 2, 4, 4, 21, 6, false, true, 2)
        S5(8, 2, 2, 4, 39, 6, false, true, 2) S5(4, 2, 4, 4, 42, 6, false, true, 2) S5(4, 2, 6, 4, 39, 9, false, true, 2)
        S4(4, 2, 3, 2, 12, 14, true, true, 4) S4(4, 2, 3, 2, 12, 14, false, true, 4) S4(4, 2, 4, 2, 16, 14, true, true, 4)
        S4(4, 2, 4, 2, 16, 14, true, true, 0) S4(4, 1, 3, 4, 12, 14, true, true, 4) S4(4, 2, 6, 2, 24, 14, true, true, 0)
        S4(4, 2, 3, 2, 8, 24, true, true, 4) S4(2, 2, 3, 2, 8, 12, true, true, 4)
        S3(4, 2, 3, 2, 10, 18, true, false, 0) S3(4, 2, 3, 2, 10, 18, true, true, 4) S3(4, 2, 4, 2, 10, 24, true, true, 4)
        S3(4, 2, 3, 2, 12, 16, true, true, 4) S3(4, 1, 3, 4, 12, 16, true, true, 4) S3(2, 2, 3, 2, 8, 12, true, true, 4)
        S6(4, 2, 3, 2, 7, 20, true, false, 0) S6(4, 2, 3, 2, 7, 20, true, true, 4) S6(4, 2, 5, 2, 13, 20, true, true, 0)
        S6(4, 1, 3, 4, 7, 20, true, false, 0) S6(2, 2, 3, 2, 7, 12, true, true, 4) S6(4, 2, 3, 2, 7, 20, false, true, 4)
        return 0;
    }
#define F2(WM, WN, MF, NF, TH, TW, R, O) time_one<3, 3, 32, WM, WN, MF, NF, 3, TH, TW, true, 0, R, true, O, false, true>("c1+c2", n, 158, 224, 32, in, w, b, out, f1, it);
#define W5(WM, WN, MF, NF, TH, TW, O, D) time_wg<9, 64, WM, WN, MF, NF, 3, TH, TW, O, true, true, D>("c5", n, 48, 70, 128, in, w, b, out, it);
#define W4(WM, WN, MF, NF, TH, TW, O, D) time_wg<3, 64, WM, WN, MF, NF, 1, TH, TW, O, true, true, D>("c4", n, 50, 72, 64, in, w, b, out, it);
#define W3(WM, WN, MF, NF, TH, TW, O, D) time_wg<3, 32, WM, WN, MF, NF, 1, TH, TW, O, true, true, D>("c3", n, 52, 74, 64, in, w, b, out, it);
#define W6(WM, WN, MF, NF, TH, TW, O, D) time_wg<1, 128, WM, WN, MF, NF, 1, TH, TW, O, true, false, D>("c6", n, 13, 22, 256, in, w, b, out, it);
    if (which == 19) {  // the shipped split-bf16 tiles (aa_cnn_tiles.h AA_X3_CFGS / AA_WG_CFGS), then fused-kernel ablations
#define FS(D) time_one<3, 3, 32, 4, 1, 4, 2, 3, 12, 21, true, D, false, true, 0, false, true>("c1+c2 d" #D, n, 158, 224, 32, in, w, b, out, f1, it);
        FS(0) S3(4, 2, 3, 2, 10, 18, true, false, 4) S4(2, 2, 3, 2, 12, 8, true, true, 0)
        W5(2, 2, 4, 2, 39, 6, 2, 0) S6(2, 2, 3, 2, 7, 12, true, true, 0)
        FS(2) FS(64) FS(4) FS(128) FS(16) FS(512) FS(576) FS(0)
        return 0;
    }
    if (which == 30) {  // Winograd 9x3: F(2,3) (round 4) vs F(6,3) (round 5), ablations (1 no staging, 2 no MFMA)
#define W5O(WM, WN, MF, NF, TH, TW, O, D, WO) time_wg<9, 64, WM, WN, MF, NF, 3, TH, TW, O, true, true, D, WO>("c5", n, 48, 70, 128, in, w, b, out, it);
        W5O(2, 2, 4, 2, 39, 6, 2, 0, 2) W5O(1, 4, 3, 1, 39, 6, 2, 0, 6)
        W5O(2, 2, 4, 2, 39, 6, 2, 1, 2) W5O(1, 4, 3, 1, 39, 6, 2, 1, 6)
        W5O(2, 2, 4, 2, 39, 6, 2, 2, 2) W5O(1, 4, 3, 1, 39, 6, 2, 2, 6)
        W5O(2, 2, 4, 2, 39, 6, 2, 3, 2) W5O(1, 4, 3, 1, 39, 6, 2, 3, 6)
        W5O(1, 4, 3, 1, 39, 6, 0, 0, 6) W5O(1, 4, 3, 1, 39, 6, 3, 0, 6)
        return 0;
    }
    if (which == 31) {  // the shipped F(6,3) 9x3 tile (f32 in, split out): full, no staging, no MFMA steps (PMC)
#define W5S(D) time_wg<9, 64, 1, 4, 3, 1, 3, 39, 6, 0, false, true, D, 6>("c5", n, 48, 70, 128, in, w, b, out, 2);
        W5S(0) W5S(1) W5S(2) W5S(3)
        return 0;
    }
    if (which == 34) {  // conv_wg vs conv_wgp ablations: 1 no staging, 2 no MFMA steps
#define WGA(D) time_wg<9, 64, 1, 4, 3, 1, 3, 39, 6, 0, false, true, D, 6>("c5", n, 48, 70, 128, in, w, b, out, it);
#define WGPA(D) WGPX(4, 0, D)
#define WGPX(NWV, OCCV, D)                                                                                        \
        {                                                                                                         \
            auto k1 = conv_wgp<9, 64, NWV, 3, 4, 3, 39, 6, OCCV, false, true, D, 6, 2>;                          \
            const size_t l1 = wgp_lds_bytes<9, 39, 6, 6, 3>();                                                   \
            (void)hipFuncSetAttribute((const void*)k1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l1);     \
            dim3 grid(11, 2, n);                                                                              \
            for (int i = 0; i < 3; ++i)                                                                           \
                hipLaunchKernelGGL(k1, grid, dim3(64 * NWV), l1, 0, (const float*)in, 48, 70, (const bf16*)w, b, (float*)out, 13, 22, 128, 11, 1, 0.3f); \
            hipEvent_t e0, e1;                                                                                    \
            (void)hipEventCreate(&e0);                                                                            \
            (void)hipEventCreate(&e1);                                                                            \
            (void)hipEventRecord(e0, 0);                                                                          \
            for (int i = 0; i < it; ++i)                                                                          \
                hipLaunchKernelGGL(k1, grid, dim3(64 * NWV), l1, 0, (const float*)in, 48, 70, (const bf16*)w, b, (float*)out, 13, 22, 128, 11, 1, 0.3f); \
            (void)hipEventRecord(e1, 0);                                                                          \
            (void)hipEventSynchronize(e1);                                                                        \
            float ms = 0;                                                                                         \
            (void)hipEventElapsedTime(&ms, e0, e1);                                                               \
            printf("wgp nw%d occ%d d%d %7.1f us\n", NWV, OCCV, D, 1e3f * ms / it);                                                      \
        }
        for (int r = 0; r < 2; ++r) {
            WGA(0) WGPA(0) WGPX(8, 0, 0) WGPX(8, 4, 0) WGA(1) WGPA(1) WGPX(8, 0, 1) WGA(2) WGPA(2) WGPX(8, 0, 2) WGA(3) WGPA(3)
        }
        return 0;
    }
    if (which == 35 || which == 36) {
        // the shipped 9x3 tile with A read from LDS at every kernel row (SLIDE 0) or sliding in
        // registers (reload every 3 rows / once per plane), on f32 N(0,1) activations and split
        // N(0,0.05) weights.  35: outputs compared word for word, then timed in alternating
        // rounds.  36 V: variant V (0 | 3 | 9) alone, 2 launches (PMC passes).
        const int Hin = 48, Win = 70, cout = 128, Hc = Hin - 8, Wc = Win - 2, Hout = Hc / 3, Wout = Wc / 3;
        const int tiles_h = (Hout * 3 + 38) / 39, tiles_w = (Wout * 3 + 5) / 6;
        const size_t on = (size_t)n * Hout * Wout * cout, in_el = (size_t)n * Hin * Win * 64;
        {
            std::vector<float> hs(in_el);
            std::vector<uint16_t> ws(hw.size());
            unsigned st = 1;
            auto gauss = [&]() {
                float a = 0;
                for (int k = 0; k < 4; ++k) { st = st * 1664525u + 1013904223u; a += (st >> 8) * (1.f / 16777216.f) - 0.5f; }
                return a * 1.7f;
            };
            auto split = [](float x, uint16_t& hi, uint16_t& lo) {
                uint32_t u; memcpy(&u, &x, 4);
                uint32_t r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000u;
                float hf; memcpy(&hf, &r, 4);
                float l = x - hf; uint32_t v; memcpy(&v, &l, 4);
                v = (v + 0x7fff + ((v >> 16) & 1)) >> 16;
                hi = (uint16_t)(r >> 16); lo = (uint16_t)v;
            };
            for (auto& x : hs) x = gauss();
            for (size_t r = 0; r < ws.size() / 64; ++r)
                for (int c = 0; c < 32; ++c) split(0.05f * gauss(), ws[r * 64 + c], ws[r * 64 + 32 + c]);
            (void)hipMemcpy(in, hs.data(), hs.size() * 4, hipMemcpyHostToDevice);
            (void)hipMemcpy(w, ws.data(), ws.size() * 2, hipMemcpyHostToDevice);
        }
        const size_t l0 = wg_lds_bytes<9, 64, 39, 6, 6, 1, 4>();
#define WGS(OCCV, BDV, SL) (const void*)conv_wg<9, 64, 1, 4, 3, 1, 3, 39, 6, OCCV, false, true, 0, 6, 1, BDV, SL>
        constexpr int NV = 7;  // (SLIDE, pinned waves per SIMD, B sets in flight)
        const void* ks[NV] = {WGS(0, 2, 0), WGS(0, 2, 3), WGS(0, 2, 9), WGS(3, 2, 9), WGS(0, 4, 9), WGS(0, 6, 9), WGS(0, 8, 9)};
        const int slide[NV] = {0, 3, 9, 9, 9, 9, 9}, occ[NV] = {0, 0, 0, 3, 0, 0, 0}, bd[NV] = {2, 2, 2, 2, 4, 6, 8};
        for (auto k : ks) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l0);
        dim3 grid(tiles_h * tiles_w, cout / 64, n);
        const float* fin = (const float*)in;
        const bf16* fw = (const bf16*)w;
        int hin = Hin, win = Win, hout = Hout, wout = Wout, co = cout, tws = tiles_w, act = 1;
        float alpha = 0.3f;
        auto run = [&](int v, void* o) {
            float* fo = (float*)o;
            void* args[] = {&fin, &hin, &win, &fw, &b, &fo, &hout, &wout, &co, &tws, &act, &alpha};
            (void)hipLaunchKernel(ks[v], grid, dim3(256), args, l0, 0);
        };
        if (which == 36) {
            const int want = argc > 2 ? atoi(argv[2]) : 0;
            for (int v = 0; v < 3; ++v)  // (the three with free occupancy and 2 B sets)
                if (slide[v] == want) { run(v, out); run(v, out); }
            const hipError_t e = hipDeviceSynchronize();
            printf("slide %d: %s\n", want, hipGetErrorString(e));
            return e != hipSuccess;
        }
        std::vector<uint32_t> ref(on), c(on);
        size_t bad = 0;
        for (int v = 0; v < NV; ++v) {
            (void)hipMemset(out, 0xff, on * 4);
            run(v, out);
            if (hipDeviceSynchronize() != hipSuccess) { printf("kernel error (variant %d)\n", v); return 2; }
            (void)hipMemcpy(v ? c.data() : ref.data(), out, on * 4, hipMemcpyDeviceToHost);
            size_t nd = 0;
            for (size_t i = 0; v && i < on; ++i) nd += ref[i] != c[i];
            if (v) printf("slide %d occ %d bd %d: %zu of %zu output words differ from slide 0\n", slide[v], occ[v], bd[v], nd, on);
            bad += nd;
        }
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        for (int round = 0; round < 5; ++round)
            for (int v = 0; v < NV; ++v) {
                for (int i = 0; i < 2; ++i) run(v, out);
                (void)hipEventRecord(e0, 0);
                for (int i = 0; i < it; ++i) run(v, out);
                (void)hipEventRecord(e1, 0);
                (void)hipEventSynchronize(e1);
                float ms = 0;
                (void)hipEventElapsedTime(&ms, e0, e1);
                printf("round %d slide %d occ %d bd %d %7.1f us\n", round, slide[v], occ[v], bd[v], 1e3f * ms / it);
            }
        return bad ? 1 : 0;
    }
    if (which == 40 || which == 41) {
        // The 3x3 32->64 (split out) and 64->64 (split in, f32 out) convs at model1's shape: the two
        // shipped conv_x3 launches back to back ("chain") against conv_x3_pair (aa_conv_pair.h), on
        // grouped-split N(0,1) activations, split N(0,0.05) weights packed with their swizzle and
        // N(0,0.1) biases.  40: every pair variant's output compared word for word with the chain's,
        // then 5 alternating rounds of 20 launches.  41 V: variant V alone (0: chain), 2 launches
        // (PMC passes).
        const int Hin = 52, Win = 74, Hm = 50, Wm = 72, Ho = 48, Wo = 70;
        const size_t in_el = (size_t)n * Hin * Win * 32, mid_el = (size_t)n * Hm * Wm * 64, on = (size_t)n * Ho * Wo * 64;
        float *bA, *bB;
        void *wA, *wB, *mid, *out2;
        (void)hipMalloc(&bA, 256);
        (void)hipMalloc(&bB, 256);
        (void)hipMalloc(&wA, 9 * 64 * 128);
        (void)hipMalloc(&wB, 18 * 64 * 128);
        (void)hipMalloc(&mid, mid_el * 4);
        (void)hipMalloc(&out2, on * 4);
        {
            unsigned st = 1;
            auto gauss = [&]() {
                float a = 0;
                for (int k = 0; k < 4; ++k) { st = st * 1664525u + 1013904223u; a += (st >> 8) * (1.f / 16777216.f) - 0.5f; }
                return a * 1.7f;
            };
            auto split = [](float x, uint16_t& hi, uint16_t& lo) {
                uint32_t u; memcpy(&u, &x, 4);
                uint32_t r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000u;
                float hf; memcpy(&hf, &r, 4);
                float l = x - hf; uint32_t v; memcpy(&v, &l, 4);
                v = (v + 0x7fff + ((v >> 16) & 1)) >> 16;
                hi = (uint16_t)(r >> 16); lo = (uint16_t)v;
            };
            std::vector<uint16_t> hs(in_el * 2);  // grouped split: per pixel 32 hi then 32 lo
            for (size_t px = 0; px < in_el / 32; ++px)
                for (int c = 0; c < 32; ++c) split(gauss(), hs[px * 64 + c], hs[px * 64 + 32 + c]);
            (void)hipMemcpy(in, hs.data(), hs.size() * 2, hipMemcpyHostToDevice);
            // packed weights: per step 64 rows of 8 units, unit u (hi 0-3, lo 4-7) of row o in slot (u + o) & 7
            auto pack = [&](int steps, void* dst) {
                std::vector<uint16_t> ws((size_t)steps * 64 * 64);
                for (int s = 0; s < steps; ++s)
                    for (int o = 0; o < 64; ++o)
                        for (int c = 0; c < 32; ++c) {
                            uint16_t hi, lo;
                            split(0.05f * gauss(), hi, lo);
                            const size_t row = ((size_t)s * 64 + o) * 64;
                            ws[row + (((c >> 3) + o) & 7) * 8 + (c & 7)] = hi;
                            ws[row + (((c >> 3) + 4 + o) & 7) * 8 + (c & 7)] = lo;
                        }
                (void)hipMemcpy(dst, ws.data(), ws.size() * 2, hipMemcpyHostToDevice);
            };
            pack(9, wA);
            pack(18, wB);
            std::vector<float> hb(64);
            for (auto& x : hb) x = 0.1f * gauss();
            (void)hipMemcpy(bA, hb.data(), 256, hipMemcpyHostToDevice);
            for (auto& x : hb) x = 0.1f * gauss();
            (void)hipMemcpy(bB, hb.data(), 256, hipMemcpyHostToDevice);
        }
        // the chain: the shipped tiles (aa_cnn_tiles.h AA_X3_CFGS)
        auto kA = conv_x3<3, 3, 32, 4, 2, 3, 2, 1, 10, 18, false, 0, true, false, 4, true, true>;
        auto kB = conv_x3<3, 3, 64, 2, 2, 3, 2, 1, 12, 8, false, 0, true, true, 0, true, false>;
        const size_t lA = x3_lds_bytes<3, 3, 32, 64, 10, 18, false, true>(), lB = x3_lds_bytes<3, 3, 64, 64, 12, 8, false, true>();
        (void)hipFuncSetAttribute((const void*)kA, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lA);
        (void)hipFuncSetAttribute((const void*)kB, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lB);
        const int twA = (Wm + 17) / 18, thA = (Hm + 9) / 10, twB = (Wo + 7) / 8, thB = (Ho + 11) / 12;
        auto chainA = [&]() {
            hipLaunchKernelGGL(kA, dim3(thA * twA, 1, n), dim3(512), lA, 0, (const float*)in, Hin, Win, (const bf16*)wA, bA,
                               (float*)mid, Hm, Wm, 64, twA, 1, 0.3f, fc);
        };
        auto chainB = [&](void* o) {
            hipLaunchKernelGGL(kB, dim3(thB * twB, 1, n), dim3(256), lB, 0, (const float*)mid, Hm, Wm, (const bf16*)wB, bB,
                               (float*)o, Ho, Wo, 64, twB, 1, 0.3f, fc);
        };
        // pair variants: (B sets in flight, A just in time, pinned schedule, pinned waves per SIMD)
#define PAIRK(BDV, JV, PV, OV, AL) (const void*)conv_x3_pair<12, 8, BDV, JV, PV, OV, AL>
        // (first sweep, group images beside the patch, 2 blocks per CU: bd2 jit pin 83.5, bd3 jit pin 82.8,
        // bd2 jit free 87.1, bd2 ahead free 84.9, bd4 jit pin 83.1 us against the chain's 84.1)
        constexpr int NV = 8;
        const void* ks[NV] = {PAIRK(2, true, true, 2, false), PAIRK(2, false, true, 0, false), PAIRK(3, false, true, 0, false),
                              PAIRK(2, true, true, 3, true),  PAIRK(2, true, true, 4, true),   PAIRK(3, true, true, 3, true),
                              PAIRK(2, true, false, 4, true), PAIRK(2, false, true, 3, true)};
        const char* kn[NV] = {"bd2 jit pin occ2", "bd2 ahead pin", "bd3 ahead pin", "alias bd2 jit pin occ3", "alias bd2 jit pin occ4",
                              "alias bd3 jit pin occ3", "alias bd2 jit free occ4", "alias bd2 ahead pin occ3"};
        const size_t lds_of[NV] = {pair_lds_bytes<12, 8, false>(), pair_lds_bytes<12, 8, false>(), pair_lds_bytes<12, 8, false>(),
                                   pair_lds_bytes<12, 8, true>(),  pair_lds_bytes<12, 8, true>(),  pair_lds_bytes<12, 8, true>(),
                                   pair_lds_bytes<12, 8, true>(),  pair_lds_bytes<12, 8, true>()};
        for (int v = 0; v < NV; ++v) (void)hipFuncSetAttribute(ks[v], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of[v]);
        auto pair = [&](int v, void* o) {
            const float* fin = (const float*)in;
            const bf16 *fa = (const bf16*)wA, *fb = (const bf16*)wB;
            float* fo = (float*)o;
            int hin = Hin, win = Win, ho = Ho, wo = Wo, co = 64, tws = twB, act = 1;
            float alpha = 0.3f;
            void* args[] = {&fin, &hin, &win, &fa, &bA, &act, &alpha, &fb, &bB, &fo, &ho, &wo, &co, &tws, &act, &alpha};
            (void)hipLaunchKernel(ks[v], dim3(thB * twB, 1, n), dim3(256), args, lds_of[v], 0);
        };
        if (which == 41) {
            const int v = argc > 2 ? atoi(argv[2]) : 0;
            for (int i = 0; i < 2; ++i) {
                if (v == 0) { chainA(); chainB(out); }
                else pair(v - 1, out2);
            }
            const hipError_t e = hipDeviceSynchronize();
            printf("variant %d (%s): %s\n", v, v ? kn[v - 1] : "chain", hipGetErrorString(e));
            return e != hipSuccess;
        }
        printf("LDS: chain A %zu, chain B %zu, pair %zu, pair alias %zu\n", lA, lB, lds_of[0], lds_of[3]);
        std::vector<uint32_t> ref(on), c(on);
        (void)hipMemset(out, 0xff, on * 4);
        chainA();
        chainB(out);
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel error (chain)\n"); return 2; }
        (void)hipMemcpy(ref.data(), out, on * 4, hipMemcpyDeviceToHost);
        size_t bad = 0;
        for (int v = 0; v < NV; ++v) {
            (void)hipMemset(out2, 0xee, on * 4);
            pair(v, out2);
            if (hipDeviceSynchronize() != hipSuccess) { printf("kernel error (pair %s)\n", kn[v]); return 2; }
            (void)hipMemcpy(c.data(), out2, on * 4, hipMemcpyDeviceToHost);
            size_t nd = 0;
            for (size_t i = 0; i < on; ++i) nd += ref[i] != c[i];
            printf("pair %-24s: %zu of %zu output words differ from the chain\n", kn[v], nd, on);
            bad += nd;
        }
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        auto timed = [&](const char* name, int round, auto&& f) {
            for (int i = 0; i < 2; ++i) f();
            (void)hipEventRecord(e0, 0);
            for (int i = 0; i < it; ++i) f();
            (void)hipEventRecord(e1, 0);
            (void)hipEventSynchronize(e1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            printf("round %d %-30s %7.1f us\n", round, name, 1e3f * ms / it);
        };
        for (int round = 0; round < 5; ++round) {
            timed("chain A (32->64)", round, [&]() { chainA(); });
            timed("chain B (64->64)", round, [&]() { chainB(out); });
            timed("chain A + B", round, [&]() { chainA(); chainB(out); });
            for (int v = 0; v < NV; ++v) {
                char nm[48];
                snprintf(nm, sizeof nm, "pair %s", kn[v]);
                timed(nm, round, [&]() { pair(v, out2); });
            }
        }
        return bad ? 1 : 0;
    }
    if (which == 32 || which == 33) {  // conv_wg (channel split) vs conv_wgp (plane split): outputs compared, then timed
        const int iters = which == 33 ? 2 : it;
        const int Hin = 48, Win = 70, cout = 128, Hc = Hin - 8, Wc = Win - 2, Hout = Hc / 3, Wout = Wc / 3;
        const int tiles_h = (Hout * 3 + 38) / 39, tiles_w = (Wout * 3 + 5) / 6;
        const size_t on = (size_t)n * Hout * Wout * cout;
        void* out2;
        (void)hipMalloc(&out2, on * 4);
        auto k0 = conv_wg<9, 64, 1, 4, 3, 1, 3, 39, 6, 0, false, true, 0, 6, 1, 2>;
        auto k1 = conv_wgp<9, 64, 4, 3, 4, 3, 39, 6, 0, false, true, 0, 6, 2>;
        const size_t l0 = wg_lds_bytes<9, 64, 39, 6, 6, 1, 4>(), l1 = wgp_lds_bytes<9, 39, 6, 6, 3>();
        (void)hipFuncSetAttribute((const void*)k0, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l0);
        (void)hipFuncSetAttribute((const void*)k1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l1);
        dim3 grid(tiles_h * tiles_w, cout / 64, n);
        auto r0 = [&](void* o) { hipLaunchKernelGGL(k0, grid, dim3(256), l0, 0, (const float*)in, Hin, Win, (const bf16*)w, b, (float*)o, Hout, Wout, cout, tiles_w, 1, 0.3f); };
        auto r1 = [&](void* o) { hipLaunchKernelGGL(k1, grid, dim3(256), l1, 0, (const float*)in, Hin, Win, (const bf16*)w, b, (float*)o, Hout, Wout, cout, tiles_w, 1, 0.3f); };
        (void)hipMemset(out, 0xff, on * 4);
        (void)hipMemset(out2, 0xee, on * 4);
        r0(out);
        r1(out2);
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel error\n"); return 2; }
        std::vector<uint32_t> a(on), c(on);
        (void)hipMemcpy(a.data(), out, on * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(c.data(), out2, on * 4, hipMemcpyDeviceToHost);
        size_t nd = 0;
        for (size_t i = 0; i < on; ++i) nd += a[i] != c[i];
        printf("LDS wg %zu wgp %zu: %zu of %zu output words differ\n", l0, l1, nd, on);
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        for (int round = 0; round < 3; ++round)
            for (int v = 0; v < 2; ++v) {
                for (int i = 0; i < 2; ++i) v ? r1(out2) : r0(out);
                (void)hipEventRecord(e0, 0);
                for (int i = 0; i < iters; ++i) v ? r1(out2) : r0(out);
                (void)hipEventRecord(e1, 0);
                (void)hipEventSynchronize(e1);
                float ms = 0;
                (void)hipEventElapsedTime(&ms, e0, e1);
                printf("%s %7.1f us\n", v ? "conv_wgp (plane split)  " : "conv_wg (channel split) ", 1e3f * ms / iters);
            }
        return nd ? 1 : 0;
    }
    if (which == 21) {  // the shipped fused kernel, three timings (variant A/B across builds)
        FS(0) FS(0) FS(0)
        return 0;
    }
    if (which == 23) {
        // the shipped fused kernel's output words on seeded first-layer weights of both signs:
        // written to argv[2]; compared word for word with argv[3] (the file another build wrote) when given
        if (argc < 3) { printf("usage: conv_bench_x3 23 OUT.bin [OTHER.bin]\n"); return 2; }
        srand(23);
        for (auto& x : hw1) x = (rand() & 0xffff) / 65536.f - 0.5f;
        for (auto& x : hb1) x = 0.2f * ((rand() & 0xffff) / 65536.f - 0.5f);
        (void)hipMemcpy(w1, hw1.data(), hw1.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(b1, hb1.data(), hb1.size() * 4, hipMemcpyHostToDevice);
        const std::vector<uint8_t> li = pack_first_lanes(hw1.data(), hb1.data());
        (void)hipMemcpy(const_cast<void*>(f1.img), li.data(), li.size(), hipMemcpyHostToDevice);
        const size_t words = (size_t)n * 52 * 74 * 32;  // pooled 156 x 222 -> 52 x 74, 32 channels, 4 B each (grouped split)
        (void)hipMemset(out, 0, words * 4);
        time_one<3, 3, 32, 4, 1, 4, 2, 3, 12, 21, true, 0, false, true, 0, false, true>("c1+c2", n, 158, 224, 32, in, w, b, out, f1, 1);
        std::vector<uint32_t> o(words), other(words);
        (void)hipMemcpy(o.data(), out, words * 4, hipMemcpyDeviceToHost);
        FILE* f = fopen(argv[2], "wb");
        if (!f || fwrite(o.data(), 4, words, f) != words) { printf("cannot write %s\n", argv[2]); return 2; }
        fclose(f);
        size_t nz = 0;
        for (uint32_t x : o) nz += x != 0;
        printf("fused stage: %zu output words (%zu nonzero) -> %s\n", words, nz, argv[2]);
        if (argc > 3) {
            f = fopen(argv[3], "rb");
            if (!f || fread(other.data(), 4, words, f) != words) { printf("cannot read %s\n", argv[3]); return 2; }
            fclose(f);
            size_t nd = 0;
            for (size_t i = 0; i < words; ++i) nd += o[i] != other[i];
            printf("fused stage: %zu of %zu output words differ from %s\n", nd, words, argv[3]);
            return nd ? 1 : 0;
        }
        return 0;
    }
    if (which == 22) {  // per-wave phase timestamps of the shipped fused kernel -> gpurun_out/fused_ts.bin
        FS(0)
        const size_t cnt = (size_t)9152 * 4 * 10;
        std::vector<unsigned long long> ts(cnt);
#define TSD(D)                                                                                                        \
        time_one<3, 3, 32, 4, 1, 4, 2, 3, 12, 21, true, 4096 | D, false, true, 0, false, true>("c1+c2 ts" #D, n, 158, 224, 32, in, w, b, out, f1, 1); \
        (void)hipMemcpy(ts.data(), (char*)out + (64u << 22), cnt * 8, hipMemcpyDeviceToHost);                         \
        { FILE* f = fopen("gpurun_out/fused_ts_" #D ".bin", "wb"); fwrite(ts.data(), 8, cnt, f); fclose(f); }
        TSD(0) TSD(8192) TSD(16384) TSD(32768) TSD(57344) TSD(64) TSD(2)
        return 0;
    }
    if (which == 20) {  // the shipped fused kernel once (PMC passes)
        time_one<3, 3, 32, 4, 1, 4, 2, 3, 12, 21, true, 0, false, true, 0, false, true>("c1+c2", n, 158, 224, 32, in, w, b, out, f1, 1);
        W5(2, 2, 4, 2, 39, 6, 2, 0)
        return 0;
    }
    if (which == 18) {  // LDS bank conflicts of the fused kernel by phase (PMC): full, no conv1 compute, no MFMA loop
        ABL2(66) ABL2(70) ABL2(578) ABL2(582)
        return 0;
    }
    if (which == 17) {  // the shipped fused first conv and Winograd 9x3 once each (PMC passes)
        time_one<3, 3, 32, 4, 1, 3, 2, 3, 9, 21, true, 0, false, true, 4, false, true>("c2", n, 158, 224, 32, in, w, b, out, f1, 1);
        W5(2, 2, 4, 2, 39, 6, 2, 0)
        return 0;
    }
    if (which == 16) {  // the fused first conv: B latency (16: weights of step 0 re-read, L1-resident)
        ABL2(0) ABL2(16) ABL2(128) ABL2(144) ABL2(1) ABL2(17) ABL2(2)
        return 0;
    }
    if (which == 15) {  // the shipped 9x3 Winograd tile: staging / MFMA ablations
        W5(2, 2, 4, 2, 39, 6, 2, 0) W5(2, 2, 4, 2, 39, 6, 2, 1) W5(2, 2, 4, 2, 39, 6, 2, 2) W5(2, 2, 4, 2, 39, 6, 2, 3)
        C5(2, 2, 4, 2, 21, 6)
        return 0;
    }
    if (which == 14) {
        W5(2, 2, 2, 2, 21, 6, 0, 0) W5(2, 2, 2, 2, 21, 6, 0, 1) W5(2, 2, 2, 2, 21, 6, 0, 2) W5(2, 2, 2, 2, 21, 6, 0, 3)
        W5(2, 2, 4, 2, 39, 6, 0, 0) W5(2, 2, 4, 2, 39, 6, 2, 0) W5(4, 1, 2, 4, 21, 6, 0, 0) W5(2, 2, 2, 4, 21, 6, 0, 0)
        W5(1, 2, 4, 2, 21, 6, 0, 0) W5(2, 1, 2, 4, 21, 6, 0, 0) W5(2, 2, 2, 2, 21, 6, 2, 0) W5(2, 2, 2, 2, 21, 6, 4, 0)
        W5(4, 2, 2, 2, 39, 6, 0, 0) W5(2, 2, 3, 2, 15, 12, 0, 0)
        W4(2, 2, 2, 2, 8, 16, 0, 0) W4(2, 2, 2, 2, 8, 16, 0, 1) W4(2, 2, 2, 2, 8, 16, 0, 2) W4(2, 2, 3, 2, 12, 16, 0, 0)
        W4(2, 2, 4, 2, 16, 16, 0, 0) W4(2, 2, 2, 2, 4, 32, 0, 0) W4(4, 2, 2, 2, 16, 16, 0, 0) W4(2, 2, 4, 2, 8, 32, 0, 0)
        W3(2, 2, 2, 2, 8, 16, 0, 0) W3(2, 2, 2, 2, 8, 16, 0, 1) W3(2, 2, 2, 2, 8, 16, 0, 2) W3(2, 2, 3, 2, 12, 16, 0, 0)
        W3(2, 2, 4, 2, 16, 16, 0, 0) W3(4, 2, 2, 2, 16, 16, 0, 0) W3(2, 2, 4, 2, 8, 32, 0, 0)
        W6(2, 2, 2, 2, 13, 8, 0, 0) W6(2, 2, 5, 2, 13, 20, 0, 0) W6(2, 2, 3, 2, 13, 12, 0, 0) W6(1, 2, 4, 2, 13, 8, 0, 0)
        return 0;
    }
    if (which == 13) {
        // data dependence: the same tiles on random bit patterns (the default
        // fill) and on properly split N(0,1) activations / N(0,0.05) weights
        S5(2, 2, 4, 2, 21, 6, false, true, 4) S5(4, 2, 4, 4, 39, 6, false, true, 2) S4(2, 2, 3, 2, 12, 8, true, true, 4)
        F2(4, 1, 3, 2, 9, 21, false, 4)
        std::vector<uint16_t> hs(h.size() * 2), ws(hw.size());
        unsigned st = 1;
        auto gauss = [&]() {
            float a = 0;
            for (int k = 0; k < 4; ++k) { st = st * 1664525u + 1013904223u; a += (st >> 8) * (1.f / 16777216.f) - 0.5f; }
            return a * 1.7f;
        };
        auto split = [](float x, uint16_t& hi, uint16_t& lo) {
            uint32_t u; memcpy(&u, &x, 4);
            uint32_t r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000u;
            float hf; memcpy(&hf, &r, 4);
            float l = x - hf; uint32_t v; memcpy(&v, &l, 4);
            v = (v + 0x7fff + ((v >> 16) & 1)) >> 16;
            hi = (uint16_t)(r >> 16); lo = (uint16_t)v;
        };
        // grouped split: per 32 channels 32 hi then 32 lo
        for (size_t px = 0; px < hs.size() / 64; ++px)
            for (int c = 0; c < 32; ++c) split(gauss(), hs[px * 64 + c], hs[px * 64 + 32 + c]);
        for (size_t r = 0; r < ws.size() / 64; ++r)
            for (int c = 0; c < 32; ++c) split(0.05f * gauss(), ws[r * 64 + c], ws[r * 64 + 32 + c]);
        (void)hipMemcpy(in, hs.data(), std::min(hs.size() * 2, h.size() * 4), hipMemcpyHostToDevice);
        (void)hipMemcpy(w, ws.data(), ws.size() * 2, hipMemcpyHostToDevice);
        printf("-- split N(0,1) data --\n");
        S5(2, 2, 4, 2, 21, 6, false, true, 4) S5(4, 2, 4, 4, 39, 6, false, true, 2) S4(2, 2, 3, 2, 12, 8, true, true, 4)
        F2(4, 1, 3, 2, 9, 21, false, 4)
        return 0;
    }
    if (which == 12) {
        S5(2, 2, 4, 4, 21, 6, false, true, 2) S5(2, 2, 4, 4, 21, 6, false, true, 0) S5(2, 2, 4, 4, 21, 6, false, true, 3)
        S5(2, 2, 4, 4, 21, 6, true, true, 2) S5(2, 2, 5, 4, 24, 6, false, true, 2) S5(2, 2, 3, 4, 15, 6, false, true, 2)
        S5(2, 2, 4, 2, 21, 6, false, true, 4) S5(4, 1, 2, 4, 21, 6, false, true, 4) S5(2, 1, 4, 8, 21, 6, false, true, 2)
        S5(2, 2, 8, 4, 39, 6, false, true, 2) S5(2, 2, 8, 4, 39, 6, false, true, 1) S5(2, 1, 4, 4, 21, 6, false, true, 4)
        S5(1, 2, 8, 4, 21, 6, false, true, 2) S5(2, 2, 4, 4, 21, 6, false, false, 2) S5(2, 4, 4, 2, 21, 6, false, true, 2)
        S4(2, 2, 3, 2, 8, 12, true, true, 4) S4(2, 2, 3, 2, 8, 12, true, true, 0) S4(2, 2, 3, 2, 8, 12, false, true, 4)
        S4(2, 2, 4, 2, 8, 16, true, true, 4) S4(2, 2, 3, 2, 6, 16, true, true, 4) S4(2, 2, 2, 2, 4, 16, true, true, 4)
        S4(2, 1, 3, 4, 8, 12, true, true, 4) S4(2, 2, 3, 2, 12, 8, true, true, 4) S4(2, 2, 4, 2, 10, 12, true, true, 4)
        S3(2, 2, 3, 2, 8, 12, true, true, 0) S3(2, 2, 3, 2, 8, 12, true, false, 0) S3(2, 2, 4, 2, 8, 16, true, false, 0)
        S3(2, 2, 3, 2, 6, 16, true, false, 0) S3(2, 2, 2, 2, 4, 16, true, false, 0) S3(4, 2, 3, 2, 10, 18, true, false, 4)
        S3(2, 2, 4, 2, 10, 12, true, false, 0) S3(2, 1, 3, 4, 8, 12, true, false, 0)
        S6(2, 2, 3, 2, 7, 12, true, true, 4) S6(2, 2, 3, 2, 7, 12, true, false, 0) S6(2, 2, 2, 2, 4, 16, true, true, 4)
        S6(2, 1, 3, 4, 7, 12, true, true, 4) S6(2, 2, 3, 2, 7, 12, false, true, 4)
        F2(4, 1, 3, 2, 9, 21, false, 4) F2(4, 1, 3, 2, 9, 21, false, 0) F2(4, 1, 4, 2, 12, 21, false, 4)
        F2(4, 1, 6, 2, 12, 30, false, 3) F2(4, 1, 3, 2, 9, 21, true, 4) F2(4, 1, 2, 2, 6, 21, false, 4)
        return 0;
    }
    if (which == 10) {  // the shipped c5 / c2 tiles alone (PMC passes)
        C5(3, 2, 5, 2, 39, 6) C2(4, 1, 3, 2, 6, 30)
        return 0;
    }
    if (!which || which == 2) {
        G2(4, 1, 3, 2, 9, 21) G2(4, 1, 4, 2, 12, 21) G2(4, 1, 5, 2, 6, 48)
        J2(4, 1, 3, 2, 9, 21, false, 0) J2(4, 1, 4, 2, 12, 21, false, 0) J2(4, 1, 5, 2, 6, 48, false, 0)
        J2(4, 1, 6, 2, 12, 30, false, 0) J2(4, 1, 8, 2, 12, 42, false, 0) J2(4, 1, 6, 2, 18, 21, false, 0)
        J2(4, 1, 3, 2, 9, 21, false, 4) J2(4, 1, 4, 2, 12, 21, false, 4) J2(4, 1, 6, 2, 12, 30, false, 3)
        J2(4, 1, 4, 2, 12, 21, true, 0) J2(4, 1, 6, 2, 12, 30, true, 0)
    }
    if (!which || which == 3) {
        C3(4, 2, 3, 2, 10, 18) J3(4, 2, 3, 2, 10, 18, true, 0) J3(4, 2, 3, 2, 10, 18, true, 4)
        J3(4, 2, 4, 2, 10, 24, true, 0) J3(4, 2, 4, 2, 10, 24, true, 4) J3(4, 2, 3, 2, 10, 18, false, 4)
        J3(4, 2, 6, 2, 25, 12, true, 0) J3(4, 2, 5, 2, 25, 12, true, 0)
    }
    if (!which || which == 4) {
        C4(4, 2, 3, 2, 12, 14) J4(4, 2, 3, 2, 12, 14, true, 0) J4(4, 2, 3, 2, 12, 14, true, 4)
        J4(4, 2, 4, 2, 16, 14, true, 0) J4(4, 2, 4, 2, 16, 14, true, 4) J4(4, 2, 4, 2, 16, 14, false, 4)
        J4(4, 2, 6, 2, 24, 14, true, 0) J4(4, 2, 7, 2, 16, 28, true, 0) J4(2, 2, 7, 2, 16, 14, true, 0)
    }
    if (!which || which == 5) {
        G5(4, 2, 4, 2, 39, 6) J5(4, 2, 4, 2, 39, 6, false, 0) J5(4, 2, 4, 2, 39, 6, false, 4)
        J5(4, 2, 4, 2, 39, 6, true, 0) J5(4, 2, 4, 2, 39, 6, true, 4) J5(4, 1, 4, 4, 39, 6, false, 0)
        J5(4, 1, 4, 4, 39, 6, false, 4) J5(8, 2, 4, 2, 39, 12, false, 0) J5(8, 2, 4, 2, 39, 12, false, 4)
        J5(4, 2, 2, 2, 3, 33, false, 4) J5(2, 2, 4, 2, 3, 33, false, 4) J5(4, 2, 4, 2, 6, 33, false, 4)
        J5(4, 2, 4, 4, 39, 6, false, 0) J5(4, 2, 4, 4, 39, 6, false, 2)
    }
    if (!which || which == 6) {
        C6(4, 2, 3, 2, 7, 20) J6(4, 2, 3, 2, 7, 20, true, 0) J6(4, 2, 3, 2, 7, 20, true, 4)
        J6(4, 2, 5, 2, 13, 20, true, 0) J6(4, 1, 3, 4, 7, 20, true, 0)
    }
    hipError_t e = hipGetLastError();
    printf("last error: %s\n", hipGetErrorString(e));
    return 0;
}
