/*
 * aa.h -- C ABI of libaa.so, the MI355X (gfx950) hot path of the
 * audio-analysis window classifier.
 *
 * Every entry point is plain C: device pointers, sizes, an opaque handle and a
 * hipStream_t passed as void*.  No torch types cross this boundary.  Buffers
 * are owned by the caller (the Python host keeps them in torch-ROCm tensors);
 * the library allocates only per-handle constants (filterbank, twiddles,
 * packed weights) at create time, never inside a *_run / *_forward call, so
 * those calls can be captured into a HIP graph.
 *
 * Reference interfaces each group replaces (file:line in
 * TheCacophonyProject/audio-analysis, mounted at /root/reference):
 *   aa_fe_*      get_spect(...)                     src/identify_tracks.py:212-288
 *                  + normalize_data                 src/identify_tracks.py:202-209
 *                  + the per-window loop body       src/identify_tracks.py:163-193
 *                  + custommel.mel_spec / mel_f     src/custommel.py:19-63
 *   aa_model_*   load_model(path, meta)             src/identify_tracks.py:302-327
 *                model.predict(np.array(d))         src/identify_tracks.py:544
 *                MagTransform.call                  src/magtransformv2.py:19-21
 *   aa_track_mean  np.mean over models, windows     src/identify_tracks.py:547-551
 *   aa_span_nonzero  get_end                        src/identify_tracks.py:387-413
 *   aa_sosfilt_*  butter_bandpass_filter's sosfilt   src/identify_tracks.py:152-162,
 *                                                      :1036-1056
 *   aa_pcm_s16_to_f32  load_recording's s16 -> f32  src/identify_tracks.py:49-62
 *   aa_resample_poly   load_recording's resample     src/identify_tracks.py:49-62
 *   aa_sn_*      signal_noise                       src/identify_tracks.py:650-706
 *   aa_ci_*      get_ci_bins + calculate's frame    src/cacophony_index.py:53-97
 *                  loop (the old cacophony index)
 *   aa_flac_*    load_recording's ffmpeg decode     src/identify_tracks.py:49-62
 *                  (FLAC; host memory, no GPU)
 *   aa_vorbis_*  load_recording's ffmpeg decode     src/identify_tracks.py:49-62
 *                  (Ogg Vorbis; host memory, no GPU)
 *
 * Return values: AA_OK (0) or an aa_status code; aa_last_error() gives a
 * thread-local message for the last failing call on this thread.
 */
#ifndef AA_H
#define AA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AA_ABI_VERSION 5

typedef enum aa_status {
    AA_OK = 0,
    AA_ERR_INVALID = 1,      /* bad argument / shape */
    AA_ERR_HIP = 2,          /* HIP runtime error */
    AA_ERR_UNSUPPORTED = 3,  /* layer pattern or size this build has no kernel for */
    AA_ERR_WORKSPACE = 4,    /* workspace too small */
} aa_status;

/* One analysis window of `win_len` samples, as a view into the recording:
 * samples [src, src + n_valid) of the PCM buffer, placed at offset pad_left
 * inside the window; every other window sample is 0 (np.pad,
 * src/identify_tracks.py:165-168).  16 bytes, device-resident array. */
typedef struct aa_window {
    int64_t src;
    int32_t n_valid;
    int32_t pad_left;
} aa_window;

/* Front-end configuration (the reference's metadata.txt keys,
 * src/identify_tracks.py:466-497). */
typedef struct aa_fe_config {
    int32_t win_len;   /* samples per window: int(sr * segment_length) */
    int32_t n_fft;     /* 256..8192: a power of two, or a multiple of 16 whose
                        * sixteenth has only the factors 2, 3, 5 (4800, 1200) */
    int32_t hop;       /* hop_length */
    int32_t n_mels;    /* rows of the filterbank */
    int32_t normalize; /* normalize_data before the STFT */
    int32_t db_scale;  /* librosa.power_to_db(ref=np.max) */
    float power;       /* |S| ** power before the filterbank */
    float amin;        /* power_to_db amin (1e-10) */
    float top_db;      /* power_to_db top_db (80) */
    int32_t mean_sub;  /* subtract each band's mean over time */
    int32_t channels;  /* repeat the single channel this many times */
    int32_t out_f16;   /* 1: aa_fe_run writes float16 log-mel (BASELINE configs[4]),
                        * 0: float32 (what get_spect returns) */
} aa_fe_config;

/* Per-window status flags written by aa_fe_run (device int32 array). */
#define AA_WIN_OK 0
#define AA_WIN_NONFINITE 1 /* librosa.util.valid_audio would raise */

int aa_abi_version(void);
const char* aa_last_error(void);

/* ---------------- front end: PCM windows -> log-mel ---------------- */
/* melfb: host float32 [n_mels][n_fft/2 + 1] dense filterbank (custommel.mel_f
 * or the Slaney filterbank); stored on the device in CSR form.
 * cfg->n_fft: 256 <= n_fft <= 8192 and either a power of two (256, 512, 1024,
 * 2048, 4096, 8192) or a multiple of 16 with n_fft / 16 = 2^a 3^b 5^c (400,
 * 960, 1200, 1920, 2400, 4800, 7776, ...); any other value (odd sizes, a
 * factor 7 or larger, 8 mod 16 such as 1000) is AA_ERR_UNSUPPORTED before any
 * device call.  The powers of two 256..1024 take any hop; every other size
 * refuses a hop whose six-frame span does not fit the LDS. */
int aa_fe_create(const aa_fe_config* cfg, const float* melfb, void** plan);
int aa_fe_destroy(void* plan);
/* frames per window T = 1 + win_len / hop */
int aa_fe_n_frames(const void* plan);
size_t aa_fe_workspace_bytes(const void* plan, int32_t max_windows);
/* out: device [n_win][n_mels][T][channels] (NHWC, H = mel band, W = frame),
 * the tensor get_spect returns per window: float32, or float16 (round to
 * nearest) when cfg.out_f16.
 * win_status: device int32 [n_win] (AA_WIN_*), may be NULL. */
int aa_fe_run(void* plan, const float* pcm, int64_t pcm_len, const aa_window* windows,
              int32_t n_win, void* out, int32_t* win_status, void* workspace,
              size_t workspace_bytes, void* stream);
/* Launch stages of aa_fe_run and their timing, same contract as
 * aa_model_stage_* below: 0 fe_stats, 2 fe_db (csrc/aa_frontend.hip), 1 the
 * stft + mel kernel the plan chose (csrc/aa_fe_plan.h choose_kernel; its name
 * is stage_info's): fe_stft_mel_small at n_fft 256..1024, fe_stft_mel from
 * 2048 up (both csrc/aa_fe_stft.h), fe_stft_mel_4096 at n_fft 4096 with the
 * kept band inside X[2..1022] (csrc/aa_fe_wave4096.h), fe_stft_mel_mixed at
 * every n_fft that is not a power of two (csrc/aa_fe_stft.h too: Stockham passes
 * of radix 8, 5, 4, 3, 2 by the plan's schedule, aa_fe_plan_passes; its flops
 * per item are counted from that schedule). */
int aa_fe_n_stages(const void* plan);
int aa_fe_stage_info(const void* plan, int32_t stage, char* name, int32_t name_len,
                     double* flops_per_item, double* bytes_per_item);
int aa_fe_set_timing(void* plan, uint32_t stage_mask);
int aa_fe_stage_time(void* plan, int32_t stage, double* total_ms, int64_t* count);

/* The plan alone, on the host (the aa_model_plan contract): aa_fe_create's
 * arguments, checks, return codes and aa_last_error texts, but no device
 * memory and no HIP call.  aa_fe_n_frames / workspace_bytes / n_stages /
 * stage_info / destroy serve a planned plan; aa_fe_run, aa_fe_set_timing and
 * aa_fe_stage_time return AA_ERR_INVALID. */
typedef enum aa_fe_kernel {
    AA_FE_K_SMALL = 0, AA_FE_K_WAVE4096 = 1, AA_FE_K_GENERIC = 2, AA_FE_K_MIXED = 3
} aa_fe_kernel;
typedef struct aa_fe_info {
    int32_t kernel;    /* aa_fe_kernel: the stft launch (stage 1) */
    int32_t T;         /* frames per window */
    int32_t kmin;      /* first and last filterbank bin with a nonzero weight */
    int32_t kmax;      /* (0, 0 for an all-zero filterbank) */
    int32_t nnz;       /* CSR values */
    int32_t nparts;    /* per-window partial maxima that fe_db reads */
    int64_t lds_bytes; /* dynamic LDS of the stft launch */
    int32_t grid;      /* its blocks for n_win windows */
} aa_fe_info;
int aa_fe_plan(const aa_fe_config* cfg, const float* melfb, void** plan);
int aa_fe_plan_info(const void* plan, int32_t n_win, aa_fe_info* out);
/* The bytes aa_fe_create would upload (the aa_model_stage_image contract: *len
 * the image's bytes; buf NULL: size query; AA_ERR_INVALID when cap < *len;
 * planned plans only, a created one has released them: AA_ERR_UNSUPPORTED).
 * which = 0 the periodic Hann f32 [n_fft], 1 tw = exp(-2 pi i m / (n_fft/2))
 * float2 [n_fft/2], 2 tw2 = exp(-2 pi i k / n_fft) float2 [n_fft/2 + 1], 3 the
 * CSR rows int32x4 [n_mels] (first bin, count, value offset, 0), 4 the CSR
 * values f32, 5 fe_stft_mel_4096's image (len 0 unless n_fft is 4096). */
int aa_fe_plan_image(const void* plan, int32_t which, void* buf, size_t cap, size_t* len);
/* The Stockham passes of the plan's n_fft/2-point complex transform, planned or
 * created: *n radices whose product is n_fft/2, written to radices[0 .. *n)
 * (at most 8; AA_ERR_INVALID with *n set when cap < *n; radices NULL with
 * cap 0: a count query).  AA_FE_K_MIXED runs exactly this schedule: 8 first
 * (from the samples), then every further 8, the 5s, one 4, the 3s, one 2, each
 * in {2, 3, 4, 5, 8}.  The other kernels report the passes built into them
 * (8, 8, 8, 4 at 4096 AA_FE_K_GENERIC; AA_FE_K_WAVE4096's register DFT-32s as
 * 8, 4 each: 8, 4, 8, 4, 2). */
int aa_fe_plan_passes(const void* plan, int32_t* radices, int32_t cap, int32_t* n);

/* ---------------- CNN: log-mel windows -> logits / probabilities ---------------- */
/* Supported layer sequences: [MagTransform] then Conv2D blocks (Conv2D
 * [BatchNormalization] [LeakyReLU|ReLU] [MaxPooling2D]) ending in either a
 * 1x1 Conv2D + GlobalMaxPool2D [+ sigmoid] head or GlobalMaxPool2D [+ Dense]
 * [+ sigmoid].  Tuned matrix-core kernels serve the build's model family
 * (stage names "conv_*"); any other conv shape or pool window runs a generic
 * f32 kernel (stage name "conv_generic_*"; not in the fp8 mode). */
typedef enum aa_op {
    AA_OP_CONV2D = 1,       /* Keras Conv2D, padding="valid", stride 1 */
    AA_OP_BATCHNORM = 2,    /* inference BatchNormalization (moving stats) */
    AA_OP_LEAKYRELU = 3,
    AA_OP_MAXPOOL2D = 4,    /* pool = strides, padding="valid" */
    AA_OP_GLOBALMAXPOOL2D = 5,
    AA_OP_SIGMOID = 6,
    AA_OP_MAGTRANSFORM = 7, /* x ** sigmoid(a) */
    AA_OP_RELU = 8,
    AA_OP_DENSE = 9,        /* after GlobalMaxPool2D: filters = units,
                             * off[0] = kernel [C_in][units], off[1] = bias */
} aa_op;

typedef struct aa_layer {
    int32_t op;      /* aa_op */
    int32_t kh, kw;  /* conv kernel or pool size */
    int32_t filters; /* conv output channels */
    float alpha;     /* leaky slope */
    float eps;       /* batchnorm epsilon */
    /* offsets (in floats) into the weight blob, -1 when absent:
     * conv: [0]=kernel (HWIO [kh][kw][cin][cout]), [1]=bias
     * batchnorm: [0]=gamma [1]=beta [2]=moving_mean [3]=moving_variance
     * magtransform: [0]=a */
    int64_t off[4];
} aa_layer;

typedef enum aa_precision {
    AA_PREC_F32 = 0,  /* f32 MFMA (exact f32 fma chain): the parity mode */
    AA_PREC_BF16 = 1, /* bf16 activations/weights, f32 accumulation */
    AA_PREC_FP8 = 2,  /* OCP e4m3fn activations/weights (per-output-channel weight
                       * scales), f32 accumulation; f32 log-mel input, the first
                       * conv on bf16 hi+lo as in AA_PREC_BF16 */
    AA_PREC_BF16X3 = 3, /* split bf16: f32 activations, operands split into
                         * bf16 hi + lo, hi*hi + hi*lo + lo*hi on bf16 MFMA
                         * with f32 accumulation (~17-bit products): meets the
                         * 1e-3 logit gate; the default of classify() */
} aa_precision;

int aa_model_create(const aa_layer* layers, int32_t n_layers, const float* blob, int64_t blob_len,
                    int32_t in_h, int32_t in_w, int32_t in_c, int32_t precision, void** model);
int aa_model_destroy(void* model);
int aa_model_n_outputs(const void* model);
size_t aa_model_workspace_bytes(const void* model, int32_t max_batch);
/* x: device [n][in_h][in_w][in_c], float32 (or float16 after
 * aa_model_set_input_f16(model, 1)); logits: device float32 [n][L]
 * (global-max outputs before the sigmoid); probs: [n][L] or NULL. */
int aa_model_forward(void* model, const void* x, int32_t n, float* logits, float* probs,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Model input as float16 (aa_fe_config.out_f16): served when the first
 * conv is fused into the second (the build's model family: 3x3 C_in = 1 ->
 * 32 before a pooled 3x3/32 conv), which converts the log-mel to f32 as it
 * stages it; AA_ERR_UNSUPPORTED otherwise. */
int aa_model_set_input_f16(void* model, int32_t f16);

/* Per-stage timing of aa_model_forward (HIP events around each stage whose
 * bit is set in stage_mask, on the launch stream; 0 disables).  Used by
 * bench.py for the roofline of the dominant kernel.  stage_info reports the
 * algorithmic flops / HBM bytes of one window (item) through the stage. */
int aa_model_n_stages(const void* model);
int aa_model_stage_info(const void* model, int32_t stage, char* name, int32_t name_len,
                        double* flops_per_item, double* bytes_per_item);
int aa_model_set_timing(void* model, uint32_t stage_mask);
int aa_model_stage_time(void* model, int32_t stage, double* total_ms, int64_t* count);

/* Read-out of one stage's activations, for per-stage checks against a
 * reference.  stage_shape: Hout, Wout, C_out of what the stage stores (any
 * pointer may be NULL); AA_ERR_UNSUPPORTED, with the reason in
 * aa_last_error, for a stage whose output never reaches memory as
 * activations: a first conv computed inside the next stage, the conv inside
 * the fused tail, and the stage that writes the logits.
 * forward_prefix: launches stages 0..stage exactly as aa_model_forward does
 * (same kernels, flags and workspace layout), then decodes that stage's
 * stored output to act, device float32 [n][Hout][Wout][C_out]: f32 copied,
 * bf16 / e4m3fn widened, the split-bf16 grouped layout summed hi + lo -- all
 * exact.  Allocates nothing; n <= 32768; workspace as for aa_model_forward. */
int aa_model_stage_shape(const void* model, int32_t stage, int32_t* h, int32_t* w, int32_t* c);
int aa_model_forward_prefix(void* model, const void* x, int32_t n, int32_t stage, float* act,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The plan alone, on the host: aa_model_create's arguments, checks, return
 * codes and aa_last_error texts, but no device memory and no HIP call, so it
 * runs on a machine without a GPU.  aa_model_n_stages / stage_info /
 * stage_shape / n_outputs / workspace_bytes / destroy serve a planned model;
 * aa_model_forward, aa_model_forward_prefix and aa_model_set_input_f16
 * return AA_ERR_INVALID.
 * stage_image copies out the bytes aa_model_create would upload for a stage:
 * which = 0 the packed weights (len 0: the stage reads a null pointer), 1 the
 * bias (fp8: followed by the dequantisation scales), 2 the fused tail's head
 * weights (len 0 unless the stage is the fused tail).  *len: the image's
 * bytes; buf NULL: size query; AA_ERR_INVALID when cap < *len.  Planned
 * models only: a created model has released its host images
 * (AA_ERR_UNSUPPORTED).
 * first_lane_image, same contract: the split-bf16 fused first conv's per-lane
 * image (6 parts x 64 lanes x 16 B: the lane's two MFMA weight operands as
 * bf16, then its 16 bias values), uploaded with stage 1's weights; len 0 when
 * the model has no such stage. */
int aa_model_plan(const aa_layer* layers, int32_t n_layers, const float* blob, int64_t blob_len,
                  int32_t in_h, int32_t in_w, int32_t in_c, int32_t precision, void** model);
int aa_model_stage_image(const void* model, int32_t stage, int32_t which, void* buf, size_t cap, size_t* len);
int aa_model_first_lane_image(const void* model, void* buf, size_t cap, size_t* len);

/* ---------------- CNN graphs (DAG models: residual / squeeze-excite / depthwise) ---------------- */
/* Models that are not a single conv chain -- Keras Functional graphs such as
 * the EfficientNet family classify() routes by name (src/identify_tracks.py:
 * 539-540) -- as a node list in topological order.  Each node reads the
 * outputs of in0 / in1 (node indices; -1 = the model input) and writes one
 * NHWC f32 tensor per window.  The host folds BatchNormalization into a
 * preceding conv, resolves "same" padding into explicit pads and folds
 * ZeroPadding2D into the consumer's pads; activations are fused into their
 * producer where it is the only consumer.  Convs with C_in >= 16 run on the
 * runtime-shaped split-bf16 MFMA kernel (AA_PREC_BF16X3) or exact f32
 * (AA_PREC_F32); the rest is f32 VALU. */
typedef enum aa_gop {
    AA_G_CONV = 1,      /* off[0] = kernel HWIO [kh][kw][cin][filters], off[1] = bias (or -1) */
    AA_G_DWCONV = 2,    /* depthwise, depth multiplier 1: off[0] = kernel [kh][kw][C], off[1] = bias */
    AA_G_MAXPOOL = 3,   /* window kh x kw, strides, pads */
    AA_G_AVGPOOL = 4,   /* the average over the taps inside the image */
    AA_G_GMAXPOOL = 5,  /* -> [1][1][C] */
    AA_G_GAVGPOOL = 6,  /* -> [1][1][C] */
    AA_G_ADD = 7,       /* in0 + in1 (same shape) */
    AA_G_MUL = 8,       /* in0 * in1; in1 may be [1][1][C] (broadcast over H, W) */
    AA_G_AFFINE = 9,    /* x * off[0][c] + off[1][c] (standalone BatchNormalization, Rescaling,
                         * Normalization); off = -1: identity (activation only) */
    AA_G_DENSE = 10,    /* [1][1][C] (or any H x W, flattened) -> [1][1][filters]:
                         * off[0] = kernel [C][filters], off[1] = bias */
    AA_G_POW = 11,      /* x ** alpha (MagTransform: alpha = sigmoid(a)) */
} aa_gop;

typedef enum aa_gact {
    AA_GACT_NONE = 0, AA_GACT_RELU = 1, AA_GACT_LEAKY = 2, AA_GACT_SIGMOID = 3, AA_GACT_SWISH = 4
} aa_gact;

typedef struct aa_node {
    int32_t op;                  /* aa_gop */
    int32_t in0, in1;            /* producer nodes (-1: the model input; in1 unused: -1) */
    int32_t kh, kw, sh, sw;      /* window / kernel, strides */
    int32_t pt, pb, pl, pr;      /* explicit zero padding (top, bottom, left, right) */
    int32_t filters;             /* conv / dense outputs */
    int32_t act;                 /* aa_gact, applied last */
    float alpha;                 /* leaky slope (AA_G_POW: the exponent) */
    int64_t off[2];              /* weight blob offsets (floats), -1 when absent */
} aa_node;

/* The last node is the output [n][1][1][L] (or [n][H][W][L], flattened);
 * logits are its values before a sigmoid activation (equal to probs
 * otherwise). */
int aa_graph_create(const aa_node* nodes, int32_t n_nodes, const float* blob, int64_t blob_len, int32_t in_h,
                    int32_t in_w, int32_t in_c, int32_t precision, void** graph);
int aa_graph_destroy(void* graph);
int aa_graph_n_outputs(const void* graph);
size_t aa_graph_workspace_bytes(const void* graph, int32_t max_batch);
int aa_graph_forward(void* graph, const float* x, int32_t n, float* logits, float* probs, void* workspace,
                     size_t workspace_bytes, void* stream);
/* launches of one forward ("conv_gx3_*", "dwconv_*", ...), their algorithmic
 * flops / bytes per window */
int aa_graph_n_stages(const void* graph);
/* Node timing (HIP events around node launches): set_timing(mask != 0) times
 * every node, 0 none; time_stage(k) node k only (-1 every node, -2 none) --
 * a graph has more nodes than a 32-bit mask holds.  stage_time as
 * aa_model_stage_time. */
int aa_graph_set_timing(void* graph, uint32_t stage_mask);
int aa_graph_time_stage(void* graph, int32_t stage);
int aa_graph_stage_time(void* graph, int32_t stage, double* total_ms, int64_t* count);
int aa_graph_stage_info(const void* graph, int32_t stage, char* name, int32_t name_len, double* flops_per_item,
                        double* bytes_per_item);

/* The launch a node was planned for, chosen once from its shape when the
 * graph is planned (csrc/aa_graph_plan.h choose_kernel). */
typedef enum aa_gkernel {
    AA_GK_X3P = 1,             /* gconv_x3p: patch-staged, 256 pixels x 16 channels */
    AA_GK_X3T_256x16 = 2,      /* gconv_x3t tiles (pixels x channels) */
    AA_GK_X3T_128x32 = 3,
    AA_GK_X3T_64x128 = 4,
    AA_GK_X3T_SPLIT_KC2 = 5,   /* split K (+ gsplit_reduce), 2 / 1 chunks per K step */
    AA_GK_X3T_SPLIT_KC1 = 6,
    AA_GK_X3T_64x64_KC2 = 7,
    AA_GK_X3T_64x64_PD2 = 8,   /* one chunk per step, two steps in flight */
    AA_GK_X3T_64x64 = 9,
    AA_GK_MATVEC = 10,         /* gmatvec: 1x1 conv on a 1x1 map */
    AA_GK_MATVEC_T = 11,       /* gmatvec_t: the same with K <= 64 */
    AA_GK_F32_S = 12,          /* gconv_f32_s<3, 3, 3> */
    AA_GK_F32_LDS_3x3x3 = 13,  /* gconv_f32_lds<3, 3, 3> */
    AA_GK_F32_LDS_3x3x1 = 14,  /* gconv_f32_lds<3, 3, 1> */
    AA_GK_F32_LDS = 15,        /* gconv_f32_lds<> */
    AA_GK_F32 = 16,            /* gconv_f32 */
    AA_GK_DWPOOL4_S1 = 17,     /* gdwconv_pool4<8, 3, 1, 1> */
    AA_GK_DWPOOL4_S2 = 18,     /* gdwconv_pool4<8, 3, 2, 1> */
    AA_GK_DWPOOL4_K3 = 19,     /* gdwconv_pool4<8, 3, 0, 1> */
    AA_GK_DWPOOL4 = 20,        /* gdwconv_pool4<8, 0, 0, 1> */
    AA_GK_DWPOOL = 21,         /* gdwconv_pool */
    AA_GK_DW4 = 22,            /* gdwconv<4> */
    AA_GK_DW1 = 23,            /* gdwconv<1> */
    AA_GK_POOL2D = 24,         /* gpool2d */
    AA_GK_GPOOL4 = 25,         /* ggpool4<16> */
    AA_GK_GPOOL = 26,          /* ggpool */
    AA_GK_BINARY = 27,         /* gbinary */
    AA_GK_AFFINE = 28,         /* gaffine */
    AA_GK_POW = 29,            /* gpow */
    AA_GK_DENSE = 30,          /* gmatvec over the flattened map */
} aa_gkernel;

/* One node of a planned graph, after the fusion passes. */
typedef struct aa_node_plan {
    int32_t H, W, C;                     /* output shape */
    int32_t kernel;                      /* aa_gkernel */
    int32_t bn, cout_pad, cin_pad;       /* MFMA convs: channel tile, padded C_out, C_in */
    int32_t split, cslice;               /* split K: slices, 32-channel chunks per slice */
    int32_t skip, nolaunch;              /* fused into a consumer / written by its producer */
    int32_t scale_src, res_src;          /* conv: squeeze-and-excite scale, residual (-2: none) */
    int32_t pool_into;                   /* depthwise conv: the global average pool it also writes (-2) */
    int32_t in0, in1, act;               /* aa_node's, as the fusions left them */
    float alpha;
    int32_t last_use;                    /* last node that reads the output */
    int64_t off;                         /* workspace offset, f32 elements per window */
} aa_node_plan;

/* The workspace of a planned graph, per window in f32 elements: node buffers
 * in [0, part_off), split-K partial sums in [part_off, per_win). */
typedef struct aa_graph_layout {
    int64_t per_win, part_off;
    int32_t n_outputs, sigmoid_out;      /* the output node's sigmoid is applied after the logits */
} aa_graph_layout;

/* The plan alone, on the host (as aa_model_plan): aa_graph_create's
 * arguments, checks, return codes and aa_last_error texts, but no device
 * memory and no HIP call.  aa_graph_n_stages / stage_info / n_outputs /
 * workspace_bytes / destroy serve a planned graph; aa_graph_forward returns
 * AA_ERR_INVALID.
 * node_image copies out the bytes aa_graph_create would upload for a node
 * (the aa_model_stage_image contract): which = 0 the weights, 1 the bias (an
 * affine node: its scale), 2 an affine node's shift, 3 the f32 stem's
 * [C_out / 32][K][32] image; len 0: the node reads a null pointer. */
int aa_graph_plan(const aa_node* nodes, int32_t n_nodes, const float* blob, int64_t blob_len, int32_t in_h,
                  int32_t in_w, int32_t in_c, int32_t precision, void** graph);
int aa_graph_node_plan(const void* graph, int32_t node, aa_node_plan* out);
int aa_graph_plan_layout(const void* graph, aa_graph_layout* out);
int aa_graph_node_image(const void* graph, int32_t node, int32_t which, void* buf, size_t cap, size_t* len);

/* ---------------- ensemble + window mean ---------------- */
/* probs: device float32, model m / window w at probs[m * model_stride + w * n_labels].
 * Track t averages windows [win_begin[t], win_begin[t] + win_count[t]) after
 * averaging over models, both in float32 with sequential accumulation like
 * numpy's axis-0 mean.  out: device float32 [n_tracks][n_labels]. */
int aa_track_mean(const float* probs, int32_t n_models, int64_t model_stride, int32_t n_labels,
                  const int32_t* win_begin, const int32_t* win_count, int32_t n_tracks,
                  float* out, void* stream);

/* ---------------------------------------------------------------- span scan */
/* flags[i] = 1 if any of pcm[spans[2i] .. spans[2i+1]) is nonzero, else 0.
 * Spans are caller-validated to lie in [0, n).  Backs get_end
 * (src/identify_tracks.py:387-413): a 170-frame chunk of the 4800/281 STFT has
 * a constant mel block exactly when every sample its frames cover is zero. */
int aa_span_nonzero(const float* pcm, int64_t n, const int64_t* spans, int32_t n_spans,
                    int32_t* flags, void* stream);

/* ---------------------------------------------------------------- band-pass filter */
/* butter_bandpass_filter's sosfilt over a track's sample range
 * (src/identify_tracks.py:152-162, :1036-1056): y = scipy.signal.sosfilt(sos,
 * x) with zero initial state, for a batch of jobs in one device PCM buffer.
 * f32 in, scipy's float64 direct-form-II-transposed arithmetic in scipy's
 * order (no fused multiply-add), one rounding to f32 out.
 *
 * The recurrence is linear in its 4-vector state (z0, z1 of section 0, then
 * of section 1): a zero-input step is s <- P s.  A job is cut into chunks of
 * AA_SOS_CHUNK samples, one lane each, AA_SOS_BLOCK samples per workgroup:
 * every lane runs its chunk from zero state, the end states are scanned with
 * the powers of P (inside the workgroup, then over the workgroups' aggregates
 * in a launch of its own), and every lane reruns its chunk from its true
 * start state.  Three launches, no workgroup waits on another. */
#define AA_SOS_MAX_SECTIONS 2
#define AA_SOS_CHUNK 32          /* samples per lane */
#define AA_SOS_BLOCK 8192        /* samples per workgroup: 256 lanes x AA_SOS_CHUNK */
#define AA_SOS_LEVELS 16         /* powers kept: P^(AA_SOS_CHUNK 2^k), k < 16 */
#define AA_SOS_MAX_N 268435456   /* samples per job, 2^28 */

/* One filter job: pcm[src, src + n) -> pcm[dst, dst + n).  Made on the host
 * by aa_sosfilt_plan, device-resident array for aa_sosfilt_run. */
typedef struct aa_sos_job {
    int64_t src, n, dst;         /* sample offsets into the PCM buffer */
    int32_t n_sections;          /* 1 (low-pass) or 2 (band-pass) */
    int32_t n_levels;            /* AA_SOS_LEVELS */
    double sos[12];              /* scipy rows b0 b1 b2 a0 a1 a2 */
    double p[16];                /* P, row-major: one zero-input step of the state */
    double pw[256];              /* level k at pw + 16 k: P^(AA_SOS_CHUNK 2^k) */
} aa_sos_job;

/* Host only, no HIP call.  sos: n_sections (1 or 2) scipy rows with a0 == 1
 * and finite coefficients; 0 <= n <= AA_SOS_MAX_N; src, dst >= 0.  P comes
 * from stepping unit states with zero input in the kernel's arithmetic, its
 * powers from repeated squaring in long double, rounded to double.
 * AA_ERR_INVALID (reason in aa_last_error) otherwise, also for a filter whose
 * powers overflow. */
int aa_sosfilt_plan(const double* sos, int32_t n_sections, int64_t src, int64_t n, int64_t dst, aa_sos_job* job);
/* Workspace of one aa_sosfilt_run over these (host) jobs; 0 for none. */
size_t aa_sosfilt_workspace_bytes(const aa_sos_job* jobs_host, int32_t n_jobs);
/* Runs every job (jobs_dev: device array; max_n: the largest job's n).
 * No dst range may overlap a src range or another dst range.  Before any
 * launch: null pointers and max_n > n_pcm or > AA_SOS_MAX_N are
 * AA_ERR_INVALID, a short workspace AA_ERR_WORKSPACE; n_jobs == 0 is AA_OK.
 * The jobs themselves are device memory the host cannot read: the kernels
 * skip a job (nothing read or written) whose ranges leave [0, n_pcm) or whose
 * n exceeds max_n, so callers validate ranges where they plan the jobs
 * (aa_amd/sosfilt.py does).  Non-finite input behaves as in the sequential
 * filter: output before it is unaffected, all output from it on is
 * non-finite.  Allocates nothing; capturable. */
int aa_sosfilt_run(float* pcm, int64_t n_pcm, const aa_sos_job* jobs_dev, int32_t n_jobs, int64_t max_n,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Device PCM16 (interleaved, `channels` <= 8) -> mono f32, as load_recording
 * delivers it (src/identify_tracks.py:49-62: ffmpeg s16, librosa buf_to_float
 * x / 32768, channel mean): bit-identical to the host decode.  Lets a batch of
 * recordings cross PCIe as int16. */
int aa_pcm_s16_to_f32(const int16_t* in, int64_t n_frames, int32_t channels, float* out, void* stream);

/* Rational polyphase resampling by L / M (load_recording's librosa.resample
 * to 48 kHz, src/identify_tracks.py:49-62; libsoxr's HQ recipe restated, see
 * aa_amd/resample.py): y[m] = sum_t bank[r][t] x[k0 - t] with q = m M + half,
 * k0 = q / L, r = q % L; x is zero outside [0, n_in).  bank: device f32
 * [L][taps] (bank[r][t] = h[r + t L] of the filter on the L-times upsampled
 * grid, centre tap `half`). */
int aa_resample_poly(const float* x, int64_t n_in, const float* bank, int32_t L, int32_t M, int32_t taps,
                     int32_t half, float* y, int64_t n_out, void* stream);

/* One recording of an aa_resample_batch launch: n_in frames of source `kind`
 * starting at element src_off of that kind's buffer (AA_RS_S16: interleaved
 * int16, `channels` (1..8) per frame; AA_RS_F32: mono f32, channels ignored),
 * n_out output samples to y[dst_off ..). */
#define AA_RS_S16 0
#define AA_RS_F32 1
typedef struct aa_rs_segment {
    int64_t src_off, n_in, dst_off, n_out;
    int32_t kind, channels;
} aa_rs_segment;
/* aa_resample_poly over n_seg (0..AA_CI_MAX_REC) recordings that share one
 * filter, in one launch (the batched old-index path, aa_amd/ci_batch.py).
 * Output m of a segment is, bit for bit, what aa_resample_poly gives on the
 * segment's samples -- for an int16 segment on what aa_pcm_s16_to_f32 makes
 * of them; no f32 copy at the source rate is written.  segs_dev: DEVICE array;
 * max_n_out: the largest n_out in it (sizes the grid: outputs of a segment
 * past max_n_out are not written).  src_s16 [n_s16 elements] / src_f32
 * [n_f32] may be NULL when their size is 0.  A segment whose kind or channels
 * is invalid, or whose source range leaves its buffer or whose output range
 * leaves y[0, n_y), is skipped (nothing read or written): callers validate
 * where they plan the table (aa_amd/ci_batch.plan_segments does).  Output
 * ranges must not overlap.  Before any HIP call: a null segs_dev / bank / y,
 * a null source with a non-zero size, negative sizes, n_seg outside
 * 0..AA_CI_MAX_REC, max_n_out outside 0..n_y, L, M or taps < 1 (L, M > 65536),
 * half >= L taps, or a filter whose tile does not fit LDS are AA_ERR_INVALID
 * with the argument named in aa_last_error.  n_seg == 0, max_n_out == 0 and
 * segments with n_out == 0 are AA_OK.  Allocates nothing; capturable. */
int aa_resample_batch(const int16_t* src_s16, int64_t n_s16, const float* src_f32, int64_t n_f32,
                      const aa_rs_segment* segs_dev, int32_t n_seg, int64_t max_n_out, const float* bank, int32_t L,
                      int32_t M, int32_t taps, int32_t half, float* y, int64_t n_y, void* stream);

/* ---------------------------------------------------------------- signal detector */
/* signal_noise (src/identify_tracks.py:650-706): |STFT| (n_fft 4096) of the
 * recording, the 3x row/column-median mask, cv2 morphology, 8-connected
 * components and the size filter, all on the device. */
typedef struct aa_sn_config {
    int32_t sr;          /* sample rate of the PCM (48000 after load_recording) */
    int32_t n_fft;       /* 4096 (:652) */
    int32_t hop_length;  /* 281 (:420) */
    double signal_width; /* SIGNAL_WIDTH seconds (:21, :673) */
    double freq_range;   /* Hz; the first bin above it sets the kernel height (:675-681) */
} aa_sn_config;

/* One kept component: the cv2 stats row (x = frame, y = frequency bin) and
 * OpenCV's label-order key, which orders components that tie on `left` in the
 * reference's stable sort (:688). */
typedef struct aa_sn_component {
    int32_t left, top, width, height, area, order;
} aa_sn_component;

#define AA_SN_NONFINITE 1    /* status: non-finite PCM (librosa valid_audio would raise) */
#define AA_SN_RUN_OVERFLOW 2 /* status: run table bound exceeded (internal error) */

int aa_sn_create(const aa_sn_config* cfg, void** plan);
int aa_sn_destroy(void* plan);
/* {dilate height, dilate width, erode height, erode width, min width, min
 * height} as derived from cfg (:673-691); host only */
int aa_sn_geometry(const aa_sn_config* cfg, int32_t* out6);
/* STFT frames of n_samples: 1 + n_samples / hop_length */
int64_t aa_sn_n_frames(const void* plan, int64_t n_samples);
size_t aa_sn_workspace_bytes(const void* plan, int64_t max_samples);
/* pcm: device f32 [n_samples] (frames[: int(sr * length)], :420).
 * out: device aa_sn_component[max_out], unordered; n_out: device int32[2] =
 * {components kept (may exceed max_out), AA_SN_* status}.
 * mask_out (may be NULL): device uint64 [2049][ceil(F / 64)], the thresholded
 * mask before morphology; bit f % 64 of word f / 64 is frame f. */
int aa_sn_run(void* plan, const float* pcm, int64_t n_samples, void* workspace, size_t workspace_bytes,
              aa_sn_component* out, int32_t max_out, int32_t* n_out, uint64_t* mask_out, void* stream);
/* signal_noise of n_rec (1..64) recordings in one device PCM buffer in one
 * pass (the batched corpus path; the reference runs it once per file,
 * src/identify_tracks.py:420): recording k is pcm[offsets[k] ..
 * offsets[k] + lengths[k]) (offsets, lengths: HOST arrays).  Its components
 * go to out + k * out_stride (out_stride >= max_out), its {count, status} to
 * n_out + k * n_out_stride (>= 2).  The per-recording STFT / medians / mask
 * launches run back to back; the morphology and components run once for the
 * whole batch.  Workspace: aa_sn_batch_workspace_bytes(plan, longest, n_rec). */
size_t aa_sn_batch_workspace_bytes(const void* plan, int64_t max_samples, int32_t n_rec);
int aa_sn_run_batch(void* plan, const float* pcm, const int64_t* offsets, const int64_t* lengths, int32_t n_rec,
                    void* workspace, size_t workspace_bytes, aa_sn_component* out, int32_t max_out,
                    int64_t out_stride, int32_t* n_out, int32_t n_out_stride, void* stream);
/* np.abs(librosa.stft(pcm, n_fft=4096, hop_length=hop)) (:654) alone, in the
 * reference's precision (f64 transform, complex64 rounding, numpy's f32
 * magnitude): out = device f32 [F][ld] (F = aa_sn_n_frames, ld >= 2049), row f
 * = frame f's 2049 bins.  No workspace. */
int aa_sn_spectrogram(void* plan, const float* pcm, int64_t n_samples, float* out, int64_t ld, void* stream);
/* Launch stages of aa_sn_run / aa_sn_run_batch (0 sn_stft64, 1 sn_transpose,
 * 2 sn_select, 3 sn_morph, 4 the component launches, 5 sn_colmed) and their timing, the
 * aa_fe_stage_* contract; an item is one STFT frame of one recording. */
int aa_sn_n_stages(const void* plan);
int aa_sn_stage_info(const void* plan, int32_t stage, char* name, int32_t name_len, double* flops_per_item,
                     double* bytes_per_item);
int aa_sn_set_timing(void* plan, uint32_t stage_mask);
int aa_sn_stage_time(void* plan, int32_t stage, double* total_ms, int64_t* count);
/* Morphology, components and filter of a given mask (mask_out's layout). */
int aa_sn_components_from_mask(void* plan, const uint64_t* mask, int64_t n_frames, void* workspace,
                               size_t workspace_bytes, aa_sn_component* out, int32_t max_out,
                               int32_t* n_out, void* stream);

/* ---------------------------------------------------------------- old cacophony index */
/* The frame loop of the old cacophony index (src/cacophony_index.py:53-97) on
 * 16 kHz mono f32 samples: frames of AA_CI_N samples at hop AA_CI_HOP, frame f
 * of a recording covering x[AA_CI_HOP (f + 1) .. AA_CI_HOP (f + 1) + AA_CI_N)
 * (the first AA_CI_HOP samples are never read, every frame lies inside the
 * recording); per frame the float64 window times the f32 samples (one
 * rounding each), the unnormalised DCT-II y[k] = 2 sum s[n] cos(pi k (2n + 1)
 * / (2 AA_CI_N)) (scipy.fftpack.dct) in float64, and the energy sum y[k]^2 of
 * AA_CI_BANDS bands [edges[b], edges[b + 1]); per pair of neighbouring frames
 * the number of bands whose energy more than halved or more than doubled.
 * The percentile scoring of those points stays on the host
 * (aa_amd/cacophony_index.py). */
#define AA_CI_N 2048
#define AA_CI_HOP 1024
#define AA_CI_BANDS 10
#define AA_CI_MAX_REC 64         /* recordings per aa_ci_run */
#define AA_CI_MAX_SAMPLES 1073741824 /* samples per recording, 2^30 */

/* Frames of a recording of n samples: len(range(1024, n - 3072, 1024)), 0 for
 * n <= 4096.  Host only. */
int64_t aa_ci_n_frames(int64_t n_samples);
/* window: host float64 [AA_CI_N] (numpy.hanning(2048)); edges: host int32
 * [AA_CI_BANDS + 1] (numpy.logspace(log10(25), log10(2048), num=11,
 * dtype=int)), non-decreasing within [0, AA_CI_N] (AA_ERR_INVALID otherwise,
 * before any HIP call).  Both are the caller's data, so numpy's bits and its
 * integer truncation stay numpy's.  aa_ci_plan: the plan alone, on the host
 * (the aa_model_plan contract: the same checks, no device memory, no HIP
 * call); aa_ci_run on it returns AA_ERR_INVALID. */
int aa_ci_create(const double* window, const int32_t* edges, void** plan);
int aa_ci_plan(const double* window, const int32_t* edges, void** plan);
int aa_ci_destroy(void* plan);
/* Workspace of one aa_ci_run over recordings of these lengths (HOST array)
 * when bins_out is NULL: the band energies; 0 for no frames. */
size_t aa_ci_workspace_bytes(const int64_t* lengths, int32_t n_rec);
/* n_rec (0..AA_CI_MAX_REC) recordings in one device f32 buffer: recording k
 * is pcm16k[offsets[k] .. offsets[k] + lengths[k]) (offsets, lengths: HOST
 * arrays; any sample alignment).  With F_k = aa_ci_n_frames(lengths[k]):
 * bins_out (device f64, may be NULL): F_k rows of AA_CI_BANDS energies per
 * recording, the recordings' rows back to back; points_out (device int32):
 * max(F_k - 1, 0) values per recording, back to back -- no comparison crosses
 * a recording's boundary.  Two launches (ci_bands: one workgroup per frame of
 * the whole batch; ci_points); the band sums are reduced in a fixed order,
 * without atomics, so a run is bit-reproducible.
 * Before any launch: null plan / pcm16k / offsets / lengths / points_out,
 * negative offsets or lengths, lengths > AA_CI_MAX_SAMPLES and n_rec outside
 * 0..AA_CI_MAX_REC are AA_ERR_INVALID; with bins_out NULL, a null, unaligned
 * (8 bytes) or short workspace is AA_ERR_WORKSPACE.  n_rec == 0 and
 * recordings without a frame are AA_OK.  Allocates nothing; capturable. */
int aa_ci_run(void* plan, const float* pcm16k, const int64_t* offsets, const int64_t* lengths, int32_t n_rec,
              void* workspace, size_t workspace_bytes, double* bins_out, int32_t* points_out, void* stream);

/* ---------------------------------------------------------------- FLAC decode */
/* load_recording (src/identify_tracks.py:49-62) decodes through ffmpeg; these
 * decode a FLAC stream (RFC 9639; an ID3v2 tag in front is skipped) held in
 * HOST memory, on the calling thread.  Samples come out as the stream's own
 * integers (bits_per_sample), interleaved; the caller applies ffmpeg's s16
 * conversion.  Header CRC-8 and frame CRC-16 are verified (AA_ERR_INVALID on
 * damage, with the byte offset in aa_last_error). */
typedef struct aa_flac_stream_info {
    int32_t sample_rate;
    int32_t channels;        /* 1..8 */
    int32_t bits_per_sample; /* 4..32 */
    int64_t total_frames;    /* samples per channel; 0 = not stated */
} aa_flac_stream_info;

int aa_flac_info(const uint8_t* data, size_t len, aa_flac_stream_info* info);
/* out: host int32 [cap_frames][channels], or NULL to count only;
 * n_frames: frames (samples per channel) decoded.  AA_ERR_WORKSPACE when the
 * stream holds more than cap_frames. */
int aa_flac_decode(const uint8_t* data, size_t len, int32_t* out, int64_t cap_frames, int64_t* n_frames);

/* FLAC decode on the device (aa_amd/flac_gpu.py, the corpus path): the host
 * indexes a stream's frames, the compressed bytes cross PCIe, and one call
 * decodes every frame of every stream of a batch.  The decoder core
 * (csrc/aa_flac_core.h) is separate code from aa_flac_decode, held to it
 * sample for sample (tests/test_flac_core.py, tests/test_gpu_flac.py). */
typedef enum aa_flac_status {
    AA_FLAC_OK = 0,
    AA_FLAC_CRC = 1,        /* decode did not end 2 bytes before the frame's end, or CRC-16 mismatch */
    AA_FLAC_MALFORMED = 2,  /* a header or subframe the host decoder rejects too, or a bad table entry */
    AA_FLAC_FALLBACK = 3,   /* valid perhaps, but beyond this path's int32 arithmetic: decode on the host */
} aa_flac_status;

/* One frame of a stream.  40 bytes; host array out of aa_flac_index,
 * device-resident array for aa_flac_decode_device.  A batch concatenates the
 * streams' bytes and tables: the caller adds each stream's base to `offset`
 * and `out_at` and sets `stream`. */
typedef struct aa_flac_frame {
    int64_t offset;    /* byte offset of the frame's sync code */
    int64_t out_at;    /* first output frame, as an element index: frame index * channels */
    int32_t nbytes;    /* bytes to the next frame start (or the stream's end), CRC-16 included */
    int32_t block;     /* samples per channel coded in the frame */
    int32_t keep;      /* samples per channel written: block, less in a last block cut by the total */
    int32_t channels;  /* 1..8 */
    int32_t bits;      /* 4..32 */
    int32_t stream;    /* index of the frame's stream in the batch */
} aa_flac_frame;

/* Index the frames of a FLAC stream in HOST memory (no HIP call): metadata as
 * aa_flac_info (and its errors), then every frame start: sync code, reserved
 * header fields, header CRC-8, the coded number the expected one (frame k for
 * fixed, the running sample number for variable block size), and the CRC-16
 * of the bytes since the previous start, so a sync pattern inside a frame's
 * payload is not taken for a start.  An ID3v1 tag ("TAG", 128 bytes) at the
 * end is not part of the last frame.  frames NULL: size query (*n_frames);
 * cap < *n_frames: AA_ERR_WORKSPACE, *n_frames set.  AA_ERR_UNSUPPORTED
 * (reason in aa_last_error) whenever the table would be less than certain --
 * a first frame not numbered 0, a header at odds with STREAMINFO, bytes
 * between frames that are no frame, fewer samples than STREAMINFO states, a
 * frame above 16 MiB: aa_flac_decode then gives today's samples or error. */
int aa_flac_index(const uint8_t* data, size_t len, aa_flac_stream_info* info, aa_flac_frame* frames, int64_t cap,
                  int64_t* n_frames);
/* AA_FLAC_WG frames share a workgroup (and its workspace slice). */
#define AA_FLAC_WG 64
/* Workspace of one aa_flac_decode_device / _host over these (host) frames. */
size_t aa_flac_device_workspace_bytes(const aa_flac_frame* frames_host, int64_t n_frames);
/* Decode n_frames frames of bytes[0, n_bytes): frame f writes its `keep`
 * interleaved samples at out_i32 + out_at (the stream's own integers, as
 * aa_flac_decode) and / or out_s16 + out_at (ffmpeg's s16: x << (16 - bits)
 * or x >> (bits - 16)); either may be NULL.  status[f] is an aa_flac_status;
 * samples of a frame whose status is not AA_FLAC_OK are undefined (inside its
 * own range).  Every load is inside bytes, every store inside the frame's
 * output range and workspace slice.  Allocates nothing; n_frames == 0 is
 * AA_OK; a short workspace AA_ERR_WORKSPACE. */
int aa_flac_decode_device(const uint8_t* bytes_dev, int64_t n_bytes, const aa_flac_frame* frames_dev,
                          int64_t n_frames, int32_t* out_i32, int16_t* out_s16, int32_t* status_dev, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The same through the same core as a host loop, every pointer HOST memory
 * (the core's CPU tests; stream is ignored). */
int aa_flac_decode_frames_host(const uint8_t* bytes, int64_t n_bytes, const aa_flac_frame* frames, int64_t n_frames,
                               int32_t* out_i32, int16_t* out_s16, int32_t* status, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------- Ogg Vorbis decode */
/* load_recording (src/identify_tracks.py:49-62) decodes through ffmpeg; these
 * decode an Ogg Vorbis stream (RFC 3533 pages, Vorbis I codec: floor 0/1,
 * residue 0/1/2, channel coupling, short/long blocks) held in HOST memory, on
 * the calling thread.  Pages failing their CRC-32 are skipped; the first
 * Vorbis logical stream is decoded.  Samples come out as float32 in [-1, 1]
 * scale, interleaved, trimmed by the granule positions (Vorbis I A.2); the
 * caller applies ffmpeg's float -> s16 conversion.  A damaged header is
 * AA_ERR_INVALID with the reason in aa_last_error. */
typedef struct aa_vorbis_stream_info {
    int32_t sample_rate;
    int32_t channels;        /* 1..255 */
    int32_t blocksize_0;     /* short block, 64..8192 */
    int32_t blocksize_1;     /* long block */
    int64_t total_frames;    /* the last page's granule position (0 = none found) */
} aa_vorbis_stream_info;

int aa_vorbis_info(const uint8_t* data, size_t len, aa_vorbis_stream_info* info);
/* out: host float32 [cap_frames][channels], or NULL to count only;
 * n_frames: frames (samples per channel) decoded.  AA_ERR_WORKSPACE when the
 * stream holds more than cap_frames. */
int aa_vorbis_decode(const uint8_t* data, size_t len, float* out, int64_t cap_frames, int64_t* n_frames);

/* Ogg Vorbis decode on the device (aa_amd/vorbis_gpu.py, the corpus path).
 * A Vorbis audio packet decodes from its own bits and the setup header alone;
 * only the overlap-add joins neighbours, and where each block lands in time
 * follows from the mode bits at the head of each packet.  So the host walks
 * the pages (CRC-32 verified, as aa_vorbis_decode), reassembles the packets,
 * lays out the block timeline and flattens the setup header (aa_vorbis_index,
 * no HIP call); the payload bytes cross PCIe, and one call decodes every
 * packet of every stream of a batch in three launches: unpack (one lane per
 * packet: floors, residues, coupling, to spectra), inverse MDCT and window
 * (one workgroup per packet and channel, float64), overlap-add and the
 * float -> s16 conversion (one thread per output sample).  The decoder core
 * (csrc/aa_vorbis_core.h) is separate code from aa_vorbis_decode, held to it
 * bit for bit (tests/test_vorbis_core.py, tests/test_gpu_vorbis.py). */
typedef enum aa_vorbis_status {
    AA_VORBIS_OK = 0,
    AA_VORBIS_FALLBACK = 1, /* a workspace slice too small, a table entry at odds with the packet's own
                               bits, or a setup index out of range: decode the file on the host */
} aa_vorbis_status;

/* One audio packet that produces a block.  56 bytes; host array out of
 * aa_vorbis_index, device-resident array for aa_vorbis_decode_device.  A batch
 * concatenates the streams' payloads and tables: the caller adds each
 * stream's bases to `offset` and `blk_at` and sets `stream`. */
typedef struct aa_vorbis_packet {
    int64_t offset;     /* byte offset of the packet in the payload buffer */
    int64_t pos;        /* timeline index of the block's first sample (the first block of a stream starts at
                           blocksize_1; block k + 1 starts 3 n_k / 4 - n_k+1 / 4 after block k) */
    int64_t blk_at;     /* float index of the windowed block in the workspace: channel c at blk_at + c * n */
    int32_t nbytes;     /* packet size */
    int32_t n;          /* block size: blocksize_0 or blocksize_1 */
    int32_t blockflag;  /* 1: a long block */
    int32_t prev, next; /* long block: the window flags read after the mode number; short block: 1, 1 */
    int32_t lstart;     /* the window's nonzero span [lstart, rend) inside the block: only it is added */
    int32_t rend;
    int32_t stream;     /* index of the packet's stream in the batch */
} aa_vorbis_packet;

/* A stream of the batch.  72 bytes.  aa_vorbis_index fills it for the stream
 * alone (setup_at, out_at, first_packet 0); the caller of a batch sets those. */
typedef struct aa_vorbis_stream {
    int64_t setup_at;      /* byte offset (a multiple of 8) of the stream's flattened setup in the setup buffer;
                              streams with byte-identical setups share one */
    int64_t out_at;        /* first output frame, as an element index into out_s16 / out_f32 */
    int64_t frames;        /* output frames: exactly aa_vorbis_decode's count (produced - start trim, capped by
                              the last page's granule), not aa_vorbis_info's estimate */
    int64_t s0;            /* timeline index of the first output frame */
    int64_t first_packet;  /* the stream's packets: [first_packet, first_packet + n_packets) of the table */
    int64_t n_packets;
    int32_t channels;      /* 1..8 */
    int32_t sample_rate;
    int32_t blocksize_0;
    int32_t blocksize_1;
    int32_t ws_need[2];    /* floats of unpack workspace a short / a long packet needs */
} aa_vorbis_stream;

/* Index an Ogg Vorbis stream in HOST memory: headers as aa_vorbis_info (the
 * same parse, so the same streams are accepted and refused, with the same
 * codes), then
 *   payload: the audio packets that produce a block, reassembled from the
 *            lacing values, back to back (*payload_bytes);
 *   packets: one record each (stream->n_packets).  A packet Decoder::audio
 *            skips -- empty, its first bit set, its mode number out of range --
 *            gets no record and leaves the timeline alone;
 *   setup:   the flattened setup (*setup_bytes, a multiple of 8; layout in
 *            csrc/aa_vorbis_core.h): codebook trees and expanded VQ tables,
 *            floor 1, residue, mapping and mode records, the inverse-dB table,
 *            per block size the inverse MDCT's twiddle and bit-reversal tables
 *            as doubles, and the window tables -- all computed here, so the
 *            device uses the host decoder's own table values.
 * Any buffer NULL or shorter than needed: AA_ERR_WORKSPACE with the three
 * sizes set (a size query).  AA_ERR_UNSUPPORTED (reason in aa_last_error) for
 * what the device path declines: a floor of type 0 in the setup (its curve
 * needs atan / cos / exp / sqrt in double), more than 8 channels, a workspace
 * need beyond int32; aa_vorbis_decode then decodes the file. */
int aa_vorbis_index(const uint8_t* data, size_t len, aa_vorbis_stream* stream, uint8_t* payload, int64_t payload_cap,
                    int64_t* payload_bytes, aa_vorbis_packet* packets, int64_t packet_cap, void* setup,
                    int64_t setup_cap, int64_t* setup_bytes);
/* AA_VORBIS_WG packets share a workgroup of the unpack launch (and its workspace slice). */
#define AA_VORBIS_WG 64
/* How one decode call divides its workspace; filled by aa_vorbis_device_workspace_bytes. */
typedef struct aa_vorbis_plan {
    int64_t stride;        /* floats of unpack workspace per packet: the largest ws_need of the table */
    int64_t blk_floats;    /* floats of windowed blocks: the largest blk_at + n * channels */
    int64_t max_out;       /* the most output elements (frames * channels) of one stream */
    int32_t max_channels;
    int32_t reserved;
} aa_vorbis_plan;
/* Workspace of one aa_vorbis_decode_device / _packets_host over these (host)
 * tables: the unpack slices, a used-floor flag per packet and channel, the
 * windowed blocks.  0 with plan zeroed for an empty or inconsistent table. */
size_t aa_vorbis_device_workspace_bytes(const aa_vorbis_packet* packets_host, int64_t n_packets,
                                        const aa_vorbis_stream* streams_host, int64_t n_streams,
                                        aa_vorbis_plan* plan);
/* Decode n_packets packets of bytes[0, n_bytes) belonging to n_streams
 * streams: stream k writes its `frames` interleaved frames at out_s16 + out_at
 * (ffmpeg's s16: clip(lrint(x * 32768)), NaN -> -32768) and / or out_f32 +
 * out_at (the decoder's float samples, aa_vorbis_decode's bit for bit); either
 * may be NULL; out_elems bounds both.  status[p] is an aa_vorbis_status; the
 * samples of a stream with any packet not AA_VORBIS_OK are undefined (inside
 * its own range).  Every load is inside bytes / the tables / the setups,
 * every store inside the stream's output range and the workspace.  plan is
 * HOST memory.  Allocates nothing; n_packets == 0 or n_streams == 0 is AA_OK
 * (a stream without packets has no frames); a short workspace
 * AA_ERR_WORKSPACE. */
int aa_vorbis_decode_device(const uint8_t* bytes_dev, int64_t n_bytes, const aa_vorbis_packet* packets_dev,
                            int64_t n_packets, const aa_vorbis_stream* streams_dev, int64_t n_streams,
                            const void* setups_dev, int64_t setups_bytes, const aa_vorbis_plan* plan,
                            int16_t* out_s16, float* out_f32, int64_t out_elems, int32_t* status_dev,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same through the same core as host loops, every pointer HOST memory
 * (the core's CPU tests; stream is ignored). */
int aa_vorbis_decode_packets_host(const uint8_t* bytes, int64_t n_bytes, const aa_vorbis_packet* packets,
                                  int64_t n_packets, const aa_vorbis_stream* streams, int64_t n_streams,
                                  const void* setups, int64_t setups_bytes, const aa_vorbis_plan* plan,
                                  int16_t* out_s16, float* out_f32, int64_t out_elems, int32_t* status,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ MP3 decode */
/* load_recording (src/identify_tracks.py:49-62) decodes through ffmpeg; these
 * decode an MPEG-1 Layer III stream (32 / 44.1 / 48 kHz; mono, stereo, dual
 * channel, joint stereo with MS; long, start, short, stop and mixed blocks;
 * CBR or VBR, padding, the bit reservoir, the CRC word skipped) held in HOST
 * memory.  An ID3v2 tag in front is skipped; behind the audio the walk resyncs
 * forward to a header agreeing with the first in version, layer and rate, else
 * the stream ends.  A Xing / Info / VBRI frame is not audio; a LAME-style tag
 * in it trims the output as ffmpeg's demuxer does (delay + 529 frames off the
 * start, everything from n_frames * 1152 - padding + 529 on off the end).
 * One decoder core (csrc/aa_mp3_core.h), float64 throughout, rounded once to
 * float32: the host decoder is that core as host loops, the device decoder
 * the same code in three kernels, equal bit for bit.  Declined with
 * AA_ERR_UNSUPPORTED: MPEG-2 / 2.5, Layers I and II, free format, a stream
 * with any intensity-stereo frame. */
typedef struct aa_mp3_stream_info {
    int32_t sample_rate;
    int32_t channels;       /* 1 or 2 */
    int64_t total_frames;   /* output frames (samples per channel) after the trim */
    int32_t n_frames;       /* audio frames (1152 samples each) */
    int32_t delay, padding; /* of the LAME-style tag; -1, -1 without one */
    int32_t reserved;
} aa_mp3_stream_info;

typedef enum aa_mp3_status {
    AA_MP3_OK = 0,
    AA_MP3_NODATA = 1,    /* the frame's main_data_begin reaches before the stream's data: silence */
    AA_MP3_MALFORMED = 2, /* the granule's side info cannot be honoured (big values beyond part2_3_length or
                             576, scalefactors beyond part2_3_length, bits past the reservoir, a table or
                             block type that does not exist): silence */
} aa_mp3_status;

/* One audio frame.  336 bytes.  The main data of a stream's frames lie back to
 * back in the payload (the bit reservoir laid out flat); a batch concatenates
 * payloads and tables: the caller adds each stream's byte base to main_at,
 * main_lo and main_end, and sets `stream`. */
typedef struct aa_mp3_frame {
    int64_t main_at;  /* payload byte where the frame's granules begin: its own data's start - main_data_begin */
    int64_t main_lo;  /* first payload byte of the frame's stream */
    int64_t main_end; /* one past the frame's own main data */
    int32_t stream;   /* index of the frame's stream in the batch */
    int32_t number;   /* index of the frame in its stream */
    int32_t ms;       /* joint stereo with MS on */
    int32_t nodata;   /* main_at < main_lo */
    int32_t scfsi[2]; /* per channel, band group 0 in bit 3 */
    /* the side info of granule gr of channel ch at [gr * 2 + ch] (table_select
     * and subblock_gain: three values each from [(gr * 2 + ch) * 3]);
     * block_type is 0 without window switching, and region0_count /
     * region1_count hold the standard's implied values with it */
    int32_t part2_3_length[4];
    int32_t big_values[4];
    int32_t global_gain[4];
    int32_t scalefac_compress[4];
    int32_t window_switching[4];
    int32_t block_type[4];
    int32_t mixed[4];
    int32_t table_select[12];
    int32_t subblock_gain[12];
    int32_t region0_count[4];
    int32_t region1_count[4];
    int32_t preflag[4];
    int32_t scalefac_scale[4];
    int32_t count1table_select[4];
} aa_mp3_frame;

/* A stream of the batch.  56 bytes.  aa_mp3_index fills it for the stream
 * alone (out_at, first_frame 0). */
typedef struct aa_mp3_stream {
    int64_t out_at;      /* first output frame, as an element index into out_s16 / out_f32 */
    int64_t frames;      /* output frames after the trim */
    int64_t skip;        /* decoded frames dropped in front */
    int64_t first_frame; /* the stream's frames: [first_frame, first_frame + n_frames) of the table */
    int64_t n_frames;
    int32_t channels;
    int32_t sample_rate;
    int32_t sr_index;    /* 0: 44.1 kHz, 1: 48 kHz, 2: 32 kHz */
    int32_t reserved;
} aa_mp3_stream;

int aa_mp3_info(const uint8_t* data, size_t len, aa_mp3_stream_info* info);
/* out: host float32 [cap_frames][channels], or NULL to count only; n_frames:
 * frames decoded.  AA_ERR_WORKSPACE when the stream holds more than
 * cap_frames.  aa_mp3_index plus aa_mp3_decode_frames_host. */
int aa_mp3_decode(const uint8_t* data, size_t len, float* out, int64_t cap_frames, int64_t* n_frames);
/* Index a stream in HOST memory: payload takes the frames' main-data bytes
 * back to back (*payload_bytes; it may be the buffer holding data: every byte
 * is read before it is overwritten), frames one record per audio frame
 * (stream->n_frames).  Either buffer NULL or short: AA_ERR_WORKSPACE with
 * both sizes set (a size query).  A stream with no decodable frame is
 * AA_ERR_INVALID; what aa_mp3_info declines is declined here. */
int aa_mp3_index(const uint8_t* data, size_t len, aa_mp3_stream* stream, uint8_t* payload, int64_t payload_cap,
                 int64_t* payload_bytes, aa_mp3_frame* frames, int64_t frame_cap);
/* The decoder's table blob (csrc/aa_mp3_core.h Tables: |is|^(4/3), 2^(k/4),
 * the IMDCT, matrixing and window values, the Huffman trees and band edges),
 * built once on the host; aa_mp3_decode_device reads a device copy of exactly
 * these bytes.  out NULL or cap short: AA_ERR_WORKSPACE with *bytes set. */
int aa_mp3_tables(void* out, int64_t cap, int64_t* bytes);
/* One restated table of the standard, read-only, as int32 values (the single
 * copy: csrc/aa_mp3_tables.h).  kind / index:
 *   0 Huffman code words, 1 their lengths: index = table number 1..31
 *     (dim * dim values, pair (x, y) at x * dim + y), 32 / 33 = count1 table
 *     A / B (16 values, v w x y as bits 3..0);
 *   2 linbits (index 0: all 32);  3 slen1 (index 0) / slen2 (index 1);
 *   4 pretab;  5 long and 6 short band edges (index: 0 44.1, 1 48, 2 32 kHz);
 *   7 the synthesis window D * 65536 (512 values).
 * *n: the values the table holds; AA_ERR_WORKSPACE when cap is short,
 * AA_ERR_INVALID for a table that does not exist (0, 4, 14). */
int aa_mp3_table(int32_t kind, int32_t index, int32_t* out, int64_t cap, int64_t* n);
/* The core's polyphase synthesis alone, on the host: sb [n_slots][32] float64
 * subband samples -> out [n_slots * 32] float64 (before the float32 rounding),
 * slots before the first taken as zero.  (tests/test_mp3_tables.py) */
int aa_mp3_synth_host(const double* sb, int64_t n_slots, double* out);
/* AA_MP3_WG lanes (frame, channel) share a workgroup of the unpack launch. */
#define AA_MP3_WG 64
/* Workspace of one aa_mp3_decode_device / _frames_host over n_frames frames:
 * the unpack slices (2.5 KB per frame and channel) and the float64 subband
 * samples (4608 bytes per granule and channel, two channels held for every
 * frame).  0 for n_frames <= 0. */
size_t aa_mp3_device_workspace_bytes(int64_t n_frames);
/* Decode n_frames frames of bytes[0, n_bytes) belonging to n_streams streams:
 * stream k writes its `frames` interleaved frames at out_s16 + out_at
 * (ffmpeg's s16: clip(lrint(x * 32768))) and / or out_f32 + out_at; either may
 * be NULL; out_elems bounds both.  status[f * 4 + gr * 2 + ch] is an
 * aa_mp3_status; a granule not AA_MP3_OK decodes as a zero spectrum, so the
 * samples are defined for every status (the host decoder's, bit for bit).
 * tables_dev: a device copy of aa_mp3_tables' bytes.  Three launches (unpack,
 * hybrid, synth); allocates nothing; n_frames == 0 or n_streams == 0 is
 * AA_OK; a short workspace AA_ERR_WORKSPACE. */
int aa_mp3_decode_device(const void* tables_dev, const uint8_t* bytes_dev, int64_t n_bytes,
                         const aa_mp3_frame* frames_dev, int64_t n_frames, const aa_mp3_stream* streams_dev,
                         int64_t n_streams, int16_t* out_s16, float* out_f32, int64_t out_elems, int32_t* status_dev, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same phases as host loops, every pointer HOST memory: the host decoder. */
int aa_mp3_decode_frames_host(const uint8_t* bytes, int64_t n_bytes, const aa_mp3_frame* frames, int64_t n_frames,
                              const aa_mp3_stream* streams, int64_t n_streams, int16_t* out_s16, float* out_f32,
                              int64_t out_elems, int32_t* status, void* workspace, size_t workspace_bytes);

/* ---- file input of the batched corpus path (aa_amd/batch.py) ----
 * The whole file at path into buf (cap bytes; a pinned staging slot), in one
 * call: open, size, read, close -- the reference reads each file through
 * ffmpeg (src/identify_tracks.py:49-62); the corpus decoder threads read
 * PCM16 WAVs raw and parse the RIFF header themselves.  *size: the file's
 * size.  AA_ERR_WORKSPACE (nothing read) when it exceeds cap;
 * AA_ERR_INVALID when it cannot be opened or read (the reason in
 * aa_last_error). */
int aa_read_file(const char* path, void* buf, int64_t cap, int64_t* size);

/* ---- track builder (host) ----
 * get_tracks_from_signals (src/identify_tracks.py:795-842, with
 * merge_signals :725-792): the signals' merge sweeps until stable, then the
 * enlarge / absorb pass and the narrow-track drop, in Python's double
 * arithmetic.  sig: n rows of (start, end, freq_start, freq_end,
 * mel_freq_start, mel_freq_end); kind: per row, which of the first four are
 * Python ints (bits 0-3: start, end, freq_start, freq_end).  end: the
 * recording's length (end_is_int: a Python int).  mel_int[f]: the mel of
 * integer frequency f (numpy's 2595 log10(1 + f / 700)), n_mel entries.
 * Out: *n_tracks rows (<= n) of the same layout into track / track_kind.
 * AA_ERR_INVALID where the Python divides by a zero mel range (it raises
 * there); AA_ERR_UNSUPPORTED when an enlarged frequency is outside mel_int or
 * an input is NaN (the caller's Python builder takes those). */
int aa_tracks_from_signals(const double* sig, const int32_t* kind, int64_t n, double end, int32_t end_is_int,
                           const double* mel_int, int64_t n_mel, double* track, int32_t* track_kind,
                           int64_t* n_tracks);

#ifdef __cplusplus
}
#endif
#endif /* AA_H */
