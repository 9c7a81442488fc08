// MPEG-1 Layer III decode on the device (C ABI aa_mp3_decode_device,
// include/aa.h): load_recording's decode (src/identify_tracks.py:49-62) for
// the corpus path, where the host decoder bounds an MP3 corpus by its CPUs.
// The host indexes a stream (aa_mp3_index: headers, side info, the bit
// reservoir laid out flat); three launches decode every frame of every stream
// of a batch through csrc/aa_mp3_core.h, the code the host decoder runs:
//
//   mp3_unpack  one lane per (frame, channel), AA_MP3_WG lanes per workgroup
//               (one wave): scalefactors and the Huffman decode of both
//               granules are serial within a lane and divergent across lanes;
//               the parallelism is the tens of thousands of frames of a
//               batch.  A lane's slice (is[576], scalefactors, nonzero bound
//               per granule) interleaves with its workgroup's element by
//               element (lane l's element i at [i * WG + l]), so the wave's
//               accesses at one index share cache lines.
//   mp3_hybrid  one workgroup per granule, both channels together (MS):
//               requantise, stereo, reorder, alias reduction and IMDCT of
//               granule g and, for the overlap, of g - 1, in float64 in LDS
//               (3 x 2 x 576 doubles: 27 KiB) -> subband samples [18][32].
//   mp3_synth   one workgroup per (granule, channel): the matrixed vectors of
//               the granule's 18 slots and the 15 before it in LDS (33 x 64
//               doubles: 16.5 KiB), then the window sums, float32, s16.
//
// This file builds with -ffp-contract=off (aa_amd/_build.py): the outputs are
// held to the host decoder's bits, and a fused multiply-add rounds once where
// the host rounds twice.
#include "aa_common.h"
#include "aa_mp3_core.h"

namespace {

using namespace aa_mp3;

constexpr int HYBRID_THREADS = 256;
constexpr int SYNTH_THREADS = 256;

static_assert(sizeof(Frame) == sizeof(aa_mp3_frame) && sizeof(Stream) == sizeof(aa_mp3_stream),
              "the core's views of the C ABI records");
static_assert(offsetof(Frame, table_select) == offsetof(aa_mp3_frame, table_select) &&
                  offsetof(Stream, sr_index) == offsetof(aa_mp3_stream, sr_index),
              "the core's views of the C ABI records");

struct BlockSync {
    __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(WG) void mp3_unpack(Batch b) {
    const long long lane = (long long)blockIdx.x * WG + threadIdx.x;
    if (lane >= 2 * b.n_frames) return;
    unpack_one(b, lane);
}

__global__ __launch_bounds__(HYBRID_THREADS) void mp3_hybrid(Batch b) {
    __shared__ double xr[2 * 576];
    __shared__ double tmp[2 * 576];
    __shared__ double tail[2 * 576];
    // (every thread of a workgroup takes the same early exits: they depend on the granule alone)
    hybrid_one(b, (long long)blockIdx.x, xr, tmp, tail, (int)threadIdx.x, HYBRID_THREADS, BlockSync{});
}

__global__ __launch_bounds__(SYNTH_THREADS) void mp3_synth(Batch b, int16_t* out_s16, float* out_f32,
                                                           long long out_elems) {
    __shared__ double M[33 * 64];
    synth_one(b, (long long)blockIdx.x, (int)blockIdx.y, M, out_s16, out_f32, out_elems, (int)threadIdx.x,
              SYNTH_THREADS, BlockSync{});
}

}  // namespace

extern "C" int aa_mp3_decode_device(const void* tables_dev, const uint8_t* bytes_dev, int64_t n_bytes,
                                    const aa_mp3_frame* frames_dev, int64_t n_frames, const aa_mp3_stream* streams_dev,
                                    int64_t n_streams, int16_t* out_s16, float* out_f32, int64_t out_elems,
                                    int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "aa_mp3_decode_device";
    AA_CHECK(n_frames >= 0 && n_bytes >= 0 && n_streams >= 0 && out_elems >= 0, AA_ERR_INVALID, "%s: bad sizes", who);
    if (n_frames == 0 || n_streams == 0) return AA_OK;
    AA_CHECK(tables_dev && bytes_dev && frames_dev && streams_dev && status_dev, AA_ERR_INVALID, "%s: null argument",
             who);
    AA_CHECK(out_s16 || out_f32, AA_ERR_INVALID, "%s: no output", who);
    AA_CHECK(n_frames <= 0x3FFFFFFF && n_streams <= 65535, AA_ERR_INVALID, "%s: too many frames or streams", who);
    Plan pl{};
    const size_t need = plan_bytes(n_frames, &pl);
    AA_CHECK(workspace && (uintptr_t)workspace % 8 == 0 && workspace_bytes >= need, AA_ERR_WORKSPACE,
             "%s: workspace null, unaligned or below %zu bytes", who, need);
    char* ws = static_cast<char*>(workspace);
    const Batch b{static_cast<const Tables*>(tables_dev),
                  bytes_dev,
                  (long long)n_bytes,
                  reinterpret_cast<const Frame*>(frames_dev),
                  (long long)n_frames,
                  reinterpret_cast<const Stream*>(streams_dev),
                  (long long)n_streams,
                  reinterpret_cast<int16_t*>(ws + pl.slices_at),
                  reinterpret_cast<double*>(ws + pl.sb_at),
                  status_dev};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned groups = (unsigned)((2 * n_frames + WG - 1) / WG);
    hipLaunchKernelGGL(mp3_unpack, dim3(groups), dim3(WG), 0, st, b);
    AA_LAUNCH_CHECK();
    hipLaunchKernelGGL(mp3_hybrid, dim3((unsigned)(2 * n_frames)), dim3(HYBRID_THREADS), 0, st, b);
    AA_LAUNCH_CHECK();
    hipLaunchKernelGGL(mp3_synth, dim3((unsigned)(2 * n_frames), 2), dim3(SYNTH_THREADS), 0, st, b, out_s16, out_f32,
                       (long long)out_elems);
    AA_LAUNCH_CHECK();
    return AA_OK;
}
