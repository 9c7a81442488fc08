// FLAC decode on the device (C ABI aa_flac_index / aa_flac_decode_device /
// aa_flac_decode_frames_host, include/aa.h): load_recording's decode
// (src/identify_tracks.py:49-62) for the corpus path, where the host's serial
// Rice / LPC recurrences (csrc/aa_flac.cpp) bound a FLAC corpus by its CPUs.
// FLAC frames are independent, so the host only finds them (aa_flac_index.h)
// and one launch decodes every frame of every stream of a batch.
//
// Mapping: one lane per frame, AA_FLAC_WG frames per workgroup (one wave).
// A lane runs the whole core (aa_flac_core.h) for its frame: header, Rice
// residuals into its int32 workspace slice, predictor restore in place,
// CRC-16, then stereo decorrelation and the interleaved stores.  Lanes of a
// workgroup interleave their workspace slices element by element (lane l's
// element i at [i * AA_FLAC_WG + l]), so the wave's stores at one sample
// index share cache lines; the LPC coefficients (32 per lane, indexed by a
// runtime order) sit in LDS, bank-interleaved the same way, and so does the
// CRC-16 table.  Nothing crosses lanes or workgroups but the LDS table.
#include <algorithm>

#include "aa_common.h"
#include "aa_flac_index.h"

namespace {

using namespace aa_flac;

constexpr int WG = AA_FLAC_WG;

AA_FLAC_HD Frame core_frame(const aa_flac_frame& f) {
    return Frame{f.offset, f.out_at, f.nbytes, f.block, f.keep, f.channels, f.bits};
}

// stride: int32 elements of workspace per frame
__global__ __launch_bounds__(WG) void flac_decode_frames(const uint8_t* __restrict__ bytes, long long n_bytes,
                                                         const aa_flac_frame* __restrict__ frames,
                                                         long long n_frames, int32_t* out_i32, int16_t* out_s16,
                                                         int32_t* __restrict__ status, int32_t* ws,
                                                         long long stride) {
    __shared__ uint16_t crc_tab[256];
    __shared__ int32_t coef[32 * WG];
    crc16_table(crc_tab, (int)threadIdx.x, WG);
    __syncthreads();
    const long long f = (long long)blockIdx.x * WG + threadIdx.x;
    if (f >= n_frames) return;
    const Buf buf{bytes, (uint64_t)n_bytes};
    const Ws w{ws + (long long)blockIdx.x * WG * stride + threadIdx.x, WG};
    const Ws c{coef + threadIdx.x, WG};
    status[f] = decode_frame(buf, core_frame(frames[f]), w, stride, c, crc_tab, out_i32, out_s16);
}

int check_args(const char* who, const void* bytes, int64_t n_bytes, const void* frames, int64_t n_frames,
               const void* out_i32, const void* out_s16, const void* status, const void* workspace) {
    AA_CHECK(n_frames >= 0 && n_bytes >= 0, AA_ERR_INVALID, "%s: bad sizes", who);
    if (n_frames == 0) return AA_OK;
    AA_CHECK(bytes && frames && status, AA_ERR_INVALID, "%s: null argument", who);
    AA_CHECK(out_i32 || out_s16, AA_ERR_INVALID, "%s: no output", who);
    AA_CHECK(workspace && (uintptr_t)workspace % 4 == 0, AA_ERR_WORKSPACE, "%s: null or unaligned workspace", who);
    return AA_OK;
}

}  // namespace

extern "C" int aa_flac_index(const uint8_t* data, size_t len, aa_flac_stream_info* info, aa_flac_frame* frames,
                             int64_t cap, int64_t* n_frames) {
    AA_CHECK(data && info && n_frames && cap >= 0, AA_ERR_INVALID, "aa_flac_index: bad argument");
    const char* why = "";
    const int rc = index_stream(data, len, info, frames, cap, n_frames, &why);
    if (rc) aa::set_error("%s", why);
    return rc;
}

// Every workgroup's slice holds AA_FLAC_WG frames of the largest block *
// channels: the per-frame stride is derived from the workspace size again,
// and a frame that does not fit its slice reports AA_FLAC_FALLBACK.
extern "C" size_t aa_flac_device_workspace_bytes(const aa_flac_frame* frames_host, int64_t n_frames) {
    if (!frames_host || n_frames <= 0) return 0;
    int64_t most = 0;
    for (int64_t i = 0; i < n_frames; ++i) {
        const aa_flac_frame& f = frames_host[i];
        if (f.block > 0 && f.block <= 65536 && f.channels > 0 && f.channels <= 8)
            most = std::max<int64_t>(most, (int64_t)f.block * f.channels);
    }
    const int64_t groups = (n_frames + WG - 1) / WG;
    return (size_t)(groups * WG * most) * sizeof(int32_t);
}

extern "C" int aa_flac_decode_device(const uint8_t* bytes_dev, int64_t n_bytes, const aa_flac_frame* frames_dev,
                                     int64_t n_frames, int32_t* out_i32, int16_t* out_s16, int32_t* status_dev,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_args("aa_flac_decode_device", bytes_dev, n_bytes, frames_dev, n_frames, out_i32, out_s16,
                              status_dev, workspace);
    if (rc || n_frames == 0) return rc;
    const int64_t groups = (n_frames + WG - 1) / WG;
    AA_CHECK(groups <= 0x7FFFFFFF, AA_ERR_INVALID, "aa_flac_decode_device: too many frames");
    const int64_t stride = (int64_t)(workspace_bytes / sizeof(int32_t)) / (groups * WG);
    AA_CHECK(stride >= 1, AA_ERR_WORKSPACE, "aa_flac_decode_device: workspace below one sample per frame");
    hipLaunchKernelGGL(flac_decode_frames, dim3((unsigned)groups), dim3(WG), 0, static_cast<hipStream_t>(stream),
                       bytes_dev, (long long)n_bytes, frames_dev, (long long)n_frames, out_i32, out_s16, status_dev,
                       static_cast<int32_t*>(workspace), (long long)stride);
    AA_LAUNCH_CHECK();
    return AA_OK;
}

extern "C" int aa_flac_decode_frames_host(const uint8_t* bytes, int64_t n_bytes, const aa_flac_frame* frames,
                                          int64_t n_frames, int32_t* out_i32, int16_t* out_s16, int32_t* status,
                                          void* workspace, size_t workspace_bytes, void*) {
    const int rc = check_args("aa_flac_decode_frames_host", bytes, n_bytes, frames, n_frames, out_i32, out_s16,
                              status, workspace);
    if (rc || n_frames == 0) return rc;
    // the device's layout: WG frames interleaved per slice
    const int64_t groups = (n_frames + WG - 1) / WG;
    const int64_t stride = (int64_t)(workspace_bytes / sizeof(int32_t)) / (groups * WG);
    AA_CHECK(stride >= 1, AA_ERR_WORKSPACE, "aa_flac_decode_frames_host: workspace below one sample per frame");
    static uint16_t crc_tab[256];
    static const bool once = (crc16_table(crc_tab, 0, 1), true);
    (void)once;
    int32_t coef[32];
    const Buf buf{bytes, (uint64_t)n_bytes};
    int32_t* ws = static_cast<int32_t*>(workspace);
    for (int64_t f = 0; f < n_frames; ++f) {
        const Ws w{ws + (f / WG) * WG * stride + f % WG, WG};
        status[f] = decode_frame(buf, core_frame(frames[f]), w, stride, Ws{coef, 1}, crc_tab, out_i32, out_s16);
    }
    return AA_OK;
}
