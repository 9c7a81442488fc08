// Ogg Vorbis decode on the device (C ABI aa_vorbis_decode_device /
// aa_vorbis_decode_packets_host / aa_vorbis_device_workspace_bytes,
// include/aa.h): load_recording's decode (src/identify_tracks.py:49-62) for
// the corpus path, where the host decoder (csrc/aa_vorbis.cpp) bounds a Vorbis
// corpus by its CPUs.  The host indexes a stream (aa_vorbis_index: pages,
// packets, block timeline, flattened setup); three launches decode every
// packet of every stream of a batch through csrc/aa_vorbis_core.h:
//
//   vorbis_unpack  one lane per packet, AA_VORBIS_WG packets per workgroup (one
//                  wave): the entropy decode is serial within a packet and
//                  divergent across packets; the parallelism is the tens of
//                  thousands of packets of a batch.  A lane's workspace slice
//                  (residues, floor curves, classifications) interleaves with
//                  its workgroup's element by element (lane l's element i at
//                  [i * WG + l]), so the wave's accesses at one index share
//                  cache lines.  One status per packet.
//   vorbis_imdct   one workgroup per (packet, channel): Imdct::run in float64
//                  in LDS (Q = n / 4 complex points, at most 2048: 32 KiB),
//                  then the float window product into the packet's block.
//   vorbis_ola     one thread per output frame and channel: the blocks covering
//                  it added onto zero in packet order, inside their nonzero
//                  spans, then libswresample's float -> s16.
//
// This file builds with -ffp-contract=off (aa_amd/_build.py): the outputs are
// held to the host decoder's bits, and a fused multiply-add rounds once where
// the host rounds twice.
#include <algorithm>
#include <vector>

#include "aa_common.h"
#include "aa_vorbis_core.h"

namespace {

using namespace aa_vorbis;

constexpr int WG = AA_VORBIS_WG;
constexpr int IMDCT_THREADS = 256;
constexpr int OLA_THREADS = 256;
constexpr int MAX_Q = 2048;

static_assert(sizeof(Packet) == sizeof(aa_vorbis_packet) && sizeof(Stream) == sizeof(aa_vorbis_stream),
              "the core's views of the C ABI records");
static_assert(offsetof(Packet, stream) == offsetof(aa_vorbis_packet, stream) &&
                  offsetof(Packet, lstart) == offsetof(aa_vorbis_packet, lstart) &&
                  offsetof(Stream, ws_need) == offsetof(aa_vorbis_stream, ws_need) &&
                  offsetof(Stream, channels) == offsetof(aa_vorbis_stream, channels),
              "the core's views of the C ABI records");

// what every phase needs to find a packet's stream and setup
struct Batch {
    const uint8_t* bytes;
    long long n_bytes;
    const Packet* packets;
    long long n_packets;
    const Stream* streams;
    long long n_streams;
    const int32_t* setups;
    long long setup_words;
    float* slices;      // [groups][stride][WG]
    long long stride;
    int32_t* nz;        // [n_packets][MAX_CH]
    float* blk;
    long long blk_floats;
};

// the stream of packet p and its setup, or false (a bad table entry)
AA_VORBIS_HD bool locate(const Batch& b, const Packet& pk, const Stream*& st, Setup& S) {
    if (pk.stream < 0 || pk.stream >= b.n_streams) return false;
    st = b.streams + pk.stream;
    if (st->setup_at < 0 || (st->setup_at & 7) || st->setup_at / 4 >= b.setup_words) return false;
    const int64_t at = st->setup_at / 4, room = b.setup_words - at;
    if (room < (int64_t)(sizeof(Hdr) / 4)) return false;
    const int64_t words = reinterpret_cast<const Hdr*>(b.setups + at)->words;
    if (words < 0 || words > room) return false;
    S = Setup{b.setups + at, words};
    return true;
}

AA_VORBIS_HD int unpack_one(const Batch& b, long long p, const Wsf& ws) {
    const Packet& pk = b.packets[p];
    const Stream* st;
    Setup S;
    int32_t nz[MAX_CH] = {0, 0, 0, 0, 0, 0, 0, 0};
    int status = ST_FALLBACK;
    if (locate(b, pk, st, S) && pk.blk_at >= 0 && pk.n > 0 && st->channels >= 1 && st->channels <= MAX_CH &&
        pk.blk_at + (int64_t)pk.n * st->channels <= b.blk_floats) {
        status = unpack_packet(b.bytes, (uint64_t)b.n_bytes, pk, S.w, S.words, ws, b.stride, nz);
        if (status == ST_OK && S.h().channels != st->channels) status = ST_FALLBACK;
    }
    for (int c = 0; c < MAX_CH; ++c) b.nz[p * MAX_CH + c] = status == ST_OK ? nz[c] : 0;
    return status;
}

// (packet, channel): the spectrum out of the packet's slice -> its windowed
// block; zeros for a silent channel or a packet that is not OK
template <class Sync>
AA_VORBIS_HD void imdct_one(const Batch& b, long long p, int c, const int32_t* status, double* re, double* im,
                            int tid, int nthr, Sync sync) {
    const Packet& pk = b.packets[p];
    const Stream* st;
    Setup S;
    if (!locate(b, pk, st, S) || c >= st->channels || pk.n < 64 || pk.n > 4 * MAX_Q) return;
    const int64_t at = pk.blk_at + (int64_t)c * pk.n;
    if (pk.blk_at < 0 || at + pk.n > b.blk_floats) return;
    float* y = b.blk + at;
    if (status[p] != ST_OK || !b.nz[p * MAX_CH + c]) {  // (status OK: the setup and the table entry were checked)
        for (int i = tid; i < pk.n; i += nthr) y[i] = 0.f;
        return;
    }
    const Hdr& H = S.h();
    const int f = pk.blockflag;
    const float* win = reinterpret_cast<const float*>(S.w + (f ? H.win_long[pk.prev * 2 + pk.next] : H.win_short));
    const Wsf X{b.slices + (p / WG) * WG * b.stride + p % WG + ((int64_t)c * (pk.n / 2)) * WG, WG};
    imdct_window(S, f, X, y, win, re, im, tid, nthr, sync);
}

AA_VORBIS_HD void ola_one(const Batch& b, long long s, long long e, int16_t* out_s16, float* out_f32,
                          long long out_elems) {
    const Stream& st = b.streams[s];
    const int C = st.channels;
    if (C < 1 || C > MAX_CH || st.frames < 0 || e >= st.frames * C) return;
    const int64_t o = st.out_at + e;
    if (st.out_at < 0 || o >= out_elems) return;
    float v = 0.f;
    if (st.first_packet >= 0 && st.n_packets >= 0 && st.first_packet + st.n_packets <= b.n_packets)
        v = ola_sample(b.packets + st.first_packet, st.n_packets, st.bs1, (int)(e % C), st.s0 + e / C, b.blk,
                       b.blk_floats);
    if (out_f32) out_f32[o] = v;
    if (out_s16) out_s16[o] = float_to_s16(v);
}

__global__ __launch_bounds__(WG) void vorbis_unpack(Batch b, int32_t* __restrict__ status) {
    const long long p = (long long)blockIdx.x * WG + threadIdx.x;
    if (p >= b.n_packets) return;
    const Wsf ws{b.slices + (long long)blockIdx.x * WG * b.stride + threadIdx.x, WG};
    status[p] = unpack_one(b, p, ws);
}

struct BlockSync {
    __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(IMDCT_THREADS) void vorbis_imdct(Batch b, const int32_t* __restrict__ status) {
    __shared__ double re[MAX_Q];
    __shared__ double im[MAX_Q];
    // (every thread of a workgroup takes the same early exits: they depend on the packet alone)
    imdct_one(b, (long long)blockIdx.x, (int)blockIdx.y, status, re, im, (int)threadIdx.x, IMDCT_THREADS,
              BlockSync{});
}

__global__ __launch_bounds__(OLA_THREADS) void vorbis_ola(Batch b, int16_t* out_s16, float* out_f32,
                                                          long long out_elems) {
    ola_one(b, (long long)blockIdx.y, (long long)blockIdx.x * OLA_THREADS + threadIdx.x, out_s16, out_f32,
            out_elems);
}

size_t plan_bytes(const aa_vorbis_plan& pl, int64_t n_packets, size_t* nz_at, size_t* blk_at) {
    const int64_t groups = (n_packets + WG - 1) / WG;
    size_t at = aa::align_up((size_t)(groups * WG * pl.stride) * sizeof(float), 256);
    *nz_at = at;
    at = aa::align_up(at + (size_t)n_packets * MAX_CH * sizeof(int32_t), 256);
    *blk_at = at;
    return aa::align_up(at + (size_t)pl.blk_floats * sizeof(float), 256);
}

int make_batch(const char* who, Batch& b, const uint8_t* bytes, int64_t n_bytes, const aa_vorbis_packet* packets,
               int64_t n_packets, const aa_vorbis_stream* streams, int64_t n_streams, const void* setups,
               int64_t setups_bytes, const aa_vorbis_plan* plan, const void* out_s16, const void* out_f32,
               int64_t out_elems, const void* status, void* workspace, size_t workspace_bytes) {
    AA_CHECK(n_packets >= 0 && n_bytes >= 0 && n_streams >= 0 && setups_bytes >= 0 && out_elems >= 0, AA_ERR_INVALID,
             "%s: bad sizes", who);
    if (n_packets == 0 || n_streams == 0) return AA_OK;
    AA_CHECK(bytes && packets && streams && setups && plan && status, AA_ERR_INVALID, "%s: null argument", who);
    AA_CHECK(out_s16 || out_f32, AA_ERR_INVALID, "%s: no output", who);
    AA_CHECK((uintptr_t)setups % 8 == 0, AA_ERR_INVALID, "%s: the setups are not 8-byte aligned", who);
    AA_CHECK(plan->stride >= 1 && plan->blk_floats >= 0 && plan->max_out >= 0 && plan->max_channels >= 1 &&
                 plan->max_channels <= MAX_CH,
             AA_ERR_INVALID, "%s: bad plan", who);
    AA_CHECK(n_packets <= 0x7FFFFFFF && n_streams <= 65535, AA_ERR_INVALID, "%s: too many packets or streams", who);
    size_t nz_at, blk_at;
    const size_t need = plan_bytes(*plan, n_packets, &nz_at, &blk_at);
    AA_CHECK(workspace && (uintptr_t)workspace % 8 == 0 && workspace_bytes >= need, AA_ERR_WORKSPACE,
             "%s: workspace null, unaligned or below %zu bytes", who, need);
    char* ws = static_cast<char*>(workspace);
    b = Batch{bytes, (long long)n_bytes, reinterpret_cast<const Packet*>(packets), (long long)n_packets,
              reinterpret_cast<const Stream*>(streams), (long long)n_streams, static_cast<const int32_t*>(setups),
              (long long)(setups_bytes / 4), reinterpret_cast<float*>(ws), (long long)plan->stride,
              reinterpret_cast<int32_t*>(ws + nz_at), reinterpret_cast<float*>(ws + blk_at),
              (long long)plan->blk_floats};
    return AA_OK;
}

}  // namespace

extern "C" size_t aa_vorbis_device_workspace_bytes(const aa_vorbis_packet* packets, int64_t n_packets,
                                                   const aa_vorbis_stream* streams, int64_t n_streams,
                                                   aa_vorbis_plan* plan) {
    aa_vorbis_plan pl{};
    if (plan) *plan = pl;
    if (!packets || !streams || !plan || n_packets <= 0 || n_streams <= 0) return 0;
    pl.stride = 1;
    pl.max_channels = 1;
    for (int64_t s = 0; s < n_streams; ++s) {
        const aa_vorbis_stream& st = streams[s];
        if (st.channels < 1 || st.channels > MAX_CH || st.frames < 0) return 0;
        pl.max_channels = std::max(pl.max_channels, st.channels);
        pl.max_out = std::max<int64_t>(pl.max_out, st.frames * st.channels);
    }
    for (int64_t p = 0; p < n_packets; ++p) {
        const aa_vorbis_packet& pk = packets[p];
        if (pk.stream < 0 || pk.stream >= n_streams || pk.n < 1 || pk.n > 8192 || pk.blk_at < 0) return 0;
        const aa_vorbis_stream& st = streams[pk.stream];
        pl.stride = std::max<int64_t>(pl.stride, st.ws_need[pk.blockflag ? 1 : 0]);
        pl.blk_floats = std::max<int64_t>(pl.blk_floats, pk.blk_at + (int64_t)pk.n * st.channels);
    }
    *plan = pl;
    size_t a, b;
    return plan_bytes(pl, n_packets, &a, &b);
}

extern "C" int aa_vorbis_decode_device(const uint8_t* bytes_dev, int64_t n_bytes, const aa_vorbis_packet* packets_dev,
                                       int64_t n_packets, const aa_vorbis_stream* streams_dev, int64_t n_streams,
                                       const void* setups_dev, int64_t setups_bytes, const aa_vorbis_plan* plan,
                                       int16_t* out_s16, float* out_f32, int64_t out_elems, int32_t* status_dev,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    Batch b{};
    const int rc = make_batch("aa_vorbis_decode_device", b, bytes_dev, n_bytes, packets_dev, n_packets, streams_dev,
                              n_streams, setups_dev, setups_bytes, plan, out_s16, out_f32, out_elems, status_dev,
                              workspace, workspace_bytes);
    if (rc || n_packets == 0 || n_streams == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned groups = (unsigned)((n_packets + WG - 1) / WG);
    hipLaunchKernelGGL(vorbis_unpack, dim3(groups), dim3(WG), 0, st, b, status_dev);
    AA_LAUNCH_CHECK();
    hipLaunchKernelGGL(vorbis_imdct, dim3((unsigned)n_packets, (unsigned)plan->max_channels), dim3(IMDCT_THREADS), 0,
                       st, b, status_dev);
    AA_LAUNCH_CHECK();
    if (plan->max_out > 0) {
        const int64_t gx = (plan->max_out + OLA_THREADS - 1) / OLA_THREADS;
        AA_CHECK(gx <= 0x7FFFFFFF, AA_ERR_INVALID, "aa_vorbis_decode_device: a stream of too many samples");
        hipLaunchKernelGGL(vorbis_ola, dim3((unsigned)gx, (unsigned)n_streams), dim3(OLA_THREADS), 0, st, b, out_s16,
                           out_f32, (long long)out_elems);
        AA_LAUNCH_CHECK();
    }
    return AA_OK;
}

extern "C" int aa_vorbis_decode_packets_host(const uint8_t* bytes, int64_t n_bytes, const aa_vorbis_packet* packets,
                                             int64_t n_packets, const aa_vorbis_stream* streams, int64_t n_streams,
                                             const void* setups, int64_t setups_bytes, const aa_vorbis_plan* plan,
                                             int16_t* out_s16, float* out_f32, int64_t out_elems, int32_t* status,
                                             void* workspace, size_t workspace_bytes, void*) {
    Batch b{};
    const int rc = make_batch("aa_vorbis_decode_packets_host", b, bytes, n_bytes, packets, n_packets, streams,
                              n_streams, setups, setups_bytes, plan, out_s16, out_f32, out_elems, status, workspace,
                              workspace_bytes);
    if (rc || n_packets == 0 || n_streams == 0) return rc;
    // the device's layout and phases, one after the other
    for (int64_t p = 0; p < n_packets; ++p)
        status[p] = unpack_one(b, p, Wsf{b.slices + (p / WG) * WG * b.stride + p % WG, WG});
    std::vector<double> re(MAX_Q), im(MAX_Q);
    for (int64_t p = 0; p < n_packets; ++p)
        for (int c = 0; c < plan->max_channels; ++c) imdct_one(b, p, c, status, re.data(), im.data(), 0, 1, NoSync{});
    for (int64_t s = 0; s < n_streams; ++s)
        for (int64_t e = 0; e < plan->max_out; ++e) ola_one(b, s, e, out_s16, out_f32, out_elems);
    return AA_OK;
}
