// MPEG-1 Layer III on the host (C ABI aa_mp3_info / aa_mp3_index /
// aa_mp3_decode / aa_mp3_decode_frames_host / aa_mp3_tables / aa_mp3_table /
// aa_mp3_synth_host, include/aa.h): load_recording's decode
// (src/identify_tracks.py:49-62) for .mp3 files.
//
// This file holds what is serial and small: the walk over the frame headers
// (ID3v2 skipped, Xing / Info / VBRI recognised, resync behind the audio), the
// side-info parse, the flattening of the bit reservoir into one byte stream,
// and the build of the table blob.  Every sample is computed by the core
// (csrc/aa_mp3_core.h), here as host loops, on the device as three kernels
// (csrc/aa_mp3_gpu.hip).  Built with -ffp-contract=off (aa_amd/_build.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(AA_MP3_STANDALONE)
// tools/mp3_core_check.cpp compiles this file with a plain C++ compiler (no
// HIP headers) and supplies aa::set_error and AA_CHECK itself
#include "../../include/aa.h"
#else
#include "aa_common.h"
#endif
#include "aa_mp3_core.h"
#include "aa_mp3_tables.h"

namespace {

using namespace aa_mp3;
namespace tab = aa_mp3_tab;

static_assert(sizeof(Frame) == sizeof(aa_mp3_frame) && sizeof(Frame) == 336, "the core's view of the ABI");
static_assert(sizeof(Stream) == sizeof(aa_mp3_stream) && sizeof(Stream) == 56, "the core's view of the ABI");
static_assert(offsetof(Frame, table_select) == offsetof(aa_mp3_frame, table_select) &&
                  offsetof(Frame, scfsi) == offsetof(aa_mp3_frame, scfsi) &&
                  offsetof(Frame, count1table_select) == offsetof(aa_mp3_frame, count1table_select) &&
                  offsetof(Stream, sr_index) == offsetof(aa_mp3_stream, sr_index),
              "the core's view of the ABI");
static_assert(sizeof(Tables) % 8 == 0, "the blob is copied as 8-byte words");
static_assert(AA_MP3_WG == WG, "one workgroup size");

const double PI = 3.14159265358979323846;

bool build_tree(const tab::CodeSet& cs, int16_t* tree) {
    const int n = cs.table == 32 ? 16 : cs.dim * cs.dim;
    int nodes = 1;
    for (int idx = 0; idx < n; ++idx) {
        const int value = cs.table == 32 ? idx : (idx / cs.dim) * 16 + idx % cs.dim;
        int node = 0;
        for (int b = cs.len[idx] - 1; b >= 0; --b) {
            int16_t& slot = tree[2 * node + ((cs.code[idx] >> b) & 1)];
            if (b == 0) {
                if (slot != 0) return false;
                slot = (int16_t)(-(value + 1));
            } else {
                if (slot < 0) return false;
                if (slot == 0) {
                    if (nodes >= 256) return false;
                    slot = (int16_t)nodes++;
                }
                node = slot;
            }
        }
    }
    return true;
}

const Tables* build_tables() {
    Tables* T = new Tables();
    memset(T, 0, sizeof *T);
    T->magic = MAGIC;
    T->bytes = (int32_t)sizeof(Tables);
    for (int i = 0; i < 8207; ++i) T->pow43[i] = std::pow((double)i, 4.0 / 3.0);
    for (int k = 0; k < 4; ++k) T->pow2q[k] = std::pow(2.0, k / 4.0);
    for (int i = 0; i < 8; ++i) {
        const double c = tab::alias_c[i], r = std::sqrt(1.0 + c * c);
        T->cs[i] = 1.0 / r;
        T->ca[i] = c / r;
    }
    for (int i = 0; i < 36; ++i)
        for (int k = 0; k < 18; ++k) T->cos36[i][k] = std::cos(PI / 72.0 * (2 * i + 1 + 18) * (2 * k + 1));
    for (int i = 0; i < 12; ++i)
        for (int k = 0; k < 6; ++k) T->cos12[i][k] = std::cos(PI / 24.0 * (2 * i + 1 + 6) * (2 * k + 1));
    for (int i = 0; i < 36; ++i) {
        const double lng = std::sin(PI / 36.0 * (i + 0.5));
        T->win[0][i] = lng;
        T->win[1][i] = i < 18 ? lng : i < 24 ? 1.0 : i < 30 ? std::sin(PI / 12.0 * (i - 18 + 0.5)) : 0.0;
        T->win[2][i] = i < 12 ? std::sin(PI / 12.0 * (i + 0.5)) : 0.0;
        T->win[3][i] = i < 6 ? 0.0 : i < 12 ? std::sin(PI / 12.0 * (i - 6 + 0.5)) : i < 18 ? 1.0 : lng;
    }
    for (int i = 0; i < 64; ++i)
        for (int k = 0; k < 32; ++k) T->cosm[i][k] = std::cos((16 + i) * (2 * k + 1) * PI / 64.0);
    for (int i = 0; i < 512; ++i) T->D[i] = tab::synth_window_q16[i] / 65536.0;
    for (int s = 0; s < N_TREES; ++s)
        if (!build_tree(tab::code_sets[s], T->tree[s])) T->magic = 0;  // (a restated table that is no prefix code)
    for (int t = 0; t < 32; ++t) {
        T->tree_of[t] = (int8_t)(t == 0 ? -1 : tab::code_set_of(t));
        T->linbits[t] = tab::linbits[t];
    }
    memcpy(T->slen, tab::slen, sizeof T->slen);
    memcpy(T->pretab, tab::pretab, sizeof T->pretab);
    memcpy(T->sfb_long, tab::sfb_long, sizeof T->sfb_long);
    memcpy(T->sfb_short, tab::sfb_short, sizeof T->sfb_short);
    return T;
}

const Tables& tables() {
    static const Tables* T = build_tables();
    return *T;
}

// ---- headers ------------------------------------------------------------------
struct Hdr {
    int version, layer, prot, br, sr, pad, mode, mode_ext;
    bool l3() const { return version == 3 && layer == 1 && br != 0; }
    int channels() const { return mode == 3 ? 1 : 2; }
    int rate() const { return sr == 0 ? 44100 : sr == 1 ? 48000 : 32000; }
    int len() const {
        static const int kbps[15] = {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320};
        return 144000 * kbps[br] / rate() + pad;
    }
    int side() const { return mode == 3 ? 17 : 32; }
    bool agrees(const Hdr& o) const { return version == o.version && layer == o.layer && sr == o.sr; }
};

bool parse_hdr(const uint8_t* p, Hdr& h) {
    if (p[0] != 0xFF || (p[1] & 0xE0) != 0xE0) return false;
    h = Hdr{(p[1] >> 3) & 3, (p[1] >> 1) & 3, p[1] & 1, p[2] >> 4, (p[2] >> 2) & 3, (p[2] >> 1) & 1, (p[3] >> 6) & 3,
            (p[3] >> 4) & 3};
    return h.version != 1 && h.layer != 0 && h.br != 15 && h.sr != 3;
}

struct Loc {
    size_t pos;
    Hdr h;
};
struct Walk {
    std::vector<Loc> frames;
    Hdr first{};
    int delay = -1, padding = -1;
};

size_t skip_id3v2(const uint8_t* d, size_t len) {
    size_t pos = 0;
    while (pos + 10 <= len && d[pos] == 'I' && d[pos + 1] == 'D' && d[pos + 2] == '3' && d[pos + 3] != 0xFF &&
           d[pos + 4] != 0xFF && !((d[pos + 6] | d[pos + 7] | d[pos + 8] | d[pos + 9]) & 0x80)) {
        const size_t sz = (size_t)d[pos + 6] << 21 | (size_t)d[pos + 7] << 14 | (size_t)d[pos + 8] << 7 | d[pos + 9];
        pos += 10 + sz + ((d[pos + 5] & 0x10) ? 10 : 0);
    }
    return std::min(pos, len);
}

// AA_OK with the audio frames located, AA_ERR_UNSUPPORTED, or AA_ERR_INVALID
int walk(const char* who, const uint8_t* d, size_t len, Walk& w) {
    AA_CHECK(d && len >= 4, AA_ERR_INVALID, "%s: no data", who);
    size_t p = skip_id3v2(d, len);
    Hdr h{};
    bool found = false;
    for (; p + 4 <= len; ++p) {
        if (!parse_hdr(d + p, h)) continue;
        AA_CHECK(h.version == 3, AA_ERR_UNSUPPORTED, "%s: MPEG-2 / MPEG-2.5 (LSF) audio is not decoded", who);
        AA_CHECK(h.layer == 1, AA_ERR_UNSUPPORTED, "%s: Layer %s audio is not decoded", who, h.layer == 3 ? "I" : "II");
        AA_CHECK(h.br != 0, AA_ERR_UNSUPPORTED, "%s: a free-format stream is not decoded", who);
        const size_t nx = p + (size_t)h.len();
        Hdr n{};
        if (nx > len) continue;
        if (nx + 4 <= len && !(parse_hdr(d + nx, n) && n.agrees(h) && n.br != 0)) continue;
        found = true;
        break;
    }
    AA_CHECK(found, AA_ERR_INVALID, "%s: no MPEG audio frame found", who);
    w.first = h;
    // the first frame may be a Xing / Info / VBRI frame: no audio
    {
        const size_t x = p + 4 + (h.prot ? 0 : 2) + h.side(), end = p + (size_t)h.len();
        bool tag = false;
        if (x + 8 <= end && (!memcmp(d + x, "Xing", 4) || !memcmp(d + x, "Info", 4))) {
            tag = true;
            const uint32_t flags = (uint32_t)d[x + 4] << 24 | d[x + 5] << 16 | d[x + 6] << 8 | d[x + 7];
            const size_t v = x + 8 + ((flags & 1) ? 4 : 0) + ((flags & 2) ? 4 : 0) + ((flags & 4) ? 100 : 0) +
                             ((flags & 8) ? 4 : 0);
            if (v + 24 <= end && (!memcmp(d + v, "LAME", 4) || !memcmp(d + v, "Lavf", 4) || !memcmp(d + v, "Lavc", 4))) {
                const uint32_t dp = (uint32_t)d[v + 21] << 16 | d[v + 22] << 8 | d[v + 23];
                w.delay = (int)(dp >> 12);
                w.padding = (int)(dp & 4095);
            }
        } else if (p + 4 + 32 + 4 <= end && !memcmp(d + p + 4 + 32, "VBRI", 4)) {
            tag = true;
        }
        if (tag) p = end;
    }
    while (p + 4 <= len) {
        Hdr n{};
        if (!(parse_hdr(d + p, n) && n.agrees(w.first) && n.br != 0)) {  // resync forward, else the stream ends
            size_t q = p + 1;
            for (; q + 4 <= len; ++q)
                if (parse_hdr(d + q, n) && n.agrees(w.first) && n.br != 0 && q + (size_t)n.len() <= len) break;
            if (q + 4 > len) break;
            p = q;
        }
        if (p + (size_t)n.len() > len) break;  // (cut short)
        AA_CHECK(!(n.mode == 1 && (n.mode_ext & 1)), AA_ERR_UNSUPPORTED, "%s: intensity stereo is not decoded", who);
        if (n.channels() != w.first.channels() && !w.frames.empty()) break;  // (another stream behind this one)
        if (w.frames.empty()) w.first = n;
        w.frames.push_back(Loc{p, n});
        p += (size_t)n.len();
    }
    AA_CHECK(!w.frames.empty(), AA_ERR_INVALID, "%s: no decodable frame", who);
    return AA_OK;
}

void stream_of_walk(const Walk& w, aa_mp3_stream& st) {
    const int64_t n = (int64_t)w.frames.size(), total = n * 1152;
    int64_t skip = 0, end = total;
    if (w.delay >= 0) {
        skip = std::min<int64_t>(total, w.delay + 529);
        end = std::min<int64_t>(total, total - w.padding + 529);
    }
    st = aa_mp3_stream{};
    st.skip = skip;
    st.frames = std::max<int64_t>(0, end - skip);
    st.n_frames = n;
    st.channels = w.first.channels();
    st.sample_rate = w.first.rate();
    st.sr_index = w.first.sr;
}

struct HostBits {
    const uint8_t* p;
    size_t pos = 0;
    uint32_t get(int n) {
        uint32_t v = 0;
        for (; n > 0; --n, ++pos) v = v << 1 | ((p[pos >> 3] >> (7 - (pos & 7))) & 1u);
        return v;
    }
};

// side info of one frame into its record; returns main_data_begin
int parse_side(const uint8_t* si, int channels, aa_mp3_frame& F) {
    HostBits b{si};
    const int mdb = (int)b.get(9);
    b.get(channels == 1 ? 5 : 3);
    for (int c = 0; c < channels; ++c) F.scfsi[c] = (int32_t)b.get(4);
    for (int g = 0; g < 2; ++g)
        for (int c = 0; c < channels; ++c) {
            const int k = g * 2 + c;
            F.part2_3_length[k] = (int32_t)b.get(12);
            F.big_values[k] = (int32_t)b.get(9);
            F.global_gain[k] = (int32_t)b.get(8);
            F.scalefac_compress[k] = (int32_t)b.get(4);
            F.window_switching[k] = (int32_t)b.get(1);
            if (F.window_switching[k]) {
                F.block_type[k] = (int32_t)b.get(2);
                F.mixed[k] = (int32_t)b.get(1);
                for (int r = 0; r < 2; ++r) F.table_select[3 * k + r] = (int32_t)b.get(5);
                for (int w = 0; w < 3; ++w) F.subblock_gain[3 * k + w] = (int32_t)b.get(3);
                F.region0_count[k] = (F.block_type[k] == 2 && !F.mixed[k]) ? 8 : 7;
                F.region1_count[k] = 20 - F.region0_count[k];
            } else {
                for (int r = 0; r < 3; ++r) F.table_select[3 * k + r] = (int32_t)b.get(5);
                F.region0_count[k] = (int32_t)b.get(4);
                F.region1_count[k] = (int32_t)b.get(3);
            }
            F.preflag[k] = (int32_t)b.get(1);
            F.scalefac_scale[k] = (int32_t)b.get(1);
            F.count1table_select[k] = (int32_t)b.get(1);
        }
    return mdb;
}

int make_batch(const char* who, Batch& b, const void* T, const uint8_t* bytes, int64_t n_bytes, const aa_mp3_frame* frames,
               int64_t n_frames, const aa_mp3_stream* streams, int64_t n_streams, const void* out_s16,
               const void* out_f32, int64_t out_elems, int32_t* status, void* workspace, size_t workspace_bytes) {
    AA_CHECK(n_frames >= 0 && n_bytes >= 0 && n_streams >= 0 && out_elems >= 0, AA_ERR_INVALID, "%s: bad sizes", who);
    if (n_frames == 0 || n_streams == 0) return AA_OK;
    AA_CHECK(T && bytes && frames && streams && status, AA_ERR_INVALID, "%s: null argument", who);
    AA_CHECK(out_s16 || out_f32, AA_ERR_INVALID, "%s: no output", who);
    AA_CHECK(n_frames <= 0x3FFFFFFF && n_streams <= 65535, AA_ERR_INVALID, "%s: too many frames or streams", who);
    Plan pl{};
    const size_t need = plan_bytes(n_frames, &pl);
    AA_CHECK(workspace && (uintptr_t)workspace % 8 == 0 && workspace_bytes >= need, AA_ERR_WORKSPACE,
             "%s: workspace null, unaligned or below %zu bytes", who, need);
    char* ws = static_cast<char*>(workspace);
    b = Batch{static_cast<const Tables*>(T), bytes, (long long)n_bytes, reinterpret_cast<const Frame*>(frames),
              (long long)n_frames, reinterpret_cast<const Stream*>(streams), (long long)n_streams,
              reinterpret_cast<int16_t*>(ws + pl.slices_at), reinterpret_cast<double*>(ws + pl.sb_at), status};
    return AA_OK;
}

}  // namespace

extern "C" int aa_mp3_info(const uint8_t* data, size_t len, aa_mp3_stream_info* info) {
    AA_CHECK(info, AA_ERR_INVALID, "aa_mp3_info: null info");
    Walk w;
    const int rc = walk("aa_mp3_info", data, len, w);
    if (rc) return rc;
    aa_mp3_stream st;
    stream_of_walk(w, st);
    *info = aa_mp3_stream_info{st.sample_rate, st.channels, st.frames, (int32_t)st.n_frames, w.delay, w.padding, 0};
    return AA_OK;
}

extern "C" int aa_mp3_index(const uint8_t* data, size_t len, aa_mp3_stream* stream, uint8_t* payload,
                            int64_t payload_cap, int64_t* payload_bytes, aa_mp3_frame* frames, int64_t frame_cap) {
    AA_CHECK(stream && payload_bytes, AA_ERR_INVALID, "aa_mp3_index: null argument");
    Walk w;
    const int rc = walk("aa_mp3_index", data, len, w);
    if (rc) return rc;
    stream_of_walk(w, *stream);
    const int C = stream->channels;
    int64_t need = 0;
    for (const Loc& l : w.frames) need += l.h.len() - 4 - (l.h.prot ? 0 : 2) - l.h.side();
    *payload_bytes = need;
    AA_CHECK(payload && frames && payload_cap >= need && frame_cap >= stream->n_frames, AA_ERR_WORKSPACE,
             "aa_mp3_index: %lld payload bytes and %lld frame records are needed", (long long)need,
             (long long)stream->n_frames);
    int64_t at = 0;
    for (size_t k = 0; k < w.frames.size(); ++k) {
        const Loc& l = w.frames[k];
        const size_t si = l.pos + 4 + (l.h.prot ? 0 : 2);
        aa_mp3_frame F{};
        const int mdb = parse_side(data + si, C, F);  // (before the frame's bytes may be written over)
        const int64_t n = l.h.len() - 4 - (l.h.prot ? 0 : 2) - l.h.side();
        memmove(payload + at, data + si + l.h.side(), (size_t)n);
        F.main_at = at - mdb;
        F.main_lo = 0;
        F.main_end = at + n;
        F.stream = 0;
        F.number = (int32_t)k;
        F.ms = l.h.mode == 1 && (l.h.mode_ext & 2);
        F.nodata = F.main_at < 0;
        frames[k] = F;
        at += n;
    }
    return AA_OK;
}

extern "C" int aa_mp3_tables(void* out, int64_t cap, int64_t* bytes) {
    AA_CHECK(bytes, AA_ERR_INVALID, "aa_mp3_tables: null argument");
    *bytes = (int64_t)sizeof(Tables);
    AA_CHECK(tables().magic == MAGIC, AA_ERR_INVALID, "aa_mp3_tables: a Huffman table is not a prefix code");
    AA_CHECK(out && cap >= *bytes, AA_ERR_WORKSPACE, "aa_mp3_tables: %lld bytes are needed", (long long)*bytes);
    memcpy(out, &tables(), sizeof(Tables));
    return AA_OK;
}

extern "C" int aa_mp3_table(int32_t kind, int32_t index, int32_t* out, int64_t cap, int64_t* n) {
    AA_CHECK(n, AA_ERR_INVALID, "aa_mp3_table: null argument");
    std::vector<int32_t> v;
    if (kind == 0 || kind == 1) {
        if (index == 33) {
            for (int i = 0; i < 16; ++i) v.push_back(kind == 0 ? 15 - i : 4);
        } else {
            const int s = index >= 1 && index <= 32 ? tab::code_set_of(index) : -1;
            AA_CHECK(s >= 0, AA_ERR_INVALID, "aa_mp3_table: there is no Huffman table %d", index);
            const tab::CodeSet& cs = tab::code_sets[s];
            const int cnt = cs.table == 32 ? 16 : cs.dim * cs.dim;
            for (int i = 0; i < cnt; ++i) v.push_back(kind == 0 ? cs.code[i] : cs.len[i]);
        }
    } else if (kind == 2) {
        v.assign(tab::linbits, tab::linbits + 32);
    } else if (kind == 3 && (index == 0 || index == 1)) {
        v.assign(tab::slen[index], tab::slen[index] + 16);
    } else if (kind == 4) {
        v.assign(tab::pretab, tab::pretab + 22);
    } else if (kind == 5 && index >= 0 && index < 3) {
        v.assign(tab::sfb_long[index], tab::sfb_long[index] + 23);
    } else if (kind == 6 && index >= 0 && index < 3) {
        v.assign(tab::sfb_short[index], tab::sfb_short[index] + 14);
    } else if (kind == 7) {
        v.assign(tab::synth_window_q16, tab::synth_window_q16 + 512);
    } else {
        AA_CHECK(false, AA_ERR_INVALID, "aa_mp3_table: no table of kind %d, index %d", kind, index);
    }
    *n = (int64_t)v.size();
    AA_CHECK(out && cap >= *n, AA_ERR_WORKSPACE, "aa_mp3_table: %lld values are needed", (long long)*n);
    std::copy(v.begin(), v.end(), out);
    return AA_OK;
}

extern "C" int aa_mp3_synth_host(const double* sb, int64_t n_slots, double* out) {
    AA_CHECK(n_slots >= 0 && (n_slots == 0 || (sb && out)), AA_ERR_INVALID, "aa_mp3_synth_host: bad arguments");
    const Tables& T = tables();
    std::vector<double> M((size_t)(n_slots + 15) * 64, 0.0);  // 15 silent slots in front
    for (int64_t t = 0; t < n_slots; ++t)
        for (int i = 0; i < 64; ++i) M[(size_t)(t + 15) * 64 + i] = matrix_elem(T, sb + t * 32, nullptr, 15, i);
    for (int64_t t = 0; t < n_slots; ++t)
        for (int j = 0; j < 32; ++j) out[t * 32 + j] = window_elem(T, M.data() + t * 64, 0, j);
    return AA_OK;
}

extern "C" size_t aa_mp3_device_workspace_bytes(int64_t n_frames) {
    if (n_frames <= 0 || n_frames > 0x3FFFFFFF) return 0;
    Plan pl{};
    return plan_bytes(n_frames, &pl);
}

extern "C" int aa_mp3_decode_frames_host(const uint8_t* bytes, int64_t n_bytes, const aa_mp3_frame* frames,
                                         int64_t n_frames, const aa_mp3_stream* streams, int64_t n_streams,
                                         int16_t* out_s16, float* out_f32, int64_t out_elems, int32_t* status,
                                         void* workspace, size_t workspace_bytes) {
    Batch b{};
    AA_CHECK(tables().magic == MAGIC, AA_ERR_INVALID, "aa_mp3_decode_frames_host: a Huffman table is not a prefix code");
    const int rc = make_batch("aa_mp3_decode_frames_host", b, &tables(), bytes, n_bytes, frames, n_frames, streams,
                              n_streams, out_s16, out_f32, out_elems, status, workspace, workspace_bytes);
    if (rc || n_frames == 0 || n_streams == 0) return rc;
    decode_frames_host(b, out_s16, out_f32, (long long)out_elems);
    return AA_OK;
}

extern "C" int aa_mp3_decode(const uint8_t* data, size_t len, float* out, int64_t cap_frames, int64_t* n_frames) {
    AA_CHECK(n_frames, AA_ERR_INVALID, "aa_mp3_decode: null argument");
    aa_mp3_stream st{};
    int64_t pb = 0;
    int rc = aa_mp3_index(data, len, &st, nullptr, 0, &pb, nullptr, 0);
    if (rc != AA_ERR_WORKSPACE) return rc ? rc : AA_ERR_INVALID;
    *n_frames = st.frames;
    if (!out) return AA_OK;
    AA_CHECK(cap_frames >= st.frames, AA_ERR_WORKSPACE, "aa_mp3_decode: the stream holds %lld frames",
             (long long)st.frames);
    std::vector<uint8_t> payload((size_t)pb + 1);
    std::vector<aa_mp3_frame> frames((size_t)st.n_frames);
    rc = aa_mp3_index(data, len, &st, payload.data(), pb, &pb, frames.data(), st.n_frames);
    if (rc) return rc;
    std::vector<int32_t> status((size_t)st.n_frames * 4);
    std::vector<int64_t> ws(aa_mp3_device_workspace_bytes(st.n_frames) / 8 + 1);
    return aa_mp3_decode_frames_host(payload.data(), pb, frames.data(), st.n_frames, &st, 1, nullptr, out,
                                     st.frames * st.channels, status.data(), ws.data(), ws.size() * 8);
}
