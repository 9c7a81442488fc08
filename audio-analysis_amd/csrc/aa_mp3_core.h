// MPEG-1 Layer III decoder core as __host__ __device__ code: the body of
// aa_mp3_decode_device's three kernels (csrc/aa_mp3_gpu.hip) and, run as host
// loops (decode_frames_host below), the host decoder itself -- aa_mp3_decode
// is aa_mp3_index plus those loops (csrc/aa_mp3.cpp); there is no second host
// implementation.  It compiles stand-alone with a plain C++ compiler
// (tools/mp3_core_check.cpp runs it under sanitizers).
//
// The host lays a stream out flat first (aa_mp3_index): headers walked, side
// info parsed into one record per frame, every frame's main-data bytes copied
// back to back, so the bit reservoir is one byte stream and each granule sits
// at an absolute bit position in it.  Then
//
//   unpack   one lane per (frame, channel): scalefactors (granule 1 may reuse
//            granule 0's through scfsi) and the Huffman decode of both
//            granules into int16 is[576], the nonzero bound and a status;
//   hybrid   one group per granule, both channels together: requantise
//            sign * |is|^(4/3) * 2^(e/4), MS stereo, short-block reorder, alias
//            reduction, the 36- / 12-point IMDCT as the standard's direct sums
//            with its four windows, overlap-add with the tails of granule
//            g - 1 (recomputed here: nothing is carried along the stream),
//            frequency inversion -> float64 subband samples [18][32];
//   synth    one group per (granule, channel): the 32 samples of slot t are the
//            window D over the matrixed vectors of slots t - 15 .. t (no V
//            FIFO), rounded once to float32, then libswresample's float -> s16.
//
// Everything is float64 and every transcendental value comes from one table
// blob (Tables) that the host builds once (aa_mp3.cpp: build_tables) and both
// sides read: |is|^(4/3), the four 2^(k/4), the IMDCT and matrixing cosines,
// the windows, the alias coefficients.  Nothing here calls pow, cos or sin.
// One work item computes each output element in one fixed order, and the
// translation units that include this build with -ffp-contract=off, so host
// and device agree bit for bit.
//
// Damage never changes the timeline: a frame whose main_data_begin reaches
// before the stream's data is ST_NODATA, a granule whose side info cannot be
// honoured is ST_MALFORMED, and both decode as a zero spectrum.
//
// Bounds: every load from the main data goes through Bits (clamped to the
// buffer), every table index is range-checked or masked, every store is to the
// lane's workspace slice, the granule's subband block or the stream's output
// range.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AA_MP3_HD __host__ __device__ inline
#else
#define AA_MP3_HD inline
#endif

namespace aa_mp3 {

enum { ST_OK = 0, ST_NODATA = 1, ST_MALFORMED = 2 };
enum { WG = 64, MAGIC = 0x3133706d, N_TREES = 16, TREE_COUNT1 = 15 };
// int16 elements of one lane's unpack slice: per granule is[576], long
// scalefactors [22], short scalefactors [13 * 3], the nonzero bound, and the
// bits of part2_3_length left behind the last value (< 0: a dropped quadruple)
enum { G_IS = 0, G_SFL = 576, G_SFS = 598, G_NZ = 637, G_LEFT = 638, G_WORDS = 640, SLICE = 2 * G_WORDS };

// ---- the table blob (host-built, read by both sides) ----------------------
struct Tables {
    int32_t magic, bytes;
    double pow43[8207];   // i^(4/3)
    double pow2q[4];      // 2^(k/4)
    double cs[8], ca[8];  // alias reduction
    double cos36[36][18]; // cos(pi / 72 (2 i + 1 + 18) (2 k + 1))
    double cos12[12][6];  // cos(pi / 24 (2 i + 1 + 6) (2 k + 1))
    double win[4][36];    // block types 0..3 (type 2: 12 values)
    double cosm[64][32];  // cos((16 + i) (2 k + 1) pi / 64)
    double D[512];        // synthesis window
    // Huffman trees: node n's children at [2 n], [2 n + 1]; > 0 a node, < 0
    // the leaf -(value + 1) with value = x * 16 + y (count1: v w x y as bits),
    // 0 none
    int16_t tree[N_TREES][512];
    int8_t tree_of[32];   // table number -> tree, -1 none
    uint8_t linbits[32];
    uint8_t slen[2][16];
    uint8_t pretab[22];
    uint8_t pad[2];
    uint16_t sfb_long[3][23];
    uint16_t sfb_short[3][14];
    uint16_t pad2;
};

// the side info of one granule of one channel, gathered out of a Frame
struct Granule {
    int32_t part2_3_length, big_values, global_gain, scalefac_compress, window_switching, block_type, mixed;
    int32_t table_select[3], subblock_gain[3];
    int32_t region0_count, region1_count, preflag, scalefac_scale, count1table_select;
};
// ---- the C ABI records (include/aa.h: aa_mp3_frame / aa_mp3_stream) ----
struct Frame {
    int64_t main_at;   // byte of the flat main data where the frame's granules begin (own start - main_data_begin)
    int64_t main_lo;   // first byte of the frame's stream in the flat main data
    int64_t main_end;  // one past the frame's own main data
    int32_t stream, number, ms, nodata, scfsi[2];
    int32_t part2_3_length[4], big_values[4], global_gain[4], scalefac_compress[4], window_switching[4], block_type[4],
        mixed[4], table_select[12], subblock_gain[12], region0_count[4], region1_count[4], preflag[4],
        scalefac_scale[4], count1table_select[4];
    AA_MP3_HD Granule g(int gr, int ch) const {
        const int k = gr * 2 + ch;
        return Granule{part2_3_length[k],
                       big_values[k],
                       global_gain[k],
                       scalefac_compress[k],
                       window_switching[k],
                       block_type[k],
                       mixed[k],
                       {table_select[3 * k], table_select[3 * k + 1], table_select[3 * k + 2]},
                       {subblock_gain[3 * k], subblock_gain[3 * k + 1], subblock_gain[3 * k + 2]},
                       region0_count[k],
                       region1_count[k],
                       preflag[k],
                       scalefac_scale[k],
                       count1table_select[k]};
    }
};
struct Stream {
    int64_t out_at, frames, skip, first_frame, n_frames;
    int32_t channels, sample_rate, sr_index, reserved;
};
struct Plan {
    int64_t n_frames, max_out;
    int64_t slices_at, sb_at;  // byte offsets into the workspace
};

// one lane's slice of the interleaved unpack workspace: element i at p[i * stride]
struct Ws {
    int16_t* p;
    int64_t stride;
    AA_MP3_HD int16_t& operator[](int i) const { return p[(int64_t)i * stride]; }
};

struct NoSync {
    AA_MP3_HD void operator()() const {}
};

// ---- bits of the flat main data, MSB first, clamped to the buffer ----------
struct Bits {
    const uint8_t* p;
    int64_t n_bytes;
    int64_t pos;  // bit position
    AA_MP3_HD uint32_t byte(int64_t i) const { return i >= 0 && i < n_bytes ? p[i] : 0u; }
    // the 25 bits at pos, left-aligned in 32
    AA_MP3_HD uint32_t window() const {
        const int64_t b = pos >> 3;
        const uint32_t w = byte(b) << 24 | byte(b + 1) << 16 | byte(b + 2) << 8 | byte(b + 3);
        return w << (pos & 7);
    }
    AA_MP3_HD uint32_t get(int n) {  // n <= 16
        if (n <= 0) return 0;
        const uint32_t v = window() >> (32 - n);
        pos += n;
        return v;
    }
};

// one code word through a tree; -1: a dead end (no restated table has one)
AA_MP3_HD int huff(const int16_t* tree, Bits& b) {
    uint32_t w = b.window();
    int node = 0;
    for (int used = 0; used < 24; ++used) {
        const int nxt = tree[((2 * node) | (int)(w >> 31)) & 511];
        w <<= 1;
        b.pos += 1;
        if (nxt < 0) return -nxt - 1;
        if (nxt == 0) return -1;
        node = nxt;
    }
    return -1;
}

// bits of scalefactors granule (gr, ch) holds
AA_MP3_HD int part2_bits(const Tables& T, const Frame& F, const Granule& G, int gr, int ch) {
    const int s1 = T.slen[0][G.scalefac_compress & 15], s2 = T.slen[1][G.scalefac_compress & 15];
    if (G.window_switching && G.block_type == 2) return G.mixed ? 17 * s1 + 18 * s2 : 18 * s1 + 18 * s2;
    if (gr == 0) return 11 * s1 + 10 * s2;
    const int f = F.scfsi[ch];
    return ((f & 8) ? 0 : 6 * s1) + ((f & 4) ? 0 : 5 * s1) + ((f & 2) ? 0 : 5 * s2) + ((f & 1) ? 0 : 5 * s2);
}

// Granule (gr, ch) of frame F, its first bit at `start`, into the lane's slice
// at base gr * G_WORDS; sfl0: granule 0's long scalefactors (written by gr 0,
// read by gr 1 under scfsi).  Returns the status.
AA_MP3_HD int unpack_granule(const Tables& T, const uint8_t* bytes, int64_t n_bytes, const Frame& F, int sr_index,
                             int gr, int ch, int64_t start, const Ws& ws, int16_t* sfl0) {
    const Granule G = F.g(gr, ch);
    const int base = gr * G_WORDS;
    for (int i = 0; i < 22; ++i) ws[base + G_SFL + i] = 0;
    for (int i = 0; i < 39; ++i) ws[base + G_SFS + i] = 0;
    ws[base + G_NZ] = 0;
    ws[base + G_LEFT] = 0;
    if (F.nodata) return ST_NODATA;
    const int64_t end = start + G.part2_3_length;
    if (start < F.main_lo * 8 || end > F.main_end * 8 || end > n_bytes * 8) return ST_MALFORMED;
    if (G.big_values < 0 || G.big_values > 288) return ST_MALFORMED;
    const bool sw = G.window_switching != 0;
    if (sw && G.block_type == 0) return ST_MALFORMED;  // (reserved)
    const bool shrt = sw && G.block_type == 2;
    if (part2_bits(T, F, G, gr, ch) > G.part2_3_length) return ST_MALFORMED;
    Bits b{bytes, n_bytes, start};
    const int s1 = T.slen[0][G.scalefac_compress & 15], s2 = T.slen[1][G.scalefac_compress & 15];
    if (shrt) {
        if (G.mixed)
            for (int s = 0; s < 8; ++s) ws[base + G_SFL + s] = (int16_t)b.get(s1);
        for (int s = G.mixed ? 3 : 0; s < 12; ++s)
            for (int w = 0; w < 3; ++w) ws[base + G_SFS + s * 3 + w] = (int16_t)b.get(s < 6 ? s1 : s2);
    } else {
        for (int s = 0; s < 21; ++s) {
            const int grp = s < 6 ? 8 : s < 11 ? 4 : s < 16 ? 2 : 1;
            int16_t v;
            if (gr == 1 && (F.scfsi[ch] & grp))
                v = sfl0[s];
            else
                v = (int16_t)b.get(s < 11 ? s1 : s2);
            ws[base + G_SFL + s] = v;
            if (gr == 0) sfl0[s] = v;
        }
    }
    // big values
    const int sr = sr_index < 0 || sr_index > 2 ? 0 : sr_index;
    int r1, r2;
    if (sw) {
        r1 = 36;
        r2 = 576;
    } else {
        const int a = G.region0_count + 1, c = G.region0_count + G.region1_count + 2;
        r1 = T.sfb_long[sr][a > 22 ? 22 : a < 0 ? 0 : a];
        r2 = T.sfb_long[sr][c > 22 ? 22 : c < 0 ? 0 : c];
    }
    const int bv = 2 * G.big_values;
    int i = 0;
    while (i < bv) {
        const int region = i < r1 ? 0 : i < r2 ? 1 : 2;
        const int limit = region == 0 ? (r1 < bv ? r1 : bv) : region == 1 ? (r2 < bv ? r2 : bv) : bv;
        const int t = G.table_select[region] & 31;
        if (t == 0) {
            for (; i < limit; ++i) ws[base + G_IS + i] = 0;
            continue;
        }
        const int tr = T.tree_of[t];
        if (tr < 0 || tr >= N_TREES) return ST_MALFORMED;
        const int lb = T.linbits[t];
        for (; i < limit; i += 2) {
            const int v = huff(T.tree[tr], b);
            if (v < 0 || b.pos > end) return ST_MALFORMED;
            int x = v >> 4, y = v & 15;
            if (lb && x == 15) x += (int)b.get(lb);
            if (x && b.get(1)) x = -x;
            if (lb && y == 15) y += (int)b.get(lb);
            if (y && b.get(1)) y = -y;
            ws[base + G_IS + i] = (int16_t)x;
            ws[base + G_IS + i + 1] = (int16_t)y;
        }
    }
    if (b.pos > end) return ST_MALFORMED;
    // count1: quadruples of -1, 0, 1 up to the granule's last bit
    while (b.pos < end && i + 4 <= 576) {
        int v;
        if (G.count1table_select)
            v = 15 - (int)b.get(4);
        else
            v = huff(T.tree[TREE_COUNT1], b);
        if (v < 0) return ST_MALFORMED;
        int q[4];
        for (int k = 0; k < 4; ++k) {
            q[k] = (v >> (3 - k)) & 1;
            if (q[k] && b.get(1)) q[k] = -1;
        }
        if (b.pos > end) break;  // overshoots the granule: dropped
        for (int k = 0; k < 4; ++k) ws[base + G_IS + i + k] = (int16_t)q[k];
        i += 4;
    }
    ws[base + G_NZ] = (int16_t)i;
    ws[base + G_LEFT] = (int16_t)(end - b.pos);
    for (; i < 576; ++i) ws[base + G_IS + i] = 0;
    return ST_OK;
}

// lane (frame, channel): both granules; status[gr * 2 + ch] of the frame
AA_MP3_HD void unpack_lane(const Tables& T, const uint8_t* bytes, int64_t n_bytes, const Frame& F, int channels,
                           int sr_index, int ch, const Ws& ws, int32_t* status) {
    if (ch >= channels) {
        status[ch] = status[2 + ch] = ST_OK;
        return;
    }
    int16_t sfl0[22];
    for (int i = 0; i < 22; ++i) sfl0[i] = 0;
    int64_t at = F.main_at * 8;
    for (int gr = 0; gr < 2; ++gr)
        for (int c = 0; c < channels; ++c) {
            if (c == ch) status[gr * 2 + ch] = unpack_granule(T, bytes, n_bytes, F, sr_index, gr, ch, at, ws, sfl0);
            at += F.part2_3_length[gr * 2 + c];
        }
}

// 2^k as a double (k clamped to [-1022, 1023]; a real stream stays within +-100)
AA_MP3_HD double pow2i(int k) {
    k = k < -1022 ? -1022 : k > 1023 ? 1023 : k;
    const uint64_t u = (uint64_t)(k + 1023) << 52;
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}

// requantised line i of a granule (bitstream order)
AA_MP3_HD double requantise(const Tables& T, const Granule& G, int sr, const Ws& ws, int base, int i) {
    const int v = ws[base + G_IS + i];
    if (v == 0 || i >= ws[base + G_NZ]) return 0.0;
    const int mult = G.scalefac_scale ? 4 : 2;
    int e4 = (G.global_gain & 255) - 210;
    const bool shrt = G.window_switching && G.block_type == 2;
    if (shrt && !(G.mixed && i < 36)) {
        int s = 0;
        while (s < 12 && 3 * T.sfb_short[sr][s + 1] <= i) ++s;
        const int width = T.sfb_short[sr][s + 1] - T.sfb_short[sr][s];
        int w = (i - 3 * T.sfb_short[sr][s]) / width;
        w = w < 0 ? 0 : w > 2 ? 2 : w;
        const int sf = s < 12 ? ws[base + G_SFS + s * 3 + w] : 0;
        e4 -= 8 * (G.subblock_gain[w] & 7) + mult * sf;
    } else {
        int s = 0;
        while (s < 21 && T.sfb_long[sr][s + 1] <= i) ++s;
        e4 -= mult * (ws[base + G_SFL + s] + (G.preflag ? T.pretab[s] : 0));
    }
    const int a = v < 0 ? -v : v;
    const double m = T.pow43[a > 8206 ? 8206 : a] * (T.pow2q[e4 & 3] * pow2i(e4 >> 2));
    return v < 0 ? -m : m;
}

// where line j of the reordered spectrum comes from (bitstream order)
AA_MP3_HD int reorder_src(const Tables& T, const Granule& G, int sr, int j) {
    if (!(G.window_switching && G.block_type == 2) || (G.mixed && j < 36)) return j;
    int s = 0;
    while (s < 12 && 3 * T.sfb_short[sr][s + 1] <= j) ++s;
    const int lo = T.sfb_short[sr][s], width = T.sfb_short[sr][s + 1] - lo, rel = j - 3 * lo;
    return 3 * lo + (rel % 3) * width + rel / 3;
}

// The spectrum of granule gr of frame F, ready for the IMDCT, into xr[2][576]
// (tmp[2][576]: scratch).  lanes[c]: channel c's unpack slice; st: the frame's
// four statuses.
template <class Sync>
AA_MP3_HD void spectrum(const Tables& T, const Frame& F, int gr, int C, int sr, const Ws* lanes, const int32_t* st,
                        double* xr, double* tmp, int tid, int nthr, Sync sync) {
    const int base = gr * G_WORDS;
    const Granule Gs[2] = {F.g(gr, 0), F.g(gr, 1)};
    for (int e = tid; e < C * 576; e += nthr) {
        const int c = e / 576, i = e % 576;
        xr[e] = st[gr * 2 + c] == ST_OK ? requantise(T, Gs[c], sr, lanes[c], base, i) : 0.0;
    }
    sync();
    if (C == 2 && F.ms) {
        const double r = 0.70710678118654752440;
        for (int i = tid; i < 576; i += nthr) {
            const double m = xr[i], s = xr[576 + i];
            xr[i] = (m + s) * r;
            xr[576 + i] = (m - s) * r;
        }
        sync();
    }
    for (int e = tid; e < C * 576; e += nthr) {
        const int c = e / 576, j = e % 576;
        tmp[e] = xr[c * 576 + reorder_src(T, Gs[c], sr, j)];
    }
    sync();
    for (int e = tid; e < C * 576; e += nthr) {
        const int c = e / 576, j = e % 576, sb = j / 18, pos = j % 18;
        const Granule& G = Gs[c];
        const int nb = (G.window_switching && G.block_type == 2) ? (G.mixed ? 1 : 0) : 31;  // boundaries 1..nb
        const double* t = tmp + c * 576;
        double v = t[j];
        if (pos < 8 && sb >= 1 && sb <= nb)
            v = t[j] * T.cs[pos] + t[18 * sb - 1 - pos] * T.ca[pos];
        else if (pos >= 10 && sb + 1 <= nb)
            v = t[j] * T.cs[17 - pos] - t[18 * (sb + 1) + (17 - pos)] * T.ca[17 - pos];
        xr[e] = v;
    }
    sync();
}

// output i (0..35) of subband sb's IMDCT, windowed
AA_MP3_HD double imdct_out(const Tables& T, const Granule& G, const double* x /* the channel's [576] */, int sb,
                           int i) {
    int bt = G.window_switching ? G.block_type & 3 : 0;
    if (bt == 2 && G.mixed && sb < 2) bt = 0;
    const double* in = x + 18 * sb;
    if (bt != 2) {
        double s = 0.0;
        for (int k = 0; k < 18; ++k) s += in[k] * T.cos36[i][k];
        return s * T.win[bt][i];
    }
    double s = 0.0;
    for (int w = 0; w < 3; ++w) {
        const int r = i - 6 - 6 * w;
        if (r < 0 || r >= 12) continue;
        double t = 0.0;
        for (int k = 0; k < 6; ++k) t += in[w + 3 * k] * T.cos12[r][k];
        s += t * T.win[2][r];
    }
    return s;
}

// everything the phases need
struct Batch {
    const Tables* T;
    const uint8_t* bytes;
    long long n_bytes;
    const Frame* frames;
    long long n_frames;
    const Stream* streams;
    long long n_streams;
    int16_t* slices;  // [groups][SLICE][WG], lane = frame * 2 + channel
    double* sb;       // [n_frames * 4][18][32], block = (frame * 2 + gr) * 2 + channel
    int32_t* status;  // [n_frames][2][2]
};

AA_MP3_HD Ws lane_ws(const Batch& b, long long lane) {
    return Ws{b.slices + (lane / WG) * WG * SLICE + lane % WG, WG};
}

AA_MP3_HD const Stream* stream_of(const Batch& b, const Frame& F) {
    if (F.stream < 0 || F.stream >= b.n_streams) return nullptr;
    const Stream* s = b.streams + F.stream;
    if (s->channels < 1 || s->channels > 2 || s->sr_index < 0 || s->sr_index > 2) return nullptr;
    return s;
}

AA_MP3_HD void unpack_one(const Batch& b, long long lane) {
    const long long f = lane >> 1;
    const int ch = (int)(lane & 1);
    const Frame& F = b.frames[f];
    const Stream* s = stream_of(b, F);
    int32_t* st = b.status + f * 4;
    if (!s) {
        st[ch] = st[2 + ch] = ST_MALFORMED;
        return;
    }
    unpack_lane(*b.T, b.bytes, b.n_bytes, F, s->channels, s->sr_index, ch, lane_ws(b, lane), st);
}

// granule G (= frame * 2 + gr over the batch): xr, tmp, tail: [2][576] each
template <class Sync>
AA_MP3_HD void hybrid_one(const Batch& b, long long G, double* xr, double* tmp, double* tail, int tid, int nthr,
                          Sync sync) {
    const long long f = G >> 1;
    const int gr = (int)(G & 1);
    const Frame& F = b.frames[f];
    const Stream* s = stream_of(b, F);
    if (!s) return;
    const int C = s->channels, sr = s->sr_index;
    const Tables& T = *b.T;
    const bool has_prev = F.number > 0 || gr > 0;
    if (has_prev && G < 1) return;  // (a table at odds with itself)
    for (int e = tid; e < 2 * 576; e += nthr) tail[e] = 0.0;
    sync();
    if (has_prev) {
        const long long pf = (G - 1) >> 1;
        const int pgr = (int)((G - 1) & 1);
        const Frame& P = b.frames[pf];
        const Ws lanes[2] = {lane_ws(b, pf * 2), lane_ws(b, pf * 2 + 1)};
        spectrum(T, P, pgr, C, sr, lanes, b.status + pf * 4, xr, tmp, tid, nthr, sync);
        const Granule Ps[2] = {P.g(pgr, 0), P.g(pgr, 1)};
        for (int e = tid; e < C * 576; e += nthr) {
            const int c = e / 576, sb = (e % 576) / 18, i = e % 18;
            tail[e] = imdct_out(T, Ps[c], xr + c * 576, sb, 18 + i);
        }
        sync();
    }
    const Ws lanes[2] = {lane_ws(b, f * 2), lane_ws(b, f * 2 + 1)};
    spectrum(T, F, gr, C, sr, lanes, b.status + f * 4, xr, tmp, tid, nthr, sync);
    const Granule Gs[2] = {F.g(gr, 0), F.g(gr, 1)};
    for (int e = tid; e < C * 576; e += nthr) {
        const int c = e / 576, sb = (e % 576) / 18, i = e % 18;
        double v = imdct_out(T, Gs[c], xr + c * 576, sb, i) + tail[e];
        if ((sb & 1) && (i & 1)) v = -v;
        b.sb[(G * 2 + c) * 576 + i * 32 + sb] = v;
    }
    sync();
}

// The matrixed vector element (slot s of 33: the 15 slots before the granule
// and its own 18, i of 64) of block (G, c); prev: the block of granule g - 1
// or null.
AA_MP3_HD double matrix_elem(const Tables& T, const double* cur, const double* prev, int s, int i) {
    const double* S = s >= 15 ? cur + (s - 15) * 32 : prev ? prev + (s + 3) * 32 : nullptr;
    if (!S) return 0.0;
    double v = 0.0;
    for (int k = 0; k < 32; ++k) v += T.cosm[i][k] * S[k];
    return v;
}

// PCM sample j (0..31) of slot u (0..17) of the granule out of M[33][64]
AA_MP3_HD double window_elem(const Tables& T, const double* M, int u, int j) {
    double sum = 0.0;
    for (int i = 0; i < 16; ++i) {
        const int a = i >> 1;
        if (i & 1)
            sum += T.D[j + 64 * a + 32] * M[(u + 15 - 2 * a - 1) * 64 + 32 + j];
        else
            sum += T.D[j + 64 * a] * M[(u + 15 - 2 * a) * 64 + j];
    }
    return sum;
}

AA_MP3_HD int16_t float_to_s16(float x) {
    const double v = __builtin_rint((double)x * 32768.0);
    if (v != v) return (int16_t)-32768;
    return (int16_t)(v < -32768.0 ? -32768.0 : v > 32767.0 ? 32767.0 : v);
}

// block (G, c): M: [33][64] scratch
template <class Sync>
AA_MP3_HD void synth_one(const Batch& b, long long G, int c, double* M, int16_t* out_s16, float* out_f32,
                         long long out_elems, int tid, int nthr, Sync sync) {
    const long long f = G >> 1;
    const Frame& F = b.frames[f];
    const Stream* s = stream_of(b, F);
    if (!s || c >= s->channels) return;
    const long long g = (long long)F.number * 2 + (G & 1);  // granule of the stream
    if (g > 0 && G < 1) return;
    const double* cur = b.sb + (G * 2 + c) * 576;
    const double* prev = g > 0 ? b.sb + ((G - 1) * 2 + c) * 576 : nullptr;
    for (int e = tid; e < 33 * 64; e += nthr) M[e] = matrix_elem(*b.T, cur, prev, e / 64, e % 64);
    sync();
    for (int e = tid; e < 576; e += nthr) {
        const int u = e / 32, j = e % 32;
        const long long n = (g * 18 + u) * 32 + j - s->skip;
        if (n < 0 || n >= s->frames || s->out_at < 0) continue;
        const long long o = s->out_at + n * s->channels + c;
        if (o >= out_elems) continue;
        const float v = (float)window_elem(*b.T, M, u, j);
        if (out_f32) out_f32[o] = v;
        if (out_s16) out_s16[o] = float_to_s16(v);
    }
    sync();
}

// ---- workspace ---------------------------------------------------------------
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

inline size_t plan_bytes(int64_t n_frames, Plan* pl) {
    const int64_t groups = (2 * n_frames + WG - 1) / WG;
    size_t at = 0;
    pl->slices_at = (int64_t)at;
    at = align256(at + (size_t)(groups * WG * SLICE) * sizeof(int16_t));
    pl->sb_at = (int64_t)at;
    at = align256(at + (size_t)n_frames * 4 * 576 * sizeof(double));
    return at;
}

// the three phases as host loops, in the device's layout
inline void decode_frames_host(const Batch& b, int16_t* out_s16, float* out_f32, long long out_elems) {
    for (long long l = 0; l < 2 * b.n_frames; ++l) unpack_one(b, l);
    double* buf = new double[6 * 576 + 33 * 64];
    for (long long G = 0; G < 2 * b.n_frames; ++G)
        hybrid_one(b, G, buf, buf + 2 * 576, buf + 4 * 576, 0, 1, NoSync{});
    for (long long G = 0; G < 2 * b.n_frames; ++G)
        for (int c = 0; c < 2; ++c) synth_one(b, G, c, buf + 6 * 576, out_s16, out_f32, out_elems, 0, 1, NoSync{});
    delete[] buf;
}

}  // namespace aa_mp3
