// Vorbis I audio packet decoder core as __host__ __device__ code: the body of
// aa_vorbis_decode_device's three kernels and of aa_vorbis_decode_packets_host's
// loops (csrc/aa_vorbis_gpu.hip); it compiles stand-alone with a plain C++
// compiler (tools/vorbis_core_check.cpp runs it under sanitizers).
//
// It restates the host decoder (csrc/aa_vorbis.cpp: Decoder::audio, Imdct::run
// and decode_all's overlap-add), which is its oracle, over a FLATTENED setup:
// one blob of 32-bit words that aa_vorbis_index writes on the host -- codebook
// trees and expanded VQ tables, floor 1 / residue / mapping / mode records,
// the inverse-dB ramp, the IMDCT twiddles (doubles) and the window tables, every
// value the one the host decoder itself uses -- so nothing here calls cos, sin
// or pow.  The rule it keeps for EVERY packet: either the samples are the host
// decoder's bit for bit and the status is ST_OK, or the status is ST_FALLBACK.
// That holds because the Vorbis specification (and the host decoder) define
// the output for every bit pattern -- an end of packet means "stop, keep what
// was added" -- and every float operation here is the host's, in the host's
// order (the translation units that include this build with -ffp-contract=off).
//
// Bounds: every load from the packet bytes goes through Bits::load64, clamped
// to the buffer; every setup access is checked against the blob's size
// (a failed check sets Ctx::bad -> ST_FALLBACK; the host-validated setup makes
// that impossible, it is checked anyway); every store is to the packet's
// workspace slice [0, ws_cap), its block [0, n) per channel, or the stream's
// output range.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AA_VORBIS_HD __host__ __device__ inline
#else
#define AA_VORBIS_HD inline
#endif

namespace aa_vorbis {

enum { ST_OK = 0, ST_FALLBACK = 1 };
enum { MAX_CH = 8, MAGIC = 0x31627356 };

// ---- the flattened setup: int32 words; `off` fields are word offsets from
// the blob's start, doubles sit on even offsets (the blob is 8-byte aligned)
struct Hdr {
    int32_t magic, words, channels, bs[2], n_books, n_floors, n_res, n_maps, n_modes;
    int32_t books, floors, res, maps, modes;  // arrays of the records below
    int32_t inv_db;                           // float[256]
    int32_t mdct[2];                          // one Mdct record per block size
    int32_t win_short, win_long[4];           // float[bs0]; float[bs1] per [prev long * 2 + next long]
    int32_t cls_cap[2];                       // words of classification buffer a packet of either size may need
    int32_t pad;
};
struct Book {
    int32_t dims, entries, lookup, single, single_len;
    int32_t n_nodes, node;  // int32[2 * n_nodes]: children, >0 node, <0 leaf -(entry + 1), 0 none
    int32_t vq;             // float[entries * dims] when lookup != 0
};
struct Floor1 {
    int32_t type, parts, mult, nv;
    int32_t part_class[31], cdim[16], csub[16], cmaster[16], subbooks[16][8];
    int32_t X[65], order1[65], lo[65], hi[65];
};
struct Res {
    int32_t type, begin, end, psize, classes, classbook, books[64][8];
};
struct Map {
    int32_t submaps, steps, mag[256], ang[256], mux[MAX_CH], sub_floor[16], sub_res[16];
};
struct Mode {
    int32_t blockflag, mapping;
};
struct Mdct {
    int32_t Q, pre_c, pre_s, post_c, post_s, fft_c, fft_s;  // double[Q] x 4, double[Q / 2 + 1] x 2
    int32_t rev;                                             // int32[Q]
};

// the fields of aa_vorbis_packet / aa_vorbis_stream the core needs (include/aa.h)
struct Packet {
    int64_t offset, pos, blk_at;
    int32_t nbytes, n, blockflag, prev, next, lstart, rend, stream;
};
struct Stream {
    int64_t setup_at, out_at, frames, s0, first_packet, n_packets;
    int32_t channels, sample_rate, bs0, bs1, ws_need[2];
};

AA_VORBIS_HD int ilog(uint32_t x) { return x ? 32 - __builtin_clz(x) : 0; }

struct Setup {
    const int32_t* w;
    int64_t words;
    AA_VORBIS_HD const Hdr& h() const { return *reinterpret_cast<const Hdr*>(w); }
    AA_VORBIS_HD bool span(int32_t off, int64_t n) const { return off >= 0 && n >= 0 && (int64_t)off + n <= words; }
    template <class T>
    AA_VORBIS_HD const T* rec(int32_t base, int i) const {
        return reinterpret_cast<const T*>(w + base) + i;
    }
    // header-level ranges, once per packet
    AA_VORBIS_HD bool ok() const {
        const int HW = (int)(sizeof(Hdr) / 4);
        if (!w || words < HW) return false;
        const Hdr& H = h();
        if (H.magic != MAGIC || H.words != words || (H.words & 1)) return false;
        if (H.channels < 1 || H.channels > MAX_CH) return false;
        for (int f = 0; f < 2; ++f)
            if (H.bs[f] < 64 || H.bs[f] > 8192 || (H.bs[f] & (H.bs[f] - 1))) return false;
        if (H.bs[0] > H.bs[1]) return false;
        if (H.n_books < 1 || H.n_floors < 1 || H.n_res < 1 || H.n_maps < 1 || H.n_modes < 1) return false;
        if (!span(H.books, (int64_t)H.n_books * (int64_t)(sizeof(Book) / 4))) return false;
        if (!span(H.floors, (int64_t)H.n_floors * (int64_t)(sizeof(Floor1) / 4))) return false;
        if (!span(H.res, (int64_t)H.n_res * (int64_t)(sizeof(Res) / 4))) return false;
        if (!span(H.maps, (int64_t)H.n_maps * (int64_t)(sizeof(Map) / 4))) return false;
        if (!span(H.modes, (int64_t)H.n_modes * (int64_t)(sizeof(Mode) / 4))) return false;
        if (!span(H.inv_db, 256)) return false;
        if (!span(H.win_short, H.bs[0])) return false;
        for (int v = 0; v < 4; ++v)
            if (!span(H.win_long[v], H.bs[1])) return false;
        for (int f = 0; f < 2; ++f) {
            if (!span(H.mdct[f], (int64_t)(sizeof(Mdct) / 4))) return false;
            const Mdct& m = *rec<Mdct>(H.mdct[f], 0);
            const int Q = H.bs[f] / 4;
            if (m.Q != Q) return false;
            const int32_t d[4] = {m.pre_c, m.pre_s, m.post_c, m.post_s};
            for (int i = 0; i < 4; ++i)
                if ((d[i] & 1) || !span(d[i], 2 * (int64_t)Q)) return false;
            if ((m.fft_c & 1) || (m.fft_s & 1) || !span(m.fft_c, 2 * (int64_t)(Q / 2 + 1)) ||
                !span(m.fft_s, 2 * (int64_t)(Q / 2 + 1)) || !span(m.rev, Q))
                return false;
            if (H.cls_cap[f] < 0) return false;
        }
        return true;
    }
};

// ---- LSB-first bit reader (Vorbis I 2.1.4) with the host's end-of-packet
// rule: a read past the packet's last bit returns 0, sets eop and parks the
// position at the end.  A 64-bit window of the bytes is kept in registers.
struct Bits {
    const uint8_t* p;  // the whole buffer
    uint64_t total;    // its size
    uint64_t at;       // the packet's first byte
    uint64_t nbits;    // the packet's size in bits
    uint64_t pos;      // bit position inside the packet
    uint64_t win, wpos;
    int have;
    bool eop;

    AA_VORBIS_HD void start(const uint8_t* buf, uint64_t n_buf, uint64_t offset, uint64_t nbytes) {
        p = buf;
        total = n_buf;
        at = offset;
        nbits = nbytes * 8;
        pos = 0;
        win = 0;
        wpos = 0;
        have = 0;
        eop = false;
    }
    AA_VORBIS_HD uint64_t load64(uint64_t b) const {  // little-endian, zero past the buffer's end
        if (b + 8 <= total) {
            uint64_t v;
            __builtin_memcpy(&v, p + b, 8);
            return v;
        }
        uint64_t v = 0;
        for (int i = 0; i < 8; ++i)
            if (b + (uint64_t)i < total) v |= (uint64_t)p[b + (uint64_t)i] << (8 * i);
        return v;
    }
    AA_VORBIS_HD uint32_t get(int k) {  // k in [0, 32]
        if (k <= 0) return 0;
        if (pos + (uint64_t)k > nbits) {
            eop = true;
            pos = nbits;
            return 0;
        }
        if (pos < wpos || pos + (uint64_t)k > wpos + (uint64_t)have) {
            wpos = pos & ~(uint64_t)7;
            win = load64(at + (wpos >> 3));
            have = 64;
        }
        const uint64_t v = win >> (pos - wpos);  // shift <= 63: pos - wpos + k <= 64, k >= 1
        pos += (uint64_t)k;
        return (uint32_t)(v & (k == 32 ? 0xffffffffull : ((1ull << k) - 1)));
    }
};

struct Wsf {  // a packet's float workspace: element i at p[i * step]
    float* p;
    int64_t step;
    AA_VORBIS_HD float& operator[](int64_t i) const { return p[i * step]; }
};

struct Ctx {
    Setup S;
    Bits br;
    bool bad;
};

// Codebook::decode: entry number, -1 at end of packet / undecodable
AA_VORBIS_HD int book_decode(Ctx& c, int bi) {
    const Hdr& H = c.S.h();
    if (bi < 0 || bi >= H.n_books) {
        c.bad = true;
        return -1;
    }
    const Book& b = *c.S.rec<Book>(H.books, bi);
    if (b.single >= 0) {
        if (b.single_len > 32) {
            c.bad = true;
            return -1;
        }
        c.br.get(b.single_len);
        return c.br.eop ? -1 : b.single;
    }
    if (b.n_nodes <= 0) return -1;
    if (!c.S.span(b.node, 2 * (int64_t)b.n_nodes)) {
        c.bad = true;
        return -1;
    }
    const int32_t* node = c.S.w + b.node;
    int32_t at = 0;
    for (;;) {
        const int bit = (int)c.br.get(1);
        if (c.br.eop) return -1;
        const int32_t nx = node[2 * at + bit];
        if (nx < 0) return -nx - 1;
        if (nx == 0) return -1;
        if (nx >= b.n_nodes) {
            c.bad = true;
            return -1;
        }
        at = nx;
    }
}

// the VQ vector of entry e of book bi (residues; the book has a lookup)
AA_VORBIS_HD const float* book_vec(Ctx& c, int bi, int e, int& dims) {
    const Hdr& H = c.S.h();
    const Book& b = *c.S.rec<Book>(H.books, bi);  // (bi was checked by book_decode)
    dims = b.dims;
    if (!b.lookup || e < 0 || e >= b.entries || b.dims < 1 ||
        !c.S.span(b.vq, (int64_t)b.entries * (int64_t)b.dims)) {
        c.bad = true;
        return nullptr;
    }
    return reinterpret_cast<const float*>(c.S.w + b.vq) + (int64_t)e * b.dims;
}

AA_VORBIS_HD int iabs(int v) { return v < 0 ? -v : v; }
AA_VORBIS_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// Vorbis I 9.2.7 into curve[0, n)
AA_VORBIS_HD void render_line(const float* inv_db, int x0, int y0, int x1, int y1, const Wsf& curve, int n) {
    const int dy = y1 - y0, adx = x1 - x0;
    if (adx <= 0) return;
    int ady = iabs(dy);
    const int base = dy / adx;
    const int sy = dy < 0 ? base - 1 : base + 1;
    ady -= iabs(base) * adx;
    int y = y0, err = 0;
    if (x0 < n) curve[x0] = inv_db[clamp255(y)];
    for (int x = x0 + 1; x < x1; ++x) {
        err += ady;
        if (err >= adx) {
            err -= adx;
            y += sy;
        } else {
            y += base;
        }
        if (x < n) curve[x] = inv_db[clamp255(y)];
    }
}

// floor 1 of one channel into curve[0, n2); false = unused
AA_VORBIS_HD bool floor1_decode(Ctx& c, const Floor1& f, int n2, const Wsf& curve) {
    Bits& br = c.br;
    if (!br.get(1) || br.eop) return false;
    if (f.type != 1 || f.mult < 1 || f.mult > 4 || f.nv < 2 || f.nv > 65 || f.parts < 0 || f.parts > 31) {
        c.bad = true;
        return false;
    }
    const int range = f.mult == 1 ? 256 : f.mult == 2 ? 128 : f.mult == 3 ? 86 : 64;
    const int nv = f.nv;
    int Y[65];
    const int rbits = ilog((uint32_t)(range - 1));
    Y[0] = (int)br.get(rbits);
    Y[1] = (int)br.get(rbits);
    int off = 2;
    for (int i = 0; i < f.parts; ++i) {
        const int cl = f.part_class[i];
        if (cl < 0 || cl > 15) {
            c.bad = true;
            return false;
        }
        const int cd = f.cdim[cl], cb = f.csub[cl], cs = (1 << cb) - 1;
        if (cd < 1 || cd > 8 || cb < 0 || cb > 3 || off + cd > nv) {
            c.bad = true;
            return false;
        }
        int cval = 0;
        if (cb) {
            cval = book_decode(c, f.cmaster[cl]);
            if (cval < 0) return false;
        }
        for (int j = 0; j < cd; ++j) {
            const int book = f.subbooks[cl][cval & cs];
            cval >>= cb;
            if (book >= 0) {
                const int e = book_decode(c, book);
                if (e < 0) return false;
                Y[off + j] = e;
            } else {
                Y[off + j] = 0;
            }
        }
        off += cd;
    }
    if (br.eop) return false;
    if (off != nv) {
        c.bad = true;
        return false;
    }
    // amplitude values (Vorbis I 7.2.4 step 1)
    int fy[65];
    uint64_t step2 = 3, step2_hi = 0;  // bit i of (step2, step2_hi): point i is used
    fy[0] = Y[0];
    fy[1] = Y[1];
    for (int i = 2; i < nv; ++i) {
        const int lo = f.lo[i], hi = f.hi[i];
        if (lo < 0 || lo >= i || hi < 0 || hi >= i) {
            c.bad = true;
            return false;
        }
        const int x0 = f.X[lo], y0 = fy[lo], x1 = f.X[hi], y1 = fy[hi];
        const int dy = y1 - y0, adx = x1 - x0, ady = iabs(dy);
        if (adx == 0) {
            c.bad = true;
            return false;
        }
        const int offp = ady * (f.X[i] - x0) / adx;
        const int pred = dy < 0 ? y0 - offp : y0 + offp;
        const int val = Y[i];
        const int highroom = range - pred, lowroom = pred;
        const int room = (highroom < lowroom ? highroom : lowroom) * 2;
        if (val) {
            step2 |= 1ull << lo;  // lo, hi < i <= 64
            step2 |= 1ull << hi;
            if (i < 64) step2 |= 1ull << i;
            else step2_hi = 1;
            if (val >= room)
                fy[i] = highroom > lowroom ? val - lowroom + pred : pred - val + highroom - 1;
            else
                fy[i] = (val & 1) ? pred - (val + 1) / 2 : pred + val / 2;
        } else {
            fy[i] = pred;
        }
    }
    // curve synthesis (step 2), in X order
    const float* inv_db = reinterpret_cast<const float*>(c.S.w + c.S.h().inv_db);
    const int o0 = f.order1[0];
    if (o0 < 0 || o0 >= nv) {
        c.bad = true;
        return false;
    }
    int hx = 0, hy = 0, lx = 0, ly = fy[o0] * f.mult;
    for (int k = 1; k < nv; ++k) {
        const int i = f.order1[k];
        if (i < 0 || i >= nv) {
            c.bad = true;
            return false;
        }
        const bool used = i < 64 ? ((step2 >> i) & 1) != 0 : step2_hi != 0;
        if (used) {
            hy = fy[i] * f.mult;
            hx = f.X[i];
            render_line(inv_db, lx, ly, hx, hy, curve, n2);
            lx = hx;
            ly = hy;
        }
    }
    if (hx < n2) render_line(inv_db, hx, hy, n2, hy, curve, n2);
    return true;
}

// The residue vectors of one submap as residue_decode01 sees them: vector j's
// element i.  Types 0 / 1: the submap's channel chs[j].  Type 2: ONE vector of
// n2 * k elements interleaving the k channels, written straight to where the
// host's de-interleave would copy it (its temporary starts zeroed, as the
// channels' vectors do).
struct View {
    Wsf ws;
    int n2, k, chs[MAX_CH];
    bool t2;
    AA_VORBIS_HD float& at(int j, int64_t i) const {
        if (t2) return ws[(int64_t)chs[i % k] * n2 + i / k];
        return ws[(int64_t)chs[j] * n2 + i];
    }
};

// residue formats 0 / 1 (Vorbis I 8.6.2-4): the host's pass and partition
// order, its classification buffer (cls, as floats of small integers), its
// early returns
AA_VORBIS_HD void residue01(Ctx& c, const Res& r, int type, const View& v, int ch, uint32_t dnd, int n,
                            const Wsf& cls, int64_t cls_cap) {
    const int lb = r.begin < n ? r.begin : n, le = r.end < n ? r.end : n;
    const int ntr = le - lb;
    if (ntr <= 0) return;
    const Hdr& H = c.S.h();
    if (r.psize < 1 || r.classes < 1 || r.classes > 64 || r.classbook < 0 || r.classbook >= H.n_books) {
        c.bad = true;
        return;
    }
    const int nparts = ntr / r.psize;
    const int cpw = c.S.rec<Book>(H.books, r.classbook)->dims;
    const int64_t W = (int64_t)nparts + cpw;
    if (cpw < 1 || (int64_t)ch * W > cls_cap) {
        c.bad = true;
        return;
    }
    for (int64_t i = 0; i < (int64_t)ch * W; ++i) cls[i] = 0.f;
    for (int pass = 0; pass < 8; ++pass) {
        int pc = 0;
        while (pc < nparts) {
            if (pass == 0) {
                for (int j = 0; j < ch; ++j) {
                    if ((dnd >> j) & 1) continue;
                    int temp = book_decode(c, r.classbook);
                    if (temp < 0) return;
                    for (int i = cpw - 1; i >= 0; --i) {
                        cls[(int64_t)j * W + i + pc] = (float)(temp % r.classes);
                        temp /= r.classes;
                    }
                }
            }
            for (int i = 0; i < cpw && pc < nparts; ++i, ++pc) {
                for (int j = 0; j < ch; ++j) {
                    if ((dnd >> j) & 1) continue;
                    const int cl = (int)cls[(int64_t)j * W + pc];
                    const int bk = r.books[cl][pass];
                    if (bk < 0) continue;
                    const int64_t base = (int64_t)lb + (int64_t)pc * r.psize;
                    int dims = 0;
                    if (type == 0) {
                        if (bk >= H.n_books) {
                            c.bad = true;
                            return;
                        }
                        const int bd = c.S.rec<Book>(H.books, bk)->dims;
                        if (bd < 1) {
                            c.bad = true;
                            return;
                        }
                        const int step = r.psize / bd;
                        for (int s = 0; s < step; ++s) {
                            const int e = book_decode(c, bk);
                            if (e < 0) return;
                            const float* vec = book_vec(c, bk, e, dims);
                            if (!vec) return;
                            for (int k = 0; k < dims; ++k) v.at(j, base + s + (int64_t)k * step) += vec[k];
                        }
                    } else {
                        int s = 0;
                        while (s < r.psize) {
                            const int e = book_decode(c, bk);
                            if (e < 0) return;
                            const float* vec = book_vec(c, bk, e, dims);
                            if (!vec) return;
                            for (int k = 0; k < dims && s < r.psize; ++k) v.at(j, base + s++) += vec[k];
                        }
                    }
                }
            }
        }
    }
}

// One audio packet up to its spectra (Decoder::audio before the IMDCT).
// ws: the packet's slice, ws_cap floats: channel c's residue / spectrum at
// [c * n2, (c + 1) * n2), its floor curve at [(C + c) * n2, ...), then the
// classification buffer.  nz_out[c]: channel c's floor is used (an unused one
// leaves the channel silent).
AA_VORBIS_HD int unpack_packet(const uint8_t* bytes, uint64_t n_bytes, const Packet& pk, const int32_t* setup,
                               int64_t setup_words, const Wsf& ws, int64_t ws_cap, int32_t* nz_out) {
    Ctx c;
    c.S = Setup{setup, setup_words};
    c.bad = false;
    if (!c.S.ok()) return ST_FALLBACK;
    if (pk.offset < 0 || pk.nbytes < 1 || (uint64_t)pk.offset + (uint64_t)pk.nbytes > n_bytes) return ST_FALLBACK;
    const Hdr& H = c.S.h();
    const int C = H.channels;
    Bits& br = c.br;
    br.start(bytes, n_bytes, (uint64_t)pk.offset, (uint64_t)pk.nbytes);
    // the table is the host's reading of these same bits
    if (br.get(1) != 0) return ST_FALLBACK;
    const int mn = (int)br.get(ilog((uint32_t)(H.n_modes - 1)));
    if (br.eop || mn >= H.n_modes) return ST_FALLBACK;
    const Mode& md = *c.S.rec<Mode>(H.modes, mn);
    const int f = md.blockflag;
    if (f < 0 || f > 1 || md.mapping < 0 || md.mapping >= H.n_maps) return ST_FALLBACK;
    const int n = H.bs[f], n2 = n / 2;
    int pl = 1, nl = 1;
    if (f) {
        pl = (int)br.get(1);
        nl = (int)br.get(1);
    }
    if (pk.n != n || pk.blockflag != f || pk.prev != pl || pk.next != nl) return ST_FALLBACK;
    const int64_t cls_at = 2 * (int64_t)C * n2, cls_cap = H.cls_cap[f];
    if (cls_at + cls_cap > ws_cap) return ST_FALLBACK;
    const Map& m = *c.S.rec<Map>(H.maps, md.mapping);
    if (m.submaps < 1 || m.submaps > 16 || m.steps < 0 || m.steps > 256) return ST_FALLBACK;
    for (int64_t i = 0; i < cls_at; ++i) ws[i] = 0.f;
    uint32_t nz = 0;
    for (int ch = 0; ch < C; ++ch) {
        const int mux = m.mux[ch];
        if (mux < 0 || mux >= m.submaps) return ST_FALLBACK;
        const int fi = m.sub_floor[mux];
        if (fi < 0 || fi >= H.n_floors) return ST_FALLBACK;
        const Wsf curve{ws.p + ((int64_t)(C + ch) * n2) * ws.step, ws.step};
        if (floor1_decode(c, *c.S.rec<Floor1>(H.floors, fi), n2, curve)) nz |= 1u << ch;
    }
    uint32_t no_res = ~nz & ((1u << C) - 1);
    for (int s = 0; s < m.steps; ++s) {
        const int a = m.mag[s], b = m.ang[s];
        if (a < 0 || a >= C || b < 0 || b >= C) return ST_FALLBACK;
        if (!((no_res >> a) & 1) || !((no_res >> b) & 1)) no_res &= ~((1u << a) | (1u << b));
    }
    const Wsf cls{ws.p + cls_at * ws.step, ws.step};
    for (int s = 0; s < m.submaps; ++s) {
        View v;
        v.ws = ws;
        v.n2 = n2;
        v.k = 0;
        uint32_t dnd = 0;
        for (int ch = 0; ch < C; ++ch)
            if (m.mux[ch] == s) {
                if ((no_res >> ch) & 1) dnd |= 1u << v.k;
                v.chs[v.k++] = ch;
            }
        const int ri = m.sub_res[s];
        if (ri < 0 || ri >= H.n_res) return ST_FALLBACK;
        const Res& r = *c.S.rec<Res>(H.res, ri);
        if (r.type == 2) {
            if (dnd == (1u << v.k) - 1) continue;  // (no channel of the submap: nothing decoded either)
            v.t2 = true;
            residue01(c, r, 1, v, 1, 0, n2 * v.k, cls, cls_cap);
        } else if (r.type == 0 || r.type == 1) {
            v.t2 = false;
            residue01(c, r, r.type, v, v.k, dnd, n2, cls, cls_cap);
        } else {
            return ST_FALLBACK;
        }
    }
    for (int s = m.steps - 1; s >= 0; --s) {  // inverse coupling (Vorbis I 4.3.5)
        const Wsf M_{ws.p + ((int64_t)m.mag[s] * n2) * ws.step, ws.step};
        const Wsf A{ws.p + ((int64_t)m.ang[s] * n2) * ws.step, ws.step};
        for (int j = 0; j < n2; ++j) {
            const float M0 = M_[j], A0 = A[j];
            float nm, na;
            if (M0 > 0) {
                if (A0 > 0) { nm = M0; na = M0 - A0; } else { na = M0; nm = M0 + A0; }
            } else {
                if (A0 > 0) { nm = M0; na = M0 + A0; } else { na = M0; nm = M0 - A0; }
            }
            M_[j] = nm;
            A[j] = na;
        }
    }
    for (int ch = 0; ch < C; ++ch) {
        nz_out[ch] = (nz >> ch) & 1;
        if (!((nz >> ch) & 1)) continue;
        for (int j = 0; j < n2; ++j) ws[(int64_t)ch * n2 + j] *= ws[(int64_t)(C + ch) * n2 + j];
    }
    return c.bad ? ST_FALLBACK : ST_OK;
}

// Imdct::run and the window product for one (packet, channel): X the spectrum
// (n / 2 values, element i at X[i]), y the block (n floats), re / im: Q = n / 4
// doubles each.  `nthr` callers share the work, `sync` is their barrier.  The
// independent butterflies of a stage are spread over the callers; each
// butterfly's arithmetic is the host's.
template <class Sync>
AA_VORBIS_HD void imdct_window(const Setup& S, int f, const Wsf& X, float* y, const float* win, double* re,
                               double* im, int tid, int nthr, Sync sync) {
    const Hdr& H = S.h();
    const Mdct& m = *S.rec<Mdct>(H.mdct[f], 0);
    const int N = H.bs[f], M = N / 2, Q = M / 2;
    const double* pre_c = reinterpret_cast<const double*>(S.w + m.pre_c);
    const double* pre_s = reinterpret_cast<const double*>(S.w + m.pre_s);
    const double* post_c = reinterpret_cast<const double*>(S.w + m.post_c);
    const double* post_s = reinterpret_cast<const double*>(S.w + m.post_s);
    const double* fft_c = reinterpret_cast<const double*>(S.w + m.fft_c);
    const double* fft_s = reinterpret_cast<const double*>(S.w + m.fft_s);
    const int32_t* rev = S.w + m.rev;
    for (int k = tid; k < Q; k += nthr) {
        const double a = X[2 * k], b = X[M - 1 - 2 * k];
        const int r = rev[k] & (Q - 1);
        re[r] = a * pre_c[k] - b * pre_s[k];
        im[r] = a * pre_s[k] + b * pre_c[k];
    }
    sync();
    for (int len = 2; len <= Q; len <<= 1) {
        const int half = len / 2, step = Q / len;
        for (int t = tid; t < Q / 2; t += nthr) {
            const int j = t & (half - 1), a = (t / half) * len + j, b = a + half;
            const double wc = fft_c[j * step], ws = fft_s[j * step];
            const double tr = re[b] * wc - im[b] * ws, ti = re[b] * ws + im[b] * wc;
            re[b] = re[a] - tr;
            im[b] = im[a] - ti;
            re[a] += tr;
            im[a] += ti;
        }
        sync();
    }
    // u[2k] = Re(c_k), u[M-1-2k] = -Im(c_k), c = V * post twiddle; the three
    // output ranges with their signs, rounded to float, times the window
    for (int i = tid; i < N; i += nthr) {
        const int mm = i < M / 2 ? i + M / 2 : i < 3 * M / 2 ? 3 * M / 2 - 1 - i : i - 3 * M / 2;
        const int k = (mm & 1) ? (M - 1 - mm) / 2 : mm / 2;
        const double cr = re[k] * post_c[k] - im[k] * post_s[k];
        const double ci = re[k] * post_s[k] + im[k] * post_c[k];
        double u = (mm & 1) ? -ci : cr;
        if (i >= M / 2) u = -u;
        float v = (float)u;
        v *= win[i];
        y[i] = v;
    }
}

// One output sample of decode_all's accumulator: timeline index x of channel c,
// the stream's blocks (pk[0, np), in packet order) added onto zero inside their
// nonzero spans.  Block centres rise strictly, and a block covering x has its
// centre within bs1 / 2 of it.
AA_VORBIS_HD float ola_sample(const Packet* pk, int64_t np, int bs1, int c, int64_t x, const float* blk,
                              int64_t blk_floats) {
    int64_t lo = 0, hi = np;
    const int64_t h = bs1 / 2;
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (pk[mid].pos + pk[mid].n / 2 < x - h) lo = mid + 1;
        else hi = mid;
    }
    float acc = 0.f;
    for (int64_t k = lo; k < np; ++k) {
        const Packet& p = pk[k];
        if (p.pos + p.n / 2 > x + h) break;
        const int64_t i = x - p.pos;
        if (p.lstart < 0 || p.rend > p.n || i < p.lstart || i >= p.rend) continue;
        const int64_t at = p.blk_at + (int64_t)c * p.n + i;
        if (p.blk_at < 0 || at >= blk_floats) continue;
        acc += blk[at];
    }
    return acc;
}

// libswresample's float -> s16: av_clip_int16(lrint(x * 32768)), NaN -> -32768
AA_VORBIS_HD int16_t float_to_s16(float x) {
    const double v = __builtin_rint((double)x * 32768.0);
    if (v != v) return (int16_t)-32768;
    return (int16_t)(v < -32768.0 ? -32768.0 : v > 32767.0 ? 32767.0 : v);
}

struct NoSync {
    AA_VORBIS_HD void operator()() const {}
};

}  // namespace aa_vorbis
