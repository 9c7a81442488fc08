// FLAC frame decoder core (RFC 9639) as __host__ __device__ code: one call
// decodes one frame out of a byte buffer into interleaved samples.  It is the
// body of aa_flac_decode_device's kernel and of aa_flac_decode_frames_host's
// loop (csrc/aa_flac_gpu.hip), and compiles stand-alone with a plain C++
// compiler (tools/flac_core_check.cpp runs it under sanitizers).
//
// It is written apart from the host decoder (csrc/aa_flac.cpp), which is its
// oracle.  The rule it keeps for EVERY input: either the frame's samples are
// the host decoder's bit for bit and the status is AA_FLAC_OK, or the status
// is not OK.  The host decoder computes in wrapping 64-bit arithmetic; here
// residuals and samples are int32 and every sum is formed in int64 from int32
// terms (|coefficient| < 2^15, 32 of them: below 2^52, no wrap), so as long
// as every stored value fits int32 the two agree, and the first one that does
// not sets AA_FLAC_FALLBACK.  A subframe of more than 32 bits (the side
// channel of a 32-bit stream) falls back outright.  Streams of up to 24 bits
// that conform never fall back: their samples, residuals included, fit.
//
// Bounds: every load goes through load8 / load32, clamped to the buffer;
// every loop runs to the block size, to block * channels, or stops at the
// frame's last bit; every store is to ws[0, block * channels) (stride
// ws_step), coef[0, 32) (stride coef_step) or out[out_at, out_at + keep *
// channels).  The caller guarantees those ranges exist.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AA_FLAC_HD __host__ __device__ inline
#else
#define AA_FLAC_HD inline
#endif

namespace aa_flac {

enum { ST_OK = 0, ST_CRC = 1, ST_MALFORMED = 2, ST_FALLBACK = 3 };

// the fields of aa_flac_frame the core needs (include/aa.h)
struct Frame {
    int64_t offset, out_at;
    int32_t nbytes, block, keep, channels, bits;
};

struct Buf {
    const uint8_t* p;
    uint64_t n;
    AA_FLAC_HD uint32_t load8(uint64_t i) const { return i < n ? p[i] : 0u; }
    AA_FLAC_HD uint32_t load32(uint64_t i) const {  // big-endian, zero past the end
        if (i + 4 <= n) {  // one (unaligned) word load
            uint32_t v;
            __builtin_memcpy(&v, p + i, 4);
            return __builtin_bswap32(v);
        }
        return (load8(i) << 24) | (load8(i + 1) << 16) | (load8(i + 2) << 8) | load8(i + 3);
    }
};

// 64-bit window kept in registers: `have` valid bits at the top of `win`
// (the rest zero), refilled 32 bits at a time: whole big-endian words counted
// from the first byte after the frame header, so a refill is in general an
// unaligned word load (load32 goes through a 4-byte memcpy).
// The word after the window is loaded one refill ahead (`next`), so a refill's
// memory latency passes under the decoding of the 32 bits before it.
struct BitReader {
    Buf b;
    uint64_t pos, end;  // bit positions in the buffer; end: the frame's last bit + 1
    uint64_t win;
    uint32_t next;      // the word at bit pos + have
    int have;

    AA_FLAC_HD void start(const Buf& buf, uint64_t byte, uint64_t end_byte) {
        b = buf;
        pos = byte * 8;
        end = end_byte * 8;
        win = ((uint64_t)b.load32(byte) << 32) | b.load32(byte + 4);
        have = 64;
        next = b.load32(byte + 8);
    }
    AA_FLAC_HD void refill() {
        if (have <= 32) {
            win |= (uint64_t)next << (32 - have);
            have += 32;
            next = b.load32((pos + (uint64_t)have) >> 3);
        }
    }
    AA_FLAC_HD uint32_t get(int k) {  // k in [0, 32]
        if (k == 0) return 0;
        refill();
        const uint32_t v = (uint32_t)(win >> (64 - k));
        win = (win << (k - 1)) << 1;
        have -= k;
        pos += (uint64_t)k;
        return v;
    }
    AA_FLAC_HD int64_t get_signed(int k) {  // k in [0, 33]
        if (k == 0) return 0;
        uint64_t u;
        if (k > 32) {
            u = (uint64_t)get(k - 32) << 32;
            u |= get(32);
        } else {
            u = get(k);
        }
        return (int64_t)(u << (64 - k)) >> (64 - k);
    }
    // zeros before the next 1 bit (consumed); false when the frame ends first
    AA_FLAC_HD bool unary(uint32_t& q) {
        uint32_t z = 0;
        for (;;) {
            if (pos >= end) return false;
            refill();
            if (win == 0) {
                z += (uint32_t)have;
                pos += (uint64_t)have;
                have = 0;
                continue;
            }
            const int c = __builtin_clzll(win);
            z += (uint32_t)c;
            win = (win << c) << 1;
            have -= c + 1;
            pos += (uint64_t)c + 1;
            q = z;
            return true;
        }
    }
    AA_FLAC_HD bool overrun() const { return pos > end; }
};

AA_FLAC_HD uint32_t crc8(const Buf& b, uint64_t at, int n) {  // x^8 + x^2 + x + 1
    uint32_t c = 0;
    for (int i = 0; i < n; ++i) {
        c ^= b.load8(at + (uint64_t)i);
        for (int k = 0; k < 8; ++k) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
    }
    return c;
}

AA_FLAC_HD void crc16_table(uint16_t* t, int first, int step) {  // x^16 + x^15 + x^2 + 1
    for (int i = first; i < 256; i += step) {
        uint32_t c = (uint32_t)i << 8;
        for (int k = 0; k < 8; ++k) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
        t[i] = (uint16_t)c;
    }
}

AA_FLAC_HD uint32_t crc16(const Buf& b, const uint16_t* t, uint64_t at, uint64_t n) {
    uint32_t c = 0;
    uint64_t i = 0;
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = b.load32(at + i);
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ (w >> 24)];
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ ((w >> 16) & 0xFF)];
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ ((w >> 8) & 0xFF)];
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ (w & 0xFF)];
    }
    for (; i < n; ++i) c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ b.load8(at + i)];
    return c;
}

// A frame header (RFC 9639 section 9.1) with the host decoder's checks.
struct Header {
    int block, ch_code, bps_code, variable, len;  // len: bytes, CRC-8 included
    uint64_t number;                             // coded frame / sample number
};

AA_FLAC_HD bool parse_header(const Buf& b, uint64_t at, uint64_t end, Header& h) {
    if (at + 6 > end) return false;
    const uint32_t w = b.load32(at);
    if ((w >> 17) != 0x7FFC) return false;  // sync code and the reserved bit after it
    h.variable = (int)((w >> 16) & 1);
    const int bs_code = (int)((w >> 12) & 15), sr_code = (int)((w >> 8) & 15);
    h.ch_code = (int)((w >> 4) & 15);
    h.bps_code = (int)((w >> 1) & 7);
    if ((w & 1) || bs_code == 0 || sr_code == 15 || h.ch_code > 10 || h.bps_code == 3) return false;
    uint64_t p = at + 4;
    const uint32_t b0 = b.load8(p++);
    int extra = 0;
    while (extra < 8 && (b0 & (0x80u >> extra))) ++extra;
    if (extra == 1 || extra == 8) return false;
    uint64_t num = extra == 0 ? b0 : (b0 & (0x7Fu >> extra));
    for (int i = 1; i < extra; ++i) {
        const uint32_t c = b.load8(p++);
        if ((c & 0xC0) != 0x80) return false;
        num = (num << 6) | (c & 0x3F);
    }
    h.number = num;
    if (bs_code == 1) h.block = 192;
    else if (bs_code <= 5) h.block = 576 << (bs_code - 2);
    else if (bs_code == 6) h.block = (int)b.load8(p++) + 1;
    else if (bs_code == 7) { h.block = (int)((b.load8(p) << 8) | b.load8(p + 1)) + 1; p += 2; }
    else h.block = 256 << (bs_code - 8);
    if (sr_code == 12) p += 1;
    else if (sr_code == 13 || sr_code == 14) p += 2;
    if (p >= end) return false;
    if (crc8(b, at, (int)(p - at)) != b.load8(p)) return false;
    h.len = (int)(p + 1 - at);
    return true;
}

AA_FLAC_HD int bps_of_code(int code) {
    return code == 1 ? 8 : code == 2 ? 12 : code == 4 ? 16 : code == 5 ? 20 : code == 6 ? 24 : code == 7 ? 32 : 0;
}

struct Ws {  // a frame's int32 workspace: element i at p[i * step]
    int32_t* p;
    int64_t step;
    AA_FLAC_HD int32_t& operator[](int64_t i) const { return p[i * step]; }
};

AA_FLAC_HD int32_t narrow(int64_t v, bool& wide) {
    if (v != (int64_t)(int32_t)v) wide = true;
    return (int32_t)v;
}

// Partitioned Rice residual into s[order .. block)
AA_FLAC_HD int read_residual(BitReader& br, int block, int order, const Ws& s, bool& wide) {
    const int method = (int)br.get(2);
    if (method > 1) return ST_MALFORMED;
    const int pbits = method == 0 ? 4 : 5, escape = method == 0 ? 15 : 31;
    const int porder = (int)br.get(4);
    const int per = block >> porder;
    if ((per << porder) != block || per < order) return ST_MALFORMED;
    int i = order;
    for (int p = 0; p < (1 << porder); ++p) {
        const int cnt = per - (p == 0 ? order : 0);
        const int k = (int)br.get(pbits);
        if (k == escape) {
            const int nb = (int)br.get(5);
            for (int j = 0; j < cnt; ++j) {
                s[i++] = (int32_t)br.get_signed(nb);  // nb <= 31
                if (br.overrun()) return ST_MALFORMED;
            }
        } else {
            for (int j = 0; j < cnt; ++j) {
                uint32_t q;
                if (!br.unary(q)) return ST_MALFORMED;
                const uint64_t v = ((uint64_t)q << k) | br.get(k);
                if (v >> 32) wide = true;
                const uint32_t u = (uint32_t)v;
                s[i++] = (int32_t)((u >> 1) ^ (0u - (u & 1)));
            }
        }
        if (br.overrun()) return ST_MALFORMED;
    }
    return ST_OK;
}

// s[i] = residual + (sum c[j] * s[i - 1 - j] >> shift) for i in [ORDER, block),
// the last ORDER samples in registers; residuals are fetched eight ahead of
// the serial chain.  FIXED predictors are the same with constant coefficients.
template <int ORDER>
AA_FLAC_HD void restore(const Ws& s, const int32_t (&c)[ORDER], int block, int shift, bool& wide) {
    int32_t h[ORDER];  // h[j] = s[i - 1 - j]
#pragma unroll
    for (int j = 0; j < ORDER; ++j) h[j] = s[ORDER - 1 - j];
    auto step = [&](int32_t r) {
        int64_t acc = 0;
#pragma unroll
        for (int j = 0; j < ORDER; ++j) acc += (int64_t)c[j] * (int64_t)h[j];
        const int32_t v = narrow((int64_t)r + (acc >> shift), wide);
#pragma unroll
        for (int j = ORDER - 1; j > 0; --j) h[j] = h[j - 1];
        h[0] = v;
        return v;
    };
    int i = ORDER;
    for (; i + 8 <= block; i += 8) {
        int32_t r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = s[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = step(r[u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) s[i + u] = r[u];
    }
    for (; i < block; ++i) s[i] = step(s[i]);
}

template <int ORDER>
AA_FLAC_HD void restore_lpc(const Ws& s, const Ws& coef, int block, int shift, bool& wide) {
    int32_t c[ORDER];
#pragma unroll
    for (int j = 0; j < ORDER; ++j) c[j] = coef[j];
    restore<ORDER>(s, c, block, shift, wide);
}

// One subframe into s[0, block), predictor restored and wasted bits shifted in.
AA_FLAC_HD int read_subframe(BitReader& br, int block, int bps, const Ws& s, const Ws& coef, bool& wide) {
    if (br.get(1) != 0) return ST_MALFORMED;
    const int type = (int)br.get(6);
    int wasted = 0;
    if (br.get(1)) {
        uint32_t q;
        if (!br.unary(q)) return ST_MALFORMED;
        if (q >= (uint32_t)(bps - 1)) return ST_MALFORMED;  // wasted = q + 1 < bps
        wasted = (int)q + 1;
        bps -= wasted;
    }
    if (bps > 32) wide = true;  // 33-bit samples: beyond int32
    if (type == 0) {  // CONSTANT
        const int32_t v = (int32_t)br.get_signed(bps);
        for (int i = 0; i < block; ++i) s[i] = v;
    } else if (type == 1) {  // VERBATIM
        for (int i = 0; i < block; ++i) {
            s[i] = (int32_t)br.get_signed(bps);
            if (br.overrun()) return ST_MALFORMED;
        }
    } else if (type >= 8 && type <= 12) {  // FIXED, order 0-4
        const int order = type - 8;
        if (order > block) return ST_MALFORMED;
        for (int i = 0; i < order; ++i) s[i] = (int32_t)br.get_signed(bps);
        const int rc = read_residual(br, block, order, s, wide);
        if (rc) return rc;
        if (order == 1) {
            const int32_t c[1] = {1};
            restore<1>(s, c, block, 0, wide);
        } else if (order == 2) {
            const int32_t c[2] = {2, -1};
            restore<2>(s, c, block, 0, wide);
        } else if (order == 3) {
            const int32_t c[3] = {3, -3, 1};
            restore<3>(s, c, block, 0, wide);
        } else if (order == 4) {
            const int32_t c[4] = {4, -6, 4, -1};
            restore<4>(s, c, block, 0, wide);
        }
    } else if (type >= 32) {  // LPC, order 1-32
        const int order = type - 31;
        if (order > block) return ST_MALFORMED;
        for (int i = 0; i < order; ++i) s[i] = (int32_t)br.get_signed(bps);
        const int prec = (int)br.get(4) + 1;
        if (prec == 16) return ST_MALFORMED;
        const int shift = (int)br.get_signed(5);
        if (shift < 0) return ST_MALFORMED;
        for (int j = 0; j < order; ++j) coef[j] = (int32_t)br.get_signed(prec);
        const int rc = read_residual(br, block, order, s, wide);
        if (rc) return rc;
        switch (order) {  // the common orders keep coefficients and history in registers
#define AA_FLAC_LPC(N) case N: restore_lpc<N>(s, coef, block, shift, wide); break;
            AA_FLAC_LPC(1) AA_FLAC_LPC(2) AA_FLAC_LPC(3) AA_FLAC_LPC(4) AA_FLAC_LPC(5) AA_FLAC_LPC(6)
            AA_FLAC_LPC(7) AA_FLAC_LPC(8) AA_FLAC_LPC(9) AA_FLAC_LPC(10) AA_FLAC_LPC(11) AA_FLAC_LPC(12)
#undef AA_FLAC_LPC
            default:
                for (int i = order; i < block; ++i) {
                    int64_t acc = 0;
                    for (int j = 0; j < order; ++j) acc += (int64_t)coef[j] * (int64_t)s[i - 1 - j];
                    s[i] = narrow((int64_t)s[i] + (acc >> shift), wide);
                }
        }
    } else {
        return ST_MALFORMED;
    }
    if (br.overrun()) return ST_MALFORMED;
    if (wasted)
        for (int i = 0; i < block; ++i) s[i] = narrow((int64_t)((uint64_t)(int64_t)s[i] << wasted), wide);
    return ST_OK;
}

// Decode frame f of buf.  ws: ws_cap int32, of which block * channels are used
// (channel c's sample i at ws[c * block + i]); coef: 32 int32; crc_tab:
// crc16_table's 256 entries.
AA_FLAC_HD int decode_frame(const Buf& buf, const Frame& f, const Ws& ws, int64_t ws_cap, const Ws& coef,
                            const uint16_t* crc_tab, int32_t* out_i32, int16_t* out_s16) {
    if (f.offset < 0 || f.nbytes < 0 || (uint64_t)f.offset + (uint64_t)f.nbytes > buf.n || f.out_at < 0 ||
        f.channels < 1 || f.channels > 8 || f.bits < 4 || f.bits > 32 || f.block < 1 || f.block > 65536 ||
        f.keep < 0 || f.keep > f.block)
        return ST_MALFORMED;
    if ((int64_t)f.block * f.channels > ws_cap) return ST_FALLBACK;
    const uint64_t at = (uint64_t)f.offset, end = at + (uint64_t)f.nbytes;
    Header h;
    if (!parse_header(buf, at, end, h)) return ST_MALFORMED;
    const int nch = h.ch_code < 8 ? h.ch_code + 1 : 2;
    if (h.block != f.block || nch != f.channels || (h.bps_code != 0 && bps_of_code(h.bps_code) != f.bits))
        return ST_MALFORMED;
    const int block = f.block;
    BitReader br;
    br.start(buf, at + (uint64_t)h.len, end);
    bool wide = false;
    for (int c = 0; c < nch; ++c) {
        const bool side = (h.ch_code == 8 && c == 1) || (h.ch_code == 9 && c == 0) || (h.ch_code == 10 && c == 1);
        const Ws s{ws.p + (int64_t)c * block * ws.step, ws.step};
        const int rc = read_subframe(br, block, f.bits + (side ? 1 : 0), s, coef, wide);
        if (rc) return rc;
    }
    const uint64_t body_end = (br.pos + 7) >> 3;
    if (body_end + 2 != end) return ST_CRC;
    if (crc16(buf, crc_tab, at, body_end - at) != ((buf.load8(body_end) << 8) | buf.load8(body_end + 1))) return ST_CRC;
    if (wide) return ST_FALLBACK;
    // stereo decorrelation and the interleaved stores; every sample must fit
    // the stream's depth (a conforming one does)
    const int64_t lim = (int64_t)1 << (f.bits - 1);
    bool big = false;
    for (int i = 0; i < f.keep; ++i) {
        int64_t a = ws[i], b = nch > 1 ? (int64_t)ws[block + i] : 0;
        if (h.ch_code == 8) {
            b = a - b;
        } else if (h.ch_code == 9) {
            a = a + b;
        } else if (h.ch_code == 10) {
            const int64_t mid = a * 2 + (b & 1);
            a = (mid + b) >> 1;
            b = (mid - b) >> 1;
        }
        for (int c = 0; c < nch; ++c) {
            const int64_t v = c == 0 ? a : c == 1 ? b : (int64_t)ws[(int64_t)c * block + i];
            if (v < -lim || v >= lim) big = true;
            const int64_t o = f.out_at + (int64_t)i * nch + c;
            if (out_i32) out_i32[o] = (int32_t)v;
            if (out_s16) out_s16[o] = (int16_t)(f.bits <= 16 ? v * ((int64_t)1 << (16 - f.bits)) : v >> (f.bits - 16));
        }
    }
    return big ? ST_FALLBACK : ST_OK;
}

}  // namespace aa_flac
