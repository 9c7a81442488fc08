// aa_flac_index's body (include/aa.h): the frame table of a FLAC stream from
// one pass over its bytes, host code without a HIP call.  A header so that
// tools/flac_core_check.cpp compiles it stand-alone next to the core.
//
// A frame start is accepted only when everything about it is certain: the
// sync code and reserved fields, the header CRC-8, the coded number being the
// expected one, and the CRC-16 of the bytes since the previous start coming
// out zero (CRC of data followed by its own CRC).  The running CRC-16 is the
// pass's cost (sliced eight bytes at a time); it is what tells a sync pattern
// inside a frame's payload, or bytes between two frames, from a frame start
// without decoding anything.
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/aa.h"
#include "aa_flac_core.h"

namespace aa_flac {

struct Crc16x8 {
    uint16_t t[8][256];  // t[k][b]: CRC of byte b followed by k zero bytes
    Crc16x8() {
        crc16_table(t[0], 0, 1);
        for (int k = 1; k < 8; ++k)
            for (int b = 0; b < 256; ++b) t[k][b] = (uint16_t)((t[k - 1][b] << 8) ^ t[0][t[k - 1][b] >> 8]);
    }
    uint32_t update(uint32_t c, const uint8_t* d, size_t n) const {
        while (n >= 8) {
            c = t[7][d[0] ^ (c >> 8)] ^ t[6][d[1] ^ (c & 0xFF)] ^ t[5][d[2]] ^ t[4][d[3]] ^ t[3][d[4]] ^ t[2][d[5]] ^
                t[1][d[6]] ^ t[0][d[7]];
            d += 8;
            n -= 8;
        }
        for (; n; --n) c = ((c << 8) & 0xFFFF) ^ t[0][(c >> 8) ^ *d++];
        return c;
    }
};

// Metadata blocks exactly as aa_flac.cpp's parse_header reads them.
inline int index_metadata(const uint8_t* d, size_t len, aa_flac_stream_info* info, size_t* frames_at,
                          const char** why) {
    size_t pos = 0;
    if (len >= 10 && memcmp(d, "ID3", 3) == 0) {
        const size_t sz = ((size_t)(d[6] & 0x7f) << 21) | ((size_t)(d[7] & 0x7f) << 14) |
                          ((size_t)(d[8] & 0x7f) << 7) | (size_t)(d[9] & 0x7f);
        pos = 10 + sz + ((d[5] & 0x10) ? 10 : 0);
    }
    if (!(pos + 4 <= len && memcmp(d + pos, "fLaC", 4) == 0)) return *why = "not a FLAC stream", AA_ERR_INVALID;
    pos += 4;
    bool have_si = false, last = false;
    while (!last) {
        if (pos + 4 > len) return *why = "FLAC: truncated metadata", AA_ERR_INVALID;
        last = (d[pos] & 0x80) != 0;
        const int type = d[pos] & 0x7f;
        const size_t blen = ((size_t)d[pos + 1] << 16) | ((size_t)d[pos + 2] << 8) | d[pos + 3];
        pos += 4;
        if (pos + blen > len) return *why = "FLAC: truncated metadata block", AA_ERR_INVALID;
        if (type == 127) return *why = "FLAC: invalid metadata block type", AA_ERR_INVALID;
        if (type == 0) {
            if (blen < 34 || have_si) return *why = "FLAC: bad STREAMINFO", AA_ERR_INVALID;
            const uint8_t* s = d + pos;
            info->sample_rate = (int32_t)(((uint32_t)s[10] << 12) | ((uint32_t)s[11] << 4) | (s[12] >> 4));
            info->channels = ((s[12] >> 1) & 7) + 1;
            info->bits_per_sample = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
            info->total_frames = ((int64_t)(s[13] & 15) << 32) | ((int64_t)s[14] << 24) | ((int64_t)s[15] << 16) |
                                 ((int64_t)s[16] << 8) | s[17];
            have_si = true;
        }
        pos += blen;
    }
    if (!have_si) return *why = "FLAC: no STREAMINFO", AA_ERR_INVALID;
    if (info->bits_per_sample < 4) return *why = "FLAC: sample depth unsupported", AA_ERR_INVALID;
    *frames_at = pos;
    return AA_OK;
}

inline int index_stream(const uint8_t* d, size_t len, aa_flac_stream_info* info, aa_flac_frame* frames, int64_t cap,
                        int64_t* n_frames, const char** why) {
    static const Crc16x8 crc;
    size_t at = 0;
    int rc = index_metadata(d, len, info, &at, why);
    if (rc) return rc;
    const int64_t total = info->total_frames;
    size_t end = len;
    if (len >= at + 128 && memcmp(d + len - 128, "TAG", 3) == 0) end = len - 128;  // ID3v1
    const Buf buf{d, end};
    int64_t n = 0, done = 0;
    *n_frames = 0;
    if (at == end) {  // no frame at all
        if (total) return *why = "FLAC index: fewer samples than STREAMINFO states", AA_ERR_UNSUPPORTED;
        return AA_OK;
    }
    Header h;
    if (!parse_header(buf, at, end, h)) return *why = "FLAC index: no frame header after the metadata", AA_ERR_UNSUPPORTED;
    if (h.number != 0) return *why = "FLAC index: first frame not numbered 0", AA_ERR_UNSUPPORTED;
    const int variable = h.variable;
    for (;;) {
        const int nch = h.ch_code < 8 ? h.ch_code + 1 : 2;
        if (nch != info->channels || (h.bps_code != 0 && bps_of_code(h.bps_code) != info->bits_per_sample))
            return *why = "FLAC index: frame header at odds with STREAMINFO", AA_ERR_UNSUPPORTED;
        const int block = h.block;
        const uint64_t want = variable ? (uint64_t)(done + block) : (uint64_t)(n + 1);
        // the next start: running CRC-16 from `at`; zero at a valid header = a frame ended there
        size_t q = at + (size_t)h.len, fed = at;
        uint32_t c = 0;
        bool found = false;
        Header hn;
        while (q + 2 <= end) {
            const uint8_t* m = (const uint8_t*)memchr(d + q, 0xFF, end - q);
            if (!m) break;
            q = (size_t)(m - d);
            if (q + 2 <= end && (d[q + 1] & 0xFE) == 0xF8 && parse_header(buf, q, end, hn) && hn.number == want &&
                hn.variable == variable) {
                c = crc.update(c, d + fed, q - fed);
                fed = q;
                if (c == 0) {
                    found = true;
                    break;
                }
            }
            ++q;
        }
        size_t stop = q;
        if (!found) {
            stop = end;
            if (crc.update(c, d + fed, end - fed) != 0)
                return *why = "FLAC index: bytes after a frame that are no frame", AA_ERR_UNSUPPORTED;
        }
        if (stop - at > ((size_t)1 << 24)) return *why = "FLAC index: frame above 16 MiB", AA_ERR_UNSUPPORTED;
        int keep = block;
        if (total && done + block > total) keep = (int)(total - done);
        if (frames) {
            if (n < cap) {
                aa_flac_frame& f = frames[n];
                f.offset = (int64_t)at;
                f.out_at = done * nch;
                f.nbytes = (int32_t)(stop - at);
                f.block = block;
                f.keep = keep;
                f.channels = nch;
                f.bits = info->bits_per_sample;
                f.stream = 0;
            }
        }
        ++n;
        done += block;
        if (!found || (total && done >= total)) break;
        at = stop;
        h = hn;
    }
    *n_frames = n;
    if (total && done < total) return *why = "FLAC index: fewer samples than STREAMINFO states", AA_ERR_UNSUPPORTED;
    if (frames && n > cap) return *why = "aa_flac_index: table too small", AA_ERR_WORKSPACE;
    return AA_OK;
}

}  // namespace aa_flac
