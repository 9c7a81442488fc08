// Stand-alone host run of the device FLAC decoder's core and indexer
// (csrc/aa_flac_core.h, csrc/aa_flac_index.h), for sanitizer builds:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//           tools/flac_core_check.cpp -o flac_core_check && ./flac_core_check STREAM...
//
// Each file is a FLAC stream, optionally followed by a second table source:
// "NAME" alone indexes and decodes NAME; "NAME@TABLE" decodes NAME's bytes
// through the table of the file TABLE (a damaged stream through its undamaged
// original's table, the case the indexer itself would refuse).  The workspace,
// outputs and coefficient array are exact-size heap blocks, so a store or load
// outside them is an ASan report.  Prints one checksum line per stream; exit
// status 0 unless a file cannot be read.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../audio-analysis_amd/csrc/aa_flac_index.h"

static bool slurp(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[1 << 14];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    using namespace aa_flac;
    std::vector<uint16_t> crc_tab(256);
    crc16_table(crc_tab.data(), 0, 1);
    for (int a = 1; a < argc; ++a) {
        std::string arg = argv[a], src = arg;
        const size_t sep = arg.find('@');
        if (sep != std::string::npos) {
            src = arg.substr(sep + 1);
            arg = arg.substr(0, sep);
        }
        std::vector<uint8_t> bytes, tbytes;
        if (!slurp(arg, bytes) || (src != arg && !slurp(src, tbytes))) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        const std::vector<uint8_t>& from = src != arg ? tbytes : bytes;
        // exact-size copy: a read past the stream's end is a heap overflow
        std::vector<uint8_t> exact(from.begin(), from.end());
        aa_flac_stream_info info{};
        int64_t n = 0;
        const char* why = "";
        int rc = index_stream(exact.data(), exact.size(), &info, nullptr, 0, &n, &why);
        std::vector<aa_flac_frame> tab((size_t)(rc == AA_OK ? n : 0));
        if (rc == AA_OK && n) rc = index_stream(exact.data(), exact.size(), &info, tab.data(), n, &n, &why);
        if (rc != AA_OK) {
            printf("%s: index %d (%s)\n", argv[a], rc, why);
            continue;
        }
        int64_t n_out = 0, most = 0;
        for (const aa_flac_frame& f : tab) {
            n_out = std::max<int64_t>(n_out, f.out_at + (int64_t)f.keep * f.channels);
            most = std::max<int64_t>(most, (int64_t)f.block * f.channels);
        }
        std::vector<uint8_t> data(bytes.begin(), bytes.end());
        std::vector<int32_t> i32((size_t)n_out), ws((size_t)most), coef(32);
        std::vector<int16_t> s16((size_t)n_out);
        uint64_t sum = 1469598103934665603ull;
        auto mix = [&sum](uint64_t v) { sum = (sum ^ v) * 1099511628211ull; };
        for (const aa_flac_frame& f : tab) {
            const Frame fr{f.offset, f.out_at, f.nbytes, f.block, f.keep, f.channels, f.bits};
            const int st = decode_frame(Buf{data.data(), data.size()}, fr, Ws{ws.data(), 1}, most, Ws{coef.data(), 1},
                                        crc_tab.data(), i32.data(), s16.data());
            mix((uint64_t)st);
            if (st == ST_OK)
                for (int64_t i = f.out_at; i < f.out_at + (int64_t)f.keep * f.channels; ++i)
                    mix((uint32_t)i32[(size_t)i]), mix((uint16_t)s16[(size_t)i]);
        }
        printf("%s: %lld frames, checksum %016llx\n", argv[a], (long long)tab.size(), (unsigned long long)sum);
    }
    return 0;
}
