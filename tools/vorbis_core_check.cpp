// Stand-alone host run of the device Vorbis decoder's index and core
// (csrc/aa_vorbis.cpp: aa_vorbis_index; csrc/aa_vorbis_core.h), for sanitizer
// builds:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//           tools/vorbis_core_check.cpp -o vorbis_core_check && ./vorbis_core_check STREAM...
//
// Each file is an Ogg Vorbis stream.  It is indexed (payload, packet table and
// flattened setup into exact-size heap blocks, so a store or load outside them
// is an ASan report), decoded through the core exactly as
// aa_vorbis_decode_packets_host does it (unpack into an interleaved slice of
// the table's stride, inverse MDCT and window, overlap-add), and compared bit
// for bit with aa_vorbis_decode, the host decoder compiled into this program.
// Prints one line per stream: its checksum, or the index's return code.  Exit
// status 0 unless a file cannot be read (2) or a stream decodes to other bits
// than the host decoder's (1).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#define AA_VORBIS_STANDALONE 1
namespace aa {
static std::string last_error;
static void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error = buf;
}
}  // namespace aa
#define AA_CHECK(cond, code, ...)         \
    do {                                  \
        if (!(cond)) {                    \
            ::aa::set_error(__VA_ARGS__); \
            return (code);                \
        }                                 \
    } while (0)

#include "../audio-analysis_amd/csrc/aa_vorbis.cpp"

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
    namespace core = aa_vorbis;
    using core::Wsf;
    constexpr int WG = AA_VORBIS_WG;
    int worst = 0;
    for (int a = 1; a < argc; ++a) {
        std::vector<uint8_t> bytes;
        if (!slurp(argv[a], bytes)) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        // exact-size copy: a read past the stream's end is a heap overflow
        std::vector<uint8_t> exact(bytes.begin(), bytes.end());
        aa_vorbis_stream st{};
        int64_t pb = 0, sb = 0;
        int rc = aa_vorbis_index(exact.data(), exact.size(), &st, nullptr, 0, &pb, nullptr, 0, nullptr, 0, &sb);
        if (rc != AA_ERR_WORKSPACE) {
            printf("%s: index %d (%s)\n", argv[a], rc, aa::last_error.c_str());
            continue;
        }
        std::vector<uint8_t> payload((size_t)pb);
        std::vector<aa_vorbis_packet> tab((size_t)st.n_packets);
        std::vector<int64_t> setup((size_t)sb / 8);  // (8-byte aligned)
        // (empty vectors: any non-null pointer, the sizes are zero)
        uint8_t none = 0;
        aa_vorbis_packet none_pk{};
        rc = aa_vorbis_index(exact.data(), exact.size(), &st, payload.empty() ? &none : payload.data(), pb, &pb,
                             tab.empty() ? &none_pk : tab.data(), (int64_t)tab.size(), setup.data(), sb, &sb);
        if (rc != AA_OK) {
            fprintf(stderr, "%s: the sized index call returned %d (%s)\n", argv[a], rc, aa::last_error.c_str());
            worst = 1;
            continue;
        }
        int64_t n_ref = 0;
        rc = aa_vorbis_decode(exact.data(), exact.size(), nullptr, 0, &n_ref);
        const int C = st.channels;
        std::vector<float> ref((size_t)(n_ref * C));
        float none_f = 0.f;
        if (rc == AA_OK)
            rc = aa_vorbis_decode(exact.data(), exact.size(), ref.empty() ? &none_f : ref.data(), n_ref, &n_ref);
        if (rc != AA_OK || n_ref != st.frames) {
            fprintf(stderr, "%s: host decoder %d, %lld frames against the index's %lld\n", argv[a], rc,
                    (long long)n_ref, (long long)st.frames);
            worst = 1;
            continue;
        }
        // the three phases in the device's layout
        const int32_t* S = reinterpret_cast<const int32_t*>(setup.data());
        const int64_t words = sb / 4, np = (int64_t)tab.size();
        int64_t stride = 1, blk_floats = 0;
        for (const aa_vorbis_packet& p : tab) {
            stride = std::max<int64_t>(stride, st.ws_need[p.blockflag ? 1 : 0]);
            blk_floats = std::max<int64_t>(blk_floats, p.blk_at + (int64_t)p.n * C);
        }
        const int64_t groups = (np + WG - 1) / WG;
        std::vector<float> slices((size_t)(groups * WG * stride)), blk((size_t)blk_floats);
        std::vector<int32_t> nz((size_t)np * core::MAX_CH), status((size_t)np);
        std::vector<double> re(2048), im(2048);
        const core::Packet* pk = reinterpret_cast<const core::Packet*>(tab.data());
        static_assert(sizeof(core::Packet) == sizeof(aa_vorbis_packet), "the core's view of the packet record");
        uint64_t sum = 1469598103934665603ull;
        auto mix = [&sum](uint64_t v) { sum = (sum ^ v) * 1099511628211ull; };
        for (int64_t p = 0; p < np; ++p) {
            const Wsf ws{slices.data() + (p / WG) * WG * stride + p % WG, WG};
            status[(size_t)p] = core::unpack_packet(payload.data(), payload.size(), pk[p], S, words, ws, stride,
                                              &nz[(size_t)p * core::MAX_CH]);
            mix((uint64_t)status[(size_t)p]);
            const core::Setup setup_view{S, words};
            for (int c = 0; c < C; ++c) {
                float* y = blk.data() + pk[p].blk_at + (int64_t)c * pk[p].n;
                if (status[(size_t)p] != core::ST_OK || !nz[(size_t)p * core::MAX_CH + c]) {
                    std::fill(y, y + pk[p].n, 0.f);
                    continue;
                }
                const core::Hdr& H = setup_view.h();
                const float* win = reinterpret_cast<const float*>(
                    S + (pk[p].blockflag ? H.win_long[pk[p].prev * 2 + pk[p].next] : H.win_short));
                const Wsf X{ws.p + ((int64_t)c * (pk[p].n / 2)) * WG, WG};
                core::imdct_window(setup_view, pk[p].blockflag, X, y, win, re.data(), im.data(), 0, 1, core::NoSync{});
            }
        }
        int64_t differ = 0;
        for (int64_t e = 0; e < st.frames * C; ++e) {
            const float v = core::ola_sample(pk, np, st.blocksize_1, (int)(e % C), st.s0 + e / C, blk.data(), blk_floats);
            uint32_t x, y;
            memcpy(&x, &v, 4);
            memcpy(&y, &ref[(size_t)e], 4);
            differ += x != y;
            mix(x);
            mix((uint16_t)core::float_to_s16(v));
        }
        if (differ) {
            fprintf(stderr, "%s: %lld samples differ from the host decoder's\n", argv[a], (long long)differ);
            worst = 1;
        }
        printf("%s: %lld packets, %lld frames, checksum %016llx\n", argv[a], (long long)np, (long long)st.frames,
               (unsigned long long)sum);
    }
    return worst;
}
