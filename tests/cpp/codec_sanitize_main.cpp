// Stand-alone program for a sanitized build (g++ -fsanitize=address,undefined): the three per-item functions of frw_codec.h on every
// case of a catalogue dump that tests/test_codec_host.py writes, each input copied into a heap buffer of EXACTLY its length and each
// output into one of exactly its size, so that a read past sig_len, past the key or past the message's end, or a write past a row, is
// a report.  The verdicts (and the rows of accepted cases) are compared with the dump: exit status 0 only if all agree.
//
// The dump, little-endian: "FRWCODEC", uint32 count, then per case  uint8 kind (0 signature, 1 key, 2 hash), uint8 logn, uint8 ok,
// uint8 0, uint32 len, [40 nonce bytes for a hash], len input bytes, [N uint16 expected coefficients where ok].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "test_codec.cpp"

static bool take(FILE *f, void *dst, size_t n) { return n == 0 || std::fread(dst, 1, n, f) == n; }

template <class T> struct Heap {                      // exactly n elements, nothing behind them
    T *p;
    explicit Heap(size_t n) : p((T *)std::malloc(n * sizeof(T))) { if (n && !p) std::abort(); }
    ~Heap() { std::free(p); }
    Heap(const Heap &) = delete;
};

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s DUMP\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    char magic[8];
    uint32_t count = 0;
    if (!f || !take(f, magic, 8) || std::memcmp(magic, "FRWCODEC", 8) || !take(f, &count, 4)) { std::fprintf(stderr, "not a dump\n"); return 2; }
    int bad = 0;
    uint32_t done[3] = {0, 0, 0};
    for (uint32_t i = 0; i < count; i++) {
        uint8_t head[4];
        uint32_t len;
        if (!take(f, head, 4) || !take(f, &len, 4) || head[0] > 2) { std::fprintf(stderr, "case %u: truncated dump\n", i); return 2; }
        const int kind = head[0], logn = head[1], n = 1 << logn;
        const bool ok = head[2] != 0;
        Heap<uint8_t> nonce(40), in(len), nonce_out(40);
        Heap<uint16_t> out(n), out2(n);
        std::vector<uint16_t> want(ok ? n : 0);
        if ((kind == 2 && !take(f, nonce.p, 40)) || !take(f, in.p, len) || !take(f, want.data(), want.size() * 2)) {
            std::fprintf(stderr, "case %u: truncated dump\n", i);
            return 2;
        }
        bool got = true, same = true;
        if (kind == 0) {
            got = t_decode_signature(logn, in.p, len, out.p, nonce_out.p) != 0;
            same = (t_decode_signature(logn, in.p, len, out2.p, nullptr) != 0) == got;
            if (got) same = same && !std::memcmp(nonce_out.p, in.p + 1, 40) && !std::memcmp(out.p, out2.p, n * 2);
        } else if (kind == 1) {
            got = t_decode_public_key(logn, in.p, out.p) != 0;
        } else {
            t_hash_to_point(logn, nonce.p, in.p, 0, len, out.p);
        }
        if (got != ok || !same || (ok && std::memcmp(out.p, want.data(), n * 2))) {
            std::fprintf(stderr, "case %u (kind %d, logn %d, %u bytes): expected %s, got %s%s\n", i, kind, logn, len, ok ? "accepted" : "refused",
                         got ? "accepted" : "refused", got == ok ? ", other coefficients or nonce" : "");
            bad++;
        }
        done[kind]++;
    }
    std::fclose(f);
    std::printf("%u signatures, %u keys, %u hashes: %d mismatches\n", done[0], done[1], done[2], bad);
    return bad ? 1 : 0;
}
