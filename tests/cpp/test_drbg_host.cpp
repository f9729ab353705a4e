// Host harness around the factor draw (falcon-r1cs_amd/csrc/frw_drbg.h), compiled with g++ through tests/cpp/hip_host.  Protocol
// (tests/test_drbg_host.py): one operation per input line, hex integers,
//   reduce lo hi              ->  (lo + 2^256 hi) mod r                 (lo, hi < 2^256)
//   draw seed counter tag j   ->  x_j                                   (seed: 64 hex digits, byte 0 first)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <hip/hip_runtime.h>
static inline int hipFree(void *) { return 0; }          // (frw_verify.h's key handle, behind frw_rerand.h, frees its device parts; none here)
#include "frw_drbg.h"

extern "C" void frw_msm_free(frw_msm *) {}

using namespace frw;

static int nibble(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

static void parse(const std::string &hex, uint64_t (&w)[4])
{
    for (int i = 0; i < 4; i++) w[i] = 0;
    int bit = 0;
    for (int i = (int)hex.size() - 1; i >= 0 && bit < 256; i--, bit += 4) w[bit >> 6] |= (uint64_t)nibble(hex[i]) << (bit & 63);
}

static void print_hex(const uint64_t *w)
{
    std::printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, a, b, c, d;
        in >> op >> a >> b >> c >> d;
        if (op.empty()) continue;
        uint64_t out[4];
        if (op == "reduce") {
            uint64_t lo[4], hi[4];
            parse(a, lo);
            parse(b, hi);
            drbg::reduce512(lo, hi, out);
            print_hex(out);
        } else if (op == "draw" && a.size() == 64) {
            uint8_t seed[32];
            for (int k = 0; k < 32; k++) seed[k] = (uint8_t)(nibble(a[2 * k]) << 4 | nibble(a[2 * k + 1]));
            uint64_t counter[4], tag[4], j[4];
            parse(b, counter);
            parse(c, tag);
            parse(d, j);
            drbg::draw_one_host(seed, counter[0], (int)tag[0], j[0], out);
            print_hex(out);
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}
