// Host harness around the run-time-field arithmetic of the witness kernels (falcon-r1cs_amd/csrc/frw_field.h), compiled with g++
// through tests/cpp/hip_host.  Protocol (tests/test_field_host.py): one operation per input line, hex integers,
//   consts p       ->  "ok one k1 k5 r2 ninv32 bits p"   or "refused"
//   u32 p x        ->  field_encode_u32(x)               (x < 2^32)
//   u160 p x       ->  field_encode_u160(x)              (x < 2^160)
// An inadmissible modulus answers "refused" to every operation.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "frw_field.h"

using namespace frw;

static void parse(const std::string &hex, uint32_t (&w)[10])
{
    for (int i = 0; i < 10; i++) w[i] = 0;
    int bit = 0;
    for (int i = (int)hex.size() - 1; i >= 0 && bit < 320; i--, bit += 4) {
        const char c = hex[i];
        const uint32_t v = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
        w[bit >> 5] |= v << (bit & 31);
    }
}

static void print_hex(const uint32_t *w, int n)
{
    bool started = false;
    for (int k = n - 1; k >= 0; k--) {
        if (!started && !w[k] && k) continue;
        std::printf(started ? "%08x" : "%x", w[k]);
        started = true;
    }
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, sp, sx;
        in >> op >> sp >> sx;
        if (op.empty()) continue;
        uint32_t pw[10], xw[10];
        parse(sp, pw);
        parse(sx, xw);
        FieldDerived d;
        uint64_t modulus[4];
        for (int j = 0; j < 4; j++) modulus[j] = (uint64_t)pw[2 * j] | ((uint64_t)pw[2 * j + 1] << 32);
        // a modulus of more than four limbs cannot be handed over at all: the caller of the C ABI is refused the same way
        if (pw[8] || pw[9] || !field_derive(modulus, &d)) {
            std::printf("refused\n");
            continue;
        }
        if (op == "consts") {
            std::printf("ok ");
            print_hex(d.fc.one, 8); std::printf(" ");
            print_hex(d.fc.k1, 8); std::printf(" ");
            print_hex(d.fc.k5, 8); std::printf(" ");
            print_hex(d.r2, 8);
            std::printf(" %x %x ", d.fc.ninv32, d.bits);
            print_hex(d.fc.p, 8);
            std::printf("\n");
        } else if (op == "u32") {
            uint32_t e[8];
            field_encode_u32(d.fc, xw[0], e);
            print_hex(e, 8);
            std::printf("\n");
        } else if (op == "u160") {
            const uint32_t x5[5] = {xw[0], xw[1], xw[2], xw[3], xw[4]};
            uint32_t e[8];
            field_encode_u160(d.fc, x5, e);
            print_hex(e, 8);
            std::printf("\n");
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}
