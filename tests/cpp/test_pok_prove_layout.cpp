// Test-only: the workspace of frw_pok_prove_from_bytes_dev (frw_layout.h pok_prove_layout).
//   as a shared library (tests/test_pok_prove_abi.py): t_pok_prove walks the layout from a null base, so a pointer IS its offset;
//   as a program (the same test builds it with -fsanitize=address,undefined and runs it): main carves real memory of exactly the size
//   the layout reports for a few (logn, batch, in_flight), fills every piece to its last byte with a value of its own and reads all of
//   them back -- a piece that overlaps a neighbour reads the neighbour's value, one that reaches past the end trips the sanitizer.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "frw_layout.h"

namespace {
constexpr int PIECES = 20;
// every piece of the layout and its length in bytes, in layout order -> the number of pieces
int pieces(const frw::PokProveBufs &b, int logn, size_t batch, size_t k, size_t num_witness, const void *p[PIECES], size_t len[PIECES])
{
    const size_t n = (size_t)1 << logn;
    int i = 0;
    auto add = [&](const void *ptr, size_t bytes) { p[i] = ptr; len[i] = bytes; i++; };
    add(b.screen.sig, batch * n * 2); add(b.screen.pk, batch * n * 2); add(b.screen.hm, batch * n * 2);
    add(b.screen.nonce, batch * 40); add(b.screen.sig_status, batch * 4); add(b.screen.pk_status, batch * 4);
    add(b.index, batch * 4); add(b.block_sums, (batch + frw::POK_SCAN_BLOCK - 1) / frw::POK_SCAN_BLOCK * 4); add(b.count, 4);
    add(b.rs, batch * 64);
    add(b.witness, k * num_witness * 32); add(b.instance, k * (2 * n + 1) * 32);
    add(b.sig, k * n * 2); add(b.pk, k * n * 2); add(b.hm, k * n * 2);
    add(b.proofs, k * 384); add(b.wire, k * frw::POK_WIRE_STAGE);
    add(b.witness_status, k * 4); add(b.wire_status, k * 4); add(b.unsatisfied, k * 4);
    return i;
}
}  // namespace

extern "C" {
// out[2 i], out[2 i + 1]: offset and length of piece i (PIECES of them), then the Groth16 workspace's offset and length, then
// fixed_bytes and per_signature_bytes; returns .bytes
uint64_t t_pok_prove(int logn, uint64_t batch, uint64_t k, uint64_t num_witness, uint64_t groth16_bytes, uint64_t *out)
{
    const frw::PokProveBufs b = frw::pok_prove_layout(nullptr, logn, batch, k, num_witness, groth16_bytes);
    const void *p[PIECES];
    size_t len[PIECES];
    const int cnt = pieces(b, logn, batch, k, num_witness, p, len);
    for (int i = 0; i < cnt; i++) { out[2 * i] = (uint64_t)(uintptr_t)p[i]; out[2 * i + 1] = len[i]; }
    out[2 * cnt] = (uint64_t)(uintptr_t)b.groth16_ws; out[2 * cnt + 1] = b.groth16_bytes;
    out[2 * cnt + 2] = b.fixed_bytes; out[2 * cnt + 3] = b.per_signature_bytes;
    return b.bytes;
}
int t_pok_prove_pieces(void) { return PIECES; }
}

int main()
{
    struct Case { int logn; size_t batch, k; } cases[] = {{9, 1, 1}, {9, 9, 2}, {9, 9, 9}, {9, 1030, 3}, {10, 3, 2}, {10, 257, 1}, {9, 0, 1}};
    for (const Case &c : cases) {
        const size_t n = (size_t)1 << c.logn, W = 153 * n + (c.logn == 9 ? 50 : 52), g16 = 4096 * c.k + 256;
        const size_t bytes = frw::pok_prove_layout(nullptr, c.logn, c.batch, c.k, W, g16).bytes;
        unsigned char *mem = (unsigned char *)aligned_alloc(256, (bytes + 255) / 256 * 256);
        if (!mem) return 2;
        const frw::PokProveBufs b = frw::pok_prove_layout(mem, c.logn, c.batch, c.k, W, g16);
        const void *p[PIECES + 1];
        size_t len[PIECES + 1];
        int cnt = pieces(b, c.logn, c.batch, c.k, W, p, len);
        p[cnt] = b.groth16_ws; len[cnt] = b.groth16_bytes; cnt++;
        for (int i = 0; i < cnt; i++) {
            if ((uintptr_t)p[i] & 15) { printf("piece %d is not 16-byte aligned\n", i); return 1; }
            if ((const unsigned char *)p[i] + len[i] > mem + bytes) { printf("piece %d ends beyond the workspace\n", i); return 1; }
            memset((void *)p[i], i + 1, len[i]);
        }
        if (((uintptr_t)b.witness & 255) || ((uintptr_t)b.groth16_ws & 255)) { printf("witness / prover workspace not 256-byte aligned\n"); return 1; }
        for (int i = 0; i < cnt; i++)
            for (size_t j = 0; j < len[i]; j++)
                if (((const unsigned char *)p[i])[j] != i + 1) { printf("piece %d overlaps another at byte %zu\n", i, j); return 1; }
        free(mem);
        printf("logn %d batch %zu in flight %zu: %zu bytes, %d pieces disjoint\n", c.logn, c.batch, c.k, bytes, cnt);
    }
    printf("pok_prove_layout: clean\n");
    return 0;
}
