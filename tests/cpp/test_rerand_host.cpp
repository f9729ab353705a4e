// Test-only: the host path of frw_rerand.h (the formulas frw_groth16_rerandomize and the device kernels share) and the workspace layout
// of the device calls (frw_layout.h rerand_layout), compiled for the host through the test-only shim.
//   as a shared library (tests/test_rerandomize_abi.py): t_rerand_layout walks the layout from a null base, so a pointer IS its offset;
//   t_rerand_factors runs the factors' arithmetic (reduction, zero test, inversion, product, the split by lambda) for Python to check;
//   as a program (tools/sanitize_cpu.sh builds it with -fsanitize=address,undefined): main re-randomises a few proofs made of the
//   generators -- equal operands in B' and C', opposite ones, points at infinity, a zero factor, in place -- checks them against the
//   one-lane formulas of frw_fq29.h used directly, and carves real memory by the layout, every piece written to its last byte.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static inline int hipFree(void *) { return 0; }          // (frw_verify.h's key handle frees its device parts; none here)
#include "frw_layout.h"
#include "frw_rerand.h"

extern "C" void frw_msm_free(frw_msm *) {}

using namespace frw;

extern "C" {
// out: offset and length of scalars, g1_points, g2_points, decoded, decode_status, encode_status; returns .bytes
uint64_t t_rerand_layout(uint64_t k, int wire, uint64_t *out)
{
    const RerandBufs b = rerand_layout(nullptr, k, wire != 0);
    const void *p[6] = {b.scalars, b.g1_points, b.g2_points, b.decoded, b.decode_status, b.encode_status};
    const uint64_t len[6] = {k * RERAND_SCALAR_BYTES, k * 2 * G1_BK_WORDS * 4, k * G2_BK_WORDS * 4, wire ? k * 384 : 0, wire ? k * 4 : 0, wire ? k * 4 : 0};
    for (int i = 0; i < 6; i++) { out[2 * i] = (uint64_t)(uintptr_t)p[i]; out[2 * i + 1] = len[i]; }
    return b.bytes;
}
// factors: r1 | r2 (8 words) -> the sixteen scalar words; returns the status
int t_rerand_factors(const uint64_t *factors, uint64_t *out) { return rerand::factors_prepare(factors, out); }
}

namespace {
int failures = 0;
void expect(bool ok, const char *what)
{
    if (!ok) { printf("FAILED: %s\n", what); failures++; }
}
void g1_limbs(const G1Xyzz &p, uint64_t *w) { rerand::store_ark<FqField>(g1_to_affine(p), w); }
void g2_limbs(const XyzzT<Fq2Field> &p, uint64_t *w) { rerand::store_ark<Fq2Field>(pt_to_affine(p), w); }
bool all_zero(const uint64_t *w, int n)
{
    uint64_t any = 0;
    for (int i = 0; i < n; i++) any |= w[i];
    return any == 0;
}
}  // namespace

int main()
{
    // the generators in ark-ff's limbs, and a few multiples by the plain formulas
    G1Affine29 g1;
    g1.x = fq_const(G1_GEN_X29); g1.y = fq_const(G1_GEN_Y29); g1.inf = false;
    AffineT<Fq2Field> g2;
    g2.x.c0 = fq_const(G2_GEN_X0_29); g2.x.c1 = fq_const(G2_GEN_X1_29); g2.y.c0 = fq_const(G2_GEN_Y0_29); g2.y.c1 = fq_const(G2_GEN_Y1_29); g2.inf = false;
    uint64_t G[12], H[24], G_2[12], H_2[24], G_neg[12], H_neg[24], H_3[24];
    rerand::store_ark<FqField>(g1, G);
    rerand::store_ark<Fq2Field>(g2, H);
    g1_limbs(g1_double(g1_from_affine(g1)), G_2);
    g2_limbs(pt_double(pt_from_affine(g2)), H_2);
    g2_limbs(pt_add_affine(pt_double(pt_from_affine(g2)), g2), H_3);
    {
        G1Affine29 n = g1;
        n.y = fq_neg<4>(g1.y);
        rerand::store_ark<FqField>(n, G_neg);
        AffineT<Fq2Field> m = g2;
        m.y = Fq2Field::neg<4>(g2.y);
        rerand::store_ark<Fq2Field>(m, H_neg);
    }
    const uint64_t one_one[8] = {1, 0, 0, 0, 1, 0, 0, 0};
    const uint64_t r_minus_one[4] = {0xffffffff00000000ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    uint64_t proof[48], out[48];
    // A = G, B = H, C = G, delta = H, r1 = r2 = 1: A' = A, B' = H + H (equal summands), C' = G + G (a doubling)
    memcpy(proof, G, 96); memcpy(proof + 12, H, 192); memcpy(proof + 36, G, 96);
    expect(rerand::rerandomize_one<Fq2Field>(proof, one_one, H, true, out) == 0, "status of the generators' proof");
    expect(!memcmp(out, G, 96) && !memcmp(out + 12, H_2, 192) && !memcmp(out + 36, G_2, 96), "A' = A, B' = 2 H, C' = 2 G");
    // the same without the subgroup ladders, and in place
    expect(rerand::rerandomize_one<Fq2Field>(proof, one_one, H, false, proof) == 0 && !memcmp(proof, out, 384), "vouched for, in place");
    // B = -delta, C = -A: both sums cancel
    memcpy(proof, G, 96); memcpy(proof + 12, H_neg, 192); memcpy(proof + 36, G_neg, 96);
    expect(rerand::rerandomize_one<Fq2Field>(proof, one_one, H, true, out) == 0, "status of the cancelling proof");
    expect(!memcmp(out, G, 96) && all_zero(out + 12, 24) && all_zero(out + 36, 12), "B' = O, C' = O");
    // r1 = r - 1 (its own inverse), r2 = 1, B = 2 H: A' = -A, B' = -(2 H) - H = -(3 H), checked through its x and the opposite y
    uint64_t f[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    memcpy(f, r_minus_one, 32);
    memcpy(proof, G, 96); memcpy(proof + 12, H_2, 192); memcpy(proof + 36, G, 96);
    expect(rerand::rerandomize_one<Fq2Field>(proof, f, H, true, out) == 0, "status with r1 = r - 1");
    expect(!memcmp(out, G_neg, 96), "A' = -A");
    expect(!memcmp(out + 12, H_3, 96) && memcmp(out + 24, H_3 + 12, 96), "B' = -3 H");
    // everything at infinity: A' = O, B' = r1 r2 delta, C' = O
    memset(proof, 0, sizeof(proof));
    expect(rerand::rerandomize_one<Fq2Field>(proof, one_one, H, true, out) == 0, "status of the proof at infinity");
    expect(all_zero(out, 12) && !memcmp(out + 12, H, 192) && all_zero(out + 36, 12), "O, delta, O");
    // refusals: a zero factor (r itself), a coordinate + q is not canonical, a point off its curve
    uint64_t zero_f[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    memcpy(zero_f, r_minus_one, 32);
    zero_f[0] += 1;
    memcpy(proof, G, 96); memcpy(proof + 12, H, 192); memcpy(proof + 36, G, 96);
    expect(rerand::rerandomize_one<Fq2Field>(proof, zero_f, H, true, out) == FRW_RERAND_ZERO_FACTOR && all_zero(out, 48), "r1 = r");
    proof[6] ^= 1;
    expect(rerand::rerandomize_one<Fq2Field>(proof, one_one, H, false, out) == -1 && all_zero(out, 48), "A off its curve");
    // the factors' arithmetic: k0 + lambda k1 = k, and (1 / r1) r1 = 1
    {
        uint64_t sc[rerand::SCALAR_WORDS], f2[8] = {0x123456789abcdef1ULL, 0xfedcba9876543210ULL, 0x0f1e2d3c4b5a6978ULL, 0x8000000000000000ULL, 7, 0, 0, 0};
        expect(rerand::factors_prepare(f2, sc) == 0, "a factor above r");
        const uint64_t lambda[4] = {0x00000000ffffffffULL, 0xac45a4010001a402ULL, 0, 0};
        uint64_t k1[4] = {sc[2], sc[3], 0, 0}, k0[4] = {sc[0], sc[1], 0, 0}, inv[4], prod[4], r1[4] = {f2[0], f2[1], f2[2], f2[3]};
        rerand::fr_mul(lambda, k1, inv);
        rerand::fr_add(inv, k0);                              // = 1 / r1
        rerand::fr_reduce(r1);
        rerand::fr_mul(inv, r1, prod);
        expect(rerand::u256_is_one(prod), "(k0 + lambda k1) r1 = 1");
        expect(!memcmp(sc + rerand::SC_R1, r1, 32), "r1 reduced");
    }
    // the layout: real memory of exactly the reported size, every piece filled to its last byte and read back
    for (int wire = 0; wire < 2; wire++)
        for (size_t k : {(size_t)1, (size_t)3, (size_t)65, (size_t)1030}) {
            const size_t bytes = rerand_layout(nullptr, k, wire).bytes;
            unsigned char *mem = (unsigned char *)aligned_alloc(16, (bytes + 15) / 16 * 16);
            if (!mem) return 2;
            const RerandBufs b = rerand_layout(mem, k, wire);
            void *p[6] = {b.scalars, b.g1_points, b.g2_points, b.decoded, b.decode_status, b.encode_status};
            const size_t len[6] = {k * RERAND_SCALAR_BYTES, k * 2 * G1_BK_WORDS * 4, k * G2_BK_WORDS * 4, k * 384, k * 4, k * 4};
            const int n = wire ? 6 : 3;
            for (int i = 0; i < n; i++) memset(p[i], 0x11 * (i + 1), len[i]);
            for (int i = 0; i < n; i++)
                for (size_t j = 0; j < len[i]; j += len[i] - 1 ? len[i] - 1 : 1)
                    expect(((unsigned char *)p[i])[j] == 0x11 * (i + 1) && (unsigned char *)p[i] + len[i] <= mem + bytes, "a piece of the layout");
            free(mem);
        }
    printf(failures ? "rerandomize host path: %d FAILED\n" : "rerandomize host path: clean\n", failures);
    return failures ? 1 : 0;
}
