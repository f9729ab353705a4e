// Test-only: the group law of falcon-r1cs_amd/csrc/frw_curve.h as a program of its own, which tests/test_curve_host.py builds with
// -fsanitize=address,undefined (g++, through tests/cpp/hip_host) and runs.  Nothing of it is loaded into Python, nothing of the library is
// linked.  Every expectation comes from the arithmetic this file carries itself -- 256-bit integers, shift-and-add products modulo q, the
// affine chord-and-tangent rule with a square-and-multiply inverse -- never from the header under test.  Over BN254's base field (b = 3,
// G = (1, 2)) and over the low-end modulus 2^160 + 7 as a bare field (the curve through (5, 7): b = 49 - 125):
//   the descriptor          curve_derive's refusals; b and one in Montgomery form
//   curve_on_curve          points, infinity, an off-curve point, a coordinate >= q, (0, y)
//   the exceptional cases   P + P through the mixed and the full addition, P + (-P), infinity + P, P + infinity, 2 infinity
//   mixed versus full       A + Q for an accumulator with ZZ != 1, both ways, against the rule
//   to-affine               of a doubled point against curve_scalar_mul and the rule; x x^-1 = 1
//   curve_scalar_mul        0, 1, 2, 2^256 - 1 and a mixed 255-bit pattern against the rule's double-and-add
// Inputs live in heap buffers of exactly their length.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "frw_curve.h"

namespace {
int failures = 0, cases = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        cases++;                                        \
        if (!(cond)) {                                  \
            printf("FAILED %s: ", #cond);               \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            failures++;                                 \
        }                                               \
    } while (0)

typedef unsigned __int128 u128;

// ---- the reference: 256-bit integers modulo q < 2^255 ------------------------------------------------------------------------------
struct U256 { uint64_t l[4]; };
bool operator==(const U256 &a, const U256 &b) { return !memcmp(a.l, b.l, 32); }
U256 u(uint64_t x) { return U256{{x, 0, 0, 0}}; }
bool is_zero(const U256 &a) { return !(a.l[0] | a.l[1] | a.l[2] | a.l[3]); }
int cmp(const U256 &a, const U256 &b)
{
    for (int i = 3; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i] ? -1 : 1;
    return 0;
}
U256 add_raw(const U256 &a, const U256 &b)
{
    U256 r;
    u128 c = 0;
    for (int i = 0; i < 4; i++) { c += (u128)a.l[i] + b.l[i]; r.l[i] = (uint64_t)c; c >>= 64; }
    return r;
}
U256 sub_raw(const U256 &a, const U256 &b)
{
    U256 r;
    uint64_t bw = 0;
    for (int i = 0; i < 4; i++) {
        const u128 x = (u128)a.l[i] - b.l[i] - bw;
        r.l[i] = (uint64_t)x;
        bw = (uint64_t)(x >> 64) & 1;
    }
    return r;
}
unsigned bit_of(const U256 &a, int i) { return (unsigned)(a.l[i >> 6] >> (i & 63)) & 1u; }
struct Ref {
    U256 q, b, rinv;                                               // rinv: 2^-256 mod q (set_rinv)
    U256 addm(const U256 &a, const U256 &c) const { const U256 s = add_raw(a, c); return cmp(s, q) >= 0 ? sub_raw(s, q) : s; }      // a, c < q < 2^255
    U256 subm(const U256 &a, const U256 &c) const { return cmp(a, c) >= 0 ? sub_raw(a, c) : sub_raw(add_raw(a, q), c); }
    U256 mulm(const U256 &a, const U256 &c) const
    {
        U256 r = u(0);
        for (int i = 255; i >= 0; i--) {
            r = addm(r, r);
            if (bit_of(c, i)) r = addm(r, a);
        }
        return r;
    }
    U256 powm(const U256 &a, const U256 &e) const
    {
        U256 r = u(1);
        for (int i = 255; i >= 0; i--) {
            r = mulm(r, r);
            if (bit_of(e, i)) r = mulm(r, a);
        }
        return r;
    }
    U256 inv(const U256 &a) const { return powm(a, sub_raw(q, u(2))); }
    void set_rinv() { rinv = u(1); rinv = inv(mont(u(1))); }
    U256 mont(const U256 &a) const      // a 2^256 mod q
    {
        U256 r = a;
        for (int i = 0; i < 256; i++) r = addm(r, r);
        return r;
    }
};
struct Pt { bool inf; U256 x, y; };
bool same(const Pt &a, const Pt &b) { return a.inf == b.inf && (a.inf || (a.x == b.x && a.y == b.y)); }
Pt ref_neg(const Ref &f, const Pt &p) { return p.inf ? p : Pt{false, p.x, f.subm(u(0), p.y)}; }
Pt ref_add(const Ref &f, const Pt &p, const Pt &s)
{
    if (p.inf) return s;
    if (s.inf) return p;
    U256 lam;
    if (p.x == s.x) {
        if (is_zero(f.addm(p.y, s.y))) return Pt{true, u(0), u(0)};
        const U256 xx = f.mulm(p.x, p.x);
        lam = f.mulm(f.addm(f.addm(xx, xx), xx), f.inv(f.addm(p.y, p.y)));
    } else {
        lam = f.mulm(f.subm(s.y, p.y), f.inv(f.subm(s.x, p.x)));
    }
    const U256 x = f.subm(f.subm(f.mulm(lam, lam), p.x), s.x);
    return Pt{false, x, f.subm(f.mulm(lam, f.subm(p.x, x)), p.y)};
}
Pt ref_mul(const Ref &f, const U256 &k, const Pt &p)
{
    Pt acc{true, u(0), u(0)};
    for (int i = 255; i >= 0; i--) {
        acc = ref_add(f, acc, acc);
        if (bit_of(k, i)) acc = ref_add(f, acc, p);
    }
    return acc;
}
bool ref_on_curve(const Ref &f, const Pt &p) { return p.inf || f.mulm(p.y, p.y) == f.addm(f.mulm(f.mulm(p.x, p.x), p.x), f.b); }

// ---- to and from the header's types, through heap buffers of exactly the length read ------------------------------------------------
frw::Affine to_affine_type(const Ref &f, const Pt &p)
{
    std::unique_ptr<uint64_t[]> buf(new uint64_t[8]);
    memset(buf.get(), 0, 64);
    if (!p.inf) {
        const U256 x = f.mont(p.x), y = f.mont(p.y);
        memcpy(buf.get(), x.l, 32);
        memcpy(buf.get() + 4, y.l, 32);
    }
    const frw::Affine a = frw::affine_from_limbs(buf.get());
    // the device's load of the same 64 bytes
    std::unique_ptr<uint32_t[]> words(new uint32_t[16]);
    memcpy(words.get(), buf.get(), 64);
    const frw::Affine b = frw::affine_load(words.get());
    CHECK(frw::fe_equal(a.x, b.x) && frw::fe_equal(a.y, b.y), "affine_load differs from affine_from_limbs");
    return a;
}
Pt from_affine_type(const Ref &f, const frw::Affine &a)
{
    std::unique_ptr<uint64_t[]> buf(new uint64_t[8]);
    frw::affine_to_limbs(a, buf.get());
    U256 x, y;
    memcpy(x.l, buf.get(), 32);
    memcpy(y.l, buf.get() + 4, 32);
    if (is_zero(x) && is_zero(y)) return Pt{true, u(0), u(0)};
    return Pt{false, f.mulm(x, f.rinv), f.mulm(y, f.rinv)};
}
const char *show(const Pt &p)
{
    static char buf[4][160];
    static int at = 0;
    char *s = buf[at++ & 3];
    if (p.inf) snprintf(s, 160, "infinity");
    else snprintf(s, 160, "(..%016llx, ..%016llx)", (unsigned long long)p.x.l[0], (unsigned long long)p.y.l[0]);
    return s;
}

void run_field(const char *name, const U256 &q, const U256 &r, const U256 &b, const Pt &g)
{
    using namespace frw;
    Ref f{q, b, u(0)};
    f.set_rinv();
    CHECK(ref_on_curve(f, g), "%s: the test's own generator", name);
    CurveDerived d;
    const char *refusal = curve_derive(q.l, r.l, b.l, &d);
    CHECK(refusal[0] == 0, "%s: curve_derive refused: %s", name, refusal);
    if (refusal[0]) return;
    const CurveConsts &cc = d.cc;
    const FieldConsts &fq = cc.fq;
    {
        U256 got;
        field_limbs(cc.b, got.l);
        CHECK(got == f.mont(b), "%s: b in Montgomery form", name);
        field_limbs(fq.one, got.l);
        CHECK(got == f.mont(u(1)), "%s: one in Montgomery form", name);
    }
    const Pt inf{true, u(0), u(0)};
    std::vector<Pt> mult(13, inf);                                 // mult[k] = k G
    for (int k = 1; k < 13; k++) mult[k] = ref_add(f, mult[k - 1], g);
    for (int k = 0; k < 13; k++) CHECK(ref_on_curve(f, mult[k]), "%s: %d G by the rule", name, k);
    auto A = [&](const Pt &p) { return to_affine_type(f, p); };
    auto back = [&](const Xyzz &p) { return from_affine_type(f, xyzz_to_affine(fq, p)); };

    // curve_on_curve
    for (int k = 0; k < 13; k++) CHECK(curve_on_curve(cc, A(mult[k])), "%s: %d G is on the curve", name, k);
    {
        Pt off = mult[3];
        off.y = f.addm(off.y, u(1));
        CHECK(!curve_on_curve(cc, A(off)), "%s: an off-curve point passes", name);
        Affine big = A(mult[3]);                                   // x + q: the same residue, not canonical
        U256 x;
        field_limbs(big.x.l, x.l);
        x = add_raw(x, q);
        field_words(x.l, big.x.l);
        CHECK(!curve_on_curve(cc, big), "%s: a coordinate >= q passes", name);
        Affine zero_x = A(mult[3]);
        zero_x.x = fe_zero();
        CHECK(!curve_on_curve(cc, zero_x), "%s: (0, y) passes", name);
    }

    // the exceptional cases
    for (int k = 1; k < 4; k++) {
        const Pt p = mult[k], twice = mult[2 * k];
        const Xyzz xp = xyzz_from_affine(fq, A(p));
        CHECK(same(back(xyzz_add_affine(fq, xp, A(p))), twice), "%s: P + P, mixed, k = %d: %s", name, k, show(back(xyzz_add_affine(fq, xp, A(p)))));
        CHECK(same(back(xyzz_add(fq, xp, xp)), twice), "%s: P + P, full, k = %d", name, k);
        CHECK(same(back(xyzz_double(fq, xp)), twice), "%s: 2 P, k = %d", name, k);
        // the same with an accumulator whose ZZ is not one: 2 P + 2 P where the operand arrives affine / as another representative
        const Xyzz x2 = xyzz_double(fq, xp);
        CHECK(same(back(xyzz_add_affine(fq, x2, A(twice))), mult[4 * k]), "%s: 2P + 2P, mixed, k = %d", name, k);
        CHECK(same(back(xyzz_add(fq, x2, xyzz_from_affine(fq, A(twice)))), mult[4 * k]), "%s: 2P + 2P, full, k = %d", name, k);
        CHECK(xyzz_is_infinity(xyzz_add_affine(fq, xp, affine_neg(fq, A(p)))), "%s: P + (-P), mixed, k = %d", name, k);
        CHECK(xyzz_is_infinity(xyzz_add_affine(fq, x2, A(ref_neg(f, twice)))), "%s: 2P + (-2P), mixed, k = %d", name, k);
        CHECK(xyzz_is_infinity(xyzz_add(fq, x2, xyzz_neg(fq, xyzz_from_affine(fq, A(twice))))), "%s: 2P + (-2P), full, k = %d", name, k);
        CHECK(same(from_affine_type(f, affine_neg(fq, A(p))), ref_neg(f, p)), "%s: -P, k = %d", name, k);
        CHECK(same(back(xyzz_add_affine(fq, xyzz_identity(), A(p))), p), "%s: infinity + P, mixed", name);
        CHECK(same(back(xyzz_add(fq, xyzz_identity(), x2)), twice), "%s: infinity + P, full", name);
        CHECK(same(back(xyzz_add_affine(fq, x2, A(inf))), twice), "%s: P + infinity, mixed", name);
        CHECK(same(back(xyzz_add(fq, x2, xyzz_identity())), twice), "%s: P + infinity, full", name);
        // a sum that passes through infinity goes on
        Xyzz acc = xyzz_add_affine(fq, xp, affine_neg(fq, A(p)));
        acc = xyzz_add_affine(fq, acc, A(mult[5]));
        CHECK(same(back(acc), mult[5]), "%s: P - P + 5 G", name);
    }
    CHECK(xyzz_is_infinity(xyzz_double(fq, xyzz_identity())), "%s: 2 infinity", name);
    CHECK(xyzz_is_infinity(xyzz_add(fq, xyzz_identity(), xyzz_identity())), "%s: infinity + infinity", name);
    CHECK(xyzz_is_infinity(xyzz_add_affine(fq, xyzz_identity(), A(inf))), "%s: infinity + infinity, mixed", name);
    CHECK(same(back(xyzz_identity()), inf), "%s: to-affine of infinity", name);

    // mixed versus full, against the rule
    for (int i = 1; i < 4; i++)
        for (int j = 1; j < 5; j++) {
            if (2 * i == j) continue;                              // (the equal case is above)
            const Xyzz acc = xyzz_double(fq, xyzz_from_affine(fq, A(mult[i])));
            const Pt mixed = back(xyzz_add_affine(fq, acc, A(mult[j])));
            CHECK(same(mixed, mult[2 * i + j]), "%s: 2 (%d G) + %d G, mixed: %s", name, i, j, show(mixed));
        }
    for (int i = 1; i < 4; i++)
        for (int j = 1; j < 4; j++) {
            if (i == j) continue;
            const Xyzz a = xyzz_double(fq, xyzz_from_affine(fq, A(mult[i]))), c = xyzz_double(fq, xyzz_from_affine(fq, A(mult[j])));
            const Pt full = back(xyzz_add(fq, a, c)), mixed = back(xyzz_add_affine(fq, a, A(mult[2 * j])));
            CHECK(same(full, mult[2 * i + 2 * j]), "%s: 2 (%d G) + 2 (%d G), full: %s", name, i, j, show(full));
            CHECK(same(full, mixed), "%s: mixed and full differ at %d, %d", name, i, j);
        }

    // the inverse, to-affine of a doubled point, curve_scalar_mul
    {
        const Affine a = A(mult[7]);
        const Fe prod = fe_mul(fq, a.x, fe_inverse(fq, a.x));
        CHECK(fe_equal(prod, fe_one(fq)), "%s: x x^-1 = 1", name);
        std::unique_ptr<uint64_t[]> two(new uint64_t[4]);
        two[0] = 2; two[1] = two[2] = two[3] = 0;
        const Pt doubled = back(xyzz_double(fq, xyzz_from_affine(fq, a)));
        CHECK(same(doubled, from_affine_type(f, curve_scalar_mul(cc, a, two.get()))), "%s: to-affine of 2 P against curve_scalar_mul", name);
        CHECK(same(doubled, ref_add(f, mult[7], mult[7])), "%s: to-affine of 2 P against the rule", name);
        const U256 ks[] = {u(0), u(1), u(2), U256{{~0ull, ~0ull, ~0ull, ~0ull}},
                           U256{{0x0123456789abcdefull, 0xfedcba9876543210ull, 0x8000000000000001ull, 0x7fffffffffffffffull}}};
        for (const U256 &k : ks) {
            std::unique_ptr<uint64_t[]> kb(new uint64_t[4]);
            memcpy(kb.get(), k.l, 32);
            const Pt got = from_affine_type(f, curve_scalar_mul(cc, a, kb.get())), want = ref_mul(f, k, mult[7]);
            CHECK(same(got, want), "%s: curve_scalar_mul by ..%016llx: %s, want %s", name, (unsigned long long)k.l[0], show(got), show(want));
            CHECK(curve_on_curve(cc, to_affine_type(f, got)), "%s: the multiple is on the curve", name);
            CHECK(same(from_affine_type(f, curve_scalar_mul(cc, A(inf), kb.get())), inf), "%s: k infinity", name);
        }
    }
}

void run_refusals()
{
    using namespace frw;
    const U256 q{{0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    const U256 r{{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    CurveDerived d;
    const U256 even = sub_raw(q, u(1)), low{{0, 0, 1ull << 32, 0}}, high{{1, 0, 0, 1ull << 63}};
    CHECK(curve_derive(q.l, r.l, u(3).l, &d)[0] == 0, "BN254 G1 is refused");
    for (const U256 &bad : {even, low, high, u(0)}) {
        CHECK(curve_derive(bad.l, r.l, u(3).l, &d)[0] != 0, "an inadmissible base modulus passes");
        CHECK(curve_derive(q.l, bad.l, u(3).l, &d)[0] != 0, "an inadmissible scalar modulus passes");
    }
    CHECK(curve_derive(q.l, r.l, u(0).l, &d)[0] != 0, "b = 0 passes");
    CHECK(curve_derive(q.l, r.l, q.l, &d)[0] != 0, "b = q passes");
    CHECK(curve_derive(q.l, r.l, U256{{~0ull, ~0ull, ~0ull, ~0ull}}.l, &d)[0] != 0, "b = 2^256 - 1 passes");
    CHECK(curve_derive(q.l, r.l, sub_raw(q, u(1)).l, &d)[0] == 0, "b = q - 1 is refused");
}

}  // namespace

int main()
{
    const U256 bn_q{{0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    const U256 bn_r{{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    run_field("bn254", bn_q, bn_r, u(3), Pt{false, u(1), u(2)});
    // 2^160 + 7 as a bare field: the curve through (5, 7) is y^2 = x^3 + (49 - 125); its order is nobody's business here (r: any
    // admissible modulus)
    const U256 low{{7, 0, 1ull << 32, 0}};
    run_field("2^160+7", low, bn_r, sub_raw(low, u(76)), Pt{false, u(5), u(7)});
    run_refusals();
    printf("%d cases, %d failed\n", cases, failures);
    if (failures) return 1;
    printf("curve_host: clean\n");
    return 0;
}
