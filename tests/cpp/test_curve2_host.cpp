// Test-only: Fe2 and the group law of falcon-r1cs_amd/csrc/frw_curve2.h as a program of its own, which tests/test_curve2_host.py builds
// with -fsanitize=address,undefined (g++, through tests/cpp/hip_host) and runs.  Nothing of it is loaded into Python, nothing of the
// library is linked.  Every expectation comes from the arithmetic this file carries itself -- 256-bit integers, shift-and-add products
// modulo q, schoolbook Fq2 = Fq[u] / (u^2 - beta), the affine chord-and-tangent rule with a square-and-multiply inverse -- never from the
// header under test.  Over BN254's base field with beta = -1 and over Pallas' base field with beta = 5 (a non-residue there); on each the
// curve through a fixed point (x, y), b' := y^2 - x^3:
//   the descriptor          curve2_derive's refusals; b', one and beta in Montgomery form; beta = -1 recognised, and only it
//   Fe2                     product, square and inverse against the schoolbook rule; a a^-1 = 1
//   curve2_on_curve         points, infinity, an off-curve point, a component >= q, (0, y)
//   the exceptional cases   P + P through the mixed and the full addition, P + (-P), infinity + P, P + infinity, 2 infinity
//   mixed versus full       A + Q for an accumulator with ZZ != 1, both ways, against the rule
//   to-affine               of a doubled point against curve2_scalar_mul and the rule
//   curve2_scalar_mul       0, 1, 2, 2^256 - 1 and a mixed 255-bit pattern against the rule's double-and-add
// Inputs live in heap buffers of exactly their length.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "frw_curve2.h"

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

// ---- the reference: 256-bit integers modulo q < 2^255, and pairs of them ---------------------------------------------------------------
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
struct Q2 { U256 c0, c1; };
bool operator==(const Q2 &a, const Q2 &b) { return a.c0 == b.c0 && a.c1 == b.c1; }
struct Ref {
    U256 q, beta, rinv;                                            // rinv: 2^-256 mod q (set_rinv)
    Q2 b;
    U256 addm(const U256 &a, const U256 &c) const { const U256 s = add_raw(a, c); return cmp(s, q) >= 0 ? sub_raw(s, q) : s; }
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
    void set_rinv() { rinv = inv(mont(u(1))); }
    U256 mont(const U256 &a) const      // a 2^256 mod q
    {
        U256 r = a;
        for (int i = 0; i < 256; i++) r = addm(r, r);
        return r;
    }
    // schoolbook Fq2
    Q2 add2(const Q2 &a, const Q2 &c) const { return Q2{addm(a.c0, c.c0), addm(a.c1, c.c1)}; }
    Q2 sub2(const Q2 &a, const Q2 &c) const { return Q2{subm(a.c0, c.c0), subm(a.c1, c.c1)}; }
    Q2 mul2(const Q2 &a, const Q2 &c) const
    {
        return Q2{addm(mulm(a.c0, c.c0), mulm(beta, mulm(a.c1, c.c1))), addm(mulm(a.c0, c.c1), mulm(a.c1, c.c0))};
    }
    Q2 inv2(const Q2 &a) const
    {
        const U256 n = inv(subm(mulm(a.c0, a.c0), mulm(beta, mulm(a.c1, a.c1))));
        return Q2{mulm(a.c0, n), subm(u(0), mulm(a.c1, n))};
    }
};
const Q2 ZERO2{{{0, 0, 0, 0}}, {{0, 0, 0, 0}}};
bool is_zero2(const Q2 &a) { return is_zero(a.c0) && is_zero(a.c1); }
struct Pt { bool inf; Q2 x, y; };
const Pt INF{true, ZERO2, ZERO2};
bool same(const Pt &a, const Pt &b) { return a.inf == b.inf && (a.inf || (a.x == b.x && a.y == b.y)); }
Pt ref_neg(const Ref &f, const Pt &p) { return p.inf ? p : Pt{false, p.x, f.sub2(ZERO2, p.y)}; }
Pt ref_add(const Ref &f, const Pt &p, const Pt &s)
{
    if (p.inf) return s;
    if (s.inf) return p;
    Q2 lam;
    if (p.x == s.x) {
        if (is_zero2(f.add2(p.y, s.y))) return INF;
        const Q2 xx = f.mul2(p.x, p.x);
        lam = f.mul2(f.add2(f.add2(xx, xx), xx), f.inv2(f.add2(p.y, p.y)));
    } else {
        lam = f.mul2(f.sub2(s.y, p.y), f.inv2(f.sub2(s.x, p.x)));
    }
    const Q2 x = f.sub2(f.sub2(f.mul2(lam, lam), p.x), s.x);
    return Pt{false, x, f.sub2(f.mul2(lam, f.sub2(p.x, x)), p.y)};
}
Pt ref_mul(const Ref &f, const U256 &k, const Pt &p)
{
    Pt acc = INF;
    for (int i = 255; i >= 0; i--) {
        acc = ref_add(f, acc, acc);
        if (bit_of(k, i)) acc = ref_add(f, acc, p);
    }
    return acc;
}
bool ref_on_curve(const Ref &f, const Pt &p) { return p.inf || f.mul2(p.y, p.y) == f.add2(f.mul2(f.mul2(p.x, p.x), p.x), f.b); }

// ---- to and from the header's types, through heap buffers of exactly the length read ------------------------------------------------
frw::Fe2 to_fe2(const Ref &f, const Q2 &a)
{
    const U256 m0 = f.mont(a.c0), m1 = f.mont(a.c1);
    frw::Fe2 r;
    frw::field_words(m0.l, r.c0.l);
    frw::field_words(m1.l, r.c1.l);
    return r;
}
Q2 from_fe2(const Ref &f, const frw::Fe2 &a)
{
    U256 m0, m1;
    frw::field_limbs(a.c0.l, m0.l);
    frw::field_limbs(a.c1.l, m1.l);
    return Q2{f.mulm(m0, f.rinv), f.mulm(m1, f.rinv)};
}
frw::Affine2 to_affine_type(const Ref &f, const Pt &p)
{
    std::unique_ptr<uint64_t[]> buf(new uint64_t[16]);
    memset(buf.get(), 0, 128);
    if (!p.inf) {
        const U256 v[4] = {f.mont(p.x.c0), f.mont(p.x.c1), f.mont(p.y.c0), f.mont(p.y.c1)};
        for (int j = 0; j < 4; j++) memcpy(buf.get() + 4 * j, v[j].l, 32);
    }
    const frw::Affine2 a = frw::affine2_from_limbs(buf.get());
    // the device's load of the same 128 bytes
    std::unique_ptr<uint32_t[]> words(new uint32_t[32]);
    memcpy(words.get(), buf.get(), 128);
    const frw::Affine2 b = frw::affine2_load(words.get());
    CHECK(frw::fe2_equal(a.x, b.x) && frw::fe2_equal(a.y, b.y), "affine2_load differs from affine2_from_limbs");
    return a;
}
Pt from_affine_type(const Ref &f, const frw::Affine2 &a)
{
    std::unique_ptr<uint64_t[]> buf(new uint64_t[16]);
    frw::affine2_to_limbs(a, buf.get());
    U256 v[4];
    for (int j = 0; j < 4; j++) memcpy(v[j].l, buf.get() + 4 * j, 32);
    if (is_zero(v[0]) && is_zero(v[1]) && is_zero(v[2]) && is_zero(v[3])) return INF;
    return Pt{false, Q2{f.mulm(v[0], f.rinv), f.mulm(v[1], f.rinv)}, Q2{f.mulm(v[2], f.rinv), f.mulm(v[3], f.rinv)}};
}
const char *show(const Pt &p)
{
    static char buf[4][160];
    static int at = 0;
    char *s = buf[at++ & 3];
    if (p.inf) snprintf(s, 160, "infinity");
    else snprintf(s, 160, "(..%016llx + ..%016llx u, ..%016llx + ..%016llx u)", (unsigned long long)p.x.c0.l[0], (unsigned long long)p.x.c1.l[0],
                  (unsigned long long)p.y.c0.l[0], (unsigned long long)p.y.c1.l[0]);
    return s;
}

void run_field(const char *name, const U256 &q, const U256 &r, const U256 &beta, bool minus_one, const Q2 &gx, const Q2 &gy)
{
    using namespace frw;
    Ref f{q, beta, u(0), ZERO2};
    f.set_rinv();
    f.b = f.sub2(f.mul2(gy, gy), f.mul2(f.mul2(gx, gx), gx));
    const Pt g{false, gx, gy};
    CHECK(ref_on_curve(f, g) && !is_zero2(f.b), "%s: the test's own point", name);
    std::unique_ptr<uint64_t[]> bb(new uint64_t[8]);
    memcpy(bb.get(), f.b.c0.l, 32);
    memcpy(bb.get() + 4, f.b.c1.l, 32);
    Curve2Derived d;
    const char *refusal = curve2_derive(q.l, r.l, beta.l, bb.get(), &d);
    CHECK(refusal[0] == 0, "%s: curve2_derive refused: %s", name, refusal);
    if (refusal[0]) return;
    const Curve2Consts &cc = d.cc;
    const Fq2Consts &f2 = cc.f2;
    {
        U256 got;
        uint32_t w[8];
        for (int j = 0; j < 8; j++) w[j] = cc.b[j];
        field_limbs(w, got.l);
        CHECK(got == f.mont(f.b.c0), "%s: b'.c0 in Montgomery form", name);
        for (int j = 0; j < 8; j++) w[j] = cc.b[8 + j];
        field_limbs(w, got.l);
        CHECK(got == f.mont(f.b.c1), "%s: b'.c1 in Montgomery form", name);
        field_limbs(f2.fq.one, got.l);
        CHECK(got == f.mont(u(1)), "%s: one in Montgomery form", name);
        field_limbs(f2.beta, got.l);
        CHECK(got == f.mont(beta), "%s: beta in Montgomery form", name);
        CHECK((f2.beta_m1 != 0) == minus_one, "%s: beta = -1 recognised wrongly", name);
    }

    // Fe2 against the schoolbook rule
    {
        const Q2 vals[] = {gx, gy, f.b, Q2{u(0), u(5)}, Q2{u(7), u(0)}, Q2{sub_raw(q, u(1)), sub_raw(q, u(2))}, ZERO2, Q2{u(1), u(0)}};
        for (const Q2 &a : vals) {
            CHECK(from_fe2(f, fe2_square(f2, to_fe2(f, a))) == f.mul2(a, a), "%s: fe2_square", name);
            CHECK(from_fe2(f, fe2_neg(f2, to_fe2(f, a))) == f.sub2(ZERO2, a), "%s: fe2_neg", name);
            if (!is_zero2(a)) {
                const Fe2 ai = fe2_inverse(f2, to_fe2(f, a));
                CHECK(from_fe2(f, ai) == f.inv2(a), "%s: fe2_inverse", name);
                CHECK(fe2_equal(fe2_mul(f2, ai, to_fe2(f, a)), fe2_one(f2)), "%s: a a^-1 = 1", name);
            }
            for (const Q2 &c : vals) {
                CHECK(from_fe2(f, fe2_mul(f2, to_fe2(f, a), to_fe2(f, c))) == f.mul2(a, c), "%s: fe2_mul", name);
                CHECK(from_fe2(f, fe2_add(f2, to_fe2(f, a), to_fe2(f, c))) == f.add2(a, c), "%s: fe2_add", name);
                CHECK(from_fe2(f, fe2_sub(f2, to_fe2(f, a), to_fe2(f, c))) == f.sub2(a, c), "%s: fe2_sub", name);
            }
        }
        CHECK(fe2_is_zero(fe2_inverse(f2, fe2_zero())), "%s: 0^-1 = 0", name);
    }

    std::vector<Pt> mult(13, INF);                                 // mult[k] = k G
    for (int k = 1; k < 13; k++) mult[k] = ref_add(f, mult[k - 1], g);
    for (int k = 0; k < 13; k++) CHECK(ref_on_curve(f, mult[k]), "%s: %d G by the rule", name, k);
    auto A = [&](const Pt &p) { return to_affine_type(f, p); };
    auto back = [&](const Xyzz2 &p) { return from_affine_type(f, xyzz2_to_affine(f2, p)); };

    // curve2_on_curve
    for (int k = 0; k < 13; k++) CHECK(curve2_on_curve(cc, A(mult[k])), "%s: %d G is on the curve", name, k);
    {
        Pt off = mult[3];
        off.y.c1 = f.addm(off.y.c1, u(1));
        CHECK(!curve2_on_curve(cc, A(off)), "%s: an off-curve point passes", name);
        for (int comp = 0; comp < 4; comp++) {                     // v + q: the same residue, not canonical
            Affine2 big = A(mult[3]);
            Fe &e = comp == 0 ? big.x.c0 : comp == 1 ? big.x.c1 : comp == 2 ? big.y.c0 : big.y.c1;
            U256 x;
            field_limbs(e.l, x.l);
            x = add_raw(x, q);
            field_words(x.l, e.l);
            CHECK(!curve2_on_curve(cc, big), "%s: component %d >= q passes", name, comp);
        }
        Affine2 zero_x = A(mult[3]);
        zero_x.x = fe2_zero();
        CHECK(!curve2_on_curve(cc, zero_x), "%s: (0, y) passes", name);
    }

    // the exceptional cases
    for (int k = 1; k < 4; k++) {
        const Pt p = mult[k], twice = mult[2 * k];
        const Xyzz2 xp = xyzz2_from_affine(f2, A(p));
        CHECK(same(back(xyzz2_add_affine(f2, xp, A(p))), twice), "%s: P + P, mixed, k = %d: %s", name, k, show(back(xyzz2_add_affine(f2, xp, A(p)))));
        CHECK(same(back(xyzz2_add(f2, xp, xp)), twice), "%s: P + P, full, k = %d", name, k);
        CHECK(same(back(xyzz2_double(f2, xp)), twice), "%s: 2 P, k = %d", name, k);
        const Xyzz2 x2 = xyzz2_double(f2, xp);                     // an accumulator whose ZZ is not one
        CHECK(same(back(xyzz2_add_affine(f2, x2, A(twice))), mult[4 * k]), "%s: 2P + 2P, mixed, k = %d", name, k);
        CHECK(same(back(xyzz2_add(f2, x2, xyzz2_from_affine(f2, A(twice)))), mult[4 * k]), "%s: 2P + 2P, full, k = %d", name, k);
        CHECK(xyzz2_is_infinity(xyzz2_add_affine(f2, xp, affine2_neg(f2, A(p)))), "%s: P + (-P), mixed, k = %d", name, k);
        CHECK(xyzz2_is_infinity(xyzz2_add_affine(f2, x2, A(ref_neg(f, twice)))), "%s: 2P + (-2P), mixed, k = %d", name, k);
        CHECK(xyzz2_is_infinity(xyzz2_add(f2, x2, xyzz2_from_affine(f2, A(ref_neg(f, twice))))), "%s: 2P + (-2P), full, k = %d", name, k);
        CHECK(same(from_affine_type(f, affine2_neg(f2, A(p))), ref_neg(f, p)), "%s: -P, k = %d", name, k);
        CHECK(same(back(xyzz2_add_affine(f2, xyzz2_identity(), A(p))), p), "%s: infinity + P, mixed", name);
        CHECK(same(back(xyzz2_add(f2, xyzz2_identity(), x2)), twice), "%s: infinity + P, full", name);
        CHECK(same(back(xyzz2_add_affine(f2, x2, A(INF))), twice), "%s: P + infinity, mixed", name);
        CHECK(same(back(xyzz2_add(f2, x2, xyzz2_identity())), twice), "%s: P + infinity, full", name);
        Xyzz2 acc = xyzz2_add_affine(f2, xp, affine2_neg(f2, A(p)));    // a sum that passes through infinity goes on
        acc = xyzz2_add_affine(f2, acc, A(mult[5]));
        CHECK(same(back(acc), mult[5]), "%s: P - P + 5 G", name);
    }
    CHECK(xyzz2_is_infinity(xyzz2_double(f2, xyzz2_identity())), "%s: 2 infinity", name);
    CHECK(xyzz2_is_infinity(xyzz2_add(f2, xyzz2_identity(), xyzz2_identity())), "%s: infinity + infinity", name);
    CHECK(xyzz2_is_infinity(xyzz2_add_affine(f2, xyzz2_identity(), A(INF))), "%s: infinity + infinity, mixed", name);
    CHECK(same(back(xyzz2_identity()), INF), "%s: to-affine of infinity", name);

    // mixed versus full, against the rule
    for (int i = 1; i < 4; i++)
        for (int j = 1; j < 5; j++) {
            if (2 * i == j) continue;                              // (the equal case is above)
            const Xyzz2 acc = xyzz2_double(f2, xyzz2_from_affine(f2, A(mult[i])));
            const Pt mixed = back(xyzz2_add_affine(f2, acc, A(mult[j])));
            CHECK(same(mixed, mult[2 * i + j]), "%s: 2 (%d G) + %d G, mixed: %s", name, i, j, show(mixed));
        }
    for (int i = 1; i < 4; i++)
        for (int j = 1; j < 4; j++) {
            if (i == j) continue;
            const Xyzz2 a = xyzz2_double(f2, xyzz2_from_affine(f2, A(mult[i]))), c = xyzz2_double(f2, xyzz2_from_affine(f2, A(mult[j])));
            const Pt full = back(xyzz2_add(f2, a, c)), mixed = back(xyzz2_add_affine(f2, a, A(mult[2 * j])));
            CHECK(same(full, mult[2 * i + 2 * j]), "%s: 2 (%d G) + 2 (%d G), full: %s", name, i, j, show(full));
            CHECK(same(full, mixed), "%s: mixed and full differ at %d, %d", name, i, j);
        }

    // to-affine of a doubled point, curve2_scalar_mul
    {
        const Affine2 a = A(mult[7]);
        std::unique_ptr<uint64_t[]> two(new uint64_t[4]);
        two[0] = 2; two[1] = two[2] = two[3] = 0;
        const Pt doubled = back(xyzz2_double(f2, xyzz2_from_affine(f2, a)));
        CHECK(same(doubled, from_affine_type(f, curve2_scalar_mul(cc, a, two.get()))), "%s: to-affine of 2 P against curve2_scalar_mul", name);
        CHECK(same(doubled, ref_add(f, mult[7], mult[7])), "%s: to-affine of 2 P against the rule", name);
        const U256 ks[] = {u(0), u(1), u(2), U256{{~0ull, ~0ull, ~0ull, ~0ull}},
                           U256{{0x0123456789abcdefull, 0xfedcba9876543210ull, 0x8000000000000001ull, 0x7fffffffffffffffull}}};
        for (const U256 &k : ks) {
            std::unique_ptr<uint64_t[]> kb(new uint64_t[4]);
            memcpy(kb.get(), k.l, 32);
            const Pt got = from_affine_type(f, curve2_scalar_mul(cc, a, kb.get())), want = ref_mul(f, k, mult[7]);
            CHECK(same(got, want), "%s: curve2_scalar_mul by ..%016llx: %s, want %s", name, (unsigned long long)k.l[0], show(got), show(want));
            CHECK(curve2_on_curve(cc, to_affine_type(f, got)), "%s: the multiple is on the curve", name);
            CHECK(same(from_affine_type(f, curve2_scalar_mul(cc, A(INF), kb.get())), INF), "%s: k infinity", name);
        }
    }
}

void run_refusals()
{
    using namespace frw;
    const U256 q{{0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    const U256 r{{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    const U256 qm1 = sub_raw(q, u(1)), all{{~0ull, ~0ull, ~0ull, ~0ull}};
    Curve2Derived d;
    auto derive = [&](const U256 &qq, const U256 &rr, const U256 &beta, const U256 &b0, const U256 &b1) {
        std::unique_ptr<uint64_t[]> bb(new uint64_t[8]);
        memcpy(bb.get(), b0.l, 32);
        memcpy(bb.get() + 4, b1.l, 32);
        return curve2_derive(qq.l, rr.l, beta.l, bb.get(), &d)[0] == 0;
    };
    const U256 even = qm1, low{{0, 0, 1ull << 32, 0}}, high{{1, 0, 0, 1ull << 63}};
    CHECK(derive(q, r, qm1, u(3), u(4)), "a curve over BN254's Fq2 is refused");
    CHECK(d.cc.f2.beta_m1 == 1, "beta = q - 1 is not recognised");
    CHECK(derive(q, r, sub_raw(q, u(2)), u(3), u(4)) && d.cc.f2.beta_m1 == 0, "beta = q - 2");
    CHECK(derive(q, r, u(1), u(3), u(0)) && d.cc.f2.beta_m1 == 0, "beta = 1 (the caller's business), b' = (3, 0)");
    CHECK(derive(q, r, qm1, u(0), u(4)), "b' = (0, 4) is refused");
    for (const U256 &bad : {even, low, high, u(0)}) {
        CHECK(!derive(bad, r, u(5), u(3), u(4)), "an inadmissible base modulus passes");
        CHECK(!derive(q, bad, qm1, u(3), u(4)), "an inadmissible scalar modulus passes");
    }
    CHECK(!derive(q, r, u(0), u(3), u(4)), "beta = 0 passes");
    CHECK(!derive(q, r, q, u(3), u(4)), "beta = q passes");
    CHECK(!derive(q, r, all, u(3), u(4)), "beta = 2^256 - 1 passes");
    CHECK(!derive(q, r, qm1, u(0), u(0)), "b' = 0 passes");
    CHECK(!derive(q, r, qm1, q, u(4)), "b'.c0 = q passes");
    CHECK(!derive(q, r, qm1, u(3), q), "b'.c1 = q passes");
    CHECK(!derive(q, r, qm1, u(3), all), "b'.c1 = 2^256 - 1 passes");
}

}  // namespace

int main()
{
    const U256 bn_q{{0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    const U256 bn_r{{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
    run_field("bn254 Fq2, beta = -1", bn_q, bn_r, sub_raw(bn_q, u(1)), true, Q2{u(1), u(2)}, Q2{u(3), u(4)});
    // Pallas' base field, beta = 5 (its multiplicative generator: a non-residue); r: any admissible modulus
    const U256 pallas{{0x992d30ed00000001ull, 0x224698fc094cf91bull, 0, 0x4000000000000000ull}};
    run_field("pallas Fq2, beta = 5", pallas, bn_r, u(5), false, Q2{u(1), u(2)}, Q2{u(3), u(4)});
    run_refusals();
    printf("%d cases, %d failed\n", cases, failures);
    if (failures) return 1;
    printf("curve2_host: clean\n");
    return 0;
}
