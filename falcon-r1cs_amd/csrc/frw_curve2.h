// frw_curve2.h -- a short Weierstrass curve y^2 = x^3 + b' (a = 0) over a QUADRATIC extension Fq2 = Fq[u] / (u^2 - beta) of any four-limb
// field, all of it given at run time: what frw_curve2_* and frw_msmf2_* of include/frw.h stand on (frw_msm_field2.hip).  The G2 of a
// pairing-friendly curve is the case users have (BN254: beta = -1, b' = 3 / (9 + u)).  Plain inline code for the host and for the device,
// on frw_curve.h's Fe; tests/cpp/test_curve2_host.cpp builds it with g++ (through tests/cpp/hip_host) under the sanitizers.
//
// A curve is {base modulus q, scalar modulus r, beta, b' = (c0, c1)}.  q and r are admissible by field_derive's rule, 0 < beta < q,
// both components of b' are below q and b' != 0.  No curve's constants appear here or anywhere in csrc/.  That beta is a non-residue
// (so that Fq2 is a field), that q and r are prime, the group's order and the SUBGROUP are the CALLER'S business: the twist of a
// pairing-friendly curve has a cofactor, and nothing here checks that a point lies in the subgroup of order r.
//
// Fe2 = c0 + c1 u, each component in Montgomery form.  Costs in fe_mul:
//     product   3 (Karatsuba) and one more by beta unless beta = -1          square   2 for beta = -1 ((a0 + a1)(a0 - a1), 2 a0 a1), else 4
//     inverse   ONE fe_inverse through the norm: (a0 - a1 u) / (a0^2 - beta a1^2), and 4 products (5 with a general beta)
// beta = -1 is recognised by curve2_derive (beta == q - 1) and costs no product: Fq2Consts::beta_m1 is a launch-uniform word, the test on
// it a uniform branch around the ONE extra fe_mul.
//
// Points.  Affine, uint64_t[16] = x.c0, x.c1, y.c0, y.c1 (ark-ff's Fp2 order), each four little-endian limbs of v 2^256 mod q; ALL ZERO is
// the point at infinity (b' != 0).  Accumulators are XYZZ over Fe2, ZZ = 0 the point at infinity, and every addition is COMPLETE by the
// case analysis of frw_curve.h -- either operand infinite, equal operands (-> doubling of the accumulator), opposite operands
// (-> infinity) -- as rarely taken branches.  In Fe2 products: mixed addition 10 (2 of them squares), full addition 14, doubling 9.
#pragma once
#include <stdint.h>
#include "frw_curve.h"

namespace frw {

struct Fq2Consts {
    FieldConsts fq;       // the components' field, by value in a kernel argument
    uint32_t beta[8];     // beta 2^256 mod q
    uint32_t beta_m1;     // beta == q - 1: u^2 = -1, no product by beta
};
struct Curve2Consts {
    Fq2Consts f2;
    uint32_t b[16];       // b' as two Montgomery words, c0 then c1
};
struct Curve2Derived {
    FieldDerived q, r;
    Curve2Consts cc;
};

struct Fe2 { Fe c0, c1; };
struct Affine2 { Fe2 x, y; };               // all zero: infinity
struct Xyzz2 { Fe2 x, y, zz, zzz; };        // zz == 0: infinity

__host__ __device__ __forceinline__ bool fe2_is_zero(const Fe2 &a) { return fe_is_zero(a.c0) && fe_is_zero(a.c1); }
__host__ __device__ __forceinline__ bool fe2_equal(const Fe2 &a, const Fe2 &b) { return fe_equal(a.c0, b.c0) && fe_equal(a.c1, b.c1); }
__host__ __device__ __forceinline__ Fe2 fe2_zero() { return Fe2{fe_zero(), fe_zero()}; }
__host__ __device__ __forceinline__ Fe2 fe2_one(const Fq2Consts &f) { return Fe2{fe_one(f.fq), fe_zero()}; }
__host__ __device__ __forceinline__ Fe2 fe2_add(const Fq2Consts &f, const Fe2 &a, const Fe2 &b) { return Fe2{fe_add(f.fq, a.c0, b.c0), fe_add(f.fq, a.c1, b.c1)}; }
__host__ __device__ __forceinline__ Fe2 fe2_sub(const Fq2Consts &f, const Fe2 &a, const Fe2 &b) { return Fe2{fe_sub(f.fq, a.c0, b.c0), fe_sub(f.fq, a.c1, b.c1)}; }
__host__ __device__ __forceinline__ Fe2 fe2_neg(const Fq2Consts &f, const Fe2 &a) { return Fe2{fe_neg(f.fq, a.c0), fe_neg(f.fq, a.c1)}; }
__host__ __device__ __forceinline__ bool fe2_below_p(const Fq2Consts &f, const Fe2 &a) { return fe_below_p(f.fq, a.c0) && fe_below_p(f.fq, a.c1); }
// t0 + beta t1
__host__ __device__ __forceinline__ Fe fe_add_beta(const Fq2Consts &f, const Fe &t0, const Fe &t1)
{
    if (f.beta_m1) return fe_sub(f.fq, t0, t1);
    Fe bt;
#pragma unroll
    for (int j = 0; j < 8; j++) bt.l[j] = f.beta[j];
    return fe_add(f.fq, t0, fe_mul(f.fq, t1, bt));
}
// (a0 + a1 u)(b0 + b1 u) = a0 b0 + beta a1 b1 + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
__host__ __device__ __forceinline__ Fe2 fe2_mul(const Fq2Consts &f, const Fe2 &a, const Fe2 &b)
{
    const Fe t2 = fe_mul(f.fq, fe_add(f.fq, a.c0, a.c1), fe_add(f.fq, b.c0, b.c1));
    const Fe t0 = fe_mul(f.fq, a.c0, b.c0), t1 = fe_mul(f.fq, a.c1, b.c1);
    Fe2 r;
    r.c1 = fe_sub(f.fq, fe_sub(f.fq, t2, t0), t1);
    r.c0 = fe_add_beta(f, t0, t1);
    return r;
}
__host__ __device__ __forceinline__ Fe2 fe2_square(const Fq2Consts &f, const Fe2 &a)
{
    Fe2 r;
    if (f.beta_m1) {
        const Fe t = fe_mul(f.fq, a.c0, a.c1);
        r.c0 = fe_mul(f.fq, fe_add(f.fq, a.c0, a.c1), fe_sub(f.fq, a.c0, a.c1));
        r.c1 = fe_add(f.fq, t, t);
        return r;
    }
    const Fe s = fe_add(f.fq, a.c0, a.c1);
    const Fe t0 = fe_mul(f.fq, a.c0, a.c0), t1 = fe_mul(f.fq, a.c1, a.c1);
    r.c1 = fe_sub(f.fq, fe_sub(f.fq, fe_mul(f.fq, s, s), t0), t1);
    r.c0 = fe_add_beta(f, t0, t1);
    return r;
}
// 1 / a = (a0 - a1 u) / (a0^2 - beta a1^2): one inversion in Fq (0 -> 0)
__host__ __device__ __forceinline__ Fe2 fe2_inverse(const Fq2Consts &f, const Fe2 &a)
{
    const Fe n = fe_add_beta(f, fe_mul(f.fq, a.c0, a.c0), fe_neg(f.fq, fe_mul(f.fq, a.c1, a.c1)));
    const Fe ni = fe_inverse(f.fq, n);
    return Fe2{fe_mul(f.fq, a.c0, ni), fe_neg(f.fq, fe_mul(f.fq, a.c1, ni))};
}

__host__ __device__ __forceinline__ bool affine2_is_infinity(const Affine2 &p) { return fe2_is_zero(p.x) && fe2_is_zero(p.y); }
__host__ __device__ __forceinline__ Affine2 affine2_neg(const Fq2Consts &f, const Affine2 &p) { return Affine2{p.x, fe2_neg(f, p.y)}; }
__host__ __device__ __forceinline__ Xyzz2 xyzz2_identity() { return Xyzz2{fe2_zero(), fe2_zero(), fe2_zero(), fe2_zero()}; }
__host__ __device__ __forceinline__ bool xyzz2_is_infinity(const Xyzz2 &p) { return fe2_is_zero(p.zz); }
__host__ __device__ __forceinline__ Xyzz2 xyzz2_from_affine(const Fq2Consts &f, const Affine2 &p)
{
    if (affine2_is_infinity(p)) return xyzz2_identity();
    return Xyzz2{p.x, p.y, fe2_one(f), fe2_one(f)};
}

// 2 P (dbl-2008-s-1 with a = 0).  ZZ = 0 in gives ZZ = 0 out; so does Y = 0.
__host__ __device__ __forceinline__ Xyzz2 xyzz2_double(const Fq2Consts &f, const Xyzz2 &p)
{
    const Fe2 u = fe2_add(f, p.y, p.y), v = fe2_square(f, u), w = fe2_mul(f, u, v), s = fe2_mul(f, p.x, v);
    const Fe2 xx = fe2_square(f, p.x), m = fe2_add(f, fe2_add(f, xx, xx), xx);
    Xyzz2 r;
    r.x = fe2_sub(f, fe2_sub(f, fe2_square(f, m), s), s);
    r.y = fe2_sub(f, fe2_mul(f, m, fe2_sub(f, s, r.x)), fe2_mul(f, w, p.y));
    r.zz = fe2_mul(f, v, p.zz);
    r.zzz = fe2_mul(f, w, p.zzz);
    return r;
}
// A + P, P affine (madd-2008-s), complete
__host__ __device__ __forceinline__ Xyzz2 xyzz2_add_affine(const Fq2Consts &f, const Xyzz2 &a, const Affine2 &p)
{
    if (affine2_is_infinity(p)) return a;
    if (xyzz2_is_infinity(a)) return Xyzz2{p.x, p.y, fe2_one(f), fe2_one(f)};
    const Fe2 pd = fe2_sub(f, fe2_mul(f, p.x, a.zz), a.x), rd = fe2_sub(f, fe2_mul(f, p.y, a.zzz), a.y);
    if (fe2_is_zero(pd)) {                                         // the same x: the same point, or its negative
        if (fe2_is_zero(rd)) return xyzz2_double(f, a);
        return xyzz2_identity();
    }
    Xyzz2 r;
    const Fe2 pp = fe2_square(f, pd), q = fe2_mul(f, a.x, pp), ppp = fe2_mul(f, pd, pp);
    r.zz = fe2_mul(f, a.zz, pp);
    r.zzz = fe2_mul(f, a.zzz, ppp);
    const Fe2 t = fe2_mul(f, a.y, ppp);
    r.x = fe2_sub(f, fe2_sub(f, fe2_sub(f, fe2_square(f, rd), ppp), q), q);
    r.y = fe2_sub(f, fe2_mul(f, rd, fe2_sub(f, q, r.x)), t);
    return r;
}
// A + B (add-2008-s), complete
__host__ __device__ __forceinline__ Xyzz2 xyzz2_add(const Fq2Consts &f, const Xyzz2 &a, const Xyzz2 &b)
{
    if (xyzz2_is_infinity(b)) return a;
    if (xyzz2_is_infinity(a)) return b;
    const Fe2 u1 = fe2_mul(f, a.x, b.zz), s1 = fe2_mul(f, a.y, b.zzz);
    const Fe2 pd = fe2_sub(f, fe2_mul(f, b.x, a.zz), u1), rd = fe2_sub(f, fe2_mul(f, b.y, a.zzz), s1);
    if (fe2_is_zero(pd)) {
        if (fe2_is_zero(rd)) return xyzz2_double(f, a);
        return xyzz2_identity();
    }
    Xyzz2 r;
    const Fe2 pp = fe2_square(f, pd), ppp = fe2_mul(f, pd, pp), q = fe2_mul(f, u1, pp);
    r.x = fe2_sub(f, fe2_sub(f, fe2_sub(f, fe2_square(f, rd), ppp), q), q);
    r.y = fe2_sub(f, fe2_mul(f, rd, fe2_sub(f, q, r.x)), fe2_mul(f, s1, ppp));
    r.zz = fe2_mul(f, fe2_mul(f, a.zz, b.zz), pp);
    r.zzz = fe2_mul(f, fe2_mul(f, a.zzz, b.zzz), ppp);
    return r;
}
// the unique affine point: 1 / Z = ZZ / ZZZ, x = X / Z^2, y = Y / ZZZ -- one inversion in Fq2, so one in Fq
__host__ __device__ __forceinline__ Affine2 xyzz2_to_affine(const Fq2Consts &f, const Xyzz2 &p)
{
    if (xyzz2_is_infinity(p)) return Affine2{fe2_zero(), fe2_zero()};
    const Fe2 izzz = fe2_inverse(f, p.zzz), iz = fe2_mul(f, izzz, p.zz);
    return Affine2{fe2_mul(f, p.x, fe2_square(f, iz)), fe2_mul(f, p.y, izzz)};
}

// components below q and y^2 = x^3 + b', or all zero
__host__ __device__ __forceinline__ bool curve2_on_curve(const Curve2Consts &c, const Affine2 &p)
{
    if (affine2_is_infinity(p)) return true;
    if (!fe2_below_p(c.f2, p.x) || !fe2_below_p(c.f2, p.y)) return false;
    Fe2 bb;
#pragma unroll
    for (int j = 0; j < 8; j++) { bb.c0.l[j] = c.b[j]; bb.c1.l[j] = c.b[8 + j]; }
    const Fe2 rhs = fe2_add(c.f2, fe2_mul(c.f2, fe2_square(c.f2, p.x), p.x), bb);
    return fe2_equal(fe2_square(c.f2, p.y), rhs);
}

__host__ __device__ __forceinline__ Fe2 fe2_load(const uint32_t *__restrict__ w)       // 16 words: c0 then c1
{
    const uint4 a = ((const uint4 *)w)[0], b = ((const uint4 *)w)[1], c = ((const uint4 *)w)[2], d = ((const uint4 *)w)[3];
    return Fe2{Fe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}}, Fe{{c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}}};
}
__host__ __device__ __forceinline__ Affine2 affine2_load(const uint32_t *__restrict__ w) { return Affine2{fe2_load(w), fe2_load(w + 16)}; }

// ---- host only -------------------------------------------------------------------------------------------------------------------
// The refusal, or the empty string and the constants.
inline const char *curve2_derive(const uint64_t q[4], const uint64_t r[4], const uint64_t beta[4], const uint64_t b[8], Curve2Derived *out)
{
    Curve2Derived d{};
    if (!field_derive(q, &d.q)) return "the base modulus is not admissible (odd, 2^160 < q < 2^255)";
    if (!field_derive(r, &d.r)) return "the scalar modulus is not admissible (odd, 2^160 < r < 2^255)";
    const FieldConsts &fq = d.q.fc;
    Fe bt, b0, b1;
    field_words(beta, bt.l);
    if (fe_is_zero(bt)) return "the non-residue is zero";
    if (!fe_below_p(fq, bt)) return "the non-residue is not below the base modulus";
    field_words(b, b0.l);
    field_words(b + 4, b1.l);
    if (fe_is_zero(b0) && fe_is_zero(b1)) return "b = 0: (0, 0) would be on the curve, and it stands for the point at infinity";
    if (!fe_below_p(fq, b0) || !fe_below_p(fq, b1)) return "a component of b is not below the base modulus";
    d.cc.f2.fq = fq;
    field_mul(fq, bt.l, d.q.r2, d.cc.f2.beta);
    Fe qm1;
    field_words(q, qm1.l);
    qm1.l[0] -= 1;                                                 // q is odd
    d.cc.f2.beta_m1 = fe_equal(bt, qm1) ? 1u : 0u;
    Fe m0, m1;
    field_mul(fq, b0.l, d.q.r2, m0.l);
    field_mul(fq, b1.l, d.q.r2, m1.l);
    for (int j = 0; j < 8; j++) { d.cc.b[j] = m0.l[j]; d.cc.b[8 + j] = m1.l[j]; }
    *out = d;
    return "";
}
inline Affine2 affine2_from_limbs(const uint64_t p[16])
{
    Affine2 a;
    field_words(p, a.x.c0.l);
    field_words(p + 4, a.x.c1.l);
    field_words(p + 8, a.y.c0.l);
    field_words(p + 12, a.y.c1.l);
    return a;
}
inline void affine2_to_limbs(const Affine2 &a, uint64_t p[16])
{
    field_limbs(a.x.c0.l, p);
    field_limbs(a.x.c1.l, p + 4);
    field_limbs(a.y.c0.l, p + 8);
    field_limbs(a.y.c1.l, p + 12);
}
// k P for ANY 256-bit integer k by plain double-and-add from the top bit: the reference of the tests and of frw_curve2_scalar_mul
inline Affine2 curve2_scalar_mul(const Curve2Consts &c, const Affine2 &p, const uint64_t k[4])
{
    Xyzz2 acc = xyzz2_identity();
    for (int bit = 255; bit >= 0; bit--) {
        acc = xyzz2_double(c.f2, acc);
        if ((k[bit >> 6] >> (bit & 63)) & 1u) acc = xyzz2_add_affine(c.f2, acc, p);
    }
    return xyzz2_to_affine(c.f2, acc);
}

}  // namespace frw
