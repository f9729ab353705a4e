// frw_curve.h -- a short Weierstrass curve y^2 = x^3 + b (a = 0) over ANY four-limb field, all of it given at run time: what
// frw_curve_* and frw_msmf_* of include/frw.h stand on (frw_msm_field.hip).  Plain inline code for the host and for the device;
// tests/cpp/test_curve_host.cpp builds it with g++ (through tests/cpp/hip_host) under the sanitizers.
//
// A curve is {base modulus q, scalar modulus r, b}.  q and r are each admissible by field_derive's rule (odd, 2^160 < . < 2^255), b is
// canonical with 0 < b < q.  No curve's constants appear here or anywhere in csrc/.  Primality of q and r, the group's order and
// that r is it are the CALLER'S business, as the modulus is in frw_field.h: the group law below is the chord-and-tangent rule over
// whatever ring q gives, and r is used for ONE thing only -- bringing a Montgomery-form scalar h 2^256 mod r back to the integer h.
// There is no subgroup check: BN254 G1, Pallas, Vesta and Grumpkin have cofactor 1; for any other curve it is the caller's.
//
// Points.  Affine, uint64_t[8] = x then y, each four little-endian limbs of v 2^256 mod q (ark-ff's Fp256); ALL ZERO is the point
// at infinity -- b != 0, so (0, 0) is never on the curve (frw_rows.h's convention).  Accumulators are XYZZ (x = X / ZZ, y = Y / ZZZ,
// ZZ^3 = ZZZ^2), ZZ = 0 the point at infinity -- no flag word: doubling a point with ZZ = 0 (or with Y = 0) gives ZZ = 0 by itself.
//
// Every addition is COMPLETE by case analysis -- either operand infinite, equal operands (-> doubling), opposite operands
// (-> infinity) -- as branches that are taken rarely, not as arithmetic on every addition: the bucket and fold kernels meet all three
// (equal bases with equal digits, P and -P in one bucket, the fold's running sum meeting itself when one bucket is populated).
// Costs in field products: mixed addition 10, full addition 14, doubling 9, to-affine one Fermat inversion
// (exponent q - 2 read from FieldConsts::p bit by bit in a uniform loop: ~255 squarings and as many products as q - 2 has bits set).
// Register arrays see compile-time indices only.
#pragma once
#include <stdint.h>
#include "frw_r1cs_field.h"

namespace frw {

struct CurveConsts {
    FieldConsts fq;       // the coordinates' field, by value in a kernel argument
    uint32_t b[8];        // b 2^256 mod q
};
struct CurveDerived {
    FieldDerived q, r;
    CurveConsts cc;
};

struct Fe { uint32_t l[8]; };
struct Affine { Fe x, y; };                 // all zero: infinity
struct Xyzz { Fe x, y, zz, zzz; };          // zz == 0: infinity

__host__ __device__ __forceinline__ bool fe_is_zero(const Fe &a)
{
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) any |= a.l[j];
    return any == 0;
}
__host__ __device__ __forceinline__ bool fe_equal(const Fe &a, const Fe &b)
{
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) any |= a.l[j] ^ b.l[j];
    return any == 0;
}
__host__ __device__ __forceinline__ Fe fe_zero() { return Fe{{0, 0, 0, 0, 0, 0, 0, 0}}; }
__host__ __device__ __forceinline__ Fe fe_mul(const FieldConsts &f, const Fe &a, const Fe &b) { Fe r; field_mul(f, a.l, b.l, r.l); return r; }
__host__ __device__ __forceinline__ Fe fe_add(const FieldConsts &f, const Fe &a, const Fe &b) { Fe r; field_add(f, a.l, b.l, r.l); return r; }
__host__ __device__ __forceinline__ Fe fe_sub(const FieldConsts &f, const Fe &a, const Fe &b) { Fe r; field_sub(f, a.l, b.l, r.l); return r; }
__host__ __device__ __forceinline__ Fe fe_neg(const FieldConsts &f, const Fe &a) { return fe_sub(f, fe_zero(), a); }      // (0 stays 0)
__host__ __device__ __forceinline__ Fe fe_one(const FieldConsts &f)
{
    Fe r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.l[j] = f.one[j];
    return r;
}
// a < q?  (what "canonical" means for a coordinate that came from outside)
__host__ __device__ __forceinline__ bool fe_below_p(const FieldConsts &f, const Fe &a)
{
    uint32_t bw = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) bw = (uint32_t)(((uint64_t)a.l[j] - f.p[j] - bw) >> 63);
    return bw != 0;
}
// a^(q - 2): the inverse for a prime q (0 -> 0).  The exponent's words are uniform; the bit loop is a loop, the word loop unrolled.
__host__ __device__ __forceinline__ Fe fe_inverse(const FieldConsts &f, const Fe &a)
{
    uint32_t e[8];
    uint32_t bw = 2;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)f.p[j] - bw;
        e[j] = (uint32_t)x;
        bw = (uint32_t)(x >> 63);
    }
    Fe acc = fe_one(f);
#pragma unroll
    for (int w = 7; w >= 0; w--) {
        const uint32_t word = e[w];
        for (int bit = 31; bit >= 0; bit--) {
            acc = fe_mul(f, acc, acc);
            if ((word >> bit) & 1u) acc = fe_mul(f, acc, a);
        }
    }
    return acc;
}

__host__ __device__ __forceinline__ bool affine_is_infinity(const Affine &p) { return fe_is_zero(p.x) && fe_is_zero(p.y); }
__host__ __device__ __forceinline__ Affine affine_neg(const FieldConsts &f, const Affine &p) { return Affine{p.x, fe_neg(f, p.y)}; }
__host__ __device__ __forceinline__ Xyzz xyzz_identity() { return Xyzz{fe_zero(), fe_zero(), fe_zero(), fe_zero()}; }
__host__ __device__ __forceinline__ bool xyzz_is_infinity(const Xyzz &p) { return fe_is_zero(p.zz); }
__host__ __device__ __forceinline__ Xyzz xyzz_neg(const FieldConsts &f, const Xyzz &p) { return Xyzz{p.x, fe_neg(f, p.y), p.zz, p.zzz}; }
__host__ __device__ __forceinline__ Xyzz xyzz_from_affine(const FieldConsts &f, const Affine &p)
{
    if (affine_is_infinity(p)) return xyzz_identity();
    return Xyzz{p.x, p.y, fe_one(f), fe_one(f)};
}

// 2 P (dbl-2008-s-1 with a = 0).  ZZ = 0 in gives ZZ = 0 out; so does Y = 0 (a point of order two doubles to infinity).
__host__ __device__ __forceinline__ Xyzz xyzz_double(const FieldConsts &f, const Xyzz &p)
{
    const Fe u = fe_add(f, p.y, p.y), v = fe_mul(f, u, u), w = fe_mul(f, u, v), s = fe_mul(f, p.x, v);
    const Fe xx = fe_mul(f, p.x, p.x), m = fe_add(f, fe_add(f, xx, xx), xx);
    Xyzz r;
    r.x = fe_sub(f, fe_sub(f, fe_mul(f, m, m), s), s);
    r.y = fe_sub(f, fe_mul(f, m, fe_sub(f, s, r.x)), fe_mul(f, w, p.y));
    r.zz = fe_mul(f, v, p.zz);
    r.zzz = fe_mul(f, w, p.zzz);
    return r;
}
// the tail of the full addition: P = U2 - U1 != 0, R = S2 - S1; (x, y) of the result, and PP, PPP for the caller's ZZ, ZZZ
__host__ __device__ __forceinline__ void xyzz_add_tail(const FieldConsts &f, const Fe &u1, const Fe &s1, const Fe &pd, const Fe &rd, Fe &x3, Fe &y3,
                                                       Fe &pp, Fe &ppp)
{
    pp = fe_mul(f, pd, pd);
    ppp = fe_mul(f, pd, pp);
    const Fe q = fe_mul(f, u1, pp);
    x3 = fe_sub(f, fe_sub(f, fe_sub(f, fe_mul(f, rd, rd), ppp), q), q);
    y3 = fe_sub(f, fe_mul(f, rd, fe_sub(f, q, x3)), fe_mul(f, s1, ppp));
}
// A + P, P affine (madd-2008-s), complete
__host__ __device__ __forceinline__ Xyzz xyzz_add_affine(const FieldConsts &f, const Xyzz &a, const Affine &p)
{
    if (affine_is_infinity(p)) return a;
    if (xyzz_is_infinity(a)) return Xyzz{p.x, p.y, fe_one(f), fe_one(f)};
    const Fe pd = fe_sub(f, fe_mul(f, p.x, a.zz), a.x), rd = fe_sub(f, fe_mul(f, p.y, a.zzz), a.y);
    if (fe_is_zero(pd)) {                                          // the same x: the same point, or its negative
        if (fe_is_zero(rd)) return xyzz_double(f, a);              // (of the accumulator, not of p: p's registers are free by now)
        return xyzz_identity();
    }
    // (written out, each operand's last use as early as it comes: this is the bucket kernel's loop body, and its registers set the occupancy)
    Xyzz r;
    const Fe pp = fe_mul(f, pd, pd), q = fe_mul(f, a.x, pp), ppp = fe_mul(f, pd, pp);
    r.zz = fe_mul(f, a.zz, pp);
    r.zzz = fe_mul(f, a.zzz, ppp);
    const Fe t = fe_mul(f, a.y, ppp);
    r.x = fe_sub(f, fe_sub(f, fe_sub(f, fe_mul(f, rd, rd), ppp), q), q);
    r.y = fe_sub(f, fe_mul(f, rd, fe_sub(f, q, r.x)), t);
    return r;
}
// A + B (add-2008-s), complete
__host__ __device__ __forceinline__ Xyzz xyzz_add(const FieldConsts &f, const Xyzz &a, const Xyzz &b)
{
    if (xyzz_is_infinity(b)) return a;
    if (xyzz_is_infinity(a)) return b;
    const Fe u1 = fe_mul(f, a.x, b.zz), s1 = fe_mul(f, a.y, b.zzz);
    const Fe pd = fe_sub(f, fe_mul(f, b.x, a.zz), u1), rd = fe_sub(f, fe_mul(f, b.y, a.zzz), s1);
    if (fe_is_zero(pd)) {
        if (fe_is_zero(rd)) return xyzz_double(f, a);
        return xyzz_identity();
    }
    Xyzz r;
    Fe pp, ppp;
    xyzz_add_tail(f, u1, s1, pd, rd, r.x, r.y, pp, ppp);
    r.zz = fe_mul(f, fe_mul(f, a.zz, b.zz), pp);
    r.zzz = fe_mul(f, fe_mul(f, a.zzz, b.zzz), ppp);
    return r;
}
// the unique affine point: 1 / Z = ZZ / ZZZ, x = X / Z^2, y = Y / ZZZ -- one inversion
__host__ __device__ __forceinline__ Affine xyzz_to_affine(const FieldConsts &f, const Xyzz &p)
{
    if (xyzz_is_infinity(p)) return Affine{fe_zero(), fe_zero()};
    const Fe izzz = fe_inverse(f, p.zzz), iz = fe_mul(f, izzz, p.zz);
    return Affine{fe_mul(f, p.x, fe_mul(f, iz, iz)), fe_mul(f, p.y, izzz)};
}

// coordinates below q and y^2 = x^3 + b, or all zero
__host__ __device__ __forceinline__ bool curve_on_curve(const CurveConsts &c, const Affine &p)
{
    if (affine_is_infinity(p)) return true;
    if (!fe_below_p(c.fq, p.x) || !fe_below_p(c.fq, p.y)) return false;
    Fe bb;
#pragma unroll
    for (int j = 0; j < 8; j++) bb.l[j] = c.b[j];
    const Fe rhs = fe_add(c.fq, fe_mul(c.fq, fe_mul(c.fq, p.x, p.x), p.x), bb);
    return fe_equal(fe_mul(c.fq, p.y, p.y), rhs);
}

__host__ __device__ __forceinline__ Affine affine_load(const uint32_t *__restrict__ w)
{
    const uint4 a = ((const uint4 *)w)[0], b = ((const uint4 *)w)[1], c = ((const uint4 *)w)[2], d = ((const uint4 *)w)[3];
    return Affine{Fe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}}, Fe{{c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}}};
}

// ---- host only -------------------------------------------------------------------------------------------------------------------
// The refusal, or the empty string and the constants.
inline const char *curve_derive(const uint64_t q[4], const uint64_t r[4], const uint64_t b[4], CurveDerived *out)
{
    CurveDerived d{};
    if (!field_derive(q, &d.q)) return "the base modulus is not admissible (odd, 2^160 < q < 2^255)";
    if (!field_derive(r, &d.r)) return "the scalar modulus is not admissible (odd, 2^160 < r < 2^255)";
    Fe bw;
    field_words(b, bw.l);
    if (fe_is_zero(bw)) return "b = 0: (0, 0) would be on the curve, and it stands for the point at infinity";
    if (!fe_below_p(d.q.fc, bw)) return "b is not below the base modulus";
    d.cc.fq = d.q.fc;
    field_mul(d.q.fc, bw.l, d.q.r2, d.cc.b);
    *out = d;
    return "";
}
inline Affine affine_from_limbs(const uint64_t p[8])
{
    Affine a;
    field_words(p, a.x.l);
    field_words(p + 4, a.y.l);
    return a;
}
inline void affine_to_limbs(const Affine &a, uint64_t p[8])
{
    field_limbs(a.x.l, p);
    field_limbs(a.y.l, p + 4);
}
// k P for ANY 256-bit integer k by plain double-and-add from the top bit: the reference of the tests and of frw_curve_scalar_mul
inline Affine curve_scalar_mul(const CurveConsts &c, const Affine &p, const uint64_t k[4])
{
    Xyzz acc = xyzz_identity();
    for (int bit = 255; bit >= 0; bit--) {
        acc = xyzz_double(c.fq, acc);
        if ((k[bit >> 6] >> (bit & 63)) & 1u) acc = xyzz_add_affine(c.fq, acc, p);
    }
    return xyzz_to_affine(c.fq, acc);
}

}  // namespace frw
