// frw_wire.h -- ark-serialize's wire format for BLS12-381 points (ark-serialize / ark-ec 0.3, short-Weierstrass affine points), host and
// device alike: the codec behind frw_groth16_proofs_to_wire / _from_wire, their _dev forms, frw_groth16_verify_wire_dev and the key
// functions (frw_wire.hip).  Restated from the crates' sources, "parity unpinned" (DESIGN.md lists what that means); include/frw.h has the
// format in full.  In short:
//   Fq     48 bytes, little-endian, the canonical integer (NOT ark-ff's x 2^384 limbs); a value >= q is malformed
//   Fq2    c0 then c1
//   flags  the top two bits of the last byte of the last field element written: bit 7 "y is the greater of y, -y", bit 6 infinity
//   greater: Fq by canonical integer; Fq2 by c1 first, then c0
//   compressed    x with flags (y = sqrt(x^3 + b), the greater root iff bit 7); infinity: x = 0, bit 6 set, bit 7 clear
//   uncompressed  x, then y with the infinity flag only; the curve equation is checked; infinity: x = y = 0, bit 6 set
// One encoding per point: both flags set, infinity with a non-zero coordinate and bit 7 in an uncompressed point are refused (ark 0.3 is
// laxer on the last two).  Subgroup membership is not the codec's business.
// Everything here is __host__ __device__ code over frw_fq29.h, so that the host and device entry points give the same bytes by construction.
#pragma once
#include <stdint.h>

#include "frw_fq29.h"
#include "frw_verify.h"

namespace frw {
namespace wire {

constexpr int COMPRESSED = 0, UNCOMPRESSED = 1;
__host__ __device__ constexpr size_t g1_bytes(int mode) { return mode == COMPRESSED ? 48 : 96; }
__host__ __device__ constexpr size_t g2_bytes(int mode) { return mode == COMPRESSED ? 96 : 192; }
__host__ __device__ constexpr size_t proof_bytes(int mode) { return 2 * g1_bytes(mode) + g2_bytes(mode); }
__host__ __device__ constexpr size_t vk_header_bytes(int mode) { return g1_bytes(mode) + 3 * g2_bytes(mode) + 8; }

// 2^812 mod q (a canonical integer -> x 2^406 by one product), 2^-1 x 2^406 mod q, (q - 1) / 2 in 32-bit words (and (q + 1) / 4 in
// fq_sqrt_candidate); tests/test_wire_codec.py re-derives all four
constexpr LimbsQ FQ29_R2 = {{0x15bef7aeu, 0x1031cd0eu, 0x02dd93e8u, 0x09226323u, 0x0e6e2cd2u, 0x11684daau, 0x1170e5dbu,
                             0x088e25b1u, 0x1b366399u, 0x1c536f47u, 0x0d1f9cbcu, 0x0278b67fu, 0x1ea66a2bu, 0x0000000cu}};
constexpr LimbsQ FQ29_HALF = {{0x01d4fdc2u, 0x15d00348u, 0x13894478u, 0x07acde62u, 0x09365b0au, 0x12c2df9bu, 0x0dc2d61eu,
                               0x1e7c2b7du, 0x1c48f65eu, 0x0d3f7602u, 0x1aad4478u, 0x13a0d636u, 0x198be187u, 0x00000004u}};
constexpr int SQRT_EXP_BITS = 379;
constexpr uint32_t Q_HALF32[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                                   0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};

// ---- bytes <-> 32-bit words (wire buffers come with no alignment promise) --------------------------------------------------------------
__host__ __device__ __forceinline__ void load_words(const uint8_t *p, uint32_t (&w)[12])
{
    if (((uintptr_t)p & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) w[k] = ((const uint32_t *)p)[k];
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++)
            w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
    }
}
__host__ __device__ __forceinline__ void store_words(const uint32_t (&w)[12], uint8_t *p)
{
    if (((uintptr_t)p & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) ((uint32_t *)p)[k] = w[k];
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            p[4 * k] = (uint8_t)w[k]; p[4 * k + 1] = (uint8_t)(w[k] >> 8); p[4 * k + 2] = (uint8_t)(w[k] >> 16); p[4 * k + 3] = (uint8_t)(w[k] >> 24);
        }
    }
}
__host__ __device__ __forceinline__ void zero_bytes(uint8_t *p, size_t n)
{
    for (size_t k = 0; k < n; k++) p[k] = 0;
}

// ---- canonical integers (twelve 32-bit words) ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool words_below_modulus(const uint32_t (&w)[12])
{
    bool below = false, decided = false;
#pragma unroll
    for (int k = 11; k >= 0; k--) {
        if (!decided && w[k] != Q32_[k]) { below = w[k] < Q32_[k]; decided = true; }
    }
    return below;
}
__host__ __device__ __forceinline__ bool words_zero(const uint32_t (&w)[12])
{
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) any |= w[k];
    return any == 0;
}
// y > -y for a canonical y: y > (q - 1) / 2
__host__ __device__ __forceinline__ bool words_greater(const uint32_t (&w)[12])
{
    bool greater = false, decided = false;
#pragma unroll
    for (int k = 11; k >= 0; k--) {
        if (!decided && w[k] != Q_HALF32[k]) { greater = w[k] > Q_HALF32[k]; decided = true; }
    }
    return greater;
}
// ark orders Fq2 by c1 first, then c0: y > -y is decided by c1 unless c1 = -c1, i.e. c1 = 0
__host__ __device__ __forceinline__ bool words2_greater(const uint32_t (&c0)[12], const uint32_t (&c1)[12])
{
    return words_zero(c1) ? words_greater(c0) : words_greater(c1);
}
// canonical integer -> x 2^406 (< 2 q), and back
__host__ __device__ __forceinline__ Fq29 fq_from_words(const uint32_t (&w)[12]) { return fq_mul(fq_unpack(w), fq_const(FQ29_R2)); }
__host__ __device__ __forceinline__ void fq_to_words(const Fq29 &a, uint32_t (&w)[12])
{
    Fq29 one = fq_zero();
    one.l[0] = 1;
    fq_pack(fq_canonical(fq_mul(a, one)), w);
}
// ark-ff's limbs (x 2^384, canonical) -> the canonical integer: one product with 2^22 (a 2^384 x 2^22 / 2^406 = a)
__host__ __device__ __forceinline__ void ark_to_words(const uint64_t *limbs, uint32_t (&w)[12])
{
    Fq29 c = fq_zero();
    c.l[0] = 1u << 22;
    fq_pack(fq_canonical(fq_mul(fq_unpack((const uint32_t *)limbs), c)), w);
}
__host__ __device__ __forceinline__ bool fq_equal(const Fq29 &a, const Fq29 &b)      // a < 2^10 q, b < 16 q
{
    return fq_is_zero(fq_sub<16>(a, b));
}
__host__ __device__ __forceinline__ Fq29 fq_four()
{
    const Fq29 one = fq_const(FQ29_ONE), two = fq_add(one, one);
    return fq_add(two, two);
}

// ---- square roots -----------------------------------------------------------------------------------------------------------------------------
// q = 3 (mod 4): a^((q + 1) / 4) squares to a or to -a.  The exponent is one constant for every lane: uniform control flow, one
// accumulator, ~379 squarings and ~229 products.  a < 2^10 q; the result < 2 q.  The caller tests the square.
__host__ __device__ inline Fq29 fq_sqrt_candidate(const Fq29 &a)
{
    constexpr uint32_t SQRT_EXP32[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                         0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
    Fq29 acc = fq_const(FQ29_ONE);
#pragma nounroll
    for (int bit = SQRT_EXP_BITS - 1; bit >= 0; bit--) {
        acc = fq_sqr(acc);
        if ((SQRT_EXP32[bit >> 5] >> (bit & 31)) & 1u) acc = fq_mul(acc, a);
    }
    return acc;
}
// A root of a = a0 + a1 u in Fq2 through the norm: with s^2 = a0^2 + a1^2 and t = (a0 + s) / 2, the root is r + a1 / (2 r) u where r^2 = t --
// or, when t is a non-residue, a1 / (2 r) + r u where r^2 = -t (the other choice of s has (a0 - s) / 2 = -a1^2 / (4 t), and -1 is a
// non-residue).  Two Fq roots and one inversion; the CALLER tests the square, which is the residue test for both roots at once.
// a1 = 0 takes s = a0 (s = -a0 would make t zero): the root is then sqrt(a0) or sqrt(-a0) u.  a0, a1: canonical.
__host__ __device__ inline Fq2_29 fq2_sqrt_candidate(const Fq29 &a0, const Fq29 &a1)
{
    uint64_t col[2 * NLQ];
    fq_mul2_cols(a0, a0, a1, a1, col);
    const Fq29 n = fq_reduce_cols(col);
    uint32_t a1_any = 0;
#pragma unroll
    for (int i = 0; i < NLQ; i++) a1_any |= a1.l[i];
    Fq29 s = fq_sqrt_candidate(n);
    if (a1_any == 0) s = a0;
    const Fq29 t = fq_mul(fq_add(a0, s), fq_const(FQ29_HALF));
    const Fq29 r = fq_sqrt_candidate(t);
    const bool direct = fq_equal(fq_sqr(r), t);
    const Fq29 other = fq_mul(fq_mul(a1, fq_const(FQ29_HALF)), fq_inv(r));        // (fq_inv(0) = 0: only a = 0 gets there)
    Fq2_29 x;
    x.c0 = direct ? r : other;
    x.c1 = direct ? other : r;
    return x;
}

// ---- G1 -----------------------------------------------------------------------------------------------------------------------------------------
// limbs: uint64_t[12], ark-ff's G1Affine (all zero = infinity); out: g1_bytes(mode).  false (and zero bytes) for limbs >= q.
__host__ __device__ inline bool g1_encode(const uint64_t *limbs, int mode, uint8_t *out)
{
    if (!verify::coordinates_canonical(limbs, 2)) { zero_bytes(out, g1_bytes(mode)); return false; }
    uint64_t any = 0;
    for (int k = 0; k < 12; k++) any |= limbs[k];
    uint32_t x[12], y[12];
    ark_to_words(limbs, x);
    ark_to_words(limbs + 6, y);
    if (mode == COMPRESSED) {
        x[11] |= any == 0 ? 0x40000000u : words_greater(y) ? 0x80000000u : 0u;
        store_words(x, out);
    } else {
        y[11] |= any == 0 ? 0x40000000u : 0u;
        store_words(x, out);
        store_words(y, out + 48);
    }
    return true;
}
// in: g1_bytes(mode); limbs: uint64_t[12].  false (and zero limbs) for every malformed case.
__host__ __device__ inline bool g1_decode(const uint8_t *in, int mode, uint64_t *limbs)
{
    for (int k = 0; k < 12; k++) limbs[k] = 0;
    uint32_t xw[12], yw[12];
    load_words(in, xw);
    uint32_t flags;
    if (mode == COMPRESSED) {
        flags = xw[11] >> 30;
        xw[11] &= 0x3fffffffu;
    } else {
        load_words(in + 48, yw);
        flags = yw[11] >> 30;
        yw[11] &= 0x3fffffffu;
        if ((flags & 2u) || !words_below_modulus(yw)) return false;
    }
    if (flags == 3u || !words_below_modulus(xw)) return false;
    if (flags & 1u) return words_zero(xw) && (mode == COMPRESSED || words_zero(yw));
    const Fq29 x = fq_from_words(xw);
    const Fq29 rhs = fq_add(fq_mul(fq_sqr(x), x), fq_four());
    Fq29 y;
    if (mode == COMPRESSED) {
        y = fq_sqrt_candidate(rhs);
        if (!fq_equal(fq_sqr(y), rhs)) return false;
        fq_to_words(y, yw);
        if (words_greater(yw) != ((flags & 2u) != 0)) y = fq_neg<4>(y);
    } else {
        y = fq_from_words(yw);
        if (!fq_equal(fq_sqr(y), rhs)) return false;
    }
    fq_to_ark(x, (uint32_t *)limbs);
    fq_to_ark(y, (uint32_t *)(limbs + 6));
    return true;
}

// ---- G2 -----------------------------------------------------------------------------------------------------------------------------------------
// limbs: uint64_t[24], x.c0 | x.c1 | y.c0 | y.c1; the flags sit in the last byte of the c1 written last
__host__ __device__ inline bool g2_encode(const uint64_t *limbs, int mode, uint8_t *out)
{
    if (!verify::coordinates_canonical(limbs, 4)) { zero_bytes(out, g2_bytes(mode)); return false; }
    uint64_t any = 0;
    for (int k = 0; k < 24; k++) any |= limbs[k];
    uint32_t x0[12], x1[12], y0[12], y1[12];
    ark_to_words(limbs, x0);
    ark_to_words(limbs + 6, x1);
    ark_to_words(limbs + 12, y0);
    ark_to_words(limbs + 18, y1);
    if (mode == COMPRESSED) {
        x1[11] |= any == 0 ? 0x40000000u : words2_greater(y0, y1) ? 0x80000000u : 0u;
        store_words(x0, out);
        store_words(x1, out + 48);
    } else {
        y1[11] |= any == 0 ? 0x40000000u : 0u;
        store_words(x0, out);
        store_words(x1, out + 48);
        store_words(y0, out + 96);
        store_words(y1, out + 144);
    }
    return true;
}
__host__ __device__ inline bool g2_decode(const uint8_t *in, int mode, uint64_t *limbs)
{
    for (int k = 0; k < 24; k++) limbs[k] = 0;
    uint32_t x0w[12], x1w[12], y0w[12], y1w[12];
    load_words(in, x0w);
    load_words(in + 48, x1w);
    uint32_t flags;
    if (mode == COMPRESSED) {
        flags = x1w[11] >> 30;
        x1w[11] &= 0x3fffffffu;
    } else {
        load_words(in + 96, y0w);
        load_words(in + 144, y1w);
        flags = y1w[11] >> 30;
        y1w[11] &= 0x3fffffffu;
        if ((flags & 2u) || !words_below_modulus(y0w) || !words_below_modulus(y1w)) return false;
    }
    if (flags == 3u || !words_below_modulus(x0w) || !words_below_modulus(x1w)) return false;
    if (flags & 1u) return words_zero(x0w) && words_zero(x1w) && (mode == COMPRESSED || (words_zero(y0w) && words_zero(y1w)));
    Fq2_29 x;
    x.c0 = fq_from_words(x0w);
    x.c1 = fq_from_words(x1w);
    // x^3 + 4 (1 + u), canonical per component
    const Fq2_29 x3 = fq2_mul(fq2_sqr(x), x);
    const Fq29 four = fq_four();
    const Fq29 r0 = fq_reduce(fq_add(x3.c0, four)), r1 = fq_reduce(fq_add(x3.c1, four));
    Fq2_29 y;
    if (mode == COMPRESSED) {
        y = fq2_sqrt_candidate(r0, r1);
    } else {
        y.c0 = fq_from_words(y0w);
        y.c1 = fq_from_words(y1w);
    }
    const Fq2_29 yy = fq2_sqr(y);
    if (!fq_equal(yy.c0, r0) || !fq_equal(yy.c1, r1)) return false;
    if (mode == COMPRESSED) {
        fq_to_words(y.c0, y0w);
        fq_to_words(y.c1, y1w);
        if (words2_greater(y0w, y1w) != ((flags & 2u) != 0)) { y.c0 = fq_neg<4>(y.c0); y.c1 = fq_neg<4>(y.c1); }
    }
    uint32_t *out = (uint32_t *)limbs;
    fq_to_ark(x.c0, out);
    fq_to_ark(x.c1, out + 12);
    fq_to_ark(y.c0, out + 24);
    fq_to_ark(y.c1, out + 36);
    return true;
}

// ---- a proof: A | B | C -------------------------------------------------------------------------------------------------------------------
// limbs: uint64_t[48]; out: proof_bytes(mode).  A refused proof leaves all zero bytes (encode) or limbs (decode).  The host entry points
// and the device's encode kernel run these; the device's decode kernels split the same three point decodes over lanes (frw_wire.hip).
__host__ __device__ inline bool proof_encode(const uint64_t *p, int mode, uint8_t *o)
{
    bool ok = g1_encode(p, mode, o);
    ok = g2_encode(p + 12, mode, o + g1_bytes(mode)) && ok;
    ok = g1_encode(p + 36, mode, o + g1_bytes(mode) + g2_bytes(mode)) && ok;
    if (!ok) zero_bytes(o, proof_bytes(mode));
    return ok;
}
__host__ __device__ __forceinline__ void proof_clear(uint64_t *p)
{
    for (int k = 0; k < 48; k++) p[k] = 0;
}
__host__ __device__ inline bool proof_decode(const uint8_t *in, int mode, uint64_t *p)
{
    bool ok = g1_decode(in, mode, p);
    ok = g2_decode(in + g1_bytes(mode), mode, p + 12) && ok;
    ok = g1_decode(in + g1_bytes(mode) + g2_bytes(mode), mode, p + 36) && ok;
    if (!ok) proof_clear(p);
    return ok;
}

// ---- what frw_verify_dev.hip needs of frw_wire.hip ------------------------------------------------------------------------------------------
// `count` proofs from d_wire into d_proofs (uint64_t[count][48]) and d_status (0 or -1), on `st`; allocates nothing
int decode_proofs_launch(size_t count, const uint8_t *d_wire, int mode, uint64_t *d_proofs, int32_t *d_status, hipStream_t st);

}  // namespace wire
}  // namespace frw
