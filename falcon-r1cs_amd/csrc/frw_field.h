// frw_field.h -- the witness encodings over ANY four-limb scalar field: Montgomery constants derived from a modulus on the
// host, and the conversion integer -> x 2^256 mod p with those constants at run time.  Compiles for the host and for the
// device (tests/cpp/test_field.cpp builds it with g++ through tests/cpp/hip_host); the same code serves frw_field_info,
// frw_expand_field_host and the ENC = 3 instantiations of frw_kernels.hip.
//
// Admissible modulus: odd, 2^160 < p < 2^255.
//   * odd            the Montgomery quotient digit needs p^-1 mod 2^32.
//   * p > 2^160      the reference's ladder values reach 160 bits (falcon_ntt.rs:31-39) and must not wrap in the field.
//   * p < 2^255      field_cios_round keeps T < 2 p (below), so 2 p < 2^256 is what lets field_cond_sub_p look at eight
//                    limbs only: T[8] == 0 on entry and one subtraction of p lands in [0, p).
// Primality is the caller's business: for a composite p the bytes x 2^256 mod p are just as well defined.
//
// Why T < 2 p after every round: T' = (T + x K + m p) / 2^32 with T < 2 p, x, m < 2^32 and K < p gives
// T' < (2 p + (2^32 - 1) (K + p)) / 2^32 < (2 p + (2^32 - 1) 2 p) / 2^32 = 2 p.  (The numerator may pass 2^288 by one bit:
// that is the tenth limb t9 of the round.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace frw {

// What a kernel needs of the field, 33 words.  Passed BY VALUE as a kernel argument: launch-uniform, so the compiler keeps
// the words in scalar registers and no lane ever reads a table.
struct FieldConsts {
    uint32_t p[8];        // the modulus, 32-bit little-endian limbs
    uint32_t one[8];      // 2^256 mod p: the Montgomery form of 1
    uint32_t k1[8];       // 2^288 mod p: REDC_1(x k1) = x 2^256 mod p for a one-limb x
    uint32_t k5[8];       // 2^416 mod p: REDC_5(x k5) = x 2^256 mod p for a five-limb x
    uint32_t ninv32;      // -p^-1 mod 2^32
};

// everything frw_field_info reports
struct FieldDerived {
    FieldConsts fc;
    uint32_t r2[8];       // 2^512 mod p
    uint32_t bits;        // bit length of p
};

// One CIOS round with run-time constants: T (9 limbs) <- (T + x K + m p) / 2^32, m = T[0] ninv32 mod 2^32.
__host__ __device__ __forceinline__ void field_cios_round(uint32_t (&T)[9], uint32_t x, const uint32_t (&K)[8], const uint32_t (&P)[8],
                                                          uint32_t ninv32)
{
    uint64_t acc;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        acc = (uint64_t)x * K[j] + T[j] + c;
        T[j] = (uint32_t)acc;
        c = (uint32_t)(acc >> 32);
    }
    acc = (uint64_t)T[8] + c;
    T[8] = (uint32_t)acc;
    const uint32_t t9 = (uint32_t)(acc >> 32);
    const uint32_t m = T[0] * ninv32;
    acc = (uint64_t)m * P[0] + T[0];
    c = (uint32_t)(acc >> 32);
#pragma unroll
    for (int j = 1; j < 8; j++) {
        acc = (uint64_t)m * P[j] + T[j] + c;
        T[j - 1] = (uint32_t)acc;
        c = (uint32_t)(acc >> 32);
    }
    acc = (uint64_t)T[8] + c;
    T[7] = (uint32_t)acc;
    T[8] = t9 + (uint32_t)(acc >> 32);
}

// T < 2 p < 2^256 on entry (T[8] == 0, see the head of this file); subtract p once if T >= p.
__host__ __device__ __forceinline__ void field_cond_sub_p(const uint32_t (&T)[9], const uint32_t (&P)[8], uint32_t (&out)[8])
{
    uint32_t d[8];
    uint32_t bw = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)T[j] - P[j] - bw;
        d[j] = (uint32_t)x;
        bw = (uint32_t)(x >> 63);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = bw ? T[j] : d[j];
}

// integer < 2^32  ->  x 2^256 mod p
__host__ __device__ __forceinline__ void field_encode_u32(const FieldConsts &f, uint32_t x, uint32_t (&out)[8])
{
    uint32_t T[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    field_cios_round(T, x, f.k1, f.p, f.ninv32);
    field_cond_sub_p(T, f.p, out);
}

// integer < 2^160 (five limbs)  ->  x 2^256 mod p
__host__ __device__ __forceinline__ void field_encode_u160(const FieldConsts &f, const uint32_t (&x)[5], uint32_t (&out)[8])
{
    uint32_t T[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 5; i++) field_cios_round(T, x[i], f.k5, f.p, f.ninv32);
    field_cond_sub_p(T, f.p, out);
}

// ---- host side: the constants of a modulus, by shift-and-reduce ----------------------------------------------------------------
// x <- 2 x mod p for x < p < 2^255 (2 x < 2^256: eight limbs hold it)
inline void field_double_mod(uint32_t (&x)[8], const uint32_t (&p)[8])
{
    uint32_t t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 8; j++) t[j] = (x[j] << 1) | (j ? x[j - 1] >> 31 : 0u);
    field_cond_sub_p(t, p, x);
}

// false: the modulus is not admissible (see the head of this file) and *out is untouched
inline bool field_derive(const uint64_t modulus[4], FieldDerived *out)
{
    FieldDerived d{};
    for (int j = 0; j < 4; j++) {
        d.fc.p[2 * j] = (uint32_t)modulus[j];
        d.fc.p[2 * j + 1] = (uint32_t)(modulus[j] >> 32);
    }
    uint32_t bits = 0;
    for (int j = 7; j >= 0 && !bits; j--)
        for (int b = 31; b >= 0; b--)
            if (d.fc.p[j] >> b & 1u) { bits = 32 * j + b + 1; break; }
    if (!(d.fc.p[0] & 1u) || bits < 161 || bits > 255) return false;     // odd with >= 161 bits is > 2^160; <= 255 bits is < 2^255
    d.bits = bits;
    uint32_t inv = d.fc.p[0];                                             // Newton: p inv = 1 mod 2^(3 -> 6 -> 12 -> 24 -> 48)
    for (int i = 0; i < 4; i++) inv *= 2u - d.fc.p[0] * inv;
    d.fc.ninv32 = 0u - inv;
    uint32_t x[8] = {1, 0, 0, 0, 0, 0, 0, 0};                             // 2^k mod p, k = 0 .. 512
    for (int k = 1; k <= 512; k++) {
        field_double_mod(x, d.fc.p);
        uint32_t *dst = k == 256 ? d.fc.one : k == 288 ? d.fc.k1 : k == 416 ? d.fc.k5 : k == 512 ? d.r2 : nullptr;
        if (dst)
            for (int j = 0; j < 8; j++) dst[j] = x[j];
    }
    *out = d;
    return true;
}

}  // namespace frw
