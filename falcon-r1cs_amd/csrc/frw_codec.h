// frw_codec.h -- Falcon's encodings, one item at a time: the SHAKE256 hash-to-point, one coefficient of an encoded public key and
// the signature decoder (Falcon specification v1.2, sections 3.7 and 3.11).  The kernels and launchers around them are
// frw_prepare.hip's; nothing here knows about a grid, so the same functions compile for the host (tests/cpp/test_codec.cpp drives
// them against a restatement of the specification, and a sanitized stand-alone program checks that none reads past its input).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "frw_keccak.h"

namespace frw {
namespace codec {

constexpr uint32_t Q = 12289;          // == frw::Q of frw_device.h, which is not for the host
constexpr int SHAKE256_RATE = 136;
constexpr int NONCE_LEN = 40;

// hm = HashToPoint(nonce || msg): SHAKE256, big-endian 16-bit words, accept w < 5q as w mod q (Falcon spec Alg. 3).  One signature: its
// 40-byte nonce, its message msgs[o0 .. o1) and its row of N coefficients, wherever the caller keeps them.
__device__ __forceinline__ void hash_to_point_one(int logn, const uint8_t *__restrict__ nonce, const uint8_t *__restrict__ msg, uint64_t o0,
                                         uint64_t o1, uint16_t *__restrict__ out)
{
    const int n = 1 << logn;
    // the host entry point rejects decreasing offsets; a device-side caller that breaks the precondition of
    // include/frw.h gets an empty message here rather than a 2^64-byte absorb loop
    const size_t total = NONCE_LEN + (size_t)(o1 >= o0 ? o1 - o0 : 0);
    uint64_t st[25];
#pragma unroll
    for (int i = 0; i < 25; i++) st[i] = 0;
    // absorb nonce || msg || pad10*1 with the SHAKE domain bits (0x1F ... 0x80)
    for (size_t pos = 0;; pos += SHAKE256_RATE) {
#pragma unroll
        for (int l = 0; l < SHAKE256_RATE / 8; l++) {
            uint64_t w = 0;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const size_t p = pos + (size_t)(l * 8 + b);
                uint32_t byte = 0;
                if (p < NONCE_LEN) byte = nonce[p];
                else if (p < total) byte = msg[p - NONCE_LEN];
                else if (p == total) byte = 0x1F;
                w |= (uint64_t)byte << (8 * b);
            }
            st[l] ^= w;
        }
        const bool last = total < pos + SHAKE256_RATE;
        if (last) st[16] ^= 0x8000000000000000ull;
        keccak_f1600(st);
        if (last) break;
    }
    // squeeze
    int cnt = 0;
    while (cnt < n) {
#pragma unroll
        for (int w = 0; w < SHAKE256_RATE / 2; w++) {
            const uint64_t lane = st[w / 4];
            const int sh = (w % 4) * 16;
            const uint32_t v = (uint32_t)((lane >> sh) & 0xff) << 8 | (uint32_t)((lane >> (sh + 8)) & 0xff);
            if (v < 5 * Q && cnt < n) out[cnt++] = (uint16_t)(v % Q);
        }
        if (cnt < n) keccak_f1600(st);
    }
}

// pk: header 0x00 + logn, then N x 14 bits, big-endian bit order.  Coefficient k of the key at p (any alignment)
__device__ __forceinline__ uint32_t public_key_coeff(const uint8_t *__restrict__ p, int k)
{
    const int bit = 14 * k, off = bit & 7;
    const uint8_t *q = p + 1 + (bit >> 3);
    uint32_t acc = (uint32_t)q[0] << 16 | (uint32_t)q[1] << 8;
    if (off + 14 > 16) acc |= q[2];
    return (acc >> (24 - 14 - off)) & 0x3fffu;
}

// what makes a key malformed: a coefficient that is not reduced, a header that is not this parameter set's
__device__ __forceinline__ bool public_key_coeff_refused(uint32_t c) { return c >= Q; }
__device__ __forceinline__ bool public_key_header_refused(const uint8_t *__restrict__ p, int logn) { return p[0] != (uint8_t)logn; }

// sig: header 0x30 + logn, 40-byte nonce, compressed coefficients, zero padding up to sig_len.  One signature at p (any alignment):
// its N coefficients -> out, its nonce -> nonce_out (may be null; only where the header is the expected one); true: well formed
__device__ __forceinline__ bool decode_signature_one(int logn, const uint8_t *__restrict__ p, size_t sig_len, uint16_t *__restrict__ out,
                                            uint8_t *__restrict__ nonce_out)
{
    const int n = 1 << logn;
    bool ok = sig_len > 1 + NONCE_LEN && p[0] == (uint8_t)(0x30 + logn);
    if (ok && nonce_out)
        for (int i = 0; i < NONCE_LEN; i++) nonce_out[i] = p[1 + i];
    const uint8_t *body = p + 1 + NONCE_LEN;
    const size_t body_len = ok ? sig_len - 1 - NONCE_LEN : 0;
    size_t v = 0;
    uint32_t acc = 0;
    int acc_len = 0;
    for (int u = 0; ok && u < n; u++) {
        if (v >= body_len) { ok = false; break; }
        acc = (acc << 8) | body[v++];
        const uint32_t b = acc >> acc_len;
        const uint32_t sign = b & 128u;
        uint32_t m = b & 127u;
        for (;;) {
            if (acc_len == 0) {
                if (v >= body_len) { ok = false; break; }
                acc = (acc << 8) | body[v++];
                acc_len = 8;
            }
            acc_len--;
            if ((acc >> acc_len) & 1u) break;
            m += 128;
            if (m > 2047) { ok = false; break; }
        }
        if (sign && m == 0) ok = false;             // "-0" is not a valid encoding
        if (ok) out[u] = (uint16_t)(sign ? Q - m : m);
    }
    if (ok && (acc & ((1u << acc_len) - 1u))) ok = false;          // unused bits of the last byte
    for (; ok && v < body_len; v++)
        if (body[v]) ok = false;                                    // padding
    return ok;
}

}  // namespace codec
}  // namespace frw
