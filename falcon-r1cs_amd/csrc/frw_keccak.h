// frw_keccak.h -- Keccak-f[1600] on the device, one lane per state: the SHAKE256 of Falcon's hash-to-point (frw_prepare.hip) and of
// the batched verifier's random scalars (frw_pairing_dev.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace frw {

static __constant__ uint64_t KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
    0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
    0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
    0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

__device__ __forceinline__ uint64_t rol64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }

// Keccak-f[1600], state as 25 lanes A[x + 5y]; every index below is a compile-time constant (registers, no scratch)
__device__ __forceinline__ void keccak_f1600(uint64_t (&a)[25])
{
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
        uint64_t c0 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20];
        uint64_t c1 = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21];
        uint64_t c2 = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22];
        uint64_t c3 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23];
        uint64_t c4 = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];
        const uint64_t d0 = c4 ^ rol64(c1, 1), d1 = c0 ^ rol64(c2, 1), d2 = c1 ^ rol64(c3, 1), d3 = c2 ^ rol64(c4, 1),
                       d4 = c3 ^ rol64(c0, 1);
        // theta + rho + pi: b[y + 5((2x+3y) mod 5)] = rol(a[x+5y] ^ d[x], rot[x][y])
        const uint64_t b0 = a[0] ^ d0;
        const uint64_t b10 = rol64(a[1] ^ d1, 1), b20 = rol64(a[2] ^ d2, 62), b5 = rol64(a[3] ^ d3, 28), b15 = rol64(a[4] ^ d4, 27);
        const uint64_t b16 = rol64(a[5] ^ d0, 36), b1 = rol64(a[6] ^ d1, 44), b11 = rol64(a[7] ^ d2, 6), b21 = rol64(a[8] ^ d3, 55),
                       b6 = rol64(a[9] ^ d4, 20);
        const uint64_t b7 = rol64(a[10] ^ d0, 3), b17 = rol64(a[11] ^ d1, 10), b2 = rol64(a[12] ^ d2, 43), b12 = rol64(a[13] ^ d3, 25),
                       b22 = rol64(a[14] ^ d4, 39);
        const uint64_t b23 = rol64(a[15] ^ d0, 41), b8 = rol64(a[16] ^ d1, 45), b18 = rol64(a[17] ^ d2, 15), b3 = rol64(a[18] ^ d3, 21),
                       b13 = rol64(a[19] ^ d4, 8);
        const uint64_t b14 = rol64(a[20] ^ d0, 18), b24 = rol64(a[21] ^ d1, 2), b9 = rol64(a[22] ^ d2, 61), b19 = rol64(a[23] ^ d3, 56),
                       b4 = rol64(a[24] ^ d4, 14);
        // chi (+ iota on lane 0)
        a[0] = b0 ^ (~b1 & b2) ^ KECCAK_RC[r]; a[1] = b1 ^ (~b2 & b3); a[2] = b2 ^ (~b3 & b4); a[3] = b3 ^ (~b4 & b0); a[4] = b4 ^ (~b0 & b1);
        a[5] = b5 ^ (~b6 & b7); a[6] = b6 ^ (~b7 & b8); a[7] = b7 ^ (~b8 & b9); a[8] = b8 ^ (~b9 & b5); a[9] = b9 ^ (~b5 & b6);
        a[10] = b10 ^ (~b11 & b12); a[11] = b11 ^ (~b12 & b13); a[12] = b12 ^ (~b13 & b14); a[13] = b13 ^ (~b14 & b10); a[14] = b14 ^ (~b10 & b11);
        a[15] = b15 ^ (~b16 & b17); a[16] = b16 ^ (~b17 & b18); a[17] = b17 ^ (~b18 & b19); a[18] = b18 ^ (~b19 & b15); a[19] = b19 ^ (~b15 & b16);
        a[20] = b20 ^ (~b21 & b22); a[21] = b21 ^ (~b22 & b23); a[22] = b22 ^ (~b23 & b24); a[23] = b23 ^ (~b24 & b20); a[24] = b24 ^ (~b20 & b21);
    }
}

}  // namespace frw
