// frw_drbg.h -- the scalars that create_random_proof and rerandomize_proof draw from their rng (ark-groth16 0.3.0 prover.rs), derived
// from a seed and a counter: ONE definition for the host function (frw_fr_draw) and the device kernel (frw_drbg.hip, fr_draw_kernel).
//     msg  = "FRW-FR-DRAW-001" (15 bytes) || tag (1) || seed (32) || le64(counter) || le64(j)              64 bytes
//     out  = SHAKE256(msg), first 64 bytes
//     x_j  = int_le(out) mod r                       r: BLS12-381's group order; x_j canonical, four little-endian 64-bit words
// The message is eight whole words of one 136-byte rate block: absorbing it is writing the state's first eight lanes, the padding two
// more XORs, and one permutation leaves the 64 bytes in lanes 0 .. 7.  The reduction is WIDE on purpose: 512 bits modulo r are within
// 2^-257 of uniform, there is no rejection loop, and every lane does the same work:
//     x = (hi mod r) (2^256 mod r) + (lo mod r)  mod r
// by frw_rerand.h's plain 64-bit arithmetic, with the CONSTANT as the operand whose bits fr_mul branches on -- no branch of the product
// depends on the secret half.  (fr_reduce's and fr_add's conditional subtractions still do: the caveat of frw_rerand.h holds here too.)
// What differs between host and device is the permutation alone: frw_keccak.h's is device code (its round constants are __constant__
// memory, its state a lane's registers), so the host has a plain loop below; tests/test_drbg_host.py and tests/test_gpu_drbg.py hold
// both to hashlib.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "frw_rerand.h"

namespace frw {
namespace drbg {

// "FRW-FR-D" and "RAW-001" as little-endian words; the tag is the sixteenth byte
constexpr uint64_t DOMAIN_W0 = 0x442d52462d575246ULL, DOMAIN_W1 = 0x003130302d574152ULL;

FRW_RR_HD uint64_t load_le64(const uint8_t *p)                          // (a seed has no alignment)
{
    uint64_t w = 0;
    for (int k = 0; k < 8; k++) w |= (uint64_t)p[k] << (8 * k);
    return w;
}
// the padded message as the state before the permutation (every index a constant: the state stays in a lane's registers)
FRW_RR_HD void absorb(const uint8_t *seed, uint64_t counter, int tag, uint64_t j, uint64_t (&a)[25])
{
    a[0] = DOMAIN_W0;
    a[1] = DOMAIN_W1 | ((uint64_t)(tag & 0xff) << 56);
    a[2] = load_le64(seed);
    a[3] = load_le64(seed + 8);
    a[4] = load_le64(seed + 16);
    a[5] = load_le64(seed + 24);
    a[6] = counter;
    a[7] = j;
    a[8] = 0x1fULL;                                                     // SHAKE's suffix 1111 and the first padding bit, byte 64
    a[9] = 0; a[10] = 0; a[11] = 0; a[12] = 0; a[13] = 0; a[14] = 0; a[15] = 0;
    a[16] = 0x80ULL << 56;                                              // the last padding bit, byte 135
    a[17] = 0; a[18] = 0; a[19] = 0; a[20] = 0; a[21] = 0; a[22] = 0; a[23] = 0; a[24] = 0;
}
// 2^256 mod r
FRW_RR_HD uint64_t two256_word(int k)
{
    return k == 0 ? 0x00000001fffffffeULL : k == 1 ? 0x5884b7fa00034802ULL : k == 2 ? 0x998c4fefecbc4ff5ULL : 0x1824b159acc5056fULL;
}
// lo + 2^256 hi modulo r (four words each, any values) -> out, canonical
FRW_RR_HD void reduce512(const uint64_t *lo, const uint64_t *hi, uint64_t *out)
{
    uint64_t l[4] = {lo[0], lo[1], lo[2], lo[3]}, h[4] = {hi[0], hi[1], hi[2], hi[3]}, t[4];
    const uint64_t c[4] = {two256_word(0), two256_word(1), two256_word(2), two256_word(3)};
    rerand::fr_reduce(l);
    rerand::fr_reduce(h);
    rerand::fr_mul(h, c, t);                                            // (the loop follows the bits of c)
    rerand::fr_add(t, l);
    for (int k = 0; k < 4; k++) out[k] = t[k];
}
// the state after the permutation -> x_j
FRW_RR_HD void squeeze(const uint64_t (&a)[25], uint64_t *out)
{
    const uint64_t lo[4] = {a[0], a[1], a[2], a[3]}, hi[4] = {a[4], a[5], a[6], a[7]};
    reduce512(lo, hi, out);
}

// Keccak-f[1600] for the host: the textbook loop (FIPS 202, 3.2), nowhere near a hot path
inline void keccak_f1600_host(uint64_t (&a)[25])
{
    static const int rho[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
    static const uint64_t rc[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
        0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
        0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
        0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    static const int pi[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
    for (int round = 0; round < 24; round++) {
        uint64_t c[5];
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
        for (int x = 0; x < 5; x++) {
            const uint64_t r1 = c[(x + 1) % 5], d = c[(x + 4) % 5] ^ ((r1 << 1) | (r1 >> 63));
            for (int y = 0; y < 25; y += 5) a[x + y] ^= d;
        }
        uint64_t cur = a[1];
        for (int i = 0; i < 24; i++) {
            const uint64_t next = a[pi[i]];
            a[pi[i]] = (cur << rho[i]) | (cur >> (64 - rho[i]));
            cur = next;
        }
        for (int y = 0; y < 25; y += 5) {
            const uint64_t row[5] = {a[y], a[y + 1], a[y + 2], a[y + 3], a[y + 4]};
            for (int x = 0; x < 5; x++) a[y + x] = row[x] ^ (~row[(x + 1) % 5] & row[(x + 2) % 5]);
        }
        a[0] ^= rc[round];
    }
}
// x_j on the host
inline void draw_one_host(const uint8_t *seed, uint64_t counter, int tag, uint64_t j, uint64_t *out)
{
    uint64_t a[25];
    absorb(seed, counter, tag, j, a);
    keccak_f1600_host(a);
    squeeze(a, out);
}

// The device's part (frw_drbg.hip), for the composed calls beside the calls they wrap (frw_msm.hip, frw_rerand.hip).  Both enqueue on
// `stream` alone and return FRW_OK or the recorded HIP error; the current device is the caller's business.
//   draw_launch      x_0 .. x_{count-1} for (seed, *d_counter, tag) into d_out[count][4]
//   advance_launch   *d_counter += 1 (modulo 2^64), a launch of its own BEHIND the draw: every lane of the draw has read the old value
int draw_launch(const uint8_t *d_seed, const uint64_t *d_counter, int tag, size_t count, uint64_t *d_out, void *stream);
int advance_launch(uint64_t *d_counter, void *stream);

}  // namespace drbg
}  // namespace frw
