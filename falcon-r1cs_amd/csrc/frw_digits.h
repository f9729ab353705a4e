// frw_digits.h -- the scalar side of the multi-scalar multiplications (frw_msm.hip), said once: a scalar as a canonical integer, its
// signed C-bit digits, and how a digit names its bucket and its entry.  Plain inline arithmetic: tests/cpp/test_digits.cpp compiles it
// for the host (tests/cpp/hip_host) and tests/test_digits_host.py holds it to Python integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frw_fr29.h"

namespace frw {

// the scalar as a canonical integer below r
__device__ __forceinline__ Fr8 scalar_canonical(const uint32_t *src, int montgomery)
{
    Fr8 w = fr_load(src);
    if (montgomery) {
        // ark-ff's h R (R = 2^256) -> h: one product with 2^5 in R' = 2^261 arithmetic (frw_fr29.h), then the canonical form
        F29 c;
#pragma unroll
        for (int k = 0; k < NL29; k++) c.l[k] = k ? 0u : 32u;
        w = f29_pack(f29_canonical(f29_mul(f29_unpack(w), c)));
    } else {
        // "canonical" is the caller's promise; any 256-bit integer is brought below r here (2^256 < 4 r: two conditional
        // subtractions), because a top digit above 2^15 would index past the buckets -- and k P = (k mod r) P anyway
        w = f29_pack(f29_canonical(f29_reduce_4p(f29_unpack(w))));
    }
    return w;
}
// The scalar 1: a Falcon witness is 45 % ones (the boolean elements that are set), which would all land in bucket 0 of window 0 --
// the sums over window tables add them up apart from the buckets (a list or a bit mask of them: msm_ones_kernel, nmsm_ones_kernel).
__device__ __forceinline__ bool scalar_is_one(const Fr8 &k)
{
    return k.l[0] == 1u && !(k.l[1] | k.l[2] | k.l[3] | k.l[4] | k.l[5] | k.l[6] | k.l[7]);
}
// W signed C-bit digits of a canonical integer: d_j in [-2^(C-1) + 1, 2^(C-1)] with sum d_j 2^(C j) = k.  A digit above 2^(C-1) borrows
// from the next window; the top window takes the last carry and is never negative (k < 2^255 keeps it <= 2^(C-1) for the widths in
// use: 16 x 16, 32 x 8 and 13 x 20 bits, the last window of the thirteen being bits 240 ..).  The C bits of a window come out of the
// two words they may straddle; where C divides 32 that folds to one shift and one mask.
template <int C, int W> __device__ __forceinline__ void signed_digits(const Fr8 &k, int (&d)[W])
{
    static_assert(C >= 2 && C <= 30 && C * W >= 255 && C * (W - 1) < 256, "W windows of C bits cover a scalar");
    int carry = 0;
#pragma unroll
    for (int j = 0; j < W; j++) {
        const int bit = C * j, word = bit >> 5, sh = bit & 31;
        const uint64_t two = (uint64_t)k.l[word] | (word + 1 < 8 ? (uint64_t)k.l[word + 1] << 32 : 0ull);
        int v = (int)((two >> sh) & ((1u << C) - 1u)) + carry;
        carry = 0;
        if (j + 1 < W && v > (1 << (C - 1))) { v -= 1 << C; carry = 1; }
        d[j] = v;
    }
}
// a non-zero digit's bucket, |v| - 1, and its entry in the bucket's list: what to add (a table row or a point) with the sign on top
__device__ __forceinline__ uint32_t digit_bucket(int v) { return (uint32_t)(v < 0 ? -v : v) - 1u; }
__device__ __forceinline__ uint32_t digit_entry(uint32_t index, int v) { return index | (v < 0 ? 0x80000000u : 0u); }

}  // namespace frw
