// frw_rows.h -- how a point lies in device memory, for the units that read or write the multi-scalar multiplication's tables
// (frw_msm.hip owns them; frw_wire.hip turns a proving key's rows back into bytes): a table ROW (x, y in fourteen 29-bit limbs per
// Fq value, x 2^406, all zero = the point at infinity) and ark-ff's affine point (6 x uint64_t per Fq value, x 2^384, all zero = infinity).
// Device code only (the two-lane Fq2 of frw_fq29.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frw_fq29.h"

namespace frw {

// per group (F = FqField: G1, Fq2Field: G2): a table row = x, y limbs (all zero = the point at infinity); a bucket = X, Y, ZZ,
// ZZZ limbs + the infinity flag (padded to 16 bytes); ark-ff's bytes of an affine point
template <class F> struct Grp {
    static constexpr int PT_WORDS = 2 * F::WORDS, BK_WORDS = 4 * F::WORDS + 4, ARK_WORDS = 2 * F::ARK_WORDS;
    static constexpr uint32_t K_AFFINE_Y = F::K_AFFINE;       // bound of a table row's y: what its negation adds
};

template <class F> __device__ __forceinline__ AffineT<F> load_row(const uint32_t *row)
{
    constexpr int PW = Grp<F>::PT_WORDS;
    AffineT<F> p;
    uint32_t any = 0;
    const uint4 *v = (const uint4 *)row;
    uint32_t w[PW];
#pragma unroll
    for (int k = 0; k < PW / 4; k++) {
        const uint4 t = v[k];
        w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w;
    }
#pragma unroll
    for (int k = 0; k < PW; k++) any |= w[k];
    p.x = F::load(w);
    p.y = F::load(w + F::WORDS);
    p.inf = any == 0;
    return p;
}
// the two-lane Fq2: every lane fetches its own component of x and y (56 bytes each, 8-byte aligned) and the pair agrees on `inf`
template <> __device__ __forceinline__ AffineT<Fq2PairField> load_row<Fq2PairField>(const uint32_t *row)
{
    AffineT<Fq2PairField> p;
    const uint32_t *mine = row + (Fq2PairField::odd() ? NLQ : 0);
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < NLQ / 2; k++) {
        const uint2 a = *(const uint2 *)(mine + 2 * k), b = *(const uint2 *)(mine + 2 * NLQ + 2 * k);
        p.x.v.l[2 * k] = a.x; p.x.v.l[2 * k + 1] = a.y;
        p.y.v.l[2 * k] = b.x; p.y.v.l[2 * k + 1] = b.y;
        any |= a.x | a.y | b.x | b.y;
    }
    any |= pair_swap_u32(any);
    p.inf = any == 0;
    return p;
}
template <class F> __device__ __forceinline__ void store_row(uint32_t *row, const AffineT<F> &p)
{
    uint32_t w[Grp<F>::PT_WORDS];
    F::store(p.x, w);
    F::store(p.y, w + F::WORDS);
#pragma unroll
    for (int k = 0; k < Grp<F>::PT_WORDS; k++) row[k] = p.inf ? 0u : w[k];
}
// the two-lane Fq2: every lane writes its own component of x and of y
template <> __device__ __forceinline__ void store_row<Fq2PairField>(uint32_t *row, const AffineT<Fq2PairField> &p)
{
    uint32_t *mine = row + (Fq2PairField::odd() ? NLQ : 0);
#pragma unroll
    for (int k = 0; k < NLQ; k++) {
        mine[k] = p.inf ? 0u : p.x.v.l[k];
        mine[2 * NLQ + k] = p.inf ? 0u : p.y.v.l[k];
    }
}
template <class F> __device__ __forceinline__ AffineT<F> load_ark_point(const uint32_t *w)
{
    AffineT<F> p;
    uint32_t any = 0;
    for (int k = 0; k < Grp<F>::ARK_WORDS; k++) any |= w[k];
    p.inf = any == 0;
    p.x = F::from_ark(w);
    p.y = F::from_ark(w + F::ARK_WORDS);
    return p;
}
template <class F> __device__ __forceinline__ void store_ark_point(uint32_t *o, const AffineT<F> &a)
{
    if (a.inf) {
        for (int k = 0; k < Grp<F>::ARK_WORDS; k++) o[k] = 0;
    } else {
        F::to_ark(a.x, o);
        F::to_ark(a.y, o + F::ARK_WORDS);
    }
}

}  // namespace frw
