// frw_pairing_dev.hip -- the pairing on the device, for Groth16 verification without the host (frw_groth16_verify_full_dev) and for the
// parity tests (frw_diag_pairing_dev).  It computes what frw_pairing.h computes -- the CUBE of the reduced ate pairing, the same final
// exponent -- so values equal frw_diag_pairing's bit for bit; the kernels are laid out for the chip instead.  One lane per pairing
// needs 15 KB of scratch per lane (an Fq12 is 168 registers), so:
//
//   Fq12 across a lane group.  Fq12 = Fq2[w] / (w^6 - xi): lane k of an 8-lane group holds the coefficient of w^k (k < 6; lanes 6 and
//   7 mirror 0 and 1 and are never read), eight pairings to a wave.  In a product lane k sums a_i b_(k-i) over i, xi applied where the
//   index wraps; the operands come from the other lanes of the group by ds_bpermute (__shfl with width 8).  A line (frw_pairing_dev.h)
//   has three coefficients, of 1, w^2, w^3: a sparse product is three Fq2 products per lane.  conj (the q^6-power) negates the odd
//   lanes and the q^j-power is conj^j of a lane's own coefficient times a constant: both lane-local.  Values are lazily reduced
//   (frw_fq29.h): < 132 q per component after a product, never canonicalised until the comparison.
//
//   g2_lines_kernel         a proof's B: its 68 line coefficients (frw_pairing_dev.h, two lanes per point with Fq2PairField), written
//                           to the workspace.  The fixed points -gamma, -delta, beta have theirs made once, on the host, at key load.
//   miller_kernel           up to three pairs per group: f <- f^2 l1 l2 l3 per bit, two Fq products per line at P (the table holds the
//                           rest); no inversions.  Pairs with a point at infinity contribute one, as on the host.
//   final_exp_easy_kernel   ^((q^6 - 1)(q^2 + 1)) with ONE fq_inv (f^-1 = conj(f) h^(q^2) h^(q^4) / N, h = f conj(f), N its norm
//                           to Fq2)
//   final_exp_hard_kernel   frw_pairing.h's chain of five z-powers, Granger - Scott squarings; then the comparison with
//                           e(alpha, beta)^3 (or with one: the batched check), or the value in frw_diag_pairing's basis
//   proof_check_kernel      the proof points' checks of frw_verify.cpp's check_proof, by the same functions: canonical limbs, on
//                           the curve, in the subgroup (a 255-bit ladder; A and C in the two lanes of a pair, B over both with
//                           Fq2PairField) unless the caller vouches for the points.
//   batch_scalar_kernel, batch_sum_kernel, fp12_tree_kernel   FRW_VERIFY_BATCHED: the random scalars rho_i (SHAKE256) and rho_i A_i,
//                           the sums of rho_i P_i, rho_i C_i and rho_i, the product tree of the Miller loops' values
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_keccak.h"
#include "frw_pairing.h"
#include "frw_pairing_dev.h"
#include "frw_verify.h"

namespace frw {
namespace pairing_dev {
namespace {

typedef Fq2_29 F2;

// ---- Fq2 in one lane ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ F2 f2_zero() { F2 r; r.c0 = r.c1 = fq_zero(); return r; }
__device__ __forceinline__ F2 f2_add(const F2 &a, const F2 &b) { F2 r; r.c0 = fq_add(a.c0, b.c0); r.c1 = fq_add(a.c1, b.c1); return r; }
__device__ __forceinline__ F2 f2_mul_xi(const F2 &a)          // (a0 + a1 u)(1 + u); a.c1 < 16 q
{
    F2 r; r.c0 = fq_sub<16>(a.c0, a.c1); r.c1 = fq_add(a.c0, a.c1); return r;
}
__device__ __forceinline__ F2 f2_conj(const F2 &a) { F2 r; r.c0 = a.c0; r.c1 = fq_neg<256>(a.c1); return r; }   // a.c1 <= 256 q
__device__ __forceinline__ F2 f2_select(bool take_a, const F2 &a, const F2 &b)
{
    F2 r; r.c0 = fq_select(take_a, a.c0, b.c0); r.c1 = fq_select(take_a, a.c1, b.c1); return r;
}
__device__ __forceinline__ F2 f2_load(const uint32_t *w)
{
    F2 r;
#pragma unroll
    for (int i = 0; i < NLQ; i++) { r.c0.l[i] = w[i]; r.c1.l[i] = w[NLQ + i]; }
    return r;
}
__device__ __forceinline__ void f2_store(const F2 &a, uint32_t *w)
{
#pragma unroll
    for (int i = 0; i < NLQ; i++) { w[i] = a.c0.l[i]; w[NLQ + i] = a.c1.l[i]; }
}
__device__ __forceinline__ F2 f2_mul_fq(const F2 &a, const Fq29 &s) { F2 r; r.c0 = fq_mul(a.c0, s); r.c1 = fq_mul(a.c1, s); return r; }

// ---- Fq12 across the eight lanes of a group ------------------------------------------------------------------------------------------
// k: this lane's coefficient index (0..5; lanes 6, 7 pass k - 6)
__device__ __forceinline__ F2 grp_shfl(const F2 &a, int src)
{
    F2 r;
#pragma unroll
    for (int i = 0; i < NLQ; i++) {
        r.c0.l[i] = (uint32_t)__shfl((int)a.c0.l[i], src, 8);
        r.c1.l[i] = (uint32_t)__shfl((int)a.c1.l[i], src, 8);
    }
    return r;
}
// a b; operands < 1024 q per component, result < 132 q
__device__ F2 fp12_mul(const F2 &a, const F2 &b, int k)
{
    F2 acc = f2_zero();
#pragma nounroll
    for (int i = 0; i < 6; i++) {
        const int j = k - i < 0 ? k - i + 6 : k - i;
        const F2 p = fq2_mul(grp_shfl(a, i), grp_shfl(b, j));
        acc = f2_add(acc, f2_select(i > k, f2_mul_xi(p), p));
    }
    return acc;
}
// fp12_mul with the operands passed through LDS: the group's coefficients are read from there term by term instead of being held
// (and shuffled) in registers -- 56 fewer live registers, what the final exponentiation's chain needs for its second wave.  Blocks of
// 256 lanes (56 KB).  One wave writes and reads its own rows only, and LDS operations of a wave complete in order.
__device__ F2 fp12_mul_lds(const F2 &a, const F2 &b, int k)
{
    __shared__ uint32_t rows[256 * 2 * COEF_WORDS];
    uint32_t *mine = rows + threadIdx.x * 2 * COEF_WORDS;
    const uint32_t *grp = rows + (threadIdx.x & ~7u) * 2 * COEF_WORDS;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // (the previous product's reads come first)
    __builtin_amdgcn_wave_barrier();
    f2_store(a, mine);
    f2_store(b, mine + COEF_WORDS);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    F2 acc = f2_zero();
#pragma nounroll
    for (int i = 0; i < 6; i++) {
        const int j = k - i < 0 ? k - i + 6 : k - i;
        const F2 p = fq2_mul(f2_load(grp + i * 2 * COEF_WORDS), f2_load(grp + j * 2 * COEF_WORDS + COEF_WORDS));
        acc = f2_add(acc, f2_select(i > k, f2_mul_xi(p), p));
    }
    return acc;
}
// f l for a line l whose only coefficients are those of 1, w^2, w^3 (zero elsewhere in l's lanes)
__device__ F2 fp12_mul_line(const F2 &f, const F2 &l, int k)
{
    F2 acc = f2_zero();
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = t == 0 ? 0 : t + 1;
        const int j = k - i < 0 ? k - i + 6 : k - i;
        const F2 p = fq2_mul(grp_shfl(l, i), grp_shfl(f, j));
        acc = f2_add(acc, f2_select(i > k, f2_mul_xi(p), p));
    }
    return acc;
}
__device__ __forceinline__ F2 fp12_conj(const F2 &a, int k)
{
    F2 n; n.c0 = fq_neg<256>(a.c0); n.c1 = fq_neg<256>(a.c1);
    return f2_select(k & 1, n, a);
}
// the q^e-power, e = 1, 2, 3: conj^e of the coefficient times frob[e - 1][k]
__device__ __forceinline__ F2 fp12_frob(const F2 &a, int e, const uint32_t *frob, int k)
{
    const F2 c = (e & 1) ? f2_conj(a) : a;
    return fq2_mul(c, f2_load(frob + ((e - 1) * 6 + k) * COEF_WORDS));
}
// a^2 for a in the cyclotomic subgroup (Granger - Scott).  Fq12 = Fq4[w] / (w^3 - s), Fq4 = Fq2[s] / (s^2 - xi), s = w^3: lanes k and
// k + 3 hold g_k = a_k + a_(k+3) s, and a = g0 + g1 w + g2 w^2 squares to
//     (3 g0^2 - 2 conj(g0)) + (3 s g2^2 + 2 conj(g1)) w + (3 g1^2 - 2 conj(g2)) w^2,      conj: s -> -s
// -- three Fq4 squares (each lane: its half of one of them) instead of a full product.  Operands < 1024 q, result < 2 q.
__device__ F2 fp12_cyclotomic_sqr(const F2 &a, int k)
{
    const bool low = k < 3;
    const F2 partner = grp_shfl(a, low ? k + 3 : k - 3);
    // g^2 = (x0^2 + xi x1^2) + (2 x0 x1) s: the low lane (x0 = a) its first half, the high lane (x1 = a) its second
    F2 sq;
    if (low) sq = f2_add(fq2_sqr(a), f2_mul_xi(fq2_sqr(partner)));
    else { const F2 t = fq2_mul(a, partner); sq = f2_add(t, t); }
    // lane k takes the square's half from lane src: w^0 <- 0, w^3 <- 3, w^1 <- 5 (times xi: s g2^2), w^4 <- 2, w^2 <- 1, w^5 <- 4
    const int src = k == 0 ? 0 : k == 3 ? 3 : k == 1 ? 5 : k == 4 ? 2 : k == 2 ? 1 : 4;
    F2 t = grp_shfl(sq, src);
    if (k == 1) { F2 x; x.c0 = fq_sub<64>(t.c0, t.c1); x.c1 = fq_add(t.c0, t.c1); t = x; }      // (t.c1 < 22 q)
    const F2 t3 = f2_add(f2_add(t, t), t), a2 = f2_add(a, a);
    F2 r;
    if (k == 0 || k == 4 || k == 2) { r.c0 = fq_sub<1024>(t3.c0, a2.c0); r.c1 = fq_sub<1024>(t3.c1, a2.c1); }   // (a < 132 q)
    else r = f2_add(t3, a2);
    // (the sum keeps a's bound: one product with one brings it back below 2 q)
    const Fq29 one = fq_const(FQ29_ONE);
    r.c0 = fq_mul(r.c0, one); r.c1 = fq_mul(r.c1, one);
    return r;
}
// a^z for a in the cyclotomic subgroup (conj = inverse); a is this lane's coefficient at `slot` (re-read where it is needed: the
// registers of the final exponentiation are what limits its waves)
__device__ F2 cyclotomic_exp_z(const uint32_t *slot, int k)
{
    F2 acc = f2_load(slot);
#pragma nounroll
    for (int bit = 62; bit >= 0; bit--) {
        acc = fp12_cyclotomic_sqr(acc, k);
        if ((Z_ABS >> bit) & 1ull) acc = fp12_mul_lds(acc, f2_load(slot), k);
    }
    return fp12_conj(acc, k);
}

// The G1 point of a pair in this lane's role: x for lane 2, y for lane 3 (the coefficients of w^2 and w^3 take them), one elsewhere.
struct PairPoint { Fq29 s; bool inf; };
__device__ __forceinline__ PairPoint load_pair_point(const uint64_t *w, int k)
{
    uint64_t any = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) any |= w[i];
    PairPoint p;
    p.inf = any == 0;
    p.s = k == 2 || k == 3 ? fq_from_ark((const uint32_t *)(w + (k == 3 ? 6 : 0))) : fq_const(FQ29_ONE);   // (k < 0: the flag only)
    return p;
}

// a pair: the G1 points at p + i * pstride (12 words each), the line tables at table + i * tstride (tstride 0: one fixed table)
struct MillerPairs {
    const uint64_t *p[3];
    const uint32_t *table[3];
    uint64_t pstride[3], tstride[3];
    int npairs;
};

// inactive: pairs whose G2 point is the point at infinity (a fixed point of the key: bit j for pair j); skip (optional): nothing to do
// when *skip is set (the batched check passed); excluded_as_one: an item with status != 0 or a degenerate loop writes one (the batched
// check leaves it out of its product) instead of nothing
__global__ __launch_bounds__(256) void miller_kernel(uint64_t n, MillerPairs mp, unsigned inactive, const int32_t *__restrict__ status,
                                                     const int32_t *__restrict__ flags, const int32_t *__restrict__ skip, int excluded_as_one,
                                                     uint32_t *__restrict__ out)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int lane = threadIdx.x & 7, k = lane < 6 ? lane : lane - 6;
    if (g >= n || (skip && *skip)) return;                         // (a whole group leaves together)
    F2 f = f2_zero();
    f.c0 = fq_select(lane == 0, fq_const(FQ29_ONE), fq_zero());
    const bool excluded = (status && status[g]) || (excluded_as_one && flags && (flags[g] & 3) == 2);
    if (excluded) {
        if (excluded_as_one && lane < 6) f2_store(f, out + g * 3 * FP12_WORDS + lane * COEF_WORDS);
        return;
    }
    unsigned active = 0;
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (j < mp.npairs && !((inactive >> j) & 1u) && !load_pair_point(mp.p[j] + g * mp.pstride[j], -1).inf &&
            !(j == 0 && flags && (flags[g] & 1)))
            active |= 1u << j;
    // coefficient of this lane in a line's table entry: lane 0 -> c0, lane 2 -> c1 (times xP), lane 3 -> c2 (times yP)
    const int coef = lane == 0 ? 0 : lane == 2 ? 1 : lane == 3 ? 2 : -1;
    int line = 0;
#pragma nounroll
    for (int bit = 62; bit >= 0; bit--) {
        f = fp12_mul(f, f, k);
        const int steps = ((Z_ABS >> bit) & 1ull) ? 2 : 1;
#pragma nounroll
        for (int st = 0; st < steps; st++, line++) {
#pragma nounroll
            for (int j = 0; j < mp.npairs; j++) {
                if (!((active >> j) & 1u)) continue;                // (uniform over the group)
                // (no dynamic index into the kernel argument's arrays: that would copy them to scratch)
                const uint32_t *tab = j == 0 ? mp.table[0] + g * mp.tstride[0] : j == 1 ? mp.table[1] + g * mp.tstride[1] : mp.table[2] + g * mp.tstride[2];
                const uint64_t *pw = j == 0 ? mp.p[0] + g * mp.pstride[0] : j == 1 ? mp.p[1] + g * mp.pstride[1] : mp.p[2] + g * mp.pstride[2];
                F2 l = f2_zero();
                if (coef >= 0)                                      // (P's coordinate converted again: fewer live registers)
                    l = f2_mul_fq(f2_load(tab + (uint64_t)line * LINE_WORDS + coef * COEF_WORDS), load_pair_point(pw, k).s);
                f = fp12_mul_line(f, l, k);
            }
        }
    }
    f = fp12_conj(f, k);                                            // z < 0
    if (lane < 6) f2_store(f, out + g * 3 * FP12_WORDS + lane * COEF_WORDS);       // (the first of the final exponentiation's slots)
}

// The easy part, ^((q^6 - 1)(q^2 + 1)), with its one inversion; the slots of item g (this lane's coefficient in each, no other lane
// reads them): s0 holds f on entry and m^3 on exit, s1 m.  A kernel of its own: the inversion (fq_inv's 256 + 112 registers, one wave)
// stays out of the hard part's chain (two waves, and nearly all of the time).
__global__ __launch_bounds__(256) void final_exp_easy_kernel(uint64_t n, uint32_t *__restrict__ stash, const uint32_t *__restrict__ frob,
                                                             const int32_t *__restrict__ status, const int32_t *__restrict__ skip)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int lane = threadIdx.x & 7, k = lane < 6 ? lane : lane - 6;
    if (g >= n || (skip && *skip) || (status && status[g])) return;
    uint32_t *s0 = stash + (g * 3 + 0) * FP12_WORDS + k * COEF_WORDS, *s1 = s0 + FP12_WORDS;
    F2 m;
    {
        // ^(q^6 - 1) = conj(f) / f = conj(f)^2 h^(q^2) h^(q^4) / N, h = f conj(f) in Fq6, N = h h^(q^2) h^(q^4) in Fq2 (lane 0)
        const F2 f = f2_load(s0);
        const F2 fc = fp12_conj(f, k);
        const F2 h = fp12_mul(f, fc, k);
        const F2 h2 = fp12_frob(h, 2, frob, k);
        const F2 t = fp12_mul(h2, fp12_frob(h2, 2, frob, k), k);
        const F2 nrm = grp_shfl(fp12_mul(h, t, k), 0);
        const Fq29 d = fq_inv(fq_add(fq_sqr(nrm.c0), fq_sqr(nrm.c1)));
        F2 ninv; ninv.c0 = fq_mul(nrm.c0, d); ninv.c1 = fq_mul(fq_neg<256>(nrm.c1), d);
        m = fq2_mul(fp12_mul(fp12_mul(fc, fc, k), t, k), ninv);
    }
    m = fp12_mul(fp12_frob(m, 2, frob, k), m, k);                   // ^(q^2 + 1)
    // (lanes 6 and 7 compute what lanes 0 and 1 do, from the same sources: they store the same words)
    f2_store(m, s1);
    f2_store(fp12_mul(fp12_mul(m, m, k), m, k), s0);                // m^3
}

// The hard part after final_exp_easy_kernel, then
// mode: FE_COMPARE  accepted[g] = status ? -1 : degenerate (flags bit 1 with pair 0 active) ? -1 : passed && *passed ? 1 (the batched
//                   check decided it) : the value == target
//       FE_IS_ONE   accepted[g] = the value == 1 (the batched check)
//       FE_VALUE    out_words[g][72]: the value in frw_diag_pairing's basis (ark-ff bytes)
enum { FE_COMPARE = 0, FE_VALUE = 1, FE_IS_ONE = 2 };
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void final_exp_hard_kernel(
    uint64_t n, uint32_t *__restrict__ stash, const uint32_t *__restrict__ frob, const uint32_t *__restrict__ target, int mode,
    const int32_t *__restrict__ status, const int32_t *__restrict__ flags, const int32_t *__restrict__ passed, int32_t *__restrict__ accepted,
    uint64_t *__restrict__ out_words)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int lane = threadIdx.x & 7, k = lane < 6 ? lane : lane - 6;
    if (g >= n) return;
    if (mode == FE_COMPARE) {
        const int32_t st = status ? status[g] : 0;
        const int32_t fl = flags ? flags[g] : 0;
        if (st || (fl & 3) == 2 || (passed && *passed)) {
            if (lane == 0) accepted[g] = st || (fl & 3) == 2 ? -1 : 1;
            return;
        }
    }
    uint32_t *s0 = stash + (g * 3 + 0) * FP12_WORDS + k * COEF_WORDS, *s1 = s0 + FP12_WORDS, *s2 = s1 + FP12_WORDS;
    // the hard part, frw_pairing.h's chain: l3 = (z - 1)^2, l2 = l3 z, l1 = l2 z - l3, l0 = l1 z + 3
    f2_store(fp12_mul_lds(cyclotomic_exp_z(s1, k), fp12_conj(f2_load(s1), k), k), s1);      // t0 = m^(z - 1)
    f2_store(fp12_mul_lds(cyclotomic_exp_z(s1, k), fp12_conj(f2_load(s1), k), k), s1);      // a = t0^(z - 1) = m^l3
    f2_store(cyclotomic_exp_z(s1, k), s2);                                              // b = a^z
    {
        const F2 c = fp12_mul_lds(cyclotomic_exp_z(s2, k), fp12_conj(f2_load(s1), k), k);   // c = b^z / a
        f2_store(fp12_mul_lds(fp12_frob(f2_load(s2), 2, frob, k), fp12_frob(f2_load(s1), 3, frob, k), k), s2);   // b^(q^2) a^(q^3)
        f2_store(c, s1);
    }
    const F2 d = fp12_mul_lds(cyclotomic_exp_z(s1, k), f2_load(s0), k);                    // d = c^z m^3
    const F2 r = fp12_mul_lds(fp12_mul_lds(d, fp12_frob(f2_load(s1), 1, frob, k), k), f2_load(s2), k);
    if (mode != FE_VALUE) {
        F2 want = f2_zero();
        if (mode == FE_COMPARE) want = f2_load(target + k * COEF_WORDS);
        else want.c0 = fq_select(lane == 0 || lane == 6, fq_const(FQ29_ONE), fq_zero());
        const bool eq = fq_is_zero(fq_sub<4>(r.c0, want.c0)) && fq_is_zero(fq_sub<4>(r.c1, want.c1));
        const uint64_t votes = __ballot(eq || lane >= 6);
        const uint32_t mine = (uint32_t)(votes >> ((threadIdx.x & 63) & ~7u)) & 0xffu;
        if (lane == 0) accepted[g] = mine == 0xffu ? 1 : 0;
    } else if (lane < 6) {
        // a v^i w^j = a w^k = (a0 - a1) w^k + a1 w^(k + 6)  (u = w^6 - 1)
        uint64_t *o = out_words + g * 72;
        fq_to_ark(fq_sub<256>(r.c0, r.c1), (uint32_t *)(o + 6 * k));
        fq_to_ark(r.c1, (uint32_t *)(o + 6 * (k + 6)));
    }
}

// B of item g (24 words at b + g * bstride) -> its line table; flags[g]: bit 0 the pair is inactive (A at a + g * astride, or B, is
// infinity), bit 1 some denominator was zero.  Two lanes per item.
__global__ __launch_bounds__(64) void g2_lines_kernel(uint64_t n, const uint64_t *__restrict__ b, uint64_t bstride, const uint64_t *__restrict__ a,
                                                      uint64_t astride, const int32_t *__restrict__ status, uint32_t *__restrict__ tables,
                                                      int32_t *__restrict__ flags)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 64 + threadIdx.x) >> 1;
    if (g >= n) return;
    const uint64_t *bw = b + g * bstride, *aw = a + g * astride;
    uint64_t bany = 0, aany = 0;
    for (int i = 0; i < 24; i++) bany |= bw[i];
    for (int i = 0; i < 12; i++) aany |= aw[i];
    const bool odd = threadIdx.x & 1;
    if ((status && status[g]) || bany == 0 || aany == 0) {
        if (!odd) flags[g] = 1;
        return;
    }
    typedef Fq2PairField P;
    const P::El qx = P::from_ark((const uint32_t *)bw), qy = P::from_ark((const uint32_t *)(bw + 12));
    uint32_t *tab = tables + g * TABLE_WORDS;
    const bool degenerate = line_table<P>(qx, qy, [&](int line, int j, const P::El &c) {
        P::store(c, tab + line * LINE_WORDS + j * COEF_WORDS);
    });
    if (!odd) flags[g] = degenerate ? 2 : 0;
}

// a G2 point in ark-ff's bytes -> frw_pairing.h's strict form (what frw_verify.cpp's check_proof reads)
__device__ inline pairing::G2 g2_strict_from_ark(const uint64_t *w)
{
    pairing::G2 p;
    uint64_t any = 0;
    for (int k = 0; k < 24; k++) any |= w[k];
    p.inf = any == 0;
    p.x = pairing::fp2_from_ark(w);
    p.y = pairing::fp2_from_ark(w + 12);
    return p;
}
// status[g] = -1 where check_proof would refuse proof g.  Two lanes per proof: A (even lane) or C (odd lane), then B over both.
// (frw_rerand.hip's rerand_check_kernel is this kernel's twin: change them together.)
__global__ __launch_bounds__(64) void proof_check_kernel(uint64_t n, const uint64_t *__restrict__ proofs, int check_subgroup, int32_t *__restrict__ status)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 64 + threadIdx.x) >> 1;
    if (g >= n) return;
    const bool odd = threadIdx.x & 1;
    const uint64_t *pw = proofs + 48 * g;
    const uint64_t *mine = pw + (odd ? 36 : 0);
    bool ok = verify::coordinates_canonical(mine, 2) && verify::coordinates_canonical(pw + 12, 4);
    const G1Affine29 p = verify::g1_lazy_from_ark(mine);
    ok = ok && pairing::g1_on_curve(verify::g1_strict(p)) && pairing::g2_on_curve(g2_strict_from_ark(pw + 12));
    if (check_subgroup) {
        ok = ok && verify::in_subgroup(p);
        typedef Fq2PairField P;
        uint64_t any = 0;
        for (int i = 0; i < 24; i++) any |= pw[12 + i];
        AffineT<P> q;
        q.x = P::from_ark((const uint32_t *)(pw + 12));
        q.y = P::from_ark((const uint32_t *)(pw + 24));
        q.inf = any == 0;
        const bool sub = verify::in_subgroup(q);                    // (both lanes of the pair, whatever the G1 checks said)
        ok = ok && sub;
    }
    const uint32_t both = (ok ? 1u : 0u) & pair_swap_u32(ok ? 1u : 0u);
    if (!odd && !both) status[g] = -1;
}

// ---- the batched check ----------------------------------------------------------------------------------------------------------------
// A G1 point in XYZZ coordinates as the batched kernels keep it in memory: x | y | zz | zzz limbs, then the infinity flag
constexpr int XYZZ_WORDS = 4 * NLQ + 4;
__device__ __forceinline__ void xyzz_store(const G1Xyzz &p, uint32_t *w)
{
    FqField::store(p.x, w); FqField::store(p.y, w + NLQ); FqField::store(p.zz, w + 2 * NLQ); FqField::store(p.zzz, w + 3 * NLQ);
    w[4 * NLQ] = p.inf ? 1u : 0u;
}
__device__ __forceinline__ G1Xyzz xyzz_load(const uint32_t *w)
{
    G1Xyzz p;
    p.x = FqField::load(w); p.y = FqField::load(w + NLQ); p.zz = FqField::load(w + 2 * NLQ); p.zzz = FqField::load(w + 3 * NLQ);
    p.inf = w[4 * NLQ] != 0;
    return p;
}
// k P for a k of `words` 64-bit words
__device__ inline G1Xyzz g1_ladder(const G1Affine29 &p, const uint64_t *k, int words)
{
    G1Xyzz acc = g1_identity();
#pragma nounroll
    for (int bit = 64 * words - 1; bit >= 0; bit--) {
        acc = g1_double(acc);
        if ((k[bit >> 6] >> (bit & 63)) & 1ull) acc = g1_add_affine(acc, p);
    }
    return acc;
}
__device__ inline void g1_store_ark(const G1Xyzz &p, uint64_t *w)
{
    const G1Affine29 a = g1_to_affine(p);
    if (a.inf) { for (int i = 0; i < 12; i++) w[i] = 0; return; }
    fq_to_ark(a.x, (uint32_t *)w);
    fq_to_ark(a.y, (uint32_t *)(w + 6));
}
struct Seed { uint64_t w[4]; };
// rho_g = SHAKE256(seed || le64(first + g) || the proof's 384 bytes), its first 128 bits (one if they are all zero); then rho A (affine,
// ark-ff's bytes), rho P and rho C (XYZZ) for the sums.  A proof the check leaves out (status != 0, or a degenerate loop) gets rho = 0.
__global__ __launch_bounds__(64) void batch_scalar_kernel(uint64_t n, uint64_t first, Seed seed, const uint64_t *__restrict__ proofs,
                                                          const uint64_t *__restrict__ prepared, const int32_t *__restrict__ status,
                                                          const int32_t *__restrict__ flags, uint64_t *__restrict__ rho,
                                                          uint64_t *__restrict__ rho_a, uint32_t *__restrict__ rho_pc)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= n) return;
    const uint64_t *pw = proofs + 48 * g;
    uint64_t r[2] = {0, 0};
    if (!status[g] && (flags[g] & 3) != 2) {
        // the message is 53 words: seed (4) | index (1) | proof (48); rate 17 words, so three blocks and a last one of two words
        uint64_t a[25];
        for (int i = 0; i < 25; i++) a[i] = 0;
#pragma nounroll
        for (int blk = 0; blk < 4; blk++) {
            for (int i = 0; i < 17; i++) {
                const int m = 17 * blk + i;
                if (m < 53) a[i] ^= m < 4 ? seed.w[m] : m == 4 ? first + g : pw[m - 5];
            }
            if (blk == 3) { a[2] ^= 0x1full; a[16] ^= 0x80ull << 56; }     // SHAKE's domain bits and the last bit of the rate
            keccak_f1600(a);
        }
        r[0] = a[0]; r[1] = a[1];
        if ((r[0] | r[1]) == 0) r[0] = 1;
    }
    rho[2 * g] = r[0]; rho[2 * g + 1] = r[1];
    g1_store_ark(g1_ladder(verify::g1_lazy_from_ark(pw), r, 2), rho_a + 12 * g);
    xyzz_store(g1_ladder(verify::g1_lazy_from_ark(prepared + 12 * g), r, 2), rho_pc + (2 * g) * XYZZ_WORDS);
    xyzz_store(g1_ladder(verify::g1_lazy_from_ark(pw + 36), r, 2), rho_pc + (2 * g + 1) * XYZZ_WORDS);
}
// One block: sum rho_i P_i, sum rho_i C_i, sum rho_i over the pass, then the pairs of the fixed points: fixed[0..2] = the two sums
// and -(sum rho_i) alpha, affine, ark-ff's bytes
constexpr int SUM_THREADS = 128;
__global__ __launch_bounds__(SUM_THREADS) void batch_sum_kernel(uint64_t n, const uint64_t *__restrict__ rho, const uint32_t *__restrict__ rho_pc,
                                                                const uint64_t *__restrict__ alpha, uint64_t *__restrict__ fixed)
{
    __shared__ uint32_t part[SUM_THREADS * XYZZ_WORDS];
    __shared__ uint64_t rs[SUM_THREADS][3];
    const int t = threadIdx.x;
    uint64_t s0 = 0, s1 = 0, s2 = 0;
    for (uint64_t i = t; i < n; i += SUM_THREADS) {
        const uint64_t lo = s0 + rho[2 * i];
        const uint64_t c0 = lo < s0;
        const uint64_t mid = s1 + rho[2 * i + 1] + c0;
        s2 += (mid < s1 || (c0 && mid == s1)) ? 1 : 0;
        s0 = lo; s1 = mid;
    }
    rs[t][0] = s0; rs[t][1] = s1; rs[t][2] = s2;
    for (int which = 0; which < 2; which++) {
        G1Xyzz acc = g1_identity();
        for (uint64_t i = t; i < n; i += SUM_THREADS) acc = g1_add(acc, xyzz_load(rho_pc + (2 * i + which) * XYZZ_WORDS));
        xyzz_store(acc, part + t * XYZZ_WORDS);
        __syncthreads();
        for (int half = SUM_THREADS / 2; half > 0; half >>= 1) {
            if (t < half) xyzz_store(g1_add(xyzz_load(part + t * XYZZ_WORDS), xyzz_load(part + (t + half) * XYZZ_WORDS)), part + t * XYZZ_WORDS);
            __syncthreads();
        }
        if (t == 0) g1_store_ark(xyzz_load(part), fixed + 12 * which);
        __syncthreads();
    }
    if (t == 0) {
        uint64_t a = 0, b = 0, c = 0;
        for (int i = 0; i < SUM_THREADS; i++) {
            const uint64_t lo = a + rs[i][0];
            const uint64_t c0 = lo < a;
            const uint64_t mid = b + rs[i][1] + c0;
            c += rs[i][2] + ((mid < b || (c0 && mid == b)) ? 1 : 0);
            a = lo; b = mid;
        }
        const uint64_t k[3] = {a, b, c};
        G1Xyzz sa = g1_ladder(verify::g1_lazy_from_ark(alpha), k, 3);
        if (!sa.inf) sa.y = fq_neg<16>(sa.y);                       // (Y < 6 q)
        g1_store_ark(sa, fixed + 24);
    }
}
// f[a] <- f[a] f[a + step] for a = 2 step g (the slot-0 values of items; one level of the product tree)
__global__ __launch_bounds__(256) void fp12_tree_kernel(uint64_t n, uint64_t step, uint32_t *__restrict__ stash)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int lane = threadIdx.x & 7, k = lane < 6 ? lane : lane - 6;
    const uint64_t a = 2 * step * g, b = a + step;
    if (b >= n) return;
    uint32_t *fa = stash + a * 3 * FP12_WORDS + k * COEF_WORDS;
    const F2 r = fp12_mul(f2_load(fa), f2_load(stash + b * 3 * FP12_WORDS + k * COEF_WORDS), k);
    if (lane < 6) f2_store(r, fa);
}
// *all = *pass (first pass) or *all & *pass
__global__ void batch_and_kernel(const int32_t *pass, int32_t *all, int first)
{
    if (threadIdx.x == 0) *all = first ? *pass : (*all & *pass);
}

inline unsigned grid(uint64_t threads, unsigned block) { return (unsigned)((threads + block - 1) / block); }

}  // namespace

// ---- the key's part: -gamma, -delta, beta's tables, Frobenius constants, e(alpha, beta)^3 ------------------------------------------------
namespace {
using namespace frw::pairing;
void put_fp2(const Fp2 &a, uint32_t *w)
{
    for (int i = 0; i < NLQ; i++) { w[i] = a.c0.v.l[i]; w[NLQ + i] = a.c1.v.l[i]; }
}
// host Fq12 (tower) -> the lane layout: coefficient of w^(2 i + j) = c_j.c_i
void put_fp12(const Fp12 &a, uint32_t *w)
{
    const Fp2 *coef[6] = {&a.c0.c0, &a.c1.c0, &a.c0.c1, &a.c1.c1, &a.c0.c2, &a.c1.c2};
    for (int k = 0; k < 6; k++) put_fp2(*coef[k], w + k * COEF_WORDS);
}
void put_frobenius(const FrobeniusConstants &fc, uint32_t *w)
{
    for (int k = 0; k < 6; k++) {
        const Fp2 g1 = fc.gamma[k], g2 = fp2_mul(fp2_conj(g1), g1), g3 = fp2_mul(fp2_conj(g2), g1);
        put_fp2(g1, w + (0 * 6 + k) * COEF_WORDS);
        put_fp2(g2, w + (1 * 6 + k) * COEF_WORDS);
        put_fp2(g3, w + (2 * 6 + k) * COEF_WORDS);
    }
}
Fq2_29 lazy(const Fp2 &a) { Fq2_29 r; r.c0 = a.c0.v; r.c1 = a.c1.v; return r; }
void put_table(const G2 &q, uint32_t *w)
{
    (void)line_table<Fq2Field>(lazy(q.x), lazy(q.y), [&](int line, int j, const Fq2_29 &c) {
        Fq2Field::store(c, w + line * LINE_WORDS + j * COEF_WORDS);
    });
}
// the layout of vk->d_pairing (words): -gamma, -delta, beta's tables | Frobenius constants | e(alpha, beta)^3 | alpha (ark-ff's 12 words)
constexpr size_t KEY_TABLES = 0, KEY_FROB = 3 * (size_t)TABLE_WORDS, KEY_TARGET = KEY_FROB + 18 * COEF_WORDS, KEY_ALPHA = KEY_TARGET + FP12_WORDS,
                 KEY_WORDS = KEY_ALPHA + 24;
// per proof in flight: B's table, the flags, f and the final exponentiation's two other slots; with FRW_VERIFY_BATCHED also rho,
// rho A, rho P and rho C
constexpr size_t PROOF_BYTES = 4 * (size_t)TABLE_WORDS + 16 + 3 * 4 * (size_t)FP12_WORDS;
constexpr size_t BATCH_PROOF_BYTES = 16 + 96 + 2 * 4 * (size_t)XYZZ_WORDS;
// per pass with FRW_VERIFY_BATCHED: the fixed points' item (f and its slots), their three G1 points, the pass's verdict
constexpr size_t BATCH_PASS_BYTES = 3 * 4 * (size_t)FP12_WORDS + 3 * 96 + 16;
static_assert(PROOF_BYTES % 16 == 0 && BATCH_PROOF_BYTES % 16 == 0 && BATCH_PASS_BYTES % 16 == 0, "16-byte aligned parts");
}  // namespace

int upload_key(frw_groth16_vk *vk, const uint64_t *alpha_ark, const uint64_t *beta_ark)
{
    std::vector<uint32_t> w(KEY_WORDS);
    G2 beta;
    {
        uint64_t any = 0;
        for (int i = 0; i < 24; i++) any |= beta_ark[i];
        beta.inf = any == 0;
        beta.x = fp2_from_ark(beta_ark);
        beta.y = fp2_from_ark(beta_ark + 12);
    }
    const G2 *fixed[3] = {&vk->gamma_neg, &vk->delta_neg, &beta};
    unsigned inf = 0;
    for (int j = 0; j < 3; j++) {
        if (!fixed[j]->inf) put_table(*fixed[j], &w[KEY_TABLES + j * (size_t)TABLE_WORDS]);
        else inf |= 1u << j;                                        // (its pairs contribute one, as in frw_pairing.h's miller_loop)
    }
    put_frobenius(vk->fc, &w[KEY_FROB]);
    put_fp12(vk->alpha_beta, &w[KEY_TARGET]);
    std::memcpy(&w[KEY_ALPHA], alpha_ark, 96);
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, KEY_WORDS * 4);
    if (e == hipSuccess) e = hipMemcpy(d, w.data(), KEY_WORDS * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return record_hip_error(e, "frw_groth16_vk_load_dev");
    }
    vk->d_pairing = (uint32_t *)d;
    vk->pairing_inf = inf;
    return FRW_OK;
}

size_t proof_workspace_bytes(int flags) { return PROOF_BYTES + ((flags & FRW_VERIFY_BATCHED) ? BATCH_PROOF_BYTES : 0); }
size_t pass_workspace_bytes(int flags) { return (flags & FRW_VERIFY_BATCHED) ? BATCH_PASS_BYTES : 0; }

int verify_proofs(const frw_groth16_vk *vk, size_t cnt, size_t first, const uint64_t *d_proofs, const uint64_t *d_prepared, int32_t *d_status,
                  int flags, const uint64_t *seed, int32_t *d_accepted, int32_t *d_batch_passed, void *d_ws, hipStream_t st)
{
    const bool batched = flags & FRW_VERIFY_BATCHED;
    uint32_t *tables = (uint32_t *)d_ws;
    int32_t *bflags = (int32_t *)(tables + cnt * TABLE_WORDS);
    uint32_t *f = (uint32_t *)((char *)bflags + ((4 * cnt + 15) & ~(size_t)15));   // cnt items (+ the fixed points' item, batched)
    char *next = (char *)(f + (cnt + (batched ? 1 : 0)) * 3 * FP12_WORDS);
    const uint32_t *key = vk->d_pairing;
    const unsigned inf = vk->pairing_inf;
    hipLaunchKernelGGL(proof_check_kernel, dim3(grid(2 * cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, d_proofs,
                       (flags & FRW_VERIFY_POINTS_ARE_CHECKED) ? 0 : 1, d_status);
    hipLaunchKernelGGL(g2_lines_kernel, dim3(grid(2 * cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, d_proofs + 12, (uint64_t)48, d_proofs,
                       (uint64_t)48, d_status, tables, bflags);
    int32_t *d_pass = nullptr;
    if (batched) {
        // Pi e(rho_i A_i, B_i) e(sum rho_i P_i, -gamma) e(sum rho_i C_i, -delta) e(-(sum rho_i) alpha, beta) == 1, one final exponentiation
        uint64_t *rho = (uint64_t *)next, *rho_a = rho + 2 * cnt;
        uint32_t *rho_pc = (uint32_t *)(rho_a + 12 * cnt);
        uint64_t *fixed = (uint64_t *)(rho_pc + 2 * cnt * XYZZ_WORDS);
        d_pass = (int32_t *)(fixed + 36);
        Seed sd;
        for (int i = 0; i < 4; i++) sd.w[i] = seed[i];
        hipLaunchKernelGGL(batch_scalar_kernel, dim3(grid(cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, (uint64_t)first, sd, d_proofs, d_prepared,
                           (const int32_t *)d_status, (const int32_t *)bflags, rho, rho_a, rho_pc);
        hipLaunchKernelGGL(batch_sum_kernel, dim3(1), dim3(SUM_THREADS), 0, st, (uint64_t)cnt, (const uint64_t *)rho, (const uint32_t *)rho_pc,
                           (const uint64_t *)(key + KEY_ALPHA), fixed);
        MillerPairs one;
        one.npairs = 1;
        one.p[0] = rho_a; one.pstride[0] = 12; one.table[0] = tables; one.tstride[0] = TABLE_WORDS;
        for (int j = 1; j < 3; j++) { one.p[j] = nullptr; one.pstride[j] = 0; one.table[j] = nullptr; one.tstride[j] = 0; }
        hipLaunchKernelGGL(miller_kernel, dim3(grid(8 * cnt, 256)), dim3(256), 0, st, (uint64_t)cnt, one, 0u, (const int32_t *)d_status,
                           (const int32_t *)bflags, (const int32_t *)nullptr, 1, f);
        MillerPairs fx;
        fx.npairs = 3;
        for (int j = 0; j < 3; j++) { fx.p[j] = fixed + 12 * j; fx.pstride[j] = 0; fx.table[j] = key + KEY_TABLES + j * TABLE_WORDS; fx.tstride[j] = 0; }
        hipLaunchKernelGGL(miller_kernel, dim3(1), dim3(256), 0, st, (uint64_t)1, fx, inf, (const int32_t *)nullptr, (const int32_t *)nullptr,
                           (const int32_t *)nullptr, 0, f + cnt * 3 * FP12_WORDS);
        for (uint64_t step = 1; step < cnt + 1; step *= 2)
            hipLaunchKernelGGL(fp12_tree_kernel, dim3(grid(8 * ((cnt + 1 + 2 * step - 1) / (2 * step)), 256)), dim3(256), 0, st, (uint64_t)(cnt + 1),
                               step, f);
        hipLaunchKernelGGL(final_exp_easy_kernel, dim3(1), dim3(256), 0, st, (uint64_t)1, f, key + KEY_FROB, (const int32_t *)nullptr,
                           (const int32_t *)nullptr);
        hipLaunchKernelGGL(final_exp_hard_kernel, dim3(1), dim3(256), 0, st, (uint64_t)1, f, key + KEY_FROB, (const uint32_t *)nullptr, (int)FE_IS_ONE,
                           (const int32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, d_pass, (uint64_t *)nullptr);
        if (d_batch_passed)
            hipLaunchKernelGGL(batch_and_kernel, dim3(1), dim3(64), 0, st, (const int32_t *)d_pass, d_batch_passed, first == 0 ? 1 : 0);
    }
    // per proof: the whole work when the batched check failed or was not asked for; returns at once where it passed
    MillerPairs mp;
    mp.npairs = 3;
    mp.p[0] = d_proofs;      mp.pstride[0] = 48; mp.table[0] = tables;                           mp.tstride[0] = TABLE_WORDS;
    mp.p[1] = d_prepared;    mp.pstride[1] = 12; mp.table[1] = key + KEY_TABLES;                 mp.tstride[1] = 0;
    mp.p[2] = d_proofs + 36; mp.pstride[2] = 48; mp.table[2] = key + KEY_TABLES + TABLE_WORDS;   mp.tstride[2] = 0;
    hipLaunchKernelGGL(miller_kernel, dim3(grid(8 * cnt, 256)), dim3(256), 0, st, (uint64_t)cnt, mp, (inf & 3u) << 1, (const int32_t *)d_status,
                       (const int32_t *)bflags, (const int32_t *)d_pass, 0, f);
    hipLaunchKernelGGL(final_exp_easy_kernel, dim3(grid(8 * cnt, 256)), dim3(256), 0, st, (uint64_t)cnt, f, key + KEY_FROB, (const int32_t *)d_status,
                       (const int32_t *)d_pass);
    hipLaunchKernelGGL(final_exp_hard_kernel, dim3(grid(8 * cnt, 256)), dim3(256), 0, st, (uint64_t)cnt, f, key + KEY_FROB, key + KEY_TARGET,
                       (int)FE_COMPARE, (const int32_t *)d_status, (const int32_t *)bflags, (const int32_t *)d_pass, d_accepted, (uint64_t *)nullptr);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : record_hip_error(e, "frw_groth16_verify_full_dev");
}

}  // namespace pairing_dev
}  // namespace frw

// ---- diagnostics: frw_diag_pairing for `count` pairs at once (host buffers; allocates, synchronises) -----------------------------------
extern "C" int frw_diag_pairing_dev(int device, size_t count, const uint64_t *g1, const uint64_t *g2, uint64_t *out)
{
    using namespace frw::pairing_dev;
    if (count && (!g1 || !g2 || !out)) return FRW_E_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    if (count == 0) return FRW_OK;
    // the host's refusals: coordinates are taken as they come (canonical or not), points must lie on their curves
    for (size_t i = 0; i < count; i++) {
        const frw::pairing::G1 p = frw::verify::g1_strict(frw::verify::g1_lazy_from_ark(g1 + 12 * i));
        frw::pairing::G2 q;
        uint64_t any = 0;
        for (int k = 0; k < 24; k++) any |= g2[24 * i + k];
        q.inf = any == 0;
        q.x = frw::pairing::fp2_from_ark(g2 + 24 * i);
        q.y = frw::pairing::fp2_from_ark(g2 + 24 * i + 12);
        if (!frw::pairing::g1_on_curve(p) || !frw::pairing::g2_on_curve(q)) return FRW_E_INVALID_ARG;
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    std::vector<uint32_t> frob(18 * COEF_WORDS);
    {
        const frw::pairing::FrobeniusConstants fc = frw::pairing::frobenius_constants();
        for (int k = 0; k < 6; k++) {
            using namespace frw::pairing;
            const Fp2 a = fc.gamma[k], b = fp2_mul(fp2_conj(a), a), c = fp2_mul(fp2_conj(b), a);
            const Fp2 *all[3] = {&a, &b, &c};
            for (int j = 0; j < 3; j++)
                for (int i = 0; i < frw::NLQ; i++) {
                    frob[(j * 6 + k) * COEF_WORDS + i] = all[j]->c0.v.l[i];
                    frob[(j * 6 + k) * COEF_WORDS + frw::NLQ + i] = all[j]->c1.v.l[i];
                }
        }
    }
    const size_t in_bytes = count * 36 * 8, tab_bytes = count * (size_t)TABLE_WORDS * 4, f_bytes = count * 3 * (size_t)FP12_WORDS * 4;
    const size_t bytes = in_bytes + tab_bytes + f_bytes + count * 4 + frob.size() * 4 + count * 72 * 8;
    char *d = nullptr;
    e = hipMalloc((void **)&d, bytes);
    if (e != hipSuccess) return frw::record_hip_error(e, "frw_diag_pairing_dev");
    uint64_t *d_g1 = (uint64_t *)d, *d_g2 = d_g1 + 12 * count;
    uint32_t *d_tab = (uint32_t *)(d + in_bytes), *d_f = (uint32_t *)(d + in_bytes + tab_bytes);
    int32_t *d_flags = (int32_t *)(d + in_bytes + tab_bytes + f_bytes);
    uint32_t *d_frob = (uint32_t *)(d_flags + count);
    uint64_t *d_out = (uint64_t *)(d_frob + frob.size());
    e = hipMemcpy(d_g1, g1, count * 96, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_g2, g2, count * 192, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_frob, frob.data(), frob.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        using namespace frw::pairing_dev;
        hipLaunchKernelGGL(g2_lines_kernel, dim3(grid(2 * count, 64)), dim3(64), 0, nullptr, (uint64_t)count, (const uint64_t *)d_g2, (uint64_t)24,
                           (const uint64_t *)d_g1, (uint64_t)12, (const int32_t *)nullptr, d_tab, d_flags);
        MillerPairs mp;
        mp.npairs = 1;
        mp.p[0] = d_g1; mp.pstride[0] = 12; mp.table[0] = d_tab; mp.tstride[0] = TABLE_WORDS;
        for (int j = 1; j < 3; j++) { mp.p[j] = nullptr; mp.pstride[j] = 0; mp.table[j] = nullptr; mp.tstride[j] = 0; }
        hipLaunchKernelGGL(miller_kernel, dim3(grid(8 * count, 256)), dim3(256), 0, nullptr, (uint64_t)count, mp, 0u, (const int32_t *)nullptr,
                           (const int32_t *)d_flags, (const int32_t *)nullptr, 0, d_f);
        hipLaunchKernelGGL(final_exp_easy_kernel, dim3(grid(8 * count, 256)), dim3(256), 0, nullptr, (uint64_t)count, d_f, (const uint32_t *)d_frob,
                           (const int32_t *)nullptr, (const int32_t *)nullptr);
        hipLaunchKernelGGL(final_exp_hard_kernel, dim3(grid(8 * count, 256)), dim3(256), 0, nullptr, (uint64_t)count, d_f,
                           (const uint32_t *)d_frob, (const uint32_t *)nullptr, (int)FE_VALUE, (const int32_t *)nullptr,
                           (const int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, count * 72 * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_diag_pairing_dev");
}
