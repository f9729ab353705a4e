// frw_rerand.h -- re-randomising a Groth16 proof: ark-groth16 0.3.0 prover.rs, rerandomize_proof(rng, vk, proof), restated from the
// crate's source (parity unpinned, as everywhere in DESIGN.md section 3; what the tests pin is the group arithmetic):
//     A' = r1^-1 A            B' = r1 B + (r1 r2) delta_g2            C' = C + r2 A
// with the two factors supplied by the caller (any 256-bit values, taken modulo the group order r; zero is refused).  What the host
// function (frw_groth16_rerandomize) and the device kernels (frw_rerand.hip) share, so that both run ONE restatement and give the same
// affine points bit for bit: the arithmetic on the factors, the proof points' checks, the three scalar-multiplication chains and the
// conversion to ark-ff's limbs.  The host runs them over Fq2Field, the device over Fq2PairField (two lanes per G2 point); an affine
// point has one representation, so the results do not depend on which.
//
// Every addition below is one of the COMPLETE formulas of frw_fq29.h (pt_add_affine: equal operands double, opposite ones cancel, the
// identity on either side is handled): B = r2 delta_g2 (equal summands in B'), B = -r2 delta_g2 (B' = O), C = r2 A (a doubling in C'),
// C = -r2 A (C' = O) and points at infinity need no code of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frw_fq29.h"
#include "frw_verify.h"

#define FRW_RR_HD __host__ __device__ inline

namespace frw {
namespace rerand {

// ---- the factors: integers modulo the group order r, four 64-bit words ------------------------------------------------------------------
// Plain 64-bit arithmetic, the same instructions on the host and in a lane: a proof needs one inversion, one product and two divisions
// by lambda, some 30,000 integer instructions beside the 5,000 field products of its ladders.
// NOT constant-time: fr_inv's trip counts and fr_mul's conditional additions depend on r1 and r2 (as do the ladders' additions, which
// follow the multipliers' bits) -- on the host, and across diverging lanes on the device.  The factors are secrets of whoever
// re-randomises; a fixed addition chain for r1^-1 would remove the inversion's share of that, not the ladders' (DESIGN.md 5.11).
FRW_RR_HD uint64_t r_word(int k)
{
    return k == 0 ? 0xffffffff00000001ULL : k == 1 ? 0x53bda402fffe5bfeULL : k == 2 ? 0x3339d80809a1d805ULL : 0x73eda753299d7d48ULL;
}
FRW_RR_HD bool u256_is_zero(const uint64_t *a) { return (a[0] | a[1] | a[2] | a[3]) == 0; }
FRW_RR_HD bool u256_is_one(const uint64_t *a) { return a[0] == 1 && (a[1] | a[2] | a[3]) == 0; }
FRW_RR_HD bool u256_ge(const uint64_t *a, const uint64_t *b)
{
    for (int j = 3; j >= 0; j--)
        if (a[j] != b[j]) return a[j] > b[j];
    return true;
}
FRW_RR_HD bool u256_ge_r(const uint64_t *a)
{
    for (int j = 3; j >= 0; j--)
        if (a[j] != r_word(j)) return a[j] > r_word(j);
    return true;
}
FRW_RR_HD void u256_sub(uint64_t *a, const uint64_t *b)             // a -= b (a >= b)
{
    uint64_t borrow = 0;
    for (int j = 0; j < 4; j++) {
        const uint64_t d = a[j] - b[j], d2 = d - borrow;
        borrow = (uint64_t)(a[j] < b[j]) | (uint64_t)(d < borrow);
        a[j] = d2;
    }
}
FRW_RR_HD void u256_sub_r(uint64_t *a)
{
    const uint64_t r[4] = {r_word(0), r_word(1), r_word(2), r_word(3)};
    u256_sub(a, r);
}
FRW_RR_HD void u256_add(uint64_t *a, const uint64_t *b)             // a += b (no overflow: the callers' sums are below 2^256)
{
    uint64_t carry = 0;
    for (int j = 0; j < 4; j++) {
        const uint64_t s = a[j] + b[j], s2 = s + carry;
        carry = (uint64_t)(s < a[j]) | (uint64_t)(s2 < s);
        a[j] = s2;
    }
}
FRW_RR_HD void u256_shr1(uint64_t *a)
{
    for (int j = 0; j < 4; j++) a[j] = (a[j] >> 1) | (j < 3 ? a[j + 1] << 63 : 0);
}
// any 256-bit value -> its residue below r (2^256 < 3 r: at most two subtractions)
FRW_RR_HD void fr_reduce(uint64_t *k)
{
    for (int round = 0; round < 2; round++)
        if (u256_ge_r(k)) u256_sub_r(k);
}
// a + b, a - b modulo r (operands below r; r < 2^255, so a + b fits)
FRW_RR_HD void fr_add(uint64_t *a, const uint64_t *b)
{
    u256_add(a, b);
    if (u256_ge_r(a)) u256_sub_r(a);
}
FRW_RR_HD void fr_sub(uint64_t *a, const uint64_t *b)
{
    if (!u256_ge(a, b)) {
        const uint64_t r[4] = {r_word(0), r_word(1), r_word(2), r_word(3)};
        u256_add(a, r);
    }
    u256_sub(a, b);
}
// x / 2 modulo r: (x + r) / 2 when x is odd
FRW_RR_HD void fr_halve(uint64_t *x)
{
    if (x[0] & 1ULL) {
        const uint64_t r[4] = {r_word(0), r_word(1), r_word(2), r_word(3)};
        u256_add(x, r);
    }
    u256_shr1(x);
}
// a b modulo r by doubling and adding over the 255 bits of b
FRW_RR_HD void fr_mul(const uint64_t *a, const uint64_t *b, uint64_t *out)
{
    uint64_t acc[4] = {0, 0, 0, 0};
    for (int bit = 254; bit >= 0; bit--) {
        fr_add(acc, acc);
        if ((b[bit >> 6] >> (bit & 63)) & 1ULL) fr_add(acc, a);
    }
    for (int j = 0; j < 4; j++) out[j] = acc[j];
}
// 1 / a modulo r, 0 < a < r: the binary extended Euclidean algorithm (u = x1 a, v = x2 a modulo r throughout; r is an odd prime, so one
// of u, v reaches 1).  Every pass of the outer loop takes at least one bit off u or v: 512 passes at most.
FRW_RR_HD void fr_inv(const uint64_t *a, uint64_t *out)
{
    uint64_t u[4] = {a[0], a[1], a[2], a[3]}, v[4] = {r_word(0), r_word(1), r_word(2), r_word(3)};
    uint64_t x1[4] = {1, 0, 0, 0}, x2[4] = {0, 0, 0, 0};
    for (int pass = 0; pass < 512 && !u256_is_one(u) && !u256_is_one(v); pass++) {
        while (!(u[0] & 1ULL) && !u256_is_zero(u)) { u256_shr1(u); fr_halve(x1); }
        while (!(v[0] & 1ULL) && !u256_is_zero(v)) { u256_shr1(v); fr_halve(x2); }
        if (u256_ge(u, v)) { u256_sub(u, v); fr_sub(x1, x2); }
        else { u256_sub(v, u); fr_sub(x2, x1); }
    }
    const bool from_u = u256_is_one(u);
    for (int j = 0; j < 4; j++) out[j] = from_u ? x1[j] : x2[j];
}
// k (below r) = k0 + lambda k1, lambda = z^2 - 1 = 0xac45a4010001a40200000000ffffffff and r = lambda^2 + lambda + 1: k0 = k mod lambda,
// k1 = k div lambda <= lambda + 1 < 2^128 -- the division frw_msm.hip's groth16_split_kernel makes of a blinding factor, so that
// k P = k0 P + k1 phi(P) is 128 doublings (frw_fq29.h: G1_ENDO_BETA29).  out: k0 (2 words) | k1 (2 words)
FRW_RR_HD void fr_split(const uint64_t *k, uint64_t *out)
{
    const uint64_t L0 = 0x00000000ffffffffULL, L1 = 0xac45a4010001a402ULL;
    uint64_t r0 = 0, r1 = 0, q0 = 0, q1 = 0;
    for (int bit = 255; bit >= 0; bit--) {
        const uint64_t top = r1 >> 63;
        r1 = (r1 << 1) | (r0 >> 63);
        r0 = (r0 << 1) | ((k[bit >> 6] >> (bit & 63)) & 1ULL);
        q1 = (q1 << 1) | (q0 >> 63);
        q0 <<= 1;
        if (top || r1 > L1 || (r1 == L1 && r0 >= L0)) {
            const uint64_t b = r0 < L0;
            r0 -= L0;
            r1 = r1 - L1 - b;
            q0 |= 1ULL;
        }
    }
    out[0] = r0; out[1] = r1; out[2] = q0; out[3] = q1;
}
// What the ladders of one proof read: the split halves of r1^-1 and of r2 (G1), then r1 and r1 r2 (G2), sixteen words.
constexpr int SCALAR_WORDS = 16;
enum { SC_INV_SPLIT = 0, SC_R2_SPLIT = 4, SC_R1 = 8, SC_R1R2 = 12 };
// factors: r1 | r2, four words each, any values.  0, or FRW_RERAND_ZERO_FACTOR where one of them is 0 modulo r (out is then untouched)
FRW_RR_HD int factors_prepare(const uint64_t *factors, uint64_t *out)
{
    uint64_t r1[4], r2[4], inv[4];
    for (int j = 0; j < 4; j++) { r1[j] = factors[j]; r2[j] = factors[4 + j]; }
    fr_reduce(r1);
    fr_reduce(r2);
    if (u256_is_zero(r1) || u256_is_zero(r2)) return FRW_RERAND_ZERO_FACTOR;
    fr_inv(r1, inv);
    fr_split(inv, out + SC_INV_SPLIT);
    fr_split(r2, out + SC_R2_SPLIT);
    for (int j = 0; j < 4; j++) out[SC_R1 + j] = r1[j];
    fr_mul(r1, r2, out + SC_R1R2);
    return 0;
}

// ---- the proof's points ------------------------------------------------------------------------------------------------------------------
// an affine point in ark-ff's limbs (all zero = the point at infinity) over either Fq2 policy: every lane of a pair reads the whole
// point for `inf`, and its own component of the coordinates
template <class F> FRW_RR_HD AffineT<F> load_ark(const uint64_t *w)
{
    AffineT<F> p;
    uint64_t any = 0;
    for (int k = 0; k < F::ARK_WORDS; k++) any |= w[k];
    p.inf = any == 0;
    p.x = F::from_ark((const uint32_t *)w);
    p.y = F::from_ark((const uint32_t *)w + F::ARK_WORDS);
    return p;
}
template <class F> FRW_RR_HD void store_ark(const AffineT<F> &a, uint64_t *w)
{
    if (a.inf) {
        for (int k = 0; k < F::ARK_WORDS; k++) w[k] = 0;        // (both lanes of a pair write the same zeros)
        return;
    }
    F::to_ark(a.x, (uint32_t *)w);
    F::to_ark(a.y, (uint32_t *)w + F::ARK_WORDS);
}
// The checks frw_groth16_verify makes of a proof's points (frw_verify.cpp check_proof, frw_pairing_dev.hip proof_check_kernel), by the
// same functions of frw_verify.h and frw_pairing.h, one point at a time: canonical limbs, on the curve, and -- unless the caller
// vouches for it -- in the subgroup of order r.  g2_point_ok<Fq2PairField> runs in both lanes of a pair and answers alike in both.
FRW_RR_HD bool g1_point_ok(const uint64_t *w, bool check_subgroup)
{
    if (!verify::coordinates_canonical(w, 2)) return false;
    const G1Affine29 p = verify::g1_lazy_from_ark(w);
    if (!pairing::g1_on_curve(verify::g1_strict(p))) return false;
    return !check_subgroup || verify::in_subgroup(p);
}
template <class F2> FRW_RR_HD bool g2_point_ok(const uint64_t *w, bool check_subgroup)
{
    if (!verify::coordinates_canonical(w, 4)) return false;
    pairing::G2 s;
    uint64_t any = 0;
    for (int k = 0; k < 24; k++) any |= w[k];
    s.inf = any == 0;
    s.x = pairing::fp2_from_ark(w);
    s.y = pairing::fp2_from_ark(w + 12);
    if (!pairing::g2_on_curve(s)) return false;
    return !check_subgroup || verify::in_subgroup(load_ark<F2>(w));
}

// Where a ladder keeps its addends.  In a lane they would be 70 (G1) or 56 (G2) live registers beside the running point and an
// addition's temporaries, and the kernels would spill; the device keeps them in LDS, a column per lane (frw_rerand.hip: LdsTable), and a
// step reads the one it adds.  The host keeps them where they are.
template <class El, int N> struct LocalTable {
    El v[N];
    __host__ __device__ void put(int i, const El &e) { v[i] = e; }
    __host__ __device__ El get(int i) const { return v[i]; }
};
// the top bit of a scalar of N words, which moves up by one: a ladder's bits without a register array indexed at run time
template <int N> FRW_RR_HD uint32_t take_top_bit(uint64_t (&k)[N])
{
    const uint32_t bit = (uint32_t)(k[N - 1] >> 63);
#pragma unroll
    for (int j = N - 1; j > 0; j--) k[j] = (k[j] << 1) | (k[j - 1] >> 63);
    k[0] <<= 1;
    return bit;
}

// k P + Q in G1, k = k0 + lambda k1 as fr_split leaves it (split: k0 | k1, two words each): 128 steps of one doubling and at most one
// mixed addition of P, phi(P) = (beta x, y) or P + phi(P) = (-(1 + beta) x, -y) -- the two have the same y, their chord is horizontal
// (frw_quad.h) -- the addend's coordinates selected, so that the loop holds ONE addition.  For P outside the subgroup (a point vouched
// for wrongly) phi(P) is not lambda P and the result is some other point of the curve: unspecified, but the same every time.
// tab: five elements -- x, beta x, -(1 + beta) x, y, -y.
template <class Tab> FRW_RR_HD G1Xyzz g1_multiple_plus(Tab &tab, const G1Affine29 &p, const uint64_t *split, const G1Affine29 &q)
{
    G1Xyzz acc = g1_identity();
    if (!p.inf) {
        const Fq29 one = fq_const(FQ29_ONE);
        const Fq29 ex = fq_mul(p.x, fq_const(G1_ENDO_BETA29));                                // < 2 q
        tab.put(0, p.x);
        tab.put(1, ex);
        tab.put(2, fq_mul(fq_neg<4>(fq_add(p.x, ex)), one));                                  // (p.x, p.y < 2 q)
        tab.put(3, p.y);
        tab.put(4, fq_mul(fq_neg<4>(p.y), one));
    }
    uint64_t k0[2] = {split[0], split[1]}, k1[2] = {split[2], split[3]};
    // step 128 adds Q: the loop's one addition serves it too (a second copy of the formula, with the doubling inside it, is what made
    // the kernel keep its points in scratch memory)
#pragma nounroll
    for (int step = p.inf ? 128 : 0; step <= 128; step++) {
        G1Affine29 t;
        if (step < 128) {
            acc = g1_double(acc);
            const uint32_t b0 = take_top_bit(k0), b1 = take_top_bit(k1);
            const uint32_t sel = b0 | (b1 << 1);
            if (sel == 0) continue;
            t.inf = false;
            t.x = tab.get(sel - 1);
            t.y = tab.get(sel == 3 ? 4 : 3);
        } else {
            t = q;
        }
        acc = g1_add_affine(acc, t);
    }
    return acc;
}
// k1 P1 + k2 P2 in G2 over either Fq2 policy (k1, k2 below r < 2^255, four words each): 255 steps of one doubling and the mixed additions
// of P1 and / or P2 where their bits are set, through ONE addition in the loop (a precomputed P1 + P2 would save a quarter of the
// additions and cost an inversion, or the full addition as a second formula, inside the kernel whose registers are the scarce thing).
// tab: four elements -- P1's x, y, P2's x, y.
template <class F2, class Tab>
FRW_RR_HD XyzzT<F2> g2_double_multiple(Tab &tab, const AffineT<F2> &p1, const uint64_t *s1, const AffineT<F2> &p2, const uint64_t *s2)
{
    tab.put(0, p1.x); tab.put(1, p1.y); tab.put(2, p2.x); tab.put(3, p2.y);
    const bool inf1 = p1.inf, inf2 = p2.inf;
    uint64_t k1[4] = {s1[0], s1[1], s1[2], s1[3]}, k2[4] = {s2[0], s2[1], s2[2], s2[3]};
    (void)take_top_bit(k1);                                                                  // bit 255 is zero
    (void)take_top_bit(k2);
    XyzzT<F2> acc = pt_identity<F2>();
#pragma nounroll
    for (int step = 0; step < 255; step++) {
        acc = pt_double(acc);
        const uint32_t b1 = take_top_bit(k1), b2 = take_top_bit(k2);
        const uint32_t sel = b1 | (b2 << 1);
#pragma nounroll
        for (uint32_t which = 0; which < 2; which++) {
            if (!((sel >> which) & 1u)) continue;
            AffineT<F2> t;
            t.inf = which ? inf2 : inf1;
            t.x = tab.get(2 * which);
            t.y = tab.get(2 * which + 1);
            acc = pt_add_affine(acc, t);
        }
    }
    return acc;
}

// One proof from end to end in one thread: the host function, and what the tests hold the kernels to.  proof, out: 48 words (they may
// be the same 48: the proof is read whole before `out` is written); delta: vk.delta_g2 in ark-ff's limbs.  Returns the status; a
// refused proof's output is all zero.
template <class F2> inline int rerandomize_one(const uint64_t *proof, const uint64_t *factors, const uint64_t *delta, bool check_subgroup, uint64_t *out)
{
    uint64_t sc[SCALAR_WORDS], res[48];
    int st = g1_point_ok(proof, check_subgroup) && g2_point_ok<F2>(proof + 12, check_subgroup) && g1_point_ok(proof + 36, check_subgroup) ? 0 : -1;
    if (st == 0) st = factors_prepare(factors, sc);
    if (st != 0) {
        for (int k = 0; k < 48; k++) out[k] = 0;
        return st;
    }
    const G1Affine29 a = load_ark<FqField>(proof), c = load_ark<FqField>(proof + 36);
    G1Affine29 none = a;
    none.inf = true;
    LocalTable<Fq29, 5> t1;
    LocalTable<typename F2::El, 4> t2;
    store_ark<FqField>(g1_to_affine(g1_multiple_plus(t1, a, sc + SC_INV_SPLIT, none)), res);
    store_ark<F2>(pt_to_affine(g2_double_multiple<F2>(t2, load_ark<F2>(proof + 12), sc + SC_R1, load_ark<F2>(delta), sc + SC_R1R2)), res + 12);
    store_ark<FqField>(g1_to_affine(g1_multiple_plus(t1, a, sc + SC_R2_SPLIT, c)), res + 36);
    for (int k = 0; k < 48; k++) out[k] = res[k];
    return 0;
}

// the key's part on the device (frw_rerand.hip): delta_g2's limbs, uploaded by frw_groth16_vk_load_dev
int upload_key(frw_groth16_vk *vk);

}  // namespace rerand
}  // namespace frw
