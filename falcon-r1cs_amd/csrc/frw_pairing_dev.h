// frw_pairing_dev.h -- what the device pairing (frw_pairing_dev.hip) shares with the host code that prepares its fixed G2 points: the
// Miller loop's line coefficients in homogeneous projective coordinates on the twist, one formula for both sides.  The host runs it
// with Fq2Field (one lane, at key load: -gamma, -delta, beta), the device with Fq2PairField (two lanes per point: a proof's B).
//
// The Miller loop of frw_pairing.h, f <- f^2 l_T,T(P) for every bit of |z| below the top one and f <- f l_T,Q(P) for every set bit,
// without inversions: T = (X : Y : Z), and every line is the affine one scaled by a factor in Fq2 -- which the final exponentiation
// sends to one (a^(q^6 - 1) = 1 for a in Fq2), so values after it equal frw_pairing.h's bit for bit.  In the basis 1, w, .., w^5 of
// Fq12 = Fq2[w] / (w^6 - xi) a line has three coefficients (w = the tower's w, w^2 = v):
//     l = c0 + (c1 xP) w^2 + (c2 yP) w^3
// c0, c1, c2 in Fq2 depend on the G2 point only: a table of LINES lines per point, and per proof two Fq products per line at P.
//   tangent at T (dbl-1998-cmo-2, scaled by 2 Y Z^2):   c0 = 3 X^3 - 2 Y^2 Z   c1 = -3 X^2 Z   c2 = 2 Y Z^2
//   chord through T and Q (madd-1998-cmo, by v Z):      c0 = u X - Y v         c1 = -u Z       c2 = v Z     u = yQ Z - Y, v = xQ Z - X
// A zero denominator of the affine loop (the host's `degenerate`) is Y = 0 in a doubling and v = 0 in an addition.
#pragma once
#include "../../include/frw.h"
#include "frw_fq29.h"

namespace frw {
namespace pairing_dev {

constexpr uint64_t Z_ABS = 0xd201000000010000ull;            // |z|, as frw_pairing.h
constexpr int LINES = 63 + 5;                                // 63 doublings, 5 additions (the set bits of |z| below the top one)
constexpr int COEF_WORDS = 2 * NLQ;                          // one Fq2 coefficient: c0 limbs | c1 limbs
constexpr int LINE_WORDS = 3 * COEF_WORDS;                   // c0 | c1 | c2
constexpr int TABLE_WORDS = LINES * LINE_WORDS;              // 5,712 words = 22,848 bytes per G2 point
constexpr int FP12_WORDS = 6 * COEF_WORDS;                   // an Fq12 value, coefficient k of w^k at words 28 k

template <class F> struct ProjT { typename F::El x, y, z; };

// Bounds (units of q per component; products of either policy < 10 q, squares < 4 q): stored X < 20, Y < 74, Z < 80; the
// coefficients c0 < 74, c1 < 16, c2 < 20.  Operands of every product stay below 2^10 q.
template <class F> __host__ __device__ inline bool line_double(ProjT<F> &t, typename F::El (&c)[3])
{
    const bool vertical = F::is_zero(t.y);
    const auto xx = F::sqr(t.x);
    const auto w = F::add(F::add(xx, xx), xx);                   // 3 X^2
    const auto s = F::mul(t.y, t.z);                             // Y Z
    const auto b = F::mul(F::mul(t.x, t.y), s);                  // X Y S
    const auto ww = F::sqr(w);
    const auto b4 = F::add(F::add(b, b), F::add(b, b));
    const auto b8 = F::add(b4, b4);
    const auto h = F::template sub<256>(ww, b8);                 // W^2 - 8 B
    const auto ys = F::mul(t.y, s);
    const auto ys2 = F::sqr(ys);
    const auto ys2_2 = F::add(ys2, ys2), ys2_4 = F::add(ys2_2, ys2_2);
    c[0] = F::template sub<64>(F::mul(t.x, w), F::add(ys, ys));  // 3 X^3 - 2 Y^2 Z
    c[1] = F::template neg<16>(F::mul(w, t.z));
    const auto sz = F::mul(s, t.z);
    c[2] = F::add(sz, sz);
    const auto hs = F::mul(h, s);
    const auto s3 = F::mul(F::sqr(s), s);
    const auto s3_2 = F::add(s3, s3), s3_4 = F::add(s3_2, s3_2);
    // Y3 = W (4 B - H) - 8 Y^2 S^2, 4 B - H = 12 B - W^2
    t.y = F::template sub<64>(F::mul(w, F::template sub<16>(F::add(b8, b4), ww)), F::add(ys2_4, ys2_4));
    t.x = F::add(hs, hs);
    t.z = F::add(s3_4, s3_4);
    return vertical;
}
template <class F> __host__ __device__ inline bool line_add(ProjT<F> &t, const typename F::El &qx, const typename F::El &qy, typename F::El (&c)[3])
{
    const auto u = F::template sub<256>(F::mul(qy, t.z), t.y);
    const auto v = F::template sub<64>(F::mul(qx, t.z), t.x);
    const bool vertical = F::is_zero(v);
    const auto vv = F::sqr(v);
    const auto vvv = F::mul(v, vv);
    const auto r = F::mul(vv, t.x);
    c[0] = F::template sub<16>(F::mul(u, t.x), F::mul(t.y, v));
    c[1] = F::template neg<16>(F::mul(u, t.z));
    c[2] = F::mul(v, t.z);
    const auto a = F::template sub<64>(F::template sub<16>(F::mul(F::sqr(u), t.z), vvv), F::add(r, r));   // u^2 Z - v^3 - 2 v^2 X
    t.y = F::template sub<16>(F::mul(u, F::template sub<256>(r, a)), F::mul(vvv, t.y));
    t.x = F::mul(v, a);
    t.z = F::mul(vvv, t.z);
    return vertical;
}

// The table of Q = (qx, qy) (not infinity): LINES lines of three coefficients, in the order the Miller loop uses them.  `put(line, j,
// coefficient)` stores one.  Returns true if some denominator was zero (the loop is then meaningless; only a point outside the
// subgroup gets there).
template <class F, class Put> __host__ __device__ inline bool line_table(const typename F::El &qx, const typename F::El &qy, Put put)
{
    ProjT<F> t;
    t.x = qx; t.y = qy; t.z = F::one();
    bool degenerate = false;
    int line = 0;
    typename F::El c[3];
#pragma nounroll
    for (int bit = 62; bit >= 0; bit--) {
        degenerate |= line_double(t, c);
        put(line, 0, c[0]); put(line, 1, c[1]); put(line, 2, c[2]);
        line++;
        if ((Z_ABS >> bit) & 1ull) {
            degenerate |= line_add(t, qx, qy, c);
            put(line, 0, c[0]); put(line, 1, c[1]); put(line, 2, c[2]);
            line++;
        }
    }
    return degenerate;
}

// ---- frw_pairing_dev.hip's entry points for frw_verify_dev.hip --------------------------------------------------------------------
// the key's device part (vk->d_pairing, vk->pairing_inf): the line tables of -gamma, -delta and beta (ark-ff's words of alpha: 12, of
// beta: 24), the Frobenius constants, e(alpha, beta)^3, alpha -- made on the host with frw_pairing.h and this header, then uploaded
int upload_key(frw_groth16_vk *vk, const uint64_t *alpha_ark, const uint64_t *beta_ark);
// workspace bytes of verify_proofs: per proof in flight, and once per pass (multiples of 16)
size_t proof_workspace_bytes(int flags);
size_t pass_workspace_bytes(int flags);
// accepted[i] for `cnt` proofs whose prepared inputs (d_prepared, 12 words each) and instance statuses (d_status: 0 or -1) are on
// the device: the proof points' checks (d_status becomes -1 where they fail), the pairings, the comparison.  With FRW_VERIFY_BATCHED
// first the batched check (seed: 4 host words; `first` the index of the pass's first proof in the whole batch; d_batch_passed
// (optional) set to the pass's result for first = 0, and-ed with it otherwise).  Stream-ordered.
int verify_proofs(const frw_groth16_vk *vk, size_t cnt, size_t first, const uint64_t *d_proofs, const uint64_t *d_prepared, int32_t *d_status,
                  int flags, const uint64_t *seed, int32_t *d_accepted, int32_t *d_batch_passed, void *d_workspace, hipStream_t st);

}  // namespace pairing_dev
}  // namespace frw
