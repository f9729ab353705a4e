// frw_qap_field.h -- the field side of the QAP witness map over ANY four-limb field (frw_field.h's rule) with a radix-2 domain: what
// frw_fft_field_info, frw_qapf_domain and frw_qapf_create of include/frw.h stand on.  Host only, no device: it compiles with g++ through
// tests/cpp/hip_host, and tests/cpp/test_qap_field_host.cpp runs it under the sanitizers.  Four parts.
//   * field_pow, field_inv (Fermat, exponent p - 2) on the Montgomery form of frw_r1cs_field.h.
//   * fft_field_derive: with p - 1 = 2^s t, t odd, the two-adicity s and the root generator^t -- what ark-ff's FftParameters lists.  The
//     generator is the caller's; what is checked of it is what the map needs: generator^(p - 1) = 1 (a Fermat test -- the inverses here
//     are Fermat inverses) and root^(2^(s - 1)) = -1 (the root has order 2^s: the generator is no square).
//   * qapf_domain_derive: ark-poly's Radix2EvaluationDomain::new(C + I) and the constants of the coset by the generator.
//   * the pass schedule of a 2^L-point transform (qapf_schedule) and the tables the kernels of frw_qap_field.hip read, every entry
//     c 2^256 mod p, canonical, 8 x 32 bits.  Each builder fills a buffer of exactly the length its _elems function names.
//
// THE SCHEDULE.  L <= 12: one pass, the array in LDS.  Above: m = ceil(L / 8) passes over digits T_1 .. T_m of the index, T_1 the most
// significant, as even as they come (the first L mod m digits one bit longer): 13 = 7 + 6, 16 = 8 + 8, 17 = 6 + 6 + 5, 18 = 6 + 6 + 6,
// 22 = 8 + 7 + 7.  Digit i sits at bits [S_i, S_i + T_i) of a position, S_i = T_(i+1) + .. + T_m, and B_i = 2^(S_i + T_i).
//   F(w), natural in, digit-reversed out, in place:  for i = 1 .. m:  a 2^T_i-point transform over digit i with root w^(n / 2^T_i),
//       natural in and out, then position x 2^S_i k + rest (k the digit, rest < 2^S_i) times w^((n / B_i) k rest)      [twist i; none at i = m]
//   G(w), digit-reversed in, natural out, in place:  the transpose -- for i = m .. 1: the transform over digit i, then twist i - 1.
//   Position pos of digit-reversed order holds index  rev(pos) = k_1 + 2^T_1 k_2 + 2^(T_1 + T_2) k_3.
// The map:  F(w^-1) on A z ++ instance, B z, C z  ->  x g^rev(pos) / n  ->  G(w)  ->  a o b - c, natural order  ->  F(w^-1), whose last
// pass multiplies index k by g^-k / (n (g^n - 1)) and writes it to h[k].  tools/dev/qap_field_schedule_model.py is the same rule in
// Python integers against a plain DFT.
#pragma once
#include <stdint.h>
#include <string>
#include "frw_layout.h"
#include "frw_r1cs_field.h"

namespace frw {

// base^e, e four 64-bit limbs; base x 2^256 mod p canonical in, the same out
inline void field_pow(const FieldDerived &d, const uint32_t (&base)[8], const uint64_t e[4], uint32_t (&out)[8])
{
    uint32_t acc[8];
    for (int j = 0; j < 8; j++) acc[j] = d.fc.one[j];
    for (int bit = 255; bit >= 0; bit--) {
        field_mul(d.fc, acc, acc, acc);
        if ((e[bit >> 6] >> (bit & 63)) & 1u) field_mul(d.fc, acc, base, acc);
    }
    for (int j = 0; j < 8; j++) out[j] = acc[j];
}
// x^(p - 2): the inverse where p is prime and x != 0
inline void field_inv(const FieldDerived &d, const uint32_t (&x)[8], uint32_t (&out)[8])
{
    uint64_t e[4];
    field_limbs(d.fc.p, e);
    const uint64_t low = e[0];
    e[0] -= 2;                                                     // p is odd and > 2^160: borrows at most into the next limbs
    if (low < 2)
        for (int j = 1; j < 4 && e[j]-- == 0; j++) {}
    field_pow(d, x, e, out);
}
inline bool field_equal(const uint32_t (&a)[8], const uint32_t (&b)[8])
{
    bool eq = true;
    for (int j = 0; j < 8; j++) eq &= a[j] == b[j];
    return eq;
}
inline void field_copy(const uint32_t (&a)[8], uint32_t *out)
{
    for (int j = 0; j < 8; j++) out[j] = a[j];
}

constexpr int QAPF_MAX_LOG_N = 22;          // schoolbook Falcon-1024 has C + I = 1,158,199: 2^21

struct FftField {
    FieldDerived fd;
    uint32_t two_adicity;
    uint32_t gen[8], root[8];               // x 2^256 mod p
};

// The empty string and *out, or the rule that refuses (modulus, generator).
inline std::string fft_field_derive(const uint64_t modulus[4], const uint64_t generator[4], FftField *out)
{
    if (!modulus || !generator || !out) return "null pointer";
    FftField f{};
    if (!field_derive(modulus, &f.fd)) return "the modulus is not odd with 2^160 < p < 2^255";
    bool below = false, zero = true;
    for (int k = 3; k >= 0; k--) zero &= generator[k] == 0;
    for (int k = 3; k >= 0; k--)
        if (generator[k] != modulus[k]) { below = generator[k] < modulus[k]; break; }
    if (zero || !below) return "the generator is 0 or not below the modulus";
    field_from_integer(f.fd, generator, false, f.gen);
    uint64_t t[4] = {modulus[0] - 1, modulus[1], modulus[2], modulus[3]};      // p is odd
    uint32_t fermat[8];
    field_pow(f.fd, f.gen, t, fermat);
    if (!field_equal(fermat, f.fd.fc.one)) return "generator^(p - 1) is not 1: the modulus is not prime (the inverses are Fermat inverses)";
    uint32_t s = 0;
    while (!(t[0] & 1u)) {
        for (int j = 0; j < 4; j++) t[j] = (t[j] >> 1) | (j < 3 ? t[j + 1] << 63 : 0);
        s++;
    }
    f.two_adicity = s;
    field_pow(f.fd, f.gen, t, f.root);
    uint32_t top[8], minus_one[8];
    const uint32_t nought[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    field_copy(f.root, top);
    for (uint32_t i = 1; i < s; i++) field_mul(f.fd.fc, top, top, top);
    field_sub(f.fd.fc, nought, f.fd.fc.one, minus_one);
    if (!field_equal(top, minus_one)) return "root^(2^(s - 1)) is not -1: the generator is a square, its odd power has no order 2^s";
    *out = f;
    return std::string();
}

struct QapfDomain {
    uint32_t log_size;
    uint32_t group_gen[8], group_gen_inv[8], size_inv[8], generator_inv[8], vanishing_inv[8];      // x 2^256 mod p
};

// Radix2EvaluationDomain::new(C + I) and the coset's constants.  The empty string and *out, or the refusal.
inline std::string qapf_domain_derive(const FftField &f, uint64_t num_constraints, uint64_t num_instance, QapfDomain *out)
{
    if (!out) return "null pointer";
    const uint64_t coeffs = num_constraints + num_instance;
    if (coeffs < num_constraints || coeffs > ((uint64_t)1 << 62)) return "C + I is beyond every domain";
    uint32_t L = 0;
    while (((uint64_t)1 << L) < coeffs) L++;
    if (L > f.two_adicity) return "the domain is larger than the field's two-adic subgroup (PolynomialDegreeTooLarge)";
    if (L > (uint32_t)QAPF_MAX_LOG_N) return "the domain is larger than 2^22";
    QapfDomain d{};
    d.log_size = L;
    field_copy(f.root, d.group_gen);
    for (uint32_t i = L; i < f.two_adicity; i++) field_mul(f.fd.fc, d.group_gen, d.group_gen, d.group_gen);
    field_inv(f.fd, d.group_gen, d.group_gen_inv);
    const uint64_t size[4] = {(uint64_t)1 << L, 0, 0, 0};
    uint32_t n_mont[8], gn[8], van[8];
    field_from_integer(f.fd, size, false, n_mont);
    field_inv(f.fd, n_mont, d.size_inv);
    field_inv(f.fd, f.gen, d.generator_inv);
    field_copy(f.gen, gn);
    for (uint32_t i = 0; i < L; i++) field_mul(f.fd.fc, gn, gn, gn);
    if (field_equal(gn, f.fd.fc.one)) return "generator^n is 1: the coset is the domain itself and the division has no inverse";
    field_sub(f.fd.fc, gn, f.fd.fc.one, van);
    field_inv(f.fd, van, d.vanishing_inv);
    *out = d;
    return std::string();
}

// ---- the schedule (the rule at the head of this file) ---------------------------------------------------------------------------------
constexpr int QAPF_LDS_LOG_N = 12;          // the largest array one workgroup keeps in LDS: 4,096 elements, 128 KiB of the 160
constexpr int QAPF_MAX_DIGIT = 8;           // a multi-pass tile: 2^8 points x 2^3 adjacent columns = 64 KiB
constexpr int QAPF_COLS_LOG = 3;            // eight elements, 256 bytes, is the shortest run a pass reads or writes
constexpr int QAPF_MAX_PASSES = 3;

struct QapfSchedule {
    int log_n, num_passes;
    int T[QAPF_MAX_PASSES], S[QAPF_MAX_PASSES];      // digit i (0-based here): bits [S[i], S[i] + T[i]) of a position
};
inline QapfSchedule qapf_schedule(int L)
{
    QapfSchedule s{};
    s.log_n = L;
    s.num_passes = L <= QAPF_LDS_LOG_N ? 1 : (L + QAPF_MAX_DIGIT - 1) / QAPF_MAX_DIGIT;
    for (int i = 0, left = L; i < s.num_passes; i++) {
        s.T[i] = L / s.num_passes + (i < L % s.num_passes ? 1 : 0);
        left -= s.T[i];
        s.S[i] = left;
    }
    return s;
}
// the index a position of digit-reversed order holds
inline uint32_t qapf_digit_reverse(const QapfSchedule &s, uint32_t pos)
{
    uint32_t index = 0;
    for (int i = 0, sh = 0; i < s.num_passes; i++) {
        index |= ((pos >> s.S[i]) & ((1u << s.T[i]) - 1u)) << sh;
        sh += s.T[i];
    }
    return index;
}

// base^(2^k)
inline void field_pow2k(const FieldDerived &d, const uint32_t (&base)[8], int k, uint32_t (&out)[8])
{
    uint32_t x[8];
    field_copy(base, x);
    for (int i = 0; i < k; i++) field_mul(d.fc, x, x, x);
    field_copy(x, out);
}

// pass i's stage twiddles: rho^j, j < 2^(T_i - 1), rho = root^(n / 2^T_i); `root` is w or w^-1
inline size_t qapf_stage_elems(const QapfSchedule &s, int i) { return (size_t)1 << (s.T[i] - 1); }
inline void qapf_build_stage(const FieldDerived &d, const uint32_t (&root)[8], const QapfSchedule &s, int i, uint32_t *out)
{
    uint32_t rho[8], x[8];
    field_pow2k(d, root, s.log_n - s.T[i], rho);
    field_copy(d.fc.one, x);
    const size_t count = qapf_stage_elems(s, i);
    for (size_t j = 0; j < count; j++) {
        field_copy(x, out + 8 * j);
        field_mul(d.fc, x, rho, x);
    }
}
// twist i (i < m - 1): position (k << S_i | rest) of a block of B_i -> (root^(n / B_i))^(k rest)
inline size_t qapf_twist_elems(const QapfSchedule &s, int i) { return (size_t)1 << (s.S[i] + s.T[i]); }
inline void qapf_build_twist(const FieldDerived &d, const uint32_t (&root)[8], const QapfSchedule &s, int i, uint32_t *out)
{
    uint32_t wb[8], step[8], x[8];
    field_pow2k(d, root, s.log_n - s.S[i] - s.T[i], wb);
    field_copy(d.fc.one, step);                                    // wb^k
    for (size_t k = 0; k < ((size_t)1 << s.T[i]); k++) {
        field_copy(d.fc.one, x);
        for (size_t rest = 0; rest < ((size_t)1 << s.S[i]); rest++) {
            field_copy(x, out + 8 * ((k << s.S[i]) | rest));
            field_mul(d.fc, x, step, x);
        }
        field_mul(d.fc, step, wb, step);
    }
}
// c base^k, k < n, at place[k]: `reversed` puts index k where digit-reversed order holds it
inline void qapf_build_powers(const FieldDerived &d, const uint32_t (&c)[8], const uint32_t (&base)[8], const QapfSchedule &s, bool reversed,
                              uint32_t *out)
{
    uint32_t x[8];
    field_copy(c, x);
    std::vector<uint32_t> where;
    if (reversed) {
        where.resize((size_t)1 << s.log_n);
        for (uint32_t pos = 0; pos < ((uint32_t)1 << s.log_n); pos++) where[qapf_digit_reverse(s, pos)] = pos;
    }
    for (size_t k = 0; k < ((size_t)1 << s.log_n); k++) {
        field_copy(x, out + 8 * (reversed ? (size_t)where[k] : k));
        field_mul(d.fc, x, base, x);
    }
}
// g^rev(pos) / n at pos, and g^-k / (n (g^n - 1)) at k: n elements each
inline void qapf_build_scale_in(const FftField &f, const QapfDomain &dom, const QapfSchedule &s, uint32_t *out)
{
    qapf_build_powers(f.fd, dom.size_inv, f.gen, s, s.num_passes > 1, out);
}
inline void qapf_build_scale_out(const FftField &f, const QapfDomain &dom, const QapfSchedule &s, uint32_t *out)
{
    uint32_t c[8];
    field_mul(f.fd.fc, dom.size_inv, dom.vanishing_inv, c);
    qapf_build_powers(f.fd, c, dom.generator_inv, s, false, out);
}

// ---- the workspace of a chunk of statements: written once, sized from a null base and carved from the caller's -------------------------
struct QapfBufs {
    uint32_t *abc;          // [statements][3][C][8]   A z, B z, C z
    uint32_t *work;         // [statements][3][n][8]   the working arrays
    uint32_t *zsmall;       // [statements][zs_stride] the check's scratch (the long rows' plain values)
    uint32_t *num;          // [statements]            the violated rows, where the caller asks for none
    size_t bytes;
};
inline QapfBufs qapf_layout(void *ws, size_t statements, size_t num_constraints, int log_n, size_t zs_stride)
{
    QapfBufs b{};
    Carve c(ws);
    b.abc = c.take<uint32_t>(statements * 3 * num_constraints * 32);
    b.work = c.take<uint32_t>((statements * 3 * 32) << log_n);
    b.zsmall = c.take<uint32_t>(statements * zs_stride * 4);
    b.num = c.take<uint32_t>(statements * 4);
    b.bytes = c.off;
    return b;
}

}  // namespace frw
