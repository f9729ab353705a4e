// Test-only: the field side of the QAP witness map over a run-time modulus (falcon-r1cs_amd/csrc/frw_qap_field.h), as a program of its
// own that tests/test_qap_field_host.py builds with -fsanitize=address,undefined (g++, through tests/cpp/hip_host) and runs.  Nothing of
// it is loaded into Python, nothing of the library is linked.  Every expectation comes from the 256-bit arithmetic this file carries
// itself (shift-and-subtract reduction, double-and-add products, square-and-multiply powers), never from the header under test:
//   field_pow, field_inv   against powmod on extreme and random bases and exponents; x x^-1 = 1
//   the root               fft_field_derive over seven (modulus, generator) pairs: s, generator^t; the refusals (a square, 0, p, p + 1,
//                          an inadmissible modulus)
//   the domain             qapf_domain_derive over bn254: group_gen, the four inverses; the three refusals
//   the schedule           digits add up, none above eight in a multi-pass schedule, digit reversal is a permutation
//   the tables             stage twiddles, twists, g^rev(pos) / n, g^-k / (n (g^n - 1)) at n = 2, 4 and 2^13 (the first two-pass size),
//                          each built into a heap buffer of exactly its length
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "frw_qap_field.h"

namespace {
int failures = 0, cases = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        cases++;                                        \
        if (!(cond)) {                                  \
            printf("FAILED %s: ", #cond);               \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            failures++;                                 \
        }                                               \
    } while (0)

typedef unsigned __int128 u128;

// ---- the reference arithmetic: 256-bit integers, four 64-bit limbs ---------------------------------------------------------------
struct U256 { uint64_t l[4]; };
bool operator==(const U256 &a, const U256 &b) { return !memcmp(a.l, b.l, 32); }
int cmp(const U256 &a, const U256 &b)
{
    for (int i = 3; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i] ? -1 : 1;
    return 0;
}
void add_to(U256 &a, const U256 &b)
{
    u128 c = 0;
    for (int i = 0; i < 4; i++) { c += (u128)a.l[i] + b.l[i]; a.l[i] = (uint64_t)c; c >>= 64; }
}
void sub_from(U256 &a, const U256 &b)
{
    uint64_t bw = 0;
    for (int i = 0; i < 4; i++) {
        const u128 x = (u128)a.l[i] - b.l[i] - bw;
        a.l[i] = (uint64_t)x;
        bw = (uint64_t)(x >> 64) & 1;
    }
}
U256 double_plus(const U256 &x, unsigned bit, const U256 &p)      // (2 x + bit) mod p for x < p < 2^255
{
    U256 r;
    for (int i = 3; i >= 0; i--) r.l[i] = (x.l[i] << 1) | (i ? x.l[i - 1] >> 63 : bit);
    if (cmp(r, p) >= 0) sub_from(r, p);
    return r;
}
U256 mod(const U256 &x, const U256 &p)
{
    U256 r{{0, 0, 0, 0}};
    for (int b = 255; b >= 0; b--) r = double_plus(r, (unsigned)(x.l[b >> 6] >> (b & 63)) & 1u, p);
    return r;
}
U256 addmod(const U256 &a, const U256 &b, const U256 &p)
{
    U256 r = a;
    add_to(r, b);
    if (cmp(r, p) >= 0) sub_from(r, p);
    return r;
}
U256 mulmod(const U256 &a, const U256 &b, const U256 &p)          // a any, b < p
{
    U256 r{{0, 0, 0, 0}};
    for (int bit = 255; bit >= 0; bit--) {
        r = double_plus(r, 0, p);
        if ((a.l[bit >> 6] >> (bit & 63)) & 1u) r = addmod(r, b, p);
    }
    return r;
}
const U256 ONE{{1, 0, 0, 0}};
U256 powmod(const U256 &base, const U256 &e, const U256 &p)        // base < p
{
    U256 r = ONE;
    for (int bit = 255; bit >= 0; bit--) {
        r = mulmod(r, r, p);
        if ((e.l[bit >> 6] >> (bit & 63)) & 1u) r = mulmod(r, base, p);
    }
    return r;
}
U256 small(uint64_t v) { return U256{{v, 0, 0, 0}}; }
U256 minus(const U256 &a, uint64_t v)                              // a - v, no wrap expected
{
    U256 r = a;
    sub_from(r, small(v));
    return r;
}
U256 shr1(const U256 &a)
{
    U256 r;
    for (int i = 0; i < 4; i++) r.l[i] = (a.l[i] >> 1) | (i < 3 ? a.l[i + 1] << 63 : 0);
    return r;
}
U256 two_to_256_mod(const U256 &p)
{
    const U256 top{{0, 0, 0, (uint64_t)1 << 63}};
    return double_plus(mod(top, p), 0, p);
}
U256 from_words(const uint32_t *w)
{
    U256 r;
    for (int j = 0; j < 4; j++) r.l[j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
    return r;
}
uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
U256 rnd_below(const U256 &p)
{
    const U256 x{{rnd(), rnd(), rnd(), rnd()}};
    return mod(x, p);
}

struct Case { const char *name; U256 p; uint64_t g; uint32_t s; };
const Case CASES[7] = {
    {"bn254", {{0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL}}, 5, 28},
    {"bls12_377", {{0x0a11800000000001ULL, 0x59aa76fed0000001ULL, 0x60b44d1e5c37b001ULL, 0x12ab655e9a2ca556ULL}}, 22, 47},
    {"pallas", {{0x992d30ed00000001ULL, 0x224698fc094cf91bULL, 0x0000000000000000ULL, 0x4000000000000000ULL}}, 5, 32},
    {"bls12_381", {{0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL}}, 7, 32},
    {"ed25519_l", {{0x5812631a5cf5d3edULL, 0x14def9dea2f79cd6ULL, 0x0000000000000000ULL, 0x1000000000000000ULL}}, 2, 2},
    {"2^255-19", {{0xffffffffffffffedULL, 0xffffffffffffffffULL, 0xffffffffffffffffULL, 0x7fffffffffffffffULL}}, 2, 2},
    {"2^160+7", {{0x0000000000000007ULL, 0x0000000000000000ULL, 0x0000000100000000ULL, 0x0000000000000000ULL}}, 5, 1},
};

// c -> c 2^256 mod p, as the header's words
struct Mont {
    U256 p, R;
    explicit Mont(const U256 &p_) : p(p_), R(two_to_256_mod(p_)) {}
    U256 to(const U256 &c) const { return mulmod(c, R, p); }
    void words(const U256 &c, uint32_t (&w)[8]) const
    {
        const U256 m = to(c);
        frw::field_words(m.l, w);
    }
};

void powers_and_inverses(const Case &c)
{
    frw::FieldDerived d;
    CHECK(frw::field_derive(c.p.l, &d), "%s: refused", c.name);
    const Mont M(c.p);
    const U256 pm1 = minus(c.p, 1), pm2 = minus(c.p, 2);
    std::vector<U256> bases = {ONE, small(2), pm1, pm2, rnd_below(c.p), rnd_below(c.p)};
    std::vector<U256> exps = {small(0), ONE, small(2), pm1, pm2, U256{{rnd(), rnd(), rnd(), rnd()}}, U256{{~0ULL, ~0ULL, ~0ULL, ~0ULL}}};
    for (const U256 &b : bases) {
        uint32_t bw[8], out[8];
        M.words(b, bw);
        for (const U256 &e : exps) {
            frw::field_pow(d, bw, e.l, out);
            CHECK(from_words(out) == M.to(powmod(b, e, c.p)), "%s: field_pow", c.name);
        }
        frw::field_inv(d, bw, out);
        CHECK(from_words(out) == M.to(powmod(b, pm2, c.p)), "%s: field_inv", c.name);
        uint32_t prod[8];
        frw::field_mul(d.fc, out, bw, prod);
        CHECK(frw::field_equal(prod, d.fc.one), "%s: x x^-1 = 1", c.name);
        frw::field_pow(d, bw, exps[3].l, bw);                                 // in place
        CHECK(frw::field_equal(bw, d.fc.one), "%s: Fermat, in place", c.name);
    }
}

void roots(const Case &c)
{
    const Mont M(c.p);
    frw::FftField f;
    const U256 g = small(c.g);
    const std::string refusal = frw::fft_field_derive(c.p.l, g.l, &f);
    CHECK(refusal.empty(), "%s: %s", c.name, refusal.c_str());
    U256 t = minus(c.p, 1);
    uint32_t s = 0;
    while (!(t.l[0] & 1)) { t = shr1(t); s++; }
    CHECK(s == c.s && f.two_adicity == s, "%s: two-adicity %u, %u", c.name, s, f.two_adicity);
    CHECK(from_words(f.root) == M.to(powmod(g, t, c.p)), "%s: the root", c.name);
    CHECK(from_words(f.gen) == M.to(g), "%s: the generator", c.name);
    // 0, p, p + 1
    frw::FftField untouched{};
    U256 pp1 = c.p;
    add_to(pp1, ONE);
    for (const U256 &bad : {small(0), c.p, pp1})
        CHECK(frw::fft_field_derive(c.p.l, bad.l, &untouched).find("generator") != std::string::npos, "%s: generator out of range", c.name);
    CHECK(untouched.two_adicity == 0, "%s: a refusal leaves the output alone", c.name);
}

void refusals()
{
    frw::FftField f;
    for (uint64_t g : {2, 3, 4, 9})
        CHECK(frw::fft_field_derive(CASES[0].p.l, small(g).l, &f).find("square") != std::string::npos, "bn254 with %d", (int)g);
    CHECK(frw::fft_field_derive(CASES[4].p.l, small(3).l, &f).find("square") != std::string::npos, "ed25519_l with 3");
    const U256 bn = CASES[0].p;
    const U256 even = minus(bn, 1), zero = small(0), low{{0, 0, (uint64_t)1 << 32, 0}}, high{{1, 0, 0, (uint64_t)1 << 63}};
    for (const U256 &p : {even, zero, low, high})
        CHECK(frw::fft_field_derive(p.l, small(5).l, &f).find("modulus") != std::string::npos, "an inadmissible modulus");
    // a composite that field_derive admits: the Fermat test is what refuses it (3 x 5 x ... : 2^200 + 1 is divisible by 257)
    const U256 composite{{1, 0, 0, (uint64_t)1 << 8}};
    CHECK(frw::fft_field_derive(composite.l, small(3).l, &f).find("prime") != std::string::npos, "a composite modulus");
    CHECK(!frw::fft_field_derive(nullptr, small(5).l, &f).empty() && !frw::fft_field_derive(bn.l, nullptr, &f).empty() &&
          !frw::fft_field_derive(bn.l, small(5).l, nullptr).empty(), "null pointers");
}

void domains()
{
    const Case &c = CASES[0];
    const Mont M(c.p);
    frw::FftField f;
    CHECK(frw::fft_field_derive(c.p.l, small(c.g).l, &f).empty(), "bn254");
    const U256 g = small(c.g), pm2 = minus(c.p, 2);
    U256 t = minus(c.p, 1);
    for (uint32_t i = 0; i < c.s; i++) t = shr1(t);
    const U256 root = powmod(g, t, c.p);
    const uint64_t sizes[10] = {1, 2, 3, 4, 5, 4095, 4096, 4097, (1u << 22) - 1, 1u << 22};
    for (uint64_t coeffs : sizes) {
        frw::QapfDomain d;
        const std::string refusal = frw::qapf_domain_derive(f, coeffs - 1, 1, &d);
        CHECK(refusal.empty(), "C + I = %llu: %s", (unsigned long long)coeffs, refusal.c_str());
        uint32_t L = 0;
        while (((uint64_t)1 << L) < coeffs) L++;
        CHECK(d.log_size == L, "C + I = %llu: log_size", (unsigned long long)coeffs);
        U256 w = root;
        for (uint32_t i = L; i < c.s; i++) w = mulmod(w, w, c.p);
        const U256 n = small((uint64_t)1 << L);
        U256 gn = g;
        for (uint32_t i = 0; i < L; i++) gn = mulmod(gn, gn, c.p);
        CHECK(from_words(d.group_gen) == M.to(w) && from_words(d.group_gen_inv) == M.to(powmod(w, pm2, c.p)), "group_gen");
        CHECK(from_words(d.size_inv) == M.to(powmod(n, pm2, c.p)) && from_words(d.generator_inv) == M.to(powmod(g, pm2, c.p)), "size_inv, generator_inv");
        CHECK(from_words(d.vanishing_inv) == M.to(powmod(minus(gn, 1), pm2, c.p)), "vanishing_inv");
    }
    frw::QapfDomain d;
    CHECK(frw::qapf_domain_derive(f, (1u << 22) - 1, 2, &d).find("2^22") != std::string::npos, "2^22 + 1 over bn254");
    frw::FftField ed, low;
    CHECK(frw::fft_field_derive(CASES[4].p.l, small(2).l, &ed).empty() && frw::fft_field_derive(CASES[6].p.l, small(5).l, &low).empty(), "small fields");
    CHECK(frw::qapf_domain_derive(ed, 3, 2, &d).find("PolynomialDegreeTooLarge") != std::string::npos, "C + I = 5 over ed25519_l");
    CHECK(frw::qapf_domain_derive(ed, 2, 2, &d).empty() && d.log_size == 2, "C + I = 4 over ed25519_l");
    CHECK(frw::qapf_domain_derive(low, 1, 2, &d).find("PolynomialDegreeTooLarge") != std::string::npos, "C + I = 3 over 2^160+7");
    frw::FftField neg;
    const U256 pm1 = minus(CASES[6].p, 1);
    CHECK(frw::fft_field_derive(CASES[6].p.l, pm1.l, &neg).empty(), "p - 1 generates the two-element subgroup");
    CHECK(frw::qapf_domain_derive(neg, 1, 1, &d).find("coset") != std::string::npos, "generator^n = 1");
}

void schedules()
{
    for (int L = 1; L <= frw::QAPF_MAX_LOG_N; L++) {
        const frw::QapfSchedule s = frw::qapf_schedule(L);
        int sum = 0;
        bool fits = s.num_passes >= 1 && s.num_passes <= frw::QAPF_MAX_PASSES;
        for (int i = 0; i < s.num_passes && fits; i++) {
            sum += s.T[i];
            fits &= s.T[i] >= 1 && s.S[i] == L - sum;
            if (s.num_passes > 1) fits &= s.T[i] <= frw::QAPF_MAX_DIGIT && s.T[i] >= frw::QAPF_COLS_LOG;
        }
        CHECK(fits && sum == L, "the schedule of 2^%d", L);
        CHECK(s.num_passes == (L <= 12 ? 1 : L <= 16 ? 2 : 3), "the passes of 2^%d", L);
    }
    for (int L : {5, 13, 17}) {
        const frw::QapfSchedule s = frw::qapf_schedule(L);
        std::vector<char> seen((size_t)1 << L, 0);
        bool perm = true;
        for (uint32_t pos = 0; pos < (1u << L); pos++) {
            const uint32_t k = frw::qapf_digit_reverse(s, pos);
            perm &= k < (1u << L) && !seen[k];
            if (k < (1u << L)) seen[k] = 1;
        }
        CHECK(perm, "digit reversal at 2^%d", L);
    }
    const frw::QapfSchedule s = frw::qapf_schedule(13);                       // 7 + 6: position k1 2^6 + k2 holds index k1 + 2^7 k2
    CHECK(s.T[0] == 7 && s.T[1] == 6 && frw::qapf_digit_reverse(s, (5u << 6) | 3u) == (5u | (3u << 7)), "2^13 = 7 + 6");
}

// a heap buffer of exactly `elems` elements: the sanitizer sees one word too many
std::unique_ptr<uint32_t[]> exact(size_t elems) { return std::unique_ptr<uint32_t[]>(new uint32_t[elems * 8]); }

void tables(const Case &c, int L)
{
    const Mont M(c.p);
    frw::FftField f;
    frw::QapfDomain d;
    CHECK(frw::fft_field_derive(c.p.l, small(c.g).l, &f).empty() && frw::qapf_domain_derive(f, ((uint64_t)1 << L) - 1, 1, &d).empty(), "%s 2^%d", c.name, L);
    const frw::QapfSchedule s = frw::qapf_schedule(L);
    const U256 g = small(c.g), pm2 = minus(c.p, 2);
    U256 t = minus(c.p, 1);
    for (uint32_t i = 0; i < c.s; i++) t = shr1(t);
    U256 w = powmod(g, t, c.p);
    for (uint32_t i = (uint32_t)L; i < c.s; i++) w = mulmod(w, w, c.p);
    const U256 w_inv = powmod(w, pm2, c.p);
    const size_t n = (size_t)1 << L;
    for (int dir = 0; dir < 2; dir++) {
        const U256 root = dir ? w_inv : w;
        const uint32_t(&root_words)[8] = dir ? d.group_gen_inv : d.group_gen;
        for (int i = 0; i < s.num_passes; i++) {
            const size_t count = frw::qapf_stage_elems(s, i);
            CHECK(count == (s.T[i] == 0 ? 1 : (size_t)1 << (s.T[i] - 1)), "stage elems");
            auto buf = exact(count);
            frw::qapf_build_stage(f.fd, root_words, s, i, buf.get());
            const U256 rho = powmod(root, small((uint64_t)n >> s.T[i]), c.p);
            U256 x = ONE;
            bool ok = true;
            for (size_t j = 0; j < count; j++) {
                ok &= from_words(buf.get() + 8 * j) == M.to(x);
                x = mulmod(x, rho, c.p);
            }
            CHECK(ok, "%s 2^%d: stage table %d, direction %d", c.name, L, i, dir);
            CHECK(count == 1 || mulmod(x, x, c.p) == ONE, "rho has order 2^T");        // x = rho^(2^(T-1)) = -1
            if (i == s.num_passes - 1) break;
            const size_t B = frw::qapf_twist_elems(s, i);
            CHECK(B == (size_t)1 << (s.S[i] + s.T[i]), "twist elems");
            auto tw = exact(B);
            frw::qapf_build_twist(f.fd, root_words, s, i, tw.get());
            const U256 wb = powmod(root, small((uint64_t)n / B), c.p);
            ok = true;
            U256 step = ONE;                                                   // wb^k
            for (size_t k = 0; k < ((size_t)1 << s.T[i]); k++) {
                U256 y = ONE;
                for (size_t rest = 0; rest < ((size_t)1 << s.S[i]); rest++) {
                    ok &= from_words(tw.get() + 8 * ((k << s.S[i]) | rest)) == M.to(y);
                    y = mulmod(y, step, c.p);
                }
                step = mulmod(step, wb, c.p);
            }
            CHECK(ok, "%s 2^%d: twist %d, direction %d", c.name, L, i, dir);
            for (int probe = 0; probe < 8; probe++) {                          // and by the definition, not the recurrence
                const size_t pos = (size_t)rnd() & (B - 1), k = pos >> s.S[i], rest = pos & (((size_t)1 << s.S[i]) - 1);
                CHECK(from_words(tw.get() + 8 * pos) == M.to(powmod(wb, small((uint64_t)(k * rest)), c.p)), "twist %d at %zu", i, pos);
            }
        }
    }
    const U256 n_inv = powmod(small((uint64_t)n), pm2, c.p), g_inv = powmod(g, pm2, c.p);
    U256 gn = g;
    for (int i = 0; i < L; i++) gn = mulmod(gn, gn, c.p);
    const U256 scale = mulmod(n_inv, powmod(minus(gn, 1), pm2, c.p), c.p);
    auto in = exact(n), out = exact(n);
    frw::qapf_build_scale_in(f, d, s, in.get());
    frw::qapf_build_scale_out(f, d, s, out.get());
    std::vector<U256> gk(n), gik(n);
    U256 x = n_inv, y = scale;
    for (size_t k = 0; k < n; k++) {
        gk[k] = x;
        gik[k] = y;
        x = mulmod(x, g, c.p);
        y = mulmod(y, g_inv, c.p);
    }
    bool ok_in = true, ok_out = true;
    for (size_t pos = 0; pos < n; pos++) {
        ok_in &= from_words(in.get() + 8 * pos) == M.to(gk[frw::qapf_digit_reverse(s, (uint32_t)pos)]);
        ok_out &= from_words(out.get() + 8 * pos) == M.to(gik[pos]);
    }
    CHECK(ok_in, "%s 2^%d: g^rev(pos) / n", c.name, L);
    CHECK(ok_out, "%s 2^%d: g^-k / (n (g^n - 1))", c.name, L);
    CHECK(mulmod(mulmod(gik[n - 1], powmod(g, small((uint64_t)n - 1), c.p), c.p), mulmod(small((uint64_t)n), minus(gn, 1), c.p), c.p) == ONE, "the last factor, by its definition");
}

void layout()
{
    const frw::QapfBufs one = frw::qapf_layout(nullptr, 1, 131070, 17, 1544), five = frw::qapf_layout(nullptr, 5, 131070, 17, 1544);
    CHECK(one.bytes >= 3 * 131070 * 32 + 3 * 32 * (1 << 17) + 1544 * 4 + 4 && one.bytes % 256 == 0, "one statement");
    CHECK(five.bytes <= 5 * one.bytes && five.bytes >= 5 * (one.bytes - 4 * 256), "five statements fit five statements' bytes");
    char base[1];
    const frw::QapfBufs b = frw::qapf_layout(base, 2, 6, 3, 0);
    CHECK((char *)b.abc == base && (char *)b.work == base + 1280 && (char *)b.zsmall == base + 1280 + 1536 && (char *)b.num == (char *)b.zsmall &&
          b.bytes == 1280 + 1536 + 256, "the carve of two small statements");
}
}  // namespace

int main()
{
    for (const Case &c : CASES) {
        powers_and_inverses(c);
        roots(c);
    }
    refusals();
    domains();
    schedules();
    for (int L : {1, 2, 13}) tables(CASES[0], L);
    tables(CASES[1], 2);
    tables(CASES[6], 1);
    layout();
    printf("%d checks, %d failed\n", cases, failures);
    if (!failures) printf("qap_field_host: clean\n");
    return failures ? 1 : 0;
}
