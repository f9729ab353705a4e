// Test-only: the host side of a constraint system over a run-time modulus (falcon-r1cs_amd/csrc/frw_r1cs_field.h), as a program of
// its own that tests/test_r1cs_field_host.py builds with -fsanitize=address,undefined (g++, through tests/cpp/hip_host) and runs;
// tools/sanitize_cpu.sh runs it too.  argv[1]: a directory to write in.  Nothing of it is loaded into Python, nothing of the
// library is linked.  Every expectation comes from the 256-bit arithmetic this file carries itself (shift-and-subtract reduction,
// double-and-add products on unsigned __int128 carries), never from the header under test:
//   arithmetic   field_mul, field_add, field_sub over five moduli on extreme and random operands
//   the lift     lift_centred on both sides of r / 2 and at 0, 1, r - 1; the 2^200 guard on either side of the bound and either sign
//   conversion   field_from_integer (x 2^256 mod p) and field_to_canonical for magnitudes below and above p
//   r1csf_lift   a small system with +-1, q, a 160-bit and a negative coefficient; a doctored one (2^232, an inverse) is refused with
//                the matrix and the row named
//   matrices     r1csf_from_csr: a value p - 1 accepted, p refused, a column beyond the variables, a decreasing row_ptr; the file
//                written and read back; a file one byte short
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "frw_r1cs_field.h"

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

using frw::host::ConstraintMatrices;
using frw::host::Fr;
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
uint64_t add_to(U256 &a, const U256 &b)          // returns the carry
{
    u128 c = 0;
    for (int i = 0; i < 4; i++) { c += (u128)a.l[i] + b.l[i]; a.l[i] = (uint64_t)c; c >>= 64; }
    return (uint64_t)c;
}
void sub_from(U256 &a, const U256 &b)            // a >= b, or the caller wants the wrap
{
    uint64_t bw = 0;
    for (int i = 0; i < 4; i++) {
        const u128 x = (u128)a.l[i] - b.l[i] - bw;
        a.l[i] = (uint64_t)x;
        bw = (uint64_t)(x >> 64) & 1;
    }
}
// (2 x + bit) mod p for x < p < 2^255
U256 double_plus(const U256 &x, unsigned bit, const U256 &p)
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
U256 addmod(const U256 &a, const U256 &b, const U256 &p)      // a, b < p
{
    U256 r = a;
    add_to(r, b);                                              // < 2 p < 2^256
    if (cmp(r, p) >= 0) sub_from(r, p);
    return r;
}
U256 mulmod(const U256 &a, const U256 &b, const U256 &p)      // a any, b < p
{
    U256 r{{0, 0, 0, 0}};
    for (int bit = 255; bit >= 0; bit--) {
        r = double_plus(r, 0, p);
        if ((a.l[bit >> 6] >> (bit & 63)) & 1u) r = addmod(r, b, p);
    }
    return r;
}
U256 negmod(const U256 &a, const U256 &p)
{
    if (!(a.l[0] | a.l[1] | a.l[2] | a.l[3])) return a;
    U256 r = p;
    sub_from(r, a);
    return r;
}
U256 two_to_256_mod(const U256 &p)
{
    const U256 top{{0, 0, 0, (uint64_t)1 << 63}};
    return double_plus(mod(top, p), 0, p);
}

U256 from_words(const uint32_t (&w)[8])
{
    U256 r;
    frw::field_limbs(w, r.l);
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

const U256 MODULI[5] = {
    {{0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL}},      // bn254: ninv32 is not -1
    {{0xffffffffffffffedULL, 0xffffffffffffffffULL, 0xffffffffffffffffULL, 0x7fffffffffffffffULL}},      // 2^255 - 19: top of the range
    {{0x0000000000000007ULL, 0x0000000000000000ULL, 0x0000000100000000ULL, 0x0000000000000000ULL}},      // 2^160 + 7: bottom of the range
    {{0x0a11800000000001ULL, 0x59aa76fed0000001ULL, 0x60b44d1e5c37b001ULL, 0x12ab655e9a2ca556ULL}},      // bls12_377
    {{0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL}},      // bls12_381
};
const char *NAMES[5] = {"bn254", "2^255-19", "2^160+7", "bls12_377", "bls12_381"};

void arithmetic(int which)
{
    const U256 p = MODULI[which];
    frw::FieldDerived d;
    CHECK(frw::field_derive(p.l, &d), "%s: refused", NAMES[which]);
    const U256 R = two_to_256_mod(p);
    CHECK(from_words(d.fc.one) == R, "%s: one", NAMES[which]);
    CHECK(from_words(d.r2) == mulmod(R, R, p), "%s: r2", NAMES[which]);
    U256 pm1 = p;
    pm1.l[0] -= 1;
    std::vector<U256> ops = {{{0, 0, 0, 0}}, {{1, 0, 0, 0}}, pm1, R, {{0xffffffffffffffffULL, 0, 0, 0}}};
    for (int i = 0; i < 12; i++) ops.push_back(rnd_below(p));
    for (const U256 &a : ops)
        for (const U256 &b : ops) {
            uint32_t aw[8], bw[8], out[8];
            frw::field_words(a.l, aw);
            frw::field_words(b.l, bw);
            frw::field_mul(d.fc, aw, bw, out);
            // out R = a b (mod p), out < p
            const U256 got = from_words(out);
            CHECK(cmp(got, p) < 0 && mulmod(got, R, p) == mulmod(a, b, p), "%s: field_mul", NAMES[which]);
            frw::field_add(d.fc, aw, bw, out);
            CHECK(from_words(out) == addmod(a, b, p), "%s: field_add", NAMES[which]);
            frw::field_sub(d.fc, aw, bw, out);
            CHECK(from_words(out) == addmod(a, negmod(b, p), p), "%s: field_sub", NAMES[which]);
            frw::field_add(d.fc, aw, bw, aw);                               // in place, as the kernels call it
            CHECK(from_words(aw) == addmod(a, b, p), "%s: field_add in place", NAMES[which]);
        }
    // the left operand of field_mul may be ANY 256-bit value (a magnitude above p; a witness element that is not canonical)
    for (int i = 0; i < 8; i++) {
        const U256 a{{rnd(), rnd(), rnd(), i ? rnd() : ~(uint64_t)0}}, b = rnd_below(p);
        uint32_t aw[8], bw[8], out[8];
        frw::field_words(a.l, aw);
        frw::field_words(b.l, bw);
        frw::field_mul(d.fc, aw, bw, out);
        const U256 got = from_words(out);
        CHECK(cmp(got, p) < 0 && mulmod(got, R, p) == mulmod(a, b, p), "%s: field_mul, wide left operand", NAMES[which]);
    }
    // integers of either sign -> x 2^256 mod p -> canonical
    const U256 mags[] = {{{0, 0, 0, 0}}, {{1, 0, 0, 0}}, {{12289, 0, 0, 0}}, {{rnd(), rnd(), rnd() & 0xffffffffu, 0}},
                         {{rnd(), rnd(), rnd(), 0xff}}, {{~(uint64_t)0, ~(uint64_t)0, ~(uint64_t)0, 0xff}}, p, pm1};
    for (const U256 &mag : mags)
        for (int neg = 0; neg < 2; neg++) {
            uint32_t mont[8];
            uint64_t canon[4];
            frw::field_from_integer(d, mag.l, neg != 0, mont);
            frw::field_to_canonical(d, mont, canon);
            const U256 want = neg ? negmod(mod(mag, p), p) : mod(mag, p);
            CHECK(!memcmp(canon, want.l, 32), "%s: integer -> canonical", NAMES[which]);
            CHECK(from_words(mont) == mulmod(want, R, p), "%s: integer -> Montgomery", NAMES[which]);
        }
}

Fr fr_from(const U256 &canonical) { return Fr::from_canonical(canonical.l); }

void lifts()
{
    const U256 r = MODULI[4];
    U256 half = r;                                                          // (r - 1) / 2
    for (int i = 0; i < 4; i++) half.l[i] = (r.l[i] >> 1) | (i < 3 ? r.l[i + 1] << 63 : 0);
    U256 half1 = half, rm1 = r, rm2 = r;
    half1.l[0] += 1;
    rm1.l[0] -= 1;
    rm2.l[0] -= 2;
    const U256 small{{rnd(), rnd(), rnd() & 0xffffffffu, 0}};              // 160 bits
    U256 minus_small = r;
    sub_from(minus_small, small);
    const U256 vs[] = {{{0, 0, 0, 0}}, {{1, 0, 0, 0}}, {{2, 0, 0, 0}}, half, half1, rm1, rm2, small, minus_small};
    for (const U256 &v : vs) {
        const frw::LiftedCoef l = frw::lift_centred(v.l);
        const bool want_neg = cmp(v, half) > 0;
        U256 mag{{l.mag[0], l.mag[1], l.mag[2], l.mag[3]}};
        CHECK(l.negative == want_neg, "lift: sign");
        if (want_neg) {
            U256 sum = mag;
            add_to(sum, v);
            CHECK(sum == r, "lift: r - v");
        } else {
            CHECK(mag == v, "lift: v");
        }
    }
    // the guard: |lift| < 2^200
    const U256 edge{{0, 0, 0, (uint64_t)1 << 8}};                           // 2^200
    U256 below = edge, neg_edge = r, neg_below = r;
    sub_from(below, U256{{1, 0, 0, 0}});
    sub_from(neg_edge, edge);
    sub_from(neg_below, below);
    CHECK(frw::lift_below_2_200(frw::lift_centred(below.l)), "2^200 - 1 is within the bound");
    CHECK(!frw::lift_below_2_200(frw::lift_centred(edge.l)), "2^200 is not");
    CHECK(frw::lift_below_2_200(frw::lift_centred(neg_below.l)), "-(2^200 - 1) is within the bound");
    CHECK(!frw::lift_below_2_200(frw::lift_centred(neg_edge.l)), "-(2^200) is not");
}

// one row per matrix entry list; I = 2, W = 2
ConstraintMatrices small_system(const std::vector<std::vector<std::pair<Fr, uint32_t>>> &a, const std::vector<std::vector<std::pair<Fr, uint32_t>>> &b,
                                const std::vector<std::vector<std::pair<Fr, uint32_t>>> &c)
{
    ConstraintMatrices m;
    m.num_instance_variables = 2;
    m.num_witness_variables = 2;
    m.num_constraints = a.size();
    m.a = a;
    m.b = b;
    m.c = c;
    return m;
}

void lifted_systems(int which)
{
    const U256 p = MODULI[which], r = MODULI[4];
    frw::FieldDerived d;
    if (!frw::field_derive(p.l, &d)) { CHECK(false, "%s: refused", NAMES[which]); return; }
    const U256 big{{0x123456789abcdef0ULL, 0x0fedcba987654321ULL, 0xdeadbeefULL, 0}};     // 160 bits: above 2^160 + 7
    const Fr one = Fr::one(), q = Fr::from(12289), bigf = fr_from(big);
    const ConstraintMatrices m = small_system({{{one, 2}, {-one, 3}}, {{q, 0}, {-q, 1}, {bigf, 2}}}, {{{-bigf, 3}}, {}}, {{{one, 1}}, {{Fr::from(0), 0}}});
    frw::FieldMatrices fm;
    const std::string why = frw::r1csf_lift(m, d, &fm);
    CHECK(why.empty(), "%s: a system of integers is refused: %s", NAMES[which], why.c_str());
    CHECK(fm.num_instance == 2 && fm.num_witness == 2 && fm.num_constraints == 2, "%s: counts", NAMES[which]);
    const std::vector<uint64_t> ptr_a = {0, 2, 5}, ptr_b = {0, 1, 1}, ptr_c = {0, 1, 2};
    CHECK(fm.row_ptr[0] == ptr_a && fm.row_ptr[1] == ptr_b && fm.row_ptr[2] == ptr_c, "%s: row_ptr", NAMES[which]);
    const std::vector<uint32_t> col_a = {2, 3, 0, 1, 2};
    CHECK(fm.col[0] == col_a, "%s: columns", NAMES[which]);
    const U256 one_u{{1, 0, 0, 0}}, q_u{{12289, 0, 0, 0}};
    const U256 want_a[5] = {one_u, negmod(one_u, p), q_u, negmod(q_u, p), mod(big, p)};
    for (int t = 0; t < 5; t++) CHECK(!memcmp(&fm.val[0][4 * t], want_a[t].l, 32), "%s: A, term %d", NAMES[which], t);
    const U256 want_b = negmod(mod(big, p), p);
    CHECK(!memcmp(&fm.val[1][0], want_b.l, 32), "%s: B, the negative 160-bit coefficient", NAMES[which]);
    CHECK(!(fm.val[2][4] | fm.val[2][5] | fm.val[2][6] | fm.val[2][7]), "%s: a zero coefficient stays a term, zero", NAMES[which]);
    // doctored: 2^232 in matrix B, row 1; then the inverse of 3 (no small integer over r) in matrix C, row 0
    const U256 huge{{0, 0, 0, (uint64_t)1 << 40}};
    frw::FieldMatrices untouched;
    std::string refusal = frw::r1csf_lift(small_system({{{one, 2}}, {{one, 2}}}, {{{one, 2}}, {{fr_from(huge), 3}}}, {{}, {}}), d, &untouched);
    CHECK(refusal.find("matrix B, row 1") != std::string::npos, "%s: 2^232 gives \"%s\"", NAMES[which], refusal.c_str());
    // 3^-1 mod r = (2 r + 1) / 3, written out: r = 3 k + 1 -> 3 (2 k + 1) = 2 r + 1
    U256 third{{0, 0, 0, 0}};
    {
        // k = (r - 1) / 3 by long division on 64-bit limbs
        U256 rm1 = r;
        rm1.l[0] -= 1;
        u128 rem = 0;
        U256 k{{0, 0, 0, 0}};
        for (int i = 3; i >= 0; i--) { const u128 cur = (rem << 64) | rm1.l[i]; k.l[i] = (uint64_t)(cur / 3); rem = cur % 3; }
        third = k;
        add_to(third, k);
        add_to(third, U256{{1, 0, 0, 0}});
        CHECK(rem == 0 && (Fr::from(3) * fr_from(third)) == one, "the test's own inverse of three");
    }
    refusal = frw::r1csf_lift(small_system({{{one, 2}}}, {{{one, 2}}}, {{{fr_from(third), 3}}}), d, &untouched);
    CHECK(refusal.find("matrix C, row 0") != std::string::npos, "%s: an inverse gives \"%s\"", NAMES[which], refusal.c_str());
    CHECK(untouched.num_constraints == 0, "%s: a refused system is written out", NAMES[which]);
}

struct Csr {
    uint64_t counts[6];
    std::vector<uint64_t> ptr[3], val[3];
    std::vector<uint32_t> col[3];
    const uint64_t *rp[3], *vp[3];
    const uint32_t *cp[3];
    void point()
    {
        for (int m = 0; m < 3; m++) { rp[m] = ptr[m].data(); cp[m] = col[m].data(); vp[m] = val[m].data(); counts[3 + m] = col[m].size(); }
    }
};
// x^3 + x + 5 = y: I = 2 (one, y), W = 3 (x, x^2, x^3); the 5 replaced by p - 1 to sit at the bound
Csr cubic(const U256 &top)
{
    Csr s{};
    s.counts[0] = 2; s.counts[1] = 3; s.counts[2] = 3;
    auto term = [&](int m, uint32_t c, const U256 &v) { s.col[m].push_back(c); s.val[m].insert(s.val[m].end(), v.l, v.l + 4); };
    const U256 one{{1, 0, 0, 0}};
    for (int m = 0; m < 3; m++) s.ptr[m].push_back(0);
    auto end_row = [&]() { for (int m = 0; m < 3; m++) s.ptr[m].push_back(s.col[m].size()); };
    term(0, 2, one); term(1, 2, one); term(2, 3, one); end_row();
    term(0, 3, one); term(1, 2, one); term(2, 4, one); end_row();
    term(0, 4, one); term(0, 2, one); term(0, 0, top); term(1, 0, one); term(2, 1, one); end_row();
    s.point();
    return s;
}

void matrices(int which, const std::string &dir)
{
    const U256 p = MODULI[which];
    frw::FieldDerived d;
    if (!frw::field_derive(p.l, &d)) { CHECK(false, "%s: refused", NAMES[which]); return; }
    U256 pm1 = p;
    pm1.l[0] -= 1;
    Csr ok = cubic(pm1);
    frw::FieldMatrices fm;
    std::string why = frw::r1csf_from_csr(d, ok.counts, ok.rp, ok.cp, ok.vp, &fm);
    CHECK(why.empty(), "%s: p - 1 refused: %s", NAMES[which], why.c_str());
    CHECK(fm.val[0] == ok.val[0] && fm.col[0] == ok.col[0] && fm.row_ptr[0] == ok.ptr[0], "%s: the arrays are not kept as they came", NAMES[which]);
    Csr bad = cubic(p);
    frw::FieldMatrices none;
    why = frw::r1csf_from_csr(d, bad.counts, bad.rp, bad.cp, bad.vp, &none);
    CHECK(why.find("matrix A, row 2") != std::string::npos && why.find("modulus") != std::string::npos, "%s: p gives \"%s\"", NAMES[which], why.c_str());
    bad = cubic(pm1);
    bad.col[1][1] = 5;
    why = frw::r1csf_from_csr(d, bad.counts, bad.rp, bad.cp, bad.vp, &none);
    CHECK(why.find("matrix B, row 1") != std::string::npos, "%s: a column beyond the variables gives \"%s\"", NAMES[which], why.c_str());
    bad = cubic(pm1);
    bad.ptr[2][1] = 2; bad.ptr[2][2] = 1;
    why = frw::r1csf_from_csr(d, bad.counts, bad.rp, bad.cp, bad.vp, &none);
    CHECK(why.find("matrix C, row 1") != std::string::npos, "%s: a decreasing row_ptr gives \"%s\"", NAMES[which], why.c_str());
    bad = cubic(pm1);
    bad.counts[0] = 0;
    CHECK(!frw::r1csf_from_csr(d, bad.counts, bad.rp, bad.cp, bad.vp, &none).empty(), "%s: no instance variable: accepted", NAMES[which]);
    CHECK(!frw::r1csf_from_csr(d, ok.counts, ok.rp, ok.cp, nullptr, &none).empty(), "%s: a null array: accepted", NAMES[which]);
    // the file: written, read back, and one byte short
    const std::string path = dir + "/cubic_" + std::to_string(which) + ".r1cs";
    CHECK(frw::r1csf_write(fm, path.c_str()), "%s: cannot write %s", NAMES[which], path.c_str());
    frw::FieldMatrices back;
    why = frw::r1csf_from_file(d, path.c_str(), &back);
    CHECK(why.empty() && back.num_instance == 2 && back.num_witness == 3 && back.num_constraints == 3, "%s: the file does not come back: %s", NAMES[which],
          why.c_str());
    for (int m = 0; m < 3; m++)
        CHECK(back.row_ptr[m] == fm.row_ptr[m] && back.col[m] == fm.col[m] && back.val[m] == fm.val[m], "%s: matrix %d differs after the round trip",
              NAMES[which], m);
    std::vector<uint8_t> bytes;
    {
        FILE *f = fopen(path.c_str(), "rb");
        if (f) {
            fseek(f, 0, SEEK_END);
            bytes.resize((size_t)ftell(f));
            fseek(f, 0, SEEK_SET);
            if (fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) bytes.clear();
            fclose(f);
        }
    }
    CHECK(bytes.size() == 8 + 48 + 3 * 4 * 8 + (5 + 3 + 3) * 36, "%s: the file has %zu bytes", NAMES[which], bytes.size());
    if (!bytes.empty()) {
        const std::string cut = dir + "/cut_" + std::to_string(which) + ".r1cs";
        FILE *f = fopen(cut.c_str(), "wb");
        if (f) {
            fwrite(bytes.data(), 1, bytes.size() - 1, f);
            fclose(f);
        }
        CHECK(!frw::r1csf_from_file(d, cut.c_str(), &none).empty(), "%s: a file one byte short: accepted", NAMES[which]);
    }
    CHECK(!frw::r1csf_from_file(d, (dir + "/absent.r1cs").c_str(), &none).empty(), "%s: a file that is not there: accepted", NAMES[which]);
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s <directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    // the moduli frw_field_info refuses are refused here too
    {
        frw::FieldDerived d;
        const U256 even{{2, 0, 0, (uint64_t)1 << 40}}, low{{~(uint64_t)0, ~(uint64_t)0, 0xffffffffULL, 0}}, high{{1, 0, 0, (uint64_t)1 << 63}};
        CHECK(!frw::field_derive(even.l, &d) && !frw::field_derive(low.l, &d) && !frw::field_derive(high.l, &d), "an inadmissible modulus is taken");
    }
    lifts();
    for (int which = 0; which < 5; which++) {
        arithmetic(which);
        lifted_systems(which);
        matrices(which, dir);
    }
    printf("%d checks, %d failed\n", cases, failures);
    if (failures) return 1;
    printf("r1cs_field_host: clean\n");
    return 0;
}
