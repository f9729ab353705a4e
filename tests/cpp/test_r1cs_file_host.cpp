// Test-only: the way in for a constraint system that comes as matrices (falcon-r1cs_amd/csrc/frw_r1cs_file.h), as a program of its
// own that tests/test_r1cs_file_host.py builds with -fsanitize=address,undefined and runs.  argv[1]: a directory to write in.
//   round trip    frw_r1cs_export(FRW_CIRCUIT_NTT, 9) -> r1cs_from_file -> ConstraintMatrices::write gives the same bytes
//   refusals      every one frw.h lists, one case each, with the matrix and the row in the message; files one byte short and one long
//   acceptance    a repeated column, a zero coefficient, an empty row, an unused variable, unsorted columns
//   the library   frw_r1cs_load_csr / frw_r1cs_load_file on device -1 (no machine has it, so the answer is the same with a GPU and
//                 without): malformed -> FRW_E_INVALID_ARG and frw_last_error() says where, well formed -> FRW_E_NO_DEVICE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "frw_r1cs_file.h"

namespace {
int failures = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            printf("FAILED %s: ", #cond);               \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            failures++;                                 \
        }                                               \
    } while (0)

using frw::host::ConstraintMatrices;
using frw::host::Fr;

std::vector<uint8_t> slurp(const std::string &path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    v.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (!v.empty() && fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}
void spit(const std::string &path, const uint8_t *p, size_t n)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { printf("cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

// a system as the callers' arrays, each exactly as long as it is said to be
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
    std::string parse(ConstraintMatrices *out) { return frw::r1cs_from_csr(counts, rp, cp, vp, out); }
    std::vector<uint8_t> file() const
    {
        std::vector<uint8_t> f(8 + 48);
        memcpy(f.data(), "FRWR1CS1", 8);
        memcpy(f.data() + 8, counts, 48);
        auto put = [&](const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; f.insert(f.end(), b, b + n); };
        for (int m = 0; m < 3; m++) { put(ptr[m].data(), ptr[m].size() * 8); put(col[m].data(), col[m].size() * 4); put(val[m].data(), val[m].size() * 8); }
        return f;
    }
};

// x^3 + x + 5 = y with y public: I = 2 (one, y), W = 3 (x, x^2, x^3), three constraints
//   x * x = x2;   x2 * x = x3;   (x3 + x + 5) * 1 = y
Csr cubic()
{
    Csr s{};
    s.counts[0] = 2; s.counts[1] = 3; s.counts[2] = 3;
    auto term = [&](int m, uint32_t c, uint64_t v) { s.col[m].push_back(c); s.val[m].insert(s.val[m].end(), {v, 0, 0, 0}); };
    for (int m = 0; m < 3; m++) s.ptr[m].push_back(0);
    auto end_row = [&]() { for (int m = 0; m < 3; m++) s.ptr[m].push_back(s.col[m].size()); };
    term(0, 2, 1); term(1, 2, 1); term(2, 3, 1); end_row();
    term(0, 3, 1); term(1, 2, 1); term(2, 4, 1); end_row();
    term(0, 4, 1); term(0, 2, 1); term(0, 0, 5); term(1, 0, 1); term(2, 1, 1); end_row();
    s.point();
    return s;
}

void expect_refusal(const char *what, Csr s, const char *needle)
{
    s.point();
    ConstraintMatrices m;
    const std::string why = s.parse(&m);
    CHECK(!why.empty(), "%s: accepted", what);
    CHECK(why.find(needle) != std::string::npos, "%s: the message is \"%s\", without \"%s\"", what, why.c_str(), needle);
    frw_r1cs *h = (frw_r1cs *)&failures;
    const int rc = frw_r1cs_load_csr(-1, s.counts, s.rp, s.cp, s.vp, &h);
    CHECK(rc == FRW_E_INVALID_ARG && h == nullptr, "%s: the library returns %d", what, rc);
    CHECK(strstr(frw_last_error(), needle) != nullptr, "%s: frw_last_error() is \"%s\"", what, frw_last_error());
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s <directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int cases = 0;

    // ---- round trip of the Falcon-512 export --------------------------------------------------------------------------------------
    {
        const std::string a = dir + "/ntt9.r1cs", b = dir + "/ntt9.again.r1cs";
        uint64_t counts[6];
        CHECK(frw_r1cs_export(FRW_CIRCUIT_NTT, 9, a.c_str(), counts) == FRW_OK, "export");
        ConstraintMatrices m;
        const std::string why = frw::r1cs_from_file(a.c_str(), &m);
        CHECK(why.empty(), "the export is refused: %s", why.c_str());
        CHECK(m.num_instance_variables == counts[0] && m.num_witness_variables == counts[1] && m.num_constraints == counts[2] &&
              m.non_zero(m.a) == counts[3] && m.non_zero(m.b) == counts[4] && m.non_zero(m.c) == counts[5], "counts");
        CHECK(m.write(b.c_str()), "write");
        const std::vector<uint8_t> fa = slurp(a), fb = slurp(b);
        CHECK(!fa.empty() && fa == fb, "parse -> write changed the file (%zu against %zu bytes)", fa.size(), fb.size());
        frw_r1cs *h = (frw_r1cs *)&failures;
        CHECK(frw_r1cs_load_file(-1, a.c_str(), &h) == FRW_E_NO_DEVICE && h == nullptr, "the export on device -1");
        remove(a.c_str());
        remove(b.c_str());
        cases++;
    }

    // ---- the small system: accepted, round trip, files of the wrong length ----------------------------------------------------------
    const Csr good = cubic();
    {
        Csr s = good;
        s.point();
        ConstraintMatrices m;
        const std::string why = s.parse(&m);
        CHECK(why.empty(), "the cubic is refused: %s", why.c_str());
        const Fr x = Fr::from(3), one = Fr::one();
        CHECK(m.is_satisfied({one, Fr::from(35)}, {x, x * x, x * x * x}), "3^3 + 3 + 5 = 35");
        CHECK(!m.is_satisfied({one, Fr::from(36)}, {x, x * x, x * x * x}), "... and not 36");
        const std::vector<uint8_t> f = s.file();
        const std::string p = dir + "/cubic.r1cs", q = dir + "/cubic.again.r1cs";
        spit(p, f.data(), f.size());
        ConstraintMatrices again;
        CHECK(frw::r1cs_from_file(p.c_str(), &again).empty() && again.write(q.c_str()) && slurp(q) == f, "the cubic's file does not come back");
        frw_r1cs *h = (frw_r1cs *)&failures;
        CHECK(frw_r1cs_load_file(-1, p.c_str(), &h) == FRW_E_NO_DEVICE && h == nullptr, "a well-formed file on device -1");
        h = (frw_r1cs *)&failures;
        CHECK(frw_r1cs_load_csr(-1, s.counts, s.rp, s.cp, s.vp, &h) == FRW_E_NO_DEVICE && h == nullptr, "well-formed arrays on device -1");
        // one byte short, one byte long, another magic, no file at all
        std::vector<uint8_t> longer = f;
        longer.push_back(0);
        std::vector<uint8_t> magic = f;
        magic[7] = '2';
        const struct { const char *what; const uint8_t *p; size_t n; } bad[] = {
            {"one byte short", f.data(), f.size() - 1}, {"one byte long", longer.data(), longer.size()}, {"another magic", magic.data(), magic.size()},
            {"header only", f.data(), 56}, {"half a header", f.data(), 20}, {"empty", f.data(), 0}};
        for (const auto &b : bad) {
            spit(p, b.p, b.n);
            ConstraintMatrices mm;
            CHECK(!frw::r1cs_from_file(p.c_str(), &mm).empty(), "%s: accepted", b.what);
            h = (frw_r1cs *)&failures;
            CHECK(frw_r1cs_load_file(-1, p.c_str(), &h) == FRW_E_INVALID_ARG && h == nullptr, "%s: the library", b.what);
            cases++;
        }
        // a header whose counts no file could hold
        {
            std::vector<uint8_t> lie = f;
            const uint64_t huge = ~(uint64_t)0 / 36;
            memcpy(lie.data() + 8 + 8 * 3, &huge, 8);
            spit(p, lie.data(), lie.size());
            ConstraintMatrices mm;
            CHECK(!frw::r1cs_from_file(p.c_str(), &mm).empty(), "a header that lies: accepted");
            cases++;
        }
        remove(p.c_str());
        remove(q.c_str());
        h = (frw_r1cs *)&failures;
        CHECK(frw_r1cs_load_file(-1, p.c_str(), &h) == FRW_E_INVALID_ARG && h == nullptr, "a file that is not there");
        CHECK(frw_r1cs_load_file(-1, nullptr, &h) == FRW_E_INVALID_ARG, "no path");
        CHECK(frw_r1cs_load_file(-1, p.c_str(), nullptr) == FRW_E_INVALID_ARG, "no out");
        cases += 3;
    }

    // ---- refusals, one case each ------------------------------------------------------------------------------------------------------
    {
        Csr s = good; s.counts[0] = 0; expect_refusal("I == 0", s, "instance");
        s = good; s.counts[2] = 0; expect_refusal("C == 0", s, "no constraint");
        s = good; s.counts[1] = ((uint64_t)1 << 30) - 2; expect_refusal("I + W == 2^30", s, "2^30 variables");
        s = good; s.counts[0] = ((uint64_t)1 << 30) - 2; s.counts[1] = 0; expect_refusal("C + I > 2^30", s, "2^30 domain");
        s = good; s.ptr[1][0] = 1; expect_refusal("row_ptr[B][0] != 0", s, "matrix B, row 0");
        s = good; s.ptr[0][1] = 3; expect_refusal("row_ptr[A] decreases", s, "matrix A, row 1");        // 0, 3 (was 1), 2, 5
        s = good; s.ptr[2][3] = 2; expect_refusal("row_ptr[C][C] != nnz", s, "matrix C, row 2");
        s = good; s.col[0][1] = 5; expect_refusal("column == I + W", s, "matrix A, row 1");
        s = good; memcpy(&s.val[2][4], Fr::P, 32); expect_refusal("value == the group order", s, "matrix C, row 1");
        s = good; s.val[1][3] = ~(uint64_t)0; expect_refusal("value of 256 bits", s, "matrix B, row 0");
        cases += 10;
        // null pointers (the arrays as they are, one pointer taken away)
        s = good;
        s.point();
        frw_r1cs *h = nullptr;
        ConstraintMatrices m;
        for (int which = 0; which < 3; which++)
            for (int mtx = 0; mtx < 3; mtx++) {
                const uint64_t *rp[3] = {s.rp[0], s.rp[1], s.rp[2]}, *vp[3] = {s.vp[0], s.vp[1], s.vp[2]};
                const uint32_t *cp[3] = {s.cp[0], s.cp[1], s.cp[2]};
                if (which == 0) rp[mtx] = nullptr; else if (which == 1) cp[mtx] = nullptr; else vp[mtx] = nullptr;
                CHECK(!frw::r1cs_from_csr(s.counts, rp, cp, vp, &m).empty(), "null array %d of matrix %d: accepted", which, mtx);
                CHECK(frw_r1cs_load_csr(-1, s.counts, rp, cp, vp, &h) == FRW_E_INVALID_ARG, "null array %d of matrix %d: the library", which, mtx);
            }
        CHECK(frw_r1cs_load_csr(-1, nullptr, s.rp, s.cp, s.vp, &h) == FRW_E_INVALID_ARG, "no counts");
        CHECK(frw_r1cs_load_csr(-1, s.counts, nullptr, s.cp, s.vp, &h) == FRW_E_INVALID_ARG, "no row_ptr");
        CHECK(frw_r1cs_load_csr(-1, s.counts, s.rp, nullptr, s.vp, &h) == FRW_E_INVALID_ARG, "no col");
        CHECK(frw_r1cs_load_csr(-1, s.counts, s.rp, s.cp, nullptr, &h) == FRW_E_INVALID_ARG, "no val");
        CHECK(frw_r1cs_load_csr(-1, s.counts, s.rp, s.cp, s.vp, nullptr) == FRW_E_INVALID_ARG, "no out");
        cases += 14;
    }

    // ---- accepted on purpose ------------------------------------------------------------------------------------------------------------
    {
        // four constraints over I = 2, W = 5 (witness 4 is in no row):
        //   row 0: (x + x) * x = 2 x2          a column repeated in A
        //   row 1: (0 x3 + x2) * x = x3        a zero coefficient
        //   row 2: () * () = ()                an empty row
        //   row 3: (5 + x + x3) * 1 = y        columns out of order
        Csr s{};
        s.counts[0] = 2; s.counts[1] = 5; s.counts[2] = 4;
        auto term = [&](int m, uint32_t c, uint64_t v) { s.col[m].push_back(c); s.val[m].insert(s.val[m].end(), {v, 0, 0, 0}); };
        for (int m = 0; m < 3; m++) s.ptr[m].push_back(0);
        auto end_row = [&]() { for (int m = 0; m < 3; m++) s.ptr[m].push_back(s.col[m].size()); };
        term(0, 2, 1); term(0, 2, 1); term(1, 2, 1); term(2, 3, 2); end_row();
        term(0, 4, 0); term(0, 3, 1); term(1, 2, 1); term(2, 4, 1); end_row();
        end_row();
        term(0, 0, 5); term(0, 4, 1); term(0, 2, 1); term(1, 0, 1); term(2, 1, 1); end_row();
        s.point();
        ConstraintMatrices m;
        const std::string why = s.parse(&m);
        CHECK(why.empty(), "refused: %s", why.c_str());
        CHECK(m.a[0].size() == 2 && m.a[1].size() == 2 && m.a[2].empty() && m.b[2].empty() && m.c[2].empty(), "the terms are kept as they come");
        const Fr x = Fr::from(3), one = Fr::one();
        CHECK(m.is_satisfied({one, Fr::from(35)}, {x, x * x, x * x * x, Fr::from(99), Fr::from(7)}), "satisfied");
        const std::string p = dir + "/odd.r1cs", q = dir + "/odd.again.r1cs";
        const std::vector<uint8_t> f = s.file();
        spit(p, f.data(), f.size());
        ConstraintMatrices again;
        CHECK(frw::r1cs_from_file(p.c_str(), &again).empty() && again.write(q.c_str()) && slurp(q) == f, "its file does not come back byte for byte");
        frw_r1cs *h = (frw_r1cs *)&failures;
        CHECK(frw_r1cs_load_csr(-1, s.counts, s.rp, s.cp, s.vp, &h) == FRW_E_NO_DEVICE && h == nullptr, "the library on device -1");
        // a matrix without a single term: its arrays may be null
        Csr e{};
        e.counts[0] = 1; e.counts[1] = 0; e.counts[2] = 1;
        for (int k = 0; k < 3; k++) e.ptr[k] = {0, 0};
        e.point();
        for (int k = 0; k < 3; k++) { e.cp[k] = nullptr; e.vp[k] = nullptr; }
        CHECK(frw::r1cs_from_csr(e.counts, e.rp, e.cp, e.vp, &m).empty(), "one empty row, nothing else: refused");
        remove(p.c_str());
        remove(q.c_str());
        cases += 2;
    }

    printf("%d cases\n", cases);
    if (failures) { printf("r1cs_file_host: %d FAILURES\n", failures); return 1; }
    printf("r1cs_file_host: clean\n");
    return 0;
}
