// frw_r1cs_field.h -- a constraint system over ANY four-limb field (frw_field.h's rule: odd, 2^160 < p < 2^255), the modulus
// given at run time: what frw_r1csf_* of include/frw.h stands on.  Three parts.
//   * arithmetic, host and device: field_mul (eight CIOS rounds of frw_field.h and one conditional subtraction), field_add,
//     field_sub -- all on the 8 x 32-bit Montgomery form x 2^256 mod p, canonical in and out.
//   * what the kernels of frw_r1cs_field.hip read (R1csfDev).
//   * host only: the matrices over p.  Every coefficient of the three Falcon circuits is an INTEGER (+-1, powers of two, +-q,
//     twiddle products, the ladder offsets; the inverses of the dual and schoolbook circuits are witness values), so the matrices
//     over p are the centred lift of the ones the host mirror emits over BLS12-381's r -- v > r / 2 ? v - r : v -- reduced mod p.
//     r1csf_lift does that and REFUSES a coefficient whose lift reaches 2^200: the premise would be broken (the largest the
//     circuits hold is 160 bits), and a wrong matrix must not pass silently.  r1csf_from_csr / r1csf_from_file take matrices
//     that come from anywhere, canonical mod p, under the framing rules of frw_r1cs_file.h.
// tests/cpp/test_r1cs_field_host.cpp builds this header with g++ (through tests/cpp/hip_host) under the sanitizers.
#pragma once
#include <stdint.h>
#include "frw_field.h"

namespace frw {

// a b / 2^256 mod p.  b < p (it is the K of field_cios_round); a is ANY 256-bit value: the rounds take it digit by digit.
__host__ __device__ __forceinline__ void field_mul(const FieldConsts &f, const uint32_t (&a)[8], const uint32_t (&b)[8], uint32_t (&out)[8])
{
    uint32_t T[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 8; i++) field_cios_round(T, a[i], b, f.p, f.ninv32);
    field_cond_sub_p(T, f.p, out);
}

// a + b mod p for a, b < p (a + b < 2 p < 2^256: the ninth limb stays zero)
__host__ __device__ __forceinline__ void field_add(const FieldConsts &f, const uint32_t (&a)[8], const uint32_t (&b)[8], uint32_t (&out)[8])
{
    uint32_t T[9];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a[j] + b[j] + c;
        T[j] = (uint32_t)x;
        c = (uint32_t)(x >> 32);
    }
    T[8] = 0;
    field_cond_sub_p(T, f.p, out);
}

// a - b mod p for a, b < p
__host__ __device__ __forceinline__ void field_sub(const FieldConsts &f, const uint32_t (&a)[8], const uint32_t (&b)[8], uint32_t (&out)[8])
{
    uint32_t d[8];
    uint32_t bw = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a[j] - b[j] - bw;
        d[j] = (uint32_t)x;
        bw = (uint32_t)(x >> 63);
    }
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)d[j] + (bw ? f.p[j] : 0u) + c;
        out[j] = (uint32_t)x;
        c = (uint32_t)(x >> 32);
    }
}

// ---- what the kernels read ------------------------------------------------------------------------------------------------------
// Rows of R1CSF_LONG_ROW terms and more (in one matrix) go to a wavefront each; everything shorter to a thread per constraint.
// 64: the row that fills every lane of a wavefront once -- below it a wavefront would idle lanes on one product apiece while
// a thread walks such a row in the time its neighbours walk theirs.
constexpr uint32_t R1CSF_LONG_ROW = 64;
constexpr int R1CSF_LONG_SIGS = 4;              // statements a long-row wavefront serves with one fetch of the coefficients
constexpr uint32_t R1CSF_PLUS_ONE = 1u, R1CSF_MINUS_ONE = 2u;      // a term's class, top two bits beside its column; 0: a product

struct R1csfMatrixDev {
    const uint64_t *row_ptr;       // [C + 1]
    const uint32_t *col_class;     // [nnz]     column | class << 30
    const uint32_t *val;           // [nnz][8]  c 2^256 mod p
};
struct R1csfLongRow { uint32_t matrix, row, first_chunk, num_chunks; };
struct R1csfDev {
    FieldConsts fc;                // by value with the rest, as a kernel argument: the modulus sits in scalar registers
    uint32_t r2[8];                // 2^512 mod p: field_mul(x, r2) = x 2^256 mod p
    uint32_t num_instance, num_witness, num_constraints, num_long;
    uint32_t num_long_vars, zs_stride;   // the variables the long rows read; words a statement's plain values take (a multiple of 8)
    R1csfMatrixDev m[3];
    const uint32_t *order;         // [C] rows by decreasing count of terms in their short matrices
    const uint8_t *long_mask;      // [C] bit m: the row is long in matrix m
    const uint32_t *long_slot;     // [3][C] -> index into long_rows
    const R1csfLongRow *long_rows; // [num_long]
    const uint32_t *long_col;      // [chunk][64]      column of the term lane l takes (padding: column 0, coefficient 0)
    const uint32_t *long_cidx;     // [chunk][64]      that column's place in long_vars
    const uint32_t *long_val;      // [chunk][8][64]   its coefficient, limb planes
    const uint32_t *long_vars;     // [num_long_vars]  the columns the long rows read, ascending (column 0 among them)
};
constexpr uint32_t R1CSF_NOT_SMALL = 0xffffffffu;      // in place of a plain value: the variable is no integer below 2^32 - 1

// The scratch of a system with long rows: the plain values of the variables they read, [statement][zs_stride] words, and (check
// only) the long rows' products, [statement][long row][8] words; with d_abc those go to their slots there.
inline size_t r1csf_scratch_bytes(const R1csfDev &r, size_t batch, bool with_abc)
{
    if (!r.num_long) return 0;
    return batch * ((size_t)r.zs_stride * 4 + (with_abc ? 0 : (size_t)r.num_long * 32));
}

}  // namespace frw

// ---- host only: the matrices over p ---------------------------------------------------------------------------------------------
#include <cstdio>
#include <string>
#include <vector>
#include "frw_r1cs_file.h"

namespace frw {

// the arrays of the FRWR1CS1 layout, values canonical mod the modulus they were made for
struct FieldMatrices {
    uint64_t num_instance = 0, num_witness = 0, num_constraints = 0;
    std::vector<uint64_t> row_ptr[3], val[3];       // val: four limbs a term
    std::vector<uint32_t> col[3];
    uint64_t nnz(int m) const { return col[m].size(); }
};

inline void field_words(const uint64_t l[4], uint32_t (&w)[8])
{
    for (int j = 0; j < 4; j++) { w[2 * j] = (uint32_t)l[j]; w[2 * j + 1] = (uint32_t)(l[j] >> 32); }
}
inline void field_limbs(const uint32_t (&w)[8], uint64_t l[4])
{
    for (int j = 0; j < 4; j++) l[j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
}

// The centred lift of a canonical residue mod BLS12-381's r: its magnitude and its sign.
struct LiftedCoef { uint64_t mag[4]; bool negative; };
inline LiftedCoef lift_centred(const uint64_t v[4])
{
    const uint64_t *r = host::Fr::P;
    // half = (r - 1) / 2; v > half  <=>  the lift is v - r < 0
    uint64_t half[4];
    for (int j = 0; j < 4; j++) half[j] = (r[j] >> 1) | (j < 3 ? r[j + 1] << 63 : 0);
    bool above = false;
    for (int j = 3; j >= 0; j--)
        if (v[j] != half[j]) { above = v[j] > half[j]; break; }
    LiftedCoef out;
    out.negative = above;
    if (!above) {
        for (int j = 0; j < 4; j++) out.mag[j] = v[j];
        return out;
    }
    uint64_t bw = 0;
    for (int j = 0; j < 4; j++) {
        const uint64_t d = r[j] - v[j], e = d - bw;
        bw = (uint64_t)(r[j] < v[j]) | (uint64_t)(d < bw);
        out.mag[j] = e;
    }
    return out;
}
inline bool lift_below_2_200(const LiftedCoef &c) { return (c.mag[3] >> 8) == 0; }

// +-mag as x 2^256 mod p; mag is any 256-bit integer (field_mul takes it digit by digit against 2^512 mod p)
inline void field_from_integer(const FieldDerived &d, const uint64_t mag[4], bool negative, uint32_t (&mont)[8])
{
    uint32_t a[8], m[8];
    field_words(mag, a);
    field_mul(d.fc, a, d.r2, m);
    bool zero = true;
    for (int j = 0; j < 8; j++) zero &= m[j] == 0;
    if (negative && !zero) {
        const uint32_t nought[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        field_sub(d.fc, nought, m, mont);
    } else {
        for (int j = 0; j < 8; j++) mont[j] = m[j];
    }
}
// x 2^256 mod p -> x, canonical
inline void field_to_canonical(const FieldDerived &d, const uint32_t (&mont)[8], uint64_t out[4])
{
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    uint32_t c[8];
    field_mul(d.fc, mont, one, c);
    field_limbs(c, out);
}

// The host mirror's matrices (over r) -> the same system over p.  The empty string, or the refusal: the matrix and the row of a
// coefficient whose centred lift reaches 2^200.
inline std::string r1csf_lift(const host::ConstraintMatrices &m, const FieldDerived &d, FieldMatrices *out)
{
    FieldMatrices fm;
    fm.num_instance = m.num_instance_variables;
    fm.num_witness = m.num_witness_variables;
    fm.num_constraints = m.num_constraints;
    const std::vector<host::ConstraintMatrices::Row> *src[3] = {&m.a, &m.b, &m.c};
    const char names[3] = {'A', 'B', 'C'};
    for (int k = 0; k < 3; k++) {
        fm.row_ptr[k].reserve(src[k]->size() + 1);
        fm.row_ptr[k].push_back(0);
        for (size_t row = 0; row < src[k]->size(); row++) {
            for (const auto &t : (*src[k])[row]) {
                uint64_t v[4], c[4];
                t.first.to_canonical(v);
                const LiftedCoef l = lift_centred(v);
                if (!lift_below_2_200(l))
                    return std::string("matrix ") + names[k] + ", row " + std::to_string(row) +
                           ": a coefficient is no small integer (its centred lift reaches 2^200), so the system does not carry over to another field";
                uint32_t mont[8];
                field_from_integer(d, l.mag, l.negative, mont);
                field_to_canonical(d, mont, c);
                fm.col[k].push_back(t.second);
                fm.val[k].insert(fm.val[k].end(), c, c + 4);
            }
            fm.row_ptr[k].push_back(fm.col[k].size());
        }
    }
    *out = std::move(fm);
    return std::string();
}

// Matrices that come from anywhere: frw_r1cs_file.h's framing rules, a column >= I + W, and a value >= the modulus.
inline std::string r1csf_from_csr(const FieldDerived &d, const uint64_t counts[6], const uint64_t *const row_ptr[3], const uint32_t *const col[3],
                                  const uint64_t *const val[3], FieldMatrices *out)
{
    if (!out) return "null pointer";
    const std::string framing = r1cs_csr_framing(counts, row_ptr, col, val);
    if (!framing.empty()) return framing;
    const uint64_t I = counts[0], W = counts[1], C = counts[2];
    uint64_t p[4];
    field_limbs(d.fc.p, p);
    const char names[3] = {'A', 'B', 'C'};
    auto at = [&](int m, uint64_t row, const char *what) {
        return std::string("matrix ") + names[m] + ", row " + std::to_string(row) + ": " + what;
    };
    FieldMatrices fm;
    fm.num_instance = I;
    fm.num_witness = W;
    fm.num_constraints = C;
    for (int m = 0; m < 3; m++) {
        for (uint64_t r = 0; r < C; r++)
            for (uint64_t t = row_ptr[m][r]; t < row_ptr[m][r + 1]; t++) {
                if (col[m][t] >= I + W) return at(m, r, "column beyond the variables");
                const uint64_t *v = val[m] + 4 * t;
                bool below = false;
                for (int k = 3; k >= 0; k--)
                    if (v[k] != p[k]) { below = v[k] < p[k]; break; }
                if (!below) return at(m, r, "coefficient not below the modulus");
            }
        fm.row_ptr[m].assign(row_ptr[m], row_ptr[m] + C + 1);
        fm.col[m].assign(col[m], col[m] + counts[3 + m]);
        fm.val[m].assign(val[m], val[m] + 4 * counts[3 + m]);
    }
    *out = std::move(fm);
    return std::string();
}

inline std::string r1csf_from_file(const FieldDerived &d, const char *path, FieldMatrices *out)
{
    if (!path || !out) return "null pointer";
    R1csFileArrays arr;
    const std::string refusal = r1cs_read_file(path, &arr);
    if (!refusal.empty()) return refusal;
    const uint64_t *rp[3] = {arr.ptr[0].data(), arr.ptr[1].data(), arr.ptr[2].data()};
    const uint32_t *cp[3] = {arr.col[0].data(), arr.col[1].data(), arr.col[2].data()};
    const uint64_t *vp[3] = {arr.val[0].data(), arr.val[1].data(), arr.val[2].data()};
    return r1csf_from_csr(d, arr.counts, rp, cp, vp, out);
}

// the FRWR1CS1 file (the file does not record the modulus)
inline bool r1csf_write(const FieldMatrices &m, const char *path)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const uint64_t hdr[6] = {m.num_instance, m.num_witness, m.num_constraints, m.nnz(0), m.nnz(1), m.nnz(2)};
    bool ok = std::fwrite("FRWR1CS1", 1, 8, f) == 8 && std::fwrite(hdr, 8, 6, f) == 6;
    for (int k = 0; k < 3 && ok; k++)
        ok = std::fwrite(m.row_ptr[k].data(), 8, m.row_ptr[k].size(), f) == m.row_ptr[k].size() &&
             (m.col[k].empty() || std::fwrite(m.col[k].data(), 4, m.col[k].size(), f) == m.col[k].size()) &&
             (m.val[k].empty() || std::fwrite(m.val[k].data(), 8, m.val[k].size(), f) == m.val[k].size());
    return std::fclose(f) == 0 && ok;
}

// the host mirror's matrices of a Falcon circuit (frw_r1cs.cpp)
host::ConstraintMatrices r1cs_build_matrices(int circuit, int logn);

}  // namespace frw

// ---- the handle and the launch sequence, for the units that stand on them (frw_r1cs_field.hip, frw_qap_field.hip) --------------------
#ifdef __HIPCC__
struct frw_r1csf {
    int device = 0;
    frw::FieldDerived field{};
    frw::R1csfDev dev{};
    uint64_t nnz[3] = {0, 0, 0};
    std::vector<void *> allocs;
};
namespace frw {
// batch <= 32768.  Everything on `st`, nothing allocated, no synchronisation; first / abc may be null.
hipError_t launch_r1csf_check(const R1csfDev &r, size_t batch, const uint64_t *witness, const uint64_t *instance, uint32_t *num_unsatisfied,
                              uint32_t *first_unsatisfied, uint64_t *abc, void *scratch, hipStream_t st);
}  // namespace frw
#endif
