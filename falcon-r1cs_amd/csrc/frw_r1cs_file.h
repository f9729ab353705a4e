// frw_r1cs_file.h -- a constraint system that comes in as matrices: the arrays of the FRWR1CS1 file (host/frw_host.hpp
// ConstraintMatrices::write is the inverse), from host memory or from a file, validated and turned into ConstraintMatrices.
// What frw_r1cs_load_csr / frw_r1cs_load_file do before they touch the device.  Host code only, nothing of the HIP runtime is
// called: tests/cpp/test_r1cs_file_host.cpp runs it under the sanitizers.
//
// Accepted on purpose: unsorted columns, a column repeated within a row (the terms add), zero coefficients, empty rows, variables
// no row mentions.  The terms are kept as they come -- not sorted, merged or dropped -- so parse -> write gives the bytes back.
// Refused, with the matrix and the row in the message: see r1cs_from_csr.
#pragma once
#include <stdint.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "host/frw_host.hpp"

namespace frw {

constexpr uint64_t R1CS_MAX_VARIABLES = (uint64_t)1 << 30;     // I + W below it (the kernels keep two flag bits beside a column)
constexpr uint64_t R1CS_MAX_DOMAIN = (uint64_t)1 << 30;        // C + I at most it (QAP_MAX_LOG_N)

// The framing of the arrays, before any term is looked at: the empty string, or what is wrong (shared with frw_r1cs_field.h, whose
// values are checked against another modulus).
inline std::string r1cs_csr_framing(const uint64_t counts[6], const uint64_t *const row_ptr[3], const uint32_t *const col[3],
                                    const uint64_t *const val[3])
{
    if (!counts || !row_ptr || !col || !val) return "null pointer";
    const uint64_t I = counts[0], W = counts[1], C = counts[2];
    if (I == 0) return "no instance variable: column 0, the constant one, is one";
    if (C == 0) return "no constraint";
    if (I >= R1CS_MAX_VARIABLES || W >= R1CS_MAX_VARIABLES || I + W >= R1CS_MAX_VARIABLES) return "2^30 variables or more";
    if (C > R1CS_MAX_DOMAIN || C + I > R1CS_MAX_DOMAIN) return "constraints + instance variables beyond the 2^30 domain";
    const char names[3] = {'A', 'B', 'C'};
    auto at = [&](int m, uint64_t row, const char *what) {
        return std::string("matrix ") + names[m] + ", row " + std::to_string(row) + ": " + what;
    };
    for (int m = 0; m < 3; m++) {
        const uint64_t nnz = counts[3 + m];
        if (!row_ptr[m] || (nnz && (!col[m] || !val[m]))) return std::string("matrix ") + names[m] + ": null pointer";
        if (row_ptr[m][0] != 0) return at(m, 0, "row_ptr does not start at 0");
        for (uint64_t r = 0; r < C; r++)
            if (row_ptr[m][r + 1] < row_ptr[m][r]) return at(m, r, "row_ptr decreases");
        if (row_ptr[m][C] != nnz) return at(m, C - 1, "row_ptr does not end at the matrix's count of terms");
    }
    return std::string();
}

// counts = {I, W, C, nnz_A, nnz_B, nnz_C}; row_ptr[m] u64[C + 1], col[m] u32[nnz_m], val[m] u64[nnz_m][4] canonical.
// Returns the empty string and fills *out, or says what is wrong: a null pointer; I == 0 or C == 0; I + W >= 2^30 or
// C + I > 2^30; row_ptr[m][0] != 0, a decreasing row_ptr, row_ptr[m][C] != nnz_m; a column >= I + W; a value >= the group order.
inline std::string r1cs_from_csr(const uint64_t counts[6], const uint64_t *const row_ptr[3], const uint32_t *const col[3],
                                 const uint64_t *const val[3], host::ConstraintMatrices *out)
{
    using host::Fr;
    if (!out) return "null pointer";
    const std::string framing = r1cs_csr_framing(counts, row_ptr, col, val);
    if (!framing.empty()) return framing;
    const uint64_t I = counts[0], W = counts[1], C = counts[2];
    const char names[3] = {'A', 'B', 'C'};
    auto at = [&](int m, uint64_t row, const char *what) {
        return std::string("matrix ") + names[m] + ", row " + std::to_string(row) + ": " + what;
    };
    host::ConstraintMatrices cm;
    cm.num_instance_variables = (size_t)I;
    cm.num_witness_variables = (size_t)W;
    cm.num_constraints = (size_t)C;
    std::vector<host::ConstraintMatrices::Row> *dst[3] = {&cm.a, &cm.b, &cm.c};
    for (int m = 0; m < 3; m++) {
        dst[m]->resize((size_t)C);
        for (uint64_t r = 0; r < C; r++) {
            host::ConstraintMatrices::Row &row = (*dst[m])[(size_t)r];
            row.reserve((size_t)(row_ptr[m][r + 1] - row_ptr[m][r]));
            for (uint64_t t = row_ptr[m][r]; t < row_ptr[m][r + 1]; t++) {
                if (col[m][t] >= I + W) return at(m, r, "column beyond the variables");
                const uint64_t *v = val[m] + 4 * t;
                bool below = false;                                        // v < the group order, from the top limb down
                for (int k = 3; k >= 0; k--) {
                    if (v[k] != Fr::P[k]) { below = v[k] < Fr::P[k]; break; }
                }
                if (!below) return at(m, r, "coefficient not below the group order");
                row.emplace_back(Fr::from_canonical(v), col[m][t]);
            }
        }
    }
    *out = std::move(cm);
    return std::string();
}

// the arrays of an FRWR1CS1 file, its length checked against its header; nothing of the values is looked at
struct R1csFileArrays {
    uint64_t counts[6];
    std::vector<uint64_t> ptr[3], val[3];
    std::vector<uint32_t> col[3];
};
inline std::string r1cs_read_file(const char *path, R1csFileArrays *arr)
{
    if (!path || !arr) return "null pointer";
    FILE *f = std::fopen(path, "rb");
    if (!f) return std::string("cannot open ") + path;
    struct Closer { FILE *f; ~Closer() { std::fclose(f); } } closer{f};
    char magic[8];
    uint64_t *counts = arr->counts;
    if (std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, "FRWR1CS1", 8) != 0) return "not an FRWR1CS1 file";
    if (std::fread(counts, 8, 6, f) != 6) return "the header is cut short";
    if (std::fseek(f, 0, SEEK_END) != 0) return "cannot seek";
    const long end = std::ftell(f);
    if (end < 56 || std::fseek(f, 56, SEEK_SET) != 0) return "cannot seek";
    const uint64_t body = (uint64_t)end - 56, C = counts[2];
    // every count against the length first: no product below can overflow, and nothing is allocated for a header that lies
    uint64_t want = 0;
    if (C >= body / 8) return "the file's length is not what its header implies";
    for (int m = 0; m < 3; m++) {
        if (counts[3 + m] > body / 36) return "the file's length is not what its header implies";
        want += 8 * (C + 1) + 36 * counts[3 + m];
    }
    if (want != body) return "the file's length is not what its header implies";
    for (int m = 0; m < 3; m++) {
        const size_t nnz = (size_t)counts[3 + m];
        arr->ptr[m].resize((size_t)C + 1);
        arr->col[m].resize(nnz);
        arr->val[m].resize(4 * nnz);
        if (std::fread(arr->ptr[m].data(), 8, arr->ptr[m].size(), f) != arr->ptr[m].size() || std::fread(arr->col[m].data(), 4, nnz, f) != nnz ||
            std::fread(arr->val[m].data(), 8, 4 * nnz, f) != 4 * nnz)
            return "the file is cut short";
    }
    return std::string();
}

// The FRWR1CS1 file: "FRWR1CS1", u64 counts[6], then per matrix row_ptr | col | val.  Refused as well: a file that cannot be opened,
// another magic, a length that is not exactly what the header implies.
inline std::string r1cs_from_file(const char *path, host::ConstraintMatrices *out)
{
    if (!path || !out) return "null pointer";
    R1csFileArrays arr;
    const std::string refusal = r1cs_read_file(path, &arr);
    if (!refusal.empty()) return refusal;
    // (a matrix without terms: its empty vectors' data() may be null, which the check accepts where there is no term)
    const uint64_t *rp[3] = {arr.ptr[0].data(), arr.ptr[1].data(), arr.ptr[2].data()};
    const uint32_t *cp[3] = {arr.col[0].data(), arr.col[1].data(), arr.col[2].data()};
    const uint64_t *vp[3] = {arr.val[0].data(), arr.val[1].data(), arr.val[2].data()};
    return r1cs_from_csr(arr.counts, rp, cp, vp, out);
}

}  // namespace frw
