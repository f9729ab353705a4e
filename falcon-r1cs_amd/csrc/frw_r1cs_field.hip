// frw_r1cs_field.hip -- frw_r1csf_*: the satisfaction check and A z, B z, C z of a constraint system over a four-limb field given
// at run time (frw_r1cs_field.h: the arithmetic, the device structures, the matrices over p).  frw_r1cs_check.hip is the same
// check with BLS12-381's modulus compiled in -- its 29-bit limbs and flattened rows encode that modulus and do not carry over;
// what does is the split of the work: rows of R1CSF_LONG_ROW terms and more (the 2 N + 1 dense N-term rows of the NTT circuits,
// the N rows of N + 2 terms of schoolbook) take a wavefront each, everything else a thread per constraint, rows visited by
// decreasing length.  A product is eight CIOS rounds with the modulus in scalar registers (FieldConsts rides in the kernel
// argument); a coefficient +1 or -1 is an addition; and in a long row a variable that is a small integer -- every one the Falcon
// circuits' long rows read -- is multiplied in as that integer, one multiply-add per limb.
//
// One launch sequence, on one stream, nothing allocated: r1csf_init_kernel (the counts, and the verdict on instance[0]) ->
// r1csf_zsmall_kernel, r1csf_long_rows_kernel (if the system has long rows) -> r1csf_eval_kernel.  Counts are integer atomicAdds and the first
// violated row an atomicMin, one of each per wavefront: no result depends on the grid or on scheduling.
//
// A statement whose instance[0] is not 2^256 mod p (a refused, zero-filled slot of the witness calls; a buffer in another
// encoding) is reported as violating every row, first row 0, and its products are zeros: none of its rows is evaluated -- a zero
// assignment would satisfy them all.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <exception>
#include <memory>
#include <new>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_r1cs_field.h"
#include "frw_stage.h"

namespace frw {
namespace {

struct F8 { uint32_t l[8]; };

__device__ __forceinline__ F8 f8_load(const uint32_t *__restrict__ p)
{
    const uint4 lo = ((const uint4 *)p)[0], hi = ((const uint4 *)p)[1];
    return F8{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}
__device__ __forceinline__ void f8_store(uint32_t *p, const F8 &v)
{
    ((uint4 *)p)[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    ((uint4 *)p)[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ F8 f8_zero()
{
    return F8{{0, 0, 0, 0, 0, 0, 0, 0}};
}

// column -> its value in one statement's vectors (column 0 is instance[0], which the kernels have checked to be one)
__device__ __forceinline__ const uint32_t *var_ptr(uint32_t col, uint32_t num_instance, const uint32_t *__restrict__ wit,
                                                   const uint32_t *__restrict__ inst)
{
    return col >= num_instance ? wit + (size_t)(col - num_instance) * 8 : inst + (size_t)col * 8;
}

// instance[0] == 2^256 mod p
__device__ __forceinline__ bool leads_with_one(const FieldConsts &fc, const uint32_t *__restrict__ inst)
{
    const F8 v = f8_load(inst);
    bool eq = true;
#pragma unroll
    for (int k = 0; k < 8; k++) eq &= v.l[k] == fc.one[k];
    return eq;
}

__device__ __forceinline__ uint32_t *product_slot(uint32_t *abc, size_t sig, uint32_t num_constraints, uint32_t matrix, uint32_t row)
{
    return abc + ((sig * 3 + matrix) * (size_t)num_constraints + row) * 8;
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void r1csf_init_kernel(R1csfDev r, size_t batch, const uint32_t *__restrict__ inst, uint32_t *__restrict__ num,
                                                           uint32_t *__restrict__ first)
{
    const size_t sig = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (sig >= batch) return;
    const bool ok = leads_with_one(r.fc, inst + sig * (size_t)r.num_instance * 8);
    num[sig] = ok ? 0u : r.num_constraints;
    if (first) first[sig] = ok ? 0xffffffffu : 0u;
}

// The plain value of every variable the long rows read -- field_mul(z R, 1) = z -- where it is an integer below 2^32 - 1, else
// R1CSF_NOT_SMALL.  In the Falcon circuits the long rows read polynomial coefficients, all below q.
__global__ __launch_bounds__(BLOCK) void r1csf_zsmall_kernel(R1csfDev r, size_t batch, const uint32_t *__restrict__ wit,
                                                             const uint32_t *__restrict__ inst, uint32_t *__restrict__ zs)
{
    const size_t sig = blockIdx.y;
    const uint32_t u = blockIdx.x * BLOCK + threadIdx.x;
    if (sig >= batch || u >= r.num_long_vars) return;
    const F8 z = f8_load(var_ptr(r.long_vars[u], r.num_instance, wit + sig * (size_t)r.num_witness * 8, inst + sig * (size_t)r.num_instance * 8));
    const uint32_t unit[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    F8 plain;
    field_mul(r.fc, z.l, unit, plain.l);
    uint32_t hi = 0;
#pragma unroll
    for (int k = 1; k < 8; k++) hi |= plain.l[k];
    zs[sig * r.zs_stride + u] = hi == 0 && plain.l[0] != R1CSF_NOT_SMALL ? plain.l[0] : R1CSF_NOT_SMALL;
}

// One wavefront per (long row, group of R1CSF_LONG_SIGS statements): lane l takes terms l, l + 64, ... -- a coefficient is
// fetched once and serves every statement of the group.  A term is (c R) z with z the PLAIN value from r1csf_zsmall_kernel: one
// multiply-add per limb into a ten-limb integer (a term is below 2^288, so 2^32 of them fit), a sixteenth of a field product.  A
// variable that is no small integer takes the field product, which enters the same sum as (z c R) x 1.  At the end the lane's
// integer X = lo + hi 2^256 comes back into the field -- field_mul(lo, 2^256 mod p) + field_mul(hi, 2^512 mod p) = X mod p, which is
// sum(c z) R -- the 64 lanes are added across the wavefront, modular additions, and lane 0 stores: into the row's slot of abc, or
// (check only) into [statement][long row] of the scratch.
struct Wide { uint32_t l[10]; };
// acc += (c R) z for one statement: z its plain value, or the field product through the same sum where it has none
static __device__ __forceinline__ void long_row_term(const R1csfDev &r, Wide &acc, const F8 &c, uint32_t cidx, uint32_t col, size_t sig,
                                                     const uint32_t *__restrict__ wit, const uint32_t *__restrict__ inst,
                                                     const uint32_t *__restrict__ zs)
{
    uint32_t zv = zs[sig * r.zs_stride + cidx];
    F8 term = c;
    if (zv == R1CSF_NOT_SMALL) {
        const F8 z = f8_load(var_ptr(col, r.num_instance, wit + sig * (size_t)r.num_witness * 8, inst + sig * (size_t)r.num_instance * 8));
        field_mul(r.fc, z.l, c.l, term.l);
        zv = 1;
    }
    uint32_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)term.l[k] * zv + acc.l[k] + carry;
        acc.l[k] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
    const uint64_t t = (uint64_t)acc.l[8] + carry;
    acc.l[8] = (uint32_t)t;
    acc.l[9] += (uint32_t)(t >> 32);
}

// the lane's integer back into the field, the 64 lanes added, lane 0 stores
static __device__ __forceinline__ void long_row_finish(const R1csfDev &r, const R1csfLongRow &d, const Wide &acc, size_t sig, size_t batch,
                                                       const uint32_t *__restrict__ inst, uint32_t *__restrict__ abc, uint32_t *__restrict__ long_out)
{
    const uint32_t lo[8] = {acc.l[0], acc.l[1], acc.l[2], acc.l[3], acc.l[4], acc.l[5], acc.l[6], acc.l[7]};
    const uint32_t hi[8] = {acc.l[8], acc.l[9], 0, 0, 0, 0, 0, 0};
    F8 sum, top;
    field_mul(r.fc, lo, r.fc.one, sum.l);
    field_mul(r.fc, hi, r.r2, top.l);
    field_add(r.fc, sum.l, top.l, sum.l);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        F8 other;
#pragma unroll
        for (int k = 0; k < 8; k++) other.l[k] = (uint32_t)__shfl_xor((int)sum.l[k], off, WAVE);
        field_add(r.fc, sum.l, other.l, sum.l);
    }
    // (a statement that does not lead with one: r1csf_eval_kernel zero-fills its products and reads none)
    if (threadIdx.x == 0 && sig < batch && leads_with_one(r.fc, inst + sig * (size_t)r.num_instance * 8))
        f8_store(abc ? product_slot(abc, sig, r.num_constraints, d.matrix, d.row) : long_out + (sig * r.num_long + blockIdx.x) * 8, sum);
}

__global__ __launch_bounds__(WAVE) void r1csf_long_rows_kernel(R1csfDev r, size_t batch, const uint32_t *__restrict__ wit,
                                                               const uint32_t *__restrict__ inst, const uint32_t *__restrict__ zs,
                                                               uint32_t *__restrict__ abc, uint32_t *__restrict__ long_out)
{
    const R1csfLongRow d = r.long_rows[blockIdx.x];
    const int lane = threadIdx.x;
    const size_t sig0 = (size_t)blockIdx.y * R1CSF_LONG_SIGS;
    Wide acc[R1CSF_LONG_SIGS];
#pragma unroll
    for (int s = 0; s < R1CSF_LONG_SIGS; s++)
#pragma unroll
        for (int k = 0; k < 10; k++) acc[s].l[k] = 0;
    static_assert(R1CSF_LONG_SIGS == 4, "the statements of a group are spelled out below");
    for (uint32_t ch = 0; ch < d.num_chunks; ch++) {
        const size_t chunk = (size_t)d.first_chunk + ch;
        const uint32_t cidx = r.long_cidx[chunk * WAVE + lane], col = r.long_col[chunk * WAVE + lane];
        F8 c;
#pragma unroll
        for (int k = 0; k < 8; k++) c.l[k] = r.long_val[(chunk * 8 + k) * WAVE + lane];
        // (spelled out, not a loop: every accumulator keeps compile-time indices whatever the unroller decides)
        long_row_term(r, acc[0], c, cidx, col, sig0 + 0 < batch ? sig0 + 0 : batch - 1, wit, inst, zs);     // a ragged last group repeats
        long_row_term(r, acc[1], c, cidx, col, sig0 + 1 < batch ? sig0 + 1 : batch - 1, wit, inst, zs);     // the last statement
        long_row_term(r, acc[2], c, cidx, col, sig0 + 2 < batch ? sig0 + 2 : batch - 1, wit, inst, zs);
        long_row_term(r, acc[3], c, cidx, col, sig0 + 3 < batch ? sig0 + 3 : batch - 1, wit, inst, zs);
    }
    long_row_finish(r, d, acc[0], sig0 + 0, batch, inst, abc, long_out);
    long_row_finish(r, d, acc[1], sig0 + 1, batch, inst, abc, long_out);
    long_row_finish(r, d, acc[2], sig0 + 2, batch, inst, abc, long_out);
    long_row_finish(r, d, acc[3], sig0 + 3, batch, inst, abc, long_out);
}

// one short row of one matrix: sum of c z over its terms, canonical
static __device__ __forceinline__ F8 row_dot_field(const FieldConsts &fc, const R1csfMatrixDev &m, uint32_t row, uint32_t num_instance,
                                            const uint32_t *__restrict__ wit, const uint32_t *__restrict__ inst)
{
    F8 acc = f8_zero();
    const uint64_t lo = m.row_ptr[row], hi = m.row_ptr[row + 1];
    for (uint64_t t = lo; t < hi; t++) {
        const uint32_t cc = m.col_class[t], col = cc & 0x3fffffffu, cls = cc >> 30;
        F8 z = f8_load(var_ptr(col, num_instance, wit, inst));
        if (cls == 0u) {
            const F8 c = f8_load(m.val + t * 8);
            F8 prod;
            field_mul(fc, z.l, c.l, prod.l);
            z = prod;
        }
        if (cls == R1CSF_MINUS_ONE) field_sub(fc, acc.l, z.l, acc.l);
        else field_add(fc, acc.l, z.l, acc.l);
    }
    return acc;
}

// A thread per constraint, rows by decreasing length (r.order) so that the 64 rows of a wavefront have similar length.  A matrix
// in which the row is long is read back: from abc (STORE) or from the scratch.  STORE: A z, B z, C z go to abc.
#ifndef FRW_R1CSF_WAVES
#define FRW_R1CSF_WAVES 4
#endif
template <bool STORE>
__global__ __launch_bounds__(BLOCK, FRW_R1CSF_WAVES) void r1csf_eval_kernel(R1csfDev r, size_t batch, const uint32_t *__restrict__ wit_all,
                                                                            const uint32_t *__restrict__ inst_all, uint32_t *__restrict__ num,
                                                                            uint32_t *__restrict__ first, uint32_t *__restrict__ abc,
                                                                            const uint32_t *__restrict__ long_out)
{
    const size_t sig = blockIdx.y;
    if (sig >= batch) return;
    const uint32_t *wit = wit_all + sig * (size_t)r.num_witness * 8, *inst = inst_all + sig * (size_t)r.num_instance * 8;
    if (!leads_with_one(r.fc, inst)) {                             // (the same for every thread of the workgroup)
        if (STORE) {
            const F8 zero = f8_zero();
            for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < r.num_constraints; i += gridDim.x * BLOCK)
#pragma unroll
                for (int m = 0; m < 3; m++) f8_store(product_slot(abc, sig, r.num_constraints, m, i), zero);
        }
        return;
    }
    unsigned bad = 0, lowest = 0xffffffffu;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < r.num_constraints; i += gridDim.x * BLOCK) {
        const uint32_t row = r.order[i], mask = r.long_mask[row];
        F8 v[3];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            if (mask & (1u << m)) {
                v[m] = f8_load(STORE ? product_slot(abc, sig, r.num_constraints, m, row)
                                     : long_out + (sig * r.num_long + r.long_slot[(size_t)m * r.num_constraints + row]) * 8);
            } else {
                v[m] = row_dot_field(r.fc, r.m[m], row, r.num_instance, wit, inst);
                if (STORE) f8_store(product_slot(abc, sig, r.num_constraints, m, row), v[m]);
            }
        }
        F8 ab;
        field_mul(r.fc, v[0].l, v[1].l, ab.l);                     // (Az R)(Bz R) / R = Az Bz R, canonical, against Cz R
        bool eq = true;
#pragma unroll
        for (int k = 0; k < 8; k++) eq &= ab.l[k] == v[2].l[k];
        bad += eq ? 0u : 1u;
        lowest = eq || row > lowest ? lowest : row;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bad += __shfl_xor(bad, off, WAVE);
        const unsigned other = __shfl_xor(lowest, off, WAVE);
        lowest = other < lowest ? other : lowest;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && bad) {
        atomicAdd(&num[sig], bad);
        if (first) atomicMin(&first[sig], lowest);
    }
}

// (declared in frw_r1cs_field.h: frw_qap_field.hip runs the same sequence)
hipError_t launch_r1csf_check(const R1csfDev &r, size_t batch, const uint64_t *witness, const uint64_t *instance, uint32_t *num_unsatisfied,
                              uint32_t *first_unsatisfied, uint64_t *abc, void *scratch, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    if (batch > 32768) return hipErrorInvalidValue;
    const uint32_t *wit = (const uint32_t *)witness, *inst = (const uint32_t *)instance;
    hipLaunchKernelGGL(r1csf_init_kernel, dim3((unsigned)((batch + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, r, batch, inst, num_unsatisfied,
                       first_unsatisfied);
    uint32_t *zs = (uint32_t *)scratch, *long_out = zs + batch * (size_t)r.zs_stride;      // (long_out: check only)
    if (r.num_long) {
        hipLaunchKernelGGL(r1csf_zsmall_kernel, dim3((r.num_long_vars + BLOCK - 1) / BLOCK, (unsigned)batch), dim3(BLOCK), 0, st, r, batch, wit, inst, zs);
        hipLaunchKernelGGL(r1csf_long_rows_kernel, dim3(r.num_long, (unsigned)((batch + R1CSF_LONG_SIGS - 1) / R1CSF_LONG_SIGS)), dim3(WAVE), 0, st,
                           r, batch, wit, inst, zs, (uint32_t *)abc, long_out);
    }
    const unsigned gx = (r.num_constraints + BLOCK - 1) / BLOCK;
    const dim3 egrid(gx > 64 ? 64 : gx, (unsigned)batch);
    if (abc)
        hipLaunchKernelGGL(r1csf_eval_kernel<true>, egrid, dim3(BLOCK), 0, st, r, batch, wit, inst, num_unsatisfied, first_unsatisfied,
                           (uint32_t *)abc, nullptr);
    else
        hipLaunchKernelGGL(r1csf_eval_kernel<false>, egrid, dim3(BLOCK), 0, st, r, batch, wit, inst, num_unsatisfied, first_unsatisfied, nullptr,
                           long_out);
    return hipGetLastError();
}

}  // namespace frw

// ---- the handle ------------------------------------------------------------------------------------------------------------------
// (struct frw_r1csf: frw_r1cs_field.h)
extern "C" void frw_r1csf_free(frw_r1csf *r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    for (void *p : r->allocs) (void)hipFree(p);
    delete r;
}

namespace {
using frw::FieldMatrices;

// the matrices over p onto `device`, in the forms the kernels read
int upload_field_matrices(int device, const frw::FieldDerived &fd, const FieldMatrices &m, frw_r1csf **out)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return FRW_E_HIP;
    frw_r1csf *r = nullptr;
    try {
        r = new frw_r1csf;
        r->device = device;
        r->field = fd;
        r->dev.fc = fd.fc;
        std::copy(fd.r2, fd.r2 + 8, r->dev.r2);
        const size_t C = (size_t)m.num_constraints;
        r->dev.num_instance = (uint32_t)m.num_instance;
        r->dev.num_witness = (uint32_t)m.num_witness;
        r->dev.num_constraints = (uint32_t)C;
        auto upload = [&](const void *src, size_t bytes) -> void * {
            void *d = nullptr;
            if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) throw std::bad_alloc();
            r->allocs.push_back(d);
            if (bytes && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy");
            return d;
        };
        uint64_t p_minus_1[4];
        frw::field_limbs(fd.fc.p, p_minus_1);
        p_minus_1[0] -= 1;                                                    // (p is odd)
        auto row_len = [&](int k, size_t row) { return (size_t)(m.row_ptr[k][row + 1] - m.row_ptr[k][row]); };
        std::vector<frw::R1csfLongRow> lrows;
        std::vector<uint32_t> lcol, lval, lslot(3 * C, 0u);
        std::vector<uint8_t> lmask(C, 0);
        for (int k = 0; k < 3; k++) {
            const size_t nnz = (size_t)m.nnz(k);
            r->nnz[k] = nnz;
            std::vector<uint32_t> cls(nnz), val(8 * nnz);
            for (size_t t = 0; t < nnz; t++) {
                const uint64_t *v = &m.val[k][4 * t];
                const bool plus = v[0] == 1 && !(v[1] | v[2] | v[3]);
                const bool minus = v[0] == p_minus_1[0] && v[1] == p_minus_1[1] && v[2] == p_minus_1[2] && v[3] == p_minus_1[3];
                cls[t] = m.col[k][t] | (plus ? frw::R1CSF_PLUS_ONE << 30 : minus ? frw::R1CSF_MINUS_ONE << 30 : 0u);
                uint32_t mont[8];
                frw::field_from_integer(fd, v, false, mont);
                std::copy(mont, mont + 8, &val[8 * t]);
            }
            for (size_t row = 0; row < C; row++) {
                const size_t n = row_len(k, row);
                if (n < frw::R1CSF_LONG_ROW) continue;
                const uint32_t chunks = (uint32_t)((n + 63) / 64), first = (uint32_t)(lcol.size() / 64);
                lslot[(size_t)k * C + row] = (uint32_t)lrows.size();
                lrows.push_back({(uint32_t)k, (uint32_t)row, first, chunks});
                lmask[row] |= (uint8_t)(1u << k);
                lcol.resize((size_t)(first + chunks) * 64, 0u);
                lval.resize((size_t)(first + chunks) * 8 * 64, 0u);
                for (size_t t = 0; t < n; t++) {
                    const size_t src = (size_t)m.row_ptr[k][row] + t, ch = first + t / 64, lane = t % 64;
                    lcol[ch * 64 + lane] = m.col[k][src];
                    for (int j = 0; j < 8; j++) lval[(ch * 8 + j) * 64 + lane] = val[8 * src + j];
                }
            }
            r->dev.m[k].row_ptr = (const uint64_t *)upload(m.row_ptr[k].data(), (C + 1) * 8);
            r->dev.m[k].col_class = (const uint32_t *)upload(cls.data(), nnz * 4);
            r->dev.m[k].val = (const uint32_t *)upload(val.data(), nnz * 32);
        }
        std::vector<size_t> short_len(C, 0);
        for (size_t row = 0; row < C; row++)
            for (int k = 0; k < 3; k++)
                if (!(lmask[row] & (1u << k))) short_len[row] += row_len(k, row);
        std::vector<uint32_t> order(C);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return short_len[x] > short_len[y]; });
        r->dev.order = (const uint32_t *)upload(order.data(), C * 4);
        r->dev.num_long = (uint32_t)lrows.size();
        r->dev.long_mask = (const uint8_t *)upload(lmask.data(), C);
        r->dev.long_slot = (const uint32_t *)upload(lslot.data(), lslot.size() * 4);
        r->dev.long_rows = (const frw::R1csfLongRow *)upload(lrows.data(), lrows.size() * sizeof(frw::R1csfLongRow));
        // the variables the long rows read (the padding reads column 0), and each term's place in that list
        std::vector<uint32_t> lvars(lcol);
        lvars.push_back(0u);
        std::sort(lvars.begin(), lvars.end());
        lvars.erase(std::unique(lvars.begin(), lvars.end()), lvars.end());
        std::vector<uint32_t> lcidx(lcol.size());
        for (size_t t = 0; t < lcol.size(); t++) lcidx[t] = (uint32_t)(std::lower_bound(lvars.begin(), lvars.end(), lcol[t]) - lvars.begin());
        r->dev.num_long_vars = (uint32_t)lvars.size();
        r->dev.zs_stride = (uint32_t)((lvars.size() + 7) & ~(size_t)7);
        r->dev.long_vars = (const uint32_t *)upload(lvars.data(), lvars.size() * 4);
        r->dev.long_cidx = (const uint32_t *)upload(lcidx.data(), lcidx.size() * 4);
        r->dev.long_col = (const uint32_t *)upload(lcol.data(), lcol.size() * 4);
        r->dev.long_val = (const uint32_t *)upload(lval.data(), lval.size() * 4);
        *out = r;
        return FRW_OK;
    } catch (const std::exception &) {
        frw_r1csf_free(r);
        return FRW_E_OUT_OF_MEMORY;
    }
}

// a Falcon circuit's matrices over the modulus: FRW_OK and *out, or FRW_E_INVALID_ARG with the reason recorded
int falcon_field_matrices(const char *what, int circuit, int logn, const uint64_t modulus[4], frw::FieldDerived *fd, FieldMatrices *out)
{
    if ((logn != 9 && logn != 10) || !frw::known_circuit(circuit) || !modulus) return FRW_E_INVALID_ARG;
    if (!frw::field_derive(modulus, fd)) {
        frw::record_error("%s: the modulus is not odd with 2^160 < p < 2^255", what);
        return FRW_E_INVALID_ARG;
    }
    const std::string refusal = frw::r1csf_lift(frw::r1cs_build_matrices(circuit, logn), *fd, out);
    if (!refusal.empty()) {
        frw::record_error("%s: %s", what, refusal.c_str());
        return FRW_E_INVALID_ARG;
    }
    return FRW_OK;
}
}  // namespace

extern "C" int frw_r1cs_export_field(int circuit, int logn, const uint64_t modulus[4], const char *path, uint64_t *counts)
{
    if (!path) return FRW_E_INVALID_ARG;
    try {
        frw::FieldDerived fd;
        FieldMatrices m;
        const int rc = falcon_field_matrices("frw_r1cs_export_field", circuit, logn, modulus, &fd, &m);
        if (rc != FRW_OK) return rc;
        if (counts) {
            counts[0] = m.num_instance; counts[1] = m.num_witness; counts[2] = m.num_constraints;
            counts[3] = m.nnz(0); counts[4] = m.nnz(1); counts[5] = m.nnz(2);
        }
        return frw::r1csf_write(m, path) ? FRW_OK : FRW_E_INVALID_ARG;
    } catch (const std::exception &) {
        return FRW_E_INVALID_ARG;
    }
}

extern "C" int frw_r1csf_load(int device, int circuit, int logn, const uint64_t modulus[4], frw_r1csf **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    if ((logn != 9 && logn != 10) || !frw::known_circuit(circuit) || !modulus) return FRW_E_INVALID_ARG;
    frw::FieldDerived fd;
    if (!frw::field_derive(modulus, &fd)) {
        frw::record_error("frw_r1csf_load: the modulus is not odd with 2^160 < p < 2^255");
        return FRW_E_INVALID_ARG;
    }
    int ndev = 0;                                                         // (before the seconds the host mirror takes)
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    try {
        FieldMatrices m;
        const int rc = falcon_field_matrices("frw_r1csf_load", circuit, logn, modulus, &fd, &m);
        return rc != FRW_OK ? rc : upload_field_matrices(device, fd, m, out);
    } catch (const std::exception &) {
        return FRW_E_OUT_OF_MEMORY;
    }
}

extern "C" int frw_r1csf_load_csr(int device, const uint64_t modulus[4], const uint64_t counts[6], const uint64_t *const row_ptr[3],
                                  const uint32_t *const col[3], const uint64_t *const val[3], frw_r1csf **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    try {
        frw::FieldDerived fd;
        if (!modulus || !frw::field_derive(modulus, &fd)) {
            frw::record_error("frw_r1csf_load_csr: the modulus is not odd with 2^160 < p < 2^255");
            return FRW_E_INVALID_ARG;
        }
        FieldMatrices m;
        const std::string refusal = frw::r1csf_from_csr(fd, counts, row_ptr, col, val, &m);
        if (!refusal.empty()) {
            frw::record_error("frw_r1csf_load_csr: %s", refusal.c_str());
            return FRW_E_INVALID_ARG;
        }
        return upload_field_matrices(device, fd, m, out);
    } catch (const std::exception &) {
        return FRW_E_OUT_OF_MEMORY;
    }
}

extern "C" int frw_r1csf_load_file(int device, const uint64_t modulus[4], const char *path, frw_r1csf **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    try {
        frw::FieldDerived fd;
        if (!modulus || !frw::field_derive(modulus, &fd)) {
            frw::record_error("frw_r1csf_load_file: the modulus is not odd with 2^160 < p < 2^255");
            return FRW_E_INVALID_ARG;
        }
        FieldMatrices m;
        const std::string refusal = frw::r1csf_from_file(fd, path, &m);
        if (!refusal.empty()) {
            frw::record_error("frw_r1csf_load_file: %s", refusal.c_str());
            return FRW_E_INVALID_ARG;
        }
        return upload_field_matrices(device, fd, m, out);
    } catch (const std::exception &) {
        return FRW_E_OUT_OF_MEMORY;
    }
}

extern "C" int frw_r1csf_info(const frw_r1csf *r, frw_r1csf_info_t *out)
{
    if (!r || !out) return FRW_E_INVALID_ARG;
    frw::field_limbs(r->field.fc.p, out->modulus);
    out->num_instance = r->dev.num_instance;
    out->num_witness = r->dev.num_witness;
    out->num_constraints = r->dev.num_constraints;
    for (int k = 0; k < 3; k++) out->nnz[k] = r->nnz[k];
    out->scratch_bytes_per_statement[0] = frw::r1csf_scratch_bytes(r->dev, 1, false);
    out->scratch_bytes_per_statement[1] = frw::r1csf_scratch_bytes(r->dev, 1, true);
    return FRW_OK;
}

extern "C" size_t frw_r1csf_scratch_bytes(const frw_r1csf *r, size_t batch, int with_products)
{
    if (!r) return 0;
    return frw::r1csf_scratch_bytes(r->dev, std::min<size_t>(batch, 32768), with_products != 0);      // the chunks run one after the other
}

extern "C" int frw_r1csf_check_dev(const frw_r1csf *r, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                                   uint32_t *d_num_unsatisfied, uint32_t *d_first_unsatisfied, uint64_t *d_abc, void *d_scratch,
                                   size_t scratch_bytes, void *stream)
{
    if (batch == 0) return FRW_OK;
    if (!r || !d_instance || !d_num_unsatisfied || (!d_witness && r->dev.num_witness)) return FRW_E_INVALID_ARG;
    const size_t need = frw_r1csf_scratch_bytes(r, batch, d_abc != nullptr);
    if (need && (!d_scratch || scratch_bytes < need || ((uintptr_t)d_scratch & 15))) return FRW_E_INVALID_ARG;
    hipError_t e = hipSetDevice(r->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    const size_t W = r->dev.num_witness, I = r->dev.num_instance, C = r->dev.num_constraints;
    for (size_t lo = 0; lo < batch; lo += 32768) {
        const size_t cnt = std::min<size_t>(32768, batch - lo);
        e = frw::launch_r1csf_check(r->dev, cnt, d_witness + lo * W * 4, d_instance + lo * I * 4, d_num_unsatisfied + lo,
                                    d_first_unsatisfied ? d_first_unsatisfied + lo : nullptr, d_abc ? d_abc + lo * 3 * C * 4 : nullptr,
                                    need ? d_scratch : nullptr, (hipStream_t)stream);
        if (e != hipSuccess) return frw::record_hip_error(e, "frw_r1csf_check_dev");
    }
    return FRW_OK;
}
