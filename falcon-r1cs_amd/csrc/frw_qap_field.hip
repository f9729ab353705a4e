// frw_qap_field.hip -- frw_qapf_*: the R1CS -> QAP witness map over a four-limb field given at run time, on its radix-2 domain
// (frw_qap_field.h: the root, the domain, the pass schedule and the tables; frw_r1cs_field.h: the arithmetic and the front end).
// frw_qap.hip and frw_qap_small.hip are the same map with BLS12-381's modulus compiled in (29-bit limbs: they do not carry over).
//
// ark-groth16's witness_map as written, for every statement whatever its witness:
//     a = A z ++ instance, b = B z, c = C z;   ifft;   coset_fft by the generator;   a o b - c;   x (g^n - 1)^-1;   coset_ifft
// ONE kernel does every pass of every transform (qapf_pass_kernel): a workgroup gathers a tile of 2^T points x 2^c adjacent columns
// into LDS, runs T radix-2 decimation-in-frequency stages there, and on the way out multiplies each element by ONE per-index factor --
// the twist for the next pass, g^k / n, or g^-k / (n (g^n - 1)).  Which positions a tile takes, the tables and the order of the passes
// are frw_qap_field.h's rule (tools/dev/qap_field_schedule_model.py is its exact-integer model).  Up to 2^12 the tile is the array:
// one workgroup per array does all the stages of a transform in LDS.  The first inverse pass reads A z ++ instance ++ 0 on the fly,
// a o b - c is fused into the first pass of the last transform, the scale factors into last passes.
//
// Arithmetic: field_mul / field_add / field_sub on 8 x 32-bit limbs, FieldConsts by value in the kernel argument (p and -p^-1 in
// scalar registers), every value canonical between operations, every table entry canonical (field_mul's right operand).  Register
// arrays are indexed by unrolled loops only: no scratch.
// LDS: limb planes, lds[limb][element] -- a wavefront's 64 lanes read 64 consecutive words of a plane (no bank conflict) where packed
// 32-byte elements would be 2-way (ds_read_b128) to 8-way (ds_read_b32) conflicted.  One radix-2 stage per LDS round trip: a
// butterfly is one field product, some 130 multiply-adds, against 32 LDS words moved, so the stages wait on the multiplier, not on LDS
// (not measured apart; profiles/qap_field_map.txt times the whole map).
//
// One launch sequence on one stream, nothing allocated: the r1csf check with d_abc in the workspace, then 3 m launches -- m passes
// for each of ifft and coset_fft over all 3 x chunk arrays, m for the last transform over the chunk's statements.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_qap_field.h"

namespace frw {

constexpr int QAPF_THREADS = 512;          // eight wavefronts: two 64 KiB tiles a CU are four waves per SIMD
enum { QAPF_SRC_WORK = 0, QAPF_SRC_ROWS = 1, QAPF_SRC_PRODUCT = 2 };

struct QapfPass {
    uint32_t *work;                   // [arrays][n][8]: read (SRC_WORK, SRC_PRODUCT) and written (unless to_h) in place
    const uint32_t *abc, *instance;   // SRC_ROWS: [statements][3][C][8], [statements][I][8]
    uint32_t *h;                      // to_h: [statements][n][8]
    const uint32_t *stage;            // rho^j, j < 2^(T - 1)
    const uint32_t *post;             // the per-index factor, null: none
    uint32_t post_mask;               // its index: (position, or with to_h the index written) & post_mask
    uint32_t num_constraints, num_instance;
    int log_n, T, cols_log;           // the tile: 2^T points x 2^cols_log columns
    int t_shift, u_shift;             // where the point and the column sit in a position
    int f0_shift, f0_width, f1_shift, f1_width;      // the same two fields, the lower first: the tile's number fills the other bits
    int src, to_h, per_statement;     // per_statement: blockIdx.y is a statement (its array a), else an array
    QapfSchedule sched;               // to_h: position -> index
};

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
__device__ __forceinline__ uint32_t insert_zeros(uint32_t x, int shift, int width)
{
    return ((x >> shift) << (shift + width)) | (x & ((1u << shift) - 1u));
}

}  // namespace

// LOG_TILE: the elements of LDS, 2^11 (64 KiB) for the passes over HBM and every array up to that size, 2^12 (128 KiB) for a 2^12 array
template <int LOG_TILE>
__global__ __launch_bounds__(QAPF_THREADS) void qapf_pass_kernel(const FieldConsts fc, const QapfPass p)
{
    constexpr uint32_t PLANE = 1u << LOG_TILE;
    __shared__ uint32_t lds[8 * PLANE];
    const uint32_t elems = 1u << (p.T + p.cols_log), cols_mask = (1u << p.cols_log) - 1u;
    const size_t y = blockIdx.y, arr = p.per_statement ? y * 3 : y;
    const uint32_t base = insert_zeros(insert_zeros(blockIdx.x, p.f0_shift, p.f0_width), p.f1_shift, p.f1_width);
    uint32_t *a = p.work + (arr << p.log_n) * 8;

    for (uint32_t e = threadIdx.x; e < elems; e += QAPF_THREADS) {
        const uint32_t pos = base | ((e >> p.cols_log) << p.t_shift) | ((e & cols_mask) << p.u_shift);
        F8 v = F8{{0, 0, 0, 0, 0, 0, 0, 0}};
        if (p.src == QAPF_SRC_ROWS) {                              // the constraint rows, then (A only) the instance values, then zeros
            const size_t sig = y / 3, which = y % 3;
            if (pos < p.num_constraints) v = f8_load(p.abc + ((sig * 3 + which) * p.num_constraints + pos) * 8);
            else if (which == 0 && pos - p.num_constraints < p.num_instance)
                v = f8_load(p.instance + (sig * p.num_instance + (pos - p.num_constraints)) * 8);
        } else if (p.src == QAPF_SRC_PRODUCT) {                    // (a R)(b R) / R - c R = (a b - c) R
            const F8 va = f8_load(a + (size_t)pos * 8), vb = f8_load(a + (((size_t)1 << p.log_n) + pos) * 8),
                     vc = f8_load(a + (((size_t)2 << p.log_n) + pos) * 8);
            F8 ab;
            field_mul(fc, va.l, vb.l, ab.l);
            field_sub(fc, ab.l, vc.l, v.l);
        } else {
            v = f8_load(a + (size_t)pos * 8);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) lds[k * PLANE + e] = v.l[k];
    }
    __syncthreads();

    // T decimation-in-frequency stages over the point bits of the element number: natural in, bit-reversed out
    for (int s = p.T; s >= 1; s--) {
        const uint32_t half = 1u << (s - 1);
        for (uint32_t j = threadIdx.x; j < elems / 2; j += QAPF_THREADS) {
            const uint32_t u = j & cols_mask, jj = j >> p.cols_log, at = jj & (half - 1u);
            const uint32_t i0 = (((((jj >> (s - 1)) << s) | at)) << p.cols_log) | u, i1 = i0 + (half << p.cols_log);
            F8 x, z, sum, dif;
#pragma unroll
            for (int k = 0; k < 8; k++) { x.l[k] = lds[k * PLANE + i0]; z.l[k] = lds[k * PLANE + i1]; }
            field_add(fc, x.l, z.l, sum.l);
            field_sub(fc, x.l, z.l, dif.l);
            if (at) {                                              // (rho^0 = 1: the lowest stage is all of these)
                const F8 w = f8_load(p.stage + ((size_t)at << (p.T - s)) * 8);
                field_mul(fc, dif.l, w.l, x.l);
                dif = x;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) { lds[k * PLANE + i0] = sum.l[k]; lds[k * PLANE + i1] = dif.l[k]; }
        }
        __syncthreads();
    }

    for (uint32_t e = threadIdx.x; e < elems; e += QAPF_THREADS) {
        const uint32_t t = e >> p.cols_log, u = e & cols_mask;
        const uint32_t from = ((__brev(t) >> (32 - p.T)) << p.cols_log) | u;
        const uint32_t pos = base | (t << p.t_shift) | (u << p.u_shift);
        uint32_t index = pos;
        if (p.to_h) {
            index = 0;
#pragma unroll
            for (int i = 0, sh = 0; i < QAPF_MAX_PASSES; i++) {
                if (i < p.sched.num_passes) {
                    index |= ((pos >> p.sched.S[i]) & ((1u << p.sched.T[i]) - 1u)) << sh;
                    sh += p.sched.T[i];
                }
            }
        }
        F8 v;
#pragma unroll
        for (int k = 0; k < 8; k++) v.l[k] = lds[k * PLANE + from];
        if (p.post) {
            const F8 f = f8_load(p.post + (size_t)(index & p.post_mask) * 8);
            F8 r;
            field_mul(fc, v.l, f.l, r.l);
            v = r;
        }
        f8_store(p.to_h ? p.h + ((y << p.log_n) + index) * 8 : a + (size_t)index * 8, v);
    }
}

}  // namespace frw

// ---- the handle ------------------------------------------------------------------------------------------------------------------
struct frw_qapf {
    const frw_r1csf *r = nullptr;
    frw::FftField field{};
    frw::QapfDomain dom{};
    frw::QapfSchedule sched{};
    int cols_log = 0, log_tile = 11;
    const uint32_t *stage_fwd[frw::QAPF_MAX_PASSES] = {}, *stage_inv[frw::QAPF_MAX_PASSES] = {};
    const uint32_t *twist_fwd[frw::QAPF_MAX_PASSES] = {}, *twist_inv[frw::QAPF_MAX_PASSES] = {};       // [i]: twist i, i < m - 1
    const uint32_t *scale_in = nullptr, *scale_out = nullptr;
    size_t zs_stride = 0, per_statement = 0;
    std::vector<void *> allocs;
};

extern "C" void frw_qapf_free(frw_qapf *q)
{
    if (!q) return;
    (void)hipSetDevice(q->r->device);
    for (void *p : q->allocs) (void)hipFree(p);
    delete q;
}

namespace {
using namespace frw;

void canonical_limbs(const FieldDerived &d, const uint32_t (&mont)[8], uint64_t out[4])
{
    field_to_canonical(d, mont, out);
}

void fill_domain(const FftField &f, const QapfDomain &dom, frw_qapf_domain_t *out)
{
    out->log_size = dom.log_size;
    out->reserved = 0;
    out->size = (uint64_t)1 << dom.log_size;
    canonical_limbs(f.fd, dom.group_gen, out->group_gen);
    canonical_limbs(f.fd, dom.group_gen_inv, out->group_gen_inv);
    canonical_limbs(f.fd, dom.size_inv, out->size_inv);
    canonical_limbs(f.fd, dom.generator_inv, out->generator_inv);
    canonical_limbs(f.fd, dom.vanishing_inv, out->vanishing_inv);
}

// one pass of one transform over `arrays` arrays (per_statement: statements), everything else from the handle
hipError_t launch_pass(const frw_qapf *q, int i, bool inverse_root, const uint32_t *post, uint32_t post_mask, int src, bool to_h, bool per_statement,
                       QapfBufs &b, const uint32_t *instance, uint32_t *h, size_t cnt, hipStream_t st)
{
    const QapfSchedule &s = q->sched;
    QapfPass p{};
    p.work = b.work;
    p.abc = b.abc;
    p.instance = instance;
    p.h = h;
    p.stage = inverse_root ? q->stage_inv[i] : q->stage_fwd[i];
    p.post = post;
    p.post_mask = post_mask;
    p.num_constraints = q->r->dev.num_constraints;
    p.num_instance = q->r->dev.num_instance;
    p.log_n = s.log_n;
    p.T = s.T[i];
    p.cols_log = q->cols_log;
    if (s.num_passes == 1) { p.t_shift = 0; p.u_shift = s.log_n; }
    else if (s.S[i] == 0) { p.t_shift = 0; p.u_shift = to_h ? s.S[0] : s.T[i]; }       // the map's last pass: columns that are adjacent in h
    else { p.t_shift = s.S[i]; p.u_shift = 0; }
    const bool t_first = p.t_shift < p.u_shift;
    p.f0_shift = t_first ? p.t_shift : p.u_shift; p.f0_width = t_first ? p.T : p.cols_log;
    p.f1_shift = t_first ? p.u_shift : p.t_shift; p.f1_width = t_first ? p.cols_log : p.T;
    p.src = src;
    p.to_h = to_h ? 1 : 0;
    p.per_statement = per_statement ? 1 : 0;
    p.sched = s;
    const dim3 grid(1u << (s.log_n - p.T - p.cols_log), (unsigned)(p.per_statement ? cnt : 3 * cnt));
    if (q->log_tile == 12) hipLaunchKernelGGL(qapf_pass_kernel<12>, grid, dim3(QAPF_THREADS), 0, st, q->field.fd.fc, p);
    else hipLaunchKernelGGL(qapf_pass_kernel<11>, grid, dim3(QAPF_THREADS), 0, st, q->field.fd.fc, p);
    return hipGetLastError();
}

}  // namespace

extern "C" int frw_fft_field_info(const uint64_t modulus[4], const uint64_t generator[4], frw_fft_field_info_t *out)
{
    if (!modulus || !generator || !out) return FRW_E_INVALID_ARG;
    FftField f;
    const std::string refusal = fft_field_derive(modulus, generator, &f);
    if (!refusal.empty()) {
        record_error("frw_fft_field_info: %s", refusal.c_str());
        return FRW_E_INVALID_ARG;
    }
    for (int j = 0; j < 4; j++) { out->modulus[j] = modulus[j]; out->generator[j] = generator[j]; }
    out->two_adicity = f.two_adicity;
    out->reserved = 0;
    canonical_limbs(f.fd, f.root, out->two_adic_root);
    field_limbs(f.root, out->two_adic_root_mont);
    return FRW_OK;
}

extern "C" int frw_qapf_domain(const uint64_t modulus[4], const uint64_t generator[4], uint64_t num_constraints, uint64_t num_instance,
                               frw_qapf_domain_t *out)
{
    if (!modulus || !generator || !out) return FRW_E_INVALID_ARG;
    FftField f;
    QapfDomain dom;
    std::string refusal = fft_field_derive(modulus, generator, &f);
    if (refusal.empty()) refusal = qapf_domain_derive(f, num_constraints, num_instance, &dom);
    if (!refusal.empty()) {
        record_error("frw_qapf_domain: %s", refusal.c_str());
        return FRW_E_INVALID_ARG;
    }
    fill_domain(f, dom, out);
    return FRW_OK;
}

extern "C" int frw_qapf_create(const frw_r1csf *r, const uint64_t generator[4], frw_qapf **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    if (!r || !generator) return FRW_E_INVALID_ARG;
    frw_qapf *q = nullptr;
    try {
        q = new frw_qapf;
        q->r = r;
        uint64_t modulus[4];
        field_limbs(r->field.fc.p, modulus);
        std::string refusal = fft_field_derive(modulus, generator, &q->field);
        if (refusal.empty()) refusal = qapf_domain_derive(q->field, r->dev.num_constraints, r->dev.num_instance, &q->dom);
        if (refusal.empty() && q->dom.log_size == 0) refusal = "a domain of one point has no transform";
        if (!refusal.empty()) {
            record_error("frw_qapf_create: %s", refusal.c_str());
            delete q;
            return FRW_E_INVALID_ARG;
        }
        const int L = (int)q->dom.log_size;
        const QapfSchedule s = q->sched = qapf_schedule(L);
        q->cols_log = s.num_passes == 1 ? 0 : QAPF_COLS_LOG;
        q->log_tile = L == QAPF_LDS_LOG_N ? 12 : 11;
        q->zs_stride = r->dev.num_long ? r->dev.zs_stride : 0;
        q->per_statement = qapf_layout(nullptr, 1, r->dev.num_constraints, L, q->zs_stride).bytes;
        hipError_t e = hipSetDevice(r->device);
        if (e != hipSuccess) { delete q; return record_hip_error(e, "hipSetDevice"); }
        std::vector<uint32_t> host;
        auto upload = [&](size_t elems) -> const uint32_t * {
            void *d = nullptr;
            if (hipMalloc(&d, elems * 32) != hipSuccess) throw std::bad_alloc();
            q->allocs.push_back(d);
            if (hipMemcpy(d, host.data(), elems * 32, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy");
            return (const uint32_t *)d;
        };
        const FieldDerived &fd = q->field.fd;
        for (int i = 0; i < s.num_passes; i++) {
            host.assign(qapf_stage_elems(s, i) * 8, 0u);
            qapf_build_stage(fd, q->dom.group_gen, s, i, host.data());
            q->stage_fwd[i] = upload(qapf_stage_elems(s, i));
            qapf_build_stage(fd, q->dom.group_gen_inv, s, i, host.data());
            q->stage_inv[i] = upload(qapf_stage_elems(s, i));
            if (i == s.num_passes - 1) break;
            host.assign(qapf_twist_elems(s, i) * 8, 0u);
            qapf_build_twist(fd, q->dom.group_gen, s, i, host.data());
            q->twist_fwd[i] = upload(qapf_twist_elems(s, i));
            qapf_build_twist(fd, q->dom.group_gen_inv, s, i, host.data());
            q->twist_inv[i] = upload(qapf_twist_elems(s, i));
        }
        host.assign((size_t)8 << L, 0u);
        qapf_build_scale_in(q->field, q->dom, s, host.data());
        q->scale_in = upload((size_t)1 << L);
        qapf_build_scale_out(q->field, q->dom, s, host.data());
        q->scale_out = upload((size_t)1 << L);
        *out = q;
        return FRW_OK;
    } catch (const std::exception &) {
        if (q) frw_qapf_free(q);
        return FRW_E_OUT_OF_MEMORY;
    }
}

extern "C" int frw_qapf_info(const frw_qapf *q, frw_qapf_info_t *out)
{
    if (!q || !out) return FRW_E_INVALID_ARG;
    fill_domain(q->field, q->dom, &out->domain);
    out->num_constraints = q->r->dev.num_constraints;
    out->num_instance = q->r->dev.num_instance;
    out->num_passes = (uint32_t)q->sched.num_passes;
    out->reserved = 0;
    out->workspace_bytes_per_statement = q->per_statement;
    return FRW_OK;
}

extern "C" int frw_qapf_witness_map_dev(const frw_qapf *q, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance, uint64_t *d_h,
                                        uint32_t *d_num_unsatisfied, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (batch == 0) return FRW_OK;
    if (!q || !d_instance || !d_h || !d_workspace || (!d_witness && q->r->dev.num_witness)) return FRW_E_INVALID_ARG;
    if (workspace_bytes < q->per_statement || ((uintptr_t)d_workspace & 15)) return FRW_E_INVALID_ARG;
    const frw_r1csf *r = q->r;
    hipError_t e = hipSetDevice(r->device);
    if (e != hipSuccess) return record_hip_error(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const QapfSchedule &s = q->sched;
    const int m = s.num_passes, L = s.log_n;
    const size_t W = r->dev.num_witness, I = r->dev.num_instance, C = r->dev.num_constraints, n = (size_t)1 << L;
    const uint32_t all = (uint32_t)(n - 1);
    const size_t chunk = std::min<size_t>(workspace_bytes / q->per_statement, 16384);       // (3 chunk arrays are a grid's y)
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = std::min(chunk, batch - lo);
        QapfBufs b = qapf_layout(d_workspace, cnt, C, L, q->zs_stride);
        const uint64_t *inst = d_instance + lo * I * 4;
        e = launch_r1csf_check(r->dev, cnt, d_witness + lo * W * 4, inst, d_num_unsatisfied ? d_num_unsatisfied + lo : b.num, nullptr,
                               (uint64_t *)b.abc, b.zsmall, st);
        // ifft, x g^k / n: F(w^-1), the rows read on the fly, digit-reversed out
        for (int i = 0; i < m && e == hipSuccess; i++)
            e = launch_pass(q, i, true, i < m - 1 ? q->twist_inv[i] : q->scale_in, i < m - 1 ? (uint32_t)(qapf_twist_elems(s, i) - 1) : all,
                            i == 0 ? QAPF_SRC_ROWS : QAPF_SRC_WORK, false, false, b, (const uint32_t *)inst, nullptr, cnt, st);
        // fft: G(w), natural out
        for (int i = m - 1; i >= 0 && e == hipSuccess; i--)
            e = launch_pass(q, i, false, i > 0 ? q->twist_fwd[i - 1] : nullptr, i > 0 ? (uint32_t)(qapf_twist_elems(s, i - 1) - 1) : 0u, QAPF_SRC_WORK,
                            false, false, b, nullptr, nullptr, cnt, st);
        // a o b - c, ifft, x g^-k / (n (g^n - 1)) -> h: F(w^-1), the last pass writing index k to h[k]
        for (int i = 0; i < m && e == hipSuccess; i++)
            e = launch_pass(q, i, true, i < m - 1 ? q->twist_inv[i] : q->scale_out, i < m - 1 ? (uint32_t)(qapf_twist_elems(s, i) - 1) : all,
                            i == 0 ? QAPF_SRC_PRODUCT : QAPF_SRC_WORK, i == m - 1, true, b, nullptr, (uint32_t *)(d_h + lo * n * 4), cnt, st);
        if (e != hipSuccess) return record_hip_error(e, "frw_qapf_witness_map_dev");
    }
    return FRW_OK;
}
