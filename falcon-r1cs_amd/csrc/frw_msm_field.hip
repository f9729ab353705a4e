// frw_msm_field.hip -- frw_curve_* and frw_msmf_*: sum_i k_i P_i on a curve y^2 = x^3 + b over a four-limb field given at run time
// (frw_curve.h: the descriptor, the points, the complete group law; frw_r1cs_field.h: the coordinates' arithmetic, 32-bit CIOS with the
// modulus in scalar registers).  frw_msm.hip is the same sum with BLS12-381 compiled in; its 29-bit limbs do not carry over.
//
// The handle holds the n bases as they came, 64 bytes a point, and NO window tables (the "bare handle" path of DESIGN 5.8): the
// windows cost no memory and their sums are joined by Horner's rule.  The schedule is a rule:
//     windows       C x W = 13 x 20 below 2^16 points, 15 x 18 from there on -- both cover 257 bits, so a plain 256-bit integer keeps
//                   its last carry (signed_digits of frw_digits.h, unchanged); keys = W 2^(C - 1) (window, bucket) pairs a statement
//     0 clear       the keys' counts to zero (a kernel: the call is a chain of kernel nodes when captured)
//     1 digits      a thread per scalar: Montgomery -> integer (one field_mul by 1 over r), W signed digits stored as int16, the
//                   keys' histogram by global atomics.  A zero digit leaves no entry.
//     2 scan        a workgroup per statement: exclusive prefix sums of the keys' counts
//     3 scatter     a thread per scalar: its entries (point index, sign on top) to their keys' runs -- ONE counting sort a statement
//     4 buckets     a lane per key: its entries' points, gathered by index, added into an XYZZ accumulator in registers (mixed
//                   additions, 10 products each)
//     5 fold        per window sum_b (b + 1) B_b: levels of 8 -- a lane turns 8 (weighted, plain) pairs into one by running sums,
//                   the block's weight by doublings; 4 launches for 2^12 buckets, 5 for 2^14
//     6 finish      a lane per statement: Horner over the windows (C doublings each), one Fermat inversion, the affine point out
// The order in which atomics place a key's entries differs from run to run; the sum of a bucket does not (the group law is complete,
// whatever order brings equal or opposite points together), and the result is the unique affine point.  A bucket far above the mean
// (all scalars equal) is one lane's chain: correct, and as slow as its length -- it is not split here.
// Everything on the caller's stream, nothing allocated, no synchronisation, no host branch on device data: the call may be captured.
// No kernel of this unit has scratch (tools/kernel_resources.py holds them to it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <new>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_curve.h"
#include "frw_digits.h"
#include "frw_layout.h"

namespace frw {

constexpr uint32_t MSMF_MAX_POINTS = 1u << 22;
constexpr uint32_t MSMF_WIDE_FROM = 1u << 16;      // points from which the windows are 15 bits
constexpr size_t MSMF_MAX_CHUNK = 32768;           // statements of one launch sequence (a grid's y)

namespace {

__device__ __forceinline__ Xyzz xyzz_load(const uint32_t *__restrict__ w)
{
    const Affine a = affine_load(w), b = affine_load(w + 16);
    return Xyzz{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void fe_store(uint32_t *w, const Fe &a)
{
    ((uint4 *)w)[0] = make_uint4(a.l[0], a.l[1], a.l[2], a.l[3]);
    ((uint4 *)w)[1] = make_uint4(a.l[4], a.l[5], a.l[6], a.l[7]);
}
__device__ __forceinline__ void xyzz_store(uint32_t *w, const Xyzz &p)
{
    fe_store(w, p.x); fe_store(w + 8, p.y); fe_store(w + 16, p.zz); fe_store(w + 24, p.zzz);
}

}  // namespace

// the first base that is not on the curve (0xffffffff: none)
__global__ __launch_bounds__(256) void msmf_check_kernel(const CurveConsts cc, uint32_t n, const uint32_t *__restrict__ bases, uint32_t *__restrict__ first_bad)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!curve_on_curve(cc, affine_load(bases + (size_t)i * 16))) atomicMin(first_bad, i);
}

// 0: the keys' counts to zero.  A kernel, not hipMemsetAsync: captured into a graph the call is then a plain chain of kernel nodes, as
// every other call over a run-time field is.
__global__ __launch_bounds__(256) void msmf_clear_kernel(uint4 *__restrict__ words, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) words[i] = make_uint4(0, 0, 0, 0);
}

// 1: the digits of scalar i of statement y, and the histogram of its keys
template <int C, int W>
__global__ __launch_bounds__(256) void msmf_digits_kernel(const FieldConsts fr, uint32_t n, uint32_t num_scalars, const uint32_t *__restrict__ scalars,
                                                          size_t stride_words, int montgomery, int16_t *__restrict__ digits /* [y][W][n] */,
                                                          uint32_t *__restrict__ counts /* [y][W][2^(C-1)] */)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const size_t y = blockIdx.y;
    if (i >= num_scalars) return;
    Fr8 k = fr_load(scalars + y * stride_words + (size_t)i * 8);
    if (montgomery) {                                              // h 2^256 mod r -> h: REDC, a product with the integer 1
        const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        Fr8 h;
        field_mul(fr, k.l, one, h.l);
        k = h;
    }
    int d[W];
    signed_digits<C, W>(k, d);
#pragma unroll
    for (int j = 0; j < W; j++) {
        digits[(y * W + j) * n + i] = (int16_t)d[j];
        if (d[j]) atomicAdd(&counts[(y * W + j) * (size_t)(1 << (C - 1)) + digit_bucket(d[j])], 1u);
    }
}

// 2: where each key's entries start, and the scatter's cursor there
__global__ __launch_bounds__(1024) void msmf_scan_kernel(uint32_t keys, const uint32_t *__restrict__ counts, uint32_t *__restrict__ offsets, uint32_t *__restrict__ cursor)
{
    __shared__ uint32_t part[1024];
    const size_t y = blockIdx.x;
    const uint32_t t = threadIdx.x, per = keys / 1024;             // keys: a multiple of 4096
    const uint32_t *cnt = counts + y * keys + (size_t)t * per;
    uint32_t s = 0;
    for (uint32_t k = 0; k < per; k++) s += cnt[k];
    part[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t k = 0; k < per; k++) {
        const size_t at = y * keys + (size_t)t * per + k;
        offsets[at] = run;
        cursor[at] = run;
        run += cnt[k];
    }
}

// 3: the entries to their keys' runs
__global__ __launch_bounds__(256) void msmf_scatter_kernel(uint32_t n, uint32_t num_scalars, int windows, uint32_t buckets, const int16_t *__restrict__ digits,
                                                           uint32_t *__restrict__ cursor, uint32_t *__restrict__ entries /* [y][windows n] */)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const size_t y = blockIdx.y;
    if (i >= num_scalars) return;
    uint32_t *ent = entries + y * windows * n;
    for (int j = 0; j < windows; j++) {
        const int v = digits[(y * windows + j) * n + i];
        if (!v) continue;
        const uint32_t at = atomicAdd(&cursor[(y * windows + j) * buckets + digit_bucket(v)], 1u);
        if (at < (uint32_t)windows * n) ent[at] = digit_entry(i, v);      // (always, with counts that are this call's: no address hangs on it)
    }
}

// 4: a lane per key.  The accumulator (32 words), the point (16) and a mixed addition's temporaries stay in registers.
__global__ __launch_bounds__(256, 4) void msmf_bucket_kernel(const FieldConsts fq, uint32_t n, uint32_t keys, size_t entries_per_statement,
                                                             const uint32_t *__restrict__ bases, const uint32_t *__restrict__ offsets,
                                                             const uint32_t *__restrict__ counts, const uint32_t *__restrict__ entries,
                                                             uint32_t *__restrict__ buckets)
{
    const size_t y = blockIdx.y;
    const uint32_t key = blockIdx.x * 256 + threadIdx.x;           // keys: a multiple of 256
    const size_t at = y * keys + key;
    // (first <= entries_per_statement and first + cnt <= it with counts that are this call's; held to it here, and an index to n below, so
    // that no address of this kernel hangs on what another kernel wrote)
    const size_t off = offsets[at], first = off < entries_per_statement ? off : entries_per_statement, room = entries_per_statement - first;
    const uint32_t cnt = counts[at] < room ? counts[at] : (uint32_t)room;
    const uint32_t *ent = entries + y * entries_per_statement + first;
    Xyzz acc = xyzz_identity();
    for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t e = ent[j];
        if ((e & 0x7fffffffu) >= n) continue;
        Affine p = affine_load(bases + (size_t)(e & 0x7fffffffu) * 16);
        if (e >> 31) p.y = fe_neg(fq, p.y);
        acc = xyzz_add_affine(fq, acc, p);
    }
    xyzz_store(buckets + at * MSMF_XYZZ_WORDS, acc);
}

// 5: one level of the fold.  The items of a window are `count` (weighted, plain) pairs, each a block of 2^log_weight buckets -- at the first
// level the buckets themselves, both halves the bucket.  Lane g of a window joins items g K .. g K + K - 1:
//     plain' = sum T_i,    weighted' = sum S_i + 2^log_weight sum i T_i      (running sums from the top: sum i T_i = sum of the runs)
__global__ __launch_bounds__(64, 1) void msmf_fold_kernel(const FieldConsts fq, uint32_t lanes /* a statement's: windows count / K */, int log_k, int log_weight,
                                                          int first, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    const size_t y = blockIdx.y;
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t K = 1u << log_k;
    const size_t item_words = first ? MSMF_XYZZ_WORDS : 2 * MSMF_XYZZ_WORDS;
    const uint32_t *src = in + (y * ((size_t)lanes << log_k) + ((size_t)g << log_k)) * item_words;
    Xyzz run = xyzz_identity(), acc = xyzz_identity(), weighted = xyzz_identity();
    for (uint32_t i = K; i-- > 0;) {
        if (!first) weighted = xyzz_add(fq, weighted, xyzz_load(src + i * item_words));
        run = xyzz_add(fq, run, xyzz_load(src + i * item_words + (first ? 0 : MSMF_XYZZ_WORDS)));
        if (i) acc = xyzz_add(fq, acc, run);
    }
    for (int k = 0; k < log_weight; k++) acc = xyzz_double(fq, acc);
    weighted = xyzz_add(fq, first ? run : weighted, acc);
    uint32_t *dst = out + (y * lanes + g) * (size_t)(2 * MSMF_XYZZ_WORDS);
    xyzz_store(dst, weighted);
    xyzz_store(dst + MSMF_XYZZ_WORDS, run);
}

// 6: Horner over a statement's window sums, the affine point out
__global__ __launch_bounds__(64, 1) void msmf_finish_kernel(const FieldConsts fq, uint32_t statements, int windows, int window_bits,
                                                            const uint32_t *__restrict__ sums /* [y][windows][2][32] */, uint32_t *__restrict__ out /* [y][16] */)
{
    const uint32_t y = blockIdx.x * 64 + threadIdx.x;
    if (y >= statements) return;
    const uint32_t *src = sums + (size_t)y * windows * (2 * MSMF_XYZZ_WORDS);
    Xyzz acc = xyzz_load(src + (size_t)(windows - 1) * (2 * MSMF_XYZZ_WORDS));
    for (int j = windows - 2; j >= 0; j--) {
        for (int k = 0; k < window_bits; k++) acc = xyzz_double(fq, acc);
        acc = xyzz_add(fq, acc, xyzz_load(src + (size_t)j * (2 * MSMF_XYZZ_WORDS)));
    }
    const Affine a = xyzz_to_affine(fq, acc);
    fe_store(out + (size_t)y * 16, a.x);
    fe_store(out + (size_t)y * 16 + 8, a.y);
}

}  // namespace frw

// ---- the handle ------------------------------------------------------------------------------------------------------------------
struct frw_msmf {
    int device = 0;
    frw::CurveDerived curve{};
    uint32_t n = 0;
    int window_bits = 0, windows = 0;
    uint32_t *bases = nullptr;
    size_t per_statement = 0;
};

namespace {
using namespace frw;

int derive_curve(const char *who, const frw_curve_t *c, CurveDerived *out)
{
    if (!c) { record_error("%s: null pointer", who); return FRW_E_INVALID_ARG; }
    const char *refusal = curve_derive(c->base_modulus, c->scalar_modulus, c->b, out);
    if (refusal[0]) { record_error("%s: %s", who, refusal); return FRW_E_INVALID_ARG; }
    return FRW_OK;
}

}  // namespace

extern "C" int frw_curve_info(const frw_curve_t *c, frw_curve_info_t *out)
{
    CurveDerived d;
    if (!out) { record_error("frw_curve_info: null pointer"); return FRW_E_INVALID_ARG; }
    const int rc = derive_curve("frw_curve_info", c, &d);
    if (rc != FRW_OK) return rc;
    out->base_bits = d.q.bits;
    out->scalar_bits = d.r.bits;
    field_limbs(d.cc.b, out->b_mont);
    field_limbs(d.q.fc.one, out->one_mont);
    field_limbs(d.r.fc.one, out->scalar_one_mont);
    return FRW_OK;
}

extern "C" int frw_curve_check_points(const frw_curve_t *c, size_t count, const uint64_t *points, int64_t *first_bad)
{
    CurveDerived d;
    if (!first_bad || (!points && count)) { record_error("frw_curve_check_points: null pointer"); return FRW_E_INVALID_ARG; }
    const int rc = derive_curve("frw_curve_check_points", c, &d);
    if (rc != FRW_OK) return rc;
    *first_bad = -1;
    for (size_t i = 0; i < count; i++)
        if (!curve_on_curve(d.cc, affine_from_limbs(points + 8 * i))) { *first_bad = (int64_t)i; break; }
    return FRW_OK;
}

extern "C" int frw_curve_scalar_mul(const frw_curve_t *c, size_t count, const uint64_t *points, const uint64_t *scalars, uint64_t *out)
{
    CurveDerived d;
    if (count && (!points || !scalars || !out)) { record_error("frw_curve_scalar_mul: null pointer"); return FRW_E_INVALID_ARG; }
    const int rc = derive_curve("frw_curve_scalar_mul", c, &d);
    if (rc != FRW_OK) return rc;
    for (size_t i = 0; i < count; i++) {
        const Affine p = affine_from_limbs(points + 8 * i);
        if (!curve_on_curve(d.cc, p)) {
            record_error("frw_curve_scalar_mul: point %zu is not on the curve", i);
            return FRW_E_INVALID_ARG;
        }
        affine_to_limbs(curve_scalar_mul(d.cc, p, scalars + 4 * i), out + 8 * i);
    }
    return FRW_OK;
}

extern "C" void frw_msmf_free(frw_msmf *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->bases) (void)hipFree(m->bases);
    delete m;
}

extern "C" int frw_msmf_load(int device, const frw_curve_t *c, size_t num_points, const uint64_t *bases, int flags, frw_msmf **out)
{
    if (!out) { record_error("frw_msmf_load: null pointer"); return FRW_E_INVALID_ARG; }
    *out = nullptr;
    if (!bases) { record_error("frw_msmf_load: null pointer"); return FRW_E_INVALID_ARG; }
    CurveDerived d;
    const int rc = derive_curve("frw_msmf_load", c, &d);
    if (rc != FRW_OK) return rc;
    if (num_points == 0 || num_points > MSMF_MAX_POINTS) {
        record_error("frw_msmf_load: %zu points (1 .. 2^22)", num_points);
        return FRW_E_INVALID_ARG;
    }
    if (flags & ~FRW_MSMF_POINTS_ARE_CHECKED) { record_error("frw_msmf_load: unknown flags"); return FRW_E_INVALID_ARG; }
    frw_msmf *m = new (std::nothrow) frw_msmf;
    if (!m) return FRW_E_OUT_OF_MEMORY;
    m->device = device;
    m->curve = d;
    m->n = (uint32_t)num_points;
    const bool wide = m->n >= MSMF_WIDE_FROM;
    m->window_bits = wide ? 15 : 13;
    m->windows = wide ? 18 : 20;
    m->per_statement = msmf_layout(nullptr, 1, m->n, m->window_bits, m->windows).bytes;
    hipError_t e = hipSetDevice(device);
    uint32_t *d_bad = nullptr;
    if (e == hipSuccess) e = hipMalloc((void **)&m->bases, num_points * 64);
    if (e == hipSuccess) e = hipMemcpy(m->bases, bases, num_points * 64, hipMemcpyHostToDevice);
    uint32_t bad = 0xffffffffu;
    if (e == hipSuccess && !(flags & FRW_MSMF_POINTS_ARE_CHECKED)) {
        e = hipMalloc((void **)&d_bad, 4);
        if (e == hipSuccess) e = hipMemcpy(d_bad, &bad, 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(msmf_check_kernel, dim3((m->n + 255) / 256), dim3(256), 0, 0, d.cc, m->n, (const uint32_t *)m->bases, d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
        if (d_bad) (void)hipFree(d_bad);
    }
    if (e != hipSuccess) { frw_msmf_free(m); return record_hip_error(e, "frw_msmf_load"); }
    if (bad != 0xffffffffu) {
        frw_msmf_free(m);
        record_error("frw_msmf_load: base %u is not on the curve", bad);
        return FRW_E_INVALID_ARG;
    }
    *out = m;
    return FRW_OK;
}

extern "C" int frw_msmf_info(const frw_msmf *m, frw_msmf_info_t *out)
{
    if (!m || !out) { record_error("frw_msmf_info: null pointer"); return FRW_E_INVALID_ARG; }
    out->num_points = m->n;
    out->window_bits = (uint32_t)m->window_bits;
    out->num_windows = (uint32_t)m->windows;
    out->reserved = 0;
    out->bases_bytes = (uint64_t)m->n * 64;
    out->workspace_bytes_per_statement = m->per_statement;
    return FRW_OK;
}

extern "C" size_t frw_msmf_workspace_bytes(const frw_msmf *m, size_t batch_in_flight)
{
    if (!m || batch_in_flight == 0) return 0;
    return msmf_layout(nullptr, batch_in_flight, m->n, m->window_bits, m->windows).bytes;
}

extern "C" int frw_msmf_dev(const frw_msmf *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, size_t num_scalars, int montgomery,
                            uint64_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!m) { record_error("frw_msmf_dev: null pointer"); return FRW_E_INVALID_ARG; }
    if (num_scalars > m->n) { record_error("frw_msmf_dev: %zu scalars for %u points", num_scalars, m->n); return FRW_E_INVALID_ARG; }
    if (scalar_stride < num_scalars) { record_error("frw_msmf_dev: a stride of %zu for %zu scalars", scalar_stride, num_scalars); return FRW_E_INVALID_ARG; }
    if (batch == 0) return FRW_OK;
    if (!d_out || !d_workspace || (!d_scalars && num_scalars)) { record_error("frw_msmf_dev: null pointer"); return FRW_E_INVALID_ARG; }
    if (((uintptr_t)d_workspace & 15) || ((uintptr_t)d_scalars & 15) || ((uintptr_t)d_out & 15)) {
        record_error("frw_msmf_dev: a buffer is not 16-byte aligned");
        return FRW_E_INVALID_ARG;
    }
    if (workspace_bytes < m->per_statement) {
        record_error("frw_msmf_dev: a workspace of %zu bytes, a statement takes %zu", workspace_bytes, m->per_statement);
        return FRW_E_INVALID_ARG;
    }
    hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) return record_hip_error(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const int C = m->window_bits, W = m->windows;
    const uint32_t n = m->n, buckets = 1u << (C - 1), keys = (uint32_t)W * buckets, ns = (uint32_t)num_scalars;
    const FieldConsts &fq = m->curve.cc.fq;
    const size_t chunk = proofs_in_flight(std::min(batch, MSMF_MAX_CHUNK), workspace_bytes,
                                          [&](size_t k) { return msmf_layout(nullptr, k, n, C, W).bytes; });
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = std::min(chunk, batch - lo);
        const MsmfBufs b = msmf_layout(d_workspace, cnt, n, C, W);
        const uint32_t *scalars = (const uint32_t *)(d_scalars + lo * scalar_stride * 4);
        const size_t count16 = cnt * keys / 4;                         // keys: a multiple of four
        hipLaunchKernelGGL(msmf_clear_kernel, dim3((unsigned)std::min<size_t>((count16 + 255) / 256, 4096)), dim3(256), 0, st, (uint4 *)b.counts, count16);
        if (ns) {
            const dim3 grid((ns + 255) / 256, (unsigned)cnt);
            if (C == 15)
                hipLaunchKernelGGL((msmf_digits_kernel<15, 18>), grid, dim3(256), 0, st, m->curve.r.fc, n, ns, scalars, scalar_stride * 8, montgomery, b.digits, b.counts);
            else
                hipLaunchKernelGGL((msmf_digits_kernel<13, 20>), grid, dim3(256), 0, st, m->curve.r.fc, n, ns, scalars, scalar_stride * 8, montgomery, b.digits, b.counts);
        }
        hipLaunchKernelGGL(msmf_scan_kernel, dim3((unsigned)cnt), dim3(1024), 0, st, keys, (const uint32_t *)b.counts, b.offsets, b.cursor);
        if (ns)
            hipLaunchKernelGGL(msmf_scatter_kernel, dim3((ns + 255) / 256, (unsigned)cnt), dim3(256), 0, st, n, ns, W, buckets, (const int16_t *)b.digits, b.cursor, b.entries);
        hipLaunchKernelGGL(msmf_bucket_kernel, dim3(keys / 256, (unsigned)cnt), dim3(256), 0, st, fq, n, keys, (size_t)W * n, (const uint32_t *)m->bases,
                           (const uint32_t *)b.offsets, (const uint32_t *)b.counts, (const uint32_t *)b.entries, b.buckets);
        const uint32_t *in = b.buckets;
        int level = 0;
        for (uint32_t count = buckets, log_weight = 0; count > 1; level++) {
            const int log_k = count >= (uint32_t)MSMF_FOLD ? MSMF_FOLD_LOG : (count == 4 ? 2 : 1);
            const uint32_t lanes = (uint32_t)W * (count >> log_k);
            uint32_t *dst = b.fold[level & 1];
            hipLaunchKernelGGL(msmf_fold_kernel, dim3((lanes + 63) / 64, (unsigned)cnt), dim3(64), 0, st, fq, lanes, log_k, (int)log_weight, level == 0 ? 1 : 0, in, dst);
            in = dst;
            count >>= log_k;
            log_weight += log_k;
        }
        hipLaunchKernelGGL(msmf_finish_kernel, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, st, fq, (uint32_t)cnt, W, C, in, (uint32_t *)(d_out + lo * 8));
        e = hipGetLastError();
        if (e != hipSuccess) return record_hip_error(e, "frw_msmf_dev");
    }
    return FRW_OK;
}
