// frw_msm_field2.hip -- frw_curve2_* and frw_msmf2_*: sum_i k_i Q_i on a curve y^2 = x^3 + b' over Fq2 = Fq[u] / (u^2 - beta), q, r, beta
// and b' given at run time (frw_curve2.h: the descriptor, Fe2, the complete group law; BN254's G2 is the case users have).  The G2 code
// of frw_msm.hip has BLS12-381's 29-bit limbs compiled in and does not carry over.
//
// The schedule is frw_msm_field.hip's rule: C x W = 13 x 20 windows below 2^16 points, 15 x 18 from there on,
// signed_digits of frw_digits.h unchanged; per chunk of statements
//     0 clear  1 digits  2 scan  3 scatter      the scalar side: it does not depend on the group and is restated here under names of
//                                               its own (that unit stays as it is, byte for byte)
//     4 buckets    a lane per key, mixed additions (10 Fe2 products = 30 to 32 field products each)
//     5 fold       levels of 8 by running sums, the block's weight by doublings
//     6 finish     a lane per statement: Horner over the windows, one inversion in Fq, the affine point out
// What is new is the shape of the group side.  An XYZZ accumulator over Fe2 is 64 words; with a point and a mixed addition's temporaries
// a lane wants more than the 256 registers that two waves per SIMD leave it, and a fold with three accumulators more than the 512 of one
// wave.  So NO accumulator lives in registers: each lane keeps its accumulators in a column of LDS (256 bytes each, sixteen 16-byte
// quads, quad k of lane t at [k][t]: consecutive lanes read consecutive quads, no bank conflict, and a lane touches its own column only,
// so no barrier), and the additions below read a coordinate when they need it and write it back as soon as it is final.  Registers
// then hold four to six Fe2 at the peak.  The LDS traffic -- 128 words in and out per addition against ~30 field products of 128
// multiply-adds each -- is noise.  The bucket kernel's 64 KiB a workgroup of 256 lanes is what two waves per SIMD take of the 160 KiB.
// Every data-dependent address is bounded as in frw_msm_field.hip.  Everything on the caller's stream, nothing allocated, no
// synchronisation, no host branch on device data: the call may be captured, and is then a chain of kernel nodes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <new>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_curve2.h"
#include "frw_digits.h"
#include "frw_layout.h"

namespace frw {

constexpr uint32_t MSMF2_MAX_POINTS = 1u << 22;
constexpr uint32_t MSMF2_WIDE_FROM = 1u << 16;     // points from which the windows are 15 bits
constexpr size_t MSMF2_MAX_CHUNK = 32768;          // statements of one launch sequence (a grid's y)
constexpr int MSMF2_QUADS = MSMF2_XYZZ_WORDS / 4;  // 16-byte quads of an XYZZ item

namespace {

// A lane's XYZZ accumulator in LDS: coordinate c (0 X, 1 Y, 2 ZZ, 3 ZZZ) is quads 4 c .. 4 c + 3 of the lane's column.
template <int LANES> struct LdsXyzz2 {
    uint4 *col;                                                    // &lds[slot][0][lane]
    // (the compiler barrier: a coordinate is READ AGAIN where it is needed, not kept in registers from its last use and not fetched ahead
    // of the products before it -- that is what holds the registers of an addition to its temporaries)
    __device__ __forceinline__ Fe fe(int quad) const
    {
        asm volatile("" ::: "memory");
        const uint4 a = col[quad * LANES], b = col[(quad + 1) * LANES];
        return Fe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
    }
    __device__ __forceinline__ void fe_put(int quad, const Fe &v) const
    {
        col[quad * LANES] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
        col[(quad + 1) * LANES] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
    }
    __device__ __forceinline__ Fe2 get(int c) const { return Fe2{fe(4 * c), fe(4 * c + 2)}; }
    __device__ __forceinline__ void put(int c, const Fe2 &v) const { fe_put(4 * c, v.c0); fe_put(4 * c + 2, v.c1); }
    __device__ __forceinline__ void set_identity() const
    {
#pragma unroll
        for (int k = 0; k < MSMF2_QUADS; k++) col[k * LANES] = make_uint4(0, 0, 0, 0);
    }
    __device__ __forceinline__ void load(const uint32_t *__restrict__ w) const       // an item of the workspace
    {
#pragma unroll
        for (int k = 0; k < MSMF2_QUADS; k++) col[k * LANES] = ((const uint4 *)w)[k];
    }
    __device__ __forceinline__ void store(uint32_t *__restrict__ w) const
    {
#pragma unroll
        for (int k = 0; k < MSMF2_QUADS; k++) ((uint4 *)w)[k] = col[k * LANES];
    }
    __device__ __forceinline__ void copy_from(const LdsXyzz2 &o) const
    {
#pragma unroll
        for (int k = 0; k < MSMF2_QUADS; k++) col[k * LANES] = o.col[k * LANES];
    }
};

// A <- 2 A (xyzz2_double): ZZ and ZZZ first, then X and Y, each read when needed and written when final
template <class A> __device__ __forceinline__ void acc_double(const Fq2Consts &f, const A &a)
{
    Fe2 t, v;
    {
        const Fe2 y = a.get(1), u = fe2_add(f, y, y);
        v = fe2_square(f, u);
        const Fe2 w = fe2_mul(f, u, v);
        a.put(3, fe2_mul(f, w, a.get(3)));
        a.put(2, fe2_mul(f, v, a.get(2)));
        t = fe2_mul(f, w, y);
    }
    const Fe2 x = a.get(0), s = fe2_mul(f, x, v), xx = fe2_square(f, x), m = fe2_add(f, fe2_add(f, xx, xx), xx);
    const Fe2 x3 = fe2_sub(f, fe2_sub(f, fe2_square(f, m), s), s);
    a.put(0, x3);
    a.put(1, fe2_sub(f, fe2_mul(f, m, fe2_sub(f, s, x3)), t));
}

// A <- A + P, P affine in registers (xyzz2_add_affine), complete
template <class A> __device__ __forceinline__ void acc_add_affine(const Fq2Consts &f, const A &a, const Affine2 &p)
{
    if (affine2_is_infinity(p)) return;
    Fe2 pd, rd;
    {
        const Fe2 zz = a.get(2);
        if (fe2_is_zero(zz)) {
            a.put(0, p.x); a.put(1, p.y); a.put(2, fe2_one(f)); a.put(3, fe2_one(f));
            return;
        }
        pd = fe2_sub(f, fe2_mul(f, p.x, zz), a.get(0));
    }
    rd = fe2_sub(f, fe2_mul(f, p.y, a.get(3)), a.get(1));
    if (fe2_is_zero(pd)) {                                         // the same x: the same point, or its negative
        if (fe2_is_zero(rd)) acc_double(f, a);
        else a.set_identity();
        return;
    }
    Fe2 q, ppp;
    {
        const Fe2 pp = fe2_square(f, pd);
        a.put(2, fe2_mul(f, a.get(2), pp));
        q = fe2_mul(f, a.get(0), pp);
        ppp = fe2_mul(f, pd, pp);
    }
    a.put(3, fe2_mul(f, a.get(3), ppp));
    const Fe2 t = fe2_mul(f, a.get(1), ppp);
    const Fe2 x3 = fe2_sub(f, fe2_sub(f, fe2_sub(f, fe2_square(f, rd), ppp), q), q);
    a.put(0, x3);
    a.put(1, fe2_sub(f, fe2_mul(f, rd, fe2_sub(f, q, x3)), t));
}

// A <- A + B, both in LDS, A != B (xyzz2_add), complete
template <class A> __device__ __forceinline__ void acc_add(const Fq2Consts &f, const A &a, const A &b)
{
    Fe2 u1, pd;
    {
        const Fe2 bzz = b.get(2);
        if (fe2_is_zero(bzz)) return;
        const Fe2 azz = a.get(2);
        if (fe2_is_zero(azz)) { a.copy_from(b); return; }
        u1 = fe2_mul(f, a.get(0), bzz);
        pd = fe2_sub(f, fe2_mul(f, b.get(0), azz), u1);
    }
    const Fe2 s1 = fe2_mul(f, a.get(1), b.get(3)), rd = fe2_sub(f, fe2_mul(f, b.get(1), a.get(3)), s1);
    if (fe2_is_zero(pd)) {
        if (fe2_is_zero(rd)) acc_double(f, a);
        else a.set_identity();
        return;
    }
    const Fe2 pp = fe2_square(f, pd), ppp = fe2_mul(f, pd, pp);
    a.put(2, fe2_mul(f, fe2_mul(f, a.get(2), b.get(2)), pp));
    a.put(3, fe2_mul(f, fe2_mul(f, a.get(3), b.get(3)), ppp));
    const Fe2 q = fe2_mul(f, u1, pp);
    const Fe2 x3 = fe2_sub(f, fe2_sub(f, fe2_sub(f, fe2_square(f, rd), ppp), q), q);
    a.put(0, x3);
    a.put(1, fe2_sub(f, fe2_mul(f, rd, fe2_sub(f, q, x3)), fe2_mul(f, s1, ppp)));
}

__device__ __forceinline__ void fe_store(uint32_t *w, const Fe &a)
{
    ((uint4 *)w)[0] = make_uint4(a.l[0], a.l[1], a.l[2], a.l[3]);
    ((uint4 *)w)[1] = make_uint4(a.l[4], a.l[5], a.l[6], a.l[7]);
}

}  // namespace

// the first base that is not on the curve (0xffffffff: none)
__global__ __launch_bounds__(256) void msmf2_check_kernel(const Curve2Consts cc, uint32_t n, const uint32_t *__restrict__ bases, uint32_t *__restrict__ first_bad)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!curve2_on_curve(cc, affine2_load(bases + (size_t)i * 32))) atomicMin(first_bad, i);
}

// 0: the keys' counts to zero (a kernel, not a memset node)
__global__ __launch_bounds__(256) void msmf2_clear_kernel(uint4 *__restrict__ words, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) words[i] = make_uint4(0, 0, 0, 0);
}

// 1: the digits of scalar i of statement y, and the histogram of its keys
template <int C, int W>
__global__ __launch_bounds__(256) void msmf2_digits_kernel(const FieldConsts fr, uint32_t n, uint32_t num_scalars, const uint32_t *__restrict__ scalars,
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
__global__ __launch_bounds__(1024) void msmf2_scan_kernel(uint32_t keys, const uint32_t *__restrict__ counts, uint32_t *__restrict__ offsets, uint32_t *__restrict__ cursor)
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
__global__ __launch_bounds__(256) void msmf2_scatter_kernel(uint32_t n, uint32_t num_scalars, int windows, uint32_t buckets, const int16_t *__restrict__ digits,
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

// 4: a lane per key.  The accumulator is the lane's column of LDS; the point (32 words) and a mixed addition's temporaries are registers.
__global__ __launch_bounds__(256, 2) void msmf2_bucket_kernel(const Fq2Consts f2, uint32_t n, uint32_t keys, size_t entries_per_statement,
                                                              const uint32_t *__restrict__ bases, const uint32_t *__restrict__ offsets,
                                                              const uint32_t *__restrict__ counts, const uint32_t *__restrict__ entries,
                                                              uint32_t *__restrict__ buckets)
{
    __shared__ uint4 lds[MSMF2_QUADS * 256];
    const size_t y = blockIdx.y;
    const uint32_t key = blockIdx.x * 256 + threadIdx.x;           // keys: a multiple of 256
    const size_t at = y * keys + key;
    // (first <= entries_per_statement and first + cnt <= it with counts that are this call's; held to it here, and an index to n below, so
    // that no address of this kernel hangs on what another kernel wrote)
    const size_t off = offsets[at], first = off < entries_per_statement ? off : entries_per_statement, room = entries_per_statement - first;
    const uint32_t cnt = counts[at] < room ? counts[at] : (uint32_t)room;
    const uint32_t *ent = entries + y * entries_per_statement + first;
    const LdsXyzz2<256> acc{lds + threadIdx.x};
    acc.set_identity();
    for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t e = ent[j];
        if ((e & 0x7fffffffu) >= n) continue;
        Affine2 p = affine2_load(bases + (size_t)(e & 0x7fffffffu) * 32);
        if (e >> 31) p.y = fe2_neg(f2, p.y);
        acc_add_affine(f2, acc, p);
    }
    acc.store(buckets + at * MSMF2_XYZZ_WORDS);
}

constexpr size_t msmf2_fold_lds_bytes(bool first) { return (size_t)(first ? 3 : 4) * MSMF2_QUADS * 64 * sizeof(uint4); }

// 5: one level of the fold.  The items of a window are `count` (weighted, plain) pairs, each a block of 2^log_weight buckets -- at the first
// level the buckets themselves, both halves the bucket.  Lane g of a window joins items g K .. g K + K - 1:
//     plain' = sum T_i,    weighted' = sum S_i + 2^log_weight sum i T_i      (running sums from the top: sum i T_i = sum of the runs)
// Slots of LDS a lane: the running sum, the sum of the runs, the item that came in, and -- not at the first level, which has no weighted
// halves to add -- the weighted sum.  LDS is what holds the kernel's occupancy (one wave per SIMD by registers, 16 KiB a slot and a
// workgroup), so the launch asks for the slots it uses: three at the first level, the one with eight times the lanes of the next.
// The additions are ONE piece of code, its operands picked by slot.
__global__ __launch_bounds__(64, 1) void msmf2_fold_kernel(const Fq2Consts f2, uint32_t lanes /* a statement's: windows count / K */, int log_k, int log_weight,
                                                           int first, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    extern __shared__ uint4 lds[];                                 // msmf2_fold_lds_bytes(first)
    enum { RUN = 0, ACC = 1, ITEM = 2, WEIGHTED = 3 };
    const size_t y = blockIdx.y;
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t K = 1u << log_k;
    const size_t item_words = first ? MSMF2_XYZZ_WORDS : 2 * MSMF2_XYZZ_WORDS;
    const uint32_t *src = in + (y * ((size_t)lanes << log_k) + ((size_t)g << log_k)) * item_words;
    auto slot = [&](int s) { return LdsXyzz2<64>{lds + s * (MSMF2_QUADS * 64) + threadIdx.x}; };
    slot(RUN).set_identity();
    slot(ACC).set_identity();
    if (!first) slot(WEIGHTED).set_identity();
    // item i from the top, step 0: weighted += S_i (not at the first level)   1: run += T_i   2: acc += run (not for i = 0);
    // then acc <- 2^log_weight acc and the last addition, acc += weighted (at the first level: += run) -- the same piece of code
    uint32_t i = K - 1;
    int step = first ? 1 : 0;
    for (bool last = false;;) {
        int dst = ACC, from = first ? RUN : WEIGHTED;
        if (!last) {
            if (step < 2) slot(ITEM).load(src + i * item_words + (step == 1 && !first ? MSMF2_XYZZ_WORDS : 0));
            dst = step == 0 ? WEIGHTED : step == 1 ? RUN : ACC;
            from = step == 2 ? RUN : ITEM;
        }
        acc_add(f2, slot(dst), slot(from));
        if (last) break;
        if (++step < (i ? 3 : 2)) continue;
        step = first ? 1 : 0;
        if (i-- == 0) {
            for (int k = 0; k < log_weight; k++) acc_double(f2, slot(ACC));
            last = true;
        }
    }
    uint32_t *dst = out + (y * lanes + g) * (size_t)(2 * MSMF2_XYZZ_WORDS);
    slot(ACC).store(dst);
    slot(RUN).store(dst + MSMF2_XYZZ_WORDS);
}

// 6: Horner over a statement's window sums, the affine point out
__global__ __launch_bounds__(64, 1) void msmf2_finish_kernel(const Fq2Consts f2, uint32_t statements, int windows, int window_bits,
                                                             const uint32_t *__restrict__ sums /* [y][windows][2][64] */, uint32_t *__restrict__ out /* [y][32] */)
{
    __shared__ uint4 lds[2 * MSMF2_QUADS * 64];
    const uint32_t y = blockIdx.x * 64 + threadIdx.x;
    if (y >= statements) return;
    const uint32_t *src = sums + (size_t)y * windows * (2 * MSMF2_XYZZ_WORDS);
    const LdsXyzz2<64> acc{lds + threadIdx.x}, item{lds + MSMF2_QUADS * 64 + threadIdx.x};
    acc.load(src + (size_t)(windows - 1) * (2 * MSMF2_XYZZ_WORDS));
    for (int j = windows - 2; j >= 0; j--) {
        for (int k = 0; k < window_bits; k++) acc_double(f2, acc);
        item.load(src + (size_t)j * (2 * MSMF2_XYZZ_WORDS));
        acc_add(f2, acc, item);
    }
    const Affine2 a = xyzz2_to_affine(f2, Xyzz2{acc.get(0), acc.get(1), acc.get(2), acc.get(3)});
    uint32_t *dst = out + (size_t)y * 32;
    fe_store(dst, a.x.c0); fe_store(dst + 8, a.x.c1); fe_store(dst + 16, a.y.c0); fe_store(dst + 24, a.y.c1);
}

}  // namespace frw

// ---- the handle ------------------------------------------------------------------------------------------------------------------
struct frw_msmf2 {
    int device = 0;
    frw::Curve2Derived curve{};
    uint32_t n = 0;
    int window_bits = 0, windows = 0;
    uint32_t *bases = nullptr;
    size_t per_statement = 0;
};

namespace {
using namespace frw;

int derive_curve2(const char *who, const frw_curve2_t *c, Curve2Derived *out)
{
    if (!c) { record_error("%s: null pointer", who); return FRW_E_INVALID_ARG; }
    const char *refusal = curve2_derive(c->base_modulus, c->scalar_modulus, c->nonresidue, c->b, out);
    if (refusal[0]) { record_error("%s: %s", who, refusal); return FRW_E_INVALID_ARG; }
    return FRW_OK;
}

}  // namespace

extern "C" int frw_curve2_info(const frw_curve2_t *c, frw_curve2_info_t *out)
{
    Curve2Derived d;
    if (!out) { record_error("frw_curve2_info: null pointer"); return FRW_E_INVALID_ARG; }
    const int rc = derive_curve2("frw_curve2_info", c, &d);
    if (rc != FRW_OK) return rc;
    out->base_bits = d.q.bits;
    out->scalar_bits = d.r.bits;
    uint32_t b0[8], b1[8];
    for (int j = 0; j < 8; j++) { b0[j] = d.cc.b[j]; b1[j] = d.cc.b[8 + j]; }
    field_limbs(b0, out->b_mont);
    field_limbs(b1, out->b_mont + 4);
    field_limbs(d.q.fc.one, out->one_mont);
    field_limbs(d.cc.f2.beta, out->nonresidue_mont);
    field_limbs(d.r.fc.one, out->scalar_one_mont);
    out->nonresidue_is_minus_one = d.cc.f2.beta_m1;
    out->reserved = 0;
    return FRW_OK;
}

extern "C" int frw_curve2_check_points(const frw_curve2_t *c, size_t count, const uint64_t *points, int64_t *first_bad)
{
    Curve2Derived d;
    if (!first_bad || (!points && count)) { record_error("frw_curve2_check_points: null pointer"); return FRW_E_INVALID_ARG; }
    const int rc = derive_curve2("frw_curve2_check_points", c, &d);
    if (rc != FRW_OK) return rc;
    *first_bad = -1;
    for (size_t i = 0; i < count; i++)
        if (!curve2_on_curve(d.cc, affine2_from_limbs(points + 16 * i))) { *first_bad = (int64_t)i; break; }
    return FRW_OK;
}

extern "C" int frw_curve2_scalar_mul(const frw_curve2_t *c, size_t count, const uint64_t *points, const uint64_t *scalars, uint64_t *out)
{
    Curve2Derived d;
    if (count && (!points || !scalars || !out)) { record_error("frw_curve2_scalar_mul: null pointer"); return FRW_E_INVALID_ARG; }
    const int rc = derive_curve2("frw_curve2_scalar_mul", c, &d);
    if (rc != FRW_OK) return rc;
    for (size_t i = 0; i < count; i++) {
        const Affine2 p = affine2_from_limbs(points + 16 * i);
        if (!curve2_on_curve(d.cc, p)) {
            record_error("frw_curve2_scalar_mul: point %zu is not on the curve", i);
            return FRW_E_INVALID_ARG;
        }
        affine2_to_limbs(curve2_scalar_mul(d.cc, p, scalars + 4 * i), out + 16 * i);
    }
    return FRW_OK;
}

extern "C" void frw_msmf2_free(frw_msmf2 *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->bases) (void)hipFree(m->bases);
    delete m;
}

extern "C" int frw_msmf2_load(int device, const frw_curve2_t *c, size_t num_points, const uint64_t *bases, int flags, frw_msmf2 **out)
{
    if (!out) { record_error("frw_msmf2_load: null pointer"); return FRW_E_INVALID_ARG; }
    *out = nullptr;
    if (!bases) { record_error("frw_msmf2_load: null pointer"); return FRW_E_INVALID_ARG; }
    Curve2Derived d;
    const int rc = derive_curve2("frw_msmf2_load", c, &d);
    if (rc != FRW_OK) return rc;
    if (num_points == 0 || num_points > MSMF2_MAX_POINTS) {
        record_error("frw_msmf2_load: %zu points (1 .. 2^22)", num_points);
        return FRW_E_INVALID_ARG;
    }
    if (flags & ~FRW_MSMF_POINTS_ARE_CHECKED) { record_error("frw_msmf2_load: unknown flags"); return FRW_E_INVALID_ARG; }
    frw_msmf2 *m = new (std::nothrow) frw_msmf2;
    if (!m) return FRW_E_OUT_OF_MEMORY;
    m->device = device;
    m->curve = d;
    m->n = (uint32_t)num_points;
    const bool wide = m->n >= MSMF2_WIDE_FROM;
    m->window_bits = wide ? 15 : 13;
    m->windows = wide ? 18 : 20;
    m->per_statement = msmf2_layout(nullptr, 1, m->n, m->window_bits, m->windows).bytes;
    hipError_t e = hipSetDevice(device);
    uint32_t *d_bad = nullptr;
    if (e == hipSuccess) e = hipMalloc((void **)&m->bases, num_points * 128);
    if (e == hipSuccess) e = hipMemcpy(m->bases, bases, num_points * 128, hipMemcpyHostToDevice);
    uint32_t bad = 0xffffffffu;
    if (e == hipSuccess && !(flags & FRW_MSMF_POINTS_ARE_CHECKED)) {
        e = hipMalloc((void **)&d_bad, 4);
        if (e == hipSuccess) e = hipMemcpy(d_bad, &bad, 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(msmf2_check_kernel, dim3((m->n + 255) / 256), dim3(256), 0, 0, d.cc, m->n, (const uint32_t *)m->bases, d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
        if (d_bad) (void)hipFree(d_bad);
    }
    if (e != hipSuccess) { frw_msmf2_free(m); return record_hip_error(e, "frw_msmf2_load"); }
    if (bad != 0xffffffffu) {
        frw_msmf2_free(m);
        record_error("frw_msmf2_load: base %u is not on the curve", bad);
        return FRW_E_INVALID_ARG;
    }
    *out = m;
    return FRW_OK;
}

extern "C" int frw_msmf2_info(const frw_msmf2 *m, frw_msmf2_info_t *out)
{
    if (!m || !out) { record_error("frw_msmf2_info: null pointer"); return FRW_E_INVALID_ARG; }
    out->num_points = m->n;
    out->window_bits = (uint32_t)m->window_bits;
    out->num_windows = (uint32_t)m->windows;
    out->reserved = 0;
    out->bases_bytes = (uint64_t)m->n * 128;
    out->workspace_bytes_per_statement = m->per_statement;
    return FRW_OK;
}

extern "C" size_t frw_msmf2_workspace_bytes(const frw_msmf2 *m, size_t batch_in_flight)
{
    if (!m || batch_in_flight == 0) return 0;
    return msmf2_layout(nullptr, batch_in_flight, m->n, m->window_bits, m->windows).bytes;
}

extern "C" int frw_msmf2_dev(const frw_msmf2 *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, size_t num_scalars, int montgomery,
                             uint64_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!m) { record_error("frw_msmf2_dev: null pointer"); return FRW_E_INVALID_ARG; }
    if (num_scalars > m->n) { record_error("frw_msmf2_dev: %zu scalars for %u points", num_scalars, m->n); return FRW_E_INVALID_ARG; }
    if (scalar_stride < num_scalars) { record_error("frw_msmf2_dev: a stride of %zu for %zu scalars", scalar_stride, num_scalars); return FRW_E_INVALID_ARG; }
    if (batch == 0) return FRW_OK;
    if (!d_out || !d_workspace || (!d_scalars && num_scalars)) { record_error("frw_msmf2_dev: null pointer"); return FRW_E_INVALID_ARG; }
    if (((uintptr_t)d_workspace & 15) || ((uintptr_t)d_scalars & 15) || ((uintptr_t)d_out & 15)) {
        record_error("frw_msmf2_dev: a buffer is not 16-byte aligned");
        return FRW_E_INVALID_ARG;
    }
    if (workspace_bytes < m->per_statement) {
        record_error("frw_msmf2_dev: a workspace of %zu bytes, a statement takes %zu", workspace_bytes, m->per_statement);
        return FRW_E_INVALID_ARG;
    }
    hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) return record_hip_error(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const int C = m->window_bits, W = m->windows;
    const uint32_t n = m->n, buckets = 1u << (C - 1), keys = (uint32_t)W * buckets, ns = (uint32_t)num_scalars;
    const Fq2Consts &f2 = m->curve.cc.f2;
    const size_t chunk = proofs_in_flight(std::min(batch, MSMF2_MAX_CHUNK), workspace_bytes,
                                          [&](size_t k) { return msmf2_layout(nullptr, k, n, C, W).bytes; });
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = std::min(chunk, batch - lo);
        const Msmf2Bufs b = msmf2_layout(d_workspace, cnt, n, C, W);
        const uint32_t *scalars = (const uint32_t *)(d_scalars + lo * scalar_stride * 4);
        const size_t count16 = cnt * keys / 4;                         // keys: a multiple of four
        hipLaunchKernelGGL(msmf2_clear_kernel, dim3((unsigned)std::min<size_t>((count16 + 255) / 256, 4096)), dim3(256), 0, st, (uint4 *)b.counts, count16);
        if (ns) {
            const dim3 grid((ns + 255) / 256, (unsigned)cnt);
            if (C == 15)
                hipLaunchKernelGGL((msmf2_digits_kernel<15, 18>), grid, dim3(256), 0, st, m->curve.r.fc, n, ns, scalars, scalar_stride * 8, montgomery, b.digits, b.counts);
            else
                hipLaunchKernelGGL((msmf2_digits_kernel<13, 20>), grid, dim3(256), 0, st, m->curve.r.fc, n, ns, scalars, scalar_stride * 8, montgomery, b.digits, b.counts);
        }
        hipLaunchKernelGGL(msmf2_scan_kernel, dim3((unsigned)cnt), dim3(1024), 0, st, keys, (const uint32_t *)b.counts, b.offsets, b.cursor);
        if (ns)
            hipLaunchKernelGGL(msmf2_scatter_kernel, dim3((ns + 255) / 256, (unsigned)cnt), dim3(256), 0, st, n, ns, W, buckets, (const int16_t *)b.digits, b.cursor, b.entries);
        hipLaunchKernelGGL(msmf2_bucket_kernel, dim3(keys / 256, (unsigned)cnt), dim3(256), 0, st, f2, n, keys, (size_t)W * n, (const uint32_t *)m->bases,
                           (const uint32_t *)b.offsets, (const uint32_t *)b.counts, (const uint32_t *)b.entries, b.buckets);
        const uint32_t *in = b.buckets;
        int level = 0;
        for (uint32_t count = buckets, log_weight = 0; count > 1; level++) {
            const int log_k = count >= (uint32_t)MSMF_FOLD ? MSMF_FOLD_LOG : (count == 4 ? 2 : 1);
            const uint32_t lanes = (uint32_t)W * (count >> log_k);
            uint32_t *dst = b.fold[level & 1];
            hipLaunchKernelGGL(msmf2_fold_kernel, dim3((lanes + 63) / 64, (unsigned)cnt), dim3(64), msmf2_fold_lds_bytes(level == 0), st, f2, lanes, log_k, (int)log_weight,
                               level == 0 ? 1 : 0, in, dst);
            in = dst;
            count >>= log_k;
            log_weight += log_k;
        }
        hipLaunchKernelGGL(msmf2_finish_kernel, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, st, f2, (uint32_t)cnt, W, C, in, (uint32_t *)(d_out + lo * 16));
        e = hipGetLastError();
        if (e != hipSuccess) return record_hip_error(e, "frw_msmf2_dev");
    }
    return FRW_OK;
}
