// frw_qap_small.hip -- the R1CS -> QAP witness map on the domains frw_qap.hip has no pass schedule for: 2^1 .. 2^13.
//
// ark-groth16's witness_map as it is written (r1cs_to_qap.rs), for every statement of a batch whatever its witness:
//     a = A z ++ instance, b = B z, c = C z;   ifft;   coset_fft (generator 7);   a o b - c;   / (7^n - 1);   coset_ifft
// A latency path for tiny problems (the systems a new user starts with), so the simple form: plain radix-2 stages, one
// workgroup per array, a barrier between stages.
//     qap_small_coset_kernel   one workgroup per (statement, matrix): the array goes into the working buffer bit-reversed,
//                              L decimation-in-time stages with w^-1 (natural order out), x g^k / n, L decimation-in-frequency
//                              stages with w (bit-reversed out) -> the statement's working array in the workspace
//     qap_small_h_kernel       one workgroup per statement: a b - c where the three lie (bit-reversed order, the same for all),
//                              L decimation-in-time stages with w^-1, x g^-k / (n (g^n - 1)), canonical -> h
// The working buffer is LDS up to 2^12 (4,096 packed elements = 128 KiB of the CU's 160), and for 2^13 -- 256 KiB -- the
// statement's own working array in the workspace: the same stages through memory, ordered by the same workgroup barriers (a
// workgroup's waves share one CU and its vector cache; __syncthreads orders their global accesses).
// Twiddles: one table per handle (frw_r1cs.cpp upload_qap_tables), every entry x R' packed and canonical.
// Arithmetic: frw_fr29.h; every stored value is < 2 p and travels packed in 8 x 32 bits, as in frw_qap.hip.  Field arithmetic
// is exact: the result is element for element what the passes of frw_qap.hip would give.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frw_device.h"
#include "frw_fr29.h"

namespace frw {

constexpr int QAP_SMALL_THREADS = 512;
constexpr int QAP_SMALL_LDS_LOG_N = 12;                                  // the largest domain whose array stays in LDS
constexpr int QAP_SMALL_LDS_WORDS = 8 << QAP_SMALL_LDS_LOG_N;            // 128 KiB

struct QapSmallArgs {
    const uint32_t *abc;        // [statements][3][C][8]
    const uint32_t *instance;   // [statements][I][8]
    uint32_t *work;             // [statements][3][n][8]
    uint32_t *h;                // [statements][n][8]
    const uint32_t *tab;        // QapDev::small_tab
    uint32_t num_constraints, num_instance;
    int L;
};

// the handle's table, in elements of 8 words: w^k and w^-k (k < n / 2; one entry at n = 2), then three per-index factors
__device__ __forceinline__ const uint32_t *small_w_fwd(const QapSmallArgs &p) { return p.tab; }
__device__ __forceinline__ const uint32_t *small_w_inv(const QapSmallArgs &p) { return p.tab + ((size_t)4 << p.L); }
__device__ __forceinline__ const uint32_t *small_scale(const QapSmallArgs &p, int which) { return p.tab + ((size_t)(8 + 8 * which) << p.L); }

// L decimation-in-time stages (bit-reversed in, natural out) over buf[n][8]; values < 2 p in and out
__device__ __forceinline__ void small_dit(uint32_t *buf, const uint32_t *w, int L)
{
    const uint32_t half_n = 1u << (L - 1);
    for (int s = 1; s <= L; s++) {
        const uint32_t half = 1u << (s - 1);
        for (uint32_t j = threadIdx.x; j < half_n; j += QAP_SMALL_THREADS) {
            const uint32_t pos = j & (half - 1), i0 = ((j >> (s - 1)) << s) | pos, i1 = i0 + half;
            const F29 u = f29_unpack(fr_load(buf + (size_t)i0 * 8));
            const F29 v = f29_mul(f29_unpack(fr_load(buf + (size_t)i1 * 8)), f29_unpack(fr_load(w + ((size_t)pos << (L - s)) * 8)));
            fr_store(buf + (size_t)i0 * 8, f29_pack(f29_reduce_4p(f29_add(u, v))));
            fr_store(buf + (size_t)i1 * 8, f29_pack(f29_reduce_4p(f29_sub_kp<2>(u, v))));
        }
        __syncthreads();
    }
}

// L decimation-in-frequency stages (natural in, bit-reversed out)
__device__ __forceinline__ void small_dif(uint32_t *buf, const uint32_t *w, int L)
{
    const uint32_t half_n = 1u << (L - 1);
    for (int s = L; s >= 1; s--) {
        const uint32_t half = 1u << (s - 1);
        for (uint32_t j = threadIdx.x; j < half_n; j += QAP_SMALL_THREADS) {
            const uint32_t pos = j & (half - 1), i0 = ((j >> (s - 1)) << s) | pos, i1 = i0 + half;
            const F29 u = f29_unpack(fr_load(buf + (size_t)i0 * 8)), v = f29_unpack(fr_load(buf + (size_t)i1 * 8));
            fr_store(buf + (size_t)i0 * 8, f29_pack(f29_reduce_4p(f29_add(u, v))));
            fr_store(buf + (size_t)i1 * 8, f29_pack(f29_mul(f29_sub_kp<2>(u, v), f29_unpack(fr_load(w + ((size_t)pos << (L - s)) * 8)))));
        }
        __syncthreads();
    }
}

// GLOBAL: the working buffer is the array's place in the workspace (2^13); else LDS
template <bool GLOBAL>
__global__ __launch_bounds__(QAP_SMALL_THREADS) void qap_small_coset_kernel(const QapSmallArgs p)
{
    __shared__ uint32_t lds[GLOBAL ? 8 : QAP_SMALL_LDS_WORDS];
    const uint32_t n = 1u << p.L, which = blockIdx.x;
    const size_t sig = blockIdx.y;
    uint32_t *out = p.work + (sig * 3 + which) * (size_t)n * 8;
    uint32_t *buf = GLOBAL ? out : lds;
    const uint32_t *rows = p.abc + (sig * 3 + which) * (size_t)p.num_constraints * 8;
    const uint32_t *inst = p.instance + sig * (size_t)p.num_instance * 8;
    // the constraint rows, then (A only) the instance values, then zeros; element i to place bitrev(i)
    for (uint32_t i = threadIdx.x; i < n; i += QAP_SMALL_THREADS) {
        Fr8 v;
#pragma unroll
        for (int k = 0; k < 8; k++) v.l[k] = 0;
        if (i < p.num_constraints) v = fr_load(rows + (size_t)i * 8);
        else if (which == 0 && i - p.num_constraints < p.num_instance) v = fr_load(inst + (size_t)(i - p.num_constraints) * 8);
        fr_store(buf + (size_t)(__brev(i) >> (32 - p.L)) * 8, v);
    }
    __syncthreads();
    small_dit(buf, small_w_inv(p), p.L);
    // g^k / n (A z: 2^5 g^k / n -- the a b product in R' = 2^261 arithmetic takes the 2^5 out again)
    const uint32_t *scale = small_scale(p, which == 0 ? 1 : 0);
    for (uint32_t k = threadIdx.x; k < n; k += QAP_SMALL_THREADS)
        fr_store(buf + (size_t)k * 8, f29_pack(f29_mul(f29_unpack(fr_load(buf + (size_t)k * 8)), f29_unpack(fr_load(scale + (size_t)k * 8)))));
    __syncthreads();
    small_dif(buf, small_w_fwd(p), p.L);
    if (!GLOBAL)
        for (uint32_t k = threadIdx.x; k < n; k += QAP_SMALL_THREADS) fr_store(out + (size_t)k * 8, fr_load(buf + (size_t)k * 8));
}

template <bool GLOBAL>
__global__ __launch_bounds__(QAP_SMALL_THREADS) void qap_small_h_kernel(const QapSmallArgs p)
{
    __shared__ uint32_t lds[GLOBAL ? 8 : QAP_SMALL_LDS_WORDS];
    const uint32_t n = 1u << p.L;
    const size_t sig = blockIdx.x;
    uint32_t *a = p.work + sig * 3 * (size_t)n * 8;
    const uint32_t *b = a + (size_t)n * 8, *c = b + (size_t)n * 8;
    uint32_t *buf = GLOBAL ? a : lds;
    // (a 2^5 R)(b R) / R' - c R = (a b - c) R on the coset, in the transforms' bit-reversed order
    for (uint32_t j = threadIdx.x; j < n; j += QAP_SMALL_THREADS) {
        const F29 ab = f29_mul(f29_unpack(fr_load(a + (size_t)j * 8)), f29_unpack(fr_load(b + (size_t)j * 8)));
        fr_store(buf + (size_t)j * 8, f29_pack(f29_reduce_4p(f29_sub_kp<2>(ab, f29_unpack(fr_load(c + (size_t)j * 8))))));
    }
    __syncthreads();
    small_dit(buf, small_w_inv(p), p.L);
    const uint32_t *scale = small_scale(p, 2);                           // g^-k / (n (g^n - 1))
    uint32_t *h = p.h + sig * (size_t)n * 8;
    for (uint32_t k = threadIdx.x; k < n; k += QAP_SMALL_THREADS)
        fr_store(h + (size_t)k * 8, f29_pack(f29_canonical(f29_mul(f29_unpack(fr_load(buf + (size_t)k * 8)), f29_unpack(fr_load(scale + (size_t)k * 8))))));
}

size_t qap_small_table_words(int L) { return (size_t)32 << L; }         // (n / 2 + n / 2 + 3 n) x 8, n / 2 taken as n / 2 >= 1

// The chunk loop and the workspace are launch_qap_witness_map's: A z, B z, C z | three working arrays | flags per statement.
hipError_t launch_qap_small(const R1csDev &r, const QapDev &q, size_t batch, const uint64_t *witness, const uint64_t *instance, uint64_t *h,
                            uint32_t *num_unsatisfied, void *workspace, size_t workspace_bytes, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    const int L = q.log_n;
    if (L < 1 || L >= QAP_MIN_LOG_N || !q.small_tab) return hipErrorInvalidValue;
    const size_t n = (size_t)1 << L, per_sig = qap_workspace_bytes_per_signature(r, q);
    size_t chunk = workspace_bytes / per_sig;
    if (chunk == 0) return hipErrorInvalidValue;
    if (chunk > 16384) chunk = 16384;
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = batch - lo < chunk ? batch - lo : chunk;
        uint32_t *abc = (uint32_t *)workspace;
        uint32_t *work = abc + cnt * 3 * (size_t)r.num_constraints * 8;
        const uint64_t *wit = witness + lo * (size_t)r.num_witness * 4, *inst = instance + lo * (size_t)r.num_instance * 4;
        // the working arrays are idle during the products: they lend the scratch (the loader has seen to it that they can)
        if (r1cs_check_scratch_bytes(r, cnt, true) > cnt * 3 * n * 32) return hipErrorInvalidValue;
        hipError_t e = launch_r1cs_check(r, cnt, wit, inst, num_unsatisfied ? num_unsatisfied + lo : nullptr, (uint64_t *)abc, st, work);
        if (e != hipSuccess) return e;
        const QapSmallArgs p{abc, (const uint32_t *)inst, work, (uint32_t *)(h + lo * n * 4), q.small_tab, r.num_constraints, r.num_instance, L};
        if (L <= QAP_SMALL_LDS_LOG_N) {
            hipLaunchKernelGGL(qap_small_coset_kernel<false>, dim3(3, (unsigned)cnt), dim3(QAP_SMALL_THREADS), 0, st, p);
            hipLaunchKernelGGL(qap_small_h_kernel<false>, dim3((unsigned)cnt), dim3(QAP_SMALL_THREADS), 0, st, p);
        } else {
            hipLaunchKernelGGL(qap_small_coset_kernel<true>, dim3(3, (unsigned)cnt), dim3(QAP_SMALL_THREADS), 0, st, p);
            hipLaunchKernelGGL(qap_small_h_kernel<true>, dim3((unsigned)cnt), dim3(QAP_SMALL_THREADS), 0, st, p);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace frw
