// frw_msm.hip -- multi-scalar multiplication over BLS12-381 G1 on the device: the step after the QAP witness map in a Groth16
// prover.  examples/pok_sig.rs:30-47 of the reference calls Groth16::<Bls12_381>::prove; ark-groth16 0.3.0 prover.rs
// (create_proof_with_reduction_and_matrices) then computes
//     h_acc = VariableBaseMSM::multi_scalar_mul(&pk.h_query, &h_assignment)          2^18 - 1 points for Falcon-1024
// (and the same over a_query / b_g1_query / l_query with the witness as scalars).  frw_qap_witness_map_dev leaves h in HBM;
// this file consumes it there.
//
// MI355X-first shape.  The bases belong to the proving key: fixed per circuit, shared by every signature ever proved.  So
// (1) frw_msm_g1_load spends 288 GB-class memory on them once: the table holds 2^(16 j) P_i for all sixteen 16-bit windows
//     j (436 MB for 2^18 points, affine, fourteen 29-bit limbs per coordinate), which turns a 255-bit MSM over n points
//     into ONE bucket accumulation over 16 n points with 16-bit signed digits -- no doublings, no per-window passes;
// (2) a call handles a batch of signatures: per signature the 16 n (digit, point) pairs are counting-sorted by bucket
//     (32,768 buckets, ~128 entries each), one thread per bucket adds its entries up in registers (XYZZ coordinates, mixed
//     additions, 8 M + 2 S), gathering the table rows it needs; 512 threads fold the buckets (sum of (b + 1) B_b by running
//     sums over 64-bucket chunks, small multiples, a tree through LDS), and the result leaves as one affine point in
//     ark-ff's bytes.
// Group addition is associative and commutative, so the result does not depend on the order the atomics of the sort
// happened to produce: the output is the unique affine point, bit for bit what any other schedule (or the CPU) gives.
// Field arithmetic: frw_fq29.h.  Bound: vector-ALU issue (a mixed addition is ~5,700 vector instructions), not HBM (a
// signature reads 16 n x 112 B = 0.47 GB of table rows).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <mutex>
#include <vector>
#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_fq29.h"
#include "frw_quad.h"
#include "frw_fr29.h"
#include "frw_digits.h"
#include "frw_drbg.h"
#include "frw_layout.h"
#include "frw_rows.h"

namespace frw {

// (MSM_C = 16, MSM_W = 16, MSM_BUCKETS = 2^15 and every other constant the workspaces' layouts depend on -- MSM_*, WIDE_*, NMSM_*: frw_layout.h)
constexpr int MSM_FOLD_THREADS = 512;           // second stage: one workgroup per signature
// (Grp<F> -- the words of a table row, a bucket, an ark-ff point -- and load_row / store_row / load_ark_point / store_ark_point: frw_rows.h)

struct MsmDev {
    uint32_t n;                 // points
    const uint32_t *table;      // [MSM_W][n][PT_WORDS]
    // narrow handles of up to 2^18 points: sum_(j in m) P_(8 g + j) for every group g of eight consecutive points and every non-empty
    // subset m of it, affine: [ceil(n / 8)][255][PT_WORDS] (as many bytes per point as the window table).  A Falcon witness is 45 % ones
    // in long runs of booleans (bit decompositions, gate outputs): with the pattern of ones of a group as ONE byte, the points whose
    // scalar is one cost one addition per group of eight instead of 3.6.  null: the ones are summed point by point from a list.
    const uint32_t *ones_table;
};

// The narrow sums of ONE sort over up to three window tables in one launch: a proof's a_query, b_g1_query and l_query sums take the
// same scalars, so their digits are sorted once -- and with the tables side by side in the grid the three sums are ONE chain of
// kernels instead of three (a proof made alone waits for the longest chain of small kernels, not for any one of them).  Grid row
// `slot` = table * sigs + signature: the sort's arrays are indexed by the signature, a table's own partial sums and its result by the slot.
struct NmsmTables {
    uint32_t n, sigs;
    const uint32_t *table[3], *ones_table[3];
    __device__ __forceinline__ MsmDev of(uint32_t slot, size_t &sig) const
    {
        const uint32_t t = slot / sigs;
        sig = slot - t * sigs;
        MsmDev m;
        m.n = n;
        m.table = t == 0 ? table[0] : t == 1 ? table[1] : table[2];
        m.ones_table = t == 0 ? ones_table[0] : t == 1 ? ones_table[1] : ones_table[2];
        return m;
    }
};

template <class F> __device__ __forceinline__ void store_bucket(uint32_t *b, const XyzzT<F> &p)
{
    F::store(p.x, b); F::store(p.y, b + F::WORDS); F::store(p.zz, b + 2 * F::WORDS); F::store(p.zzz, b + 3 * F::WORDS);
    b[4 * F::WORDS] = p.inf ? 1u : 0u;
}
template <class F> __device__ __forceinline__ XyzzT<F> load_bucket(const uint32_t *b)
{
    XyzzT<F> p;
    p.x = F::load(b); p.y = F::load(b + F::WORDS); p.zz = F::load(b + 2 * F::WORDS); p.zzz = F::load(b + 3 * F::WORDS);
    p.inf = b[4 * F::WORDS] != 0;
    return p;
}

// ---- load time: table[j][i] = 2^(16 j) P_i, affine, Montgomery limbs ----------------------------------------------------------
template <class F>
__global__ __launch_bounds__(64) void msm_precompute_kernel(uint32_t n, const uint32_t *__restrict__ bases /* [n][ARK_WORDS] ark-ff */,
                                                            uint32_t *__restrict__ table, int window_bits /* 16 or 8 */)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int windows = 256 / window_bits;
    AffineT<F> p = load_ark_point<F>(bases + (size_t)i * Grp<F>::ARK_WORDS);
    for (int j = 0; j < windows; j++) {
        store_row<F>(table + ((size_t)j * n + i) * Grp<F>::PT_WORDS, p);
        if (j + 1 == windows) break;
        XyzzT<F> d = pt_from_affine(p);
        for (int k = 0; k < window_bits; k++) d = pt_double(d);
        p = pt_to_affine(d);
    }
}

// the same from table ROWS (a bare handle's: what the device-side setup fills): a key made on the device grows its window tables here
template <class F>
__global__ __launch_bounds__(64) void msm_precompute_rows_kernel(uint32_t n, const uint32_t *__restrict__ rows /* [n][PT_WORDS] */,
                                                                 uint32_t *__restrict__ table, int window_bits /* 16 or 8 */)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int windows = 256 / window_bits;
    AffineT<F> p = load_row<F>(rows + (size_t)i * Grp<F>::PT_WORDS);
    for (int j = 0; j < windows; j++) {
        store_row<F>(table + ((size_t)j * n + i) * Grp<F>::PT_WORDS, p);
        if (j + 1 == windows) break;
        XyzzT<F> d = pt_from_affine(p);
        for (int k = 0; k < window_bits; k++) d = pt_double(d);
        p = pt_to_affine(d);
    }
}

// load time: ones_table[g][m - 1] = the sum of the points 8 g + j with bit j of m set (window 0 of the table holds the points)
template <class F>
__global__ __launch_bounds__(64) void msm_ones_table_kernel(uint32_t n, const uint32_t *__restrict__ table, uint32_t *__restrict__ ones_table)
{
    const size_t id = (size_t)blockIdx.x * 64 + threadIdx.x, g = id / 255;
    const uint32_t m = (uint32_t)(id % 255) + 1u;
    if (g >= ((size_t)n + 7) / 8) return;
    XyzzT<F> acc = pt_identity<F>();
    for (int j = 0; j < 8; j++) {
        const size_t i = g * 8 + j;
        if (((m >> j) & 1u) && i < n) acc = pt_add_affine(acc, load_row<F>(table + i * Grp<F>::PT_WORDS));
    }
    store_row<F>(ones_table + id * Grp<F>::PT_WORDS, pt_to_affine(acc));
}

// ---- the scalars: canonical integer, signed digits, the bucket and the entry of a digit: frw_digits.h ---------------------------------
// Sixteen 16-bit digits here (32 of 8 bits in the narrow pipeline, 13 of 20 on wide windows).  The scalar 1 gets no digits where it is
// told apart (the sums over window tables, and the narrow sums of bare handles): a Falcon witness is 45 % ones, which would all land in
// bucket 0 of window 0 -- they are summed by msm_ones_kernel / nmsm_ones_kernel instead.  To the dense sums of a bare handle the scalar
// one is digit 1 of window 0 like any other value.

// The counting sort of a signature's 16 n (digit, point) pairs by bucket, without a global atomic: the points are cut into
// MSM_SLICES slices, a workgroup per (signature, slice) histograms its slice in LDS (32,768 counters = 128 KB of the CU's
// 160 KB), the histograms are turned into per-slice starting positions inside every bucket, and the same workgroups then hand
// out positions from LDS again.  (With one global atomicAdd per pair the sort took a third of the whole call: 10^10 atomics
// per second is what the L2 gives, and a signature has 4 x 10^6 pairs to place twice.)
// 32 slices per signature for a batch (their histograms live in the buckets' memory until the first bucket is stored: room for 60);
// a call with ONE signature (an aggregate statement's sum over 2^22 points) would keep 32 of the 256 CUs busy with them, so it cuts
// 224, and parks their histograms in the work items' partial sums instead (131,072 x 240 bytes and more: room for 240), which
// nothing writes before the bucket kernel.
// A BARE handle (round 5) holds the points themselves and nothing else -- 112 bytes a point instead of 1,792: the key of a
// 1,024-statement aggregate is 2^27 points of h_query alone, whose window tables would be 240 GB.  The sum is then sixteen bucket
// accumulations, one per 16-bit window, over the SAME rows: grid row y of every kernel below is window y of ONE scalar vector
// (instead of signature y with all its windows), a row's entries are point indices, and msm_horner_kernel puts the sixteen window
// sums together (15 x 16 doublings).  The number of bucket additions is the table path's: one per (point, non-zero digit).

// The elements [lo, hi) of n that the workgroup's slice (blockIdx.x of gridDim.x) sorts: equal runs, the last ones short or empty (lo may
// lie past hi: slices x ceil(n / slices) < n + slices, nowhere near 2^32).  round_to: runs of whole tiles -- those slices may begin far
// past n, so they are clamped, in 64 bits.
struct SliceRange { uint32_t lo, hi; };
__device__ __forceinline__ SliceRange slice_range(uint32_t n, uint32_t round_to = 1)
{
    const uint32_t slices = gridDim.x, slice = blockIdx.x, per = ((n + slices - 1) / slices + round_to - 1) / round_to * round_to;
    if (round_to == 1) return SliceRange{slice * per, slice * per + per < n ? slice * per + per : n};
    const uint32_t lo = (uint64_t)slice * per < n ? slice * per : n;
    return SliceRange{lo, (uint64_t)lo + per < n ? lo + per : n};
}

// A bare handle's sixteen window rows would each turn the scalars into digits again -- sixteen times the 32-byte reads and the
// Montgomery products, and of the 2^27-point sum over h_query's 446 ms the counting sort took 95 (profiles/r05_aggregate1024_timeline.txt).
// So: ONE pass writes the digits, window-major (int16[16][n]: two bytes per scalar and window), and the rows' histogram and scatter
// read their own window's.
__global__ __launch_bounds__(256) void msm_digits_kernel(uint32_t n, const uint32_t *__restrict__ scalars, int montgomery, int16_t *__restrict__ digits)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int d[MSM_W];
    signed_digits<MSM_C, MSM_W>(scalar_canonical(scalars + (size_t)i * 8, montgomery), d);
#pragma unroll
    for (int j = 0; j < MSM_W; j++) digits[(size_t)j * n + i] = (int16_t)(d[j] == (1 << 15) ? -32768 : d[j]);     // (+2^15 does not fit: stored as its negative's code, told apart below)
}
// digits are in [-2^15 + 1, 2^15]: the one value outside int16, +2^15, travels as -32768 (which no digit is)
__device__ __forceinline__ int msm_digit_load(const int16_t *digits, size_t at)
{
    const int v = digits[at];
    return v == -32768 ? 1 << 15 : v;
}

// Where the digits of a flat sort come from.  A source says how many buckets a grid row has (BUCKETS), how many entries an element can
// leave in it (PER_ROW: a row's entries are [row][PER_ROW n]), and hands each() the non-zero digits of element i of a row, each with the
// id its entry carries; the histogram's pass (`first`) is also the one that records a scalar equal to one.
// Window tables: grid row = signature, every window of the scalar, entry id = the table row j n + i of window j.  A scalar that is one
// goes to the signature's list -- or, MASKED and asked for, into its bit mask (zeroed by the caller; the first n / 32 words of the list).
template <int C, int W, bool MASKED> struct TableDigits {
    static constexpr int BUCKETS = 1 << (C - 1), PER_ROW = W;
    const uint32_t *scalars;
    size_t sig_stride_words;
    int montgomery;
    uint32_t *ones_count /* [sig] */, *ones_list /* [sig][n] */;
    int ones_as_mask;
    template <class Fn> __device__ __forceinline__ void each(size_t sig, uint32_t n, uint32_t i, bool first, Fn fn) const
    {
        const Fr8 k = scalar_canonical(scalars + sig * sig_stride_words + (size_t)i * 8, montgomery);
        if (scalar_is_one(k)) {
            if (!first) return;
            if (MASKED && ones_as_mask) atomicOr(&ones_list[sig * n + (i >> 5)], 1u << (i & 31));
            else ones_list[sig * n + atomicAdd(&ones_count[sig], 1u)] = i;
            return;
        }
        int d[W];
        signed_digits<C, W>(k, d);
#pragma unroll
        for (int j = 0; j < W; j++)
            if (d[j]) fn(d[j], (uint32_t)j * n + i);
    }
};
typedef TableDigits<MSM_C, MSM_W, false> DenseTableDigits;
typedef TableDigits<NMSM_C, NMSM_W, true> NarrowTableDigits;
// A dense bare handle: grid row = window, its stored digit of scalar i, entry id = the point i.  No scalar is told apart as one.
struct StoredDigits {
    static constexpr int BUCKETS = MSM_BUCKETS, PER_ROW = 1;
    const int16_t *digits;
    template <class Fn> __device__ __forceinline__ void each(size_t row, uint32_t n, uint32_t i, bool, Fn fn) const
    {
        const int v = msm_digit_load(digits, row * n + i);
        if (v) fn(v, i);
    }
};
template <class Src>
__global__ __launch_bounds__(1024) void msm_sort_hist_kernel(uint32_t n, const Src src, uint32_t *__restrict__ slice_hist /* [row][slice][buckets] */)
{
    __shared__ uint32_t hist[Src::BUCKETS];
    const size_t row = blockIdx.y;
    const SliceRange s = slice_range(n);
    for (int b = threadIdx.x; b < Src::BUCKETS; b += 1024) hist[b] = 0;
    __syncthreads();
    for (uint32_t i = s.lo + threadIdx.x; i < s.hi; i += 1024)
        src.each(row, n, i, true, [&](int v, uint32_t) { atomicAdd(&hist[digit_bucket(v)], 1u); });
    __syncthreads();
    uint32_t *out = slice_hist + (row * gridDim.x + blockIdx.x) * Src::BUCKETS;
    for (int b = threadIdx.x; b < Src::BUCKETS; b += 1024) out[b] = hist[b];
}
template <class Src>
__global__ __launch_bounds__(1024) void msm_sort_scatter_kernel(uint32_t n, const Src src, const uint32_t *__restrict__ offsets,
                                                                const uint32_t *__restrict__ slice_hist, uint32_t *__restrict__ entries)
{
    __shared__ uint32_t cursor[Src::BUCKETS];
    const size_t row = blockIdx.y;
    const SliceRange s = slice_range(n);
    const uint32_t *first = slice_hist + (row * gridDim.x + blockIdx.x) * Src::BUCKETS, *off = offsets + row * Src::BUCKETS;
    for (int b = threadIdx.x; b < Src::BUCKETS; b += 1024) cursor[b] = off[b] + first[b];
    __syncthreads();
    uint32_t *ent = entries + row * (size_t)Src::PER_ROW * n;
    for (uint32_t i = s.lo + threadIdx.x; i < s.hi; i += 1024)
        src.each(row, n, i, false, [&](int v, uint32_t id) { ent[atomicAdd(&cursor[digit_bucket(v)], 1u)] = digit_entry(id, v); });
}

// ---- WIDE windows for the largest bare sums (round 5) -------------------------------------------------------------------------------
// A bare handle's windows cost no table, so their width is free: thirteen 20-bit windows instead of sixteen 16-bit ones are 19 % fewer
// bucket additions (one per point and non-zero digit: 13 n instead of 16 n) -- what the 2^27-point sum over h_query of the 1,024-statement
// aggregate spends 350 of its 430 ms on.  2^19 buckets per window do not fit the LDS histograms of the counting sort above; they need not:
// bucket m = |d| - 1 of window j is bucket (m mod 2^15) of ROW j 16 + (m >> 15), and a row is to every kernel from the fine sort on what a
// window (or a signature) was -- 32,768 buckets, work items, combine, the two-stage fold -- 208 rows of them.  The sort is in two levels
// (below: bins of 1,024 buckets, then the buckets of a bin), every pass writing runs.  A row's buckets fold to S1 = sum (lo + 1) B_lo AND
// S0 = sum B_lo; a window is sum_hi S1_hi + 2^15 sum_hi hi S0_hi (msm_wide_window_kernel), the windows join by Horner's rule with 20
// doublings each.  The folds of 13 x 2^19 buckets are a fixed 14 ms, three windows' additions 0.18 ns a point: handles of 2^26 points and
// more take wide windows by themselves (MSM_WIDE_FROM_DEFAULT), smaller ones when loaded so.
// The sort, every pass writing RUNS (the first version of it scattered 4-byte entries into 208 x 32,768 open cache lines: each such write a
// read-modify-write of a line in HBM, 76 ms for 1.7 x 10^9 of them -- all that three windows' additions saved):
//   digits     int32[13][n], written once
//   bins       per window, its points by bin = m >> 10 (512 bins): a workgroup sorts a TILE of 4,096 entries by bin in LDS and copies the
//              runs out (a bin's run of a tile to consecutive addresses: 8 entries = 64 bytes on average, whole lines)
//   buckets    per bin (262,000 entries of 1,024 buckets: one workgroup, 4 KB of counters): the 4-byte entries of a bin go into a 1 MB region
//              whose 1,024 open lines stay in the L2
// A row's thirty-two bins lie one after the other, so rows and bins share one numbering: bin g = row (g >> 5), buckets [1,024 (g & 31), ..).
static_assert(WIDE_BIN_BUCKETS == 1024 && WIDE_ALL_BINS == WIDE_ROWS * 32, "a row = 32 bins of 1,024 buckets");
__global__ __launch_bounds__(256) void msm_wide_digits_kernel(uint32_t n, const uint32_t *__restrict__ scalars, int montgomery, int32_t *__restrict__ digits)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int d[WIDE_W];
    signed_digits<WIDE_C, WIDE_W>(scalar_canonical(scalars + (size_t)i * 8, montgomery), d);     // (the top window: bits 240 ..)
#pragma unroll
    for (int j = 0; j < WIDE_W; j++) digits[(size_t)j * n + i] = d[j];
}
__global__ __launch_bounds__(1024) void msm_wide_bin_hist_kernel(uint32_t n, const int32_t *__restrict__ digits, uint32_t *__restrict__ slice_hist /* [window][slice][512] */)
{
    __shared__ uint32_t hist[WIDE_BINS];
    const size_t j = blockIdx.y;
    const SliceRange s = slice_range(n, WIDE_TILE);
    if (threadIdx.x < WIDE_BINS) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = s.lo + threadIdx.x; i < s.hi; i += 1024) {
        const int v = digits[j * n + i];
        if (v) atomicAdd(&hist[digit_bucket(v) >> 10], 1u);
    }
    __syncthreads();
    if (threadIdx.x < WIDE_BINS) slice_hist[(j * gridDim.x + blockIdx.x) * WIDE_BINS + threadIdx.x] = hist[threadIdx.x];
}
// every slice's first position inside its bins; the bins' sizes and starts; the rows' (one workgroup)
__global__ __launch_bounds__(1024) void msm_wide_bin_offsets_kernel(uint32_t slices, uint32_t *__restrict__ slice_hist, uint32_t *__restrict__ bin_count,
                                                                    unsigned long long *__restrict__ bin_start, uint32_t *__restrict__ row_count,
                                                                    unsigned long long *__restrict__ row_start)
{
    for (uint32_t g = threadIdx.x; g < (uint32_t)WIDE_ALL_BINS; g += 1024) {
        const uint32_t j = g / WIDE_BINS, bin = g % WIDE_BINS;
        uint32_t run = 0;
        for (uint32_t s_ = 0; s_ < slices; s_++) {
            uint32_t *h = slice_hist + ((size_t)j * slices + s_) * WIDE_BINS + bin;
            const uint32_t c = *h;
            *h = run;
            run += c;
        }
        bin_count[g] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long at = 0;
        for (int g = 0; g < WIDE_ALL_BINS; g++) { bin_start[g] = at; at += bin_count[g]; }
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)WIDE_ROWS) {
        const uint32_t r = threadIdx.x;
        uint32_t c = 0;
        for (int k = 0; k < 32; k++) c += bin_count[r * 32 + k];
        row_count[r] = c;
        row_start[r] = bin_start[r * 32];
    }
}
__global__ __launch_bounds__(1024) void msm_wide_bin_scatter_kernel(uint32_t n, const int32_t *__restrict__ digits, const uint32_t *__restrict__ slice_hist,
                                                                    const unsigned long long *__restrict__ bin_start,
                                                                    uint2 *__restrict__ coarse /* point | sign << 31, bucket of the bin */)
{
    __shared__ uint2 stage[WIDE_TILE];
    __shared__ uint16_t sbin[WIDE_TILE];
    __shared__ uint32_t tcount[WIDE_BINS], tstart[WIDE_BINS], tfill[WIDE_BINS], wtotal[WIDE_BINS / 64];
    __shared__ unsigned long long gpos[WIDE_BINS];
    const size_t j = blockIdx.y;
    const uint32_t t = threadIdx.x;
    const SliceRange s = slice_range(n, WIDE_TILE);
    const uint32_t hi = s.hi;
    if (t < WIDE_BINS) gpos[t] = bin_start[j * WIDE_BINS + t] + slice_hist[(j * gridDim.x + blockIdx.x) * WIDE_BINS + t];
    for (uint32_t tile0 = s.lo; tile0 < hi; tile0 += WIDE_TILE) {
        if (t < WIDE_BINS) { tcount[t] = 0; tfill[t] = 0; }
        __syncthreads();
        int dv[WIDE_TILE / 1024];
#pragma unroll
        for (int k = 0; k < WIDE_TILE / 1024; k++) {
            const uint32_t i = tile0 + t + 1024u * k;
            dv[k] = i < hi ? digits[j * n + i] : 0;
            if (dv[k]) atomicAdd(&tcount[digit_bucket(dv[k]) >> 10], 1u);
        }
        __syncthreads();
        // exclusive prefix sums of the 512 counts: within each of the first eight wavefronts by shuffles, their totals through LDS (two
        // barriers; a scan of nine steps through LDS was eighteen, most of this kernel's waiting)
        {
            uint32_t incl = t < WIDE_BINS ? tcount[t] : 0u;
            const uint32_t own = incl, lane = t & 63;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t v = __shfl_up(incl, off, 64);
                if (lane >= (uint32_t)off) incl += v;
            }
            if (t < WIDE_BINS && lane == 63) wtotal[t >> 6] = incl;
            __syncthreads();
            if (t < WIDE_BINS) {
                uint32_t before = 0;
                for (uint32_t w_ = 0; w_ < (t >> 6); w_++) before += wtotal[w_];
                tstart[t] = before + incl - own;
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < WIDE_TILE / 1024; k++) {
            if (!dv[k]) continue;
            const uint32_t i = tile0 + t + 1024u * k, m = digit_bucket(dv[k]), bin = m >> 10;
            const uint32_t pos = tstart[bin] + atomicAdd(&tfill[bin], 1u);
            stage[pos] = make_uint2(digit_entry(i, dv[k]), m & (WIDE_BIN_BUCKETS - 1));
            sbin[pos] = (uint16_t)bin;
        }
        __syncthreads();
        const uint32_t total = tstart[WIDE_BINS - 1] + tcount[WIDE_BINS - 1];
        for (uint32_t p = t; p < total; p += 1024) {
            const uint32_t bin = sbin[p];
            coarse[gpos[bin] + (p - tstart[bin])] = stage[p];
        }
        __syncthreads();
        if (t < WIDE_BINS) gpos[t] += tcount[t];
        __syncthreads();
    }
}
// The buckets' sort: a bin's 4-byte entries go into its 1 MB of the entry array, 1,024 lines open at a time -- and with a workgroup per
// bin, 512 bins in flight, those 512 MB of open lines left the L2 one dirty word at a time (33 ms: 77 bytes of HBM traffic per entry; with
// cursors in global memory shared by the workgroups of a bin, 107 ms: device-wide atomics).  So a bin is cut into WIDE_PARTS parts by entry,
// one workgroup each with its cursors in LDS (a part's own first positions come from the parts' histograms), and the parts of a bin run on
// the SAME XCD at the same time (workgroups go to the XCDs round robin, w % 8): two bins in flight per XCD, their lines complete before
// they leave its L2.  The order inside a bucket is what the LDS atomics make it within a part; parts in order.
static_assert(WIDE_ALL_BINS % 8 == 0, "bins go to the XCDs eight at a time");
struct WidePart { size_t g; uint32_t part, lo, hi; };
__device__ __forceinline__ WidePart wide_part_of(uint32_t w, const uint32_t *__restrict__ bin_count)
{
    WidePart p;
    const uint32_t q = w >> 3;
    p.part = q % WIDE_PARTS;
    p.g = (size_t)(q / WIDE_PARTS) * 8 + (w & 7);
    const uint32_t cnt = bin_count[p.g];
    p.lo = (uint32_t)((uint64_t)cnt * p.part / WIDE_PARTS);
    p.hi = (uint32_t)((uint64_t)cnt * (p.part + 1) / WIDE_PARTS);
    return p;
}
// the sizes of the 1,024 buckets within every part (grid: bins x parts)
__global__ __launch_bounds__(1024) void msm_wide_bucket_hist_kernel(const uint2 *__restrict__ coarse, const uint32_t *__restrict__ bin_count,
                                                                    const unsigned long long *__restrict__ bin_start, uint32_t *__restrict__ part_hist)
{
    __shared__ uint32_t hist[WIDE_BIN_BUCKETS];
    const WidePart p = wide_part_of(blockIdx.x, bin_count);
    const uint2 *src = coarse + bin_start[p.g];
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = p.lo + threadIdx.x; i < p.hi; i += 1024) atomicAdd(&hist[src[i].y], 1u);
    __syncthreads();
    part_hist[(p.g * WIDE_PARTS + p.part) * WIDE_BIN_BUCKETS + threadIdx.x] = hist[threadIdx.x];
}
// per bin: a part's first position within each bucket, and the buckets' sizes straight into the rows' count arrays (grid: the 6,656 bins)
__global__ __launch_bounds__(1024) void msm_wide_bucket_parts_kernel(uint32_t *__restrict__ part_hist, uint32_t *__restrict__ counts)
{
    const size_t g = blockIdx.x;
    uint32_t run = 0;
    for (int part = 0; part < WIDE_PARTS; part++) {
        uint32_t *h = part_hist + (g * WIDE_PARTS + part) * WIDE_BIN_BUCKETS + threadIdx.x;
        const uint32_t c = *h;
        *h = run;
        run += c;
    }
    counts[g * WIDE_BIN_BUCKETS + threadIdx.x] = run;
}
__global__ __launch_bounds__(1024) void msm_wide_bucket_scatter_kernel(const uint2 *__restrict__ coarse, const uint32_t *__restrict__ bin_count,
                                                                       const unsigned long long *__restrict__ bin_start, const uint32_t *__restrict__ offsets,
                                                                       const uint32_t *__restrict__ part_hist, const unsigned long long *__restrict__ row_start,
                                                                       uint32_t *__restrict__ entries)
{
    __shared__ uint32_t cursor[WIDE_BIN_BUCKETS];
    const WidePart p = wide_part_of(blockIdx.x, bin_count);
    const uint2 *src = coarse + bin_start[p.g];
    // (relative to the row: offsets are [row][32,768] = [bin][1,024])
    cursor[threadIdx.x] = offsets[p.g * WIDE_BIN_BUCKETS + threadIdx.x] + part_hist[(p.g * WIDE_PARTS + p.part) * WIDE_BIN_BUCKETS + threadIdx.x];
    __syncthreads();
    uint32_t *ent = entries + row_start[p.g >> 5];
    // (a part is some 8,000 entries, eight a thread: all its loads first -- one memory latency for the workgroup instead of eight in a row,
    // 213,000 workgroups long: 15.8 -> ms of this kernel were those)
    constexpr int U = 8;
    for (uint32_t i0 = p.lo + threadIdx.x; i0 < p.hi; i0 += 1024 * U) {
        uint2 e[U];
#pragma unroll
        for (int k = 0; k < U; k++) e[k] = i0 + 1024u * k < p.hi ? src[i0 + 1024u * k] : make_uint2(0u, 0u);
#pragma unroll
        for (int k = 0; k < U; k++)
            if (i0 + 1024u * k < p.hi) ent[atomicAdd(&cursor[e[k].y], 1u)] = e[k].x;
    }
}
// window j = sum_hi S1(j, hi) + 2^15 sum_hi hi S0(j, hi): one lane per window (F::LANES lanes)
template <class F>
__global__ __launch_bounds__(64) void msm_wide_window_kernel(const uint32_t *__restrict__ s1 /* [208][BK_WORDS] */, const uint32_t *__restrict__ s0,
                                                             uint32_t *__restrict__ window_sums /* [13][BK_WORDS] */)
{
    __builtin_amdgcn_s_setprio(2);
    constexpr int BW = Grp<F>::BK_WORDS;
    if (threadIdx.x >= (unsigned)F::LANES) return;
    const size_t j = blockIdx.x;
    XyzzT<F> run = pt_identity<F>(), weighted = pt_identity<F>(), plain = load_bucket<F>(s1 + (j * WIDE_H) * BW);
    for (int hi = WIDE_H - 1; hi >= 1; hi--) {
        run = pt_add(run, load_bucket<F>(s0 + (j * WIDE_H + hi) * BW));
        weighted = pt_add(weighted, run);                            // sum_(hi >= 1) hi S0_hi
        plain = pt_add(plain, load_bucket<F>(s1 + (j * WIDE_H + hi) * BW));
    }
    for (int k = 0; k < MSM_C - 1; k++) weighted = pt_double(weighted);
    store_bucket<F>(window_sums + j * BW, pt_add(plain, weighted));
}

// per bucket: its size (counts) and, in place of every slice's count, the slice's first position inside the bucket
__global__ __launch_bounds__(256) void msm_slice_offsets_kernel(uint32_t *__restrict__ slice_hist, uint32_t *__restrict__ counts, int slices)
{
    const size_t sig = blockIdx.y;
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    uint32_t *h = slice_hist + sig * slices * (size_t)MSM_BUCKETS + b;
    uint32_t run = 0;
#pragma unroll 4
    for (int s_ = 0; s_ < slices; s_++) {
        const uint32_t c = h[(size_t)s_ * MSM_BUCKETS];
        h[(size_t)s_ * MSM_BUCKETS] = run;
        run += c;
    }
    counts[sig * MSM_BUCKETS + b] = run;
}

// exclusive prefix sums of a signature's 32,768 bucket sizes: where each bucket's entries start
__global__ __launch_bounds__(1024) void msm_scan_kernel(const uint32_t *__restrict__ counts, uint32_t *__restrict__ offsets)
{
    __shared__ uint32_t part[1024];
    const size_t sig = blockIdx.x;
    const uint32_t *cnt = counts + sig * MSM_BUCKETS;
    const int t = threadIdx.x;
    constexpr int PER = MSM_BUCKETS / 1024;
    uint32_t local[PER], s = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { local[k] = s; s += cnt[t * PER + k]; }
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const uint32_t base = part[t] - s;
#pragma unroll
    for (int k = 0; k < PER; k++) offsets[sig * MSM_BUCKETS + t * PER + k] = base + local[k];
}

// Work items.  A bucket is added up by one thread, so a bucket far above the mean is a serial chain the whole call waits for:
// a Falcon witness as scalars leaves 35,000 pairs in all, 775 of them in the bucket of digit +-1 (carries of the recoding),
// and a lone wavefront needs ~18 us per addition.  Buckets are therefore cut into ITEMS of at most `split` entries, equal
// parts of their bucket, with split = max(32, 1.5 x the mean bucket size) decided per call on the device: the 2^18-point sum
// of h (mean 128, sigma 11) is not cut at all, the witness-side sums are cut at 32.  Items are laid out by decreasing bucket
// size (a counting sort), so the 64 lanes of a wavefront run equally long; a bucket's items are neighbours, and
// msm_combine_kernel adds them up.  At most 32,768 + 21,845 items whatever the scalars (sum of ceil(c_b / split)).
constexpr int MSM_SIZE_CLASSES = 1024;         // sizes >= this share the first class
// Sums over more than 2^18 points (an aggregate statement's h_query: ONE signature, 2^22 points, buckets of 2,048 entries) are cut
// finer still: `finer` = 24 makes a bucket of the mean size 16 items of 128 entries -- 524,288 items, four rounds of the chip's
// 131,072 thread slots at two wavefronts per SIMD (with 4 it was 98,304 items: a quarter of the slots idle and half the SIMDs with a
// single wavefront, 1.55 x the time per addition of a 64-signature call: 16.7 ms; with 12, two rounds: 14.4 ms; with 24: 13.4 ms, the
// combine's extra additions included).  Bound: 32,768 + 32,768 finer / 1.5.
// (msm_split_of rounds the split DOWN, by less than one entry in at least 32: 33 / 32 of that bound is what the list must hold; an item is
// two words, bucket and part -- packed into one, `part << 15` overflowed for a bucket cut into more than 2^17 parts, which one digit repeated
// in all the scalars of a 2^22-point sum produces: round 4's ADVICE)
// `finer`: 1 for a batch, 4 for one or two signatures at a time -- a bucket of the mean size is then three items instead of one
// (a lone proof waits for ~128 dependent additions otherwise), and msm_combine_kernel adds them up
__device__ __forceinline__ uint32_t msm_split_of(uint32_t total, uint32_t finer)
{
    const uint32_t s = (uint32_t)(((uint64_t)total * 3 + 2 * MSM_BUCKETS - 1) / (2 * MSM_BUCKETS)) / finer;
    return s < 32u ? 32u : s;
}
// a row's entries in all (the last bucket's start and size), and how many items a bucket of c entries becomes: equal parts of at most `split`
__device__ __forceinline__ uint32_t row_total(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ counts, size_t row, int buckets)
{
    return offsets[row * buckets + buckets - 1] + counts[row * buckets + buckets - 1];
}
__device__ __forceinline__ uint32_t items_of(uint32_t c, uint32_t split) { return c <= split ? 1u : (c + split - 1) / split; }
__global__ __launch_bounds__(1024) void msm_order_kernel(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                         uint32_t *__restrict__ order, uint32_t *__restrict__ item_first /* [sig][buckets] */,
                                                         uint32_t *__restrict__ items /* [sig][max_items][2]: bucket, part */,
                                                         uint32_t *__restrict__ item_count /* [sig] */, uint32_t finer, uint32_t max_items)
{
    __shared__ uint32_t hist[MSM_SIZE_CLASSES];
    const size_t sig = blockIdx.x;
    const uint32_t *cnt = counts + sig * MSM_BUCKETS;
    uint32_t *ord = order + sig * MSM_BUCKETS;
    const int t = threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    auto cls = [](uint32_t c) { return c >= (uint32_t)MSM_SIZE_CLASSES ? 0u : (uint32_t)(MSM_SIZE_CLASSES - 1) - c; };   // big first
    for (int b = t; b < MSM_BUCKETS; b += 1024) atomicAdd(&hist[cls(cnt[b])], 1u);
    __syncthreads();
    // exclusive scan of the 1,024 class counts
    const uint32_t mine = hist[t];
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? hist[t - off] : 0u;
        __syncthreads();
        hist[t] += v;
        __syncthreads();
    }
    const uint32_t excl = hist[t] - mine;
    __syncthreads();
    hist[t] = excl;
    __syncthreads();
    for (int b = t; b < MSM_BUCKETS; b += 1024) ord[atomicAdd(&hist[cls(cnt[b])], 1u)] = (uint32_t)b;
    __threadfence_block();
    __syncthreads();
    // items: rank by rank, ceil(c / split) each (an empty bucket keeps one: its thread stores the identity)
    const uint32_t split = msm_split_of(row_total(offsets, counts, sig, MSM_BUCKETS), finer);
    constexpr int PER = MSM_BUCKETS / 1024;
    uint32_t k[PER], local = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const uint32_t c = cnt[ord[t * PER + j]];
        k[j] = items_of(c, split);
        local += k[j];
    }
    hist[t] = local;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? hist[t - off] : 0u;
        __syncthreads();
        hist[t] += v;
        __syncthreads();
    }
    uint32_t pos = hist[t] - local;
    if (t == 1023) item_count[sig] = hist[t] < max_items ? hist[t] : max_items;     // (the bound above holds; a list is never overrun if it did not)
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const uint32_t b = ord[t * PER + j];
        item_first[sig * MSM_BUCKETS + b] = pos;
        for (uint32_t c = 0; c < k[j] && pos + c < max_items; c++) {
            uint32_t *it = items + (sig * (size_t)max_items + pos + c) * 2;
            it[0] = b;
            it[1] = c;
        }
        pos += k[j];
    }
}

// one thread per (signature, item): the sum of the item's table rows, in registers.  G1: the row of entry k + 1 is fetched
// while entry k is added (an addition is ~5,000 vector instructions: the gather of 112 bytes hides behind it); G2 has no
// registers to spare for that (an accumulator alone is 112).
template <class F, bool PREFETCH>
__global__ __launch_bounds__(64, 2) void msm_bucket_kernel(MsmDev m, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ counts,
                                                           const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
                                                           const uint32_t *__restrict__ entries, uint32_t *__restrict__ partial_items, uint32_t finer,
                                                           uint32_t max_items, size_t ent_stride /* entries per row: 16 n, a bare handle's: n */,
                                                           const unsigned long long *__restrict__ row_base /* wide windows: where each row's entries start; else null */)
{
    constexpr int PW = Grp<F>::PT_WORDS;
    const size_t sig = blockIdx.y;
    const uint32_t it = blockIdx.x * 64 + threadIdx.x;
    if (it >= item_count[sig]) return;
    const uint2 item = *(const uint2 *)(items + (sig * (size_t)max_items + it) * 2);
    const uint32_t b = item.x, chunk = item.y;
    const uint32_t c = counts[sig * MSM_BUCKETS + b];
    const uint32_t k = items_of(c, msm_split_of(row_total(offsets, counts, sig, MSM_BUCKETS), finer));
    const uint32_t lo = (uint32_t)((uint64_t)c * chunk / k), cnt = (uint32_t)((uint64_t)c * (chunk + 1) / k) - lo;     // equal parts
    const uint32_t *ent = entries + (row_base ? (size_t)row_base[sig] : sig * ent_stride) + offsets[sig * MSM_BUCKETS + b] + lo;
    XyzzT<F> acc = pt_identity<F>();
    if (PREFETCH) {
        uint32_t e = cnt ? ent[0] : 0u;
        AffineT<F> p = load_row<F>(m.table + (size_t)(e & 0x7fffffffu) * PW);
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t e_next = j + 1 < cnt ? ent[j + 1] : e;
            const AffineT<F> p_next = load_row<F>(m.table + (size_t)(e_next & 0x7fffffffu) * PW);
            if (e >> 31) p.y = F::template neg<Grp<F>::K_AFFINE_Y>(p.y);
            acc = pt_add_affine(acc, p);
            e = e_next;
            p = p_next;
        }
    } else {
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t e = ent[j];
            AffineT<F> p = load_row<F>(m.table + (size_t)(e & 0x7fffffffu) * PW);
            if (e >> 31) p.y = F::template neg<Grp<F>::K_AFFINE_Y>(p.y);
            acc = pt_add_affine(acc, p);
        }
    }
    store_bucket<F>(partial_items + (sig * (size_t)max_items + it) * (size_t)Grp<F>::BK_WORDS, acc);
}

// sum_j 2^(window_bits j) S_j for the window sums S_j of a bare handle (Horner: window_bits doublings and one addition per window:
// 255 point operations of ONE chain -- F::LANES lanes -- whatever the size of the sum: 5 ms beside the 10^9 additions it crowns).
// Grid: one workgroup per sum (the three G1 tables of a proof side by side); sums: [sum][windows][BK_WORDS].
template <class F>
__global__ __launch_bounds__(64) void msm_horner_kernel(const uint32_t *__restrict__ sums, int windows, int window_bits,
                                                        uint32_t *__restrict__ out /* [sum][ARK_WORDS], or [sum][BK_WORDS] */, int xyzz_out,
                                                        uint32_t out_step = 1 /* XYZZ rows: sum i goes to row i out_step */)
{
    __builtin_amdgcn_s_setprio(2);
    constexpr int BW = Grp<F>::BK_WORDS;
    if (threadIdx.x >= (unsigned)F::LANES) return;
    const uint32_t *src = sums + (size_t)blockIdx.x * windows * BW;
    XyzzT<F> acc = load_bucket<F>(src + (size_t)(windows - 1) * BW);
    for (int j = windows - 2; j >= 0; j--) {
        for (int k = 0; k < window_bits; k++) acc = pt_double(acc);
        acc = pt_add(acc, load_bucket<F>(src + (size_t)j * BW));
    }
    if (xyzz_out) store_bucket<F>(out + (size_t)blockIdx.x * out_step * BW, acc);
    else store_ark_point<F>(out + (size_t)blockIdx.x * Grp<F>::ARK_WORDS, pt_to_affine(acc));
}
// the rows of a table that hold a point (not all words zero), in order: per block of 1,024 rows their number, then -- the blocks' running
// totals in between, one workgroup -- their indices
template <int PT_WORDS_>
__global__ __launch_bounds__(1024) void live_rows_kernel(const uint32_t *__restrict__ rows, uint32_t n, uint32_t *__restrict__ block_counts /* in: null or the blocks' first positions */,
                                                         uint32_t *__restrict__ index /* null: count only */)
{
    __shared__ uint32_t wave_total[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t any = 0;
    if (i < n) {
        const uint4 *v = (const uint4 *)(rows + (size_t)i * PT_WORDS_);
#pragma unroll
        for (int k = 0; k < PT_WORDS_ / 4; k++) { const uint4 w = v[k]; any |= w.x | w.y | w.z | w.w; }
    }
    const unsigned long long ballot = __builtin_amdgcn_ballot_w64(any != 0);
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < 16; w++) { before += w < wave ? wave_total[w] : 0u; total += wave_total[w]; }
    if (!index) {
        if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
        return;
    }
    if (any) index[block_counts[blockIdx.x] + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1))] = i;
}
__global__ __launch_bounds__(1024) void live_rows_scan_kernel(uint32_t *__restrict__ block_counts, uint32_t blocks, uint32_t *__restrict__ total)
{
    // one workgroup: every thread a run of blocks, the runs' totals scanned through LDS
    __shared__ uint32_t run_total[1024];
    const uint32_t per = (blocks + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < blocks ? lo + per : blocks;
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; b++) sum += block_counts[b];
    run_total[threadIdx.x] = sum;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t t = 0; t < threadIdx.x; t++) before += run_total[t];
    for (uint32_t b = lo; b < hi; b++) { const uint32_t c = block_counts[b]; block_counts[b] = before; before += c; }
    if (threadIdx.x == 1023) *total = before;
}

// bucket b = the sum of its items (one for almost every bucket: a copy)
template <class F>
__global__ __launch_bounds__(64, 2) void msm_combine_kernel(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ counts,
                                                            const uint32_t *__restrict__ item_first, const uint32_t *__restrict__ partial_items,
                                                            uint32_t *__restrict__ buckets, uint32_t finer, uint32_t max_items)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int BW = Grp<F>::BK_WORDS;
    const size_t sig = blockIdx.y;
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    const uint32_t c = counts[sig * MSM_BUCKETS + b];
    const uint32_t k = items_of(c, msm_split_of(row_total(offsets, counts, sig, MSM_BUCKETS), finer));
    const uint32_t *src = partial_items + (sig * (size_t)max_items + item_first[sig * MSM_BUCKETS + b]) * (size_t)BW;
    XyzzT<F> acc = load_bucket<F>(src);
    for (uint32_t j = 1; j < k; j++) acc = pt_add(acc, load_bucket<F>(src + (size_t)j * BW));
    store_bucket<F>(buckets + (sig * MSM_BUCKETS + b) * (size_t)BW, acc);
}

// the points whose scalar is one, summed by the threads of the fold's first stage (thread t: every nthreads-th of the list); the
// partial sums enter the fold with weight one
template <class F>
__global__ __launch_bounds__(64, 2) void msm_ones_kernel(MsmDev m, const uint32_t *__restrict__ ones_count, const uint32_t *__restrict__ ones_list,
                                                         uint32_t *__restrict__ partial /* [sig][MSM_FOLD1_THREADS][BK_WORDS] */)
{
    const size_t sig = blockIdx.y;
    const uint32_t nthreads = gridDim.x * 64;
    const uint32_t t = blockIdx.x * 64 + threadIdx.x, cnt = ones_count[sig];
    const uint32_t *list = ones_list + sig * m.n;
    XyzzT<F> acc = pt_identity<F>();
    for (uint32_t k = t; k < cnt; k += nthreads)
        acc = pt_add_affine(acc, load_row<F>(m.table + (size_t)list[k] * Grp<F>::PT_WORDS));      // window 0 of the table = the point itself
    store_bucket<F>(partial + (sig * MSM_FOLD1_THREADS + t) * (size_t)Grp<F>::BK_WORDS, acc);
}

// sum_b (b + 1) B_b per signature, in two stages (one workgroup of 512 threads x 64 buckets each was 200 dependent point
// operations long: 6 ms for G1, 19 for G2, whatever the batch).  Stage 1: 32,768 / CHUNK threads x CHUNK buckets: running sums,
// the multiple CHUNK g x (sum of the chunk) by double-and-add, plus the thread's share of the scalars that are one; overwrites
// `partial`.  CHUNK = 2^LOG_CHUNK is 8 for small batches (latency) and up to 64 for large ones (the multiples are a third of the
// work at 8).
template <class F, int LOG_CHUNK>
__global__ __launch_bounds__(64, 2) void msm_fold1_kernel(const uint32_t *__restrict__ buckets, uint32_t *__restrict__ partial,
                                                          uint32_t *__restrict__ partial_plain /* wide windows: the chunk's UNWEIGHTED sum too; else null */)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int BW = Grp<F>::BK_WORDS, CHUNK = 1 << LOG_CHUNK;
    const size_t sig = blockIdx.y;
    const int g = blockIdx.x * 64 + threadIdx.x;
    const uint32_t *bk = buckets + (sig * MSM_BUCKETS + (size_t)g * CHUNK) * BW;
    XyzzT<F> run = pt_identity<F>(), sum = pt_identity<F>();
    for (int k = CHUNK - 1; k >= 0; k--) {
        run = pt_add(run, load_bucket<F>(bk + (size_t)k * BW));
        sum = pt_add(sum, run);
    }
    // sum = sum_k (k + 1) B_(CHUNK g + k); the buckets' weights are CHUNK g + k + 1: add (CHUNK g) run = 2^LOG_CHUNK (g run)
    XyzzT<F> mult = pt_identity<F>();
    for (int bit = 14 - LOG_CHUNK; bit >= 0; bit--) {
        mult = pt_double(mult);
        if ((g >> bit) & 1) mult = pt_add(mult, run);
    }
    for (int k = 0; k < LOG_CHUNK; k++) mult = pt_double(mult);
    sum = pt_add(sum, mult);
    uint32_t *mine = partial + (sig * MSM_FOLD1_THREADS + g) * (size_t)BW;
    sum = pt_add(sum, load_bucket<F>(mine));                           // the scalars that are one
    store_bucket<F>(mine, sum);
    if (partial_plain) store_bucket<F>(partial_plain + (sig * MSM_FOLD1_THREADS + g) * (size_t)BW, run);
}
// Stage 2: 512 threads add `each` partial sums each, a tree through LDS, one inversion, ark-ff's bytes out
template <class F>
__global__ __launch_bounds__(MSM_FOLD_THREADS) void msm_fold2_kernel(const uint32_t *__restrict__ partial, int each,
                                                                     uint32_t *__restrict__ out /* [batch][ARK_WORDS], or [batch][BK_WORDS] */, int xyzz_out)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int SLOT = 4 * F::WORDS + 1, BW = Grp<F>::BK_WORDS;
    __shared__ uint32_t lds[MSM_FOLD_THREADS / 2 * SLOT];            // 58 KB (G1) / 116 KB (G2): the upper half of a tree level parks here
    const size_t sig = blockIdx.x;
    const int t = threadIdx.x;
    const uint32_t *src = partial + (sig * MSM_FOLD1_THREADS + (size_t)t * each) * BW;
    XyzzT<F> sum = load_bucket<F>(src);
    for (int k = 1; k < each; k++) sum = pt_add(sum, load_bucket<F>(src + (size_t)k * BW));
    for (int stride = MSM_FOLD_THREADS / 2; stride >= 1; stride >>= 1) {
        if (t >= stride && t < 2 * stride) store_bucket<F>(lds + (t - stride) * SLOT, sum);
        __syncthreads();
        if (t < stride) sum = pt_add(sum, load_bucket<F>(lds + t * SLOT));
        __syncthreads();
    }
    // xyzz_out: the sum as it stands, no inversion -- for a caller that goes on adding (frw_groth16_prove_dev)
    if (t == 0) {
        if (xyzz_out) store_bucket<F>(out + sig * BW, sum);
        else store_ark_point<F>(out + sig * Grp<F>::ARK_WORDS, pt_to_affine(sum));
    }
}

// (launch bounds of the narrow kernels: two waves per SIMD for G1; the two-lane G2 policy is written for ONE -- its mixed addition holds an
// accumulator, a row, the neighbour's copies of both operands of a product and 28 64-bit columns: 256 registers and then some, which at a
// bound of two went to AGPR moves and scratch under a warning that the target was missed.  Said so, the compiler may use the AGPRs it has.)
// ---- narrow windows: the witness-side sums ---------------------------------------------------------------------------------------
// The sums over a_query, b_g1_query, b_g2_query and l_query take a WITNESS as scalars: 46 % zeros, 45 % ones, and of the rest
// all but two thousand values are below 2^16 (Falcon-1024: 13 N values that are not boolean, 2 N of them ~146 bits).  Through
// the 16-bit pipeline above such a sum is 35,000 additions into 32,768 buckets -- and then 65,536 full additions to fold mostly
// empty buckets, ten kernels of one wavefront per SIMD each: a third of a whole proof's time for a thirtieth of its
// arithmetic.  With 8-bit windows (32 of them: a table twice as long) the same scalars are 70,000 additions into 128 buckets
// per signature, cut into ~2,048 equal work items, and the fold is one workgroup: a suffix scan and a tree over 128 points.
// slices of the counting sort (a workgroup of 1,024 threads each): 16 per signature, 128 beyond 2^18 scalars (an aggregate statement is
// one "signature": 16 workgroups for 2.5 M scalars were 1.2 ms at the head of every other kernel of its proof)
// (1,024 slices for the 2^27-scalar sums were tried: the histogram no faster -- it waited for ONE global counter, that of the list of
// ones: see nmsm_hist_bare_kernel -- and the scatter three times slower: a slice's run inside a bucket is a 1,024th of it, and the entry array's lines left the L2 half written)
// Work items per signature: 2,048 for the per-signature circuits (n < 2^18 points), n / 128 rounded up to a multiple of 2,048 beyond
// (an aggregate statement is ONE "signature" with sixteen times the points: 2,048 items would be 32 wavefronts on 1,024 SIMDs, each
// a chain of 550 additions); items <= buckets + total / split <= 128 + target, rounded up to whole wavefronts.
// the scalars equal to one: 256 .. 4,096 threads per signature, by the batch, one partial sum per 64 of them (<= 64: one per thread of
// the fold); with more than 2^18 points up to 65,536 threads, whose <= 1,024 partial sums a small kernel brings down to 64 first
// threads of the one-workgroup fold: 128 for the buckets + 256 (G1) / 128 (G2: four waves = one per SIMD, the whole register file
// for an addition that needs 300 live registers) for the ones' partial sums
__device__ __forceinline__ uint32_t nmsm_split_of(uint32_t total, uint32_t target)
{
    const uint32_t s = (total + target - 1) / target;
    return s < 32u ? 32u : s;
}
// one workgroup of 128 threads per signature: bucket sizes and starts, every slice's first position inside its buckets, the
// work items (bucket | part << 8: equal parts of at most `split` entries)
__global__ __launch_bounds__(NMSM_BUCKETS) void nmsm_plan_kernel(uint32_t *__restrict__ slice_hist, uint32_t *__restrict__ counts, uint32_t *__restrict__ offsets,
                                                                 uint32_t *__restrict__ item_first, uint32_t *__restrict__ items /* [sig][max_items] */,
                                                                 uint32_t *__restrict__ item_count /* [sig] */, uint32_t target, uint32_t max_items, uint32_t slices)
{
    __shared__ uint32_t scan[NMSM_BUCKETS];
    const size_t sig = blockIdx.x;
    const int b = threadIdx.x;
    uint32_t *h = slice_hist + sig * slices * (size_t)NMSM_BUCKETS + b;
    uint32_t c = 0;
    for (uint32_t s_ = 0; s_ < slices; s_++) {
        const uint32_t v = h[(size_t)s_ * NMSM_BUCKETS];
        h[(size_t)s_ * NMSM_BUCKETS] = c;
        c += v;
    }
    auto inclusive_scan = [&](uint32_t mine) {
        scan[b] = mine;
        __syncthreads();
        for (int off = 1; off < NMSM_BUCKETS; off <<= 1) {
            const uint32_t v = b >= off ? scan[b - off] : 0u;
            __syncthreads();
            scan[b] += v;
            __syncthreads();
        }
        const uint32_t r = scan[b];
        __syncthreads();
        return r;
    };
    const uint32_t incl = inclusive_scan(c);
    scan[b] = incl;
    __syncthreads();
    const uint32_t total = scan[NMSM_BUCKETS - 1], split = nmsm_split_of(total, target);
    __syncthreads();
    counts[sig * NMSM_BUCKETS + b] = c;
    offsets[sig * NMSM_BUCKETS + b] = incl - c;
    const uint32_t k = items_of(c, split);
    const uint32_t kincl = inclusive_scan(k), first = kincl - k;
    item_first[sig * NMSM_BUCKETS + b] = first;
    if (b == NMSM_BUCKETS - 1) item_count[sig] = kincl;
    for (uint32_t part = 0; part < k; part++) items[sig * (size_t)max_items + first + part] = (uint32_t)b | (part << 8);
}
// ---- the narrow sums of a BARE handle (round 5: a key whose window tables would not fit; the points only) ------------------------------
// One scalar vector, thirty-two 8-bit windows: the counting sort is over (window, digit) -- 4,096 counters in 16 KB of LDS, ONE pass over
// the scalars for all the windows -- and from there on window w is what signature w is to the kernels above: its own 128 buckets, its own
// work items, its own fold; an entry is a point index (a table row: the tables have no other), a window's entries start at
// entry_base[w] (the windows' totals differ by orders of magnitude: the low two hold every 14-bit value of a witness, the upper
// thirteen nothing), and msm_horner_kernel puts the thirty-two window sums of every table together.  Scalars equal to one: a list,
// summed with window 0.
// `index` (or null): element k of the sum is scalar -- and table row -- index[k]: the rows of a table that are not the point at infinity
// (frw_groth16_pk.b_index: b_g1_query / b_g2_query hold a point for 59 % of the variables of a Falcon circuit, and of those variables'
// values half of a witness's ones and every full-size value are elsewhere: a third of the additions are left).
__global__ __launch_bounds__(1024) void nmsm_hist_bare_kernel(uint32_t n, const uint32_t *__restrict__ scalars, int montgomery,
                                                              uint32_t *__restrict__ slice_hist /* [window][slice][128] */,
                                                              uint32_t *__restrict__ ones_count /* [0] */, uint32_t *__restrict__ ones_list /* [n] */,
                                                              const uint32_t *__restrict__ index)
{
    // The scalars equal to one (55 % of a witness) go to ONE list with ONE counter: appended a wavefront at a time that was an atomic of
    // one address per wavefront and round of the loop -- 1.5 M of them in a row, 8 ns each: the whole 12 - 21 ms of this kernel, its waves
    // waiting 95 % of their cycles (SQ counters, tools/dev/pmc_sort.sh).  So a workgroup collects its ones in LDS (a counter there costs
    // nothing) and moves them out 3,072 at least at a time: one global atomic per flush, and the list is written in whole lines.
    constexpr uint32_t ONES_CAP = 4096;
    __shared__ uint32_t hist[NMSM_W * NMSM_BUCKETS];
    __shared__ uint32_t ones_buf[ONES_CAP];
    __shared__ uint32_t ones_fill, ones_base;
    const uint32_t slices = gridDim.x, slice = blockIdx.x;
    const SliceRange s = slice_range(n);
    const uint32_t hi = s.hi;
    for (int b = threadIdx.x; b < NMSM_W * NMSM_BUCKETS; b += 1024) hist[b] = 0;
    if (threadIdx.x == 0) ones_fill = 0;
    __syncthreads();
    auto flush = [&](uint32_t fill) {                                  // (every thread of the workgroup with the same `fill`; nobody appends meanwhile)
        if (threadIdx.x == 0 && fill) ones_base = atomicAdd(&ones_count[0], fill);
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < fill; t += 1024) ones_list[ones_base + t] = ones_buf[t];
        __syncthreads();
        if (threadIdx.x == 0) ones_fill = 0;
        __syncthreads();
    };
    for (uint32_t k0 = s.lo; k0 < hi; k0 += 1024) {                    // (the same number of rounds for every thread: barriers inside)
        const uint32_t k = k0 + threadIdx.x;
        bool one = false;
        if (k < hi) {
            const uint32_t i = index ? index[k] : k;
            const Fr8 sc = scalar_canonical(scalars + (size_t)i * 8, montgomery);
            one = scalar_is_one(sc);
            if (one) {
                ones_buf[atomicAdd(&ones_fill, 1u)] = i;               // (at most 1,024 a round, and a round starts with 3,072 free)
            } else {
                int d[NMSM_W];
                signed_digits<NMSM_C, NMSM_W>(sc, d);
#pragma unroll
                for (int j = 0; j < NMSM_W; j++)
                    if (d[j]) atomicAdd(&hist[j * NMSM_BUCKETS + digit_bucket(d[j])], 1u);
            }
        }
        __syncthreads();
        const uint32_t fill = ones_fill;                               // (read between two barriers: the same value in every thread)
        __syncthreads();
        if (fill > ONES_CAP - 1024) flush(fill);
    }
    flush(ones_fill);
    __syncthreads();
    for (int b = threadIdx.x; b < NMSM_W * NMSM_BUCKETS; b += 1024)
        slice_hist[((size_t)(b / NMSM_BUCKETS) * slices + slice) * NMSM_BUCKETS + (b % NMSM_BUCKETS)] = hist[b];
}
// where each window's entries start: the running total of the windows before it (64 bits: thirty-two windows of 2^27 scalars can be 2^32 entries)
__global__ __launch_bounds__(64) void nmsm_entry_base_kernel(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                             unsigned long long *__restrict__ entry_base /* [32] */)
{
    if (threadIdx.x) return;
    unsigned long long run = 0;
    for (int w = 0; w < NMSM_W; w++) {
        entry_base[w] = run;
        run += (unsigned long long)offsets[w * NMSM_BUCKETS + NMSM_BUCKETS - 1] + counts[w * NMSM_BUCKETS + NMSM_BUCKETS - 1];
    }
}
__global__ __launch_bounds__(1024) void nmsm_scatter_bare_kernel(uint32_t n, const uint32_t *__restrict__ scalars, int montgomery,
                                                                 const uint32_t *__restrict__ offsets /* [window][128] */,
                                                                 const uint32_t *__restrict__ slice_hist,
                                                                 const unsigned long long *__restrict__ entry_base, uint32_t *__restrict__ entries,
                                                                 const uint32_t *__restrict__ index)
{
    __shared__ uint32_t cursor[NMSM_W * NMSM_BUCKETS];
    __shared__ unsigned long long base[NMSM_W];
    const uint32_t slices = gridDim.x, slice = blockIdx.x;
    const SliceRange s = slice_range(n);
    for (int b = threadIdx.x; b < NMSM_W * NMSM_BUCKETS; b += 1024)
        cursor[b] = offsets[b] + slice_hist[((size_t)(b / NMSM_BUCKETS) * slices + slice) * NMSM_BUCKETS + (b % NMSM_BUCKETS)];
    if (threadIdx.x < NMSM_W) base[threadIdx.x] = entry_base[threadIdx.x];
    __syncthreads();
    for (uint32_t k = s.lo + threadIdx.x; k < s.hi; k += 1024) {
        const uint32_t i = index ? index[k] : k;
        const Fr8 sc = scalar_canonical(scalars + (size_t)i * 8, montgomery);
        if (scalar_is_one(sc)) continue;
        int d[NMSM_W];
        signed_digits<NMSM_C, NMSM_W>(sc, d);
#pragma unroll
        for (int j = 0; j < NMSM_W; j++)
            if (d[j]) entries[base[j] + atomicAdd(&cursor[j * NMSM_BUCKETS + digit_bucket(d[j])], 1u)] = digit_entry(i, d[j]);
    }
}
// one thread per (signature, item): the sum of the item's table rows
template <class F, bool PREFETCH>
__global__ __launch_bounds__(64, F::LANES > 1 ? 1 : 2) void nmsm_bucket_kernel(NmsmTables tables, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ counts,
                                                            const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
                                                            const uint32_t *__restrict__ entries, uint32_t *__restrict__ partial_items,
                                                            uint32_t target, uint32_t max_items,
                                                            const unsigned long long *__restrict__ entry_base /* a bare handle's windows; else null */)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int PW = Grp<F>::PT_WORDS;
    const size_t slot = blockIdx.y;
    size_t sig;
    const MsmDev m = tables.of(blockIdx.y, sig);
    const uint32_t it = (blockIdx.x * 64 + threadIdx.x) / F::LANES;            // F::LANES adjacent lanes share an item (the two-lane Fq2)
    if (it >= item_count[sig]) return;
    const uint32_t item = items[sig * (size_t)max_items + it], b = item & (NMSM_BUCKETS - 1), part = item >> 8;
    const uint32_t c = counts[sig * NMSM_BUCKETS + b];
    const uint32_t k = items_of(c, nmsm_split_of(row_total(offsets, counts, sig, NMSM_BUCKETS), target));
    const uint32_t lo = (uint32_t)((uint64_t)c * part / k), cnt = (uint32_t)((uint64_t)c * (part + 1) / k) - lo;     // equal parts
    const uint32_t *ent = entries + (entry_base ? (size_t)entry_base[sig] : sig * (size_t)NMSM_W * m.n) + offsets[sig * NMSM_BUCKETS + b] + lo;
    XyzzT<F> acc = pt_identity<F>();
    if (PREFETCH) {
        uint32_t e = cnt ? ent[0] : 0u;
        AffineT<F> p = load_row<F>(m.table + (size_t)(e & 0x7fffffffu) * PW);
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t e_next = j + 1 < cnt ? ent[j + 1] : e;
            const AffineT<F> p_next = load_row<F>(m.table + (size_t)(e_next & 0x7fffffffu) * PW);
            if (e >> 31) p.y = F::template neg<Grp<F>::K_AFFINE_Y>(p.y);
            acc = pt_add_affine(acc, p);
            e = e_next;
            p = p_next;
        }
    } else {
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t e = ent[j];
            AffineT<F> p = load_row<F>(m.table + (size_t)(e & 0x7fffffffu) * PW);
            if (e >> 31) p.y = F::template neg<Grp<F>::K_AFFINE_Y>(p.y);
            acc = pt_add_affine(acc, p);
        }
    }
    store_bucket<F>(partial_items + (slot * (size_t)max_items + it) * (size_t)Grp<F>::BK_WORDS, acc);
}
// the points whose scalar is one: thread t of `gridDim.x * 64` per signature takes every such-th of the list, the 64 sums of a
// workgroup are added up through LDS (six steps instead of the 64 / 128-fold serial addition they would cost the fold), and one
// partial sum per workgroup goes out: gridDim.x <= 64 of them per signature
template <class F>
__global__ __launch_bounds__(64, F::LANES > 1 ? 1 : 2) void nmsm_ones_kernel(NmsmTables tables, const uint32_t *__restrict__ ones_count, const uint32_t *__restrict__ ones_list,
                                                          uint32_t *__restrict__ partial_ones /* [blockIdx.y][groups_stride][BK_WORDS] */, uint32_t groups_stride,
                                                          uint32_t row_step /* 1; a bare handle's tables: 32 -- grid row y is (table y, window 0), the only window with ones */)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int SLOT = 4 * F::WORDS + 1, PER = 64 / F::LANES;                 // PER chains per workgroup (F::LANES lanes each)
    __shared__ uint32_t lds[32 * SLOT];
    const size_t slot = blockIdx.y;
    size_t sig;
    const MsmDev m = tables.of(blockIdx.y * row_step, sig);
    const uint32_t nthreads = gridDim.x * PER, t = blockIdx.x * PER + threadIdx.x / F::LANES;
    const uint32_t *list = ones_list + sig * m.n;
    XyzzT<F> acc = pt_identity<F>();
    if (m.ones_table) {
        // `list` is the mask of ones: one addition per group of eight points whose byte of it is not zero
        const uint32_t groups = (m.n + 7) / 8;
        for (uint32_t g = t; g < groups; g += nthreads) {
            const uint32_t byte = (list[g >> 2] >> (8 * (g & 3))) & 0xffu;
            if (byte) acc = pt_add_affine(acc, load_row<F>(m.ones_table + ((size_t)g * 255 + (byte - 1)) * Grp<F>::PT_WORDS));
        }
    } else {
        const uint32_t cnt = ones_count[sig];
        for (uint32_t k = t; k < cnt; k += nthreads)
            acc = pt_add_affine(acc, load_row<F>(m.table + (size_t)list[k] * Grp<F>::PT_WORDS));  // window 0 of the table = the point itself
    }
    const int lane = threadIdx.x / F::LANES;
    for (int stride = PER / 2; stride >= 1; stride >>= 1) {
        if (lane >= stride && lane < 2 * stride) store_bucket<F>(lds + (lane - stride) * SLOT, acc);
        __syncthreads();
        if (lane < stride) acc = pt_add(acc, load_bucket<F>(lds + lane * SLOT));
        __syncthreads();
    }
    if (lane == 0) store_bucket<F>(partial_ones + (slot * (size_t)groups_stride + blockIdx.x) * (size_t)Grp<F>::BK_WORDS, acc);
}
// the policy a group's narrow sum runs with: G2 in two lanes per point (frw_fq29.h Fq2PairField) -- the layout in memory is that of
// either G2 policy; the window tables and the dense pipeline keep the one-lane form
template <class F> struct BulkPolicy { typedef F type; };
template <> struct BulkPolicy<Fq2Field> { typedef Fq2PairField type; };
// more than 64 partial sums of ones (sums over more than 2^18 points): workgroup g of 64 adds up the partial sums g, g + 64, ... of its
// signature -- one per lane, then a tree through LDS -- and leaves sum g of 64 in the first 64 slots of the second stage's array
template <class F>
__global__ __launch_bounds__(64, F::LANES > 1 ? 1 : 2) void nmsm_ones_fold_kernel(const uint32_t *__restrict__ partial_ones, uint32_t groups, uint32_t groups_stride,
                                                               uint32_t *__restrict__ folded /* [sig][64][BK_WORDS] */)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int SLOT = 4 * F::WORDS + 1, BW = Grp<F>::BK_WORDS, PER = 64 / F::LANES;   // one wavefront: PER chains of F::LANES lanes
    __shared__ uint32_t lds[32 * SLOT];
    const size_t sig = blockIdx.y;
    const uint32_t g = blockIdx.x, lane = threadIdx.x / F::LANES;
    const uint32_t *src = partial_ones + sig * (size_t)groups_stride * BW;
    XyzzT<F> acc = pt_identity<F>();
    for (uint32_t k = g + 64 * lane; k < groups; k += 64 * PER) acc = pt_add(acc, load_bucket<F>(src + (size_t)k * BW));
    for (int stride = PER / 2; stride >= 1; stride >>= 1) {
        if ((int)lane >= stride && (int)lane < 2 * stride) store_bucket<F>(lds + (lane - stride) * SLOT, acc);
        __syncthreads();
        if ((int)lane < stride) acc = pt_add(acc, load_bucket<F>(lds + lane * SLOT));
        __syncthreads();
    }
    if (lane == 0) store_bucket<F>(folded + (sig * 64 + g) * (size_t)BW, acc);
}
// bucket b = the sum of its items, by a workgroup of its own: the buckets of small digits hold many times the mean (the high
// bytes of 14-bit values fall into 48 of them), and fifty items added up by one thread were the longest chain of the whole sum
template <class F>
__global__ __launch_bounds__(64, F::LANES > 1 ? 1 : 2) void nmsm_combine_kernel(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                             const uint32_t *__restrict__ item_first, const uint32_t *__restrict__ partial_items,
                                                             uint32_t *__restrict__ buckets /* [slot][128][BK_WORDS] */, uint32_t target, uint32_t max_items,
                                                             uint32_t sigs)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int SLOT = 4 * F::WORDS + 1, BW = Grp<F>::BK_WORDS, PER = 64 / F::LANES;
    __shared__ uint32_t lds[32 * SLOT];
    const size_t slot = blockIdx.y, sig = slot % sigs;
    const uint32_t b = blockIdx.x, lane = threadIdx.x / F::LANES;
    const uint32_t c = counts[sig * NMSM_BUCKETS + b];
    const uint32_t k = items_of(c, nmsm_split_of(row_total(offsets, counts, sig, NMSM_BUCKETS), target));
    const uint32_t *src = partial_items + (slot * (size_t)max_items + item_first[sig * NMSM_BUCKETS + b]) * (size_t)BW;
    XyzzT<F> acc = pt_identity<F>();
    for (uint32_t j = lane; j < k; j += PER) acc = pt_add(acc, load_bucket<F>(src + (size_t)j * BW));
    for (int stride = PER / 2; stride >= 1; stride >>= 1) {
        if ((int)lane >= stride && (int)lane < 2 * stride) store_bucket<F>(lds + (lane - stride) * SLOT, acc);
        __syncthreads();
        if ((int)lane < stride) acc = pt_add(acc, load_bucket<F>(lds + lane * SLOT));
        __syncthreads();
    }
    if (lane == 0) store_bucket<F>(buckets + (slot * NMSM_BUCKETS + b) * (size_t)BW, acc);
}

// ONE WAVEFRONT per signature folds the 128 buckets and the ones' partial sums into the result.  (The first version was one
// workgroup of 384 / 256 threads: a workgroup of several wavefronts that is issued while the 2^18-point bucket kernel occupies the
// chip -- two wavefronts of 240 registers on every SIMD -- finds no CU with room for all of it until that kernel ends; 42 ms late in
// profiles/r04_groth16_timeline_64_starved.txt.  A single wavefront takes whatever slot frees up next.)
// PER = 64 / F::LANES chains, NB = 128 / PER adjacent buckets each; bucket b = i NB + k has weight b + 1 = i NB + (k + 1):
//     result = sum_i [ sum_k (k + 1) B_(i,k) ] + NB sum_(i >= 1) Suffix_i + ones,   Suffix_i = sum_(j >= i) sum_k B_(j,k)
//   phase 0   chain i adds up its buckets from the last to the first (their items one after the other, unless nmsm_combine_kernel has
//             done that), parking run_k = B_k + .. + B_(NB-1) after each: run_0 is the chain's total, sum_k run_k its weighted sum
//   phase 1   suffix scan of the totals over the chains (log2 PER steps through LDS)
//   phase 2   x NB (the value added to itself log2 NB times; chain 0 contributes nothing), + the chain's weighted sum, + the ones
//   phase 3   tree over the chains, one inversion, ark-ff's bytes out
// ONE addition site: every step is "sum (+)= the point at p", p in global memory or in LDS.
template <class F>
__global__ __launch_bounds__(64) void nmsm_finish_kernel(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                         const uint32_t *__restrict__ item_first, const uint32_t *__restrict__ partial_items,
                                                         const uint32_t *__restrict__ buckets /* [sig][128][BK_WORDS], or null */,
                                                         const uint32_t *__restrict__ partial_ones /* [sig][ones_stride][BK_WORDS] */,
                                                         int ones_groups, uint32_t ones_stride, uint32_t target, uint32_t max_items,
                                                         uint32_t *__restrict__ out /* [slot][ARK_WORDS], or [slot][BK_WORDS] */, int xyzz_out,
                                                         uint32_t sigs, int ones_window0 /* a bare handle: rows are (table, window); the ones' sums are [table] and go with window 0 */)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    constexpr int SLOT = 4 * F::WORDS + 1, BW = Grp<F>::BK_WORDS, PER = 64 / F::LANES, NB = NMSM_BUCKETS / PER;
    constexpr int LOG_PER = PER == 64 ? 6 : 5, LOG_NB = NB == 2 ? 1 : 2;
    static_assert(PER * NB == NMSM_BUCKETS && (1 << LOG_PER) == PER && (1 << LOG_NB) == NB, "64 or 32 chains of 2 or 4 buckets");
    __shared__ uint32_t lds[NMSM_BUCKETS * SLOT];                     // 29 KB (G1) / 58 KB (G2): slot i NB + k
    __shared__ uint32_t longest[NB];
    const size_t slot = blockIdx.x, sig = slot % sigs;
    const int i = threadIdx.x / F::LANES;
    // the items of the chain's buckets (one each when they come combined)
    const uint32_t *src[NB];
    uint32_t mine[NB];
    if (threadIdx.x < NB) longest[threadIdx.x] = 1;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NB; k++) {
        const int b = i * NB + k;
        if (buckets) {
            src[k] = buckets + (slot * NMSM_BUCKETS + b) * (size_t)BW;
            mine[k] = 1;
        } else {
            const uint32_t c = counts[sig * NMSM_BUCKETS + b];
            mine[k] = items_of(c, nmsm_split_of(row_total(offsets, counts, sig, NMSM_BUCKETS), target));
            src[k] = partial_items + (slot * (size_t)max_items + item_first[sig * NMSM_BUCKETS + b]) * (size_t)BW;
            atomicMax(&longest[k], mine[k]);
        }
    }
    __syncthreads();
    uint32_t phase0 = 0;
#pragma unroll
    for (int k = 0; k < NB; k++) phase0 += longest[k] + 1;            // the items of bucket k, then the step that parks run_k
    const int ones_steps = (ones_groups + PER - 1) / PER;
    const uint32_t at_local = phase0, at_reload = at_local + (NB - 1) + 1, at_scan = at_reload + 1, at_weight = at_scan + LOG_PER,
                   at_final = at_weight + LOG_NB, at_ones = at_final + 1, at_tree = at_ones + ones_steps, steps = at_tree + LOG_PER;
    XyzzT<F> sum = pt_identity<F>();
    for (uint32_t step = 0; step < steps; step++) {
        int store_slot = -1;
        bool reset = false, add = false;
        const uint32_t *p = lds;
        if (step < phase0) {
            // bucket k = NB - 1 .. 0
            uint32_t s = step;
            int k = NB - 1;
#pragma unroll
            for (int kk = NB - 1; kk >= 1; kk--)
                if (k == kk && s >= longest[kk] + 1) { s -= longest[kk] + 1; k = kk - 1; }
            const uint32_t *sp = src[0];
            uint32_t mk = mine[0], lk = longest[0];
#pragma unroll
            for (int kk = 1; kk < NB; kk++)
                if (k == kk) { sp = src[kk]; mk = mine[kk]; lk = longest[kk]; }     // (selects: a register array indexed at run time would live in scratch)
            if (s < lk) { add = s < mk; p = sp + (size_t)s * BW; }
            else store_slot = i * NB + k;                              // run_k
        } else if (step < at_reload - 1) {                             // weighted sum: run_0 (held) + run_1 + .. + run_(NB-1)
            add = true; p = lds + (i * NB + 1 + (int)(step - at_local)) * SLOT;
        } else if (step == at_reload - 1) {
            store_slot = i * NB + 1;                                   // the chain's weighted sum parks where run_1 was
        } else if (step == at_reload) {
            reset = true; add = true; p = lds + (i * NB) * SLOT;       // the chain's total again
        } else if (step < at_weight) {                                 // suffix scan, offset 1, 2, .., PER / 2
            const int off = 1 << (step - at_scan);
            store_slot = i * NB;
            add = i + off < PER; p = lds + ((i + off) * NB) * SLOT;
        } else if (step < at_final) {                                  // x 2, log2 NB times
            store_slot = i * NB;
            add = true; p = lds + (i * NB) * SLOT;
        } else if (step == at_final) {
            reset = i == 0;                                            // weight i NB: nothing from the first chain
            add = true; p = lds + (i * NB + 1) * SLOT;
        } else if (step < at_tree) {
            const int g = i + PER * (int)(step - at_ones);
            const size_t ones_row = ones_window0 ? slot / sigs : slot;
            add = g < ones_groups && !(ones_window0 && sig != 0); p = partial_ones + (ones_row * (size_t)ones_stride + (size_t)g) * BW;
        } else {
            const int stride = PER >> (step - at_tree + 1);
            if (i >= stride && i < 2 * stride) store_slot = (i - stride) * NB;
            add = i < stride; p = lds + (i * NB) * SLOT;
        }
        if (store_slot >= 0) store_bucket<F>(lds + store_slot * SLOT, sum);
        __syncthreads();
        if (reset) sum = pt_identity<F>();
        if (add) sum = pt_add(sum, load_bucket<F>(p));
        __syncthreads();
    }
    if (i == 0) {
        if (xyzz_out) store_bucket<F>(out + slot * BW, sum);         // as msm_fold2_kernel
        else store_ark_point<F>(out + slot * Grp<F>::ARK_WORDS, pt_to_affine(sum));
    }
}

// ---- k G for many scalars: the FixedBaseMSM of ark-groth16's generator (generator.rs builds h_query, a_query, l_query and
// b_g2_query this way from the toxic waste).  8-bit windows of the generator: table[w][d] = d 2^(8 w) G, then 32 mixed additions.
constexpr int FB_WINDOWS = 32, FB_DIGITS = 256;
template <class F> __device__ __forceinline__ AffineT<F> group_generator();
template <> __device__ __forceinline__ AffineT<FqField> group_generator<FqField>()
{
    AffineT<FqField> g;
    g.x = fq_const(G1_GEN_X29); g.y = fq_const(G1_GEN_Y29); g.inf = false;
    return g;
}
template <> __device__ __forceinline__ AffineT<Fq2Field> group_generator<Fq2Field>()
{
    AffineT<Fq2Field> g;
    g.x.c0 = fq_const(G2_GEN_X0_29); g.x.c1 = fq_const(G2_GEN_X1_29); g.y.c0 = fq_const(G2_GEN_Y0_29); g.y.c1 = fq_const(G2_GEN_Y1_29);
    g.inf = false;
    return g;
}
template <class F>
__global__ __launch_bounds__(64) void fixed_base_table_kernel(uint32_t *__restrict__ table /* [32][256][PT_WORDS] */)
{
    const int id = blockIdx.x * 64 + threadIdx.x, w = id >> 8, d = id & 255;
    if (w >= FB_WINDOWS) return;
    const AffineT<F> g = group_generator<F>();
    XyzzT<F> acc = pt_identity<F>();
    for (int bit = 7; bit >= 0; bit--) {                      // d G
        acc = pt_double(acc);
        if ((d >> bit) & 1) acc = pt_add_affine(acc, g);
    }
    for (int k = 0; k < 8 * w; k++) acc = pt_double(acc);     // 2^(8 w) d G
    store_row<F>(table + (size_t)id * Grp<F>::PT_WORDS, pt_to_affine(acc));
}
template <class F>
__global__ __launch_bounds__(64) void fixed_base_kernel(size_t count, const uint32_t *__restrict__ scalars /* [count][8], canonical */,
                                                        const uint32_t *__restrict__ table, uint32_t *__restrict__ out /* [count][ARK_WORDS] */)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const Fr8 k = fr_load(scalars + i * 8);
    XyzzT<F> acc = pt_identity<F>();
    for (int w = 0; w < FB_WINDOWS; w++) {
        const uint32_t d = (k.l[w >> 2] >> (8 * (w & 3))) & 255u;
        if (d) acc = pt_add_affine(acc, load_row<F>(table + ((size_t)w * FB_DIGITS + d) * Grp<F>::PT_WORDS));
    }
    store_ark_point<F>(out + i * Grp<F>::ARK_WORDS, pt_to_affine(acc));
}
// ---- the same for a key made on the device (frw_groth16_setup_r1cs_opts: 5 x 10^8 G1 and 1.2 x 10^8 G2 multiples for the 1,024-statement
// aggregate): SIXTEEN-bit windows -- table[w][d] = d 2^(16 w) G, 2^20 rows (117 MB, G2 235 MB), sixteen mixed additions per scalar instead of
// thirty-two -- G2 with two lanes per point (with one lane and 3.8 KB of scratch the 123 M rows of b_g2_query took 85 of the first version's
// 94 seconds), and the multiples written as table rows (29-bit limbs, what load_row reads) straight into a bare handle: a 2^27-point
// h_query never exists as ark-ff bytes anywhere.
constexpr int FBW_WINDOWS = 16, FBW_DIGITS = 65536;
// B_w = 2^(16 w) G, w < 16, one after the other (240 doublings of one chain)
template <class F>
__global__ __launch_bounds__(64) void fixed_base_window_gens_kernel(uint32_t *__restrict__ gens /* [16][PT_WORDS] */)
{
    if (threadIdx.x || blockIdx.x) return;
    XyzzT<F> acc = pt_from_affine(group_generator<F>());
    for (int w = 0; w < FBW_WINDOWS; w++) {
        store_row<F>(gens + (size_t)w * Grp<F>::PT_WORDS, pt_to_affine(acc));
        for (int k = 0; k < 16; k++) acc = pt_double(acc);
    }
}
template <class F>
__global__ __launch_bounds__(64) void fixed_base_wide_table_kernel(const uint32_t *__restrict__ gens, uint32_t *__restrict__ table /* [16][65536][PT_WORDS] */)
{
    const uint32_t id = blockIdx.x * 64 + threadIdx.x, w = id >> 16, d = id & 65535u;
    if (w >= (uint32_t)FBW_WINDOWS) return;
    const AffineT<F> g = load_row<F>(gens + (size_t)w * Grp<F>::PT_WORDS);
    XyzzT<F> acc = pt_identity<F>();
    for (int bit = 15; bit >= 0; bit--) {
        acc = pt_double(acc);
        if ((d >> bit) & 1u) acc = pt_add_affine(acc, g);
    }
    store_row<F>(table + (size_t)id * Grp<F>::PT_WORDS, pt_to_affine(acc));
}
// F: FqField, or Fq2PairField (two adjacent lanes per scalar).  ARK_OUT: ark-ff's affine bytes (the verifying key's points) instead of rows.
template <class F, bool ARK_OUT>
__global__ __launch_bounds__(64) void fixed_base_wide_kernel(size_t count, const uint32_t *__restrict__ scalars /* [count][8], canonical */,
                                                             const uint32_t *__restrict__ table, uint32_t *__restrict__ out)
{
    const size_t i = ((size_t)blockIdx.x * 64 + threadIdx.x) / F::LANES;
    if (i >= count) return;
    const Fr8 k = fr_load(scalars + i * 8);
    XyzzT<F> acc = pt_identity<F>();
    for (int w = 0; w < FBW_WINDOWS; w++) {
        const uint32_t d = (k.l[w >> 1] >> (16 * (w & 1))) & 65535u;
        if (d) acc = pt_add_affine(acc, load_row<F>(table + ((size_t)w * FBW_DIGITS + d) * Grp<F>::PT_WORDS));
    }
    if (ARK_OUT) store_ark_point<F>(out + i * Grp<F>::ARK_WORDS, pt_to_affine(acc));
    else store_row<F>(out + i * Grp<F>::PT_WORDS, pt_to_affine(acc));
}

}  // namespace frw

#if !defined(FRW_MSM_PROBE)     // (tools/kernel_resources.py compiles single instantiations of the kernels above through a probe unit)
// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
struct frw_msm {
    int device;
    int group;                  // 1: G1, 2: G2
    int window_bits;            // 16: the dense pipeline (32,768 buckets), 8: the narrow one (128 buckets)
    bool bare = false;          // the table is the points themselves (one row each): the sums run window by window (round 5)
    bool wide = false;          // ... a dense bare handle on thirteen 20-bit windows (frw::WIDE_*): from 2^23 points, or asked for at load time
    uint64_t row_lo = 0;        // a slice of a sharded key: the index of row 0 in the whole query (the caller offsets the scalars by it)
    frw::MsmDev dev;
    void *table;
    void *ones_table;           // narrow handles of up to 2^18 points (MsmDev::ones_table), else null
};

namespace {
using frw::FqField;
using frw::Fq2Field;
using frw::MsmBufs; using frw::MsmWideBufs; using frw::NmsmBufs;
static_assert(frw::Grp<FqField>::BK_WORDS == frw::G1_BK_WORDS && frw::Grp<Fq2Field>::BK_WORDS == frw::G2_BK_WORDS, "frw_layout.h lays the workspaces out by these");
// Wide windows (frw::WIDE_*): bare dense handles of 2^26 points and more, and those LOADED so (frw_msm_g1_load_bare(.., narrow = 2, ..): the
// tests do, on the small adversarial vectors and on 2^18 points).  Measured on the 2^27-point sum of the 1,024-statement aggregate
// (profiles/r05_wide_windows_ab.txt): the bucket kernel 350 -> 308 ms, the sort 65 -> 34 ms once every pass of it wrote runs (the first
// version's scatter into 208 x 32,768 open cache lines took 76 ms and gave the gain back), the proof 683 - 698 -> 613 ms.
constexpr uint32_t MSM_WIDE_FROM_DEFAULT = (1u << 26) - 1;           // (h_query of the 2^26 domain has 2^26 - 1 points)
static uint32_t msm_wide_from()
{
    static const uint32_t v = [] {
        const char *e = getenv("FRW_BARE_WIDE_FROM_LOG2");             // (measurement switch: tools/time_aggregate_large.py)
        const int lg = e ? atoi(e) : 0;
        return lg >= 10 && lg <= 31 ? ((uint32_t)1 << lg) - 1 : MSM_WIDE_FROM_DEFAULT;
    }();
    return v;
}

template <class F> int msm_load(int device, int group, size_t num_points, const uint64_t *bases, int window_bits, bool bare, frw_msm **out, bool force_wide = false)
{
    // (a table row index and its window share 31 bits of an entry: 2^26 points x 16 windows, 2^25 x 32; a bare handle's entries are point indices)
    if (!out || !bases || num_points == 0 || num_points > (bare ? ((size_t)1 << 31) - 1 : (size_t)1 << (window_bits == 8 ? 25 : 26))) return FRW_E_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    frw_msm *m = new (std::nothrow) frw_msm;
    if (!m) return FRW_E_OUT_OF_MEMORY;
    m->device = device;
    m->group = group;
    m->window_bits = window_bits;
    m->bare = bare;
    m->wide = bare && window_bits == 16 && (force_wide || num_points >= msm_wide_from());
    m->table = nullptr;
    m->ones_table = nullptr;
    m->dev.ones_table = nullptr;
    m->dev.n = (uint32_t)num_points;
    void *d_bases = nullptr;
    const size_t table_bytes = (size_t)(bare ? 1 : 256 / window_bits) * num_points * frw::Grp<F>::PT_WORDS * 4, ark_bytes = (size_t)frw::Grp<F>::ARK_WORDS * 4;
    e = hipMalloc(&m->table, table_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_bases, num_points * ark_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_bases, bases, num_points * ark_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(frw::msm_precompute_kernel<F>, dim3((unsigned)((num_points + 63) / 64)), dim3(64), 0, nullptr,
                           (uint32_t)num_points, (const uint32_t *)d_bases, (uint32_t *)m->table, bare ? 256 : window_bits);     // (256-bit "windows": one row per point)
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (d_bases) (void)hipFree(d_bases);
    d_bases = nullptr;
    // the subset sums of every group of eight points, for the scalars equal to one (narrow handles of per-signature size: an aggregate
    // statement's tables are tens of gigabytes as it is, and its ones go through the list)
    if (e == hipSuccess && !bare && window_bits == 8 && num_points <= ((size_t)1 << 18)) {
        const size_t entries = (num_points + 7) / 8 * 255;
        e = hipMalloc(&m->ones_table, entries * frw::Grp<F>::PT_WORDS * 4);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(frw::msm_ones_table_kernel<F>, dim3((unsigned)((entries + 63) / 64)), dim3(64), 0, nullptr, (uint32_t)num_points,
                               (const uint32_t *)m->table, (uint32_t *)m->ones_table);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) {
        frw_msm_free(m);
        return frw::record_hip_error(e, "frw_msm_load");
    }
    m->dev.table = (const uint32_t *)m->table;
    m->dev.ones_table = (const uint32_t *)m->ones_table;
    *out = m;
    return FRW_OK;
}

template <class F> int fixed_base(int device, size_t count, const uint64_t *scalars, uint64_t *out)
{
    if (count && (!scalars || !out)) return FRW_E_INVALID_ARG;
    if (count == 0) return FRW_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    hipError_t e = hipSetDevice(device);
    void *d_table = nullptr, *d_sc = nullptr, *d_out = nullptr;
    const size_t ark_bytes = (size_t)frw::Grp<F>::ARK_WORDS * 4;
    if (e == hipSuccess) e = hipMalloc(&d_table, (size_t)frw::FB_WINDOWS * frw::FB_DIGITS * frw::Grp<F>::PT_WORDS * 4);
    if (e == hipSuccess) e = hipMalloc(&d_sc, count * 32);
    if (e == hipSuccess) e = hipMalloc(&d_out, count * ark_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_sc, scalars, count * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(frw::fixed_base_table_kernel<F>, dim3(frw::FB_WINDOWS * frw::FB_DIGITS / 64), dim3(64), 0, nullptr, (uint32_t *)d_table);
        hipLaunchKernelGGL(frw::fixed_base_kernel<F>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, nullptr, count,
                           (const uint32_t *)d_sc, (const uint32_t *)d_table, (uint32_t *)d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, count * ark_bytes, hipMemcpyDeviceToHost);
    for (void *p : {d_table, d_sc, d_out})
        if (p) (void)hipFree(p);
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_fixed_base");
}

// One chunk of the dense pipeline: `rows` grid rows -- signatures with all their windows, or (a bare handle) the sixteen windows of ONE
// scalar vector -- to `rows` sums in `out` (XYZZ buckets or ark-ff's affine bytes).
template <class F, bool PREFETCH>
hipError_t msm_rows(const frw_msm *m, size_t rows, const uint32_t *sc, size_t stride_words, int montgomery, uint32_t *out, bool xyzz_out,
                    void *d_workspace, hipStream_t st)
{
    const uint32_t n = m->dev.n;
    const bool bare = m->bare;
    const MsmBufs b = frw::msm_layout(d_workspace, rows, n, bare, frw::Grp<F>::BK_WORDS);
    uint32_t *slice_hist = b.buckets;                                // [rows][32][32,768], dead before the first bucket is stored (rows == 1: see below)
    const int slices = rows == 1 ? frw::MSM_SLICES_LONE : frw::MSM_SLICES;
    if (rows == 1) slice_hist = b.partial_items;                     // [224][32,768], dead before the first work item's sum is stored
    const dim3 sgrid((unsigned)slices, (unsigned)rows);
    hipError_t e = hipMemsetAsync(b.ones_count, 0, rows * 16, st);
    if (e != hipSuccess) return e;
    // where the sort's digits come from: a bare handle's are stored once, window-major, and its grid rows read their own window's
    const frw::DenseTableDigits from_scalars{sc, stride_words, montgomery, b.ones_count, b.ones_list, 0};
    const frw::StoredDigits from_digits{(const int16_t *)b.digits};
    if (bare) {
        hipLaunchKernelGGL(frw::msm_digits_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, sc, montgomery, b.digits);
        hipLaunchKernelGGL(frw::msm_sort_hist_kernel<frw::StoredDigits>, sgrid, dim3(1024), 0, st, n, from_digits, slice_hist);
    } else {
        hipLaunchKernelGGL(frw::msm_sort_hist_kernel<frw::DenseTableDigits>, sgrid, dim3(1024), 0, st, n, from_scalars, slice_hist);
    }
    hipLaunchKernelGGL(frw::msm_slice_offsets_kernel, dim3(frw::MSM_BUCKETS / 256, (unsigned)rows), dim3(256), 0, st, slice_hist, b.counts, slices);
    hipLaunchKernelGGL(frw::msm_scan_kernel, dim3((unsigned)rows), dim3(1024), 0, st, b.counts, b.offsets);
    // (four at a time: 12.6 ms with the finer split, 12.1 without); beyond 2^18 points: see MSM_MAX_ITEMS_LARGE
    // (a lone Falcon-1024 proof with 2 / 3 / 4: 4.72 / 4.27 / 4.05 ms -- the finer cut shares the chip better with the proof's other
    // sums; 5, with a longer item list, changes nothing any more: 3.86 - 3.91 against 3.90 ms, the sums overlap either way)
    // (a bare handle's sixteen windows are sixteen rows of equal buckets: 524,288 items as they are)
    const uint32_t finer = bare ? 1u : rows <= 2 ? (n > (1u << 18) ? 24u : 4u) : 1u;
    hipLaunchKernelGGL(frw::msm_order_kernel, dim3((unsigned)rows), dim3(1024), 0, st, b.counts, b.offsets, b.order, b.item_first, b.items, b.item_count, finer,
                       b.max_items);
    if (bare) hipLaunchKernelGGL(frw::msm_sort_scatter_kernel<frw::StoredDigits>, sgrid, dim3(1024), 0, st, n, from_digits, b.offsets, slice_hist, b.entries);
    else hipLaunchKernelGGL(frw::msm_sort_scatter_kernel<frw::DenseTableDigits>, sgrid, dim3(1024), 0, st, n, from_scalars, b.offsets, slice_hist, b.entries);
    hipLaunchKernelGGL((frw::msm_bucket_kernel<F, PREFETCH>), dim3(b.max_items / 64, (unsigned)rows), dim3(64), 0, st, m->dev, b.offsets,
                       b.counts, b.items, b.item_count, b.entries, b.partial_items, finer, b.max_items, b.ent_stride, (const unsigned long long *)nullptr);
    hipLaunchKernelGGL(frw::msm_combine_kernel<F>, dim3(frw::MSM_BUCKETS / 64, (unsigned)rows), dim3(64), 0, st, b.offsets, b.counts, b.item_first,
                       b.partial_items, b.buckets, finer, b.max_items);
    // first stage of the fold: enough threads to occupy the chip (~2^16), as few as that allows
    // (64 per call with 16 / 32 / 64 buckets per thread: 927 - 929 / 927 - 930 / 919 proofs/s -- the fold is 3 of a call's 69 ms)
    const int log_chunk = rows >= 128 ? 6 : rows >= 32 ? 5 : 3;
    const unsigned t1 = (unsigned)frw::MSM_BUCKETS >> log_chunk;
    frw::MsmDev ones_dev = m->dev;
    if (bare) ones_dev.n = 0;                                        // (no list: every row's count is zero and its slice of the list the same empty one)
    hipLaunchKernelGGL(frw::msm_ones_kernel<F>, dim3(t1 / 64, (unsigned)rows), dim3(64), 0, st, ones_dev, b.ones_count, b.ones_list, b.partial);
    if (log_chunk == 6) hipLaunchKernelGGL((frw::msm_fold1_kernel<F, 6>), dim3(t1 / 64, (unsigned)rows), dim3(64), 0, st, b.buckets, b.partial, (uint32_t *)nullptr);
    else if (log_chunk == 5) hipLaunchKernelGGL((frw::msm_fold1_kernel<F, 5>), dim3(t1 / 64, (unsigned)rows), dim3(64), 0, st, b.buckets, b.partial, (uint32_t *)nullptr);
    else hipLaunchKernelGGL((frw::msm_fold1_kernel<F, 3>), dim3(t1 / 64, (unsigned)rows), dim3(64), 0, st, b.buckets, b.partial, (uint32_t *)nullptr);
    hipLaunchKernelGGL(frw::msm_fold2_kernel<F>, dim3((unsigned)rows), dim3(frw::MSM_FOLD_THREADS), 0, st, b.partial,
                       (int)(t1 / frw::MSM_FOLD_THREADS), out, xyzz_out ? 1 : 0);
    return hipGetLastError();
}
// ONE scalar vector over a bare handle on wide windows (frw::WIDE_*): the coarse sort, the rows' fine sorts, work items, buckets, the
// two-stage folds (weighted and plain), the windows, Horner's rule
template <class F, bool PREFETCH>
hipError_t msm_rows_wide(const frw_msm *m, const uint32_t *sc, int montgomery, uint32_t *out, bool xyzz_out, void *d_workspace, hipStream_t st)
{
    constexpr unsigned R = frw::WIDE_ROWS;
    const uint32_t n = m->dev.n;
    const MsmWideBufs w = frw::msm_layout_wide(d_workspace, n, frw::Grp<F>::BK_WORDS);
    const MsmBufs &b = w.rows;
    hipError_t e = hipMemsetAsync(b.ones_count, 0, R * 16, st);
    if (e != hipSuccess) return e;
    const dim3 sgrid(frw::WIDE_SLICES, frw::WIDE_W);
    hipLaunchKernelGGL(frw::msm_wide_digits_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, sc, montgomery, w.digits);
    hipLaunchKernelGGL(frw::msm_wide_bin_hist_kernel, sgrid, dim3(1024), 0, st, n, (const int32_t *)w.digits, w.slice_hist);
    hipLaunchKernelGGL(frw::msm_wide_bin_offsets_kernel, dim3(1), dim3(1024), 0, st, (uint32_t)frw::WIDE_SLICES, w.slice_hist, w.bin_count, w.bin_start, w.row_count,
                       w.row_start);
    hipLaunchKernelGGL(frw::msm_wide_bin_scatter_kernel, sgrid, dim3(1024), 0, st, n, (const int32_t *)w.digits, (const uint32_t *)w.slice_hist,
                       (const unsigned long long *)w.bin_start, w.coarse);
    uint32_t *part_hist = b.buckets;                                  // [6,656][32][1,024]: 0.9 GB of the buckets' 1.5, dead before the first bucket is stored
    static_assert((size_t)frw::WIDE_ALL_BINS * frw::WIDE_PARTS * frw::WIDE_BIN_BUCKETS <= (size_t)R * frw::MSM_BUCKETS * frw::Grp<F>::BK_WORDS, "the parts' histograms borrow the buckets");
    const dim3 pgrid(frw::WIDE_ALL_BINS * frw::WIDE_PARTS);
    hipLaunchKernelGGL(frw::msm_wide_bucket_hist_kernel, pgrid, dim3(1024), 0, st, (const uint2 *)w.coarse, (const uint32_t *)w.bin_count,
                       (const unsigned long long *)w.bin_start, part_hist);
    hipLaunchKernelGGL(frw::msm_wide_bucket_parts_kernel, dim3(frw::WIDE_ALL_BINS), dim3(1024), 0, st, part_hist, b.counts);
    hipLaunchKernelGGL(frw::msm_scan_kernel, dim3(R), dim3(1024), 0, st, b.counts, b.offsets);
    hipLaunchKernelGGL(frw::msm_order_kernel, dim3(R), dim3(1024), 0, st, b.counts, b.offsets, b.order, b.item_first, b.items, b.item_count, 1u, b.max_items);
    hipLaunchKernelGGL(frw::msm_wide_bucket_scatter_kernel, pgrid, dim3(1024), 0, st, (const uint2 *)w.coarse, (const uint32_t *)w.bin_count,
                       (const unsigned long long *)w.bin_start, (const uint32_t *)b.offsets, (const uint32_t *)part_hist, (const unsigned long long *)w.row_start,
                       w.entries);
    hipLaunchKernelGGL((frw::msm_bucket_kernel<F, PREFETCH>), dim3(b.max_items / 64, R), dim3(64), 0, st, m->dev, b.offsets, b.counts, b.items, b.item_count,
                       w.entries, b.partial_items, 1u, b.max_items, (size_t)0, (const unsigned long long *)w.row_start);
    hipLaunchKernelGGL(frw::msm_combine_kernel<F>, dim3(frw::MSM_BUCKETS / 64, R), dim3(64), 0, st, b.offsets, b.counts, b.item_first, b.partial_items,
                       b.buckets, 1u, b.max_items);
    // the folds: 64 buckets per thread (208 rows x 512 threads fill the chip), weighted and plain; then 512 threads per row and sum
    constexpr int LOG_CHUNK = 6;
    const unsigned t1 = (unsigned)frw::MSM_BUCKETS >> LOG_CHUNK;
    frw::MsmDev ones_dev = m->dev;
    ones_dev.n = 0;
    hipLaunchKernelGGL(frw::msm_ones_kernel<F>, dim3(t1 / 64, R), dim3(64), 0, st, ones_dev, b.ones_count, b.ones_list, b.partial);     // (no ones: the partial sums start as the identity)
    hipLaunchKernelGGL((frw::msm_fold1_kernel<F, LOG_CHUNK>), dim3(t1 / 64, R), dim3(64), 0, st, b.buckets, b.partial, w.partial_plain);
    hipLaunchKernelGGL(frw::msm_fold2_kernel<F>, dim3(R), dim3(frw::MSM_FOLD_THREADS), 0, st, b.partial, (int)(t1 / frw::MSM_FOLD_THREADS), w.s1, 1);
    hipLaunchKernelGGL(frw::msm_fold2_kernel<F>, dim3(R), dim3(frw::MSM_FOLD_THREADS), 0, st, w.partial_plain, (int)(t1 / frw::MSM_FOLD_THREADS), w.s0, 1);
    hipLaunchKernelGGL(frw::msm_wide_window_kernel<F>, dim3(frw::WIDE_W), dim3(64), 0, st, (const uint32_t *)w.s1, (const uint32_t *)w.s0, w.window_sums);
    hipLaunchKernelGGL(frw::msm_horner_kernel<F>, dim3(1), dim3(64), 0, st, (const uint32_t *)w.window_sums, (int)frw::WIDE_W, (int)frw::WIDE_C, out, xyzz_out ? 1 : 0);
    return hipGetLastError();
}
// the whole call for one group; `d_out` rows are ARK_WORDS / 2 uint64_t
template <class F, bool PREFETCH>
int msm_run(const frw_msm *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, int montgomery, uint64_t *d_out,
            void *d_workspace, size_t workspace_bytes, hipStream_t st, bool xyzz_out = false)
{
    const uint32_t n = m->dev.n;
    const size_t per = frw::msm_workspace_per_signature(n, m->bare, m->wide, frw::Grp<F>::BK_WORDS);
    size_t chunk = workspace_bytes / per;
    if (chunk == 0 || ((uintptr_t)d_workspace & 15)) return FRW_E_INVALID_ARG;
    if (chunk > 32768) chunk = 32768;                                  // grid.y
    constexpr int BW = frw::Grp<F>::BK_WORDS;
    hipError_t e = hipSetDevice(m->device);
    if (m->wide) {
        for (size_t sig = 0; e == hipSuccess && sig < batch; sig++)
            e = msm_rows_wide<F, PREFETCH>(m, (const uint32_t *)(d_scalars + sig * scalar_stride * 4), montgomery,
                                           (uint32_t *)d_out + sig * (xyzz_out ? BW : frw::Grp<F>::ARK_WORDS), xyzz_out, d_workspace, st);
        return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_msm_dev");
    }
    if (m->bare) {
        // one scalar vector at a time: its sixteen windows fill the grid; the window sums wait at the end of the workspace for Horner's rule
        uint32_t *window_sums = frw::msm_layout(d_workspace, frw::MSM_W, n, true, BW).window_sums;
        for (size_t sig = 0; e == hipSuccess && sig < batch; sig++) {
            e = msm_rows<F, PREFETCH>(m, frw::MSM_W, (const uint32_t *)(d_scalars + sig * scalar_stride * 4), 0, montgomery, window_sums, true, d_workspace, st);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(frw::msm_horner_kernel<F>, dim3(1), dim3(64), 0, st, window_sums, frw::MSM_W, frw::MSM_C,
                               (uint32_t *)d_out + sig * (xyzz_out ? BW : frw::Grp<F>::ARK_WORDS), xyzz_out ? 1 : 0);
            e = hipGetLastError();
        }
        return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_msm_dev");
    }
    for (size_t lo = 0; e == hipSuccess && lo < batch; lo += chunk) {
        const size_t cnt = batch - lo < chunk ? batch - lo : chunk;
        e = msm_rows<F, PREFETCH>(m, cnt, (const uint32_t *)(d_scalars + lo * scalar_stride * 4), scalar_stride * 8, montgomery,
                                  (uint32_t *)d_out + lo * (xyzz_out ? BW : frw::Grp<F>::ARK_WORDS), xyzz_out, d_workspace, st);
    }
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_msm_dev");
}
// ---- the narrow pipeline in two halves: the counting sort of the scalars' digits (which knows nothing of the points), and the sums
// over one window table with a sort's result.  The four witness-side sums of a proof take the SAME scalars -- z ++ [1, r, s] against
// a_query, b_g1_query, b_g2_query and l_query, each table padded to the same length with points at infinity -- so a proof sorts once
// (frw_groth16_prove_dev); frw_msm_g1_dev / _g2_dev on a narrow handle are one sort and one sum.
// ones_as_mask: every table that will be summed with this sort has the subset sums of its groups of eight (MsmDev::ones_table): the
// scalars equal to one are then recorded as a bit mask (the first n / 32 words of each signature's list) instead of a list
hipError_t nmsm_sort(const NmsmBufs &b, uint32_t n, size_t cnt, const uint32_t *sc, size_t stride_words, int montgomery, bool ones_as_mask, hipStream_t st)
{
    const uint32_t slices = frw::nmsm_slices(n);
    const dim3 sgrid(slices, (unsigned)cnt);
    hipError_t e = hipMemsetAsync(b.ones_count, 0, cnt * 4, st);
    if (e == hipSuccess && ones_as_mask) e = hipMemsetAsync(b.ones_list, 0, cnt * (size_t)n * 4, st);
    if (e != hipSuccess) return e;
    const frw::NarrowTableDigits from_scalars{sc, stride_words, montgomery, b.ones_count, b.ones_list, ones_as_mask ? 1 : 0};
    hipLaunchKernelGGL(frw::msm_sort_hist_kernel<frw::NarrowTableDigits>, sgrid, dim3(1024), 0, st, n, from_scalars, b.slice_hist);
    hipLaunchKernelGGL(frw::nmsm_plan_kernel, dim3((unsigned)cnt), dim3(frw::NMSM_BUCKETS), 0, st, b.slice_hist, b.counts, b.offsets, b.item_first, b.items,
                       b.item_count, b.target, b.max_items, slices);
    hipLaunchKernelGGL(frw::msm_sort_scatter_kernel<frw::NarrowTableDigits>, sgrid, dim3(1024), 0, st, n, from_scalars, b.offsets, b.slice_hist, b.entries);
    return hipGetLastError();
}
// ... of ONE scalar vector for bare handles: all thirty-two windows in one pass (`b` from frw::nmsm_layout_bare)
// `index`: the sum is over the scalars (and rows) index[0 .. n) of `sc` (null: over 0 .. n)
hipError_t nmsm_sort_bare(const NmsmBufs &b, uint32_t n, const uint32_t *sc, int montgomery, hipStream_t st, const uint32_t *index = nullptr)
{
    const uint32_t slices = frw::nmsm_slices(n);
    hipError_t e = hipMemsetAsync(b.ones_count, 0, 16, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(frw::nmsm_hist_bare_kernel, dim3(slices), dim3(1024), 0, st, n, sc, montgomery, b.slice_hist, b.ones_count, b.ones_list, index);
    hipLaunchKernelGGL(frw::nmsm_plan_kernel, dim3(frw::NMSM_W), dim3(frw::NMSM_BUCKETS), 0, st, b.slice_hist, b.counts, b.offsets, b.item_first, b.items,
                       b.item_count, b.target, b.max_items, slices);
    hipLaunchKernelGGL(frw::nmsm_entry_base_kernel, dim3(1), dim3(64), 0, st, b.counts, b.offsets, b.entry_base);
    hipLaunchKernelGGL(frw::nmsm_scatter_bare_kernel, dim3(slices), dim3(1024), 0, st, n, sc, montgomery, b.offsets, b.slice_hist, b.entry_base, b.entries,
                       index);
    return hipGetLastError();
}
// ---- what both forms of the narrow sums share ----
// the tables of one launch side by side (NmsmTables); with_ones_tables: the sort left a mask of the ones, not a list
frw::NmsmTables nmsm_tables(const frw_msm *const *ms, int tables, uint32_t n, uint32_t sigs, bool with_ones_tables)
{
    frw::NmsmTables dev;
    dev.n = n; dev.sigs = sigs;
    for (int t = 0; t < 3; t++) {
        const frw_msm *m = ms[t < tables ? t : 0];
        dev.table[t] = m->dev.table;
        dev.ones_table[t] = with_ones_tables ? m->dev.ones_table : nullptr;
    }
    return dev;
}
// two lanes per point (G2): WITHOUT the prefetch of the next row the bucket kernel is 249 registers = two waves per SIMD; with it 256 + 26
// AGPRs = one (round 4 ran it that way).  FRW_G2_PREFETCH in the environment brings the prefetch back (the A/B of profiles/r05_g2_*).
bool g2_prefetch()
{
    static const bool v = std::getenv("FRW_G2_PREFETCH") != nullptr;
    return v;
}
// the work items' sums of `rows` grid rows; entry_base: a bare handle's windows, else null
template <class FB, bool PREFETCH>
void nmsm_launch_bucket(const frw::NmsmTables &dev, unsigned rows, const NmsmBufs &sorted, uint32_t *partial_items, const unsigned long long *entry_base, hipStream_t st)
{
    const dim3 grid((sorted.max_items * FB::LANES + 63) / 64, rows);
    if (PREFETCH || (FB::LANES > 1 && g2_prefetch()))
        hipLaunchKernelGGL((frw::nmsm_bucket_kernel<FB, true>), grid, dim3(64), 0, st, dev, sorted.offsets, sorted.counts, sorted.items, sorted.item_count,
                           sorted.entries, partial_items, sorted.target, sorted.max_items, entry_base);
    else
        hipLaunchKernelGGL((frw::nmsm_bucket_kernel<FB, false>), grid, dim3(64), 0, st, dev, sorted.offsets, sorted.counts, sorted.items, sorted.item_count,
                           sorted.entries, partial_items, sorted.target, sorted.max_items, entry_base);
}
// The sums of the scalars that are one, `threads` threads for each of `rows` grid rows (row y reads the tables' row y row_step): one partial
// sum per 64 threads, and more than 64 of those brought down to 64 by a second kernel.  Returns what the fold is to read.
struct OnesSums { const uint32_t *sums; uint32_t groups, stride; };
template <class FB>
OnesSums nmsm_launch_ones(const frw::NmsmTables &dev, uint32_t threads, unsigned rows, uint32_t row_step, const NmsmBufs &sorted, const NmsmBufs &own, hipStream_t st)
{
    hipLaunchKernelGGL(frw::nmsm_ones_kernel<FB>, dim3(threads / 64, rows), dim3(64), 0, st, dev, sorted.ones_count, sorted.ones_list, own.partial_ones,
                       own.ones_stride, row_step);
    if (threads / 64 <= 64) return OnesSums{own.partial_ones, threads / 64, own.ones_stride};
    hipLaunchKernelGGL(frw::nmsm_ones_fold_kernel<FB>, dim3(64, rows), dim3(64), 0, st, own.partial_ones, threads / 64, own.ones_stride, own.folded_ones);
    return OnesSums{own.folded_ones, 64, 64};
}
// `sorted`: whose sort arrays to read; `own`: where the tables' partial sums go -- carved for `tables * cnt` signatures when there is
// more than one table (the same carve as `sorted` for a sum on its own); d_out: [tables][cnt] results.  Every kernel here is a grid of
// single wavefronts: none of them can be kept waiting by a kernel that fills the chip.
// ones_stream / ones_done: the sums of the scalars that are one need nothing of the work items' sums and the other way round -- as two
// launches on one stream the second waited for the first.  A caller with a second stream that is ordered after the sort (and an event
// to spare) gives it here: the ones are summed there, `st` waits for them before the fold (a quarter of a millisecond off the chain of
// a proof made alone).
template <class F, bool PREFETCH>
hipError_t nmsm_accumulate(const frw_msm *const *ms, int tables, const NmsmBufs &sorted, const NmsmBufs &own, size_t cnt, uint32_t *d_out, bool ones_as_mask,
                           hipStream_t st, bool xyzz_out = false, bool ones_elsewhere = false, hipStream_t ones_stream = nullptr, hipEvent_t ones_done = nullptr)
{
    if (!ones_elsewhere) ones_stream = st;                          // (a caller's stream may be the null stream: the flag says whether it was given)
    const uint32_t n = ms[0]->dev.n;
    const frw::NmsmTables dev = nmsm_tables(ms, tables, n, (uint32_t)cnt, ones_as_mask);
    const unsigned rows = (unsigned)(cnt * (size_t)tables);
    typedef typename frw::BulkPolicy<F>::type FB;
    // the ones' partial sums: enough threads to occupy the chip (~2^16 over the batch), between 256 and 4,096 per signature
    uint32_t ones_threads = 256;
    while (ones_threads < frw::nmsm_ones_max(n) && (size_t)ones_threads * rows < 65536) ones_threads <<= 1;
    const OnesSums ones = nmsm_launch_ones<FB>(dev, ones_threads, rows, 1u, sorted, own, ones_stream);
    if (ones_elsewhere) {
        const hipError_t e = hipEventRecord(ones_done, ones_stream);
        if (e != hipSuccess) return e;
    }
    nmsm_launch_bucket<FB, PREFETCH>(dev, rows, sorted, own.partial_items, nullptr, st);
    // the items of a bucket: added up by a workgroup per bucket where latency counts (a lone proof: 12 ms -> 8.6), by the fold's own
    // thread where throughput does (the combine is nine times the wave-level additions: 3 % of a 64-proof call)
    const bool combine = cnt <= 16;
    if (combine)
        hipLaunchKernelGGL(frw::nmsm_combine_kernel<FB>, dim3(frw::NMSM_BUCKETS, rows), dim3(64), 0, st, sorted.counts, sorted.offsets, sorted.item_first,
                           own.partial_items, own.bucket_sums, sorted.target, sorted.max_items, (uint32_t)cnt);
    if (ones_elsewhere) {
        const hipError_t e = hipStreamWaitEvent(st, ones_done, 0);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(frw::nmsm_finish_kernel<FB>, dim3(rows), dim3(64), 0, st, sorted.counts, sorted.offsets, sorted.item_first, own.partial_items,
                       combine ? own.bucket_sums : (uint32_t *)nullptr, ones.sums, (int)ones.groups, ones.stride, sorted.target, sorted.max_items,
                       d_out, xyzz_out ? 1 : 0, (uint32_t)cnt, 0);
    return hipGetLastError();
}
// The sums of ONE scalar vector over `tables` bare handles that share its sort (`b` from frw::nmsm_layout_bare(.., tables, n, ..): the sort's
// arrays and the tables' own): grid row = (table, window); a window's buckets are cut into work items, combined by a workgroup per bucket
// (the low windows hold every small value of a witness: a bucket of 250,000 entries is a thousand items), folded by one wavefront per
// (table, window); the scalars equal to one -- a list -- are summed by up to 65,536 threads per table and join window 0; Horner's rule
// over the thirty-two window sums.  d_out: [tables] results.
template <class F, bool PREFETCH>
hipError_t nmsm_accumulate_bare(const frw_msm *const *ms, int tables, const NmsmBufs &b, uint32_t *d_out, hipStream_t st, bool xyzz_out, uint32_t out_step = 1)
{
    // (b.n is the sort's: the tables' rows, or those an index names)
    const frw::NmsmTables dev = nmsm_tables(ms, tables, b.n, frw::NMSM_W, false);
    const unsigned rows = (unsigned)tables * frw::NMSM_W;
    typedef typename frw::BulkPolicy<F>::type FB;
    // the ones: 4,096 threads per table, or 65,536 beyond 2^18 points; grid row y is (table y, window 0), the only window with ones
    const OnesSums ones = nmsm_launch_ones<FB>(dev, frw::nmsm_ones_max(b.n), (unsigned)tables, (uint32_t)frw::NMSM_W, b, b, st);
    nmsm_launch_bucket<FB, PREFETCH>(dev, rows, b, b.partial_items, (const unsigned long long *)b.entry_base, st);
    hipLaunchKernelGGL(frw::nmsm_combine_kernel<FB>, dim3(frw::NMSM_BUCKETS, rows), dim3(64), 0, st, b.counts, b.offsets, b.item_first,
                       b.partial_items, b.bucket_sums, b.target, b.max_items, (uint32_t)frw::NMSM_W);
    hipLaunchKernelGGL(frw::nmsm_finish_kernel<FB>, dim3(rows), dim3(64), 0, st, b.counts, b.offsets, b.item_first, b.partial_items,
                       b.bucket_sums, ones.sums, (int)ones.groups, ones.stride, b.target, b.max_items,
                       b.window_sums, 1, (uint32_t)frw::NMSM_W, 1);
    hipLaunchKernelGGL(frw::msm_horner_kernel<FB>, dim3((unsigned)tables), dim3(64), 0, st, b.window_sums, frw::NMSM_W, frw::NMSM_C, d_out, xyzz_out ? 1 : 0,
                       out_step);
    return hipGetLastError();
}
// the narrow pipeline for one group
template <class F, bool PREFETCH>
int nmsm_run(const frw_msm *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, int montgomery, uint64_t *d_out,
             void *d_workspace, size_t workspace_bytes, hipStream_t st)
{
    const uint32_t n = m->dev.n;
    const size_t per = frw::nmsm_workspace_per_signature(n, m->bare, frw::Grp<F>::BK_WORDS);
    size_t chunk = workspace_bytes / per;
    if (chunk == 0 || ((uintptr_t)d_workspace & 15)) return FRW_E_INVALID_ARG;
    if (chunk > 32768) chunk = 32768;                                  // grid.y
    hipError_t e = hipSetDevice(m->device);
    if (m->bare) {
        const NmsmBufs b = frw::nmsm_layout_bare(d_workspace, 1, n, frw::Grp<F>::BK_WORDS);
        for (size_t sig = 0; e == hipSuccess && sig < batch; sig++) {
            e = nmsm_sort_bare(b, n, (const uint32_t *)(d_scalars + sig * scalar_stride * 4), montgomery, st);
            if (e == hipSuccess) e = nmsm_accumulate_bare<F, PREFETCH>(&m, 1, b, (uint32_t *)(d_out + sig * (frw::Grp<F>::ARK_WORDS / 2)), st, false);
        }
        return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_msm_dev");
    }
    for (size_t lo = 0; e == hipSuccess && lo < batch; lo += chunk) {
        const size_t cnt = batch - lo < chunk ? batch - lo : chunk;
        const NmsmBufs b = frw::nmsm_layout(d_workspace, cnt, n, frw::Grp<F>::BK_WORDS);
        e = nmsm_sort(b, n, cnt, (const uint32_t *)(d_scalars + lo * scalar_stride * 4), scalar_stride * 8, montgomery, m->ones_table != nullptr, st);
        if (e == hipSuccess)
            e = nmsm_accumulate<F, PREFETCH>(&m, 1, b, b, cnt, (uint32_t *)(d_out + lo * (frw::Grp<F>::ARK_WORDS / 2)), m->ones_table != nullptr, st);
    }
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_msm_dev");
}
}  // namespace

extern "C" void frw_msm_free(frw_msm *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->table) (void)hipFree(m->table);
    if (m->ones_table) (void)hipFree(m->ones_table);
    delete m;
}

extern "C" int frw_msm_g1_load(int device, size_t num_points, const uint64_t *bases, frw_msm **out)
{
    return msm_load<FqField>(device, 1, num_points, bases, 16, false, out);
}
extern "C" int frw_msm_g1_load_narrow(int device, size_t num_points, const uint64_t *bases, frw_msm **out)
{
    return msm_load<FqField>(device, 1, num_points, bases, 8, false, out);
}
extern "C" int frw_msm_g2_load_narrow(int device, size_t num_points, const uint64_t *bases, frw_msm **out)
{
    return msm_load<Fq2Field>(device, 2, num_points, bases, 8, false, out);
}
extern "C" int frw_msm_g2_load(int device, size_t num_points, const uint64_t *bases, frw_msm **out)
{
    return msm_load<Fq2Field>(device, 2, num_points, bases, 16, false, out);
}
extern "C" int frw_msm_g1_load_bare(int device, size_t num_points, const uint64_t *bases, int narrow, frw_msm **out)
{
    if (narrow < 0 || narrow > 2) return FRW_E_INVALID_ARG;
    return msm_load<FqField>(device, 1, num_points, bases, narrow == 1 ? 8 : 16, true, out, narrow == 2);
}
extern "C" int frw_msm_g2_load_bare(int device, size_t num_points, const uint64_t *bases, int narrow, frw_msm **out)
{
    if (narrow < 0 || narrow > 2) return FRW_E_INVALID_ARG;
    return msm_load<Fq2Field>(device, 2, num_points, bases, narrow == 1 ? 8 : 16, true, out, narrow == 2);
}
extern "C" int frw_g1_fixed_base(int device, size_t count, const uint64_t *scalars, uint64_t *out)
{
    return fixed_base<FqField>(device, count, scalars, out);
}
extern "C" int frw_g2_fixed_base(int device, size_t count, const uint64_t *scalars, uint64_t *out)
{
    return fixed_base<Fq2Field>(device, count, scalars, out);
}

extern "C" int frw_msm_info(const frw_msm *m, frw_msm_info_t *out)
{
    if (!m || !out) return FRW_E_INVALID_ARG;
    const bool g2 = m->group == 2;
    out->num_points = m->dev.n;
    const bool narrow = m->window_bits == 8;
    out->window_bits = m->wide ? frw::WIDE_C : m->window_bits;
    out->num_windows = m->wide ? frw::WIDE_W : 256 / m->window_bits;
    out->table_bytes = (uint64_t)(m->bare ? 1 : out->num_windows) * m->dev.n * (g2 ? frw::Grp<Fq2Field>::PT_WORDS : frw::Grp<FqField>::PT_WORDS) * 4;
    if (m->ones_table) out->table_bytes += (uint64_t)((m->dev.n + 7) / 8) * 255 * (g2 ? frw::Grp<Fq2Field>::PT_WORDS : frw::Grp<FqField>::PT_WORDS) * 4;
    const uint32_t n = m->dev.n;
    const bool bare = m->bare;
    const size_t bw = g2 ? frw::G2_BK_WORDS : frw::G1_BK_WORDS;
    out->workspace_bytes_per_signature = narrow ? frw::nmsm_workspace_per_signature(n, bare, bw) : frw::msm_workspace_per_signature(n, bare, m->wide, bw);
    return FRW_OK;
}

// the sums of one group's handle: PREFETCH is G1's (G2 has no registers to spare for the next row)
template <class F, bool PREFETCH>
static int msm_dev(int group, const frw_msm *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, int montgomery, uint64_t *d_out,
                   void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!m || m->group != group || (batch && (!d_scalars || !d_out || !d_workspace)) || scalar_stride < m->dev.n) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (m->window_bits == 8) return nmsm_run<F, PREFETCH>(m, batch, d_scalars, scalar_stride, montgomery, d_out, d_workspace, workspace_bytes, (hipStream_t)stream);
    return msm_run<F, PREFETCH>(m, batch, d_scalars, scalar_stride, montgomery, d_out, d_workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int frw_msm_g1_dev(const frw_msm *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, int montgomery,
                              uint64_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return msm_dev<FqField, true>(1, m, batch, d_scalars, scalar_stride, montgomery, d_out, d_workspace, workspace_bytes, stream);
}
extern "C" int frw_msm_g2_dev(const frw_msm *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, int montgomery,
                              uint64_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return msm_dev<Fq2Field, false>(2, m, batch, d_scalars, scalar_stride, montgomery, d_out, d_workspace, workspace_bytes, stream);
}

extern "C" int frw_groth16_msm_h_dev(const frw_msm *m, size_t batch, const uint64_t *d_h, size_t domain_size, uint64_t *d_out,
                                     void *d_workspace, size_t workspace_bytes, void *stream)
{
    // prover.rs: the scalars are h's coefficients 0 .. n - 2 (h_query has n - 1 points; the zip drops the last coefficient)
    if (!m || (size_t)m->dev.n + 1 != domain_size) return FRW_E_INVALID_ARG;
    return frw_msm_g1_dev(m, batch, d_h, domain_size, 1, d_out, d_workspace, workspace_bytes, stream);
}

// ---- a whole Groth16 proof per signature, on the device ------------------------------------------------------------------------------
// ark-groth16 0.3.0 prover.rs, create_proof_with_reduction_and_matrices (what examples/pok_sig.rs:30-47 of the reference runs),
// for every signature of a resident batch of witnesses:
//     h    = witness_map(...)                                                   frw_qap_witness_map_dev
//     g_a  = r delta_g1 + a_query[0] + MSM(a_query[1..], assignment) + alpha_g1      one sum over  a_query ++ [alpha, delta1]   with z ++ [1, r]
//     g1_b = s delta_g1 + b_g1_query[0] + MSM(b_g1_query[1..], ...) + beta_g1        the sum over  b_g1_query ++ [beta1]        with z ++ [1]   (g1_b - s delta1)
//     g2_b = s delta_g2 + b_g2_query[0] + MSM(b_g2_query[1..], ...) + beta_g2        one sum over  b_g2_query ++ [beta2, O, delta2]  with z ++ [1, r, s]
//     g_c  = s g_a + r g1_b - r s delta_g1 + MSM(l_query, aux) + MSM(h_query, h)  =  L + H + s g_a + r (g1_b - s delta1)
// z = instance_assignment ++ witness_assignment (z[0] = 1 is the scalar of query[0]); the blinding terms ride in the sums as
// extra points, the two scalar multiplications of g_c are done by four lanes each at the end (frw_quad.h).
namespace frw {
// 2^517 mod p in nine 29-bit limbs: f29_mul(x, 2^517) = x 2^256, the Montgomery form of a canonical scalar
__device__ const uint32_t FR_TO_MONT[NL29] = {0x1e538d9eu, 0x19e99103u, 0x13b31eccu, 0x04e2d5e4u, 0x181dac62u, 0x115f1ba1u,
                                              0x1e414fbbu, 0x11b3009cu, 0x00013fecu};
// the tail of every signature's scalar vector: [1, r, s] in Montgomery form after the nv assignment values
__global__ __launch_bounds__(64) void groth16_tails_kernel(size_t batch, const uint32_t *__restrict__ rs /* [batch][2][8] canonical */,
                                                           uint32_t *__restrict__ zext, size_t stride_words, size_t nv)
{
    const size_t sig = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (sig >= batch) return;
    uint32_t *dst = zext + sig * stride_words + nv * 8;
    constexpr uint32_t one[8] = FRW_R32;
    Fr8 o;
#pragma unroll
    for (int k = 0; k < 8; k++) o.l[k] = one[k];
    fr_store(dst, o);
    F29 c;
#pragma unroll
    for (int k = 0; k < NL29; k++) c.l[k] = FR_TO_MONT[k];
    for (int j = 0; j < 2; j++)
        fr_store(dst + 8 * (j + 1), f29_pack(f29_canonical(f29_mul(f29_unpack(fr_load(rs + (sig * 2 + j) * 8)), c))));
}
// k (any 256-bit value; taken mod the group order r) = k0 + lambda k1, lambda = z^2 - 1 = 0xac45a4010001a40200000000ffffffff,
// r = lambda^2 + lambda + 1: k0 = k mod lambda, k1 = k div lambda <= lambda + 1 < 2^128 -- for both blinding factors of every proof,
// one thread each (plain schoolbook division, a bit at a time: two scalars per proof).  out: [batch][2][k0 (2 x u64) | k1 (2 x u64)].
// On the device so that a call with its blinding factors in device memory never waits on the host (frw_groth16_prove_rs_dev).
__global__ __launch_bounds__(64) void groth16_split_kernel(size_t count, const uint64_t *__restrict__ rs /* [count][4] */, uint64_t *__restrict__ out /* [count][4] */)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    const uint64_t L0 = 0x00000000ffffffffULL, L1 = 0xac45a4010001a402ULL;
    uint64_t k[4] = {rs[i * 4], rs[i * 4 + 1], rs[i * 4 + 2], rs[i * 4 + 3]};
    for (int round = 0; round < 2; round++) {                       // 2^256 < 3 r: at most two subtractions
        bool ge = true;
        for (int j = 3; j >= 0; j--)
            if (k[j] != R[j]) { ge = k[j] > R[j]; break; }
        if (!ge) break;
        uint64_t borrow = 0;
        for (int j = 0; j < 4; j++) {
            const uint64_t d = k[j] - R[j], d2 = d - borrow;
            borrow = (k[j] < R[j]) | (d < borrow);
            k[j] = d2;
        }
    }
    uint64_t r0 = 0, r1 = 0, q0 = 0, q1 = 0;
    for (int bit = 255; bit >= 0; bit--) {
        const uint64_t top = r1 >> 63;
        r1 = (r1 << 1) | (r0 >> 63);
        r0 = (r0 << 1) | ((k[bit >> 6] >> (bit & 63)) & 1ULL);
        q1 = (q1 << 1) | (q0 >> 63);                                 // k < r: the quotient's bits above 127 are zero
        q0 <<= 1;
        if (top || r1 > L1 || (r1 == L1 && r0 >= L0)) {
            const uint64_t b = r0 < L0;
            r0 -= L0;
            r1 = r1 - L1 - b;
            q0 |= 1ULL;
        }
    }
    out[i * 4] = r0; out[i * 4 + 1] = r1; out[i * 4 + 2] = q0; out[i * 4 + 3] = q1;
}
// k P for one point per signature (s g_a and r (g1_b - s delta1) of g_c); runs on the side stream that made P.  A point that exists
// only now: the chain of doublings is the latency of a proof made alone, so the scalar comes split by the endomorphism
// (k = k0 + lambda k1: groth16_split_kernel) and the two 128-bit halves share their doublings: 128
// doublings and ~96 additions of P, phi(P) or P + phi(P) instead of 256 and ~128.  P arrives in XYZZ coordinates as its sum left it
// and k P leaves the same way (the proof needs one inversion, at the very end: groth16_finish_kernel).  phi(P) and P + phi(P) come
// for free in the same denominators -- phi(x, y) = (beta x, y), and since the two have the same y their chord is horizontal:
// P + phi(P) = (-(1 + beta) x, -y) -- so a step is ONE doubling and ONE addition whose operand is selected.  (Until late in round 4
// one thread per scalar multiplication ran this loop with the one-lane formulas of frw_fq29.h: 3.1 ms of a lone proof's 5.6.)
// On FOUR lanes (frw_quad.h): the formulas' independent products side by side -- three dependent levels per
// doubling instead of nine products, four per addition instead of fourteen -- with the results in a register file in LDS.  One
// quad per workgroup: its lanes take the same branches (they depend on the scalar's bits and on zero tests every lane sees
// alike), so nothing diverges, and a batch of scalar multiplications spreads over as many SIMDs.
struct QuadLaneExec {
    uint32_t *lds;
    uint32_t lane;
    // LDS serves a wavefront's requests in order; what must not happen is the COMPILER moving a level's reads above the previous
    // level's writes (per lane they touch different slots)
    static __device__ __forceinline__ void fence()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    static __device__ __forceinline__ uint32_t from_lane0(uint32_t x)
    {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x00 /* quad_perm [0, 0, 0, 0] */, 0xf, 0xf, true);
    }
    template <const quad::Step &S> __device__ __forceinline__ void step(uint32_t qx, uint32_t qy)
    {
        Fq29 a;
        const Fq29 r = quad::compute<S>(lds, lane, qx, qy, a);
        quad::store<S>(lds, lane, r);
        fence();
    }
    template <const quad::Step &S> __device__ __forceinline__ void step_test(uint32_t qx, uint32_t qy, bool &pz)
    {
        Fq29 a;
        const Fq29 r = quad::compute<S>(lds, lane, qx, qy, a);
        quad::store<S>(lds, lane, r);
        fence();
        pz = from_lane0(fq_is_zero(a) ? 1u : 0u) != 0;
    }
    __device__ __forceinline__ bool degenerate(uint32_t qx, uint32_t qy)
    {
        uint32_t inf = 0;
        if (lane == 0) inf = quad::add_degenerate(lds, qx, qy) ? 1u : 0u;
        fence();
        return from_lane0(inf) != 0;
    }
};
// Both scalar multiplications of a batch in one launch: workgroup b < batch is s g_a of signature b (the second scalar of its pair),
// workgroup batch + b is r (g1_b - s delta1) (the first); pts = [2][batch] points as the sums left them, out likewise.
__global__ __launch_bounds__(4) void groth16_scale_quad_kernel(size_t batch, const uint32_t *__restrict__ split /* [batch][2][8]: k0 | k1, 128 bits each */,
                                                               const uint32_t *__restrict__ pts /* [2][batch][BK_WORDS] */,
                                                               uint32_t *__restrict__ out /* [2][batch][BK_WORDS] */)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    typedef FqField F;
    constexpr int BW = Grp<F>::BK_WORDS;
    __shared__ __attribute__((aligned(16))) uint32_t file[quad::NSLOTS * quad::SLOT_WORDS];
    const size_t slot = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (slot >= 2 * batch) return;
    const size_t sig = slot < batch ? slot : slot - batch;
    const int which = slot < batch ? 1 : 0;
    if (pts[slot * BW + 4 * F::WORDS] != 0) {                                              // k O = O
        if (lane == 0) store_bucket<F>(out + slot * BW, pt_identity<F>());
        return;
    }
    if (lane == 0) quad::setup(file, load_bucket<F>(pts + slot * BW));
    QuadLaneExec::fence();
    const uint32_t *k = split + (sig * 2 + which) * 8;
    uint32_t k0[4], k1[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { k0[i] = k[i]; k1[i] = k[4 + i]; }
    QuadLaneExec ex{file, lane};
    const bool inf = quad::scalar_mul(ex, k0, k1);
    if (lane == 0) store_bucket<F>(out + slot * BW, inf ? pt_identity<F>() : quad::running_point(file, false));
}
// (A/B, negative, round 4: a workgroup of three wavefronts per scalar multiplication -- one running the 128 doublings from the LOW end
// of the scalar and parking 2^i P in LDS, two adding the parked points where k0 / k1 have bits set, a tree, phi on the k1 sum -- is
// bit-exact and SLOWER for a proof made alone, in two builds (the second with nothing but the doubled point live in the doubler's loop
// and the doubling inlined): 5.5 and 4.9 ms against the 3.3 ms of the chain above; profiles/r04_groth16_scale_wave_ab.txt.  Removed.)
// C = L + H + s A + r B1', then the proof row A (12 u64) | B (24) | C (12).  TWO lanes per proof: the even one adds up C, the odd one
// holds A, and both turn their XYZZ point into ark-ff's affine bytes at once -- the one inversion on a proof's critical path
// (the sums and the scalar multiplications hand their results over in XYZZ coordinates).
__global__ __launch_bounds__(64) void groth16_finish_kernel(size_t batch, const uint32_t *__restrict__ a_pts, const uint32_t *__restrict__ sa_pts,
                                                            const uint32_t *__restrict__ rb1_pts, const uint32_t *__restrict__ l_pts,
                                                            const uint32_t *__restrict__ h_pts /* all five [batch][BK_WORDS] */,
                                                            const uint32_t *__restrict__ b2_pts /* [batch][48], affine */,
                                                            uint32_t *__restrict__ proofs /* [batch][96] */)
{
    __builtin_amdgcn_s_setprio(2);                               // latency, not throughput: ahead of a chip-filling bucket kernel's waves on the same SIMD
    typedef FqField F;
    constexpr int BW = Grp<F>::BK_WORDS;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x, sig = t >> 1;
    const bool holds_a = (t & 1) != 0;
    if (sig >= batch) return;
    XyzzT<F> acc = load_bucket<F>((holds_a ? a_pts : l_pts) + sig * BW);
#pragma nounroll
    for (int j = 0; j < 3; j++) {
        const uint32_t *p = j == 0 ? h_pts : j == 1 ? sa_pts : rb1_pts;
        if (!holds_a) acc = pt_add(acc, load_bucket<F>(p + sig * BW));
    }
    uint32_t *o = proofs + sig * 96;
    if (!holds_a)
        for (int k = 0; k < 48; k++) o[24 + k] = b2_pts[sig * 48 + k];
    store_ark_point<F>(o + (holds_a ? 0 : 72), pt_to_affine(acc));
}
// ---- a key in slices (round 5): every rank sums its slice of every query; the five partial sums of a rank leave as ark-ff's affine
// bytes -- A | B1' | L | H (G1, 12 u64 each) | B (G2, 24) -- and any rank puts `world` of them together
__global__ __launch_bounds__(64) void groth16_partial_kernel(const uint32_t *__restrict__ g1_pts /* [4][BK_WORDS]: A, B1', L, H */,
                                                             const uint32_t *__restrict__ b2_ark /* [48] */, uint32_t *__restrict__ out /* [144] */)
{
    const uint32_t t = threadIdx.x;
    if (t < 4) store_ark_point<FqField>(out + t * 24, pt_to_affine(load_bucket<FqField>(g1_pts + t * Grp<FqField>::BK_WORDS)));
    else if (t < 4 + 48) out[96 + (t - 4)] = b2_ark[t - 4];
}
__global__ __launch_bounds__(64) void groth16_combine_kernel(uint32_t world, const uint32_t *__restrict__ partials /* [world][144] */,
                                                             uint32_t *__restrict__ g1_pts /* [4][BK_WORDS] */, uint32_t *__restrict__ b2_ark /* [48] */)
{
    const uint32_t t = threadIdx.x;
    if (t < 4) {
        XyzzT<FqField> acc = pt_identity<FqField>();
        for (uint32_t r = 0; r < world; r++) acc = pt_add_affine(acc, load_ark_point<FqField>(partials + (size_t)r * 144 + t * 24));
        store_bucket<FqField>(g1_pts + t * Grp<FqField>::BK_WORDS, acc);
    } else if (t == 4) {
        XyzzT<Fq2Field> acc = pt_identity<Fq2Field>();
        for (uint32_t r = 0; r < world; r++) acc = pt_add_affine(acc, load_ark_point<Fq2Field>(partials + (size_t)r * 144 + 96));
        store_ark_point<Fq2Field>(b2_ark, pt_to_affine(acc));
    }
}
}  // namespace frw

struct frw_groth16_pk {
    int device;
    uint64_t num_instance, num_witness, domain_size;
    frw_msm *h, *a, *b1, *l, *b2;
    // round 5: a key of bare handles (the points only: 83 GB for the 1,024-statement aggregate instead of 3.6 KB per variable), and a
    // key in slices: this handle holds rows [z_lo, z_hi) of the nv + 3 rows of the four witness-side tables and [h_lo, h_hi) of h_query
    bool bare = false;
    uint32_t rank = 0, world = 1;
    uint64_t z_lo = 0, z_hi = 0, h_lo = 0, h_hi = 0;
    // (bare) the rows of b_g2_query -- and with them of b_g1_query -- that hold a point, in order: the sums over these two tables are over
    // those rows only.  A variable that no constraint has on its B side has the point at infinity there: 41 % of a Falcon circuit's, and
    // with them half of a witness's ones and all its full-size values -- 114 M additions per table against 37.5 M (the 1,024-statement mix).
    uint32_t *b_index = nullptr;
    uint32_t b_rows = 0;
    // FOUR streams of the key's own, created one after the other -- as many as the device has hardware queues (HIP's default), so
    // that no two of them wait in line for the same queue.  `main`: the witness map + the sum over h_query; side[0]: the three G1
    // witness-side sums as one chain of kernels, then both scalar multiplications; side[2]: the sum over b_g2_query; side[1]: the G1
    // sums' ones when latency counts.  The caller's stream (a fifth stream on four queues: it shares one, which one is not ours to know)
    // sorts the scalars' digits, forks into the others by events and joins them again (frw_groth16_prove_dev has the order things are
    // enqueued in, and why).  Two things learnt from timelines (profiles/r03_groth16_timeline_64.txt, r04_groth16_timeline_64.txt,
    // r04_aggregate16_timeline.txt): when the caller's stream carried the witness map it sat behind a side stream's whole chain on a
    // shared queue (a quarter of the call); and a kernel whose workgroups have several wavefronts (the sorts' 1,024 threads) does not
    // start once the 2^18-point bucket kernel runs -- two wavefronts of 240 registers per SIMD leave no CU with room for such a
    // workgroup -- so the sort goes first and everything after it is grids of single wavefronts.
    hipStream_t main, side[3];
    hipEvent_t fork, sorted, ones_done, join[4];   // fork: the call's inputs are in place; sorted: the digits of its scalars too; join[3]: main
    std::mutex enqueue;         // the side streams and events are the key's: one call at a time puts its work on them
};

extern "C" void frw_groth16_pk_free(frw_groth16_pk *pk)
{
    if (!pk) return;
    for (frw_msm *m : {pk->h, pk->a, pk->b1, pk->l, pk->b2}) frw_msm_free(m);
    (void)hipSetDevice(pk->device);
    if (pk->b_index) (void)hipFree(pk->b_index);
    for (int i = 0; i < 4; i++) {
        if (i < 3 && pk->side[i]) (void)hipStreamDestroy(pk->side[i]);
        if (pk->join[i]) (void)hipEventDestroy(pk->join[i]);
    }
    if (pk->main) (void)hipStreamDestroy(pk->main);
    if (pk->fork) (void)hipEventDestroy(pk->fork);
    if (pk->sorted) (void)hipEventDestroy(pk->sorted);
    if (pk->ones_done) (void)hipEventDestroy(pk->ones_done);
    delete pk;
}

namespace {
// the key's own streams and events (see the struct)
int pk_create(int device, uint64_t ni, uint64_t nw, uint64_t n, frw_groth16_pk **out)
{
    frw_groth16_pk *pk = new (std::nothrow) frw_groth16_pk;
    if (!pk) return FRW_E_OUT_OF_MEMORY;
    pk->device = device;
    pk->num_instance = ni; pk->num_witness = nw; pk->domain_size = n;
    pk->h = pk->a = pk->b1 = pk->l = pk->b2 = nullptr;
    pk->fork = pk->sorted = pk->ones_done = nullptr;
    pk->main = nullptr;
    for (int i = 0; i < 4; i++) { if (i < 3) pk->side[i] = nullptr; pk->join[i] = nullptr; }
    pk->z_lo = 0; pk->z_hi = ni + nw + 3; pk->h_lo = 0; pk->h_hi = n - 1;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pk->fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pk->sorted, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pk->ones_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&pk->main, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; i++) {
        if (i < 3) e = hipStreamCreateWithFlags(&pk->side[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&pk->join[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        frw_groth16_pk_free(pk);
        return frw::record_hip_error(e, "frw_groth16_pk_load");
    }
    *out = pk;
    return FRW_OK;
}
// a bare handle with room for `rows` rows and nothing in them yet
template <class F> int msm_alloc_bare_t(int device, int group, int window_bits, size_t rows, uint64_t row_lo, frw_msm **out)
{
    if (!out || rows == 0 || rows >= ((size_t)1 << 31)) return FRW_E_INVALID_ARG;
    *out = nullptr;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    frw_msm *m = new (std::nothrow) frw_msm;
    if (!m) return FRW_E_OUT_OF_MEMORY;
    m->device = device; m->group = group; m->window_bits = window_bits; m->bare = true; m->row_lo = row_lo;
    m->wide = window_bits == 16 && rows >= msm_wide_from();
    m->table = nullptr; m->ones_table = nullptr;
    m->dev.n = (uint32_t)rows; m->dev.ones_table = nullptr;
    e = hipMalloc(&m->table, rows * frw::Grp<F>::PT_WORDS * 4);
    if (e != hipSuccess) { delete m; return frw::record_hip_error(e, "frw_msm: the key's rows"); }
    m->dev.table = (const uint32_t *)m->table;
    *out = m;
    return FRW_OK;
}
// rows [first, first + count) of a bare handle from `count` ark-ff points in HOST memory, a few megabytes at a time
template <class F> int msm_upload_rows(frw_msm *m, size_t first, size_t count, const std::function<const uint64_t *(size_t)> &point_of /* null: infinity */)
{
    constexpr size_t AW = frw::Grp<F>::ARK_WORDS / 2, CHUNK = (size_t)1 << 18;
    std::vector<uint64_t> stage(std::min(count, CHUNK) * AW);
    void *d_stage = nullptr;
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) e = hipMalloc(&d_stage, stage.size() * 8);
    for (size_t lo = 0; e == hipSuccess && lo < count; lo += CHUNK) {
        const size_t cnt = std::min(CHUNK, count - lo);
        for (size_t i = 0; i < cnt; i++) {
            const uint64_t *src = point_of(lo + i);
            if (src) std::memcpy(&stage[i * AW], src, AW * 8);
            else std::memset(&stage[i * AW], 0, AW * 8);
        }
        e = hipMemcpy(d_stage, stage.data(), cnt * AW * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(frw::msm_precompute_kernel<F>, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, nullptr, (uint32_t)cnt, (const uint32_t *)d_stage,
                           (uint32_t *)m->table + (first + lo) * frw::Grp<F>::PT_WORDS, 256);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (d_stage) (void)hipFree(d_stage);
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_groth16_pk_load: rows");
}
}  // namespace

namespace {
// a bare handle -> the handle with window tables over the same points (the bare one is freed)
template <class F> int msm_expand_tables_t(frw_msm **pm)
{
    frw_msm *b = *pm;
    const size_t n = b->dev.n;
    if (!b->bare || n > ((size_t)1 << (b->window_bits == 8 ? 25 : 26))) return FRW_E_INVALID_ARG;
    hipError_t e = hipSetDevice(b->device);
    frw_msm *m = new (std::nothrow) frw_msm;
    if (!m) return FRW_E_OUT_OF_MEMORY;
    m->device = b->device; m->group = b->group; m->window_bits = b->window_bits; m->bare = false; m->row_lo = 0;
    m->table = nullptr; m->ones_table = nullptr; m->dev.n = (uint32_t)n; m->dev.ones_table = nullptr;
    if (e == hipSuccess) e = hipMalloc(&m->table, (size_t)(256 / b->window_bits) * n * frw::Grp<F>::PT_WORDS * 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(frw::msm_precompute_rows_kernel<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, (uint32_t)n, (const uint32_t *)b->table,
                           (uint32_t *)m->table, b->window_bits);
        e = hipGetLastError();
    }
    if (e == hipSuccess && b->window_bits == 8 && n <= ((size_t)1 << 18)) {
        const size_t entries = (n + 7) / 8 * 255;
        e = hipMalloc(&m->ones_table, entries * frw::Grp<F>::PT_WORDS * 4);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(frw::msm_ones_table_kernel<F>, dim3((unsigned)((entries + 63) / 64)), dim3(64), 0, nullptr, (uint32_t)n,
                               (const uint32_t *)m->table, (uint32_t *)m->ones_table);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        frw_msm_free(m);
        return frw::record_hip_error(e, "frw_groth16_setup: window tables");
    }
    m->dev.table = (const uint32_t *)m->table;
    m->dev.ones_table = (const uint32_t *)m->ones_table;
    frw_msm_free(b);
    *pm = m;
    return FRW_OK;
}
}  // namespace

namespace frw {
int msm_expand_tables(frw_msm **m) { return (*m)->group == 1 ? msm_expand_tables_t<FqField>(m) : msm_expand_tables_t<Fq2Field>(m); }
// slice `rank` of `world` of `total` rows
void groth16_shard_range(uint64_t total, uint32_t rank, uint32_t world, uint64_t *lo, uint64_t *hi)
{
    if (world <= 1) { *lo = 0; *hi = total; return; }
    *lo = total / world * rank + std::min<uint64_t>(rank, total % world);
    *hi = *lo + total / world + (rank < total % world ? 1 : 0);
}
int msm_alloc_bare(int device, int group, int window_bits, size_t rows, uint64_t row_lo, frw_msm **out)
{
    return group == 1 ? msm_alloc_bare_t<FqField>(device, 1, window_bits, rows, row_lo, out)
                      : msm_alloc_bare_t<Fq2Field>(device, 2, window_bits, rows, row_lo, out);
}
// rows [first_row, first_row + count) of a bare handle from `count` ark-ff points in DEVICE memory (msm_upload_rows' device side without
// its host arrays: the wire-format key loader decodes into such a buffer); d_ark null: the point at infinity in every row.  On `st`.
hipError_t msm_fill_ark_dev(frw_msm *m, size_t first_row, size_t count, const uint32_t *d_ark, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    if (!m->bare || first_row + count > m->dev.n) return hipErrorInvalidValue;
    const size_t pw = m->group == 1 ? Grp<FqField>::PT_WORDS : Grp<Fq2Field>::PT_WORDS;
    uint32_t *rows = (uint32_t *)m->table + first_row * pw;
    if (!d_ark) return hipMemsetAsync(rows, 0, count * pw * 4, st);
    if (m->group == 1)
        hipLaunchKernelGGL(msm_precompute_kernel<FqField>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, (uint32_t)count, d_ark, rows, 256);
    else
        hipLaunchKernelGGL(msm_precompute_kernel<Fq2Field>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, (uint32_t)count, d_ark, rows, 256);
    return hipGetLastError();
}
// a handle's points as table rows -- a bare handle's rows, window 0 of a window table (msm_precompute_kernel) -- and how many; *group: 1 or 2
const uint32_t *msm_point_rows(const frw_msm *m, int *group, uint64_t *rows)
{
    *group = m->group;
    *rows = m->dev.n;
    return m->dev.table;
}
int fixed_base_gen_create(int device, FixedBaseGen *g)
{
    g->g1 = g->g2 = nullptr;
    hipError_t e = hipSetDevice(device);
    void *gens1 = nullptr, *gens2 = nullptr;
    if (e == hipSuccess) e = hipMalloc((void **)&g->g1, (size_t)FBW_WINDOWS * FBW_DIGITS * Grp<FqField>::PT_WORDS * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&g->g2, (size_t)FBW_WINDOWS * FBW_DIGITS * Grp<Fq2Field>::PT_WORDS * 4);
    if (e == hipSuccess) e = hipMalloc(&gens1, (size_t)FBW_WINDOWS * Grp<FqField>::PT_WORDS * 4);
    if (e == hipSuccess) e = hipMalloc(&gens2, (size_t)FBW_WINDOWS * Grp<Fq2Field>::PT_WORDS * 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fixed_base_window_gens_kernel<FqField>, dim3(1), dim3(64), 0, nullptr, (uint32_t *)gens1);
        hipLaunchKernelGGL(fixed_base_window_gens_kernel<Fq2Field>, dim3(1), dim3(64), 0, nullptr, (uint32_t *)gens2);
        hipLaunchKernelGGL(fixed_base_wide_table_kernel<FqField>, dim3(FBW_WINDOWS * FBW_DIGITS / 64), dim3(64), 0, nullptr, (const uint32_t *)gens1, g->g1);
        hipLaunchKernelGGL(fixed_base_wide_table_kernel<Fq2Field>, dim3(FBW_WINDOWS * FBW_DIGITS / 64), dim3(64), 0, nullptr, (const uint32_t *)gens2, g->g2);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (gens1) (void)hipFree(gens1);
    if (gens2) (void)hipFree(gens2);
    if (e != hipSuccess) { fixed_base_gen_free(g); return record_hip_error(e, "fixed-base tables"); }
    return FRW_OK;
}
void fixed_base_gen_free(FixedBaseGen *g)
{
    if (g->g1) (void)hipFree(g->g1);
    if (g->g2) (void)hipFree(g->g2);
    g->g1 = g->g2 = nullptr;
}
// rows [first_row, first_row + count) of a bare handle = d_scalars[i] x the group's generator (canonical scalars in device memory)
hipError_t msm_fill_fixed_base(frw_msm *m, const FixedBaseGen &g, size_t first_row, size_t count, const uint32_t *d_scalars, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    if (!m->bare || first_row + count > m->dev.n) return hipErrorInvalidValue;
    if (m->group == 1)
        hipLaunchKernelGGL((fixed_base_wide_kernel<FqField, false>), dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, count, d_scalars, (const uint32_t *)g.g1,
                           (uint32_t *)m->table + first_row * Grp<FqField>::PT_WORDS);
    else
        hipLaunchKernelGGL((fixed_base_wide_kernel<Fq2PairField, false>), dim3((unsigned)((count + 31) / 32)), dim3(64), 0, st, count, d_scalars,
                           (const uint32_t *)g.g2, (uint32_t *)m->table + first_row * Grp<Fq2Field>::PT_WORDS);
    return hipGetLastError();
}
// ... as ark-ff's affine bytes in device memory (the verifying key's points)
hipError_t fixed_base_ark_dev(const FixedBaseGen &g, int group, size_t count, const uint32_t *d_scalars, uint32_t *d_out, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    if (group == 1)
        hipLaunchKernelGGL((fixed_base_wide_kernel<FqField, true>), dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, count, d_scalars, (const uint32_t *)g.g1, d_out);
    else
        hipLaunchKernelGGL((fixed_base_wide_kernel<Fq2PairField, true>), dim3((unsigned)((count + 31) / 32)), dim3(64), 0, st, count, d_scalars,
                           (const uint32_t *)g.g2, d_out);
    return hipGetLastError();
}
// a key of bare handles from its five tables (ownership passes to the key, also on failure)
int groth16_pk_assemble(int device, uint64_t ni, uint64_t nw, uint64_t n, uint32_t rank, uint32_t world, frw_msm *h, frw_msm *a, frw_msm *b1, frw_msm *l,
                        frw_msm *b2, frw_groth16_pk **out)
{
    const bool bare = h->bare;
    frw_groth16_pk *pk = nullptr;
    const int rc = pk_create(device, ni, nw, n, &pk);
    if (rc != FRW_OK) {
        for (frw_msm *m : {h, a, b1, l, b2}) frw_msm_free(m);
        return rc;
    }
    pk->h = h; pk->a = a; pk->b1 = b1; pk->l = l; pk->b2 = b2;
    pk->bare = bare;
    pk->rank = rank; pk->world = world < 1 ? 1 : world;
    groth16_shard_range(ni + nw + 3, rank, pk->world, &pk->z_lo, &pk->z_hi);
    groth16_shard_range(n - 1, rank, pk->world, &pk->h_lo, &pk->h_hi);
    if (bare) {
        // the rows of b_g2_query that hold a point (b_g1_query's are the same variables': row nv + 2 -- delta_2 -- is the one more G2 has)
        const uint32_t rows = b2->dev.n, blocks = (rows + 1023) / 1024;
        uint32_t *counts = nullptr, live = 0;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc((void **)&counts, ((size_t)blocks + 1) * 4);
        if (e == hipSuccess) {
            constexpr int PW2 = Grp<Fq2Field>::PT_WORDS;
            hipLaunchKernelGGL(live_rows_kernel<PW2>, dim3(blocks), dim3(1024), 0, nullptr, (const uint32_t *)b2->dev.table, rows, counts, (uint32_t *)nullptr);
            hipLaunchKernelGGL(live_rows_scan_kernel, dim3(1), dim3(1024), 0, nullptr, counts, blocks, counts + blocks);
            e = hipMemcpy(&live, counts + blocks, 4, hipMemcpyDeviceToHost);
            // (a slice without a single point in these tables still sums something: row 0, the point at infinity)
            if (e == hipSuccess) e = hipMalloc((void **)&pk->b_index, (size_t)(live ? live : 1) * 4);
            if (e == hipSuccess) e = hipMemset(pk->b_index, 0, 4);
            if (e == hipSuccess && live) {
                hipLaunchKernelGGL(live_rows_kernel<PW2>, dim3(blocks), dim3(1024), 0, nullptr, (const uint32_t *)b2->dev.table, rows, counts, pk->b_index);
                e = hipDeviceSynchronize();
            }
            pk->b_rows = live ? live : 1;
        }
        if (counts) (void)hipFree(counts);
        if (e != hipSuccess) {
            frw_groth16_pk_free(pk);
            return record_hip_error(e, "frw_groth16_pk_load (the rows of b_g2_query that hold a point)");
        }
    }
    *out = pk;
    return FRW_OK;
}
void groth16_pk_counts(const frw_groth16_pk *pk, int *device, uint64_t *ni, uint64_t *nw, uint64_t *n)
{
    *device = pk->device;
    *ni = pk->num_instance; *nw = pk->num_witness; *n = pk->domain_size;
}
}  // namespace frw

extern "C" int frw_groth16_pk_load_opts(int device, const frw_groth16_pk_desc_t *d, const frw_groth16_key_opts_t *opts, frw_groth16_pk **out)
{
    if (!out || !d || !d->alpha_g1 || !d->beta_g1 || !d->delta_g1 || !d->beta_g2 || !d->delta_g2 || !d->a_query || !d->b_g1_query ||
        !d->b_g2_query || !d->h_query || !d->l_query || d->num_instance == 0 || d->domain_size < 2)
        return FRW_E_INVALID_ARG;
    *out = nullptr;
    const size_t ni = (size_t)d->num_instance, nv = (size_t)(d->num_instance + d->num_witness);
    int mode = opts ? opts->mode : FRW_KEY_AUTO;
    const uint32_t world = opts && opts->world > 1 ? opts->world : 1, rank = opts ? opts->rank : 0;
    if ((mode != FRW_KEY_AUTO && mode != FRW_KEY_TABLES && mode != FRW_KEY_BARE) || rank >= world) return FRW_E_INVALID_ARG;
    if (mode == FRW_KEY_AUTO) mode = world > 1 || nv > FRW_KEY_AUTO_TABLE_VARIABLES ? FRW_KEY_BARE : FRW_KEY_TABLES;
    if (mode == FRW_KEY_TABLES && world > 1) return FRW_E_INVALID_ARG;          // a key in slices is a key of bare handles
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    if (mode == FRW_KEY_BARE) {
        // rows [z_lo, z_hi) of the four witness-side tables (a_query ++ [alpha, delta, O], b_g1_query ++ [beta, O, O],
        // O x I ++ l_query ++ [O, O, O], b_g2_query ++ [beta2, O, delta2]) and [h_lo, h_hi) of h_query, as they are
        uint64_t z_lo, z_hi, h_lo, h_hi;
        frw::groth16_shard_range(nv + 3, rank, world, &z_lo, &z_hi);
        frw::groth16_shard_range((uint64_t)d->domain_size - 1, rank, world, &h_lo, &h_hi);
        if (z_hi == z_lo || h_hi == h_lo) return FRW_E_INVALID_ARG;             // more ranks than rows
        frw_msm *t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};          // h, a, b1, l, b2
        int rc = frw::msm_alloc_bare(device, 1, 16, h_hi - h_lo, h_lo, &t[0]);
        for (int k = 1; k < 5 && rc == FRW_OK; k++) rc = frw::msm_alloc_bare(device, k == 4 ? 2 : 1, 8, z_hi - z_lo, z_lo, &t[k]);
        try {
            if (rc == FRW_OK) rc = msm_upload_rows<FqField>(t[0], 0, h_hi - h_lo, [&](size_t i) { return d->h_query + 12 * (h_lo + i); });
            if (rc == FRW_OK)
                rc = msm_upload_rows<FqField>(t[1], 0, z_hi - z_lo, [&](size_t i) -> const uint64_t * {
                    const size_t g = z_lo + i;
                    return g < nv ? d->a_query + 12 * g : g == nv ? d->alpha_g1 : g == nv + 1 ? d->delta_g1 : nullptr;
                });
            if (rc == FRW_OK)
                rc = msm_upload_rows<FqField>(t[2], 0, z_hi - z_lo, [&](size_t i) -> const uint64_t * {
                    const size_t g = z_lo + i;
                    return g < nv ? d->b_g1_query + 12 * g : g == nv ? d->beta_g1 : nullptr;
                });
            if (rc == FRW_OK)
                rc = msm_upload_rows<FqField>(t[3], 0, z_hi - z_lo, [&](size_t i) -> const uint64_t * {
                    const size_t g = z_lo + i;
                    return g >= ni && g < nv ? d->l_query + 12 * (g - ni) : nullptr;
                });
            if (rc == FRW_OK)
                rc = msm_upload_rows<Fq2Field>(t[4], 0, z_hi - z_lo, [&](size_t i) -> const uint64_t * {
                    const size_t g = z_lo + i;
                    return g < nv ? d->b_g2_query + 24 * g : g == nv ? d->beta_g2 : g == nv + 2 ? d->delta_g2 : nullptr;
                });
        } catch (const std::exception &) {
            rc = FRW_E_OUT_OF_MEMORY;
        }
        if (rc != FRW_OK) {
            for (frw_msm *m : t) frw_msm_free(m);
            return rc;
        }
        return frw::groth16_pk_assemble(device, d->num_instance, d->num_witness, d->domain_size, rank, world, t[0], t[1], t[2], t[3], t[4], out);
    }
    frw_groth16_pk *pk = nullptr;
    int rc = pk_create(device, d->num_instance, d->num_witness, d->domain_size, &pk);
    if (rc != FRW_OK) return rc;
    try {
        // The four witness-side sums take the same scalars, z ++ [1, r, s] (nv + 3 of them), and so ONE sort of their digits: every
        // table has nv + 3 rows, the points that a sum does not have being the point at infinity (all-zero rows, which cost an
        // addition nothing): a_query ++ [alpha, delta, O], b_g1_query ++ [beta, O, O], O x I ++ l_query ++ [O, O, O], and
        // b_g2_query ++ [beta2, O, delta2].
        std::vector<uint64_t> g1(12 * (nv + 3)), g2(24 * (nv + 3), 0);
        std::fill(g1.begin(), g1.end(), 0);
        std::memcpy(g1.data(), d->a_query, nv * 96);
        std::memcpy(g1.data() + 12 * nv, d->alpha_g1, 96);
        std::memcpy(g1.data() + 12 * (nv + 1), d->delta_g1, 96);
        rc = frw_msm_g1_load_narrow(device, nv + 3, g1.data(), &pk->a);       // the four witness-side sums: narrow windows
        if (rc == FRW_OK) {
            std::fill(g1.begin(), g1.end(), 0);
            std::memcpy(g1.data(), d->b_g1_query, nv * 96);
            std::memcpy(g1.data() + 12 * nv, d->beta_g1, 96);
            rc = frw_msm_g1_load_narrow(device, nv + 3, g1.data(), &pk->b1);
        }
        if (rc == FRW_OK) {
            std::fill(g1.begin(), g1.end(), 0);
            std::memcpy(g1.data() + 12 * (size_t)d->num_instance, d->l_query, (size_t)d->num_witness * 96);
            rc = frw_msm_g1_load_narrow(device, nv + 3, g1.data(), &pk->l);
        }
        if (rc == FRW_OK) rc = frw_msm_g1_load(device, (size_t)d->domain_size - 1, d->h_query, &pk->h);
        if (rc == FRW_OK) {
            std::memcpy(g2.data(), d->b_g2_query, nv * 192);
            std::memcpy(g2.data() + 24 * nv, d->beta_g2, 192);                 // row nv + 1 stays the point at infinity (the scalar there is r)
            std::memcpy(g2.data() + 24 * (nv + 2), d->delta_g2, 192);
            rc = frw_msm_g2_load_narrow(device, nv + 3, g2.data(), &pk->b2);
        }
    } catch (const std::exception &) {
        rc = FRW_E_OUT_OF_MEMORY;
    }
    if (rc != FRW_OK) {
        frw_groth16_pk_free(pk);
        return rc;
    }
    *out = pk;
    return FRW_OK;
}
extern "C" int frw_groth16_pk_load(int device, const frw_groth16_pk_desc_t *d, frw_groth16_pk **out)
{
    const frw_groth16_key_opts_t opts = {FRW_KEY_TABLES, 0, 1};                // (as before round 5: window tables, whatever the size)
    return frw_groth16_pk_load_opts(device, d, &opts, out);
}
extern "C" const frw_msm *frw_groth16_pk_query(const frw_groth16_pk *pk, int which)
{
    if (!pk) return nullptr;
    return which == FRW_QUERY_H ? pk->h : which == FRW_QUERY_A ? pk->a : which == FRW_QUERY_B1 ? pk->b1 : which == FRW_QUERY_L ? pk->l
         : which == FRW_QUERY_B2 ? pk->b2 : nullptr;
}
extern "C" int frw_groth16_pk_info(const frw_groth16_pk *pk, frw_groth16_pk_info_t *out)
{
    if (!pk || !out) return FRW_E_INVALID_ARG;
    out->mode = pk->bare ? FRW_KEY_BARE : FRW_KEY_TABLES;
    out->rank = pk->rank; out->world = pk->world;
    out->z_lo = pk->z_lo; out->z_hi = pk->z_hi; out->h_lo = pk->h_lo; out->h_hi = pk->h_hi;
    out->key_bytes = 0;
    frw_msm_info_t mi;
    for (const frw_msm *m : {pk->h, pk->a, pk->b1, pk->l, pk->b2})
        if (frw_msm_info(m, &mi) == FRW_OK) out->key_bytes += mi.table_bytes;
    return FRW_OK;
}

namespace {
// what the prover's layouts (frw_layout.h) are made of: the bytes per signature of the witness map and of the sums over h_query, a_query,
// b_g1_query, l_query and b_g2_query, as their handles report them (ok = false: not a usable R1CS handle)
struct Groth16Parts { bool ok; size_t qap, domain, nv, msm[5]; uint32_t nz, b_rows; };
Groth16Parts groth16_parts(const frw_groth16_pk *pk, const frw_r1cs *r)
{
    Groth16Parts s{};
    frw_qap_info_t q;
    frw_msm_info_t mi;
    if (frw_qap_info(r, &q) != FRW_OK) return s;
    s.ok = true; s.qap = q.workspace_bytes_per_signature;
    s.domain = (size_t)pk->domain_size; s.nv = (size_t)(pk->num_instance + pk->num_witness);
    if (pk->bare) { s.nz = pk->a->dev.n; s.b_rows = pk->b_rows; }         // (the rows of this slice of the key, those b_g2_query holds a point in)
    int i = 0;
    for (const frw_msm *m : {pk->h, pk->a, pk->b1, pk->l, pk->b2}) { frw_msm_info(m, &mi); s.msm[i++] = mi.workspace_bytes_per_signature; }
    return s;
}
}  // namespace

extern "C" size_t frw_groth16_workspace_bytes(const frw_groth16_pk *pk, const frw_r1cs *r, size_t batch_in_flight)
{
    if (!pk || !r) return 0;
    const Groth16Parts s = groth16_parts(pk, r);
    if (!s.ok) return 0;
    if (pk->bare) return batch_in_flight ? frw::groth16_layout_bare(nullptr, s.qap, s.msm[0], s.domain, s.nv, s.nz, s.b_rows).bytes : 0;      // one statement at a time
    return frw::groth16_layout(nullptr, 1, s.qap, s.domain, s.nv, s.msm).bytes * batch_in_flight;
}

// (diagnostic: what the witness-side sums of a key of bare handles add up for the scalars z -- the benchmark prices its roofline with these)
extern "C" int frw_diag_groth16_side_counts(const frw_groth16_pk *pk, const uint64_t *d_z, void *d_workspace, size_t workspace_bytes, void *stream,
                                            uint64_t *out)
{
    if (!pk || !pk->bare || !d_z || !d_workspace || !out || ((uintptr_t)d_workspace & 255)) return FRW_E_INVALID_ARG;
    const uint32_t nz = pk->a->dev.n;
    frw::Carve c(d_workspace);
    const frw::Groth16Sides sides = frw::groth16_sides_layout(c, nz, pk->b_rows);
    const NmsmBufs &g1 = sides.g1, &gb = sides.gb;
    if ((size_t)((char *)gb.end - (char *)d_workspace) > workspace_bytes) return FRW_E_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSetDevice(pk->device);
    if (e == hipSuccess) e = nmsm_sort_bare(g1, nz, (const uint32_t *)d_z, 1, st);
    if (e == hipSuccess) e = nmsm_sort_bare(gb, pk->b_rows, (const uint32_t *)d_z, 1, st, pk->b_index);
    out[0] = pk->b_rows;
    for (int k = 0; k < 2 && e == hipSuccess; k++) {
        const NmsmBufs &b = k ? gb : g1;
        std::vector<uint32_t> counts((size_t)frw::NMSM_W * frw::NMSM_BUCKETS);
        uint32_t ones = 0;
        e = hipMemcpyAsync(counts.data(), b.counts, counts.size() * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&ones, b.ones_count, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        uint64_t total = 0;
        for (uint32_t c : counts) total += c;
        out[1 + 2 * k] = total;
        out[2 + 2 * k] = ones;
    }
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_diag_groth16_side_counts");
}

namespace {
// A key of bare handles: one statement at a time (its sums fill the chip by themselves: 2 x 10^9 bucket additions for the 1,024-statement
// aggregate).  The same five sums, the same streams; the sort of the scalars' digits is the bare handles' (thirty-two windows, one pass),
// shared by the three G1 tables -- one chain of kernels -- and the G2 table; the sum over h_query runs window by window.
// d_proofs: [batch][48] (a whole key), or d_partial: [batch][72] (a slice: the five partial sums, frw.h FRW_GROTH16_PARTIAL_WORDS).
int groth16_prove_bare(const frw_groth16_pk *pk, const frw_r1cs *r1cs, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                       const uint64_t *rs_host, const uint64_t *rs_dev, uint64_t *d_proofs, uint64_t *d_partial, uint32_t *d_num_unsatisfied,
                       void *d_workspace, size_t workspace_bytes, void *stream, bool args_only = false)
{
    const Groth16Parts parts = groth16_parts(pk, r1cs);
    const frw::Groth16BareBufs g = frw::groth16_layout_bare(d_workspace, parts.qap, parts.msm[0], parts.domain, parts.nv, parts.nz, parts.b_rows);     // (every statement's)
    if (workspace_bytes < g.bytes || ((uintptr_t)d_workspace & 255)) return FRW_E_INVALID_ARG;
    if (args_only) return FRW_OK;
    uint64_t *const h = g.h, *const zext = g.zext, *const pB2 = g.pts.B2, *const d_rs = g.pts.rs, *const d_split = g.pts.split;
    uint32_t *const pA = g.pts.A, *const pH = g.pts.H, *const pSA = g.pts.SA, *const pRB1 = g.pts.RB1;      // [A | B1' | L] [H] [s A | r B1']
    const NmsmBufs &g1 = g.sides.g1, &gb = g.sides.gb, &g2 = g.sides.g2;
    const size_t I = (size_t)pk->num_instance, W = (size_t)pk->num_witness, nv = I + W, n = (size_t)pk->domain_size, stride = nv + 3;
    const uint32_t nz = pk->a->dev.n;                                    // rows of this slice of the witness-side tables
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSetDevice(pk->device);
    int rc = FRW_OK;
    bool forked = false;
    std::unique_lock<std::mutex> lock(const_cast<frw_groth16_pk *>(pk)->enqueue, std::defer_lock);
    for (size_t b = 0; e == hipSuccess && rc == FRW_OK && b < batch; b++) {
        if (lock.owns_lock()) lock.unlock();
        const uint64_t *wit = d_witness + b * W * 4, *inst = d_instance + b * I * 4;
        const uint64_t *rs_now = rs_dev ? rs_dev + b * 8 : d_rs;
        if (rs_host) {
            e = hipMemcpyAsync(d_rs, rs_host + b * 8, 64, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) break;
        }
        lock.lock();
        hipLaunchKernelGGL(frw::groth16_split_kernel, dim3(1), dim3(64), 0, st, (size_t)2, rs_now, d_split);
        e = hipMemcpyAsync(zext, inst, I * 32, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(zext + I * 4, wit, W * 32, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(frw::groth16_tails_kernel, dim3(1), dim3(64), 0, st, (size_t)1, (const uint32_t *)rs_now, (uint32_t *)zext, stride * 8, nv);
        e = hipEventRecord(pk->fork, st);
        forked = true;
        if (e == hipSuccess) e = hipStreamWaitEvent(pk->main, pk->fork, 0);
        if (e != hipSuccess) break;
        // the sorts first, on the caller's stream (workgroups of 1,024 threads: they would not start under the bucket kernels): one over
        // all the slice's scalars for a_query and l_query, one over the rows that b_g1_query / b_g2_query hold a point in
        // (both before any sum starts: a sort's workgroups are 1,024 threads of 70 - 128 registers -- a whole CU's register file -- and
        // with the G2 sum's kernels already on the chip the long sort's scatter took 39 ms instead of 7: profiles/r05_witness_sorts.txt)
        e = nmsm_sort_bare(g1, nz, (const uint32_t *)(zext + pk->z_lo * 4), 1, st);
        if (e == hipSuccess) e = nmsm_sort_bare(gb, pk->b_rows, (const uint32_t *)(zext + pk->z_lo * 4), 1, st, pk->b_index);
        if (e != hipSuccess) break;
        e = hipEventRecord(pk->sorted, st);
        for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipStreamWaitEvent(pk->side[i], pk->sorted, 0);
        if (e != hipSuccess) break;
        // (the witness-side sums first: the witness map of a mixed aggregate is hundreds of launches, and what the one host thread enqueues
        // behind them starts that much later -- 50 ms of an idle chip at the head of the 1,024-statement proof, profiles/r05_aggregate1024_timeline.txt)
        // pA: [A | B1' | L]: a_query and l_query share a chain of kernels (rows 0 and 2), b_g1_query has the key's spare stream
        const frw_msm *g1s[2] = {pk->a, pk->l};
        e = nmsm_accumulate_bare<FqField, true>(g1s, 2, g1, pA, pk->side[0], true, 2);
        if (e != hipSuccess) break;
        e = nmsm_accumulate_bare<Fq2Field, false>(&pk->b2, 1, g2, (uint32_t *)pB2, pk->side[2], false);
        if (e != hipSuccess) break;
        e = nmsm_accumulate_bare<FqField, true>(&pk->b1, 1, gb, g.pts.B1, pk->side[1], true);
        if (e != hipSuccess) break;
        rc = frw_qap_witness_map_dev(r1cs, 1, wit, inst, h, d_num_unsatisfied ? d_num_unsatisfied + b : nullptr, g.first_ws, g.qap, pk->main);
        if (rc != FRW_OK) break;
        // h's coefficients [h_lo, h_hi) against this slice of h_query
        rc = msm_run<FqField, true>(pk->h, 1, h + pk->h_lo * 4, n, 1, (uint64_t *)pH, g.first_ws, g.msm_h, pk->main, true);      // (one region, one stream: frw::groth16_layout_bare)
        if (rc != FRW_OK) break;
        for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventRecord(pk->join[i], pk->side[i]);
        if (e == hipSuccess) e = hipEventRecord(pk->join[3], pk->main);
        for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipStreamWaitEvent(st, pk->join[i], 0);
        if (e != hipSuccess) break;
        if (d_partial) {
            hipLaunchKernelGGL(frw::groth16_partial_kernel, dim3(1), dim3(64), 0, st, (const uint32_t *)pA, (const uint32_t *)pB2,
                               (uint32_t *)(d_partial + b * FRW_GROTH16_PARTIAL_WORDS));
        } else {
            hipLaunchKernelGGL(frw::groth16_scale_quad_kernel, dim3(2), dim3(4), 0, st, (size_t)1, (const uint32_t *)d_split, (const uint32_t *)pA, pSA);
            hipLaunchKernelGGL(frw::groth16_finish_kernel, dim3(1), dim3(64), 0, st, (size_t)1, (const uint32_t *)pA, (const uint32_t *)pSA,
                               (const uint32_t *)pRB1, (const uint32_t *)g.pts.L, (const uint32_t *)pH, (const uint32_t *)pB2,
                               (uint32_t *)(d_proofs + b * 48));
        }
        e = hipGetLastError();
        // the next statement reuses the workspace: everything of this one must be through (the streams are ordered by `st` from here on)
    }
    if (e != hipSuccess || rc != FRW_OK) {
        if (forked) (void)hipDeviceSynchronize();
        return e != hipSuccess ? frw::record_hip_error(e, "frw_groth16_prove_dev") : rc;
    }
    return FRW_OK;
}
// rs_host: the blinding factors in host memory (uploaded, and waited for: the array may be short-lived); rs_dev: in device memory;
// args_only: the refusals alone, nothing enqueued (what frw_groth16_prove_seeded_dev asks before it draws)
int groth16_prove(const frw_groth16_pk *pk, const frw_r1cs *r1cs, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                  const uint64_t *rs_host, const uint64_t *rs_dev, uint64_t *d_proofs, uint32_t *d_num_unsatisfied, void *d_workspace,
                  size_t workspace_bytes, void *stream, bool args_only = false)
{
    const uint64_t *rs = rs_host ? rs_host : rs_dev;
    if (!pk || !r1cs || (batch && (!d_witness || !d_instance || !rs || !d_proofs || !d_workspace))) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    frw_qap_info_t q;
    if (frw_qap_info(r1cs, &q) != FRW_OK || q.domain_size != pk->domain_size || q.num_instance != pk->num_instance) return FRW_E_INVALID_ARG;
    if (pk->bare) {
        if (pk->world > 1) return FRW_E_INVALID_ARG;                        // a slice makes partial sums: frw_groth16_prove_partial_dev
        return groth16_prove_bare(pk, r1cs, batch, d_witness, d_instance, rs_host, rs_dev, d_proofs, nullptr, d_num_unsatisfied, d_workspace, workspace_bytes, stream,
                                  args_only);
    }
    const Groth16Parts parts = groth16_parts(pk, r1cs);
    const size_t chunk = std::min<size_t>(workspace_bytes / frw::groth16_layout(nullptr, 1, parts.qap, parts.domain, parts.nv, parts.msm).bytes, 4096);
    if (chunk == 0 || ((uintptr_t)d_workspace & 255)) return FRW_E_INVALID_ARG;
    if (args_only) return FRW_OK;
    const size_t I = (size_t)pk->num_instance, W = (size_t)pk->num_witness, nv = I + W, n = (size_t)pk->domain_size, stride = nv + 3;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSetDevice(pk->device);
    int rc = FRW_OK;
    bool forked = false;
    // The key's side streams and events take one chunk's work at a time (pk->enqueue); the host-side wait for the upload of r, s
    // happens BEFORE the lock is taken, so provers that share a key wait for their own stream only, not for each other's.
    std::unique_lock<std::mutex> lock(const_cast<frw_groth16_pk *>(pk)->enqueue, std::defer_lock);
    for (size_t lo = 0; e == hipSuccess && rc == FRW_OK && lo < batch; lo += chunk) {
        if (lock.owns_lock()) lock.unlock();
        const size_t cnt = std::min(chunk, batch - lo);
        const frw::Groth16Bufs g = frw::groth16_layout(d_workspace, cnt, parts.qap, parts.domain, parts.nv, parts.msm);
        uint64_t *const h = g.h, *const zext = g.zext, *const pB2 = g.pts.B2, *const d_rs = g.pts.rs, *const d_split = g.pts.split;
        // the G1 points stay in XYZZ coordinates until the proof is put together: [A | B1' | L] is what the three G1 sums write, [s A | r B1'] the scalar multiplications
        uint32_t *const pA = g.pts.A, *const pL = g.pts.L, *const pH = g.pts.H, *const pSA = g.pts.SA, *const pRB1 = g.pts.RB1;
        const uint64_t *wit = d_witness + lo * W * 4, *inst = d_instance + lo * I * 4;
        // the blinding factors: a host array (the prover draws them) is uploaded before anything reads them -- and waited for, the
        // array may be pageable and short-lived; factors that are in device memory already cost no wait (and the call is capturable)
        const uint64_t *rs_now = rs_dev ? rs_dev + lo * 8 : d_rs;
        if (rs_host) {
            e = hipMemcpyAsync(d_rs, rs_host + lo * 8, cnt * 64, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) break;
        }
        lock.lock();
        hipLaunchKernelGGL(frw::groth16_split_kernel, dim3((unsigned)((2 * cnt + 63) / 64)), dim3(64), 0, st, 2 * cnt, rs_now, d_split);
        // z ++ [1, r, s] per signature, then the witness-side sums on their own streams ...
        e = hipMemcpy2DAsync(zext, stride * 32, inst, I * 32, I * 32, cnt, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpy2DAsync(zext + I * 4, stride * 32, wit, W * 32, W * 32, cnt, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(frw::groth16_tails_kernel, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, st, cnt, (const uint32_t *)rs_now,
                           (uint32_t *)zext, stride * 8, nv);
        // Four chains of small kernels, and ONE host thread that enqueues them at 15 - 35 us a launch (some 45 launches: a chain
        // enqueued last starts a millisecond late; profiles/r04_groth16_batch1_latency.txt) -- so after the short sort the head of
        // the longest chain goes first, and the sum over h_query -- which cannot start before the witness map is through, and whose
        // bucket kernel then fills the chip -- last (for a lone proof, enqueued right behind the map instead: the same 3.92 - 3.97 ms).
        //   main      the witness map (a dozen launches, 0.7 ms; needs nothing of the sort) and the sum over h_query
        //   caller's  the sort of the digits of z ++ [1, r, s]: ONE counting sort for all four witness-side sums (its arrays live in
        //             b_g2_query's workspace; the workspaces of a_query, b_g1_query and l_query, one after the other, are the three G1
        //             sums' as one)
        //   side[0]   the three G1 sums (A, B1' and L land one after the other) as ONE chain of kernels, then both scalar
        //             multiplications as soon as their points exist
        //   side[1]   for a few proofs at a time the G1 sums' ones, beside their work items; nothing otherwise
        //   side[2]   G2
        // The key's four streams were created one after the other and sit on four different hardware queues (HIP's default); the
        // caller's stream shares a queue with ONE of them, which one depends on how many streams its process made before.  So nothing
        // but the short sort (first) and the assembly (last) runs on the caller's stream: the ones' sums, put there at first, waited
        // behind the whole witness-map chain in a process whose stream shared `main`'s queue (the sixteen-statement aggregate under the
        // profiler: 26.6 ms with them there, 22.8 ms with them on side[1]).
        const bool lone = cnt <= 4;                                        // latency counts, not throughput
        e = hipEventRecord(pk->fork, st);
        forked = true;
        if (e == hipSuccess) e = hipStreamWaitEvent(pk->main, pk->fork, 0);
        if (e != hipSuccess) break;
        // the sort first: its kernels are workgroups of 1,024 threads, which do not start under the sum over h_query's bucket kernel
        // (0.8 ms late in a trace where the host was slow to get to them)
        const NmsmBufs sorted = frw::nmsm_layout(g.msm_ws[4], cnt, (uint32_t)stride, frw::G2_BK_WORDS);
        const bool ones_as_mask = pk->a->ones_table && pk->b1->ones_table && pk->l->ones_table && pk->b2->ones_table;
        e = nmsm_sort(sorted, (uint32_t)stride, cnt, (const uint32_t *)zext, stride * 8, 1, ones_as_mask, st);
        if (e != hipSuccess) break;
        e = hipEventRecord(pk->sorted, st);
        for (int i = 0; i < 3 && e == hipSuccess; i++)
            if (i != 1 || lone) e = hipStreamWaitEvent(pk->side[i], pk->sorted, 0);
        if (e != hipSuccess) break;
        rc = frw_qap_witness_map_dev(r1cs, cnt, wit, inst, h, d_num_unsatisfied ? d_num_unsatisfied + lo : nullptr, g.qap_ws, cnt * g.qap, pk->main);
        if (rc != FRW_OK) break;
        const frw_msm *g1s[3] = {pk->a, pk->b1, pk->l};
        e = nmsm_accumulate<FqField, true>(g1s, 3, sorted, frw::nmsm_layout(g.msm_ws[1], 3 * cnt, (uint32_t)stride, frw::G1_BK_WORDS), cnt, pA, ones_as_mask, pk->side[0], true,
                                           lone, pk->side[1], pk->ones_done);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(frw::groth16_scale_quad_kernel, dim3((unsigned)(2 * cnt)), dim3(4), 0, pk->side[0], cnt, (const uint32_t *)d_split,
                           (const uint32_t *)pA, pSA);
        e = nmsm_accumulate<Fq2Field, false>(&pk->b2, 1, sorted, sorted, cnt, (uint32_t *)pB2, ones_as_mask, pk->side[2]);
        if (e != hipSuccess) break;
        // (h_query has n - 1 points and the dense pipeline: frw_groth16_pk_load; the scalars are h's coefficients 0 .. n - 2)
        rc = msm_run<FqField, true>(pk->h, cnt, h, n, 1, (uint64_t *)pH, g.msm_ws[0], cnt * g.msm[0], pk->main, true);
        if (rc != FRW_OK) break;
        // (side[1] is neither recorded nor waited for: what it carries, if anything, side[0] has waited for -- and inside a stream
        // capture an event of a stream that is not part of the capture could not be waited for)
        for (int i = 0; i < 3 && e == hipSuccess; i += 2) e = hipEventRecord(pk->join[i], pk->side[i]);
        if (e == hipSuccess) e = hipEventRecord(pk->join[3], pk->main);
        if (e != hipSuccess) break;
        for (int i = 0; i < 4 && e == hipSuccess; i++)
            if (i != 1) e = hipStreamWaitEvent(st, pk->join[i], 0);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(frw::groth16_finish_kernel, dim3((unsigned)((2 * cnt + 63) / 64)), dim3(64), 0, st, cnt, (const uint32_t *)pA,
                           (const uint32_t *)pSA, (const uint32_t *)pRB1, (const uint32_t *)pL, (const uint32_t *)pH, (const uint32_t *)pB2,
                           (uint32_t *)(d_proofs + lo * 48));
        e = hipGetLastError();
    }
    if (e != hipSuccess || rc != FRW_OK) {
        // a call that gave up half way may have work on the side streams that nothing joins: wait for it here, so that the
        // caller can release the workspace when the error comes back
        if (forked) (void)hipDeviceSynchronize();
        return e != hipSuccess ? frw::record_hip_error(e, "frw_groth16_prove_dev") : rc;
    }
    return FRW_OK;
}
}  // namespace

extern "C" int frw_groth16_prove_dev(const frw_groth16_pk *pk, const frw_r1cs *r1cs, size_t batch, const uint64_t *d_witness,
                                     const uint64_t *d_instance, const uint64_t *rs, uint64_t *d_proofs, uint32_t *d_num_unsatisfied,
                                     void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!rs && batch) return FRW_E_INVALID_ARG;
    return groth16_prove(pk, r1cs, batch, d_witness, d_instance, rs, nullptr, d_proofs, d_num_unsatisfied, d_workspace, workspace_bytes, stream);
}
extern "C" int frw_groth16_prove_rs_dev(const frw_groth16_pk *pk, const frw_r1cs *r1cs, size_t batch, const uint64_t *d_witness,
                                        const uint64_t *d_instance, const uint64_t *d_rs, uint64_t *d_proofs, uint32_t *d_num_unsatisfied,
                                        void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!d_rs && batch) return FRW_E_INVALID_ARG;
    return groth16_prove(pk, r1cs, batch, d_witness, d_instance, nullptr, d_rs, d_proofs, d_num_unsatisfied, d_workspace, workspace_bytes, stream);
}
// The same with the blinding factors DRAWN on the device (frw_drbg.h): the refusals of the call above, ONE draw of 2 batch scalars into the
// caller's d_rs, the call as it stands, the counter's step -- the draw and the step on `stream`.  A refused call has drawn nothing and
// leaves the counter alone.
extern "C" int frw_groth16_prove_seeded_dev(const frw_groth16_pk *pk, const frw_r1cs *r1cs, size_t batch, const uint64_t *d_witness,
                                            const uint64_t *d_instance, const uint8_t *d_seed, uint64_t *d_counter, uint64_t *d_rs,
                                            uint64_t *d_proofs, uint32_t *d_num_unsatisfied, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (batch == 0) return FRW_OK;
    if (!d_seed || !d_counter || !d_rs) return FRW_E_INVALID_ARG;
    int rc = groth16_prove(pk, r1cs, batch, d_witness, d_instance, nullptr, d_rs, d_proofs, d_num_unsatisfied, d_workspace, workspace_bytes, stream, true);
    if (rc != FRW_OK) return rc;
    const hipError_t e = hipSetDevice(pk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    rc = frw::drbg::draw_launch(d_seed, d_counter, FRW_DRAW_BLINDING, 2 * batch, d_rs, stream);
    if (rc == FRW_OK) rc = groth16_prove(pk, r1cs, batch, d_witness, d_instance, nullptr, d_rs, d_proofs, d_num_unsatisfied, d_workspace, workspace_bytes, stream);
    return rc == FRW_OK ? frw::drbg::advance_launch(d_counter, stream) : rc;
}

// ---- a key in slices: the partial sums of one rank, and their combination ---------------------------------------------------------------
extern "C" int frw_groth16_prove_partial_dev(const frw_groth16_pk *pk, const frw_r1cs *r1cs, size_t batch, const uint64_t *d_witness,
                                             const uint64_t *d_instance, const uint64_t *rs, uint64_t *d_partial, uint32_t *d_num_unsatisfied,
                                             void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!pk || !pk->bare || !r1cs || (batch && (!d_witness || !d_instance || !rs || !d_partial || !d_workspace))) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    frw_qap_info_t q;
    if (frw_qap_info(r1cs, &q) != FRW_OK || q.domain_size != pk->domain_size || q.num_instance != pk->num_instance) return FRW_E_INVALID_ARG;
    return groth16_prove_bare(pk, r1cs, batch, d_witness, d_instance, rs, nullptr, nullptr, d_partial, d_num_unsatisfied, d_workspace, workspace_bytes, stream);
}

extern "C" int frw_groth16_prove_combine_dev(const frw_groth16_pk *pk, size_t world, const uint64_t *d_partials, const uint64_t *rs, uint64_t *d_proof,
                                             void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!pk || world == 0 || world > 65536 || !d_partials || !rs || !d_proof || !d_workspace || workspace_bytes < FRW_GROTH16_COMBINE_WORKSPACE ||
        ((uintptr_t)d_workspace & 255))
        return FRW_E_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSetDevice(pk->device);
    frw::Carve c(d_workspace);
    const frw::Groth16Points p = frw::groth16_points_layout(c, 1);
    uint32_t *const pA = p.A, *const pH = p.H, *const pSA = p.SA, *const pRB1 = p.RB1;
    uint64_t *const pB2 = p.B2, *const d_rs = p.rs, *const d_split = p.split;
    static_assert(frw::GROTH16_POINTS_BYTES <= FRW_GROTH16_COMBINE_WORKSPACE, "the combine step's points fit its workspace");
    if (e == hipSuccess) e = hipMemcpyAsync(d_rs, rs, 64, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                     // (the array may be short-lived)
    if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_prove_combine_dev");
    hipLaunchKernelGGL(frw::groth16_split_kernel, dim3(1), dim3(64), 0, st, (size_t)2, (const uint64_t *)d_rs, d_split);
    hipLaunchKernelGGL(frw::groth16_combine_kernel, dim3(1), dim3(64), 0, st, (uint32_t)world, (const uint32_t *)d_partials, pA, (uint32_t *)pB2);
    hipLaunchKernelGGL(frw::groth16_scale_quad_kernel, dim3(2), dim3(4), 0, st, (size_t)1, (const uint32_t *)d_split, (const uint32_t *)pA, pSA);
    hipLaunchKernelGGL(frw::groth16_finish_kernel, dim3(1), dim3(64), 0, st, (size_t)1, (const uint32_t *)pA, (const uint32_t *)pSA, (const uint32_t *)pRB1,
                       (const uint32_t *)p.L, (const uint32_t *)pH, (const uint32_t *)pB2, (uint32_t *)d_proof);
    e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_groth16_prove_combine_dev");
}
#endif   // FRW_MSM_PROBE
