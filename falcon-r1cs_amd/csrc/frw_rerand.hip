// frw_rerand.hip -- re-randomising Groth16 proofs (ark-groth16 0.3.0 prover.rs, rerandomize_proof): the host function and the device's
// kernel chain, both over the formulas of frw_rerand.h.
//     A' = r1^-1 A            B' = r1 B + (r1 r2) delta_g2            C' = C + r2 A
// Five scalar multiplications of points that differ from proof to proof (delta_g2 apart): nothing to sort, no tables, no memory traffic
// to speak of -- chains of dependent field products, A' and C' side by side in one launch, B' in the next:
//   rerand_check_kernel     two lanes per proof: the checks of frw_groth16_verify's proof points by the same functions -- canonical
//                           limbs, on the curve and, unless the caller vouches, in the subgroup (255-bit ladders: A in the even lane,
//                           C in the odd one, B over both with Fq2PairField).  Writes every status: 0 or -1.
//   rerand_factor_kernel    one lane per proof: r1, r2 modulo r, the zero test (FRW_RERAND_ZERO_FACTOR), r1^-1, r1 r2 and the
//                           endomorphism's halves of the two G1 multipliers, in plain 64-bit integers
//   rerand_g1_kernel        two lanes per proof: r1^-1 A in the even lane, r2 A + C in the odd one; 128 steps each over
//                           {P, phi(P), P + phi(P)}, one doubling and at most one mixed addition a step
//   rerand_g2_kernel        two lanes per proof on Fq2PairField: r1 B + (r1 r2) delta_g2 as ONE ladder of 255 doublings shared by both
//                           terms.  This chain is the longest: 255 steps against 128, and an Fq2 product a step where G1 has an Fq one.
//   rerand_finish_kernel    <FqField>: a lane per G1 result, <Fq2PairField>: two lanes per G2 result: XYZZ -> ark-ff's affine limbs, one
//                           inversion per point (frw_fq29.h's fq_inv is 25 passes of 31 Euclidean rounds: a tenth of a ladder); zeros
//                           for a refused slot.  A kernel of its own because the inversion's registers would halve the ladders' waves.
//   rerand_wire_clear_kernel  the wire form: a refused slot's bytes are zeros, not the encoding of three points at infinity
// All on the caller's stream, nothing allocated: capture-safe, no parallel branches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <new>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_drbg.h"
#include "frw_layout.h"
#include "frw_rerand.h"
#include "frw_verify.h"
#include "frw_wire.h"

namespace frw {
namespace rerand {
namespace {

// The TWIN of frw_pairing_dev.hip's proof_check_kernel (the same pair layout and meeting of the two lanes' verdicts, the predicates
// shared through frw_verify.h / frw_rerand.h; this one also writes 0 and takes the decoder's refusals): change them together.
__global__ __launch_bounds__(64) void rerand_check_kernel(uint64_t n, const uint64_t *proofs, int check_subgroup, const int32_t *prior, int32_t *status)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 64 + threadIdx.x) >> 1;
    if (g >= n) return;
    const bool odd = threadIdx.x & 1;
    const uint64_t *pw = proofs + 48 * g;
    const bool mine = g1_point_ok(pw + (odd ? 36 : 0), check_subgroup != 0);
    const bool b = g2_point_ok<Fq2PairField>(pw + 12, check_subgroup != 0);          // (both lanes, whatever the G1 checks said)
    const uint32_t ok = mine && b ? 1u : 0u;
    const uint32_t both = ok & pair_swap_u32(ok);
    if (!odd) status[g] = both && !(prior && prior[g]) ? 0 : -1;
}

__global__ __launch_bounds__(64) void rerand_factor_kernel(uint64_t n, const uint64_t *__restrict__ factors, int32_t *__restrict__ status,
                                                           uint64_t *__restrict__ scalars)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= n || status[g]) return;
    uint64_t sc[SCALAR_WORDS];
    const int st = factors_prepare(factors + 8 * g, sc);
    if (st) { status[g] = st; return; }
    for (int k = 0; k < SCALAR_WORDS; k++) scalars[SCALAR_WORDS * g + k] = sc[k];
}

// a point in XYZZ coordinates as frw_layout.h budgets it (a bucket): X | Y | ZZ | ZZZ limbs, then the infinity flag
template <class F> __device__ __forceinline__ void bucket_store(const XyzzT<F> &p, uint32_t *w)
{
    F::store(p.x, w); F::store(p.y, w + F::WORDS); F::store(p.zz, w + 2 * F::WORDS); F::store(p.zzz, w + 3 * F::WORDS);
    w[4 * F::WORDS] = p.inf ? 1u : 0u;                                                // (both lanes of a pair write the same flag)
}
template <class F> __device__ __forceinline__ XyzzT<F> bucket_load(const uint32_t *w)
{
    XyzzT<F> p;
    p.x = F::load(w); p.y = F::load(w + F::WORDS); p.zz = F::load(w + 2 * F::WORDS); p.zzz = F::load(w + 3 * F::WORDS);
    p.inf = w[4 * F::WORDS] != 0;
    return p;
}

// A ladder's addends in LDS (frw_rerand.h): element i of this lane is fourteen words, word w at [i][w][lane] -- consecutive lanes read
// consecutive words, no bank is asked twice.  A lane reads only what it wrote itself: no barrier.
template <int N> struct LdsTable {
    uint32_t *mine;                                                                   // &words[0][0][lane]
    __device__ __forceinline__ void put(int i, const Fq29 &e)
    {
#pragma unroll
        for (int w = 0; w < NLQ; w++) mine[(i * NLQ + w) * 64] = e.l[w];
    }
    __device__ __forceinline__ void put(int i, const Fq2Half &e) { put(i, e.v); }
    __device__ __forceinline__ Fq29 get_fq(int i) const
    {
        Fq29 r;
#pragma unroll
        for (int w = 0; w < NLQ; w++) r.l[w] = mine[(i * NLQ + w) * 64];
        return r;
    }
};
struct LdsTableG1 : LdsTable<5> { __device__ __forceinline__ Fq29 get(int i) const { return get_fq(i); } };
struct LdsTableG2 : LdsTable<4> { __device__ __forceinline__ Fq2Half get(int i) const { Fq2Half r; r.v = get_fq(i); return r; } };

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void rerand_g1_kernel(uint64_t n, const uint64_t *__restrict__ proofs, const uint64_t *__restrict__ scalars,
                                                       const int32_t *__restrict__ status, uint32_t *__restrict__ points)
{
    __shared__ uint32_t words[5 * NLQ * 64];
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x, g = t >> 1;
    if (g >= n || status[g]) return;
    const bool odd = t & 1;
    LdsTableG1 tab;
    tab.mine = words + threadIdx.x;
    const uint64_t *pw = proofs + 48 * g;
    const G1Affine29 a = load_ark<FqField>(pw);
    G1Affine29 c = load_ark<FqField>(pw + 36);
    c.inf = c.inf || !odd;                                                            // A' has no addend
    uint64_t split[4];
    for (int k = 0; k < 4; k++) split[k] = scalars[SCALAR_WORDS * g + (odd ? SC_R2_SPLIT : SC_INV_SPLIT) + k];
    bucket_store<FqField>(g1_multiple_plus(tab, a, split, c), points + t * G1_BK_WORDS);
}

__global__ __launch_bounds__(64) void rerand_g2_kernel(uint64_t n, const uint64_t *__restrict__ proofs, const uint64_t *__restrict__ delta,
                                                       const uint64_t *__restrict__ scalars, const int32_t *__restrict__ status,
                                                       uint32_t *__restrict__ points)
{
    typedef Fq2PairField P;
    __shared__ uint32_t words[4 * NLQ * 64];
    const uint64_t g = ((uint64_t)blockIdx.x * 64 + threadIdx.x) >> 1;
    if (g >= n || status[g]) return;                                                  // (a pair leaves together)
    LdsTableG2 tab;
    tab.mine = words + threadIdx.x;
    uint64_t k1[4], k2[4];
    for (int k = 0; k < 4; k++) { k1[k] = scalars[SCALAR_WORDS * g + SC_R1 + k]; k2[k] = scalars[SCALAR_WORDS * g + SC_R1R2 + k]; }
    const XyzzT<P> r = g2_double_multiple<P>(tab, load_ark<P>(proofs + 48 * g + 12), k1, load_ark<P>(delta), k2);
    bucket_store<P>(r, points + g * G2_BK_WORDS);
}

// points: F::LANES lanes each, `per` of them a proof; point j of proof g goes to out + 48 g + at + stride j (words of 64 bits)
template <class F>
__global__ __launch_bounds__(64) void rerand_finish_kernel(uint64_t n, int per, int at, int stride, const uint32_t *__restrict__ points,
                                                           const int32_t *__restrict__ status, uint64_t *__restrict__ out)
{
    const uint64_t i = ((uint64_t)blockIdx.x * 64 + threadIdx.x) / F::LANES;
    const uint64_t g = i / (uint64_t)per;
    if (g >= n) return;
    uint64_t *o = out + 48 * g + at + stride * (int)(i % (uint64_t)per);
    if (status[g]) {
        for (int k = 0; k < F::ARK_WORDS; k++) o[k] = 0;
        return;
    }
    store_ark<F>(pt_to_affine(bucket_load<F>(points + i * (4 * F::WORDS + 4))), o);
}

__global__ __launch_bounds__(256) void rerand_wire_clear_kernel(uint64_t n, uint64_t bytes, const int32_t *__restrict__ status, uint8_t *__restrict__ out)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n || !status[g]) return;
    for (uint64_t k = 0; k < bytes; k++) out[g * bytes + k] = 0;
}

inline unsigned grid(uint64_t threads, unsigned block) { return (unsigned)((threads + block - 1) / block); }
static_assert(G1_BK_WORDS == 4 * FqField::WORDS + 4 && G2_BK_WORDS == 4 * Fq2PairField::WORDS + 4, "a bucket of frw_layout.h");
static_assert(RERAND_SCALAR_BYTES == SCALAR_WORDS * 8, "the scalars of a proof");

// `cnt` proofs through the chain: d_proofs -> d_out (they may be the same), statuses into d_status; prior (optional): slots refused
// before the chain (the decoder's)
int chain(const frw_groth16_vk *vk, size_t cnt, const uint64_t *d_proofs, const uint64_t *d_factors, int flags, const int32_t *prior,
          uint64_t *d_out, int32_t *d_status, const RerandBufs &b, hipStream_t st)
{
    hipLaunchKernelGGL(rerand_check_kernel, dim3(grid(2 * cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, d_proofs,
                       (flags & FRW_VERIFY_POINTS_ARE_CHECKED) ? 0 : 1, prior, d_status);
    hipLaunchKernelGGL(rerand_factor_kernel, dim3(grid(cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, d_factors, d_status, b.scalars);
    hipLaunchKernelGGL(rerand_g1_kernel, dim3(grid(2 * cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, d_proofs, (const uint64_t *)b.scalars,
                       (const int32_t *)d_status, b.g1_points);
    hipLaunchKernelGGL(rerand_g2_kernel, dim3(grid(2 * cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, d_proofs, (const uint64_t *)vk->d_delta,
                       (const uint64_t *)b.scalars, (const int32_t *)d_status, b.g2_points);
    // (every read of d_proofs is behind: d_out may be the same memory)
    hipLaunchKernelGGL(rerand_finish_kernel<FqField>, dim3(grid(2 * cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, 2, 0, 36, (const uint32_t *)b.g1_points,
                       (const int32_t *)d_status, d_out);
    hipLaunchKernelGGL(rerand_finish_kernel<Fq2PairField>, dim3(grid(2 * cnt, 64)), dim3(64), 0, st, (uint64_t)cnt, 1, 12, 0,
                       (const uint32_t *)b.g2_points, (const int32_t *)d_status, d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : record_hip_error(e, "frw_groth16_rerandomize_dev");
}

bool mode_ok(int mode) { return mode == FRW_WIRE_COMPRESSED || mode == FRW_WIRE_UNCOMPRESSED; }
bool have_device()
{
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

}  // namespace

int upload_key(frw_groth16_vk *vk)
{
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(vk->delta_ark));
    if (e == hipSuccess) e = hipMemcpy(d, vk->delta_ark, sizeof(vk->delta_ark), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return record_hip_error(e, "frw_groth16_vk_load_dev");
    }
    vk->d_delta = (uint64_t *)d;
    return FRW_OK;
}

}  // namespace rerand
}  // namespace frw

using namespace frw::rerand;

extern "C" int frw_groth16_rerandomize(const frw_groth16_vk *vk, size_t batch, const uint64_t *proofs, const uint64_t *factors, int flags,
                                       uint64_t *out, int32_t *status)
{
    if (batch == 0) return FRW_OK;
    if (!vk || !proofs || !factors || !out || !status || (flags & ~FRW_VERIFY_POINTS_ARE_CHECKED)) return FRW_E_INVALID_ARG;
    try {
        const bool ok = frw::verify::for_each_proof(batch, [&](size_t i) {
            status[i] = rerandomize_one<frw::Fq2Field>(proofs + 48 * i, factors + 8 * i, vk->delta_ark, !(flags & FRW_VERIFY_POINTS_ARE_CHECKED), out + 48 * i);
        });
        return ok ? FRW_OK : FRW_E_OUT_OF_MEMORY;
    } catch (...) {
        return FRW_E_OUT_OF_MEMORY;
    }
}

extern "C" size_t frw_groth16_rerandomize_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight, int wire_mode)
{
    if (!vk || batch_in_flight == 0 || (wire_mode != -1 && !mode_ok(wire_mode))) return 0;
    return frw::rerand_layout(nullptr, batch_in_flight, wire_mode != -1).bytes;
}

// The two device calls; args_only: the refusals alone, nothing enqueued (what the seeded calls ask before they draw)
static int rerandomize_limbs(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_proofs, const uint64_t *d_factors, int flags, uint64_t *d_out,
                             int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream, bool args_only)
{
    if (batch == 0) return FRW_OK;
    if (!vk || !d_proofs || !d_factors || !d_out || !d_status || !d_workspace || ((uintptr_t)d_workspace & 15) ||
        (flags & ~FRW_VERIFY_POINTS_ARE_CHECKED))
        return FRW_E_INVALID_ARG;
    if (!have_device()) return FRW_E_NO_DEVICE;
    if (!vk->d_delta) return FRW_E_INVALID_ARG;
    const size_t chunk = frw::proofs_in_flight(batch, workspace_bytes, [](size_t k) { return frw::rerand_layout(nullptr, k, false).bytes; });
    if (chunk == 0) return FRW_E_INVALID_ARG;
    if (args_only) return FRW_OK;
    const hipError_t e = hipSetDevice(vk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    const frw::RerandBufs b = frw::rerand_layout(d_workspace, chunk, false);
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = batch - lo < chunk ? batch - lo : chunk;
        const int rc = chain(vk, cnt, d_proofs + 48 * lo, d_factors + 8 * lo, flags, nullptr, d_out + 48 * lo, d_status + lo, b, (hipStream_t)stream);
        if (rc != FRW_OK) return rc;
    }
    return FRW_OK;
}

extern "C" int frw_groth16_rerandomize_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_proofs, const uint64_t *d_factors, int flags,
                                           uint64_t *d_out, int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return rerandomize_limbs(vk, batch, d_proofs, d_factors, flags, d_out, d_status, d_workspace, workspace_bytes, stream, false);
}

static int rerandomize_wire(const frw_groth16_vk *vk, size_t batch, const uint8_t *d_wire_in, int mode, const uint64_t *d_factors, int flags,
                            uint8_t *d_wire_out, int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream, bool args_only)
{
    if (batch == 0) return FRW_OK;
    if (!vk || !d_wire_in || !d_factors || !d_wire_out || !d_status || !d_workspace || ((uintptr_t)d_workspace & 15) || !mode_ok(mode) ||
        (flags & ~FRW_VERIFY_POINTS_ARE_CHECKED))
        return FRW_E_INVALID_ARG;
    if (!have_device()) return FRW_E_NO_DEVICE;
    if (!vk->d_delta) return FRW_E_INVALID_ARG;
    const size_t chunk = frw::proofs_in_flight(batch, workspace_bytes, [](size_t k) { return frw::rerand_layout(nullptr, k, true).bytes; });
    if (chunk == 0) return FRW_E_INVALID_ARG;
    if (args_only) return FRW_OK;
    const hipError_t e = hipSetDevice(vk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    const hipStream_t st = (hipStream_t)stream;
    const frw::RerandBufs b = frw::rerand_layout(d_workspace, chunk, true);
    const size_t wire_bytes = frw::wire::proof_bytes(mode);
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = batch - lo < chunk ? batch - lo : chunk;
        int rc = frw::wire::decode_proofs_launch(cnt, d_wire_in + lo * wire_bytes, mode, b.decoded, b.decode_status, st);
        if (rc == FRW_OK) rc = chain(vk, cnt, b.decoded, d_factors + 8 * lo, flags, b.decode_status, b.decoded, d_status + lo, b, st);
        if (rc == FRW_OK) rc = frw_groth16_proofs_to_wire_dev(vk->device, cnt, b.decoded, mode, d_wire_out + lo * wire_bytes, b.encode_status, stream);
        if (rc != FRW_OK) return rc;
        hipLaunchKernelGGL(rerand_wire_clear_kernel, dim3(grid(cnt, 256)), dim3(256), 0, st, (uint64_t)cnt, (uint64_t)wire_bytes,
                           (const int32_t *)(d_status + lo), d_wire_out + lo * wire_bytes);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) return frw::record_hip_error(le, "frw_groth16_rerandomize_wire_dev");
    }
    return FRW_OK;
}

extern "C" int frw_groth16_rerandomize_wire_dev(const frw_groth16_vk *vk, size_t batch, const uint8_t *d_wire_in, int mode, const uint64_t *d_factors,
                                                int flags, uint8_t *d_wire_out, int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                                                void *stream)
{
    return rerandomize_wire(vk, batch, d_wire_in, mode, d_factors, flags, d_wire_out, d_status, d_workspace, workspace_bytes, stream, false);
}

// ---- the same with the factors drawn on the device (frw_drbg.h): the wrapped call's refusals, ONE draw of 2 batch scalars into the caller's
// d_factors, the call as it stands, the counter's step -- all on `stream`.  A refused call has drawn nothing and leaves the counter alone.
template <class Call> static int seeded(const frw_groth16_vk *vk, size_t batch, const uint8_t *d_seed, uint64_t *d_counter, uint64_t *d_factors, void *stream,
                                        Call call)
{
    if (batch == 0) return FRW_OK;
    if (!d_seed || !d_counter) return FRW_E_INVALID_ARG;
    int rc = call(true);
    if (rc != FRW_OK) return rc;
    const hipError_t e = hipSetDevice(vk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    rc = frw::drbg::draw_launch(d_seed, d_counter, FRW_DRAW_RERANDOMIZE, 2 * batch, d_factors, stream);
    if (rc == FRW_OK) rc = call(false);
    return rc == FRW_OK ? frw::drbg::advance_launch(d_counter, stream) : rc;
}

extern "C" int frw_groth16_rerandomize_seeded_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_proofs, const uint8_t *d_seed,
                                                  uint64_t *d_counter, uint64_t *d_factors, int flags, uint64_t *d_out, int32_t *d_status,
                                                  void *d_workspace, size_t workspace_bytes, void *stream)
{
    return seeded(vk, batch, d_seed, d_counter, d_factors, stream, [&](bool args_only) {
        return rerandomize_limbs(vk, batch, d_proofs, d_factors, flags, d_out, d_status, d_workspace, workspace_bytes, stream, args_only);
    });
}

extern "C" int frw_groth16_rerandomize_wire_seeded_dev(const frw_groth16_vk *vk, size_t batch, const uint8_t *d_wire_in, int mode, const uint8_t *d_seed,
                                                       uint64_t *d_counter, uint64_t *d_factors, int flags, uint8_t *d_wire_out, int32_t *d_status,
                                                       void *d_workspace, size_t workspace_bytes, void *stream)
{
    return seeded(vk, batch, d_seed, d_counter, d_factors, stream, [&](bool args_only) {
        return rerandomize_wire(vk, batch, d_wire_in, mode, d_factors, flags, d_wire_out, d_status, d_workspace, workspace_bytes, stream, args_only);
    });
}
