// frw_verify_dev.hip -- Groth16 verification with prepare_inputs on the device (round 6): ark-groth16 0.3.0 verifier.rs's
// prepare_inputs, gamma_abc_g1[0] + sum x_i gamma_abc_g1[i], over instance vectors that are in device memory already (the witness
// kernels and frw_aggregate_assign_dev write them there), and the checks ark's deserialiser makes of the key's gamma_abc_g1 points.
// The host verifier (frw_verify.cpp) does both on host threads: 0.21 s of the 1,024-statement aggregate's verification is its
// prepare_inputs, and a full check of that key's 1.57 M points is a 255-bit ladder each.  Here:
//   vk_point_check_kernel   one thread per gamma_abc_g1 row: canonical limbs, y^2 = x^3 + 4, r P = O -- frw_verify.h's
//                           g1_point_valid, the very function the host load runs; the first bad index goes back to the host
//   instance_check_kernel   every raw instance value below r, element 0 equal to one in its encoding: d_status per proof,
//                           decided BEFORE the sum (the MSM would take a value >= r mod r)
//   the sum                 frw_msm_g1_dev over the key's narrow handle: x_0 = 1, so it sums all num_instance points, gamma_0 included
//   prepared_clear_kernel   the point of a malformed vector is written as zeros (what it would have been is of no use to anybody)
// Everything after prepare_inputs -- the proof points' checks, three Miller loops, the final exponentiation -- is the host's
// frw::verify::verify_prepared in frw_groth16_verify_dev, the code frw_groth16_verify runs too; frw_groth16_verify_full_dev runs it on
// the device instead (frw_pairing_dev.hip), after the same prepare_inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_layout.h"
#include "frw_pairing_dev.h"
#include "frw_rerand.h"
#include "frw_verify.h"
#include "frw_wire.h"

namespace frw {
namespace {

// ---- the key's points --------------------------------------------------------------------------------------------------------------
// 255 doublings and ~128 mixed additions of XYZZ coordinates per point (about 3,600 Fq products), no memory traffic to speak of:
// a thread per point, 64 to a workgroup like the MSM's point kernels (tools/kernel_resources.py --full reports registers and waves)
__global__ __launch_bounds__(64) void vk_point_check_kernel(uint64_t n, const uint64_t *__restrict__ rows, unsigned long long *__restrict__ first_bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (!verify::g1_point_valid(rows + 12 * i)) atomicMin(first_bad, (unsigned long long)i);
}

// ---- the instance vectors ----------------------------------------------------------------------------------------------------------
// one: 1 (canonical) or R = 2^256 mod r (ark-ff's Montgomery form of 1)
__global__ __launch_bounds__(256) void instance_check_kernel(uint64_t total, uint64_t n, const uint64_t *__restrict__ inst, int montgomery,
                                                             int32_t *__restrict__ status)
{
    const uint64_t one[4] = {montgomery ? 0x00000001fffffffeULL : 1ULL, montgomery ? 0x5884b7fa00034802ULL : 0ULL,
                             montgomery ? 0x998c4fefecbc4ff5ULL : 0ULL, montgomery ? 0x1824b159acc5056fULL : 0ULL};
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (uint64_t)gridDim.x * 256) {
        const uint64_t *w = inst + 4 * k;
        const uint64_t i = k % n;
        bool bad = !verify::fr_limbs_below_modulus(w);
        if (i == 0) bad = bad || w[0] != one[0] || w[1] != one[1] || w[2] != one[2] || w[3] != one[3];
        if (bad) status[k / n] = -1;                                 // (every writer writes the same value)
    }
}

__global__ __launch_bounds__(256) void prepared_clear_kernel(uint64_t batch, const int32_t *__restrict__ status, uint64_t *__restrict__ prepared)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < batch * 12 && status[k / 12]) prepared[k] = 0;
}

// Which narrow handle holds the key's points.  A table handle (3.5 KB a point, and up to 2^18 points the subset sums of every eight,
// which the long runs of ones of a Falcon instance vector use) sums a whole batch per call: the keys of per-signature circuits and of
// aggregates of up to ~80 statements (a sixteen-statement key has 32,769 points: 115 MB).  Beyond 2^18 points the table loses its
// subset sums and grows to gigabytes (5.6 GB for the 1,024-statement key's 1.57 M points), so the handle is BARE there: 112 bytes a
// point, one vector per call -- an aggregate's statement is verified one proof at a time anyway.
constexpr size_t VK_TABLE_MAX_POINTS = (size_t)1 << 18;

size_t msm_workspace(const frw_groth16_vk *vk)
{
    frw_msm_info_t info;
    return frw_msm_info(vk->msm, &info) == FRW_OK ? (size_t)info.workspace_bytes_per_signature : 0;
}
bool msm_bare(const frw_groth16_vk *vk) { return vk->num_instance > VK_TABLE_MAX_POINTS; }
// the workspace of `k` proofs in flight (frw::verify_layout); pairing: with the device pairing's part, wire: with the decoder's in front
VerifyBufs layout(const frw_groth16_vk *vk, void *ws, size_t k, bool pairing = false, int flags = 0, bool wire = false)
{
    return verify_layout(ws, k, msm_workspace(vk), msm_bare(vk), pairing ? pairing_dev::proof_workspace_bytes(flags) : 0,
                         pairing ? pairing_dev::pass_workspace_bytes(flags) : 0, wire);
}

int prepare(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, uint64_t *d_prepared, int32_t *d_status,
            void *d_msm_ws, size_t msm_ws_bytes, hipStream_t st)
{
    const uint64_t n = vk->num_instance, total = batch * n;
    hipError_t e = hipMemsetAsync(d_status, 0, batch * sizeof(int32_t), st);
    if (e != hipSuccess) return record_hip_error(e, "frw_groth16_prepare_inputs_dev");
    const uint64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(instance_check_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, total, n, d_instance,
                       encoding == FRW_ENC_MONTGOMERY ? 1 : 0, d_status);
    e = hipGetLastError();
    if (e != hipSuccess) return record_hip_error(e, "frw_groth16_prepare_inputs_dev");
    const int rc = frw_msm_g1_dev(vk->msm, batch, d_instance, n, encoding == FRW_ENC_MONTGOMERY ? 1 : 0, d_prepared, d_msm_ws, msm_ws_bytes, st);
    if (rc != FRW_OK) return rc;
    hipLaunchKernelGGL(prepared_clear_kernel, dim3((unsigned)((batch * 12 + 255) / 256)), dim3(256), 0, st, (uint64_t)batch, d_status, d_prepared);
    e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : record_hip_error(e, "frw_groth16_prepare_inputs_dev");
}

}  // namespace
}  // namespace frw

extern "C" int frw_groth16_vk_load_dev(int device, const uint64_t *vk, size_t num_instance, int flags, frw_groth16_vk **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    if (!vk || num_instance == 0 || num_instance > ((size_t)1 << 31) - 1 || flags != 0) return FRW_E_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    // every gamma_abc_g1 row, checked on the device before anything is built from it
    const uint64_t *rows = vk + 84;
    void *d_rows = nullptr;
    unsigned long long *d_bad = nullptr, bad = ~0ull;
    e = hipMalloc(&d_rows, num_instance * 96);
    if (e == hipSuccess) e = hipMalloc((void **)&d_bad, sizeof(bad));
    if (e == hipSuccess) e = hipMemcpy(d_rows, rows, num_instance * 96, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_bad, &bad, sizeof(bad), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(frw::vk_point_check_kernel, dim3((unsigned)((num_instance + 63) / 64)), dim3(64), 0, nullptr, (uint64_t)num_instance,
                           (const uint64_t *)d_rows, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    if (d_rows) (void)hipFree(d_rows);
    if (d_bad) (void)hipFree(d_bad);
    if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_vk_load_dev");
    if (bad != ~0ull) return FRW_E_INVALID_ARG;
    // the host key (the four fixed points checked there, e(alpha, beta) computed), then the device's copy of gamma_abc_g1
    frw_groth16_vk *k = nullptr;
    int rc = frw::verify::vk_load(vk, num_instance, false, &k);
    if (rc != FRW_OK) return rc;
    frw_msm *m = nullptr;
    rc = num_instance > frw::VK_TABLE_MAX_POINTS ? frw_msm_g1_load_bare(device, num_instance, rows, 1, &m)
                                                  : frw_msm_g1_load_narrow(device, num_instance, rows, &m);
    if (rc != FRW_OK) {
        frw_groth16_vk_free(k);
        return rc;
    }
    k->device = device;
    k->msm = m;
    // the device pairing's fixed part: -gamma, -delta and beta's line tables, the Frobenius constants, e(alpha, beta)^3
    rc = frw::pairing_dev::upload_key(k, vk, vk + 12);
    if (rc == FRW_OK) rc = frw::rerand::upload_key(k);             // delta_g2 for frw_groth16_rerandomize_dev
    if (rc != FRW_OK) {
        frw_groth16_vk_free(k);
        return rc;
    }
    *out = k;
    return FRW_OK;
}

extern "C" size_t frw_groth16_verify_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight)
{
    if (!vk || !vk->msm || batch_in_flight == 0) return 0;
    return frw::layout(vk, nullptr, batch_in_flight).bytes;
}

extern "C" int frw_groth16_prepare_inputs_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, uint64_t *d_prepared,
                                              int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!vk || !vk->msm) return FRW_E_INVALID_ARG;
    if (encoding != FRW_ENC_MONTGOMERY && encoding != FRW_ENC_CANONICAL) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_instance || !d_prepared || !d_status || !d_workspace || ((uintptr_t)d_workspace & 15) ||
        workspace_bytes < frw::layout(vk, nullptr, 1).bytes)
        return FRW_E_INVALID_ARG;
    hipError_t e = hipSetDevice(vk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    // (the sum gets the whole workspace: a table handle runs as many vectors per pass as it holds)
    return frw::prepare(vk, batch, d_instance, encoding, d_prepared, d_status, d_workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int frw_groth16_verify_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, const uint64_t *d_proofs,
                                      int flags, int32_t *accepted, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!vk || !vk->msm) return FRW_E_INVALID_ARG;
    if (encoding != FRW_ENC_MONTGOMERY && encoding != FRW_ENC_CANONICAL) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_instance || !d_proofs || !accepted || !d_workspace || ((uintptr_t)d_workspace & 15)) return FRW_E_INVALID_ARG;
    const size_t chunk = frw::proofs_in_flight(batch, workspace_bytes, [&](size_t k) { return frw::layout(vk, nullptr, k).bytes; });
    if (chunk == 0) return FRW_E_INVALID_ARG;
    hipError_t e = hipSetDevice(vk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    const hipStream_t st = (hipStream_t)stream;
    const size_t n = vk->num_instance;
    try {
        const frw::VerifyBufs v = frw::layout(vk, d_workspace, chunk);
        std::vector<uint64_t> prepared(12 * chunk), proofs(48 * chunk);
        std::vector<int32_t> status(chunk);
        for (size_t lo = 0; lo < batch; lo += chunk) {
            const size_t cnt = batch - lo < chunk ? batch - lo : chunk;
            const int rc = frw::prepare(vk, cnt, d_instance + lo * n * 4, encoding, v.prepared, v.status, v.msm_ws, v.msm_bytes, st);
            if (rc != FRW_OK) return rc;
            e = hipMemcpyAsync(prepared.data(), v.prepared, cnt * 96, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(status.data(), v.status, cnt * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(proofs.data(), d_proofs + lo * 48, cnt * 384, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_verify_dev");
            // the rest is frw_groth16_verify's own code, one proof per host thread
            const bool ok = frw::verify::for_each_proof(cnt, [&](size_t i) {
                accepted[lo + i] = status[i] ? -1 : frw::verify::verify_prepared(*vk, &prepared[12 * i], &proofs[48 * i], flags);
            });
            if (!ok) return FRW_E_OUT_OF_MEMORY;
        }
    } catch (...) {
        return FRW_E_OUT_OF_MEMORY;
    }
    return FRW_OK;
}

// ---- the whole verification on the device --------------------------------------------------------------------------------------------
namespace frw {
namespace {
// a proof the decoder refused is malformed for everything that follows (after prepare, which sets d_status from the instance vector)
__global__ __launch_bounds__(256) void wire_status_kernel(uint64_t n, const int32_t *__restrict__ decoded, int32_t *__restrict__ status)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < n && decoded[g]) status[g] = -1;
}
// The chain, `chunk` proofs at a time: (d_wire: the decoder, in place of d_proofs,) prepare_inputs, (the decoder's refusals into the
// statuses,) the proofs' checks and the pairings.  The entry points have validated the arguments and found `chunk`.
int verify_chain(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, const uint64_t *d_proofs, const uint8_t *d_wire, int mode,
                 int flags, const uint64_t *seed, int32_t *d_accepted, int32_t *d_batch_passed, void *d_workspace, size_t chunk, hipStream_t st)
{
    const bool wire = d_wire != nullptr;
    const VerifyBufs v = layout(vk, d_workspace, chunk, true, flags, wire);
    const size_t n = vk->num_instance, wire_bytes = wire ? wire::proof_bytes(mode) : 0;
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = batch - lo < chunk ? batch - lo : chunk;
        int rc = wire ? wire::decode_proofs_launch(cnt, d_wire + lo * wire_bytes, mode, v.decoded, v.decode_status, st) : FRW_OK;
        if (rc == FRW_OK) rc = prepare(vk, cnt, d_instance + lo * n * 4, encoding, v.prepared, v.status, v.msm_ws, v.msm_bytes, st);
        if (rc != FRW_OK) return rc;
        if (wire) hipLaunchKernelGGL(wire_status_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (uint64_t)cnt, (const int32_t *)v.decode_status, v.status);
        rc = pairing_dev::verify_proofs(vk, cnt, lo, wire ? v.decoded : d_proofs + lo * 48, v.prepared, v.status, flags, seed, d_accepted + lo, d_batch_passed,
                                        v.pairing_ws, st);
        if (rc != FRW_OK) return rc;
    }
    return FRW_OK;
}
}  // namespace
}  // namespace frw

extern "C" size_t frw_groth16_verify_full_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight, int flags)
{
    if (!vk || !vk->msm || !vk->d_pairing || batch_in_flight == 0 || (flags & ~(FRW_VERIFY_POINTS_ARE_CHECKED | FRW_VERIFY_BATCHED))) return 0;
    return frw::layout(vk, nullptr, batch_in_flight, true, flags).bytes;
}

extern "C" int frw_groth16_verify_full_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding,
                                           const uint64_t *d_proofs, int flags, const uint64_t *seed, int32_t *d_accepted,
                                           int32_t *d_batch_passed, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!vk || !vk->msm || !vk->d_pairing) return FRW_E_INVALID_ARG;
    if (encoding != FRW_ENC_MONTGOMERY && encoding != FRW_ENC_CANONICAL) return FRW_E_INVALID_ARG;
    if (flags & ~(FRW_VERIFY_POINTS_ARE_CHECKED | FRW_VERIFY_BATCHED)) return FRW_E_INVALID_ARG;
    if ((flags & FRW_VERIFY_BATCHED) && !seed) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_instance || !d_proofs || !d_accepted || !d_workspace || ((uintptr_t)d_workspace & 15)) return FRW_E_INVALID_ARG;
    const size_t chunk = frw::proofs_in_flight(batch, workspace_bytes, [&](size_t k) { return frw::layout(vk, nullptr, k, true, flags).bytes; });
    if (chunk == 0) return FRW_E_INVALID_ARG;
    hipError_t e = hipSetDevice(vk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    return frw::verify_chain(vk, batch, d_instance, encoding, d_proofs, nullptr, 0, flags, seed, d_accepted, d_batch_passed, d_workspace, chunk, (hipStream_t)stream);
}

// ---- the same from proofs in ark-serialize's wire format (frw_wire.h) ----------------------------------------------------------------
extern "C" size_t frw_groth16_verify_wire_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight, int flags, int mode)
{
    if (mode != FRW_WIRE_COMPRESSED && mode != FRW_WIRE_UNCOMPRESSED) return 0;
    if (!frw_groth16_verify_full_workspace_bytes(vk, batch_in_flight, flags)) return 0;           // (its checks of vk and flags)
    return frw::layout(vk, nullptr, batch_in_flight, true, flags, true).bytes;
}

extern "C" int frw_groth16_verify_wire_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, const uint8_t *d_wire,
                                           int mode, int flags, const uint64_t *seed, int32_t *d_accepted, int32_t *d_batch_passed,
                                           void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!vk || !vk->msm || !vk->d_pairing) return FRW_E_INVALID_ARG;
    if (encoding != FRW_ENC_MONTGOMERY && encoding != FRW_ENC_CANONICAL) return FRW_E_INVALID_ARG;
    if (mode != FRW_WIRE_COMPRESSED && mode != FRW_WIRE_UNCOMPRESSED) return FRW_E_INVALID_ARG;
    if (flags & ~(FRW_VERIFY_POINTS_ARE_CHECKED | FRW_VERIFY_BATCHED)) return FRW_E_INVALID_ARG;
    if ((flags & FRW_VERIFY_BATCHED) && !seed) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_instance || !d_wire || !d_accepted || !d_workspace || ((uintptr_t)d_workspace & 15)) return FRW_E_INVALID_ARG;
    const size_t chunk = frw::proofs_in_flight(batch, workspace_bytes, [&](size_t k) { return frw::layout(vk, nullptr, k, true, flags, true).bytes; });
    if (chunk == 0) return FRW_E_INVALID_ARG;
    hipError_t e = hipSetDevice(vk->device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    return frw::verify_chain(vk, batch, d_instance, encoding, nullptr, d_wire, mode, flags, seed, d_accepted, d_batch_passed, d_workspace, chunk, (hipStream_t)stream);
}
