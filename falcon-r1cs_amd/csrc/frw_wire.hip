// frw_wire.hip -- Groth16 proofs and verifying keys in ark-serialize's wire format (frw_wire.h has the format and the codec): the kernels
// that encode and decode them on the device, and the C ABI on both sides.  Host and device run the SAME functions of frw_wire.h, so their
// bytes and limbs agree by construction.
//   wire_encode_proofs_kernel     a lane per proof: twelve products, the rest is loads and stores
//   wire_g1_decode_kernel         two lanes per proof, A in the even lane and C in the odd one (proof_check_kernel's idiom): one
//                                 a^((q + 1) / 4) each when compressed -- ~610 dependent Fq products, one accumulator, no scratch
//   wire_g2_decode_kernel         a lane per proof for B: two such roots and an inversion (frw_wire.h fq2_sqrt_candidate); it runs after
//                                 the G1 kernel on the same stream, folds B's verdict into the proof's status and clears a refused proof
//   wire_g1_run_decode_kernel     a lane per point of a run of G1 points (a key's gamma_abc_g1); the first bad index goes back
// frw_groth16_verify_wire_dev itself is in frw_verify_dev.hip, next to the chain it feeds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_verify.h"
#include "frw_wire.h"

namespace frw {
namespace wire {
namespace {

__global__ __launch_bounds__(64) void wire_encode_proofs_kernel(uint64_t n, const uint64_t *__restrict__ proofs, int mode, uint8_t *__restrict__ out,
                                                                int32_t *__restrict__ status)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= n) return;
    status[g] = proof_encode(proofs + 48 * g, mode, out + proof_bytes(mode) * g) ? 0 : -1;
}

__global__ __launch_bounds__(64) void wire_g1_decode_kernel(uint64_t n, const uint8_t *__restrict__ in, int mode, uint64_t *__restrict__ proofs,
                                                            int32_t *__restrict__ status)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 64 + threadIdx.x) >> 1;
    if (g >= n) return;
    const bool odd = threadIdx.x & 1;
    const uint8_t *src = in + proof_bytes(mode) * g + (odd ? g1_bytes(mode) + g2_bytes(mode) : 0);
    const bool ok = g1_decode(src, mode, proofs + 48 * g + (odd ? 36 : 0));
    const uint32_t both = (ok ? 1u : 0u) & pair_swap_u32(ok ? 1u : 0u);
    if (!odd) status[g] = both ? 0 : -1;
}

__global__ __launch_bounds__(64) void wire_g2_decode_kernel(uint64_t n, const uint8_t *__restrict__ in, int mode, uint64_t *__restrict__ proofs,
                                                            int32_t *__restrict__ status)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= n) return;
    uint64_t *p = proofs + 48 * g;
    const bool ok = g2_decode(in + proof_bytes(mode) * g + g1_bytes(mode), mode, p + 12);
    if (!ok || status[g]) {
        status[g] = -1;
        proof_clear(p);
    }
}

__global__ __launch_bounds__(64) void wire_g1_run_decode_kernel(uint64_t n, const uint8_t *__restrict__ in, int mode, uint64_t *__restrict__ rows,
                                                                unsigned long long *__restrict__ first_bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (!g1_decode(in + g1_bytes(mode) * i, mode, rows + 12 * i)) atomicMin(first_bad, (unsigned long long)i);
}

bool mode_ok(int mode) { return mode == FRW_WIRE_COMPRESSED || mode == FRW_WIRE_UNCOMPRESSED; }

int have_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    const hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? FRW_OK : record_hip_error(e, "hipSetDevice");
}

// the key's header -- alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | le64(n) -- into limbs[0, 84) and *n; false if a point is malformed
bool vk_header_decode(const uint8_t *bytes, int mode, uint64_t *limbs, uint64_t *n)
{
    bool ok = g1_decode(bytes, mode, limbs);
    for (int j = 0; j < 3; j++) ok = g2_decode(bytes + g1_bytes(mode) + j * g2_bytes(mode), mode, limbs + 12 + 24 * j) && ok;
    const uint8_t *c = bytes + vk_header_bytes(mode) - 8;
    uint64_t v = 0;
    for (int k = 7; k >= 0; k--) v = v << 8 | c[k];
    *n = v;
    return ok;
}
// the embedded count if `len` is exactly the key's size for it (and the count is not zero), else 0
uint64_t vk_count(const uint8_t *bytes, size_t len, int mode)
{
    if (len < vk_header_bytes(mode)) return 0;
    const uint8_t *c = bytes + vk_header_bytes(mode) - 8;
    uint64_t n = 0;
    for (int k = 7; k >= 0; k--) n = n << 8 | c[k];
    const size_t rest = len - vk_header_bytes(mode);
    if (n == 0 || n > ((uint64_t)1 << 31) - 1 || rest % g1_bytes(mode) != 0 || rest / g1_bytes(mode) != n) return 0;
    return n;
}

}  // namespace

int decode_proofs_launch(size_t count, const uint8_t *d_wire, int mode, uint64_t *d_proofs, int32_t *d_status, hipStream_t st)
{
    hipLaunchKernelGGL(wire_g1_decode_kernel, dim3((unsigned)((2 * count + 63) / 64)), dim3(64), 0, st, (uint64_t)count, d_wire, mode, d_proofs, d_status);
    hipLaunchKernelGGL(wire_g2_decode_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, (uint64_t)count, d_wire, mode, d_proofs, d_status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : record_hip_error(e, "frw_groth16_proofs_from_wire_dev");
}

}  // namespace wire
}  // namespace frw

using namespace frw::wire;

extern "C" size_t frw_groth16_proof_wire_bytes(int mode) { return mode_ok(mode) ? proof_bytes(mode) : 0; }

extern "C" size_t frw_groth16_vk_wire_bytes(size_t num_instance, int mode)
{
    return mode_ok(mode) ? vk_header_bytes(mode) + num_instance * g1_bytes(mode) : 0;
}

extern "C" int frw_groth16_proofs_to_wire(size_t batch, const uint64_t *proofs, int mode, uint8_t *out, int32_t *status)
{
    if (!mode_ok(mode)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!proofs || !out || !status) return FRW_E_INVALID_ARG;
    const bool ok = frw::verify::for_each_proof(batch, [&](size_t i) { status[i] = proof_encode(proofs + 48 * i, mode, out + proof_bytes(mode) * i) ? 0 : -1; });
    return ok ? FRW_OK : FRW_E_OUT_OF_MEMORY;
}

extern "C" int frw_groth16_proofs_from_wire(size_t batch, const uint8_t *in, int mode, uint64_t *proofs, int32_t *status)
{
    if (!mode_ok(mode)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!in || !proofs || !status) return FRW_E_INVALID_ARG;
    const bool ok = frw::verify::for_each_proof(batch, [&](size_t i) { status[i] = proof_decode(in + proof_bytes(mode) * i, mode, proofs + 48 * i) ? 0 : -1; });
    return ok ? FRW_OK : FRW_E_OUT_OF_MEMORY;
}

extern "C" int frw_groth16_proofs_to_wire_dev(int device, size_t batch, const uint64_t *d_proofs, int mode, uint8_t *d_out, int32_t *d_status, void *stream)
{
    if (!mode_ok(mode) || (batch && (!d_proofs || !d_out || !d_status))) return FRW_E_INVALID_ARG;
    const int rc = have_device(device);
    if (rc != FRW_OK || batch == 0) return rc;
    hipLaunchKernelGGL(wire_encode_proofs_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (uint64_t)batch, d_proofs, mode,
                       d_out, d_status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : frw::record_hip_error(e, "frw_groth16_proofs_to_wire_dev");
}

extern "C" int frw_groth16_proofs_from_wire_dev(int device, size_t batch, const uint8_t *d_in, int mode, uint64_t *d_proofs, int32_t *d_status, void *stream)
{
    if (!mode_ok(mode) || (batch && (!d_in || !d_proofs || !d_status))) return FRW_E_INVALID_ARG;
    const int rc = have_device(device);
    if (rc != FRW_OK || batch == 0) return rc;
    return decode_proofs_launch(batch, d_in, mode, d_proofs, d_status, (hipStream_t)stream);
}

extern "C" int frw_groth16_vk_to_wire(const uint64_t *vk, size_t num_instance, int mode, uint8_t *out)
{
    if (!mode_ok(mode) || !vk || !out || num_instance == 0) return FRW_E_INVALID_ARG;
    bool ok = g1_encode(vk, mode, out);
    for (int j = 0; j < 3; j++) ok = g2_encode(vk + 12 + 24 * j, mode, out + g1_bytes(mode) + j * g2_bytes(mode)) && ok;
    uint8_t *c = out + vk_header_bytes(mode) - 8;
    for (int k = 0; k < 8; k++) c[k] = (uint8_t)((uint64_t)num_instance >> (8 * k));
    for (size_t i = 0; i < num_instance; i++) ok = g1_encode(vk + 84 + 12 * i, mode, out + vk_header_bytes(mode) + g1_bytes(mode) * i) && ok;
    if (!ok) memset(out, 0, vk_header_bytes(mode) + num_instance * g1_bytes(mode));
    return ok ? FRW_OK : FRW_E_INVALID_ARG;
}

extern "C" int frw_groth16_vk_load_wire(const uint8_t *bytes, size_t len, int mode, frw_groth16_vk **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    if (!mode_ok(mode) || !bytes) return FRW_E_INVALID_ARG;
    const uint64_t n = vk_count(bytes, len, mode);
    if (n == 0) return FRW_E_INVALID_ARG;
    try {
        std::vector<uint64_t> limbs(84 + 12 * (size_t)n);
        std::vector<uint8_t> bad((size_t)n, 0);
        uint64_t again = 0;
        if (!vk_header_decode(bytes, mode, limbs.data(), &again)) return FRW_E_INVALID_ARG;
        const uint8_t *rows = bytes + vk_header_bytes(mode);
        if (!frw::verify::for_each_proof((size_t)n, [&](size_t i) { bad[i] = g1_decode(rows + g1_bytes(mode) * i, mode, &limbs[84 + 12 * i]) ? 0 : 1; }))
            return FRW_E_OUT_OF_MEMORY;
        for (size_t i = 0; i < (size_t)n; i++)
            if (bad[i]) return FRW_E_INVALID_ARG;
        return frw_groth16_vk_load(limbs.data(), (size_t)n, out);
    } catch (const std::bad_alloc &) {
        return FRW_E_OUT_OF_MEMORY;
    }
}

extern "C" int frw_groth16_vk_load_wire_dev(int device, const uint8_t *bytes, size_t len, int mode, frw_groth16_vk **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    if (!mode_ok(mode) || !bytes) return FRW_E_INVALID_ARG;
    const uint64_t n = vk_count(bytes, len, mode);
    if (n == 0) return FRW_E_INVALID_ARG;
    const int rc = have_device(device);
    if (rc != FRW_OK) return rc;
    try {
        std::vector<uint64_t> limbs(84 + 12 * (size_t)n);
        uint64_t again = 0;
        if (!vk_header_decode(bytes, mode, limbs.data(), &again)) return FRW_E_INVALID_ARG;
        // gamma_abc_g1: decoded on the device, a lane per point
        const size_t in_bytes = (size_t)n * g1_bytes(mode);
        uint8_t *d_in = nullptr;
        uint64_t *d_rows = nullptr;
        unsigned long long *d_bad = nullptr, bad = ~0ull;
        hipError_t e = hipMalloc((void **)&d_in, in_bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&d_rows, (size_t)n * 96);
        if (e == hipSuccess) e = hipMalloc((void **)&d_bad, sizeof(bad));
        if (e == hipSuccess) e = hipMemcpy(d_in, bytes + vk_header_bytes(mode), in_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_bad, &bad, sizeof(bad), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(wire_g1_run_decode_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, n, (const uint8_t *)d_in, mode, d_rows,
                               d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(&limbs[84], d_rows, (size_t)n * 96, hipMemcpyDeviceToHost);
        if (d_in) (void)hipFree(d_in);
        if (d_rows) (void)hipFree(d_rows);
        if (d_bad) (void)hipFree(d_bad);
        if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_vk_load_wire_dev");
        if (bad != ~0ull) return FRW_E_INVALID_ARG;
        // every point checked (on the curve again, in the subgroup), no vouching flag
        return frw_groth16_vk_load_dev(device, limbs.data(), (size_t)n, 0, out);
    } catch (const std::bad_alloc &) {
        return FRW_E_OUT_OF_MEMORY;
    }
}

extern "C" int frw_diag_wire_greater(const uint64_t *c0, const uint64_t *c1)
{
    if (!c0) return FRW_E_INVALID_ARG;
    uint32_t a[12], b[12];
    memcpy(a, c0, 48);
    if (!c1) return words_greater(a) ? 1 : 0;
    memcpy(b, c1, 48);
    return words2_greater(a, b) ? 1 : 0;
}
