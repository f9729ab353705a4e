// frw_drbg.hip -- drawing Groth16's blinding and re-randomising factors on the device (frw_drbg.h has the derivation), so that a captured
// prover or re-randomiser is fresh on every replay with the host out of the loop:
//   fr_draw_kernel          one lane per scalar, the Keccak state in the lane's registers as in hash_to_point (frw_prepare.hip); workgroups
//                           of 64, so that the few scalars of a small batch still spread over the CUs.  Reads *counter and the seed.
//   fr_draw_advance_kernel  one thread: *counter += 1, modulo 2^64.  A launch of its own BEHIND the draw on the same stream, so that every
//                           lane of the draw has read the old value: no atomics, no ticket.
// Both on the caller's stream alone, nothing allocated, copied or synchronised: capture-safe, no parallel branches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_drbg.h"
#include "frw_keccak.h"

namespace frw {
namespace drbg {
namespace {

__global__ __launch_bounds__(64) void fr_draw_kernel(uint64_t first, uint64_t n, const uint8_t *__restrict__ seed, const uint64_t *__restrict__ counter,
                                                     int tag, uint64_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = first + i;
    uint64_t a[25], x[4];
    absorb(seed, *counter, tag, j, a);
    keccak_f1600(a);
    squeeze(a, x);
    uint64_t *o = out + 4 * j;
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = x[3];
}

__global__ __launch_bounds__(64) void fr_draw_advance_kernel(uint64_t *counter)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *counter = *counter + 1;
}

constexpr uint64_t LANES_PER_LAUNCH = 1ull << 30;                       // (a grid's x dimension is below 2^31 workgroups)

}  // namespace

int draw_launch(const uint8_t *d_seed, const uint64_t *d_counter, int tag, size_t count, uint64_t *d_out, void *stream)
{
    for (uint64_t lo = 0; lo < count; lo += LANES_PER_LAUNCH) {
        const uint64_t n = count - lo < LANES_PER_LAUNCH ? count - lo : LANES_PER_LAUNCH;
        hipLaunchKernelGGL(fr_draw_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, lo, n, d_seed, d_counter, tag, d_out);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : record_hip_error(e, "frw_fr_draw_dev");
}

int advance_launch(uint64_t *d_counter, void *stream)
{
    hipLaunchKernelGGL(fr_draw_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_counter);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FRW_OK : record_hip_error(e, "frw_fr_draw_dev");
}

}  // namespace drbg
}  // namespace frw

using namespace frw::drbg;

extern "C" int frw_fr_draw(const uint8_t seed[32], uint64_t counter, int tag, size_t count, uint64_t *out)
{
    if (count == 0) return FRW_OK;
    if (!seed || !out || tag < 0 || tag > 255) return FRW_E_INVALID_ARG;
    for (size_t j = 0; j < count; j++) draw_one_host(seed, counter, tag, (uint64_t)j, out + 4 * j);
    return FRW_OK;
}

extern "C" int frw_fr_draw_dev(int device, const uint8_t *d_seed, uint64_t *d_counter, int tag, size_t count, uint64_t *d_out, void *stream)
{
    if (count == 0) return FRW_OK;
    if (!d_seed || !d_counter || !d_out || tag < 0 || tag > 255) return FRW_E_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FRW_E_NO_DEVICE;
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return frw::record_hip_error(e, "hipSetDevice");
    const int rc = draw_launch(d_seed, d_counter, tag, count, d_out, stream);
    return rc == FRW_OK ? advance_launch(d_counter, stream) : rc;
}
