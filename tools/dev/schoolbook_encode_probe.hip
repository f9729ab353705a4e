// The two routes to mont(sig[j] * b) of the schoolbook kernel's columns, one field element a lane each, for an
// instruction count of the emitted gfx950 code (no GPU needed):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S tools/dev/schoolbook_encode_probe.hip -o probe.s
// and count the v_ instructions between each probe kernel's label and its s_endpgm (tools/dev/schoolbook_encode_count.py).
//   probe_cios   the route the kernel uses: prod = sig[j] * b as an integer, one one-word CIOS round (encode_u32<1>)
//   probe_small  mont(sig[j]) made once per signature (here: loaded), times the 14-bit b, reduced by a quotient estimate
// probe_small loads its Montgomery element from GLOBAL memory (eight dword loads and their addresses); the real route would read it
// from LDS (two ds_read_b128), so its 216 instructions are the probe's, not the in-kernel cost: compare the vector ALU and the
// v_mad_u64_u32 columns.  The include below brings in the whole kernel file for encode_u32 / cond_sub_p; only the two probes are emitted.
#include "../../falcon-r1cs_amd/csrc/frw_kernels.hip"

namespace frw {

// M < p, b <= q < 2^14: M * b mod p.  x = M b < 2^14 p; its top 29 bits against (p >> 240) + 1 = 0x73ee give a quotient that is
// never above floor(x / p) and at most one below it, so one conditional subtraction finishes.
__device__ __forceinline__ void mul_small_mod_p(const uint32_t (&M)[8], uint32_t b, uint32_t (&out)[8])
{
    constexpr uint32_t P[8] = FRW_P32;
    uint32_t T[9];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t acc = (uint64_t)M[j] * b + c;
        T[j] = (uint32_t)acc;
        c = (uint32_t)(acc >> 32);
    }
    T[8] = c;
    const uint32_t qe = ((T[8] << 16) | (T[7] >> 16)) / 0x73eeu;
    uint32_t bw = 0;
    c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t acc = (uint64_t)qe * P[j] + c;
        c = (uint32_t)(acc >> 32);
        const uint64_t d = (uint64_t)T[j] - (uint32_t)acc - bw;
        T[j] = (uint32_t)d;
        bw = (uint32_t)(d >> 63);
    }
    T[8] = 0;                                   // the remainder is below 2 p < 2^256
    cond_sub_p(T, out);
}

__global__ void probe_cios(const uint16_t *sig, const uint16_t *bb, uint32_t *out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t e8[8];
    encode_u32<1>((uint32_t)sig[k] * bb[k], e8);
#pragma unroll
    for (int j = 0; j < 8; j++) out[j * gridDim.x * blockDim.x + k] = e8[j];
}

__global__ void probe_small(const uint32_t *msig, const uint16_t *bb, uint32_t *out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, n = gridDim.x * blockDim.x;
    uint32_t M[8], e8[8];
#pragma unroll
    for (int j = 0; j < 8; j++) M[j] = msig[j * n + k];
    mul_small_mod_p(M, bb[k], e8);
#pragma unroll
    for (int j = 0; j < 8; j++) out[j * n + k] = e8[j];
}

}  // namespace frw
