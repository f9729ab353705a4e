// frw_prepare.hip -- input preparation in front of the witness kernels: what the reference does
// with falcon-rust before any gadget runs (falcon-r1cs/src/circuits/falcon_ntt.rs:27-28,44):
//     sig_poly = Polynomial::from(&sig)            -> decode_signatures_kernel   (Falcon spec Alg. 18, Decompress)
//     pk_poly  = Polynomial::from(&pk)             -> decode_public_keys_kernel  (14-bit modq_decode)
//     hm       = Polynomial::from_hash_of_message(msg, sig.nonce())  -> hash_to_point_kernel (SHAKE256, Alg. 3)
// falcon-rust is not under /root/reference; the formats are the Falcon specification's (v1.2 sections 3.7, 3.11).
//
// These kernels are latency/ALU work on a few KB per signature (Keccak-f[1600]: ~17 permutations per Falcon-1024
// hash), two orders of magnitude below the witness kernel's 5 MB write stream; one lane per signature keeps every
// lane of a wavefront in the same permutation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "frw_device.h"
#include "frw_keccak.h"

namespace frw {

constexpr int SHAKE256_RATE = 136;
constexpr int NONCE_LEN = 40;

// hm = HashToPoint(nonce || msg): SHAKE256, big-endian 16-bit words, accept w < 5q as w mod q (Falcon spec Alg. 3)
__global__ __launch_bounds__(BLOCK) void hash_to_point_kernel(int logn, size_t batch, const uint8_t *__restrict__ nonces,
                                                              const uint8_t *__restrict__ msgs,
                                                              const uint64_t *__restrict__ msg_off, uint16_t *__restrict__ hm)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= batch) return;
    const int n = 1 << logn;
    const uint8_t *nonce = nonces + s * NONCE_LEN;
    const uint8_t *msg = msgs + msg_off[s];
    // the host entry point rejects decreasing offsets; a device-side caller that breaks the precondition of
    // include/frw.h gets an empty message here rather than a 2^64-byte absorb loop
    const uint64_t o0 = msg_off[s], o1 = msg_off[s + 1];
    const size_t total = NONCE_LEN + (size_t)(o1 >= o0 ? o1 - o0 : 0);
    uint64_t st[25];
#pragma unroll
    for (int i = 0; i < 25; i++) st[i] = 0;
    // absorb nonce || msg || pad10*1 with the SHAKE domain bits (0x1F ... 0x80)
    for (size_t pos = 0;; pos += SHAKE256_RATE) {
#pragma unroll
        for (int l = 0; l < SHAKE256_RATE / 8; l++) {
            uint64_t w = 0;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const size_t p = pos + (size_t)(l * 8 + b);
                uint32_t byte = 0;
                if (p < NONCE_LEN) byte = nonce[p];
                else if (p < total) byte = msg[p - NONCE_LEN];
                else if (p == total) byte = 0x1F;
                w |= (uint64_t)byte << (8 * b);
            }
            st[l] ^= w;
        }
        const bool last = total < pos + SHAKE256_RATE;
        if (last) st[16] ^= 0x8000000000000000ull;
        keccak_f1600(st);
        if (last) break;
    }
    // squeeze
    uint16_t *out = hm + s * (size_t)n;
    int cnt = 0;
    while (cnt < n) {
#pragma unroll
        for (int w = 0; w < SHAKE256_RATE / 2; w++) {
            const uint64_t lane = st[w / 4];
            const int sh = (w % 4) * 16;
            const uint32_t v = (uint32_t)((lane >> sh) & 0xff) << 8 | (uint32_t)((lane >> (sh + 8)) & 0xff);
            if (v < 5 * Q && cnt < n) out[cnt++] = (uint16_t)(v % Q);
        }
        if (cnt < n) keccak_f1600(st);
    }
}

// pk: header 0x00 + logn, then N x 14 bits, big-endian bit order
__global__ __launch_bounds__(BLOCK) void decode_public_keys_kernel(int logn, size_t batch, const uint8_t *__restrict__ pk_bytes,
                                                                   uint16_t *__restrict__ pk, int32_t *__restrict__ status)
{
    const int n = 1 << logn;
    const size_t pk_len = 1 + (size_t)14 * n / 8;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * (size_t)n) return;
    const size_t s = idx >> logn;
    const int k = (int)(idx & (size_t)(n - 1));
    const uint8_t *p = pk_bytes + s * pk_len;
    const int bit = 14 * k, off = bit & 7;
    const uint8_t *q = p + 1 + (bit >> 3);
    uint32_t acc = (uint32_t)q[0] << 16 | (uint32_t)q[1] << 8;
    if (off + 14 > 16) acc |= q[2];
    const uint32_t c = (acc >> (24 - 14 - off)) & 0x3fffu;
    pk[idx] = (uint16_t)c;
    if (c >= Q || (k == 0 && p[0] != (uint8_t)logn)) atomicMax(&status[s], ST_DECODE);
}

// sig: header 0x30 + logn, 40-byte nonce, compressed coefficients, zero padding up to sig_len
__global__ __launch_bounds__(BLOCK) void decode_signatures_kernel(int logn, size_t batch, const uint8_t *__restrict__ sig_bytes,
                                                                  size_t sig_len, uint16_t *__restrict__ sig,
                                                                  uint8_t *__restrict__ nonce_out, int32_t *__restrict__ status)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= batch) return;
    const int n = 1 << logn;
    const uint8_t *p = sig_bytes + s * sig_len;
    uint16_t *out = sig + s * (size_t)n;
    bool ok = sig_len > 1 + NONCE_LEN && p[0] == (uint8_t)(0x30 + logn);
    if (ok && nonce_out)
        for (int i = 0; i < NONCE_LEN; i++) nonce_out[s * NONCE_LEN + i] = p[1 + i];
    const uint8_t *body = p + 1 + NONCE_LEN;
    const size_t body_len = ok ? sig_len - 1 - NONCE_LEN : 0;
    size_t v = 0;
    uint32_t acc = 0;
    int acc_len = 0;
    for (int u = 0; ok && u < n; u++) {
        if (v >= body_len) { ok = false; break; }
        acc = (acc << 8) | body[v++];
        const uint32_t b = acc >> acc_len;
        const uint32_t sign = b & 128u;
        uint32_t m = b & 127u;
        for (;;) {
            if (acc_len == 0) {
                if (v >= body_len) { ok = false; break; }
                acc = (acc << 8) | body[v++];
                acc_len = 8;
            }
            acc_len--;
            if ((acc >> acc_len) & 1u) break;
            m += 128;
            if (m > 2047) { ok = false; break; }
        }
        if (sign && m == 0) ok = false;             // "-0" is not a valid encoding
        if (ok) out[u] = (uint16_t)(sign ? Q - m : m);
    }
    if (ok && (acc & ((1u << acc_len) - 1u))) ok = false;          // unused bits of the last byte
    for (; ok && v < body_len; v++)
        if (body[v]) ok = false;                                    // padding
    status[s] = ok ? ST_OK : ST_DECODE;
}

// ---- compaction for the prover from bytes (frw_pok_prove_from_bytes_dev): the witness and prover calls take dense batches, the caller's
// batch has refused slots anywhere in it.  An order-preserving scan over the status words lists the accepted slots, gathers make their
// inputs dense a chunk at a time, and after the prover a scatter puts every result back into its slot.  All of it is index arithmetic
// on a few KB per signature, next to the prover's sums over the whole key.

// the rank of this thread's flag among the set flags of its workgroup (exclusive), and their number in `total`
__device__ inline uint32_t pok_block_rank(bool flag, uint32_t &total)
{
    __shared__ uint32_t wave_count[WAVES];
    const uint64_t mask = __ballot(flag);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        if (w < wave) before += wave_count[w];
        total += wave_count[w];
    }
    return before + (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1));
}

// pass 1: accepted slots (status == FRW_ST_OK) of every block of BLOCK slots
__global__ __launch_bounds__(BLOCK) void pok_scan_count_kernel(size_t batch, const int32_t *__restrict__ status,
                                                               uint32_t *__restrict__ block_sums)
{
    const size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t total;
    (void)pok_block_rank(s < batch && status[s] == ST_OK, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// pass 2, ONE workgroup: block_sums -> the accepted slots before each block (in place), their number -> count[0]
__global__ __launch_bounds__(BLOCK) void pok_scan_offsets_kernel(size_t num_blocks, uint32_t *__restrict__ block_sums,
                                                                 uint32_t *__restrict__ count)
{
    __shared__ uint32_t wave_sum[WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    uint32_t carry = 0;
    for (size_t base = 0; base < num_blocks; base += BLOCK) {
        const size_t i = base + threadIdx.x;
        const uint32_t v = i < num_blocks ? block_sums[i] : 0;
        uint32_t incl = v;                                  // inclusive scan inside the wavefront
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, WAVE);
            if (lane >= d) incl += up;
        }
        if (lane == WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            if (w < wave) before += wave_sum[w];
            tile += wave_sum[w];
        }
        if (i < num_blocks) block_sums[i] = carry + before + incl - v;
        carry += tile;
        __syncthreads();                                    // wave_sum is written again by the next tile
    }
    if (threadIdx.x == 0) count[0] = carry;
}

// pass 3: index[j] = the j-th accepted slot
__global__ __launch_bounds__(BLOCK) void pok_scan_write_kernel(size_t batch, const int32_t *__restrict__ status,
                                                               const uint32_t *__restrict__ block_offsets, uint32_t *__restrict__ index)
{
    const size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool ok = s < batch && status[s] == ST_OK;
    uint32_t total;
    const uint32_t rank = pok_block_rank(ok, total);
    if (ok) index[block_offsets[blockIdx.x] + rank] = (uint32_t)s;
}

// dense_rs[j] = rs[index[j]]: eight words per proof, a lane per word
__global__ __launch_bounds__(BLOCK) void pok_gather_rs_kernel(size_t count, const uint32_t *__restrict__ index,
                                                              const uint64_t *__restrict__ rs, uint64_t *__restrict__ dense_rs)
{
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count * 8) return;
    dense_rs[t] = rs[(size_t)index[t / 8] * 8 + (t & 7)];
}

// the (sig, pk, hm) rows of the chunk's slots, a workgroup per signature, 16 bytes per lane (the rows are N x 2 bytes, 16-byte aligned)
__global__ __launch_bounds__(BLOCK) void pok_gather_inputs_kernel(int logn, const uint32_t *__restrict__ index,
                                                                  const uint16_t *__restrict__ sig, const uint16_t *__restrict__ pk,
                                                                  const uint16_t *__restrict__ hm, uint16_t *__restrict__ sig_out,
                                                                  uint16_t *__restrict__ pk_out, uint16_t *__restrict__ hm_out)
{
    const size_t j = blockIdx.x, slot = index[j];
    const uint32_t row = (2u << logn) / 16;                 // uint4 per row
    for (uint32_t t = threadIdx.x; t < 3 * row; t += BLOCK) {
        const uint32_t a = t / row, v = t % row;
        const uint16_t *src = a == 0 ? sig : a == 1 ? pk : hm;
        uint16_t *dst = a == 0 ? sig_out : a == 1 ? pk_out : hm_out;
        ((uint4 *)dst)[j * row + v] = ((const uint4 *)src)[slot * row + v];
    }
}

// What the outputs of a slot are: its wire bytes (any alignment), and where asked for (non-null) the proof's 48 limbs, its instance
// vector of inst_words uint64_t and its count of violated rows.
struct PokOutputs { uint8_t *wire; uint64_t *proofs, *instance; uint32_t *unsatisfied; uint32_t wire_len, inst_words; };

// every refused slot (status != FRW_ST_OK): all-zero bytes in every output; a workgroup per slot, strided over the grid
__global__ __launch_bounds__(BLOCK) void pok_zero_refused_kernel(size_t batch, const int32_t *__restrict__ status, PokOutputs out)
{
    for (size_t s = blockIdx.x; s < batch; s += gridDim.x) {
        if (status[s] == ST_OK) continue;
        for (uint32_t t = threadIdx.x; t < out.wire_len; t += BLOCK) out.wire[s * out.wire_len + t] = 0;
        if (out.proofs && threadIdx.x < 48) out.proofs[s * 48 + threadIdx.x] = 0;
        if (out.instance)
            for (uint32_t t = threadIdx.x; t < out.inst_words; t += BLOCK) out.instance[s * out.inst_words + t] = 0;
        if (out.unsatisfied && threadIdx.x == 0) out.unsatisfied[s] = 0;
    }
}

// the chunk's results into their slots: result j of the chunk belongs to slot index[j]; a workgroup per result
__global__ __launch_bounds__(BLOCK) void pok_scatter_kernel(const uint32_t *__restrict__ index, const uint8_t *__restrict__ wire,
                                                            const uint64_t *__restrict__ proofs, const uint64_t *__restrict__ instance,
                                                            const uint32_t *__restrict__ unsatisfied, PokOutputs out)
{
    const size_t j = blockIdx.x, s = index[j];
    for (uint32_t t = threadIdx.x; t < out.wire_len; t += BLOCK) out.wire[s * out.wire_len + t] = wire[j * out.wire_len + t];
    if (out.proofs && threadIdx.x < 48) out.proofs[s * 48 + threadIdx.x] = proofs[j * 48 + threadIdx.x];
    if (out.instance)
        for (uint32_t t = threadIdx.x; t < out.inst_words; t += BLOCK) out.instance[s * out.inst_words + t] = instance[j * out.inst_words + t];
    if (out.unsatisfied && threadIdx.x == 0) out.unsatisfied[s] = unsatisfied[j];
}

hipError_t launch_pok_scan(size_t batch, const int32_t *status, uint32_t *block_sums, uint32_t *index, uint32_t *count, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    const size_t blocks = (batch + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(pok_scan_count_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, st, batch, status, block_sums);
    hipLaunchKernelGGL(pok_scan_offsets_kernel, dim3(1), dim3(BLOCK), 0, st, blocks, block_sums, count);
    hipLaunchKernelGGL(pok_scan_write_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, st, batch, status, (const uint32_t *)block_sums, index);
    return hipGetLastError();
}

hipError_t launch_pok_gather_rs(size_t count, const uint32_t *index, const uint64_t *rs, uint64_t *dense_rs, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(pok_gather_rs_kernel, dim3((unsigned)((count * 8 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, count, index, rs, dense_rs);
    return hipGetLastError();
}

hipError_t launch_pok_gather_inputs(int logn, size_t cnt, const uint32_t *index, const uint16_t *sig, const uint16_t *pk, const uint16_t *hm,
                                    uint16_t *sig_out, uint16_t *pk_out, uint16_t *hm_out, hipStream_t st)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(pok_gather_inputs_kernel, dim3((unsigned)cnt), dim3(BLOCK), 0, st, logn, index, sig, pk, hm, sig_out, pk_out, hm_out);
    return hipGetLastError();
}

hipError_t launch_pok_zero_refused(size_t batch, const int32_t *status, int wire_len, int inst_words, uint8_t *wire, uint64_t *proofs,
                                   uint64_t *instance, uint32_t *unsatisfied, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    const PokOutputs out = {wire, proofs, instance, unsatisfied, (uint32_t)wire_len, (uint32_t)inst_words};
    hipLaunchKernelGGL(pok_zero_refused_kernel, dim3((unsigned)std::min<size_t>(batch, 65536)), dim3(BLOCK), 0, st, batch, status, out);
    return hipGetLastError();
}

hipError_t launch_pok_scatter(size_t cnt, const uint32_t *index, int wire_len, int inst_words, const uint8_t *wire_in,
                              const uint64_t *proofs_in, const uint64_t *instance_in, const uint32_t *unsatisfied_in, uint8_t *wire,
                              uint64_t *proofs, uint64_t *instance, uint32_t *unsatisfied, hipStream_t st)
{
    if (cnt == 0) return hipSuccess;
    const PokOutputs out = {wire, proofs, instance, unsatisfied, (uint32_t)wire_len, (uint32_t)inst_words};
    hipLaunchKernelGGL(pok_scatter_kernel, dim3((unsigned)cnt), dim3(BLOCK), 0, st, index, wire_in, proofs_in, instance_in, unsatisfied_in, out);
    return hipGetLastError();
}

hipError_t launch_hash_to_point(int logn, size_t batch, const uint8_t *nonces, const uint8_t *msgs, const uint64_t *msg_off,
                                uint16_t *hm, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(hash_to_point_kernel, dim3((unsigned)((batch + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, logn, batch, nonces,
                       msgs, msg_off, hm);
    return hipGetLastError();
}

hipError_t launch_decode_public_keys(int logn, size_t batch, const uint8_t *pk_bytes, uint16_t *pk, int32_t *status, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(status, 0, batch * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const size_t total = batch << logn;
    hipLaunchKernelGGL(decode_public_keys_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, logn, batch,
                       pk_bytes, pk, status);
    return hipGetLastError();
}

hipError_t launch_decode_signatures(int logn, size_t batch, const uint8_t *sig_bytes, size_t sig_len, uint16_t *sig,
                                    uint8_t *nonce_out, int32_t *status, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(decode_signatures_kernel, dim3((unsigned)((batch + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, logn, batch,
                       sig_bytes, sig_len, sig, nonce_out, status);
    return hipGetLastError();
}

}  // namespace frw
