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
#include "frw_codec.h"
#include "frw_layout.h"

namespace frw {

// the three per-item functions -- one hash, one key coefficient, one signature -- are frw_codec.h's, where the host can compile them too
using codec::NONCE_LEN;
using codec::decode_signature_one;
using codec::hash_to_point_one;
using codec::public_key_coeff;
using codec::public_key_coeff_refused;
using codec::public_key_header_refused;

__global__ __launch_bounds__(BLOCK) void hash_to_point_kernel(int logn, size_t batch, const uint8_t *__restrict__ nonces,
                                                              const uint8_t *__restrict__ msgs,
                                                              const uint64_t *__restrict__ msg_off, uint16_t *__restrict__ hm)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= batch) return;
    const uint64_t o0 = msg_off[s], o1 = msg_off[s + 1];
    hash_to_point_one(logn, nonces + s * NONCE_LEN, msgs + o0, o0, o1, hm + (s << logn));
}

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
    const uint32_t c = public_key_coeff(p, k);
    pk[idx] = (uint16_t)c;
    if (public_key_coeff_refused(c) || (k == 0 && public_key_header_refused(p, logn))) atomicMax(&status[s], ST_DECODE);
}

__global__ __launch_bounds__(BLOCK) void decode_signatures_kernel(int logn, size_t batch, const uint8_t *__restrict__ sig_bytes,
                                                                  size_t sig_len, uint16_t *__restrict__ sig,
                                                                  uint8_t *__restrict__ nonce_out, int32_t *__restrict__ status)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= batch) return;
    const bool ok = decode_signature_one(logn, sig_bytes + s * sig_len, sig_len, sig + (s << logn),
                                         nonce_out ? nonce_out + s * NONCE_LEN : nullptr);
    status[s] = ok ? ST_OK : ST_DECODE;
}

// ---- the inputs of an aggregate (frw_aggregate_*_from_bytes_dev): the encoded keys and signatures of statements of BOTH parameter sets
// laid end to end in statement order, read where they lie.  One launch per parameter set and stage: item k of set g is statement
// stmt[k] (R1csAggSet::stmt), its bytes are where aggregate_route (frw_layout.h) says, its decoded row is row k of the set's dense
// array, which is what the per-set kernels downstream take.  Nonces stay in statement order.  The bodies are the kernels' above.
__global__ __launch_bounds__(BLOCK) void agg_hash_to_point_kernel(int logn, size_t count, const uint32_t *__restrict__ stmt,
                                                                  const uint8_t *__restrict__ nonces, const uint8_t *__restrict__ msgs,
                                                                  const uint64_t *__restrict__ msg_off, uint16_t *__restrict__ hm)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const size_t s = stmt[k];
    const uint64_t o0 = msg_off[s], o1 = msg_off[s + 1];
    hash_to_point_one(logn, nonces + aggregate_route(logn - 9, k, s).nonce_off, msgs + o0, o0, o1, hm + (k << logn));
}

__global__ __launch_bounds__(BLOCK) void agg_decode_public_keys_kernel(int logn, size_t count, const uint32_t *__restrict__ stmt,
                                                                       const uint8_t *__restrict__ pk_bytes, uint16_t *__restrict__ pk,
                                                                       int32_t *__restrict__ status)
{
    const int n = 1 << logn;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count * (size_t)n) return;
    const size_t k = idx >> logn;
    const int j = (int)(idx & (size_t)(n - 1));
    const uint8_t *p = pk_bytes + aggregate_route(logn - 9, k, stmt[k]).pk_off;
    const uint32_t c = public_key_coeff(p, j);
    pk[idx] = (uint16_t)c;                                   // row k of the set's dense array: idx = k N + j
    if (public_key_coeff_refused(c) || (j == 0 && public_key_header_refused(p, logn))) atomicMax(&status[k], ST_DECODE);
}

// the nonce is copied out whatever the header says: the verifier's statement is made from the 40 bytes after it, not from a verdict
__global__ __launch_bounds__(BLOCK) void agg_decode_signatures_kernel(int logn, size_t count, const uint32_t *__restrict__ stmt,
                                                                      const uint8_t *__restrict__ sig_bytes, uint16_t *__restrict__ sig,
                                                                      uint8_t *__restrict__ nonces, int32_t *__restrict__ status)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const AggRoute r = aggregate_route(logn - 9, k, stmt[k]);
    const uint8_t *p = sig_bytes + r.sig_off;
    for (int i = 0; i < NONCE_LEN; i++) nonces[r.nonce_off + i] = p[1 + i];
    status[k] = decode_signature_one(logn, p, aggregate_sig_len(logn - 9), sig + (k << logn), nullptr) ? ST_OK : ST_DECODE;
}

// the per-set screen's verdicts (and norms, where asked for) back into statement order: a lane per item of either set
struct AggVerdicts { const uint32_t *stmt[2]; const int32_t *status[2]; const uint64_t *norm[2]; uint32_t count[2]; };
__global__ __launch_bounds__(BLOCK) void agg_scatter_verdicts_kernel(AggVerdicts v, int32_t *__restrict__ status, uint64_t *__restrict__ norm)
{
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int g = 0;
    if (k >= v.count[0]) { k -= v.count[0]; g = 1; }
    if (k >= v.count[g]) return;
    const size_t s = v.stmt[g][k];
    status[s] = v.status[g][k];
    if (norm) norm[s] = v.norm[g][k];
}

// ONE workgroup: refused[0] = the statements whose status is not FRW_ST_OK -- the one value the aggregate prover's host side reads
__global__ __launch_bounds__(BLOCK) void agg_count_refused_kernel(size_t count, const int32_t *__restrict__ status, uint32_t *__restrict__ refused)
{
    __shared__ uint32_t wave_count[WAVES];
    uint32_t mine = 0;
    for (size_t s = threadIdx.x; s < count; s += BLOCK) mine += status[s] != ST_OK;
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_count[threadIdx.x / WAVE] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) total += wave_count[w];
        refused[0] = total;
    }
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

hipError_t launch_agg_hash_to_point(int logn, size_t count, const uint32_t *stmt, const uint8_t *nonces, const uint8_t *msgs,
                                    const uint64_t *msg_off, uint16_t *hm, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(agg_hash_to_point_kernel, dim3((unsigned)((count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, logn, count, stmt, nonces,
                       msgs, msg_off, hm);
    return hipGetLastError();
}

hipError_t launch_agg_decode_public_keys(int logn, size_t count, const uint32_t *stmt, const uint8_t *pk_bytes, uint16_t *pk, int32_t *status,
                                         hipStream_t st)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(status, 0, count * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const size_t total = count << logn;
    hipLaunchKernelGGL(agg_decode_public_keys_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, logn, count, stmt,
                       pk_bytes, pk, status);
    return hipGetLastError();
}

hipError_t launch_agg_decode_signatures(int logn, size_t count, const uint32_t *stmt, const uint8_t *sig_bytes, uint16_t *sig, uint8_t *nonces,
                                        int32_t *status, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(agg_decode_signatures_kernel, dim3((unsigned)((count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, logn, count, stmt,
                       sig_bytes, sig, nonces, status);
    return hipGetLastError();
}

hipError_t launch_agg_verdicts(const uint32_t *const stmt[2], const int32_t *const set_status[2], const uint64_t *const set_norm[2],
                               const size_t count[2], int32_t *status, uint64_t *norm, uint32_t *refused, hipStream_t st)
{
    const size_t total = count[0] + count[1];
    if (total == 0) return hipSuccess;
    const AggVerdicts v = {{stmt[0], stmt[1]}, {set_status[0], set_status[1]}, {set_norm[0], set_norm[1]}, {(uint32_t)count[0], (uint32_t)count[1]}};
    hipLaunchKernelGGL(agg_scatter_verdicts_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, v, status, norm);
    hipLaunchKernelGGL(agg_count_refused_kernel, dim3(1), dim3(BLOCK), 0, st, total, (const int32_t *)status, refused);
    return hipGetLastError();
}

}  // namespace frw
