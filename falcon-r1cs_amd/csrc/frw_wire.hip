// frw_wire.hip -- Groth16 proofs and verifying keys in ark-serialize's wire format (frw_wire.h has the format and the codec): the kernels
// that encode and decode them on the device, and the C ABI on both sides.  Host and device run the SAME functions of frw_wire.h, so their
// bytes and limbs agree by construction.
//   wire_encode_proofs_kernel     a lane per proof: twelve products, the rest is loads and stores
//   wire_g1_decode_kernel         two lanes per proof, A in the even lane and C in the odd one (proof_check_kernel's idiom): one
//                                 a^((q + 1) / 4) each when compressed -- ~610 dependent Fq products, one accumulator, no scratch
//   wire_g2_decode_kernel         a lane per proof for B: two such roots and an inversion (frw_wire.h fq2_sqrt_candidate); it runs after
//                                 the G1 kernel on the same stream, folds B's verdict into the proof's status and clears a refused proof
//   wire_g1_run_decode_kernel     a lane per point of a run of G1 points (a key's gamma_abc_g1); the first bad index goes back
//   wire_g2_run_decode_kernel     the same for a run of G2 points (a proving key's b_g2_query)
//   wire_run_subgroup_kernel<F>   r P = O for every decoded point of a run (frw_verify.h in_subgroup, the ladder every loader runs): a lane
//                                 per G1 point, the two-lane Fq2 (frw_fq29.h) per G2 point; infinity rows pass untouched
//   wire_rows_encode_kernel<F>    a lane per table ROW of a multi-scalar-multiplication handle: row -> ark-ff limbs -> bytes
// frw_groth16_verify_wire_dev itself is in frw_verify_dev.hip, next to the chain it feeds.  The proving key's functions
// (frw_groth16_pk_*wire*) are at the end: the framing on the host, every point of every run on the device, FRW_PK_WIRE_CHUNK_BYTES at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/frw.h"
#include "frw_device.h"
#include "frw_rows.h"
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

__global__ __launch_bounds__(64) void wire_g2_run_decode_kernel(uint64_t n, const uint8_t *__restrict__ in, int mode, uint64_t *__restrict__ rows,
                                                                unsigned long long *__restrict__ first_bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (!g2_decode(in + g2_bytes(mode) * i, mode, rows + 24 * i)) atomicMin(first_bad, (unsigned long long)i);
}

// rows: `n` decoded points in ark-ff's limbs (what the two run decoders write; a refused point is all zero = infinity and passes here: its
// index is in the decoder's own first_bad).  F::LANES lanes per point: FqField 1, Fq2PairField 2 (both lanes of a pair see the same point).
template <class F>
__global__ __launch_bounds__(64) void wire_run_subgroup_kernel(uint64_t n, const uint64_t *__restrict__ rows, unsigned long long *__restrict__ first_bad)
{
    const uint64_t i = ((uint64_t)blockIdx.x * 64 + threadIdx.x) / F::LANES;
    if (i >= n) return;
    const AffineT<F> p = load_ark_point<F>((const uint32_t *)rows + (size_t)Grp<F>::ARK_WORDS * i);
    if (!verify::in_subgroup(p)) atomicMin(first_bad, (unsigned long long)i);
}

// rows: `n` table rows of a handle (frw_rows.h; all zero = infinity, which encodes as infinity); out: n x g1_bytes / g2_bytes(mode)
template <class F>
__global__ __launch_bounds__(64) void wire_rows_encode_kernel(uint64_t n, const uint32_t *__restrict__ rows, int mode, uint8_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint64_t limbs[Grp<F>::ARK_WORDS / 2];
    store_ark_point<F>((uint32_t *)limbs, load_row<F>(rows + (size_t)Grp<F>::PT_WORDS * i));
    if (F::ARK_WORDS == 12) (void)g1_encode(limbs, mode, out + g1_bytes(mode) * i);
    else (void)g2_encode(limbs, mode, out + g2_bytes(mode) * i);
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

// ---- proving keys ---------------------------------------------------------------------------------------------------------------------------
namespace {
using frw::FqField;
using frw::Fq2Field;
using frw::Fq2PairField;

uint64_t le64(const uint8_t *c)
{
    uint64_t v = 0;
    for (int k = 7; k >= 0; k--) v = v << 8 | c[k];
    return v;
}
void put_le64(uint8_t *c, uint64_t v)
{
    for (int k = 0; k < 8; k++) c[k] = (uint8_t)(v >> (8 * k));
}
// the size of a key of these counts; 0 for counts no key has (or beyond 2^40: the sum below then cannot overflow)
size_t pk_bytes_for(uint64_t ni, uint64_t nw, uint64_t n, int mode)
{
    constexpr uint64_t CAP = (uint64_t)1 << 40;
    if (ni == 0 || ni >= CAP || nw >= CAP || n < 2 || n > CAP || (n & (n - 1))) return 0;
    const uint64_t nv = ni + nw;
    return vk_header_bytes(mode) + 5 * 8 + (ni + 2 + 2 * nv + (n - 1) + nw) * g1_bytes(mode) + nv * g2_bytes(mode);
}
// the framing: every length field is tested against what is left of the buffer BEFORE anything behind it is touched
bool pk_walk(const uint8_t *b, size_t len, int mode, frw_groth16_pk_wire_info_t *o)
{
    const size_t g1 = g1_bytes(mode), g2 = g2_bytes(mode);
    size_t pos = vk_header_bytes(mode);
    if (len < pos) return false;
    const uint64_t ni = le64(b + pos - 8);
    if (ni == 0 || ni > (len - pos) / g1) return false;
    pos += ni * g1;                                   // gamma_abc_g1
    if (len - pos < 2 * g1) return false;
    pos += 2 * g1;                                    // beta_g1, delta_g1
    uint64_t cnt[5], off[5];                          // a_query, b_g1_query, b_g2_query, h_query, l_query
    for (int k = 0; k < 5; k++) {
        const size_t pt = k == 2 ? g2 : g1;
        if (len - pos < 8) return false;
        cnt[k] = le64(b + pos);
        pos += 8;
        if (cnt[k] > (len - pos) / pt) return false;
        off[k] = pos;
        pos += cnt[k] * pt;
    }
    if (pos != len) return false;
    const uint64_t nv = cnt[0], n = cnt[3] + 1;
    if (cnt[1] != nv || cnt[2] != nv || nv < ni || cnt[4] != nv - ni) return false;
    if (n < 2 || (n & (n - 1))) return false;
    o->num_instance = ni; o->num_witness = nv - ni; o->domain_size = n;
    o->a_query_offset = off[0]; o->b_g1_query_offset = off[1]; o->b_g2_query_offset = off[2]; o->h_query_offset = off[3]; o->l_query_offset = off[4];
    return true;
}
frw::AffineT<Fq2Field> g2_from_ark(const uint64_t *w)
{
    frw::AffineT<Fq2Field> p;
    uint64_t any = 0;
    for (int k = 0; k < 24; k++) any |= w[k];
    p.inf = any == 0;
    p.x = Fq2Field::from_ark((const uint32_t *)w);
    p.y = Fq2Field::from_ark((const uint32_t *)(w + 12));
    return p;
}

// the device side of both directions: wire bytes of one chunk, its points in ark-ff's limbs, the two first-bad indices (decoder, subgroup)
struct PkStage {
    uint8_t *d_bytes = nullptr;
    uint64_t *d_limbs = nullptr;
    unsigned long long *d_bad = nullptr;
    hipError_t alloc(size_t bytes, size_t limb_bytes)
    {
        hipError_t e = hipMalloc((void **)&d_bytes, bytes);
        if (e == hipSuccess && limb_bytes) e = hipMalloc((void **)&d_limbs, limb_bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&d_bad, 2 * sizeof(unsigned long long));
        return e;
    }
    ~PkStage()
    {
        if (d_bytes) (void)hipFree(d_bytes);
        if (d_limbs) (void)hipFree(d_limbs);
        if (d_bad) (void)hipFree(d_bad);
    }
};
size_t chunk_points(size_t point_bytes) { return FRW_PK_WIRE_CHUNK_BYTES / point_bytes; }

// One run of `count` points of group 1 or 2 at `src`: staged, decoded and (check) tested for the subgroup a chunk at a time; sink(lo, cnt,
// d_limbs) takes each chunk's decoded limbs where they are, in device memory.  FRW_E_INVALID_ARG names the run and the first bad index.
template <class Sink>
int pk_decode_run(const char *name, int group, const uint8_t *src, uint64_t count, int mode, bool check, PkStage &s, Sink sink)
{
    const size_t pt = group == 1 ? g1_bytes(mode) : g2_bytes(mode);
    const uint64_t per = chunk_points(pt);
    for (uint64_t lo = 0; lo < count; lo += per) {
        const uint64_t cnt = std::min<uint64_t>(per, count - lo);
        unsigned long long bad[2] = {~0ull, ~0ull};
        hipError_t e = hipMemcpy(s.d_bytes, src + lo * pt, cnt * pt, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s.d_bad, bad, sizeof(bad), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            const dim3 grid((unsigned)((cnt + 63) / 64));
            if (group == 1) {
                hipLaunchKernelGGL(wire_g1_run_decode_kernel, grid, dim3(64), 0, nullptr, cnt, (const uint8_t *)s.d_bytes, mode, s.d_limbs, s.d_bad);
                if (check) hipLaunchKernelGGL(wire_run_subgroup_kernel<FqField>, grid, dim3(64), 0, nullptr, cnt, (const uint64_t *)s.d_limbs, s.d_bad + 1);
            } else {
                hipLaunchKernelGGL(wire_g2_run_decode_kernel, grid, dim3(64), 0, nullptr, cnt, (const uint8_t *)s.d_bytes, mode, s.d_limbs, s.d_bad);
                if (check)
                    hipLaunchKernelGGL(wire_run_subgroup_kernel<Fq2PairField>, dim3((unsigned)((2 * cnt + 63) / 64)), dim3(64), 0, nullptr, cnt,
                                       (const uint64_t *)s.d_limbs, s.d_bad + 1);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = sink(lo, cnt, (const uint64_t *)s.d_limbs);
        if (e == hipSuccess) e = hipMemcpy(bad, s.d_bad, sizeof(bad), hipMemcpyDeviceToHost);       // (waits for the chunk's kernels)
        if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_pk_load_wire_dev");
        if (bad[0] != ~0ull || bad[1] != ~0ull) {
            if (bad[0] != ~0ull && bad[0] <= bad[1])
                frw::record_error("frw_groth16_pk_load_wire_dev: %s[%llu] is malformed", name, (unsigned long long)(lo + bad[0]));
            else
                frw::record_error("frw_groth16_pk_load_wire_dev: %s[%llu] is not in the subgroup of order r", name, (unsigned long long)(lo + bad[1]));
            return FRW_E_INVALID_ARG;
        }
    }
    return FRW_OK;
}

// rows [first, first + count) of a handle as wire bytes into HOST memory at dst, a chunk at a time
int pk_encode_rows(const frw_msm *m, uint64_t first, uint64_t count, int mode, PkStage &s, uint8_t *dst)
{
    int group = 0;
    uint64_t rows = 0;
    const uint32_t *table = frw::msm_point_rows(m, &group, &rows);
    if (first + count > rows) return FRW_E_INVALID_ARG;
    const size_t pt = group == 1 ? g1_bytes(mode) : g2_bytes(mode);
    const size_t pw = group == 1 ? frw::Grp<FqField>::PT_WORDS : frw::Grp<Fq2Field>::PT_WORDS;
    const uint64_t per = chunk_points(pt);
    for (uint64_t lo = 0; lo < count; lo += per) {
        const uint64_t cnt = std::min<uint64_t>(per, count - lo);
        const dim3 grid((unsigned)((cnt + 63) / 64));
        const uint32_t *src = table + (first + lo) * pw;
        if (group == 1) hipLaunchKernelGGL(wire_rows_encode_kernel<FqField>, grid, dim3(64), 0, nullptr, cnt, src, mode, s.d_bytes);
        else hipLaunchKernelGGL(wire_rows_encode_kernel<Fq2Field>, grid, dim3(64), 0, nullptr, cnt, src, mode, s.d_bytes);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(dst + lo * pt, s.d_bytes, cnt * pt, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_pk_to_wire_dev");
    }
    return FRW_OK;
}
}  // namespace

extern "C" size_t frw_groth16_pk_wire_bytes(uint64_t num_instance, uint64_t num_witness, uint64_t domain_size, int mode)
{
    return mode_ok(mode) ? pk_bytes_for(num_instance, num_witness, domain_size, mode) : 0;
}

extern "C" int frw_groth16_pk_wire_info(const uint8_t *bytes, size_t len, int mode, frw_groth16_pk_wire_info_t *out)
{
    if (!bytes || !out || !mode_ok(mode)) return FRW_E_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    frw_groth16_pk_wire_info_t w;
    if (!pk_walk(bytes, len, mode, &w)) return FRW_E_INVALID_ARG;
    *out = w;
    return FRW_OK;
}

extern "C" int frw_groth16_pk_load_wire_dev(int device, const uint8_t *bytes, size_t len, int mode, int flags, const frw_groth16_key_opts_t *opts,
                                            frw_groth16_pk **pk_out, uint64_t *vk_out)
{
    if (!pk_out) return FRW_E_INVALID_ARG;
    *pk_out = nullptr;
    if (!mode_ok(mode) || !bytes || (flags & ~FRW_PK_POINTS_ARE_CHECKED)) return FRW_E_INVALID_ARG;
    int key_mode = opts ? opts->mode : FRW_KEY_AUTO;
    if (key_mode != FRW_KEY_AUTO && key_mode != FRW_KEY_TABLES && key_mode != FRW_KEY_BARE) return FRW_E_INVALID_ARG;
    if (opts && (opts->world > 1 || opts->rank != 0)) return FRW_E_INVALID_ARG;        // (a key in slices from wire bytes: out of scope)
    frw_groth16_pk_wire_info_t w;
    if (!pk_walk(bytes, len, mode, &w)) {
        frw::record_error("frw_groth16_pk_load_wire_dev: the framing (lengths that disagree, a truncated or over-long buffer)");
        return FRW_E_INVALID_ARG;
    }
    const uint64_t ni = w.num_instance, nw = w.num_witness, n = w.domain_size, nv = ni + nw;
    if (nv + 3 >= ((uint64_t)1 << 31) || n > ((uint64_t)1 << 31)) return FRW_E_INVALID_ARG;
    if (key_mode == FRW_KEY_AUTO) key_mode = nv > FRW_KEY_AUTO_TABLE_VARIABLES ? FRW_KEY_BARE : FRW_KEY_TABLES;
    int rc = have_device(device);
    if (rc != FRW_OK) return rc;
    const bool check = !(flags & FRW_PK_POINTS_ARE_CHECKED);
    const size_t g1 = g1_bytes(mode), g2 = g2_bytes(mode);

    // the seven fixed points, on the host by the same codec: alpha_g1 | beta_g2 | gamma_g2 | delta_g2 (the key's header), beta_g1, delta_g1
    uint64_t head[84], fixed_g1[24], count_again = 0;
    const uint8_t *after_vk = bytes + vk_header_bytes(mode) + ni * g1;
    if (!vk_header_decode(bytes, mode, head, &count_again) || !g1_decode(after_vk, mode, fixed_g1) || !g1_decode(after_vk + g1, mode, fixed_g1 + 12)) {
        frw::record_error("frw_groth16_pk_load_wire_dev: one of the seven fixed points (the verifying key's, beta_g1, delta_g1) is malformed");
        return FRW_E_INVALID_ARG;
    }
    if (check) {
        bool in = frw::verify::in_subgroup(frw::verify::g1_lazy_from_ark(head));
        for (int j = 0; j < 3; j++) in = in && frw::verify::in_subgroup(g2_from_ark(head + 12 + 24 * j));
        for (int j = 0; j < 2; j++) in = in && frw::verify::in_subgroup(frw::verify::g1_lazy_from_ark(fixed_g1 + 12 * j));
        if (!in) {
            frw::record_error("frw_groth16_pk_load_wire_dev: one of the seven fixed points is not in the subgroup of order r");
            return FRW_E_INVALID_ARG;
        }
    }

    // the six runs, on the device: the bytes through d_bytes a chunk at a time, the decoded limbs from d_limbs straight into the tables' rows
    PkStage s;
    frw_msm *t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};                    // h, a, b1, l, b2
    {
        const uint64_t most_g1 = std::max(std::max(ni, nv), n - 1);
        const size_t pts1 = (size_t)std::min<uint64_t>(most_g1, chunk_points(g1)), pts2 = (size_t)std::min<uint64_t>(nv, chunk_points(g2));
        const hipError_t e = s.alloc(std::max(pts1 * g1, pts2 * g2), std::max<size_t>(std::max(pts1 * 96, pts2 * 192), 144 * 8));
        if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_pk_load_wire_dev");
    }
    rc = frw::msm_alloc_bare(device, 1, 16, n - 1, 0, &t[0]);
    for (int k = 1; k < 5 && rc == FRW_OK; k++) rc = frw::msm_alloc_bare(device, k == 4 ? 2 : 1, 8, nv + 3, 0, &t[k]);
    auto into = [&](frw_msm *m, uint64_t row0) {
        return [m, row0](uint64_t lo, uint64_t cnt, const uint64_t *d_limbs) { return frw::msm_fill_ark_dev(m, row0 + lo, cnt, (const uint32_t *)d_limbs, nullptr); };
    };
    if (rc == FRW_OK)
        rc = pk_decode_run("gamma_abc_g1", 1, bytes + vk_header_bytes(mode), ni, mode, check, s, [&](uint64_t lo, uint64_t cnt, const uint64_t *d_limbs) {
            return vk_out ? hipMemcpy(vk_out + 84 + 12 * lo, d_limbs, cnt * 96, hipMemcpyDeviceToHost) : hipSuccess;
        });
    if (rc == FRW_OK) rc = pk_decode_run("a_query", 1, bytes + w.a_query_offset, nv, mode, check, s, into(t[1], 0));
    if (rc == FRW_OK) rc = pk_decode_run("b_g1_query", 1, bytes + w.b_g1_query_offset, nv, mode, check, s, into(t[2], 0));
    if (rc == FRW_OK) rc = pk_decode_run("b_g2_query", 2, bytes + w.b_g2_query_offset, nv, mode, check, s, into(t[4], 0));
    if (rc == FRW_OK) rc = pk_decode_run("h_query", 1, bytes + w.h_query_offset, n - 1, mode, check, s, into(t[0], 0));
    if (rc == FRW_OK) rc = pk_decode_run("l_query", 1, bytes + w.l_query_offset, nw, mode, check, s, into(t[3], ni));
    if (rc == FRW_OK) {
        // the three padding rows of the witness-side tables (frw_groth16_pk_load_opts): a_query ++ [alpha, delta, O], b_g1_query ++ [beta, O, O],
        // O x I ++ l_query ++ [O, O, O], b_g2_query ++ [beta2, O, delta2]
        uint64_t tail[144] = {0};
        memcpy(tail, head, 96);                          // a: alpha_g1
        memcpy(tail + 12, fixed_g1 + 12, 96);            //    delta_g1
        memcpy(tail + 36, fixed_g1, 96);                 // b1: beta_g1
        memcpy(tail + 72, head + 12, 192);               // b2: beta_g2
        memcpy(tail + 72 + 48, head + 60, 192);          //     delta_g2
        hipError_t e = hipMemcpy(s.d_limbs, tail, sizeof(tail), hipMemcpyHostToDevice);
        const uint32_t *d_tail = (const uint32_t *)s.d_limbs;
        if (e == hipSuccess) e = frw::msm_fill_ark_dev(t[1], nv, 3, d_tail, nullptr);
        if (e == hipSuccess) e = frw::msm_fill_ark_dev(t[2], nv, 3, d_tail + 2 * 36, nullptr);
        if (e == hipSuccess) e = frw::msm_fill_ark_dev(t[4], nv, 3, d_tail + 2 * 72, nullptr);
        if (e == hipSuccess) e = frw::msm_fill_ark_dev(t[3], 0, ni, nullptr, nullptr);
        if (e == hipSuccess) e = frw::msm_fill_ark_dev(t[3], nv, 3, nullptr, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = frw::record_hip_error(e, "frw_groth16_pk_load_wire_dev: the padding rows");
    }
    // a key of window tables grows them from the rows, as a key made on the device does
    if (key_mode == FRW_KEY_TABLES)
        for (int k = 0; k < 5 && rc == FRW_OK; k++) rc = frw::msm_expand_tables(&t[k]);
    if (rc != FRW_OK) {
        for (frw_msm *m : t) frw_msm_free(m);
        return rc;
    }
    rc = frw::groth16_pk_assemble(device, ni, nw, n, 0, 1, t[0], t[1], t[2], t[3], t[4], pk_out);
    if (rc == FRW_OK && vk_out) memcpy(vk_out, head, sizeof(head));
    return rc;
}

extern "C" int frw_groth16_pk_to_wire_dev(const frw_groth16_pk *pk, const uint64_t *vk, size_t num_instance, int mode, uint8_t *out, size_t out_len)
{
    if (!pk || !vk || !out || !mode_ok(mode)) return FRW_E_INVALID_ARG;
    frw_groth16_pk_info_t info;
    if (frw_groth16_pk_info(pk, &info) != FRW_OK || info.world > 1) return FRW_E_INVALID_ARG;
    int device = 0;
    uint64_t ni = 0, nw = 0, n = 0;
    frw::groth16_pk_counts(pk, &device, &ni, &nw, &n);
    const uint64_t nv = ni + nw;
    if (num_instance != ni || out_len == 0 || out_len != pk_bytes_for(ni, nw, n, mode)) return FRW_E_INVALID_ARG;
    int rc = have_device(device);
    if (rc != FRW_OK) return rc;
    const size_t g1 = g1_bytes(mode), g2 = g2_bytes(mode);
    const frw_msm *h = frw_groth16_pk_query(pk, FRW_QUERY_H), *a = frw_groth16_pk_query(pk, FRW_QUERY_A), *b1 = frw_groth16_pk_query(pk, FRW_QUERY_B1),
                  *l = frw_groth16_pk_query(pk, FRW_QUERY_L), *b2 = frw_groth16_pk_query(pk, FRW_QUERY_B2);
    // what the handle does not hold, from the caller's limbs on the host: gamma_g2, gamma_abc_g1
    uint8_t *abc = out + vk_header_bytes(mode);
    std::atomic<bool> canonical{g2_encode(vk + 36, mode, out + g1 + g2)};
    put_le64(abc - 8, ni);
    if (!frw::verify::for_each_proof((size_t)ni, [&](size_t i) { if (!g1_encode(vk + 84 + 12 * i, mode, abc + g1 * i)) canonical = false; }))
        return FRW_E_OUT_OF_MEMORY;
    if (!canonical) {
        frw::record_error("frw_groth16_pk_to_wire_dev: a coordinate of gamma_g2 or gamma_abc_g1 is not below the field modulus");
        return FRW_E_INVALID_ARG;
    }
    // everything else from the handle's own rows, encoded on the device
    PkStage s;
    {
        const uint64_t most_g1 = std::max(nv, n - 1);
        const size_t pts1 = (size_t)std::min<uint64_t>(most_g1, chunk_points(g1)), pts2 = (size_t)std::min<uint64_t>(nv, chunk_points(g2));
        const hipError_t e = s.alloc(std::max(pts1 * g1, pts2 * g2), 0);
        if (e != hipSuccess) return frw::record_hip_error(e, "frw_groth16_pk_to_wire_dev");
    }
    rc = pk_encode_rows(a, nv, 1, mode, s, out);                                           // alpha_g1
    if (rc == FRW_OK) rc = pk_encode_rows(b2, nv, 1, mode, s, out + g1);                   // beta_g2
    if (rc == FRW_OK) rc = pk_encode_rows(b2, nv + 2, 1, mode, s, out + g1 + 2 * g2);      // delta_g2
    uint8_t *p = abc + ni * g1;
    if (rc == FRW_OK) rc = pk_encode_rows(b1, nv, 1, mode, s, p);                          // beta_g1
    if (rc == FRW_OK) rc = pk_encode_rows(a, nv + 1, 1, mode, s, p + g1);                  // delta_g1
    p += 2 * g1;
    struct Run { const frw_msm *m; uint64_t first, count; size_t pt; };
    const Run runs[5] = {{a, 0, nv, g1}, {b1, 0, nv, g1}, {b2, 0, nv, g2}, {h, 0, n - 1, g1}, {l, ni, nw, g1}};
    for (const Run &r : runs) {
        if (rc != FRW_OK) break;
        put_le64(p, r.count);
        rc = pk_encode_rows(r.m, r.first, r.count, mode, s, p + 8);
        p += 8 + r.count * r.pt;
    }
    if (rc == FRW_OK && p != out + out_len) rc = FRW_E_INVALID_ARG;
    return rc;
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
