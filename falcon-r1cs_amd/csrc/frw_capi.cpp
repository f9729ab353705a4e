// frw_capi.cpp -- the C ABI of include/frw.h over the gfx950 kernels of frw_kernels.hip.
// Host-side only: contexts, table construction, argument checking, chunked host-buffer variants.
// There is deliberately no CPU compute path here: without a HIP device every entry point that
// would produce a witness returns FRW_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <new>
#include <vector>

#include "../../include/frw.h"
#include "frw_arena.h"
#include "frw_device.h"
#include "frw_stage.h"

struct frw_ctx {
    int device;
    int num_cu;
    frw::Tables *d_tables;
    frw::HostArena arena;            // streams, events, device and page-locked memory of the host-buffer entry points
    // the fields registered with frw_ctx_field_encoding: encoding FRW_ENC_FIELD_BASE + i is fields[i]; lives and dies with the context
    int num_fields;
    uint64_t field_modulus[FRW_MAX_FIELDS][4];
    frw::FieldConsts fields[FRW_MAX_FIELDS];
};

namespace {

thread_local char g_last_error[256] = "";

int hip_fail(hipError_t e, const char *what)
{
    snprintf(g_last_error, sizeof g_last_error, "%s: %s", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? FRW_E_OUT_OF_MEMORY : FRW_E_HIP;
}

#define FRW_HIP(call)                                     \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

uint32_t powmod(uint32_t b, uint32_t e)
{
    uint64_t r = 1, x = b;
    while (e) {
        if (e & 1) r = r * x % frw::Q;
        x = x * x % frw::Q;
        e >>= 1;
    }
    return (uint32_t)r;
}

// falcon-rust NTT_TABLE[i] = 7^bitrev10(i) mod q (script/ntt_param.sage:3-132: Falcon's GMb / R);
// C_k = 2^k q^(k+1) (falcon_ntt.rs:31-39).
void build_tables(frw::Tables &t)
{
    for (uint32_t i = 0; i < 1024; i++) {
        uint32_t r = 0;
        for (int b = 0; b < 10; b++)
            if (i & (1u << b)) r |= 1u << (9 - b);
        t.tw[i] = (uint16_t)powmod(7, r);
        t.itw[i] = (uint16_t)powmod(7, (2048 - r) % 2048);
    }
    uint32_t c[5] = {frw::Q, 0, 0, 0, 0};
    memcpy(t.ck[0], c, sizeof c);
    for (int k = 1; k <= 10; k++) {
        uint64_t carry = 0;
        for (int i = 0; i < 5; i++) {
            carry += (uint64_t)c[i] * (2 * frw::Q);
            c[i] = (uint32_t)carry;
            carry >>= 32;
        }
        memcpy(t.ck[k], c, sizeof c);
    }
    frw::schoolbook_inverses(t.sb_qinv, t.sb_nqinv);
}

bool bad_common(const frw_ctx *ctx, int logn, int encoding)
{
    return !ctx || (logn != 9 && logn != 10) || (encoding != FRW_ENC_CANONICAL && encoding != FRW_ENC_MONTGOMERY);
}

// An encoding of the ABI as the kernels know it: canonical, Montgomery and compact as they are, a field registered on the context
// (FRW_ENC_FIELD_BASE + i) as ENC 3 with its constants.  False: not an encoding; an id that this context did not hand out is none.
bool kernel_encoding(const frw_ctx *ctx, int encoding, frw::KernelEnc *ke)
{
    *ke = frw::KernelEnc(encoding);
    if (encoding == FRW_ENC_CANONICAL || encoding == FRW_ENC_MONTGOMERY || encoding == FRW_ENC_COMPACT) return true;
    if (!ctx || encoding < FRW_ENC_FIELD_BASE || encoding >= FRW_ENC_FIELD_BASE + ctx->num_fields) return false;
    *ke = frw::KernelEnc(3, &ctx->fields[encoding - FRW_ENC_FIELD_BASE]);
    return true;
}
// the calls that take the two BLS12-381 encodings or a registered field
bool bad_field_common(const frw_ctx *ctx, int logn, int encoding, frw::KernelEnc *ke)
{
    return !ctx || (logn != 9 && logn != 10) || !kernel_encoding(ctx, encoding, ke) || ke->enc == FRW_ENC_COMPACT;
}
// The encodings a witness circuit takes.  NTT: canonical, Montgomery, compact, a registered field; dual and schoolbook: canonical and
// Montgomery only (no compact form, and their field inverses are made by BLS12-381 host code).
bool bad_witness(const frw_ctx *ctx, int circuit, int logn, int encoding, frw::KernelEnc *ke)
{
    return !ctx || (logn != 9 && logn != 10) || !kernel_encoding(ctx, encoding, ke) || (circuit != FRW_CIRCUIT_NTT && ke->enc > FRW_ENC_MONTGOMERY);
}


// frw_layout*: the segment table of a circuit's witness laid end to end.  The counts are frw::circuit_shape's; the table has to add up
// to its witness count.
template <class Layout, int N> int fill_layout(int circuit, int logn, const int (&len)[N], Layout *out)
{
    const frw::CircuitShape shape = frw::circuit_shape(circuit, logn);
    int off = 0;
    out->logn = logn;
    out->n = (int)shape.n;
    for (int i = 0; i < N; i++) {
        out->seg_off[i] = off;
        out->seg_len[i] = len[i];
        off += len[i];
    }
    out->num_witness = (int)shape.num_witness;
    out->num_instance = (int)shape.num_instance;
    out->num_constraints = (int)shape.num_constraints;
    if ((size_t)off == shape.num_witness) return FRW_OK;
    snprintf(g_last_error, sizeof g_last_error, "frw_layout: the segments of circuit %d add up to %d, not to its %zu witness variables", circuit, off,
             shape.num_witness);
    return FRW_E_INVALID_ARG;
}
}  // namespace

namespace frw {
int record_hip_error(hipError_t e, const char *what) { return hip_fail(e, what); }
void record_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
}
}  // namespace frw

extern "C" {

int frw_layout(int logn, frw_layout_t *out)
{
    if (!out || (logn != 9 && logn != 10)) return FRW_E_INVALID_ARG;
    const int n = 1 << logn, nb = logn == 9 ? 50 : 52;
    const int len[FRW_NUM_SEGMENTS] = {n, n, 27 * n, 29 * n, 29 * n, 30 * n, 36 * n, nb};
    return fill_layout(FRW_CIRCUIT_NTT, logn, len, out);
}

const char *frw_strerror(int code)
{
    switch (code) {
    case FRW_OK: return "ok";
    case FRW_E_INVALID_ARG: return "invalid argument";
    case FRW_E_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
    case FRW_E_HIP: return "HIP runtime error (see frw_last_error)";
    case FRW_E_OUT_OF_MEMORY: return "out of device memory";
    case FRW_E_RANGE: return "strict mode: a signature failed its range checks";
    default: return "unknown error";
    }
}

const char *frw_last_error(void) { return g_last_error; }

int frw_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int frw_ctx_create(int device, frw_ctx **out)
{
    if (!out) return FRW_E_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        snprintf(g_last_error, sizeof g_last_error, "no HIP device %d (%d visible)", device, n);
        return FRW_E_NO_DEVICE;
    }
    FRW_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    FRW_HIP(hipGetDeviceProperties(&prop, device));
    frw_ctx *ctx = new (std::nothrow) frw_ctx;
    if (!ctx) return FRW_E_OUT_OF_MEMORY;
    ctx->device = device;
    ctx->num_cu = prop.multiProcessorCount;
    ctx->d_tables = nullptr;
    ctx->num_fields = 0;
    frw::Tables host;
    build_tables(host);
    hipError_t e = hipMalloc((void **)&ctx->d_tables, sizeof(frw::Tables));
    if (e == hipSuccess) e = hipMemcpy(ctx->d_tables, &host, sizeof host, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = ctx->arena.init();
    if (e != hipSuccess) {
        frw_ctx_destroy(ctx);
        return hip_fail(e, "context setup");
    }
    // everything a launch needs is known now (residency of the persistent kernels): the _dev entry points are one
    // kernel launch each -- no allocation, no query, no per-launch device state -- and therefore stream-capture safe
    frw::init_launch_config();
    *out = ctx;
    return FRW_OK;
}

void frw_ctx_destroy(frw_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->d_tables) (void)hipFree(ctx->d_tables);
    ctx->arena.destroy();
    delete ctx;
}

int frw_diag_host_allocations(frw_ctx *ctx, uint64_t *count)
{
    if (!ctx || !count) return FRW_E_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->arena.mu);
    *count = ctx->arena.allocations;
    return FRW_OK;
}

int frw_ctx_trim(frw_ctx *ctx)
{
    if (!ctx) return FRW_E_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->arena.mu);
    FRW_HIP(hipSetDevice(ctx->device));
    ctx->arena.trim();
    return FRW_OK;
}

int frw_ntt_modq_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_poly, int encoding, uint64_t *d_witness,
                     uint16_t *d_ntt_out, int32_t *d_status, void *stream)
{
    frw::KernelEnc ke;
    if (bad_field_common(ctx, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_poly || !d_witness || !d_ntt_out || !d_status) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_ntt_modq(ctx->d_tables, ctx->num_cu, logn, ke, batch, d_poly, d_witness, d_ntt_out, d_status, (hipStream_t)stream));
    return FRW_OK;
}

namespace {
bool any_refused(const int32_t *status, size_t batch)
{
    bool any_bad = false;
    for (size_t i = 0; i < batch; i++) any_bad |= status[i] != FRW_ST_OK;
    return any_bad;
}
// what a strict host-buffer call returns once its passes are through: the buffers are complete either way
int strict_verdict(int rc, int strict, const int32_t *status, size_t batch)
{
    return rc != FRW_OK ? rc : strict && any_refused(status, batch) ? FRW_E_RANGE : FRW_OK;
}
// rows lo .. lo + cnt - 1 of each of `src` (uint16_t[batch][n]) one after the other into the page-locked `stage`, and from there to d_in:
// ONE host-to-device copy whatever memory the caller holds the polynomials in
hipError_t stage_rows(std::initializer_list<const uint16_t *> src, size_t n, size_t lo, size_t cnt, char *stage, void *d_in, hipStream_t st)
{
    char *h = stage;
    for (const uint16_t *rows : src) {
        memcpy(h, rows + lo * n, cnt * n * 2);
        h += cnt * n * 2;
    }
    return hipMemcpyAsync(d_in, stage, (size_t)(h - stage), hipMemcpyHostToDevice, st);
}
// the witness kernel of a circuit (the NTT circuit's compact form: d_witness is the compact buffer, d_instance unused)
hipError_t launch_witness(const frw_ctx *ctx, int circuit, int logn, frw::KernelEnc ke, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk,
                          const uint16_t *d_hm, void *d_witness, uint64_t *d_instance, int32_t *d_status, hipStream_t st)
{
    if (circuit == FRW_CIRCUIT_SCHOOLBOOK)
        return frw::launch_witness_schoolbook_verify(ctx->d_tables, ctx->num_cu, logn, ke.enc, batch, d_sig, d_pk, d_hm, (uint64_t *)d_witness,
                                                     d_instance, d_status, st);
    if (circuit == FRW_CIRCUIT_DUAL_NTT)
        return frw::launch_witness_dual_ntt_verify(ctx->d_tables, ctx->num_cu, logn, ke.enc, batch, d_sig, d_pk, d_hm, (uint64_t *)d_witness,
                                                   d_instance, d_status, st);
    return frw::launch_witness_ntt_verify(ctx->d_tables, ctx->num_cu, logn, ke, batch, d_sig, d_pk, d_hm, d_witness, d_instance, d_status, st);
}

// The device-buffer witness calls of the three circuits: one kernel launch on the caller's stream.  The compact form's d_witness is the
// compact buffer (16-byte aligned), its d_instance is unused and may be NULL.
int witness_dev(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk, const uint16_t *d_hm,
                int encoding, void *d_witness, uint64_t *d_instance, int32_t *d_status, void *stream)
{
    frw::KernelEnc ke;
    if (bad_witness(ctx, circuit, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    const bool compact = ke.enc == FRW_ENC_COMPACT;
    if (!d_sig || !d_pk || !d_hm || !d_witness || (!d_instance && !compact) || !d_status) return FRW_E_INVALID_ARG;
    if (compact && ((uintptr_t)d_witness & 15)) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(launch_witness(ctx, circuit, logn, ke, batch, d_sig, d_pk, d_hm, d_witness, d_instance, d_status, (hipStream_t)stream));
    return FRW_OK;
}

// The host-buffer witness calls of the three circuits.  The pass loop is frw::host_passes (frw_arena.h); this says what a pass is: the
// three polynomials of a chunk staged and copied in at once, the circuit's kernel, and witness, instance and status on the way out.  A
// batch that fits one chunk -- the reference's own call pattern is one signature per generate_constraints -- takes one slot and one
// stream: copy in, kernel, copies out, one synchronisation.  A longer one takes two, so that a chunk's witness leaves while the next
// one is computed.
int witness_host(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint16_t *sig, const uint16_t *pk,
                 const uint16_t *hm, int encoding, uint64_t *witness, uint64_t *instance, int32_t *status, int strict)
{
    frw::KernelEnc ke;
    if (bad_witness(ctx, circuit, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    const bool compact = ke.enc == FRW_ENC_COMPACT;                                     // `witness` = compact buffer, `instance` unused
    if (batch == 0) return FRW_OK;
    if (!sig || !pk || !hm || !witness || (!instance && !compact) || !status) return FRW_E_INVALID_ARG;
    const frw::CircuitShape shape = frw::circuit_shape(circuit, logn);
    const size_t n = shape.n;
    const size_t wbytes = compact ? frw::compact_layout(logn).bytes : shape.num_witness * 32;
    const size_t ibytes = compact ? 0 : shape.num_instance * 32;
    // 2 x (<= 1.6 GB) of device witness; a schoolbook witness is 10.0 | 36.8 MB, so a slot holds 128 | 32 of them (1.3 | 1.2 GB)
    const size_t chunk = std::min<size_t>(batch, compact ? 2048 : circuit == FRW_CIRCUIT_SCHOOLBOOK ? (logn == 9 ? 128 : 32) : 256);
    const size_t in_bytes = 3 * chunk * n * 2;                              // sig | pk | hm of one chunk, contiguous
    frw::Carve c(nullptr);
    const size_t o_in = c.off;   c.take(in_bytes);
    const size_t o_wit = c.off;  c.take(chunk * wbytes);
    const size_t o_inst = c.off; c.take(chunk * ibytes + 16);
    const size_t o_st = c.off;   c.take(chunk * sizeof(int32_t));
    const int rc = frw::host_passes(
        ctx->arena, ctx->device, batch, chunk, batch > chunk ? 2 : 1, c.off, in_bytes,
        {{witness, o_wit, wbytes}, {compact ? nullptr : instance, o_inst, ibytes}, {status, o_st, sizeof(int32_t)}},
        [&](char *d, char *stage, size_t lo, size_t cnt, hipStream_t st) -> int {
            const uint16_t *d_in = (const uint16_t *)(d + o_in);
            FRW_HIP(stage_rows({sig, pk, hm}, n, lo, cnt, stage, d + o_in, st));
            FRW_HIP(launch_witness(ctx, circuit, logn, ke, cnt, d_in, d_in + cnt * n, d_in + 2 * cnt * n, d + o_wit,
                                   (uint64_t *)(d + o_inst), (int32_t *)(d + o_st), st));
            return FRW_OK;
        });
    return strict_verdict(rc, strict, status, batch);
}
}  // namespace

int frw_witness_ntt_verify(frw_ctx *ctx, int logn, size_t batch, const uint16_t *sig, const uint16_t *pk,
                           const uint16_t *hm, int encoding, uint64_t *witness, uint64_t *instance, int32_t *status,
                           int strict)
{
    return witness_host(ctx, FRW_CIRCUIT_NTT, logn, batch, sig, pk, hm, encoding, witness, instance, status, strict);
}

int frw_witness_ntt_verify_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk,
                               const uint16_t *d_hm, int encoding, uint64_t *d_witness, uint64_t *d_instance,
                               int32_t *d_status, void *stream)
{
    return witness_dev(ctx, FRW_CIRCUIT_NTT, logn, batch, d_sig, d_pk, d_hm, encoding, d_witness, d_instance, d_status, stream);
}

int frw_witness_dual_ntt_verify(frw_ctx *ctx, int logn, size_t batch, const uint16_t *sig, const uint16_t *pk,
                                const uint16_t *hm, int encoding, uint64_t *witness, uint64_t *instance,
                                int32_t *status, int strict)
{
    return witness_host(ctx, FRW_CIRCUIT_DUAL_NTT, logn, batch, sig, pk, hm, encoding, witness, instance, status, strict);
}

int frw_witness_dual_ntt_verify_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk,
                                    const uint16_t *d_hm, int encoding, uint64_t *d_witness, uint64_t *d_instance,
                                    int32_t *d_status, void *stream)
{
    return witness_dev(ctx, FRW_CIRCUIT_DUAL_NTT, logn, batch, d_sig, d_pk, d_hm, encoding, d_witness, d_instance, d_status, stream);
}

int frw_compact_layout(int logn, frw_compact_layout_t *out)
{
    if (!out || (logn != 9 && logn != 10)) return FRW_E_INVALID_ARG;
    const frw::CompactLayout c = frw::compact_layout(logn);
    const uint64_t n = (uint64_t)1 << logn, seg = 27 * n;
    out->logn = logn;
    out->n = (int32_t)n;
    out->bytes_per_signature = c.bytes;
    out->small_off = 0;
    out->num_small = c.num_small;
    out->t_off = c.t_off;
    out->num_t = c.num_t;
    out->bits_off = c.bits_off;
    out->num_bit_words = c.bit_words;
    for (int i = 0; i < 5; i++) out->bit_seg_off[i] = (uint64_t)i * seg;
    out->bit_seg_off[5] = 4 * seg + 32 * n;
    out->instance_off = c.instance_off;
    out->num_instance_values = c.num_instance;
    out->status_off = c.status_off;
    return FRW_OK;
}

int frw_witness_ntt_verify_compact_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk,
                                       const uint16_t *d_hm, void *d_compact, int32_t *d_status, void *stream)
{
    return witness_dev(ctx, FRW_CIRCUIT_NTT, logn, batch, d_sig, d_pk, d_hm, FRW_ENC_COMPACT, d_compact, nullptr, d_status, stream);
}

int frw_expand_dev(frw_ctx *ctx, int logn, size_t batch, const void *d_compact, uint64_t *d_witness, uint64_t *d_instance,
                   void *stream)
{
    if (bad_common(ctx, logn, FRW_ENC_MONTGOMERY)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_compact || !d_witness || !d_instance || ((uintptr_t)d_compact & 15)) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_expand(ctx->num_cu, logn, FRW_ENC_MONTGOMERY, batch, d_compact, d_witness, d_instance, (hipStream_t)stream));
    return FRW_OK;
}

// Host-side expansion of compact signatures received over PCIe: a format conversion (integers -> ark-ff's Montgomery
// representation, bits -> 0 / 1 elements), the counterpart of frw_expand_dev for a consumer that wants arkworks' vectors
// in host memory.  BLS12-381 scalar field, 64-bit limbs.
namespace {
constexpr uint64_t FR_P[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
constexpr uint64_t FR_R2[4] = {0xc999e990f3f29c6dull, 0x2b6cedcb87925c23ull, 0x05d314967254398full, 0x0748d9d99f59ff11ull};
constexpr uint64_t FR_ONE[4] = {0x00000001fffffffeull, 0x5884b7fa00034802ull, 0x998c4fefecbc4ff5ull, 0x1824b159acc5056full};
constexpr uint64_t FR_INV = 0xfffffffeffffffffull;          // -p^-1 mod 2^64

// out = x * 2^256 mod p for x < 2^192 given as three 64-bit limbs: Montgomery product of x and R^2 (CIOS)
inline void fr_to_montgomery(const uint64_t x[3], uint64_t out[4])
{
    typedef unsigned __int128 u128;
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        const uint64_t xi = i < 3 ? x[i] : 0;
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)xi * FR_R2[j] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * FR_INV;
        c = ((u128)m * FR_P[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * FR_P[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    uint64_t d[4];
    unsigned borrow = 0;
    for (int j = 0; j < 4; j++) {
        const u128 diff = (u128)t[j] - FR_P[j] - borrow;
        d[j] = (uint64_t)diff;
        borrow = (unsigned)((diff >> 64) & 1);
    }
    const bool ge = t[4] != 0 || !borrow;
    for (int j = 0; j < 4; j++) out[j] = ge ? d[j] : t[j];
}

// The relayout of frw_expand_host for any field.  What an element is comes from the caller: fr_to_montgomery(x as three 64-bit limbs, out)
// and FR_ONE, the field's one -- under the names the body had when BLS12-381's were the only ones.
extern "C++" template <class ToField>
int expand_host_with(int logn, size_t batch, const void *compact, uint64_t *witness, uint64_t *instance, const uint64_t (&FR_ONE)[4],
                     ToField fr_to_montgomery)
{
    const frw::CompactLayout c = frw::compact_layout(logn);
    const frw::CircuitShape shape = frw::circuit_shape(FRW_CIRCUIT_NTT, logn);
    const size_t n = shape.n, nb = shape.nb, W = shape.num_witness, I = shape.num_instance;
    for (size_t s = 0; s < batch; s++) {
        const unsigned char *base = (const unsigned char *)compact + s * c.bytes;
        const uint32_t *small = (const uint32_t *)base;                   // next small value
        const uint32_t *tq = (const uint32_t *)(base + c.t_off);           // next 5-limb quotient
        const uint32_t *bits = (const uint32_t *)(base + c.bits_off);
        const uint32_t *ins = (const uint32_t *)(base + c.instance_off);
        size_t bit = 0;
        uint64_t *w = witness + s * W * 4, *in = instance + s * I * 4;
        if (*(const uint32_t *)(base + c.status_off) == (uint32_t)FRW_ST_COEFF_RANGE) {   // rejected: zeros, as the direct path
            memset(w, 0, W * 32);
            memset(in, 0, I * 32);
            continue;
        }
        auto value = [&](int count) {
            for (int i = 0; i < count; i++, w += 4) {
                const uint64_t x[3] = {*small++, 0, 0};
                fr_to_montgomery(x, w);
            }
        };
        auto quotient = [&]() {
            const uint64_t x[3] = {(uint64_t)tq[0] | ((uint64_t)tq[1] << 32), (uint64_t)tq[2] | ((uint64_t)tq[3] << 32), tq[4]};
            fr_to_montgomery(x, w);
            tq += 5;
            w += 4;
        };
        auto booleans = [&](int count) {
            for (int i = 0; i < count; i++, bit++, w += 4) {
                if ((bits[bit >> 5] >> (bit & 31)) & 1u) memcpy(w, FR_ONE, 32);
                else memset(w, 0, 32);
            }
        };
        memcpy(in, FR_ONE, 32);
        for (size_t k = 0; k < 2 * n; k++) {
            const uint64_t x[3] = {ins[k], 0, 0};
            fr_to_montgomery(x, in + 4 + 4 * k);
        }
        value((int)(2 * n));                                              // S0, S1
        booleans((int)(27 * n));                                          // S2
        // S3, S4: [t, b, 27 booleans]; the b values of S3 (N) and of S4 (N) follow sig and v in `small`, the quotients of
        // S3 then S4 are in `t`
        for (int seg = 0; seg < 2; seg++)
            for (size_t k = 0; k < n; k++) { quotient(); value(1); booleans(27); }
        for (size_t k = 0; k < n; k++) { value(3); booleans(27); }         // S5: [prod, t, c, 27 booleans]
        for (size_t k = 0; k < 2 * n; k++) { booleans(16); value(2); }     // S6: [16 booleans, r, sq]
        bit = (4 * c.seg_words + n) * 32;                                 // S7 has two words of its own
        booleans((int)nb);
    }
    return FRW_OK;
}
}  // namespace

int frw_expand_host(int logn, size_t batch, const void *compact, uint64_t *witness, uint64_t *instance)
{
    if ((logn != 9 && logn != 10) || (batch && (!compact || !witness || !instance))) return FRW_E_INVALID_ARG;
    return expand_host_with(logn, batch, compact, witness, instance, FR_ONE, fr_to_montgomery);
}

// ---- any four-limb scalar field (frw_field.h): constants of a modulus, the context's registry, the compact expansion ------------
namespace {
void limbs64(const uint32_t (&w)[8], uint64_t out[4])
{
    for (int j = 0; j < 4; j++) out[j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
}
}  // namespace

int frw_field_info(const uint64_t modulus[4], frw_field_info_t *out)
{
    frw::FieldDerived d;
    if (!modulus || !out || !frw::field_derive(modulus, &d)) return FRW_E_INVALID_ARG;
    limbs64(d.fc.p, out->modulus);
    limbs64(d.fc.one, out->one);
    limbs64(d.r2, out->r2);
    out->ninv32 = d.fc.ninv32;
    out->bits = d.bits;
    return FRW_OK;
}

int frw_ctx_field_encoding(frw_ctx *ctx, const uint64_t modulus[4], int *encoding)
{
    frw::FieldDerived d;
    if (!ctx || !modulus || !encoding || !frw::field_derive(modulus, &d)) return FRW_E_INVALID_ARG;
    for (int i = 0; i < ctx->num_fields; i++)
        if (!memcmp(ctx->field_modulus[i], modulus, 32)) {
            *encoding = FRW_ENC_FIELD_BASE + i;
            return FRW_OK;
        }
    if (ctx->num_fields == FRW_MAX_FIELDS) {
        snprintf(g_last_error, sizeof g_last_error, "frw_ctx_field_encoding: the context already holds %d fields", FRW_MAX_FIELDS);
        return FRW_E_INVALID_ARG;
    }
    memcpy(ctx->field_modulus[ctx->num_fields], modulus, 32);
    ctx->fields[ctx->num_fields] = d.fc;
    *encoding = FRW_ENC_FIELD_BASE + ctx->num_fields++;
    return FRW_OK;
}

int frw_expand_field_dev(frw_ctx *ctx, int logn, size_t batch, const void *d_compact, int encoding, uint64_t *d_witness,
                         uint64_t *d_instance, void *stream)
{
    frw::KernelEnc ke;
    if (bad_field_common(ctx, logn, encoding, &ke) || !ke.fc) return FRW_E_INVALID_ARG;       // a registered field, nothing else
    if (batch == 0) return FRW_OK;
    if (!d_compact || !d_witness || !d_instance || ((uintptr_t)d_compact & 15)) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_expand(ctx->num_cu, logn, ke, batch, d_compact, d_witness, d_instance, (hipStream_t)stream));
    return FRW_OK;
}

int frw_expand_field_host(const uint64_t modulus[4], int logn, size_t batch, const void *compact, uint64_t *witness, uint64_t *instance)
{
    frw::FieldDerived d;
    if (!modulus || !frw::field_derive(modulus, &d)) return FRW_E_INVALID_ARG;
    if ((logn != 9 && logn != 10) || (batch && (!compact || !witness || !instance))) return FRW_E_INVALID_ARG;
    uint64_t one[4];
    limbs64(d.fc.one, one);
    const frw::FieldConsts &fc = d.fc;
    return expand_host_with(logn, batch, compact, witness, instance, one, [&fc](const uint64_t x[3], uint64_t out[4]) {
        const uint32_t x5[5] = {(uint32_t)x[0], (uint32_t)(x[0] >> 32), (uint32_t)x[1], (uint32_t)(x[1] >> 32), (uint32_t)x[2]};
        uint32_t e[8];
        if (!(x5[1] | x5[2] | x5[3] | x5[4])) frw::field_encode_u32(fc, x5[0], e);
        else frw::field_encode_u160(fc, x5, e);
        limbs64(e, out);
    });
}

int frw_diag_launch_shape(frw_ctx *ctx, int logn, int encoding, size_t batch, int32_t out[4])
{
    frw::KernelEnc ke;
    if (!out || bad_witness(ctx, FRW_CIRCUIT_NTT, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    int o[4];
    frw::launch_shape_witness_ntt_verify(ctx->num_cu, logn, ke, batch, o);
    for (int i = 0; i < 4; i++) out[i] = o[i];
    return FRW_OK;
}

int frw_layout_dual(int logn, frw_layout_dual_t *out)
{
    if (!out || (logn != 9 && logn != 10)) return FRW_E_INVALID_ARG;
    const int n = 1 << logn, nb = logn == 9 ? 50 : 52;
    const int len[FRW_NUM_SEGMENTS_DUAL] = {n, n, n, 2, n, n, n, 2, 29 * n, 29 * n, 29 * n, 29 * n, 60 * n, 4 * n, nb};
    return fill_layout(FRW_CIRCUIT_DUAL_NTT, logn, len, out);
}

int frw_layout_schoolbook(int logn, frw_layout_schoolbook_t *out)
{
    if (!out || (logn != 9 && logn != 10)) return FRW_E_INVALID_ARG;
    const int n = 1 << logn, nb = logn == 9 ? 50 : 52;
    const int len[FRW_NUM_SEGMENTS_SCHOOLBOOK] = {n, 28 * n, n * (n + 34), 36 * n, nb};
    out->column_len = n + 34;
    return fill_layout(FRW_CIRCUIT_SCHOOLBOOK, logn, len, out);
}

int frw_witness_schoolbook_verify_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk,
                                      const uint16_t *d_hm, int encoding, uint64_t *d_witness, uint64_t *d_instance,
                                      int32_t *d_status, void *stream)
{
    return witness_dev(ctx, FRW_CIRCUIT_SCHOOLBOOK, logn, batch, d_sig, d_pk, d_hm, encoding, d_witness, d_instance, d_status, stream);
}

int frw_witness_schoolbook_verify(frw_ctx *ctx, int logn, size_t batch, const uint16_t *sig, const uint16_t *pk,
                                  const uint16_t *hm, int encoding, uint64_t *witness, uint64_t *instance,
                                  int32_t *status, int strict)
{
    return witness_host(ctx, FRW_CIRCUIT_SCHOOLBOOK, logn, batch, sig, pk, hm, encoding, witness, instance, status, strict);
}

int frw_ntt_modq(frw_ctx *ctx, int logn, size_t batch, const uint16_t *poly, int encoding, uint64_t *witness,
                 uint16_t *ntt_out, int32_t *status)
{
    frw::KernelEnc ke;
    if (bad_field_common(ctx, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!poly || !witness || !ntt_out || !status) return FRW_E_INVALID_ARG;
    // as witness_host: one slot and one stream for a batch that fits a chunk, else two
    const size_t n = (size_t)1 << logn, wbytes = 29 * n * 32;
    const size_t chunk = std::min<size_t>(batch, 2048);
    frw::Carve c(nullptr);
    const size_t o_in = c.off;  c.take(chunk * n * 2);
    const size_t o_out = c.off; c.take(chunk * n * 2);
    const size_t o_wit = c.off; c.take(chunk * wbytes);
    const size_t o_st = c.off;  c.take(chunk * sizeof(int32_t));
    return frw::host_passes(
        ctx->arena, ctx->device, batch, chunk, batch > chunk ? 2 : 1, c.off, chunk * n * 2,
        {{witness, o_wit, wbytes}, {ntt_out, o_out, n * 2}, {status, o_st, sizeof(int32_t)}},
        [&](char *d, char *stage, size_t lo, size_t cnt, hipStream_t st) -> int {
            FRW_HIP(stage_rows({poly}, n, lo, cnt, stage, d + o_in, st));
            FRW_HIP(frw::launch_ntt_modq(ctx->d_tables, ctx->num_cu, logn, ke, cnt, (const uint16_t *)(d + o_in),
                                         (uint64_t *)(d + o_wit), (uint16_t *)(d + o_out), (int32_t *)(d + o_st), st));
            return FRW_OK;
        });
}

int frw_hash_to_point_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_nonces, const uint8_t *d_msgs,
                          const uint64_t *d_msg_off, uint16_t *d_hm, void *stream)
{
    if (bad_common(ctx, logn, FRW_ENC_CANONICAL)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_nonces || !d_msgs || !d_msg_off || !d_hm) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_hash_to_point(logn, batch, d_nonces, d_msgs, d_msg_off, d_hm, (hipStream_t)stream));
    return FRW_OK;
}

int frw_decode_public_keys_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_pk_bytes, uint16_t *d_pk,
                               int32_t *d_status, void *stream)
{
    if (bad_common(ctx, logn, FRW_ENC_CANONICAL)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_pk_bytes || !d_pk || !d_status) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_decode_public_keys(logn, batch, d_pk_bytes, d_pk, d_status, (hipStream_t)stream));
    return FRW_OK;
}

int frw_decode_signatures_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_sig_bytes, size_t sig_len,
                              uint16_t *d_sig, uint8_t *d_nonce_out, int32_t *d_status, void *stream)
{
    if (bad_common(ctx, logn, FRW_ENC_CANONICAL)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!d_sig_bytes || !d_sig || !d_status || sig_len <= 1 + FRW_NONCE_LEN) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_decode_signatures(logn, batch, d_sig_bytes, sig_len, d_sig, d_nonce_out, d_status, (hipStream_t)stream));
    return FRW_OK;
}

int frw_prepare_inputs(frw_ctx *ctx, int logn, size_t batch, const uint8_t *pk_bytes, const uint8_t *sig_bytes,
                       size_t sig_len, const uint8_t *msgs, const uint64_t *msg_off, uint16_t *sig, uint16_t *pk,
                       uint16_t *hm, int32_t *status)
{
    if (bad_common(ctx, logn, FRW_ENC_CANONICAL)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    if (!pk_bytes || !sig_bytes || !msg_off || !sig || !pk || !hm || !status || sig_len <= 1 + FRW_NONCE_LEN) return FRW_E_INVALID_ARG;
    if (!frw::message_offsets_ok(msgs, msg_off, batch)) return FRW_E_INVALID_ARG;
    frw::HostArena &A = ctx->arena;
    std::lock_guard<std::mutex> lock(A.mu);
    frw::DrainOnExit drain(A);
    FRW_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << logn;
    // one device slot, carved; the encoded inputs travel in ONE copy through the page-locked buffer (one pass of the whole batch), the
    // results and both status vectors come back in ONE copy
    const frw::StagedInputs in(logn, batch, batch, pk_bytes, sig_bytes, sig_len, msgs, msg_off);
    frw::Carve os(nullptr);                                             // layout of the results
    const size_t o_sig = os.off; os.take(batch * n * 2);
    const size_t o_pk = os.off; os.take(batch * n * 2);
    const size_t o_hm = os.off; os.take(batch * n * 2);
    const size_t o_st1 = os.off; os.take(batch * sizeof(int32_t));
    const size_t o_st2 = os.off; os.take(batch * sizeof(int32_t));
    const size_t out_total = os.off;
    const size_t nonce_bytes = (batch * FRW_NONCE_LEN + 255) & ~(size_t)255;
    FRW_HIP(A.reserve_device(0, in.bytes + out_total + nonce_bytes));
    FRW_HIP(A.reserve_pinned(std::max(in.bytes, out_total)));
    char *d_in = (char *)A.d_slot[0], *d_out = d_in + in.bytes, *d_nonce = d_out + out_total, *h = (char *)A.h_pin;
    in.fill(h, 0, batch);
    hipStream_t st = A.compute;
    FRW_HIP(hipMemcpyAsync(d_in, h, in.bytes, hipMemcpyHostToDevice, st));
    FRW_HIP(hipMemsetAsync(d_nonce, 0, batch * FRW_NONCE_LEN, st));
    FRW_HIP(frw::launch_decode_public_keys(logn, batch, in.d_pk(d_in), (uint16_t *)(d_out + o_pk), (int32_t *)(d_out + o_st1), st));
    FRW_HIP(frw::launch_decode_signatures(logn, batch, in.d_second(d_in), sig_len, (uint16_t *)(d_out + o_sig), (uint8_t *)d_nonce,
                                          (int32_t *)(d_out + o_st2), st));
    FRW_HIP(frw::launch_hash_to_point(logn, batch, (const uint8_t *)d_nonce, in.d_msgs(d_in), in.d_off(d_in), (uint16_t *)(d_out + o_hm), st));
    FRW_HIP(hipStreamSynchronize(st));                                   // the staged inputs have been read
    FRW_HIP(hipMemcpyAsync(h, d_out, out_total, hipMemcpyDeviceToHost, st));
    FRW_HIP(hipStreamSynchronize(st));
    drain.settled = true;
    memcpy(sig, h + o_sig, batch * n * 2);
    memcpy(pk, h + o_pk, batch * n * 2);
    memcpy(hm, h + o_hm, batch * n * 2);
    const int32_t *st1 = (const int32_t *)(h + o_st1), *st2 = (const int32_t *)(h + o_st2);
    for (size_t i = 0; i < batch; i++) status[i] = st2[i] != FRW_ST_OK ? st2[i] : st1[i];
    return FRW_OK;
}

// ---- the verifier's statement: instance_assignment from (pk, hm), or from the key's and the message's bytes; no signature -------------
namespace {
// (a registered field is accepted for every circuit: the instance values are below q in all three)
bool bad_statement(const frw_ctx *ctx, int circuit, int logn, int encoding, frw::KernelEnc *ke)
{
    return bad_field_common(ctx, logn, encoding, ke) || !frw::known_circuit(circuit);
}
// the schoolbook circuit's public inputs are the coefficients themselves (falcon_schoolbook.rs:66-83), the NTT circuits' their transforms
int statement_form(int circuit) { return circuit == FRW_CIRCUIT_SCHOOLBOOK ? 1 : 0; }
constexpr size_t STATEMENT_CHUNK = 4096;          // statements of one pass of the host-buffer forms: 270 MB of Falcon-1024 instance vectors
}  // namespace

int frw_statement_dev(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint16_t *d_pk, const uint16_t *d_hm, int encoding,
                      uint64_t *d_instance, int32_t *d_status, void *stream)
{
    frw::KernelEnc ke;
    if (bad_statement(ctx, circuit, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    if (!d_pk || !d_hm || !d_instance || !d_status) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_statement(ctx->d_tables, ctx->num_cu, logn, statement_form(circuit), ke, batch, d_pk, d_hm,
                                  d_instance, nullptr, 1, nullptr, d_status, nullptr, (hipStream_t)stream));
    return FRW_OK;
}

size_t frw_statement_workspace_bytes(int logn, size_t batch)
{
    if (logn != 9 && logn != 10) return 0;
    return frw::statement_layout(nullptr, logn, batch).bytes;
}

int frw_statement_from_bytes_dev(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint8_t *d_pk_bytes, const uint8_t *d_nonces,
                                 const uint8_t *d_msgs, const uint64_t *d_msg_off, int encoding, uint64_t *d_instance, int32_t *d_status,
                                 void *d_workspace, size_t workspace_bytes, void *stream)
{
    frw::KernelEnc ke;
    if (bad_statement(ctx, circuit, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    if (!d_pk_bytes || !d_nonces || !d_msgs || !d_msg_off || !d_instance || !d_status || !d_workspace) return FRW_E_INVALID_ARG;
    if (((uintptr_t)d_workspace & 15) || workspace_bytes < frw_statement_workspace_bytes(logn, batch)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    const frw::StatementBufs ws = frw::statement_layout(d_workspace, logn, batch);
    hipStream_t st = (hipStream_t)stream;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_decode_public_keys(logn, batch, d_pk_bytes, ws.pk, ws.decode_status, st));
    FRW_HIP(frw::launch_hash_to_point(logn, batch, d_nonces, d_msgs, d_msg_off, ws.hm, st));
    FRW_HIP(frw::launch_statement(ctx->d_tables, ctx->num_cu, logn, statement_form(circuit), ke, batch, ws.pk, ws.hm,
                                  d_instance, nullptr, 1, ws.decode_status, d_status, nullptr, st));
    return FRW_OK;
}

int frw_statement(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint16_t *pk, const uint16_t *hm, int encoding,
                  uint64_t *instance, int32_t *status, int strict)
{
    frw::KernelEnc ke;
    if (bad_statement(ctx, circuit, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    if (!pk || !hm || !instance || !status) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    const size_t n = (size_t)1 << logn, ibytes = frw::circuit_shape(circuit, logn).num_instance * 32, chunk = std::min(batch, STATEMENT_CHUNK);
    frw::Carve c(nullptr);
    const size_t o_in = c.off;   c.take(2 * chunk * n * 2);
    const size_t o_inst = c.off; c.take(chunk * ibytes);
    const size_t o_st = c.off;   c.take(chunk * sizeof(int32_t));
    const int rc = frw::host_passes(
        ctx->arena, ctx->device, batch, chunk, 1, c.off, 2 * chunk * n * 2, {{instance, o_inst, ibytes}, {status, o_st, sizeof(int32_t)}},
        [&](char *d, char *stage, size_t lo, size_t cnt, hipStream_t st) -> int {
            const uint16_t *d_in = (const uint16_t *)(d + o_in);
            FRW_HIP(stage_rows({pk, hm}, n, lo, cnt, stage, d + o_in, st));
            FRW_HIP(frw::launch_statement(ctx->d_tables, ctx->num_cu, logn, statement_form(circuit), ke, cnt, d_in,
                                          d_in + cnt * n, (uint64_t *)(d + o_inst), nullptr, 1, nullptr, (int32_t *)(d + o_st), nullptr, st));
            return FRW_OK;
        });
    return strict_verdict(rc, strict, status, batch);
}

int frw_statement_from_bytes(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint8_t *pk_bytes, const uint8_t *nonces,
                             const uint8_t *msgs, const uint64_t *msg_off, int encoding, uint64_t *instance, int32_t *status, int strict)
{
    frw::KernelEnc ke;
    if (bad_statement(ctx, circuit, logn, encoding, &ke)) return FRW_E_INVALID_ARG;
    if (!pk_bytes || !nonces || !msg_off || !instance || !status) return FRW_E_INVALID_ARG;
    if (!frw::message_offsets_ok(msgs, msg_off, batch)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    const size_t ibytes = frw::circuit_shape(circuit, logn).num_instance * 32, chunk = std::min(batch, STATEMENT_CHUNK);
    const frw::StagedInputs in(logn, batch, chunk, pk_bytes, nonces, FRW_NONCE_LEN, msgs, msg_off);
    frw::Carve c(nullptr);
    c.take(in.bytes);
    const size_t o_ws = c.off;   c.take(frw_statement_workspace_bytes(logn, chunk));
    const size_t o_inst = c.off; c.take(chunk * ibytes);
    const size_t o_st = c.off;   c.take(chunk * sizeof(int32_t));
    const int rc = frw::host_passes(
        ctx->arena, ctx->device, batch, chunk, 1, c.off, in.bytes, {{instance, o_inst, ibytes}, {status, o_st, sizeof(int32_t)}},
        [&](char *d, char *stage, size_t lo, size_t cnt, hipStream_t st) -> int {
            in.fill(stage, lo, cnt);
            FRW_HIP(hipMemcpyAsync(d, stage, in.bytes, hipMemcpyHostToDevice, st));
            const frw::StatementBufs ws = frw::statement_layout(d + o_ws, logn, cnt);
            FRW_HIP(frw::launch_decode_public_keys(logn, cnt, in.d_pk(d), ws.pk, ws.decode_status, st));
            FRW_HIP(frw::launch_hash_to_point(logn, cnt, in.d_second(d), in.d_msgs(d), in.d_off(d), ws.hm, st));
            FRW_HIP(frw::launch_statement(ctx->d_tables, ctx->num_cu, logn, statement_form(circuit), ke, cnt, ws.pk, ws.hm,
                                          (uint64_t *)(d + o_inst), nullptr, 1, ws.decode_status, (int32_t *)(d + o_st), nullptr, st));
            return FRW_OK;
        });
    return strict_verdict(rc, strict, status, batch);
}

int frw_aggregate_statement_dev(const frw_r1cs *aggregate, frw_ctx *ctx, const uint16_t *d_pk_512, const uint16_t *d_hm_512,
                                const uint16_t *d_pk_1024, const uint16_t *d_hm_1024, int encoding, uint64_t *d_instance,
                                int32_t *d_status, void *stream)
{
    int device = -1;
    const frw::R1csAgg *agg = frw::r1cs_aggregate(aggregate, &device);
    if (!agg || bad_common(ctx, 10, encoding) || !d_instance || !d_status || device != ctx->device) return FRW_E_INVALID_ARG;
    const uint16_t *pk[2] = {d_pk_512, d_pk_1024}, *hm[2] = {d_hm_512, d_hm_1024};
    for (int g = 0; g < 2; g++)
        if (agg->set[g].count && (!pk[g] || !hm[g])) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    bool first = true;                  // one launch per parameter set; the first one writes the aggregate's constant
    for (int g = 0; g < 2; g++) {
        const frw::R1csAggSet &set = agg->set[g];
        if (!set.count) continue;
        FRW_HIP(frw::launch_statement(ctx->d_tables, ctx->num_cu, 9 + g, 0, encoding, set.count, pk[g], hm[g], d_instance, set.offs,
                                      first ? 2 : 0, nullptr, d_status, set.stmt, (hipStream_t)stream));
        first = false;
    }
    return FRW_OK;
}

// ---- Falcon verification: the verdict (and the norm) of (sig, pk, hm), or of the encoded key, signature and message; no witness -------
namespace {
bool bad_falcon_verify(const frw_ctx *ctx, int logn, int rule)
{
    return !ctx || (logn != 9 && logn != 10) || (rule != FRW_RULE_CIRCUIT && rule != FRW_RULE_SPEC);
}
constexpr size_t FALCON_VERIFY_CHUNK = 16384;     // signatures of one pass of the host-buffer forms: 100 MB of Falcon-1024 coefficients
}  // namespace

int frw_falcon_verify_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk, const uint16_t *d_hm,
                          int rule, int32_t *d_status, uint64_t *d_norm, void *stream)
{
    if (bad_falcon_verify(ctx, logn, rule)) return FRW_E_INVALID_ARG;
    if (!d_sig || !d_pk || !d_hm || !d_status) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_falcon_verify(ctx->d_tables, ctx->num_cu, logn, rule, batch, d_sig, d_pk, d_hm, nullptr, nullptr, d_status,
                                      d_norm, (hipStream_t)stream));
    return FRW_OK;
}

size_t frw_falcon_verify_workspace_bytes(int logn, size_t batch)
{
    if (logn != 9 && logn != 10) return 0;
    return frw::falcon_verify_layout(nullptr, logn, batch).bytes;
}

namespace {
// the four kernels of the bytes path on `st`: both decoders and SHAKE256 into the workspace, then the verdicts.  A signature a decoder
// refused leaves its nonce and part of its coefficients as the workspace held them: the hash reads 40 bytes that are the workspace's
// whatever they hold, and the kernel reads the decoders' statuses first and no coefficient of such a signature.
hipError_t falcon_verify_chain(const frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_pk_bytes, const uint8_t *d_sig_bytes,
                               size_t sig_len, const uint8_t *d_msgs, const uint64_t *d_msg_off, int rule, int32_t *d_status,
                               uint64_t *d_norm, void *d_workspace, hipStream_t st)
{
    const frw::FalconVerifyBufs ws = frw::falcon_verify_layout(d_workspace, logn, batch);
    hipError_t e = frw::launch_decode_public_keys(logn, batch, d_pk_bytes, ws.pk, ws.pk_status, st);
    if (e == hipSuccess) e = frw::launch_decode_signatures(logn, batch, d_sig_bytes, sig_len, ws.sig, ws.nonce, ws.sig_status, st);
    if (e == hipSuccess) e = frw::launch_hash_to_point(logn, batch, ws.nonce, d_msgs, d_msg_off, ws.hm, st);
    if (e == hipSuccess)
        e = frw::launch_falcon_verify(ctx->d_tables, ctx->num_cu, logn, rule, batch, ws.sig, ws.pk, ws.hm, ws.sig_status, ws.pk_status,
                                      d_status, d_norm, st);
    return e;
}
}  // namespace

int frw_falcon_verify_from_bytes_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_pk_bytes, const uint8_t *d_sig_bytes,
                                     size_t sig_len, const uint8_t *d_msgs, const uint64_t *d_msg_off, int rule, int32_t *d_status,
                                     uint64_t *d_norm, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (bad_falcon_verify(ctx, logn, rule)) return FRW_E_INVALID_ARG;
    if (!d_pk_bytes || !d_sig_bytes || !d_msgs || !d_msg_off || !d_status || !d_workspace) return FRW_E_INVALID_ARG;
    if (sig_len <= 1 + FRW_NONCE_LEN) return FRW_E_INVALID_ARG;
    if (((uintptr_t)d_workspace & 15) || workspace_bytes < frw_falcon_verify_workspace_bytes(logn, batch)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(falcon_verify_chain(ctx, logn, batch, d_pk_bytes, d_sig_bytes, sig_len, d_msgs, d_msg_off, rule, d_status, d_norm,
                                d_workspace, (hipStream_t)stream));
    return FRW_OK;
}

int frw_falcon_verify(frw_ctx *ctx, int logn, size_t batch, const uint16_t *sig, const uint16_t *pk, const uint16_t *hm, int rule,
                      int32_t *status, uint64_t *norm, int strict)
{
    if (bad_falcon_verify(ctx, logn, rule)) return FRW_E_INVALID_ARG;
    if (!sig || !pk || !hm || !status) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    const size_t n = (size_t)1 << logn, chunk = std::min(batch, FALCON_VERIFY_CHUNK);
    frw::Carve c(nullptr);
    const size_t o_in = c.off;   c.take(3 * chunk * n * 2);
    const size_t o_norm = c.off; c.take(chunk * sizeof(uint64_t));
    const size_t o_st = c.off;   c.take(chunk * sizeof(int32_t));
    const int rc = frw::host_passes(
        ctx->arena, ctx->device, batch, chunk, 1, c.off, 3 * chunk * n * 2, {{status, o_st, sizeof(int32_t)}, {norm, o_norm, sizeof(uint64_t)}},
        [&](char *d, char *stage, size_t lo, size_t cnt, hipStream_t st) -> int {
            const uint16_t *d_in = (const uint16_t *)(d + o_in);
            FRW_HIP(stage_rows({sig, pk, hm}, n, lo, cnt, stage, d + o_in, st));
            FRW_HIP(frw::launch_falcon_verify(ctx->d_tables, ctx->num_cu, logn, rule, cnt, d_in, d_in + cnt * n, d_in + 2 * cnt * n, nullptr,
                                              nullptr, (int32_t *)(d + o_st), (uint64_t *)(d + o_norm), st));
            return FRW_OK;
        });
    return strict_verdict(rc, strict, status, batch);
}

int frw_falcon_verify_from_bytes(frw_ctx *ctx, int logn, size_t batch, const uint8_t *pk_bytes, const uint8_t *sig_bytes, size_t sig_len,
                                 const uint8_t *msgs, const uint64_t *msg_off, int rule, int32_t *status, uint64_t *norm, int strict)
{
    if (bad_falcon_verify(ctx, logn, rule)) return FRW_E_INVALID_ARG;
    if (!pk_bytes || !sig_bytes || !msgs || !msg_off || !status || sig_len <= 1 + FRW_NONCE_LEN) return FRW_E_INVALID_ARG;
    if (!frw::message_offsets_ok(msgs, msg_off, batch)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    const size_t chunk = std::min(batch, FALCON_VERIFY_CHUNK);
    const frw::StagedInputs in(logn, batch, chunk, pk_bytes, sig_bytes, sig_len, msgs, msg_off);
    frw::Carve c(nullptr);
    c.take(in.bytes);
    const size_t o_ws = c.off;   c.take(frw_falcon_verify_workspace_bytes(logn, chunk));
    const size_t o_norm = c.off; c.take(chunk * sizeof(uint64_t));
    const size_t o_st = c.off;   c.take(chunk * sizeof(int32_t));
    const int rc = frw::host_passes(
        ctx->arena, ctx->device, batch, chunk, 1, c.off, in.bytes, {{status, o_st, sizeof(int32_t)}, {norm, o_norm, sizeof(uint64_t)}},
        [&](char *d, char *stage, size_t lo, size_t cnt, hipStream_t st) -> int {
            in.fill(stage, lo, cnt);
            FRW_HIP(hipMemcpyAsync(d, stage, in.bytes, hipMemcpyHostToDevice, st));
            FRW_HIP(falcon_verify_chain(ctx, logn, cnt, in.d_pk(d), in.d_second(d), sig_len, in.d_msgs(d), in.d_off(d), rule,
                                        (int32_t *)(d + o_st), (uint64_t *)(d + o_norm), d + o_ws, st));
            return FRW_OK;
        });
    return strict_verdict(rc, strict, status, batch);
}

// ---- the prover from bytes: (pk bytes, msg, sig bytes) -> Groth16 proofs on the wire, one call ----------------------------------------
namespace {
// what the arguments say about the circuit, before any handle is looked at
bool bad_pok_prove(const frw_ctx *ctx, int circuit, int logn, int wire_mode, size_t sig_len)
{
    return !ctx || (logn != 9 && logn != 10) || !frw::known_circuit(circuit) || frw_groth16_proof_wire_bytes(wire_mode) == 0 ||
           sig_len <= 1 + FRW_NONCE_LEN;
}
// ... and whether the handles are that circuit's: a per-signature system with its I, W, C, and a whole key over it.  W in *num_witness.
bool pok_prove_shape(const frw_groth16_pk *pk, const frw_r1cs *r, int circuit, int logn, size_t *num_witness)
{
    if (!pk || !r || (logn != 9 && logn != 10) || !frw::known_circuit(circuit)) return false;
    const frw::CircuitShape s = frw::circuit_shape(circuit, logn);
    frw_r1cs_info_t info;
    frw_groth16_pk_info_t ki;
    if (frw_r1cs_info(r, &info) != FRW_OK || frw_groth16_pk_info(pk, &ki) != FRW_OK) return false;
    // the handle frw_r1cs_load made for this circuit: a system that came in as matrices is not it, whatever its counts (the export loaded
    // back has Falcon's) -- the witness kernels behind these calls know the Falcon circuits only
    if (!frw::r1cs_is_circuit(r, circuit, logn)) return false;
    if (info.num_statements != 1 || info.num_instance != s.num_instance || info.num_witness != s.num_witness ||
        info.num_constraints != s.num_constraints)
        return false;
    if (ki.world > 1) return false;                                       // a slice of a key proves nothing by itself
    int device = -1;
    uint64_t ni = 0, nw = 0, dom = 0;
    frw::groth16_pk_counts(pk, &device, &ni, &nw, &dom);
    if (ni != info.num_instance || nw != s.num_witness || device != frw::r1cs_device(r)) return false;
    *num_witness = s.num_witness;
    return true;
}
constexpr size_t POK_PROVE_MAX_IN_FLIGHT = 4096;  // (the prover's own bound on a chunk)
constexpr size_t POK_PROVE_CHUNK = 256;           // slots of one pass of the host-buffer form ...
constexpr size_t POK_PROVE_HOST_IN_FLIGHT = 8;    // ... and the proofs in flight its share of the arena is sized for
}  // namespace

size_t frw_pok_prove_workspace_bytes(const frw_groth16_pk *pk, const frw_r1cs *r, int circuit, int logn, size_t batch, size_t in_flight)
{
    size_t W = 0;
    if (in_flight == 0 || !pok_prove_shape(pk, r, circuit, logn, &W)) return 0;
    const size_t g = frw_groth16_workspace_bytes(pk, r, in_flight);
    return g ? frw::pok_prove_layout(nullptr, logn, batch, in_flight, W, g).bytes : 0;
}

int frw_pok_prove_from_bytes_dev(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *r, int circuit, int logn, size_t batch,
                                 const uint8_t *d_pk_bytes, const uint8_t *d_sig_bytes, size_t sig_len, const uint8_t *d_msgs,
                                 const uint64_t *d_msg_off, const uint64_t *d_rs, int wire_mode, uint8_t *d_wire, uint64_t *d_proofs,
                                 uint64_t *d_instance, int32_t *d_status, uint32_t *d_num_unsatisfied, void *d_workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (bad_pok_prove(ctx, circuit, logn, wire_mode, sig_len)) return FRW_E_INVALID_ARG;
    if (!pk || !r || !d_pk_bytes || !d_sig_bytes || !d_msgs || !d_msg_off || !d_rs || !d_wire || !d_status || !d_workspace)
        return FRW_E_INVALID_ARG;
    if ((uintptr_t)d_workspace & 255) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    size_t W = 0;
    if (!pok_prove_shape(pk, r, circuit, logn, &W) || frw::r1cs_device(r) != ctx->device) return FRW_E_INVALID_ARG;
    const auto size = [&](size_t k) { return frw::pok_prove_layout(nullptr, logn, batch, k, W, frw_groth16_workspace_bytes(pk, r, k)).bytes; };
    if (frw_groth16_workspace_bytes(pk, r, 1) == 0) return FRW_E_INVALID_ARG;
    const size_t k = frw::proofs_in_flight(std::min(batch, POK_PROVE_MAX_IN_FLIGHT), workspace_bytes, size);
    if (k == 0) return FRW_E_INVALID_ARG;
    const frw::PokProveBufs ws = frw::pok_prove_layout(d_workspace, logn, batch, k, W, frw_groth16_workspace_bytes(pk, r, k));
    const int wire_len = (int)frw_groth16_proof_wire_bytes(wire_mode), inst_words = (int)(((size_t)2 << logn) + 1) * 4;
    hipStream_t st = (hipStream_t)stream;
    FRW_HIP(hipSetDevice(ctx->device));
    // decode, hash and screen: d_status is frw_falcon_verify_from_bytes_dev's, word for word
    FRW_HIP(falcon_verify_chain(ctx, logn, batch, d_pk_bytes, d_sig_bytes, sig_len, d_msgs, d_msg_off, FRW_RULE_CIRCUIT, d_status, nullptr,
                                ws.screen.sig, st));
    // the accepted slots, in slot order, and how many they are -- the one value the host needs (chunks are host loops): one wait
    FRW_HIP(frw::launch_pok_scan(batch, d_status, ws.block_sums, ws.index, ws.count, st));
    FRW_HIP(frw::launch_pok_zero_refused(batch, d_status, wire_len, inst_words, d_wire, d_proofs, d_instance, d_num_unsatisfied, st));
    uint32_t count = 0;
    FRW_HIP(hipMemcpyAsync(&count, ws.count, sizeof count, hipMemcpyDeviceToHost, st));
    FRW_HIP(hipStreamSynchronize(st));
    if (count > batch) return FRW_E_HIP;                                  // (cannot happen: the index list has `batch` entries)
    FRW_HIP(frw::launch_pok_gather_rs(count, ws.index, d_rs, ws.rs, st));
    for (size_t lo = 0; lo < count; lo += k) {
        const size_t cnt = std::min<size_t>(k, count - lo);
        const uint32_t *index = ws.index + lo;
        FRW_HIP(frw::launch_pok_gather_inputs(logn, cnt, index, ws.screen.sig, ws.screen.pk, ws.screen.hm, ws.sig, ws.pk, ws.hm, st));
        FRW_HIP(launch_witness(ctx, circuit, logn, FRW_ENC_MONTGOMERY, cnt, ws.sig, ws.pk, ws.hm, ws.witness, ws.instance, ws.witness_status, st));
        int rc = frw_groth16_prove_rs_dev(pk, r, cnt, ws.witness, ws.instance, ws.rs + lo * 8, ws.proofs, ws.unsatisfied, ws.groth16_ws,
                                          ws.groth16_bytes, st);
        if (rc == FRW_OK) rc = frw_groth16_proofs_to_wire_dev(ctx->device, cnt, ws.proofs, wire_mode, ws.wire, ws.wire_status, st);
        if (rc != FRW_OK) return rc;
        FRW_HIP(frw::launch_pok_scatter(cnt, index, wire_len, inst_words, ws.wire, ws.proofs, ws.instance, ws.unsatisfied, d_wire, d_proofs,
                                        d_instance, d_num_unsatisfied, st));
    }
    return FRW_OK;
}

int frw_pok_prove_from_bytes(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *r, int circuit, int logn, size_t batch,
                             const uint8_t *pk_bytes, const uint8_t *sig_bytes, size_t sig_len, const uint8_t *msgs,
                             const uint64_t *msg_off, const uint64_t *rs, int wire_mode, uint8_t *wire, uint64_t *proofs,
                             uint64_t *instance, int32_t *status, uint32_t *num_unsatisfied, int strict)
{
    if (bad_pok_prove(ctx, circuit, logn, wire_mode, sig_len)) return FRW_E_INVALID_ARG;
    if (!pk || !r || !pk_bytes || !sig_bytes || !msgs || !msg_off || !rs || !wire || !status) return FRW_E_INVALID_ARG;
    if (!frw::message_offsets_ok(msgs, msg_off, batch)) return FRW_E_INVALID_ARG;
    if (batch == 0) return FRW_OK;
    size_t W = 0;
    if (!pok_prove_shape(pk, r, circuit, logn, &W) || frw::r1cs_device(r) != ctx->device) return FRW_E_INVALID_ARG;
    const size_t chunk = std::min(batch, POK_PROVE_CHUNK), ibytes = frw::circuit_shape(circuit, logn).num_instance * 32;
    const size_t wire_len = frw_groth16_proof_wire_bytes(wire_mode);
    const frw::StagedInputs in(logn, batch, chunk, pk_bytes, sig_bytes, sig_len, msgs, msg_off, rs);
    const size_t ws_bytes = frw_pok_prove_workspace_bytes(pk, r, circuit, logn, chunk, std::min(chunk, POK_PROVE_HOST_IN_FLIGHT));
    if (ws_bytes == 0) return FRW_E_INVALID_ARG;
    frw::Carve c(nullptr);
    c.take(in.bytes);
    const size_t o_ws = c.off;   c.take(ws_bytes);
    const size_t o_wire = c.off; c.take(chunk * wire_len);
    const size_t o_prf = c.off;  c.take(chunk * 384);
    const size_t o_inst = c.off; c.take(instance ? chunk * ibytes : 0);
    const size_t o_st = c.off;   c.take(chunk * sizeof(int32_t));
    const size_t o_uns = c.off;  c.take(chunk * sizeof(uint32_t));
    const int rc = frw::host_passes(
        ctx->arena, ctx->device, batch, chunk, 1, c.off, in.bytes,
        {{wire, o_wire, wire_len}, {proofs, o_prf, 384}, {instance, o_inst, ibytes}, {status, o_st, sizeof(int32_t)},
         {num_unsatisfied, o_uns, sizeof(uint32_t)}},
        [&](char *d, char *stage, size_t lo, size_t cnt, hipStream_t st) -> int {
            in.fill(stage, lo, cnt);
            FRW_HIP(hipMemcpyAsync(d, stage, in.bytes, hipMemcpyHostToDevice, st));
            return frw_pok_prove_from_bytes_dev(ctx, pk, r, circuit, logn, cnt, in.d_pk(d), in.d_second(d), sig_len, in.d_msgs(d), in.d_off(d),
                                                in.d_rs(d), wire_mode, (uint8_t *)(d + o_wire), proofs ? (uint64_t *)(d + o_prf) : nullptr,
                                                instance ? (uint64_t *)(d + o_inst) : nullptr, (int32_t *)(d + o_st),
                                                num_unsatisfied ? (uint32_t *)(d + o_uns) : nullptr, d + o_ws, ws_bytes, st);
        });
    return strict_verdict(rc, strict, status, batch);
}

// ---- an aggregate from bytes: the encoded (pk, msg, sig) of its statements, in statement order -> verdicts, the verifier's statement,
// ONE proof on the wire ---------------------------------------------------------------------------------------------------------------
namespace {
// an aggregate handle on the context's device, and how many statements of each parameter set it has; null: not one
const frw::R1csAgg *aggregate_on(const frw_r1cs *aggregate, const frw_ctx *ctx, size_t count[2])
{
    int device = -1;
    const frw::R1csAgg *agg = frw::r1cs_aggregate(aggregate, &device);
    if (!agg || (ctx && device != ctx->device)) return nullptr;
    count[0] = agg->set[0].count;
    count[1] = agg->set[1].count;
    return agg;
}
// the routed decoders and SHAKE256 into the per-set arrays of `ws`, one launch per parameter set and stage, then each set's verification
// kernel; the verdicts (and norms) go back into statement order, and the number of refused statements into ws.refused
hipError_t aggregate_screen_chain(const frw_ctx *ctx, const frw::R1csAgg *agg, const uint8_t *d_pk_bytes, const uint8_t *d_sig_bytes,
                                  const uint8_t *d_msgs, const uint64_t *d_msg_off, int rule, int32_t *d_status, uint64_t *d_norm,
                                  const frw::AggregateScreenBufs &ws, hipStream_t st)
{
    hipError_t e = hipSuccess;
    for (int g = 0; g < 2 && e == hipSuccess; g++) {
        const frw::R1csAggSet &set = agg->set[g];
        if (!set.count) continue;
        e = frw::launch_agg_decode_public_keys(9 + g, set.count, set.stmt, d_pk_bytes, ws.pk[g], ws.pk_status[g], st);
        if (e == hipSuccess) e = frw::launch_agg_decode_signatures(9 + g, set.count, set.stmt, d_sig_bytes, ws.sig[g], ws.nonce, ws.sig_status[g], st);
        if (e == hipSuccess) e = frw::launch_agg_hash_to_point(9 + g, set.count, set.stmt, ws.nonce, d_msgs, d_msg_off, ws.hm[g], st);
        if (e == hipSuccess)
            e = frw::launch_falcon_verify(ctx->d_tables, ctx->num_cu, 9 + g, rule, set.count, ws.sig[g], ws.pk[g], ws.hm[g], ws.sig_status[g],
                                          ws.pk_status[g], ws.status[g], ws.norm[g], st);
    }
    if (e != hipSuccess) return e;
    const uint32_t *stmt[2] = {agg->set[0].stmt, agg->set[1].stmt};
    const size_t count[2] = {agg->set[0].count, agg->set[1].count};
    return frw::launch_agg_verdicts(stmt, ws.status, ws.norm, count, d_status, d_norm, ws.refused, st);
}
// frw_aggregate_statement_dev's launches on decoded keys and hashed messages that are in `ws` already, the key decoder's verdicts first
hipError_t aggregate_statement_launches(const frw_ctx *ctx, const frw::R1csAgg *agg, int encoding, uint64_t *d_instance, int32_t *d_status,
                                        const frw::AggregateScreenBufs &ws, hipStream_t st)
{
    hipError_t e = hipSuccess;
    bool first = true;
    for (int g = 0; g < 2 && e == hipSuccess; g++) {
        const frw::R1csAggSet &set = agg->set[g];
        if (!set.count) continue;
        e = frw::launch_statement(ctx->d_tables, ctx->num_cu, 9 + g, 0, encoding, set.count, ws.pk[g], ws.hm[g], d_instance, set.offs,
                                  first ? 2 : 0, ws.pk_status[g], d_status, set.stmt, st);
        first = false;
    }
    return e;
}
// whether `pk` is a whole key with the aggregate's instance and witness counts, on its device
bool aggregate_key_fits(const frw_groth16_pk *pk, const frw_r1cs *aggregate)
{
    frw_r1cs_info_t info;
    frw_groth16_pk_info_t ki;
    if (!pk || frw_r1cs_info(aggregate, &info) != FRW_OK || frw_groth16_pk_info(pk, &ki) != FRW_OK || ki.world > 1) return false;
    int device = -1;
    uint64_t ni = 0, nw = 0, dom = 0;
    frw::groth16_pk_counts(pk, &device, &ni, &nw, &dom);
    return ni == info.num_instance && nw == info.num_witness && device == frw::r1cs_device(aggregate);
}
}  // namespace

size_t frw_aggregate_screen_workspace_bytes(const frw_r1cs *aggregate)
{
    size_t count[2];
    return aggregate_on(aggregate, nullptr, count) ? frw::aggregate_screen_layout(nullptr, count[0], count[1]).bytes : 0;
}

int frw_aggregate_falcon_verify_from_bytes_dev(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *d_pk_bytes, const uint8_t *d_sig_bytes,
                                               const uint8_t *d_msgs, const uint64_t *d_msg_off, int rule, int32_t *d_status, uint64_t *d_norm,
                                               void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!ctx || (rule != FRW_RULE_CIRCUIT && rule != FRW_RULE_SPEC)) return FRW_E_INVALID_ARG;
    if (!aggregate || !d_pk_bytes || !d_sig_bytes || !d_msgs || !d_msg_off || !d_status || !d_workspace) return FRW_E_INVALID_ARG;
    if ((uintptr_t)d_workspace & 15) return FRW_E_INVALID_ARG;
    size_t count[2];
    const frw::R1csAgg *agg = aggregate_on(aggregate, ctx, count);
    if (!agg || workspace_bytes < frw::aggregate_screen_layout(nullptr, count[0], count[1]).bytes) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(aggregate_screen_chain(ctx, agg, d_pk_bytes, d_sig_bytes, d_msgs, d_msg_off, rule, d_status, d_norm,
                                   frw::aggregate_screen_layout(d_workspace, count[0], count[1]), (hipStream_t)stream));
    return FRW_OK;
}

int frw_aggregate_statement_from_bytes_dev(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *d_pk_bytes, const uint8_t *d_nonces,
                                           const uint8_t *d_msgs, const uint64_t *d_msg_off, int encoding, uint64_t *d_instance,
                                           int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (bad_common(ctx, 10, encoding)) return FRW_E_INVALID_ARG;
    if (!aggregate || !d_pk_bytes || !d_nonces || !d_msgs || !d_msg_off || !d_instance || !d_status || !d_workspace) return FRW_E_INVALID_ARG;
    if ((uintptr_t)d_workspace & 15) return FRW_E_INVALID_ARG;
    size_t count[2];
    const frw::R1csAgg *agg = aggregate_on(aggregate, ctx, count);
    if (!agg || workspace_bytes < frw::aggregate_screen_layout(nullptr, count[0], count[1]).bytes) return FRW_E_INVALID_ARG;
    const frw::AggregateScreenBufs ws = frw::aggregate_screen_layout(d_workspace, count[0], count[1]);
    hipStream_t st = (hipStream_t)stream;
    FRW_HIP(hipSetDevice(ctx->device));
    for (int g = 0; g < 2; g++) {
        const frw::R1csAggSet &set = agg->set[g];
        FRW_HIP(frw::launch_agg_decode_public_keys(9 + g, set.count, set.stmt, d_pk_bytes, ws.pk[g], ws.pk_status[g], st));
        FRW_HIP(frw::launch_agg_hash_to_point(9 + g, set.count, set.stmt, d_nonces, d_msgs, d_msg_off, ws.hm[g], st));
    }
    FRW_HIP(aggregate_statement_launches(ctx, agg, encoding, d_instance, d_status, ws, st));
    return FRW_OK;
}

size_t frw_aggregate_prove_workspace_bytes(const frw_groth16_pk *pk, const frw_r1cs *aggregate)
{
    size_t count[2];
    if (!pk || !aggregate_on(aggregate, nullptr, count) || !aggregate_key_fits(pk, aggregate)) return 0;
    const size_t g = frw_groth16_workspace_bytes(pk, aggregate, 1);
    return g ? frw::aggregate_prove_layout(nullptr, count[0], count[1], g).bytes : 0;
}

int frw_aggregate_prove_from_bytes_dev(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *aggregate, const uint8_t *d_pk_bytes,
                                       const uint8_t *d_sig_bytes, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint64_t *d_rs,
                                       int wire_mode, uint8_t *d_wire, uint64_t *d_proof, uint64_t *d_instance, uint8_t *d_nonces_out,
                                       int32_t *d_status, uint32_t *d_num_unsatisfied, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const size_t wire_len = frw_groth16_proof_wire_bytes(wire_mode);
    if (!ctx || wire_len == 0) return FRW_E_INVALID_ARG;
    if (!pk || !aggregate || !d_pk_bytes || !d_sig_bytes || !d_msgs || !d_msg_off || !d_rs || !d_wire || !d_status || !d_workspace)
        return FRW_E_INVALID_ARG;
    if ((uintptr_t)d_workspace & 255) return FRW_E_INVALID_ARG;
    size_t count[2];
    const frw::R1csAgg *agg = aggregate_on(aggregate, ctx, count);
    if (!agg || !aggregate_key_fits(pk, aggregate)) return FRW_E_INVALID_ARG;
    const size_t g16 = frw_groth16_workspace_bytes(pk, aggregate, 1);
    if (g16 == 0 || workspace_bytes < frw::aggregate_prove_layout(nullptr, count[0], count[1], g16).bytes) return FRW_E_INVALID_ARG;
    const frw::AggregateProveBufs ws = frw::aggregate_prove_layout(d_workspace, count[0], count[1], g16);
    const size_t total = count[0] + count[1];
    hipStream_t st = (hipStream_t)stream;
    FRW_HIP(hipSetDevice(ctx->device));
    // 1. decode, hash and screen: d_status is frw_aggregate_falcon_verify_from_bytes_dev's under FRW_RULE_CIRCUIT
    FRW_HIP(aggregate_screen_chain(ctx, agg, d_pk_bytes, d_sig_bytes, d_msgs, d_msg_off, FRW_RULE_CIRCUIT, d_status, nullptr, ws.screen, st));
    // 2. the verifier's statement, from the keys, nonces and messages alone (its own status words stay in the workspace)
    if (d_instance) FRW_HIP(aggregate_statement_launches(ctx, agg, FRW_ENC_MONTGOMERY, d_instance, ws.statement_status, ws.screen, st));
    if (d_nonces_out) FRW_HIP(hipMemcpyAsync(d_nonces_out, ws.screen.nonce, total * FRW_NONCE_LEN, hipMemcpyDeviceToDevice, st));
    // 3. the one host wait
    uint32_t refused = 0;
    FRW_HIP(hipMemcpyAsync(&refused, ws.screen.refused, sizeof refused, hipMemcpyDeviceToHost, st));
    FRW_HIP(hipStreamSynchronize(st));
    if (refused) {      // 4. an aggregate with a statement that cannot be proven has no proof
        FRW_HIP(hipMemsetAsync(d_wire, 0, wire_len, st));
        if (d_proof) FRW_HIP(hipMemsetAsync(d_proof, 0, 384, st));
        if (d_num_unsatisfied) FRW_HIP(hipMemsetAsync(d_num_unsatisfied, 0xff, sizeof(uint32_t), st));
        frw::record_error("frw_aggregate_prove_from_bytes_dev: %u of %zu statements refused (see the status words)", refused, total);
        return FRW_E_RANGE;
    }
    // 5. every statement was accepted: the witness batches are complete, in one encoding, none zero-filled
    for (int g = 0; g < 2; g++)
        if (count[g])
            FRW_HIP(launch_witness(ctx, FRW_CIRCUIT_NTT, 9 + g, FRW_ENC_MONTGOMERY, count[g], ws.screen.sig[g], ws.screen.pk[g], ws.screen.hm[g],
                                   ws.set_witness[g], ws.set_instance[g], ws.witness_status[g], st));
    int rc = frw_aggregate_assign_dev(aggregate, ws.set_witness[0], ws.set_instance[0], ws.set_witness[1], ws.set_instance[1], ws.witness,
                                      ws.instance, st);
    if (rc == FRW_OK) rc = frw_groth16_prove_rs_dev(pk, aggregate, 1, ws.witness, ws.instance, d_rs, ws.proof, ws.unsatisfied, ws.groth16_ws, ws.groth16_bytes, st);
    if (rc == FRW_OK) rc = frw_groth16_proofs_to_wire_dev(ctx->device, 1, ws.proof, wire_mode, ws.wire, ws.wire_status, st);
    if (rc != FRW_OK) return rc;
    FRW_HIP(hipMemcpyAsync(d_wire, ws.wire, wire_len, hipMemcpyDeviceToDevice, st));
    if (d_proof) FRW_HIP(hipMemcpyAsync(d_proof, ws.proof, 384, hipMemcpyDeviceToDevice, st));
    if (d_num_unsatisfied) FRW_HIP(hipMemcpyAsync(d_num_unsatisfied, ws.unsatisfied, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    return FRW_OK;
}

// The host-buffer forms: an aggregate is not divisible, so each is ONE pass of frw::host_passes over the whole statement (to the pass
// driver: a batch of one item, the aggregate), staged by StagedAggregate (frw_stage.h).
int frw_aggregate_falcon_verify_from_bytes(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *pk_bytes, const uint8_t *sig_bytes,
                                           const uint8_t *msgs, const uint64_t *msg_off, int rule, int32_t *status, uint64_t *norm)
{
    if (!ctx || (rule != FRW_RULE_CIRCUIT && rule != FRW_RULE_SPEC)) return FRW_E_INVALID_ARG;
    if (!aggregate || !pk_bytes || !sig_bytes || !msgs || !msg_off || !status) return FRW_E_INVALID_ARG;
    size_t count[2];
    if (!aggregate_on(aggregate, ctx, count)) return FRW_E_INVALID_ARG;
    const size_t total = count[0] + count[1];
    if (!frw::message_offsets_ok(msgs, msg_off, total)) return FRW_E_INVALID_ARG;
    const frw::StagedAggregate in(count[0], count[1], false, pk_bytes, sig_bytes, msgs, msg_off);
    const size_t ws_bytes = frw_aggregate_screen_workspace_bytes(aggregate);
    frw::Carve c(nullptr);
    c.take(in.bytes);
    const size_t o_ws = c.off;   c.take(ws_bytes);
    const size_t o_norm = c.off; c.take(total * sizeof(uint64_t));
    const size_t o_st = c.off;   c.take(total * sizeof(int32_t));
    return frw::host_passes(
        ctx->arena, ctx->device, 1, 1, 1, c.off, in.bytes, {{status, o_st, total * sizeof(int32_t)}, {norm, o_norm, total * sizeof(uint64_t)}},
        [&](char *d, char *stage, size_t, size_t, hipStream_t st) -> int {
            in.fill(stage);
            FRW_HIP(hipMemcpyAsync(d, stage, in.bytes, hipMemcpyHostToDevice, st));
            return frw_aggregate_falcon_verify_from_bytes_dev(aggregate, ctx, in.d_pk(d), in.d_second(d), in.d_msgs(d), in.d_off(d), rule,
                                                              (int32_t *)(d + o_st), (uint64_t *)(d + o_norm), d + o_ws, ws_bytes, st);
        });
}

int frw_aggregate_statement_from_bytes(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *pk_bytes, const uint8_t *nonces,
                                       const uint8_t *msgs, const uint64_t *msg_off, int encoding, uint64_t *instance, int32_t *status)
{
    if (bad_common(ctx, 10, encoding)) return FRW_E_INVALID_ARG;
    if (!aggregate || !pk_bytes || !nonces || !msgs || !msg_off || !instance || !status) return FRW_E_INVALID_ARG;
    size_t count[2];
    if (!aggregate_on(aggregate, ctx, count)) return FRW_E_INVALID_ARG;
    const size_t total = count[0] + count[1];
    if (!frw::message_offsets_ok(msgs, msg_off, total)) return FRW_E_INVALID_ARG;
    frw_r1cs_info_t info;
    if (frw_r1cs_info(aggregate, &info) != FRW_OK) return FRW_E_INVALID_ARG;
    const frw::StagedAggregate in(count[0], count[1], true, pk_bytes, nonces, msgs, msg_off);
    const size_t ws_bytes = frw_aggregate_screen_workspace_bytes(aggregate), ibytes = (size_t)info.num_instance * 32;
    frw::Carve c(nullptr);
    c.take(in.bytes);
    const size_t o_ws = c.off;   c.take(ws_bytes);
    const size_t o_inst = c.off; c.take(ibytes);
    const size_t o_st = c.off;   c.take(total * sizeof(int32_t));
    return frw::host_passes(
        ctx->arena, ctx->device, 1, 1, 1, c.off, in.bytes, {{instance, o_inst, ibytes}, {status, o_st, total * sizeof(int32_t)}},
        [&](char *d, char *stage, size_t, size_t, hipStream_t st) -> int {
            in.fill(stage);
            FRW_HIP(hipMemcpyAsync(d, stage, in.bytes, hipMemcpyHostToDevice, st));
            return frw_aggregate_statement_from_bytes_dev(aggregate, ctx, in.d_pk(d), in.d_second(d), in.d_msgs(d), in.d_off(d), encoding,
                                                          (uint64_t *)(d + o_inst), (int32_t *)(d + o_st), d + o_ws, ws_bytes, st);
        });
}

int frw_aggregate_prove_from_bytes(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *aggregate, const uint8_t *pk_bytes,
                                   const uint8_t *sig_bytes, const uint8_t *msgs, const uint64_t *msg_off, const uint64_t *rs, int wire_mode,
                                   uint8_t *wire, uint64_t *proof, uint64_t *instance, uint8_t *nonces_out, int32_t *status,
                                   uint32_t *num_unsatisfied)
{
    const size_t wire_len = frw_groth16_proof_wire_bytes(wire_mode);
    if (!ctx || wire_len == 0) return FRW_E_INVALID_ARG;
    if (!pk || !aggregate || !pk_bytes || !sig_bytes || !msgs || !msg_off || !rs || !wire || !status) return FRW_E_INVALID_ARG;
    size_t count[2];
    if (!aggregate_on(aggregate, ctx, count)) return FRW_E_INVALID_ARG;
    const size_t total = count[0] + count[1];
    if (!frw::message_offsets_ok(msgs, msg_off, total)) return FRW_E_INVALID_ARG;
    const size_t ws_bytes = frw_aggregate_prove_workspace_bytes(pk, aggregate);
    frw_r1cs_info_t info;
    if (ws_bytes == 0 || frw_r1cs_info(aggregate, &info) != FRW_OK) return FRW_E_INVALID_ARG;
    const frw::StagedAggregate in(count[0], count[1], false, pk_bytes, sig_bytes, msgs, msg_off, rs);
    const size_t ibytes = (size_t)info.num_instance * 32;
    frw::Carve c(nullptr);
    c.take(in.bytes);
    const size_t o_ws = c.off;   c.take(ws_bytes);
    const size_t o_wire = c.off; c.take(wire_len);
    const size_t o_prf = c.off;  c.take(384);
    const size_t o_inst = c.off; c.take(instance ? ibytes : 0);
    const size_t o_non = c.off;  c.take(total * FRW_NONCE_LEN);
    const size_t o_st = c.off;   c.take(total * sizeof(int32_t));
    const size_t o_uns = c.off;  c.take(sizeof(uint32_t));
    bool refused = false;           // the outputs of a refused aggregate are complete and go out like any others; the verdict comes after
    const int rc = frw::host_passes(
        ctx->arena, ctx->device, 1, 1, 1, c.off, in.bytes,
        {{wire, o_wire, wire_len}, {proof, o_prf, 384}, {instance, o_inst, ibytes}, {nonces_out, o_non, total * FRW_NONCE_LEN},
         {status, o_st, total * sizeof(int32_t)}, {num_unsatisfied, o_uns, sizeof(uint32_t)}},
        [&](char *d, char *stage, size_t, size_t, hipStream_t st) -> int {
            in.fill(stage);
            FRW_HIP(hipMemcpyAsync(d, stage, in.bytes, hipMemcpyHostToDevice, st));
            const int r = frw_aggregate_prove_from_bytes_dev(ctx, pk, aggregate, in.d_pk(d), in.d_second(d), in.d_msgs(d), in.d_off(d), in.d_rs(d),
                                                             wire_mode, (uint8_t *)(d + o_wire), proof ? (uint64_t *)(d + o_prf) : nullptr,
                                                             instance ? (uint64_t *)(d + o_inst) : nullptr,
                                                             nonces_out ? (uint8_t *)(d + o_non) : nullptr, (int32_t *)(d + o_st),
                                                             num_unsatisfied ? (uint32_t *)(d + o_uns) : nullptr, d + o_ws, ws_bytes, st);
            refused = r == FRW_E_RANGE;
            return refused ? FRW_OK : r;
        });
    return rc == FRW_OK && refused ? FRW_E_RANGE : rc;
}

int frw_gadget_block_len(int kind)
{
    static const int len[6] = {27, 29, 29, 18, 50, 52};
    return kind >= 0 && kind < 6 ? len[kind] : FRW_E_INVALID_ARG;
}

int frw_gadget_dev(frw_ctx *ctx, int kind, size_t count, const void *d_a, const uint64_t *d_b, int encoding,
                   uint64_t *d_out, int32_t *d_status, void *stream)
{
    frw::KernelEnc ke;
    if (bad_field_common(ctx, 10, encoding, &ke) || frw_gadget_block_len(kind) < 0) return FRW_E_INVALID_ARG;
    if (count == 0) return FRW_OK;
    if (!d_a || !d_out || (kind == FRW_G_ADD_MOD && !d_b)) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_gadget(kind, ke, count, d_a, d_b, d_out, d_status, (hipStream_t)stream));
    return FRW_OK;
}

int frw_gadget(frw_ctx *ctx, int kind, size_t count, const void *a, const uint64_t *b, int encoding, uint64_t *out,
               int32_t *status)
{
    frw::KernelEnc ke;
    if (bad_field_common(ctx, 10, encoding, &ke) || frw_gadget_block_len(kind) < 0) return FRW_E_INVALID_ARG;
    if (count == 0) return FRW_OK;
    if (!a || !out || (kind == FRW_G_ADD_MOD && !b)) return FRW_E_INVALID_ARG;
    frw::HostArena &A = ctx->arena;
    std::lock_guard<std::mutex> lock(A.mu);
    frw::DrainOnExit drain(A);
    FRW_HIP(hipSetDevice(ctx->device));
    const size_t in_bytes = count * (kind == FRW_G_MOD_Q ? 20 : 8), b_bytes = kind == FRW_G_ADD_MOD ? count * 8 : 0;
    const size_t out_bytes = count * (size_t)frw_gadget_block_len(kind) * 32;
    frw::Carve size(nullptr);
    size.take(in_bytes); size.take(b_bytes); size.take(out_bytes); size.take(count * sizeof(int32_t));
    FRW_HIP(A.reserve_device(0, size.off));
    frw::Carve c(A.d_slot[0]);
    void *d_a = c.take(in_bytes);
    uint64_t *d_b = c.take<uint64_t>(b_bytes);
    uint64_t *d_out = c.take<uint64_t>(out_bytes);
    int32_t *d_st = c.take<int32_t>(count * sizeof(int32_t));
    hipStream_t st = A.compute;
    FRW_HIP(hipMemcpyAsync(d_a, a, in_bytes, hipMemcpyHostToDevice, st));
    if (b_bytes) FRW_HIP(hipMemcpyAsync(d_b, b, b_bytes, hipMemcpyHostToDevice, st));
    FRW_HIP(frw::launch_gadget(kind, ke, count, d_a, b_bytes ? d_b : nullptr, d_out, d_st, st));
    FRW_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    if (status) FRW_HIP(hipMemcpyAsync(status, d_st, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FRW_HIP(hipStreamSynchronize(st));
    drain.settled = true;
    return FRW_OK;
}

int frw_digest_dev(frw_ctx *ctx, const uint64_t *d_buf, size_t words_per_item, size_t items, uint64_t *d_out,
                   void *stream)
{
    if (!ctx || !d_buf || !d_out) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_digest(d_buf, words_per_item, items, d_out, (hipStream_t)stream));
    return FRW_OK;
}

int frw_diag_write_stream_dev(frw_ctx *ctx, void *d_buf, size_t bytes, size_t slab_bytes, void *stream)
{
    if (!ctx || !d_buf || slab_bytes < 16) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(frw::launch_write_stream(d_buf, bytes, slab_bytes, ctx->num_cu, (hipStream_t)stream));
    return FRW_OK;
}

int frw_diag_valu_rates(frw_ctx *ctx, double out[4])
{
    if (!ctx || !out) return FRW_E_INVALID_ARG;
    frw::HostArena &A = ctx->arena;
    std::lock_guard<std::mutex> lock(A.mu);
    frw::DrainOnExit drain(A);
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(A.reserve_device(0, (size_t)ctx->num_cu * 8192));
    FRW_HIP(frw::diag_valu_rates(ctx->num_cu, A.d_slot[0], out, A.compute));
    return FRW_OK;
}

int frw_host_alloc(frw_ctx *ctx, size_t bytes, void **ptr)
{
    if (!ctx || !ptr) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return FRW_OK;
}

int frw_host_free(frw_ctx *ctx, void *ptr)
{
    // ctx may be NULL (page-locked memory does not belong to a device; a buffer may outlive the context it came from)
    if (ctx) FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(hipHostFree(ptr));
    return FRW_OK;
}

int frw_malloc(frw_ctx *ctx, size_t bytes, void **d_ptr)
{
    if (!ctx || !d_ptr) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(hipMalloc(d_ptr, bytes));
    return FRW_OK;
}

int frw_free(frw_ctx *ctx, void *d_ptr)
{
    if (!ctx) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(hipFree(d_ptr));
    return FRW_OK;
}

int frw_memcpy_h2d(frw_ctx *ctx, void *d_dst, const void *src, size_t bytes)
{
    if (!ctx) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return FRW_OK;
}

int frw_memcpy_d2h(frw_ctx *ctx, void *dst, const void *d_src, size_t bytes)
{
    if (!ctx) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return FRW_OK;
}

int frw_synchronize(frw_ctx *ctx, void *stream)
{
    if (!ctx) return FRW_E_INVALID_ARG;
    FRW_HIP(hipSetDevice(ctx->device));
    FRW_HIP(hipStreamSynchronize((hipStream_t)stream));
    return FRW_OK;
}

}  // extern "C"
