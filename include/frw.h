/*
 * frw.h -- C ABI of the MI355X Falcon-verification R1CS witness engine (libfrw.so).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (zhenfeizhang/falcon-r1cs, all citations relative to its root) has no FFI of its own; the
 * path is the Rust generic API
 *     FalconNTTVerificationCircuit::generate_constraints   falcon-r1cs/src/circuits/falcon_ntt.rs:26-123
 *     NTTPolyVar::ntt_circuit                              falcon-r1cs/src/gadgets/poly.rs:104-159
 *     mod_q / add_mod                                      falcon-r1cs/src/gadgets/arithmetics.rs:105-149, :214-262
 *     enforce_less_than_q / is_less_than_6144 / enforce_less_than_norm_bound
 *                                                          falcon-r1cs/src/gadgets/range_proofs.rs:42-94, :289-333, :274-284
 *     l2_norm_var / enforce_decompose                      falcon-r1cs/src/gadgets/misc.rs:30-51, :9-24
 * whose only observable product is the pair of assignment vectors of the arkworks
 * ConstraintSystem (witness_assignment, instance_assignment).  Because the circuit is the same
 * for every signature of one parameter set, the replacement is a batch witness filler: a Rust
 * host keeps allocating variables and emitting constraints exactly as today and takes the
 * VALUES of all W witnesses and I instance variables of `batch` signatures from one call
 * (binding shown in INTEGRATION.md).
 *
 * Conventions
 *   - plain C types only; all buffers are caller-owned; no callbacks.
 *   - `logn` is 9 (Falcon-512) or 10 (Falcon-1024); the reference selects it with a cargo
 *     feature (falcon-r1cs/Cargo.toml:28-32), here it is a run-time argument.
 *   - polynomials are `uint16_t[batch][N]`, row-major, coefficients in [0, q), q = 12289
 *     (what falcon-rust's Polynomial::coeff() returns; falcon_ntt.rs:27-28,44).
 *   - a field element is 4 x uint64_t little-endian limbs (ark-ff Fp256 over the BLS12-381
 *     scalar field).  encoding FRW_ENC_MONTGOMERY stores x*2^256 mod p -- byte-identical to
 *     what arkworks keeps in witness_assignment; FRW_ENC_CANONICAL stores x itself.  The reference is generic
 *     over F: PrimeField; every witness value is an integer below 2^160, so FRW_ENC_CANONICAL and FRW_ENC_COMPACT
 *     are field-agnostic, and a field encoding (FRW_ENC_FIELD_BASE + i, frw_ctx_field_encoding) stores x*2^256 mod p
 *     for any odd p with 2^160 < p < 2^255 in the witness, ntt, gadget and statement calls.  The R1CS satisfaction check
 *     and the products A z, B z, C z follow the field too (frw_r1csf_*, a handle made for a modulus).  What stays
 *     BLS12-381 only is everything after them: the QAP map, the MSMs, proving, verifying and the aggregates.
 *   - witness:  uint64_t[batch][W][4] in arkworks allocation order (layout: frw_layout()).
 *     instance: uint64_t[batch][I][4], I = 2N+1: [1, pk_ntt[0..N), hm_ntt[0..N)]
 *     (falcon_ntt.rs:63,67; public-input order as in examples/pok_sig.rs:38-45).
 *   - status:   int32_t[batch]: FRW_ST_OK, FRW_ST_COEFF_RANGE (an input coefficient >= q; that signature's
 *     witness and instance slots are zero-filled), FRW_ST_NORM_BOUND (l2 norm >= SIG_L2_BOUND; the witness IS written,
 *     with the truncated bit decomposition the reference assigns when its `#[cfg(not(test))]`
 *     panic is compiled out (range_proofs.rs:112-117,203-208), so the system is unsatisfied).
 *   - every function returns FRW_OK (0) or a negative FRW_E_* code; frw_strerror() names it.
 *     There is NO CPU fallback: without a usable HIP device every compute entry point fails
 *     with FRW_E_NO_DEVICE.
 *   - a context is bound to one HIP device and may be used by one host thread at a time;
 *     independent contexts may be used concurrently (the reference's ConstraintSystemRef is an
 *     Rc<RefCell<..>>, i.e. one circuit per thread as well).
 */
#ifndef FRW_H
#define FRW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRW_OK               0
#define FRW_E_INVALID_ARG   -1   /* bad logn / encoding / null pointer */
#define FRW_E_NO_DEVICE     -2   /* no HIP device, or device ordinal out of range */
#define FRW_E_HIP           -3   /* a HIP runtime call failed; see frw_last_error() */
#define FRW_E_OUT_OF_MEMORY -4
#define FRW_E_RANGE         -5   /* strict mode: at least one signature has status != FRW_ST_OK (the reference panics) */

#define FRW_ENC_CANONICAL   0
#define FRW_ENC_MONTGOMERY  1

#define FRW_ST_OK           0
#define FRW_ST_COEFF_RANGE  1
#define FRW_ST_NORM_BOUND   2
#define FRW_ST_DECODE       3   /* input preparation: malformed public key / signature encoding */

#define FRW_NUM_SEGMENTS    8

/* Witness layout = allocation order of falcon_ntt.rs:58-122, in units of field elements. */
typedef struct frw_layout {
    int32_t logn;
    int32_t n;                 /* N = 1 << logn */
    int32_t num_witness;       /* W = 153 N + {50 | 52}        (README.md:44,55: 156,724 / 78,386) */
    int32_t num_instance;      /* I = 2 N + 1                  (README.md:44,55: 2,049 / 1,025)   */
    int32_t num_constraints;   /* C = 159 N + {52 | 54}        (README.md:44,55: 162,870 / 81,460) */
    /* S0 sig[i]                          falcon_ntt.rs:58-59       N
     * S1 v[i]                            falcon_ntt.rs:71          N
     * S2 enforce_less_than_q(v[i])       falcon_ntt.rs:73-77       27 N
     * S3 mod_q blocks of ntt_circuit(sig) falcon_ntt.rs:88-89      29 N
     * S4 mod_q blocks of ntt_circuit(v)  falcon_ntt.rs:90-91       29 N
     * S5 pointwise product + add_mod     falcon_ntt.rs:94-111      30 N
     * S6 l2_norm_var over v || sig       falcon_ntt.rs:116-120     18 * 2N
     * S7 enforce_less_than_norm_bound    falcon_ntt.rs:122         50 | 52 */
    int32_t seg_off[FRW_NUM_SEGMENTS];
    int32_t seg_len[FRW_NUM_SEGMENTS];
} frw_layout_t;

typedef struct frw_ctx frw_ctx;

/* ---- structure --------------------------------------------------------------------------- */
int frw_layout(int logn, frw_layout_t *out);
const char *frw_strerror(int code);
/* text of the last failing HIP call on this thread ("" if none) */
const char *frw_last_error(void);

/* ---- device context ---------------------------------------------------------------------- */
int frw_device_count(void);
/* device = HIP ordinal >= 0.  Builds the twiddle / offset tables on that device. */
int frw_ctx_create(int device, frw_ctx **out);
void frw_ctx_destroy(frw_ctx *ctx);

/* ---- hot path, device-resident buffers (hipStream_t passed as void*; NULL = default stream) ----
 * Replaces one generate_constraints() call per signature (falcon_ntt.rs:26-123): fills the
 * witness and instance assignment of `batch` signatures.  All pointers are device pointers.
 * Asynchronous w.r.t. the host: returns after enqueueing on `stream`.
 * encoding FRW_ENC_COMPACT (see below): d_witness is the compact buffer, d_instance is ignored. */
int frw_witness_ntt_verify_dev(frw_ctx *ctx, int logn, size_t batch,
                               const uint16_t *d_sig, const uint16_t *d_pk, const uint16_t *d_hm,
                               int encoding, uint64_t *d_witness, uint64_t *d_instance,
                               int32_t *d_status, void *stream);

/* Replaces NTTPolyVar::ntt_circuit alone (poly.rs:104-159; the "ntt conversion" row of
 * examples/constraint_counts.rs:74-113): d_witness = uint64_t[batch][29 N][4] (the N mod_q
 * blocks [t, b, ltq(b)]), d_ntt_out = uint16_t[batch][N] (the b values == NTTPolynomial::from).
 * d_status: FRW_ST_OK or FRW_ST_COEFF_RANGE. */
int frw_ntt_modq_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_poly, int encoding,
                     uint64_t *d_witness, uint16_t *d_ntt_out, int32_t *d_status, void *stream);

/* ---- hot path, host buffers ----------------------------------------------------------------
 * Same results through host memory (pageable, or page-locked from frw_host_alloc: faster): H2D of the inputs, the
 * kernels, D2H of the outputs, chunked so that any batch fits the device.  This is the call the reference's own
 * consumers make -- one signature per generate_constraints (examples/constraint_counts.rs:61-63, pok_sig.rs:24-32) --
 * so it is built for batch = 1 as much as for 10^5: device buffers, a page-locked staging buffer, streams and events
 * belong to the context and only grow (a call after the first allocates nothing; frw_diag_host_allocations counts,
 * frw_ctx_trim gives the memory back), and a batch that fits one chunk is one copy in, one launch, the copies out and
 * one synchronisation.  Calls on one context are serialised (a mutex); use one context per host thread for concurrency.
 * strict != 0 mirrors the reference's non-test build: returns FRW_E_RANGE if any status != FRW_ST_OK (outputs of those
 * signatures must not be used).  strict == 0 mirrors its cfg(test) build (see FRW_ST_NORM_BOUND above).
 * encoding FRW_ENC_COMPACT: `witness` receives batch x bytes_per_signature compact bytes, `instance` may be NULL. */
int frw_witness_ntt_verify(frw_ctx *ctx, int logn, size_t batch,
                           const uint16_t *sig, const uint16_t *pk, const uint16_t *hm,
                           int encoding, uint64_t *witness, uint64_t *instance,
                           int32_t *status, int strict);

int frw_ntt_modq(frw_ctx *ctx, int logn, size_t batch, const uint16_t *poly, int encoding,
                 uint64_t *witness, uint16_t *ntt_out, int32_t *status);
/* number of device / page-locked allocations the host-buffer entry points of this context have made so far (it stops
 * growing once the largest batch shape has been seen), and release of everything they hold */
int frw_diag_host_allocations(frw_ctx *ctx, uint64_t *count);
int frw_ctx_trim(frw_ctx *ctx);

/* ---- compact encoding (no counterpart in the reference; for GPU-side consumers, the multi-GPU gather and PCIe) ----
 * 140 N + nb of the W witness elements of falcon_ntt.rs:58-122 are booleans, and all but 2 N of the others are integers
 * below 2^28.  FRW_ENC_COMPACT keeps, per signature (frw_compact_layout), the VALUES as plain integers:
 *   small     11 N x uint32_t   the non-boolean witness elements that fit 32 bits, in witness order:
 *                               sig[N], v[N], b of ntt_circuit(sig) [N], b of ntt_circuit(v) [N],
 *                               [prod, t, c] of the pointwise add_mod [3 N], [r, sq] of the 2 N l2-norm elements [4 N]
 *   t         2 N x 5 uint32_t  the mod_q quotients t = floor(a / q) of ntt_circuit(sig), then of ntt_circuit(v)
 *                               (132 / 146 bits; little-endian limbs)
 *   bits      uint32_t words    the boolean elements as a bit array in witness order (bit i of the array = bit i%32 of
 *                               word i/32): enforce_less_than_q(v[i]) 27 N bits, then the 27-bit enforce_less_than_q
 *                               blocks of the S3, S4, S5 segments (27 N each), the 16 booleans of every l2-norm element
 *                               (32 N), and the norm-bound block (50 | 52 bits, in two words of their own)
 *   instance  2 N x uint32_t    pk_ntt, hm_ntt (the leading constant one is implied)
 *   status    uint32_t          FRW_ST_* of this signature, then zeros up to the stride: a record tells its receiver (the
 *                               other end of an all-gather, say) that the signature was rejected
 * = 112,256 bytes per Falcon-1024 signature instead of 5,080,736.  frw_expand_dev / frw_expand_host rebuild, bit for bit,
 * the buffers frw_witness_ntt_verify_dev(..., FRW_ENC_MONTGOMERY, ...) writes (x -> x * 2^256 mod p for the values, 0 / the
 * Montgomery form of 1 for the booleans); a Rust host can equally build its Vec<Fr> with Fr::from(u64) / from limbs.
 * A signature with FRW_ST_COEFF_RANGE is all zeros but for its status word, and expands to what the direct entry point
 * leaves for it: zeros in the witness and in the instance vector (no leading one).  The producer writes every byte of a
 * record (padding as zeros), so equal inputs give equal bytes. */
#define FRW_ENC_COMPACT     2
typedef struct frw_compact_layout {
    int32_t logn, n;
    uint64_t bytes_per_signature;     /* stride of the compact buffer, a multiple of 128 */
    uint64_t small_off, num_small;    /* byte offset (0) and number (11 N) of the uint32_t values */
    uint64_t t_off, num_t;            /* byte offset and number (2 N) of the 5 x uint32_t quotients */
    uint64_t bits_off, num_bit_words; /* byte offset and number of uint32_t words of the bit array */
    uint64_t bit_seg_off[6];          /* first bit of S2, S3, S4, S5, S6, S7 booleans inside the bit array */
    uint64_t instance_off, num_instance_values;
    uint64_t status_off;              /* byte offset of the status word (= instance_off + 4 x num_instance_values) */
} frw_compact_layout_t;
int frw_compact_layout(int logn, frw_compact_layout_t *out);
/* d_compact: batch x bytes_per_signature bytes, 16-byte aligned.  Same statuses as frw_witness_ntt_verify_dev. */
int frw_witness_ntt_verify_compact_dev(frw_ctx *ctx, int logn, size_t batch,
                                       const uint16_t *d_sig, const uint16_t *d_pk, const uint16_t *d_hm,
                                       void *d_compact, int32_t *d_status, void *stream);
/* compact -> witness uint64_t[batch][W][4], instance uint64_t[batch][I][4] (FRW_ENC_MONTGOMERY bytes) */
int frw_expand_dev(frw_ctx *ctx, int logn, size_t batch, const void *d_compact,
                   uint64_t *d_witness, uint64_t *d_instance, void *stream);
/* The same expansion in host memory (no device; a format conversion: integers to Montgomery form, bits to 0 / 1 elements),
 * for a host that took the compact form over PCIe: frw_witness_ntt_verify(..., FRW_ENC_COMPACT, compact, NULL, status,
 * strict) moves 0.11 MB per Falcon-1024 signature instead of 5.08 MB.  Signatures are independent: callers may split
 * `batch` over threads. */
int frw_expand_host(int logn, size_t batch, const void *compact, uint64_t *witness, uint64_t *instance);

/* ---- any four-limb scalar field: the Montgomery encoding over a modulus given at run time ------------------------
 * The reference's circuits are generic over F: PrimeField (falcon_ntt.rs:20).  A host on another field -- BN254,
 * BLS12-377, Pallas / Vesta, the Jubjub or Curve25519 scalar fields -- registers F's modulus on its context and passes
 * the encoding it gets back wherever FRW_ENC_MONTGOMERY goes below; the bytes are x * 2^256 mod p, what ark-ff keeps for
 * an Fp256 over that modulus.
 *   admissible modulus   odd, 2^160 < p < 2^255 (the ladder values reach 160 bits and must not wrap; the top bit keeps the
 *                        one conditional subtraction after a Montgomery reduction enough).  Anything else:
 *                        FRW_E_INVALID_ARG.  Primality is the caller's business: a composite modulus still has
 *                        well-defined bytes x * 2^256 mod p.
 *   registry             a context holds up to FRW_MAX_FIELDS moduli; the same modulus twice gives the same encoding,
 *                        one more distinct modulus FRW_E_INVALID_ARG; the registry lives and dies with the context, and
 *                        an encoding means nothing on another context.  BLS12-381's own Fr may be registered: its field
 *                        encoding writes FRW_ENC_MONTGOMERY's bytes.
 *   accepted by          frw_witness_ntt_verify(_dev), frw_ntt_modq(_dev), frw_gadget(_dev), frw_statement(_dev) and
 *                        frw_statement_from_bytes(_dev) for every circuit (instance values are below q in all three),
 *                        frw_diag_launch_shape, frw_expand_field_dev.  Statuses, zero-fill of refused signatures,
 *                        `strict`, stream ordering and capture safety as for FRW_ENC_MONTGOMERY.
 *   refused by           (FRW_E_INVALID_ARG) the dual and schoolbook witness calls -- their is_zero multipliers and
 *                        (-q)^-1 tables are field inverses made by BLS12-381 host code --, frw_aggregate_statement*, and
 *                        every call when the id was not registered on that context.
 * frw_field_info needs no device: the constants ark-ff's FpParameters would list for the modulus. */
#define FRW_ENC_FIELD_BASE 16          /* encodings 16 .. 16 + FRW_MAX_FIELDS - 1: a field registered on the context */
#define FRW_MAX_FIELDS     8
typedef struct frw_field_info {
    uint64_t modulus[4];               /* p, little-endian limbs */
    uint64_t one[4];                   /* 2^256 mod p: what ark-ff stores for F::one() */
    uint64_t r2[4];                    /* 2^512 mod p */
    uint32_t ninv32;                   /* -p^-1 mod 2^32 */
    uint32_t bits;                     /* bit length of p */
} frw_field_info_t;
int frw_field_info(const uint64_t modulus[4], frw_field_info_t *out);
/* register `modulus` on the context, or look it up: *encoding = FRW_ENC_FIELD_BASE + its index */
int frw_ctx_field_encoding(frw_ctx *ctx, const uint64_t modulus[4], int *encoding);
/* frw_expand_dev / frw_expand_host over a registered field / a modulus: the bytes of the direct call with that encoding */
int frw_expand_field_dev(frw_ctx *ctx, int logn, size_t batch, const void *d_compact, int encoding,
                         uint64_t *d_witness, uint64_t *d_instance, void *stream);
int frw_expand_field_host(const uint64_t modulus[4], int logn, size_t batch, const void *compact,
                          uint64_t *witness, uint64_t *instance);

/* ---- the signed-split variant: FalconDualNTTVerificationCircuit (circuits/falcon_dual_ntt.rs:26-132) -----------
 * Same statement, signature and v split into non-negative (pos, neg) parts (gadgets/dual_poly.rs:15-31), four
 * ntt_circuits, two mod_q per NTT coefficient, squares without range checks (gadgets/misc.rs:55-65).
 * W = 186 N + 4 + {50|52}, I = 2 N + 1, C = 189 N + 10 + {50|52}.  Segment order (allocation order):
 *   0 sig.pos N | 1 sig.neg N | 2 pos*neg products N | 3 is_zero [is_not_equal, multiplier] 2
 *   4 v.pos N | 5 v.neg N | 6 products N | 7 is_zero 2
 *   8..11 mod_q blocks of ntt_circuit(sig.pos), (sig.neg), (v.pos), (v.neg), 29 N each
 *   12 per coefficient [sig_ntt.neg*pk_ntt, t, b, ltq(b)] [sig_ntt.pos*pk_ntt, t, b, ltq(b)], 60 N
 *   13 squares of v.pos, v.neg, sig.pos, sig.neg, 4 N | 14 norm bound
 * The signed lift uses the threshold q/2 = 6144 (falcon-rust's DualPolynomial; un-vendored). */
#define FRW_NUM_SEGMENTS_DUAL 15
typedef struct frw_layout_dual {
    int32_t logn, n, num_witness, num_instance, num_constraints;
    int32_t seg_off[FRW_NUM_SEGMENTS_DUAL];
    int32_t seg_len[FRW_NUM_SEGMENTS_DUAL];
} frw_layout_dual_t;

int frw_layout_dual(int logn, frw_layout_dual_t *out);
int frw_witness_dual_ntt_verify_dev(frw_ctx *ctx, int logn, size_t batch,
                                    const uint16_t *d_sig, const uint16_t *d_pk, const uint16_t *d_hm,
                                    int encoding, uint64_t *d_witness, uint64_t *d_instance,
                                    int32_t *d_status, void *stream);
int frw_witness_dual_ntt_verify(frw_ctx *ctx, int logn, size_t batch,
                                const uint16_t *sig, const uint16_t *pk, const uint16_t *hm,
                                int encoding, uint64_t *witness, uint64_t *instance,
                                int32_t *status, int strict);

/* ---- the schoolbook variant: FalconSchoolBookVerificationCircuit (circuits/falcon_schoolbook.rs:26-131) --------
 * Same statement over the COEFFICIENTS: instance = [1, pk[0..N), hm[0..N)] (no NTT values), and v = hm - sig * pk is
 * proved by N inner products mod q (gadgets/arithmetics.rs:34-100), one per output coefficient.
 * W = N^2 + 99 N + {50|52}, I = 2 N + 1, C = N^2 + 105 N + {52|54}.  Segments (allocation order):
 *   0 sig N
 *   1 N blocks [v[i], enforce_less_than_q(v[i]) 27]
 *   2 N columns of column_len = N + 34: [t, c, prod_0 .. prod_{N-1}, enforce_less_than_q(c) 27, ne1, mult1, ne2, mult2, and]
 *     prod_j = sig[j] * b_j with b_j = pk[i-j] (j <= i) or q - pk[N+i-j] (j > i, not reduced), sum_j prod_j = t q + c; the
 *     tail is the two is_eq gadgets and the or of rhs = hm[i] + q - c against v[i] and v[i] + q (mult = AllocatedFp::is_neq's
 *     multiplier: the inverse of the difference, or one where the operands are equal)
 *   3 l2_norm_var over v || sig, 2N blocks of 18 | 4 norm bound
 * 10.0 MB per Falcon-512 signature, 36.8 MB per Falcon-1024 signature.  Encodings FRW_ENC_CANONICAL and
 * FRW_ENC_MONTGOMERY (FRW_ENC_COMPACT: FRW_E_INVALID_ARG); statuses, `strict` and every other convention as for
 * frw_witness_dual_ntt_verify.  The _dev form is one kernel launch (stream-capture safe). */
#define FRW_NUM_SEGMENTS_SCHOOLBOOK 5
typedef struct frw_layout_schoolbook {
    int32_t logn, n, num_witness, num_instance, num_constraints, column_len;
    int32_t seg_off[FRW_NUM_SEGMENTS_SCHOOLBOOK];
    int32_t seg_len[FRW_NUM_SEGMENTS_SCHOOLBOOK];
} frw_layout_schoolbook_t;

int frw_layout_schoolbook(int logn, frw_layout_schoolbook_t *out);
int frw_witness_schoolbook_verify_dev(frw_ctx *ctx, int logn, size_t batch,
                                      const uint16_t *d_sig, const uint16_t *d_pk, const uint16_t *d_hm,
                                      int encoding, uint64_t *d_witness, uint64_t *d_instance,
                                      int32_t *d_status, void *stream);
int frw_witness_schoolbook_verify(frw_ctx *ctx, int logn, size_t batch,
                                  const uint16_t *sig, const uint16_t *pk, const uint16_t *hm,
                                  int encoding, uint64_t *witness, uint64_t *instance,
                                  int32_t *status, int strict);

/* ---- R1CS matrix export (structure only; host, no GPU) --------------------------------------------------------
 * What a prover ingests after the hot path (examples/pok_sig.rs:30-32: Groth16 setup/prove call cs.to_matrices()):
 * A, B, C of the chosen circuit with every symbolic linear combination inlined.  Column j < I is instance variable
 * j (column 0 = the constant one), column I + k is witness k -- the same order as the witness/instance buffers
 * above.  File: "FRWR1CS1", u64 {I, W, C, nnz_A, nnz_B, nnz_C}, then per matrix CSR: u64 row_ptr[C+1],
 * u32 col[nnz], u64 value[nnz][4] (canonical little-endian).  counts (optional) receives the six header words. */
#define FRW_CIRCUIT_NTT       0   /* FalconNTTVerificationCircuit      circuits/falcon_ntt.rs      */
#define FRW_CIRCUIT_DUAL_NTT  1   /* FalconDualNTTVerificationCircuit  circuits/falcon_dual_ntt.rs */
#define FRW_CIRCUIT_SCHOOLBOOK 2  /* FalconSchoolBookVerificationCircuit circuits/falcon_schoolbook.rs */
int frw_r1cs_export(int circuit, int logn, const char *path, uint64_t *counts);

/* Batch satisfaction check on the device: the reference's `assert!(cs.is_satisfied())` (falcon_ntt.rs:159) for every
 * signature of an HBM-resident batch, against the matrices above (emitted from the gadget definitions, independently
 * of the witness kernels' closed form).  frw_r1cs_load builds them on the host (seconds) and uploads them once;
 * d_witness / d_instance are the buffers of the witness entry points with encoding FRW_ENC_MONTGOMERY;
 * d_num_unsatisfied[i] = number of constraint rows signature i violates (0 = satisfied).
 * (Diagnostics: with FRW_R1CS_NO_FLAT set in the environment at load time the handle's short rows are evaluated by the CSR walk
 * instead of from their flattened form -- the route of a circuit with more than 254 distinct coefficients; the tests run both.) */
typedef struct frw_r1cs frw_r1cs;
int frw_r1cs_load(int device, int circuit, int logn, frw_r1cs **out);
void frw_r1cs_free(frw_r1cs *r);
int frw_r1cs_check_dev(const frw_r1cs *r, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                       uint32_t *d_num_unsatisfied, void *stream);
/* Same pass, additionally writing the three matrix-vector products a prover's QAP witness map starts from (what
 * ark-groth16 computes on the CPU right after generate_constraints, examples/pok_sig.rs:32):
 * d_abc = uint64_t[batch][3][C][4] = A z, B z, C z per signature, Montgomery form, rows in constraint order.
 * frw_r1cs_check_dev and frw_r1cs_eval_dev take a stream-ordered scratch allocation (hipMallocAsync / hipFreeAsync on
 * `stream`) per call -- they are NOT stream-capture safe -- and run slower kernels should that allocation fail.  The
 * _scratch_ variant below is the same computation with the caller's scratch: no allocation, one fixed kernel sequence. */
int frw_r1cs_eval_dev(const frw_r1cs *r, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                      uint32_t *d_num_unsatisfied, uint64_t *d_abc, void *stream);
/* d_scratch: at least frw_r1cs_eval_scratch_bytes(r, batch, d_abc != NULL) bytes, 16-byte aligned (may be NULL when
 * that is 0).  d_abc may be NULL (check only). */
size_t frw_r1cs_eval_scratch_bytes(const frw_r1cs *r, size_t batch, int with_products);
int frw_r1cs_eval_scratch_dev(const frw_r1cs *r, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                              uint32_t *d_num_unsatisfied, uint64_t *d_abc, void *d_scratch, size_t scratch_bytes,
                              void *stream);

/* ---- any constraint system: A, B, C as CSR arrays, or the FRWR1CS1 file frw_r1cs_export writes ------------------------------
 * Everything behind a `frw_r1cs *` -- the satisfaction check and A z, B z, C z, the witness map, frw_groth16_setup_r1cs(_opts),
 * the prove / partial / verify / wire / re-randomise calls and their keys -- is Groth16 over BLS12-381 for the system the handle holds;
 * these two make a handle from matrices that come from anywhere (a Rust host: ark-relations' cs.to_matrices()).
 *     counts   {I, W, C, nnz_A, nnz_B, nnz_C}
 *     for m = 0, 1, 2 (A, B, C): row_ptr[m] u64[C + 1], col[m] u32[nnz_m], val[m] u64[nnz_m][4] canonical little-endian -- the
 *     arrays of the file, in host memory (read during the call only)
 * Columns as in the export: 0 is the constant one, 1 .. I - 1 the public inputs, I + k witness k.  Every consumer's buffers are
 * witness uint64_t[batch][W][4] and instance uint64_t[batch][I][4] in ark-ff's Montgomery bytes, element 0 of the instance = one;
 * every element canonical (limbs < p) -- the precondition of frw_qap_witness_map_dev below holds for these handles too.
 * Accepted on purpose: unsorted columns, a column repeated within a row (the terms add), zero coefficients, empty rows, variables no
 * row mentions (their a_query, b_*_query and l_query entries are the point at infinity).
 * Refused with FRW_E_INVALID_ARG before any device call, frw_last_error() naming the matrix and the row: a null pointer; I == 0 or
 * C == 0; I + W >= 2^30 or C + I > 2^30; row_ptr[m][0] != 0, a decreasing row_ptr, row_ptr[m][C] != nnz_m; a column >= I + W; a
 * value >= the group order; and for files one that cannot be opened, another magic, or a length that is not exactly what the
 * header implies.  Validation comes first, then the device: without a GPU a malformed system is FRW_E_INVALID_ARG and a
 * well-formed one FRW_E_NO_DEVICE.
 * The QAP domain is next_power_of_two(C + I), as ark-groth16 takes it (the key depends on it): 2^1 .. 2^30, every one of them with
 * a witness map on the device (below 2^14: frw_qap_small.hip).
 * What stays Falcon-only: the witness kernels, and with them frw_pok_prove_from_bytes(_dev), frw_pok_prove_workspace_bytes (0) and
 * the aggregate calls -- they refuse these handles, also one whose counts are a Falcon circuit's (the export loaded back).
 * frw_r1cs_info reports num_statements = 1 and count_logn9 = count_logn10 = 0 for them: how a caller tells them from
 * frw_r1cs_load's. */
int frw_r1cs_load_csr(int device, const uint64_t counts[6], const uint64_t *const row_ptr[3], const uint32_t *const col[3],
                      const uint64_t *const val[3], frw_r1cs **out);
int frw_r1cs_load_file(int device, const char *path, frw_r1cs **out);

/* ---- the check and the products over ANY four-limb field: a handle made for a modulus given at run time ---------------------
 * The reference's circuits are `impl<F: PrimeField> ConstraintSynthesizer<F>`; a field encoding (frw_ctx_field_encoding) makes the
 * witness over any odd p with 2^160 < p < 2^255, and these calls say whether it satisfies the circuit -- cs.is_satisfied() and
 * which_is_unsatisfied() over that field -- and give A z, B z, C z, the three vectors a foreign-field prover's witness_map starts
 * from.  The modulus follows frw_field_info's rule (anything else: FRW_E_INVALID_ARG); BLS12-381's own group order is admissible.
 * A `frw_r1csf *` goes into these calls and into frw_qapf_create (the QAP witness map over that field, below) only: the hard-wired
 * QAP map, the keys and the provers take a `frw_r1cs *`, BLS12-381.
 *
 * frw_r1cs_export_field / frw_r1csf_load: the matrices the host mirror emits (frw_r1cs_export), carried over to p.  Every
 * coefficient of the three Falcon circuits is an integer (+-1, powers of two, +-q, twiddle products, ladder offsets -- the inverses
 * of the dual and schoolbook circuits are witness values), so the matrices over p are the centred lift of the matrices over the group
 * order r (v > r / 2 ? v - r : v) reduced mod p.  A coefficient whose lift reaches 2^200 (the largest a circuit holds is 160 bits)
 * breaks that premise: FRW_E_INVALID_ARG, frw_last_error() naming the matrix and the row.  The file is the FRWR1CS1 layout with values
 * canonical mod `modulus`; it does not record the modulus.  `circuit` is any of FRW_CIRCUIT_*.
 * frw_r1csf_load_csr / frw_r1csf_load_file: matrices that come from anywhere, canonical mod `modulus`; accepted and refused as
 * frw_r1cs_load_csr lists above, "a value >= the group order" reading "a value >= modulus".  Validation comes first, then the device:
 * without a GPU a malformed system is FRW_E_INVALID_ARG and a well-formed one FRW_E_NO_DEVICE.
 *
 * frw_r1csf_check_dev: d_witness uint64_t[batch][W][4] and d_instance uint64_t[batch][I][4] in ark-ff's bytes over that modulus
 * (x 2^256 mod p: what a field encoding writes, what Fp256<P> holds), every element canonical (limbs < p; an element >= p gives an
 * unspecified count, the call stays memory-safe).
 *     d_num_unsatisfied[i]    the rows statement i violates
 *     d_first_unsatisfied[i]  optional: the lowest violated row, 0xffffffff if none (ark's which_is_unsatisfied, as an index)
 *     d_abc                   optional: uint64_t[batch][3][C][4] = A z, B z, C z, Montgomery form over p, rows in constraint order
 *                             (the layout of frw_r1cs_eval_dev); NULL: check only
 * A statement whose instance[0] is not 2^256 mod p -- a refused, zero-filled slot of the witness calls; a buffer in another
 * encoding -- is reported with num = C, first = 0 and zeros in its d_abc slot, and none of its rows is evaluated: a zero assignment
 * satisfies a system whose constant is read from it, and must not pass as "0 violated rows".
 * d_scratch: at least frw_r1csf_scratch_bytes(r, batch, d_abc != NULL) bytes, 16-byte aligned; may be NULL where that is 0 (a system
 * without rows of 64 terms or more).  It holds the plain values of the variables the long rows read and, check only, those rows' products.
 * Nothing is allocated and nothing synchronises: everything is ordered on `stream` alone, one kernel after the other, so the call
 * may be captured and the captured graph has no parallel branches.  batch = 0 returns FRW_OK before anything else is looked at. */
typedef struct frw_r1csf frw_r1csf;
typedef struct {
    uint64_t modulus[4];
    uint64_t num_instance, num_witness, num_constraints, nnz[3];
    uint64_t scratch_bytes_per_statement[2];  /* check only, with products */
} frw_r1csf_info_t;
int frw_r1cs_export_field(int circuit, int logn, const uint64_t modulus[4], const char *path, uint64_t *counts);
int frw_r1csf_load(int device, int circuit, int logn, const uint64_t modulus[4], frw_r1csf **out);
int frw_r1csf_load_csr(int device, const uint64_t modulus[4], const uint64_t counts[6],
                       const uint64_t *const row_ptr[3], const uint32_t *const col[3],
                       const uint64_t *const val[3], frw_r1csf **out);
int frw_r1csf_load_file(int device, const uint64_t modulus[4], const char *path, frw_r1csf **out);
void frw_r1csf_free(frw_r1csf *r);
int frw_r1csf_info(const frw_r1csf *r, frw_r1csf_info_t *out);
size_t frw_r1csf_scratch_bytes(const frw_r1csf *r, size_t batch, int with_products);
int frw_r1csf_check_dev(const frw_r1csf *r, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                        uint32_t *d_num_unsatisfied, uint32_t *d_first_unsatisfied /* may be NULL */,
                        uint64_t *d_abc /* may be NULL: check only */, void *d_scratch, size_t scratch_bytes, void *stream);

/* ---- the QAP witness map over ANY four-limb field with a radix-2 domain ------------------------------------------------------
 * The step after A z, B z, C z in Groth16::prove over a field other than BLS12-381's: R1CStoQAP::witness_map,
 * h(X) = (A(X) B(X) - C(X)) / (X^n - 1) over ark-poly's Radix2EvaluationDomain::new(C + I) of that field (the QAP map section below
 * restates it).  The G1 sum over such a field's curve is frw_msmf_* (below); a foreign key or prover is not here.
 *
 * frw_fft_field_info (no device): with p - 1 = 2^s t, t odd, two_adicity = s and two_adic_root = generator^t -- what ark-ff's
 * FftParameters lists.  The multiplicative generator is the caller's (ark-bn254: 5, ark-bls12-381: 7, ark-bls12-377: 22, Pallas and
 * Vesta: 5); the library hard-wires none.  FRW_E_INVALID_ARG, frw_last_error() naming the rule: a modulus outside frw_field_info's
 * rule; a generator that is 0 or >= p; generator^(p - 1) != 1 (a failed Fermat test -- the inverses below are Fermat inverses, so this
 * much primality is the library's business); root^(2^(s - 1)) != -1 (the generator is a square: the root has no order 2^s).
 * frw_qapf_domain (no device): Radix2EvaluationDomain::new(C + I), every value canonical.  Refused: log_size > s (ark's
 * PolynomialDegreeTooLarge), log_size > 22, generator^n = 1 (the coset is the domain itself and the division has no inverse).
 *
 * frw_qapf_create borrows `r` (r must outlive the handle) and makes the domain's tables on r's device; frw_qapf_witness_map_dev has the
 * semantics of frw_qap_witness_map_dev:
 *     d_h                uint64_t[batch][n][4], Montgomery form over p, canonical, coefficient k of h at index k
 *     d_num_unsatisfied  optional uint32_t[batch]: the rows statement i violates (frw_r1csf_check_dev's count)
 *     d_workspace        16-byte aligned, at least workspace_bytes_per_statement bytes (less: FRW_E_INVALID_ARG); the batch is processed
 *                        in chunks of as many statements as it holds
 * ark-groth16's seven transforms as written, for EVERY statement -- a = A z ++ instance, b = B z, c = C z; ifft; coset_fft by the
 * generator; a o b - c; x vanishing_inv; coset_ifft -- so an unsatisfied witness gets ark's interpolant like a satisfied one (there is
 * no six-transform quotient and no list mode over a foreign field).  A statement whose instance[0] is not 2^256 mod p reports
 * num = C, as the check does, and its h slot is all zero.  Domains 2^1 .. 2^min(s, 22): up to 2^12 a workgroup keeps an array in LDS
 * for a whole transform (num_passes = 1); 2^13 .. 2^16 take two passes over HBM, 2^17 .. 2^22 three.  Over p = BLS12-381's r with
 * generator 7 the result is byte for byte frw_qap_witness_map_dev's.  Nothing is allocated and nothing synchronises: everything runs on
 * `stream` as one chain without parallel branches, so the call may be captured.  batch = 0 returns FRW_OK before anything else is
 * looked at.  Same canonical-limbs precondition as frw_r1csf_check_dev. */
typedef struct {
    uint64_t modulus[4];
    uint64_t generator[4];
    uint32_t two_adicity;              /* s */
    uint32_t reserved;
    uint64_t two_adic_root[4];         /* generator^t, canonical */
    uint64_t two_adic_root_mont[4];    /* ... x 2^256 mod p: what ark-ff stores */
} frw_fft_field_info_t;
typedef struct {
    uint32_t log_size;
    uint32_t reserved;
    uint64_t size;                     /* n = next_power_of_two(C + I) */
    uint64_t group_gen[4];             /* the root squared s - log_size times */
    uint64_t group_gen_inv[4];
    uint64_t size_inv[4];
    uint64_t generator_inv[4];
    uint64_t vanishing_inv[4];         /* (generator^n - 1)^-1 */
} frw_qapf_domain_t;
typedef struct {
    frw_qapf_domain_t domain;
    uint64_t num_constraints, num_instance;    /* C, I */
    uint32_t num_passes;               /* HBM passes one transform takes at this size */
    uint32_t reserved;
    uint64_t workspace_bytes_per_statement;
} frw_qapf_info_t;
typedef struct frw_qapf frw_qapf;
int frw_fft_field_info(const uint64_t modulus[4], const uint64_t generator[4], frw_fft_field_info_t *out);
int frw_qapf_domain(const uint64_t modulus[4], const uint64_t generator[4], uint64_t num_constraints, uint64_t num_instance,
                    frw_qapf_domain_t *out);
int frw_qapf_create(const frw_r1csf *r, const uint64_t generator[4], frw_qapf **out);
void frw_qapf_free(frw_qapf *q);
int frw_qapf_info(const frw_qapf *q, frw_qapf_info_t *out);
int frw_qapf_witness_map_dev(const frw_qapf *q, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                             uint64_t *d_h, uint32_t *d_num_unsatisfied /* may be NULL */, void *d_workspace,
                             size_t workspace_bytes, void *stream);

/* ---- multi-scalar multiplication over ANY four-limb curve y^2 = x^3 + b -----------------------------------------------------------
 * The step after h in Groth16::prove over BN254 or a Pasta curve (and a KZG / IPA commitment on its own): VariableBaseMSM::
 * multi_scalar_mul over G1.  A curve is {base modulus q, scalar modulus r, b}: a = 0, q and r each admissible by frw_field_info's rule
 * (odd, 2^160 < . < 2^255), b canonical with 0 < b < q.  The library hard-wires no curve.  Primality of q and r and the group's order are
 * the caller's business; r serves ONE purpose, bringing a Montgomery-form scalar back to its integer.  There is NO subgroup check: BN254
 * G1, Pallas, Vesta and Grumpkin have cofactor 1; for any other curve it is the caller's.  The same sum over G2 is frw_msmf2_* (below); foreign
 * keys, pairings and a foreign prover are not here.
 *
 * A point is affine, uint64_t[8]: x then y, each four little-endian limbs of v 2^256 mod q (ark-ff's Fp256); all zero is the point at
 * infinity (b != 0: (0, 0) is never on the curve).
 *
 * Host only, no device: frw_curve_info (the refusals of a descriptor, and its constants); frw_curve_check_points (*first_bad = the first
 * point with a coordinate >= q or off the curve, -1: none); frw_curve_scalar_mul (out[i] = scalars[i] points[i] for plain 256-bit
 * integers, ANY value up to 2^256 - 1, by double-and-add: the reference; a point off the curve is refused).
 *
 * frw_msmf_load copies the n <= 2^22 bases to `device` as they are -- 64 bytes a point, no window tables -- after one thread per base
 * has checked it: a bad base refuses the load with FRW_E_INVALID_ARG and frw_last_error() names the first bad index;
 * FRW_MSMF_POINTS_ARE_CHECKED skips the check.  frw_msmf_dev writes, per statement s < batch,
 *     d_out[s] = sum_{i < num_scalars} k_(s,i) P_i        k_(s,i) = d_scalars[(s scalar_stride + i) 4 ..], four limbs
 * as the unique affine point (infinity: all zero).  num_scalars <= num_points uses the first num_scalars bases: a key loaded once for a
 * domain of n points serves h directly with scalar_stride = n, num_scalars = n - 1, which is what ark-groth16 sums.
 *     montgomery = 0     k is a plain 256-bit integer: the integer multiple, for any value up to 2^256 - 1, no reduction by r
 *     montgomery != 0    k is ark-ff's h 2^256 mod r (what frw_qapf_witness_map_dev writes), brought to the integer h < r first
 *     d_workspace        16-byte aligned, at least workspace_bytes_per_statement bytes; the batch goes through it in chunks of as many
 *                        statements as it holds (frw_msmf_workspace_bytes(m, k): what k statements in flight take)
 * Stream-ordered, nothing allocated, no synchronisation, capturable.  batch = 0 and num_scalars = 0 are valid (the latter writes infinity).
 * FRW_E_INVALID_ARG with a message: an inadmissible q or r, b = 0 or b >= q, num_points = 0 or > 2^22, num_scalars > num_points,
 * scalar_stride < num_scalars, a workspace smaller than one statement's or a misaligned buffer, null pointers. */
typedef struct { uint64_t base_modulus[4], scalar_modulus[4], b[4]; } frw_curve_t;
typedef struct {
    uint32_t base_bits, scalar_bits;   /* bit lengths of q and r */
    uint64_t b_mont[4];                /* b 2^256 mod q */
    uint64_t one_mont[4];              /* 2^256 mod q: a coordinate equal to one */
    uint64_t scalar_one_mont[4];       /* 2^256 mod r: a Montgomery-form scalar equal to one */
} frw_curve_info_t;
typedef struct {
    uint64_t num_points;
    uint32_t window_bits, num_windows; /* 13 x 20 below 2^16 points, 15 x 18 from there on: signed digits, 2^(window_bits - 1) buckets a window */
    uint64_t reserved;
    uint64_t bases_bytes;              /* device memory the handle holds */
    uint64_t workspace_bytes_per_statement;
} frw_msmf_info_t;
#define FRW_MSMF_POINTS_ARE_CHECKED 1
typedef struct frw_msmf frw_msmf;
int frw_curve_info(const frw_curve_t *c, frw_curve_info_t *out);
int frw_curve_check_points(const frw_curve_t *c, size_t count, const uint64_t *points, int64_t *first_bad);
int frw_curve_scalar_mul(const frw_curve_t *c, size_t count, const uint64_t *points, const uint64_t *scalars /* [count][4] */,
                         uint64_t *out /* [count][8] */);
int frw_msmf_load(int device, const frw_curve_t *c, size_t num_points, const uint64_t *bases, int flags, frw_msmf **out);
void frw_msmf_free(frw_msmf *m);
int frw_msmf_info(const frw_msmf *m, frw_msmf_info_t *out);
size_t frw_msmf_workspace_bytes(const frw_msmf *m, size_t batch_in_flight);
int frw_msmf_dev(const frw_msmf *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, size_t num_scalars, int montgomery,
                 uint64_t *d_out /* [batch][8] */, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- multi-scalar multiplication over G2: a curve y^2 = x^3 + b' over a run-time Fq2 --------------------------------------------------
 * What a Groth16 prover over BN254 sums for B in G2 (b_g2_query), and what a loader of such a key checks: VariableBaseMSM::
 * multi_scalar_mul over a curve on the quadratic extension Fq2 = Fq[u] / (u^2 - nonresidue).  A curve is {base modulus q, scalar modulus
 * r, nonresidue, b' = c0 + c1 u}: q and r as frw_curve_t's, 0 < nonresidue < q, both components of b' canonical below q and b' != 0.
 * nonresidue = q - 1 (u^2 = -1: BN254, BLS12-381) is recognised and costs no product; any other value costs one more field product per
 * Fq2 product.  The library hard-wires no curve.  THE CALLER'S BUSINESS, none of it checked: that nonresidue is a quadratic non-residue
 * mod q (otherwise Fq2 is no field and the inversions are wrong), that q and r are prime, the group's order, and the SUBGROUP -- the
 * twist of a pairing-friendly curve has a cofactor (BN254's G2: 2 q - r), and there is NO subgroup check here.  r serves ONE purpose,
 * bringing a Montgomery-form scalar back to its integer.  Foreign keys, pairings and a foreign prover are not here.
 *
 * A point is affine, uint64_t[16]: x.c0, x.c1, y.c0, y.c1 (ark-ff's Fp2 order), each four little-endian limbs of v 2^256 mod q; all zero
 * is the point at infinity.
 *
 * Host only, no device: frw_curve2_info, frw_curve2_check_points (*first_bad = the first point with a component >= q or off the curve,
 * -1: none), frw_curve2_scalar_mul (plain 256-bit integers, ANY value, double-and-add: the reference; a point off the curve is refused).
 *
 * frw_msmf2_load / _free / _info / _workspace_bytes / _dev are frw_msmf_*'s contract word for word -- the scalars, scalar_stride,
 * num_scalars, montgomery, the chunking through d_workspace, the 16-byte alignment, batch = 0 and num_scalars = 0, stream order and
 * capture -- with 128 bytes a base and d_out uint64_t[batch][16].  FRW_MSMF_POINTS_ARE_CHECKED skips the on-curve check of the load.
 * FRW_E_INVALID_ARG with a message: an inadmissible q or r, nonresidue = 0 or >= q, a component of b' >= q or b' = 0, num_points = 0 or
 * > 2^22, num_scalars > num_points, scalar_stride < num_scalars, a workspace smaller than one statement's or a misaligned buffer, null
 * pointers, a base that is not on the curve (named by its index). */
typedef struct { uint64_t base_modulus[4], scalar_modulus[4], nonresidue[4], b[8]; } frw_curve2_t;   /* b = c0 then c1, canonical */
typedef struct {
    uint32_t base_bits, scalar_bits;   /* bit lengths of q and r */
    uint64_t b_mont[8];                /* b' 2^256 mod q, c0 then c1 */
    uint64_t one_mont[4];              /* 2^256 mod q: the c0 of a coordinate equal to one */
    uint64_t nonresidue_mont[4];       /* nonresidue 2^256 mod q */
    uint64_t scalar_one_mont[4];       /* 2^256 mod r */
    uint32_t nonresidue_is_minus_one;  /* 1: u^2 = -1, the cheaper products */
    uint32_t reserved;
} frw_curve2_info_t;
typedef struct {
    uint64_t num_points;
    uint32_t window_bits, num_windows; /* 13 x 20 below 2^16 points, 15 x 18 from there on */
    uint64_t reserved;
    uint64_t bases_bytes;              /* device memory the handle holds */
    uint64_t workspace_bytes_per_statement;
} frw_msmf2_info_t;
typedef struct frw_msmf2 frw_msmf2;
int frw_curve2_info(const frw_curve2_t *c, frw_curve2_info_t *out);
int frw_curve2_check_points(const frw_curve2_t *c, size_t count, const uint64_t *points /* [count][16] */, int64_t *first_bad);
int frw_curve2_scalar_mul(const frw_curve2_t *c, size_t count, const uint64_t *points, const uint64_t *scalars /* [count][4] */,
                          uint64_t *out /* [count][16] */);
int frw_msmf2_load(int device, const frw_curve2_t *c, size_t num_points, const uint64_t *bases, int flags, frw_msmf2 **out);
void frw_msmf2_free(frw_msmf2 *m);
int frw_msmf2_info(const frw_msmf2 *m, frw_msmf2_info_t *out);
size_t frw_msmf2_workspace_bytes(const frw_msmf2 *m, size_t batch_in_flight);
int frw_msmf2_dev(const frw_msmf2 *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, size_t num_scalars, int montgomery,
                  uint64_t *d_out /* [batch][16] */, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- QAP witness map (the step after the hot path in a Groth16 prover) ------------------------------------------
 * examples/pok_sig.rs:30-47 hands the circuit to Groth16::<Bls12_381>::prove; after generate_constraints the prover's
 * first step is ark-groth16 0.3.0's R1CStoQAP::witness_map (r1cs_to_qap.rs): the coefficients of
 *     h(X) = (A(X) B(X) - C(X)) / (X^n - 1)
 * over ark-poly's Radix2EvaluationDomain of size n = next_power_of_two(C + I) (2^17 for Falcon-512, 2^18 for
 * Falcon-1024), computed as  a = A z ++ instance values, b = B z, c = C z;  ifft, coset_fft (generator 7);
 * a o b - c;  / (7^n - 1);  coset_ifft.  frw_qap_witness_map_dev returns exactly that h for every signature of an HBM-resident
 * batch, whatever the witness -- by running the six-transform quotient below for all of them (the same h wherever the witness
 * satisfies the system) and then ark-groth16's seven transforms, as written, for just the signatures whose witness does not
 * (normally none: those launches find an empty list) -- from the buffers the witness entry points wrote (FRW_ENC_MONTGOMERY):
 *     d_h               uint64_t[batch][n][4], Montgomery form, coefficient k of h at index k (what the prover feeds,
 *                       after into_repr, to the MSM over pk.h_query; the last coefficient is zero for a satisfied system)
 *     d_num_unsatisfied optional uint32_t[batch]: constraint rows the witness violates (h is then not a quotient)
 *     d_workspace       at least workspace_bytes_per_signature bytes; the batch is processed in chunks of as many
 *                       signatures as fit.
 * Returns FRW_E_INVALID_ARG for a null pointer, a workspace smaller than one signature's, or a domain outside 2^1 .. 2^30.
 * Domains 2^1 .. 2^13 (systems loaded by frw_r1cs_load_csr / frw_r1cs_load_file; tests/test_gpu_r1cs_custom.py): ark-groth16's seven
 * transforms as written for every statement, plain radix-2 stages, one workgroup per array -- in LDS up to 2^12, through the workspace
 * at 2^13 (frw_qap_small.hip); same buffers, same workspace formula, same properties.  From 2^14
 * (the transforms run as passes of six, five or four radix-2 stages: 2^17 = 6 + 6 + 5 and 2^18 = 6 + 6 + 6 for the Falcon
 * circuits, 2^19 = 6 + 5 + 4 + 4 .. 2^24 = 6 + 6 + 6 + 6, 2^25 = 6 + 5 + 5 + 5 + 4 .. 2^27 = 6 + 6 + 5 + 5 + 5 for aggregate statements.
 * RUN AND TESTED: every domain 2^17 .. 2^27 (tests/test_gpu_qap.py, tests/test_gpu_aggregate.py) -- 2^27 is the 1,024-statement
 * aggregate of BASELINE configs[4], whose thirteen per-index factor tables (56 GB) are made on the device; the schedules of
 * 2^28 .. 2^30 come from the same rule and are checked by the exact-integer model of tests/test_qap_schedule.py only: a 2^28 domain's
 * tables alone are 120 GB, and the smallest statement that needs it is 1,600 Falcon-1024 verifications).  Stream-ordered: everything is enqueued on
 * `stream` and NOTHING is allocated -- the sparse products borrow the working arrays, idle at that point, as their
 * scratch -- so a call may be captured in a HIP graph.  A HIP failure is recorded for frw_last_error().
 * Precondition: every witness / instance element is canonical Montgomery form (limbs < p), which is what arkworks and
 * the witness entry points produce; the 29-bit evaluation path does not reduce its inputs, so an element >= p gives an
 * h that is wrong without an error code. */
typedef struct {
    int32_t log_domain_size;
    uint64_t domain_size;                      /* n */
    uint64_t num_constraints, num_instance;    /* C, I */
    uint64_t workspace_bytes_per_signature;    /* 3 C x 32 (A z, B z, C z) + 3 x 32 n (working arrays) + 64 (flags) */
} frw_qap_info_t;
int frw_qap_info(const frw_r1cs *r, frw_qap_info_t *out);
int frw_qap_witness_map_dev(const frw_r1cs *r, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                            uint64_t *d_h, uint32_t *d_num_unsatisfied, void *d_workspace, size_t workspace_bytes,
                            void *stream);
/* The same quotient with six transforms instead of seven, for witnesses that satisfy the system: with
 * a(X) b(X) = lo(X) + X^n hi(X), h = hi = ((a b mod X^n - 1) - (a b mod X^n + 1)) / 2 -- the first from the pointwise
 * products on the domain, the second from those on the coset psi H, psi^n = -1; C z is computed for d_num_unsatisfied but
 * not transformed.  d_num_unsatisfied[i] == 0  =>  d_h[i] is exactly frw_qap_witness_map_dev's (ark-groth16's) h.
 * Otherwise d_h[i] is still hi, which is NOT what ark-groth16 returns for an unsatisfied system (nor a quotient).
 * Same arguments and workspace as frw_qap_witness_map_dev.  On the domains below 2^14 there is one map: this call returns
 * frw_qap_witness_map_dev's h there, for every witness. */
int frw_qap_quotient_dev(const frw_r1cs *r, size_t batch, const uint64_t *d_witness, const uint64_t *d_instance,
                         uint64_t *d_h, uint32_t *d_num_unsatisfied, void *d_workspace, size_t workspace_bytes,
                         void *stream);
/* Host buffers: witness uint64_t[batch][W][4], instance uint64_t[batch][I][4] (the constant one first) -- the bytes of
 * arkworks' witness_assignment / instance_assignment -- to h uint64_t[batch][n][4]; num_unsatisfied may be NULL.
 * Synchronous; 64 signatures in flight; the device buffers belong to the handle and only grow (a second call of the
 * same shape allocates nothing: frw_r1cs_diag_host_allocations).  Same canonical-limbs precondition as above. */
int frw_qap_witness_map(const frw_r1cs *r, size_t batch, const uint64_t *witness, const uint64_t *instance,
                        uint64_t *h, uint32_t *num_unsatisfied);
int frw_r1cs_diag_host_allocations(const frw_r1cs *r, uint64_t *count);

/* ---- an aggregate statement: many Falcon verifications, ONE constraint system, ONE proof ---------------------------------------
 * BASELINE configs[4] / SURVEY 8-f row 4.  The reference's falcon-aggregate-sig crate is an empty stub
 * (falcon-aggregate-sig/src/main.rs:1-3); the statement is defined the only way the reference's own circuits allow:
 * FalconNTTVerificationCircuit::generate_constraints (falcon_ntt.rs:26-123) run once per (pk, msg, sig) on one constraint
 * system, in order (host mirror: FalconAggregateVerificationCircuit in csrc/host/frw_host.hpp), proved by the flow of
 * examples/pok_sig.rs:30-47.  For statements i = 0 .. count-1 with parameter sets logn[i] (9 or 10, freely mixed):
 *     instance_assignment = [1, pk_ntt_0, hm_ntt_0, pk_ntt_1, hm_ntt_1, ...]            I = 1 + sum 2 N_i
 *     witness_assignment  = witness_0 ++ witness_1 ++ ...                              W = sum W_i
 *     constraints         = those of statement 0, then of statement 1, ...            C = sum C_i
 *     QAP domain          = next_power_of_two(C + I):  2^18 for 512 + 1024, 2^19 for two Falcon-1024, 2^20 for four, 2^22 for sixteen
 * frw_r1cs_load_aggregate returns a handle that every entry point taking a `frw_r1cs *` accepts (frw_r1cs_check_dev,
 * frw_r1cs_eval_dev, frw_qap_info, frw_qap_witness_map_dev, frw_qap_quotient_dev, frw_groth16_workspace_bytes,
 * frw_groth16_prove_dev), with d_witness = uint64_t[batch][W][4] and d_instance = uint64_t[batch][I][4] the aggregate's OWN
 * vectors (batch = number of aggregate statements of this shape, normally 1) -- which frw_aggregate_assign_dev makes from the
 * batches the witness entry points wrote: statement i takes the next unused signature of its parameter set's batch, so
 * d_witness_512 / d_instance_512 hold the Falcon-512 statements in order and d_witness_1024 / d_instance_1024 the Falcon-1024
 * ones (either pair may be NULL if the aggregate has no such statement).  The aggregate's matrices are never materialised: they
 * are the per-signature systems' blocks, and a run of consecutive statements of one parameter set is one launch of that set's
 * kernels reading the aggregate vectors in place.  d_num_unsatisfied counts the violated rows of the whole statement.
 * frw_aggregate_assign_dev -- preconditions it cannot check: the Falcon-512 batch holds at least count_logn9 signatures and the
 * Falcon-1024 batch count_logn10 (frw_r1cs_info), both written with the SAME encoding (the aggregate's constant one is copied from the
 * first statement's own instance vector) and none of them rejected (FRW_ST_COEFF_RANGE zero-fills a slot: its leading one too).
 * Device-to-device copies on `stream` only -- two per run of consecutive statements of one parameter set --, capture-safe.
 * THE CHECKED WAY IN is frw_aggregate_prove_from_bytes_dev (below): it screens every statement first and calls this only when all
 * were accepted, so the three preconditions hold by construction; a chain assembled by hand must keep them itself.
 * frw_groth16_setup_r1cs is frw_groth16_setup for the system behind any handle; the proving key of an aggregate has one query
 * point per variable of the whole statement.  As window tables that is 3.6 KB of G1 tables x 3 and 7.2 KB of G2 per variable and
 * 1.8 KB per domain point of h_query: 53 GB for sixteen Falcon-1024 statements -- the fastest proofs, up to there.  Beyond, the key
 * keeps the points alone (FRW_KEY_BARE below: 112 / 224 bytes a point) and the sums run window by window over them: the 1,024 mixed
 * statements of BASELINE configs[4] (513 Falcon-512 + 511 Falcon-1024: C + I = 126.6 M, the 2^27 domain -- round 4 had written 2^28
 * and 480 GB here, both wrong) are 121.9 M variables, 83 GB of points, ONE proof in 0.6 s on one MI355X. */
typedef struct {
    uint64_t num_statements;                    /* 1 for the handles of frw_r1cs_load, frw_r1cs_load_csr and frw_r1cs_load_file */
    uint64_t count_logn9, count_logn10;         /* both 0: a system that came in as matrices (frw_r1cs_load_csr / _file) */
    uint64_t num_instance, num_witness, num_constraints;    /* I (with the constant one), W, C of the whole system */
    int32_t log_domain_size;
    int32_t witness_map_on_device;              /* 0: the device has no transform for this domain (2^1 .. 2^30 have) */
} frw_r1cs_info_t;
int frw_r1cs_load_aggregate(int device, size_t count, const int32_t *logn, frw_r1cs **out);
int frw_r1cs_info(const frw_r1cs *r, frw_r1cs_info_t *out);
int frw_aggregate_assign_dev(const frw_r1cs *aggregate, const uint64_t *d_witness_512, const uint64_t *d_instance_512,
                             const uint64_t *d_witness_1024, const uint64_t *d_instance_1024, uint64_t *d_witness,
                             uint64_t *d_instance, void *stream);

/* ---- multi-scalar multiplication over BLS12-381 G1 (the step after the witness map in a Groth16 prover) --------------
 * ark-groth16 0.3.0 prover.rs, create_proof_with_reduction_and_matrices (what examples/pok_sig.rs:30-47 runs):
 *     h_acc = VariableBaseMSM::multi_scalar_mul(&pk.h_query, &h_assignment)
 * and likewise over a_query / b_g1_query / l_query.  The bases are the proving key's: fixed per circuit.  frw_msm_g1_load
 * takes them once (host memory, ark-ff's bytes: per point x then y, each 6 x uint64_t little-endian limbs of the Fq element
 * in Montgomery form, all zero = the point at infinity) and builds a device table of 2^(16 j) P_i for the sixteen 16-bit
 * windows j (448 bytes per point); frw_msm_g1_dev then computes sum_i k_i P_i for every signature of a batch:
 *     d_scalars   uint64_t[batch][scalar_stride][4]; the first num_points elements of each signature's vector are used.
 *                 montgomery != 0: ark-ff's Fr Montgomery form (what frw_qap_witness_map_dev writes); 0: canonical
 *                 integers < r (what into_repr() gives; a 256-bit integer >= r is taken mod r, never out of bounds)
 *     d_out       uint64_t[batch][12]: the affine result in ark-ff's bytes (x, y; all zero = infinity) -- the bytes of the
 *                 G1Affine arkworks' into_affine() would hold
 *     d_workspace at least workspace_bytes_per_signature (frw_msm_info) bytes, 16-byte aligned; the batch is processed in
 *                 chunks of as many signatures as fit
 * Stream-ordered, allocates nothing.  Scalars that are zero cost nothing and scalars that are one are summed apart from the
 * buckets, so the witness-side sums of the prover (a_query, b_g1_query, l_query with a Falcon witness: 91 % of its elements
 * are 0 or 1) run as fast as h_acc, whose coefficients are uniform field elements.  Any other heavy repetition of ONE digit
 * (all scalars equal to 2, say) is computed correctly and still in parallel: a bucket above 1.5 x the mean size is cut into
 * equal work items, one thread each, whose sums a second kernel adds up.
 * frw_groth16_msm_h_dev is the call for h_acc: scalars = the first domain_size - 1 coefficients of every h as the witness
 * map left them (stride domain_size, Montgomery form); num_points must equal domain_size - 1. */
/* k_i G1 for `count` canonical scalars (uint64_t[count][4], < r) -> uint64_t[count][12] affine points in ark-ff's bytes, host
 * buffers: the FixedBaseMSM over the generator ark-groth16's generator.rs builds the proving key's queries with (h_query[i] =
 * (zt / delta) t^i G1, ...) -- here so that a key can be made on the device; 8-bit windows, 32 mixed additions per scalar. */
int frw_g1_fixed_base(int device, size_t count, const uint64_t *scalars, uint64_t *out);
/* The same in G2 (b_g2_query[i] = v_i(t) G2): uint64_t[count][24] out -- x.c0, x.c1, y.c0, y.c1 of the Fq2 coordinates. */
int frw_g2_fixed_base(int device, size_t count, const uint64_t *scalars, uint64_t *out);
typedef struct frw_msm frw_msm;
typedef struct {
    uint64_t num_points;
    int32_t window_bits, num_windows;          /* 16, 16; a _narrow handle: 8, 32 */
    uint64_t table_bytes;                      /* 16 x num_points x 112 (G2: 224); a _narrow handle: 32 x num_points x 112, and for up to 2^18
                                                * points as much again for the sums of the 255 non-empty subsets of every group of eight points */
    uint64_t workspace_bytes_per_signature;    /* sort keys (64 num_points bytes), the list of scalars equal to one (4 num_points),
                                                * 32,768 buckets + 131,072 work items + 4,096 partial sums x 240 bytes (G2: 464),
                                                * counters; a _narrow handle: 128 + 4 num_points bytes of keys and list, the partial
                                                * sums of its work items and of the ones */
} frw_msm_info_t;
int frw_msm_g1_load(int device, size_t num_points, const uint64_t *bases, frw_msm **out);
void frw_msm_free(frw_msm *m);
int frw_msm_info(const frw_msm *m, frw_msm_info_t *out);
int frw_msm_g1_dev(const frw_msm *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, int montgomery,
                   uint64_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
int frw_groth16_msm_h_dev(const frw_msm *m, size_t batch, const uint64_t *d_h, size_t domain_size, uint64_t *d_out,
                          void *d_workspace, size_t workspace_bytes, void *stream);
/* G2 (the prover's g2_b = MSM(b_g2_query, assignment) + ...): bases uint64_t[num_points][24], results uint64_t[batch][24]
 * (x.c0, x.c1, y.c0, y.c1; ark-ff's G2Affine limbs), everything else as for G1.  A handle serves the group it was loaded for;
 * the other group's _dev call returns FRW_E_INVALID_ARG.  Same algorithm over Fq2 (a G2 addition is three times a G1 one and
 * the kernel spills registers: fine for the 10^5 additions a witness-side sum needs, not tuned for more). */
int frw_msm_g2_load(int device, size_t num_points, const uint64_t *bases, frw_msm **out);
/* The same handles with 8-bit windows (32 of them: the table is twice as long; num_points <= 2^25): 128 buckets per signature
 * instead of 32,768, so nothing is spent on folding empty buckets.  For sums whose scalars are mostly zero, one or small -- a
 * witness as scalars (the sums over a_query, b_g1_query, b_g2_query, l_query: frw_groth16_pk_load uses these) -- this is three
 * times faster than the 16-bit tables; for dense 255-bit scalars (h) it is twice the additions and the 16-bit tables win.
 * A narrow handle of up to 2^18 points also holds, for every group of eight consecutive points, the sums of its 255 non-empty subsets:
 * the scalars equal to one (45 % of a Falcon witness, in long runs of booleans) then cost one addition per group instead of one each.
 * Every other call (frw_msm_info, frw_msm_g1_dev / _g2_dev, frw_msm_free) takes either kind of handle. */
int frw_msm_g1_load_narrow(int device, size_t num_points, const uint64_t *bases, frw_msm **out);
int frw_msm_g2_load_narrow(int device, size_t num_points, const uint64_t *bases, frw_msm **out);
int frw_msm_g2_dev(const frw_msm *m, size_t batch, const uint64_t *d_scalars, size_t scalar_stride, int montgomery,
                   uint64_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
/* BARE handles (round 5): the points themselves and no window table -- 112 (G2: 224) bytes a point, up to 2^31 - 1 of them.  A sum then
 * runs window by window over the same rows (narrow == 0: sixteen 16-bit windows, the dense pipeline -- for uniform scalars such as h;
 * narrow != 0: thirty-two 8-bit windows sorted in one pass -- for a witness as scalars), the window sums put together by Horner's rule:
 * the bucket additions of the table path, one per point and non-zero digit, plus 255 point operations.  Results are the same affine
 * points, bit for bit.  frw_msm_info: table_bytes = num_points x 112 (224); one scalar vector is summed at a time, whatever the workspace.
 * narrow == 2: a dense bare handle on WIDE windows -- thirteen of 20 bits instead of sixteen of 16: 19 % fewer bucket additions (a bare
 * handle's windows cost no memory), a two-level counting sort whose passes write runs; frw_msm_info then says 20 and 13.  A dense bare
 * handle of 2^26 points and more takes wide windows by itself (the folds of 13 x 2^19 buckets are a fixed 14 ms: below that size they cost
 * more than three windows' additions save); on the 2^27-point sum of the 1,024-statement aggregate 423 -> 356 ms. */
int frw_msm_g1_load_bare(int device, size_t num_points, const uint64_t *bases, int narrow, frw_msm **out);
int frw_msm_g2_load_bare(int device, size_t num_points, const uint64_t *bases, int narrow, frw_msm **out);

/* ---- a whole Groth16 proof per signature (the rest of examples/pok_sig.rs:30-47) ---------------------------------------------------
 * ark-groth16 0.3.0 prover.rs, create_proof_with_reduction_and_matrices, for every signature of a resident batch of witnesses:
 * the witness map, the five multi-scalar multiplications (h_query; a_query, b_g1_query, l_query, b_g2_query with the
 * assignment), the blinding terms and the assembly of (A, B, C).  frw_groth16_pk_load takes the proving key's elements in
 * ark-ff's bytes (host memory; G1 points 12 x uint64_t, G2 points 24) and builds the five device tables once.
 *     rs        host, uint64_t[batch][2][4]: the blinding factors r, s of every proof, canonical integers < the group order
 *               (create_random_proof draws them; create_proof_no_zk passes zeros)
 *     d_proofs  uint64_t[batch][48]: A (G1Affine limbs, 12), B (G2Affine limbs, 24), C (12)
 *     d_num_unsatisfied  optional uint32_t[batch]: constraint rows the witness violates (the proof is then worthless)
 *     d_workspace  frw_groth16_workspace_bytes(pk, r, in_flight) bytes, 256-byte aligned; the batch runs in chunks that fit
 * d_witness / d_instance: what the witness entry points wrote (FRW_ENC_MONTGOMERY).  Ordered on `stream` -- the sort of the
 * scalars' digits runs there, the rest on streams of the key's own (the witness map and the sum over h_query on one, the three G1
 * witness-side sums as one chain of kernels followed by both scalar multiplications on another, G2 on a third), forked from and
 * joined back into `stream` by events -- except for the upload of `rs`, which is waited for before the call goes on (the array
 * may be short-lived).
 * Calls with one key may come from several host threads: they take turns putting their work on the key's streams (each with a
 * workspace of its own).  A call that returns an error has waited for whatever it had already started.
 * NOT stream-capture safe (frw_groth16_prove_rs_dev is): once per chunk the call waits on the host (hipStreamSynchronize on
 * `stream`) for the upload of r, s -- i.e. also for whatever `stream` held before -- and only then takes the
 * key's lock, so concurrent provers do not wait for each other's streams. */
typedef struct frw_groth16_pk frw_groth16_pk;
typedef struct {
    uint64_t num_instance, num_witness, domain_size;      /* I (with the constant one), W, n */
    const uint64_t *alpha_g1, *beta_g1, *delta_g1;         /* vk.alpha_g1, pk.beta_g1, pk.delta_g1 */
    const uint64_t *beta_g2, *delta_g2;                    /* vk.beta_g2, vk.delta_g2 */
    const uint64_t *a_query, *b_g1_query;                  /* [I + W][12] */
    const uint64_t *b_g2_query;                            /* [I + W][24] */
    const uint64_t *h_query;                               /* [n - 1][12] */
    const uint64_t *l_query;                               /* [W][12] */
} frw_groth16_pk_desc_t;
int frw_groth16_pk_load(int device, const frw_groth16_pk_desc_t *desc, frw_groth16_pk **out);
/* ---- keys beyond what window tables can hold, and keys in slices (round 5; BASELINE configs[4]: ONE proof for 1,024 statements) -------
 * The window tables above are a speed-up, not a requirement: 3.6 KB per variable and 1.8 KB per domain point make a sixteen-statement key
 * 53 GB.  A key of BARE handles keeps the points only (112 bytes a G1 point, 224 a G2 point: 83 GB for the 1,024-statement aggregate --
 * 513 Falcon-512 + 511 Falcon-1024, 121.9 M variables, the 2^27 domain) and its sums run window by window over the same rows: the same
 * number of bucket additions (one per point and non-zero digit), plus 255 point operations per sum to put the windows together.  Such a
 * key also knows in which rows b_g1_query / b_g2_query hold a point -- the variables some constraint has on its B side: 59 % of a Falcon
 * circuit's, with half of a witness's ones and none of its full-size values: a third of the additions -- and sums those two tables over them alone (an index
 * made when the key is put together, a second, short sort per proof: frw_diag_groth16_side_counts has the numbers).
 *   FRW_KEY_TABLES  window tables (the fastest proofs; what frw_groth16_pk_load and frw_groth16_setup make)
 *   FRW_KEY_BARE    the points only
 *   FRW_KEY_AUTO    tables up to FRW_KEY_AUTO_TABLE_VARIABLES variables (some sixteen Falcon-1024 statements: 50 GB), bare beyond
 * rank / world: a key in slices (bare handles only) -- this handle holds slice `rank` of `world` of every query: rows [z_lo, z_hi) of the
 * nv + 3 rows of a_query ++ [alpha, delta, O] and of the three tables laid out like it, and [h_lo, h_hi) of h_query (frw_groth16_pk_info;
 * the split is by equal counts, the first `total mod world` slices one longer).  A slice proves nothing by itself: every rank runs
 * frw_groth16_prove_partial_dev on the WHOLE witness (the witness map is recomputed by every rank: a tenth of the sums' time) with the SAME
 * blinding factors, which sums its slices of the five queries into FRW_GROTH16_PARTIAL_WORDS uint64_t -- A | B1' | L | H as G1Affine limbs (12
 * each) | B as G2Affine limbs (24), partial sums all, the blinding terms r delta_1, alpha_1, beta, s delta_2 inside those of the last rank;
 * the partial sums of all ranks in rank order (one all-gather of 576 bytes per rank) go to frw_groth16_prove_combine_dev on any rank, which
 * adds them up, applies s A + r B1' and writes the proof A | B | C -- byte for byte the proof of the whole key. */
#define FRW_KEY_AUTO    0
#define FRW_KEY_TABLES  1
#define FRW_KEY_BARE    2
#define FRW_KEY_AUTO_TABLE_VARIABLES 3000000
typedef struct {
    int32_t mode;               /* FRW_KEY_* */
    uint32_t rank, world;       /* world <= 1: the whole key */
} frw_groth16_key_opts_t;
typedef struct {
    int32_t mode;               /* FRW_KEY_TABLES or FRW_KEY_BARE */
    uint32_t rank, world;
    uint64_t z_lo, z_hi;        /* rows of the witness-side tables this handle holds, of num_instance + num_witness + 3 */
    uint64_t h_lo, h_hi;        /* rows of h_query, of domain_size - 1 */
    uint64_t key_bytes;         /* device memory of the five tables */
} frw_groth16_pk_info_t;
int frw_groth16_pk_load_opts(int device, const frw_groth16_pk_desc_t *desc, const frw_groth16_key_opts_t *opts, frw_groth16_pk **out);
int frw_groth16_pk_info(const frw_groth16_pk *pk, frw_groth16_pk_info_t *out);
/* one of the key's five tables as the frw_msm handle it is (borrowed: it goes with the key; never frw_msm_free it) -- for sums over a
 * single query, e.g. frw_groth16_msm_h_dev(frw_groth16_pk_query(pk, FRW_QUERY_H), ...) checked against (h(t) zt / delta) G1.  The
 * witness-side tables have num_instance + num_witness + 3 rows (see frw_groth16_key_opts_t); a slice of a key is a slice here too. */
#define FRW_QUERY_H   0
#define FRW_QUERY_A   1
#define FRW_QUERY_B1  2
#define FRW_QUERY_L   3
#define FRW_QUERY_B2  4
const frw_msm *frw_groth16_pk_query(const frw_groth16_pk *pk, int which);
/* ark-groth16 0.3.0 generator.rs generate_parameters for one of the Falcon circuits, with the toxic waste GIVEN:
 * toxic = uint64_t[5][4], canonical: alpha, beta, gamma, delta and the evaluation point t (circuit_specific_setup draws them
 * from its rng, and random generators of G1 / G2; here the published generators are used).  The QAP is evaluated at t on the
 * host (the circuit's matrices, Lagrange coefficients), the queries are fixed-base multiples made on the device, and the proving
 * key comes back loaded.  vk_out (optional): alpha_g1 (12) | beta_g2 (24) | gamma_g2 (24) | delta_g2 (24) | gamma_abc_g1 [I][12]
 * uint64_t -- the verifying key's elements in ark-ff's bytes.  FRW_E_INVALID_ARG if t lies in the domain or gamma / delta is 0.
 * A key whose toxic waste somebody knows proves nothing to anybody else; this is for tests, benchmarks and ceremonies that
 * combine contributions. */
int frw_groth16_setup(int device, int circuit, int logn, const uint64_t *toxic, frw_groth16_pk **pk_out, uint64_t *vk_out);
/* the same for the system behind a handle (a per-signature circuit or an aggregate statement), on the handle's device;
 * vk_out: 84 + 12 x num_instance uint64_t */
int frw_groth16_setup_r1cs(const frw_r1cs *r, const uint64_t *toxic, frw_groth16_pk **pk_out, uint64_t *vk_out);
/* The same with the kind of key chosen (frw_groth16_setup_r1cs is FRW_KEY_AUTO, whole).  A key of bare handles is made ON THE DEVICE end to
 * end: the Lagrange coefficients of the whole domain at t, the QAP's polynomials at t as transposed sparse products over the per-signature
 * matrices (block by block, in place), the queries' scalars, and every query point written straight into its table row by the fixed-base
 * kernels -- nothing of the statement's size exists in host memory but the verifying key's gamma_abc_g1 (the 1,024-statement key: 83 GB of
 * rows, 1.57 M points of gamma_abc_g1).  With world > 1 only this rank's slices are made (vk_out, if given, is the whole verifying key on
 * every rank). */
int frw_groth16_setup_r1cs_opts(const frw_r1cs *r, const uint64_t *toxic, const frw_groth16_key_opts_t *opts, frw_groth16_pk **pk_out,
                                uint64_t *vk_out);
void frw_groth16_pk_free(frw_groth16_pk *pk);
size_t frw_groth16_workspace_bytes(const frw_groth16_pk *pk, const frw_r1cs *r, size_t batch_in_flight);
int frw_groth16_prove_dev(const frw_groth16_pk *pk, const frw_r1cs *r, size_t batch, const uint64_t *d_witness,
                          const uint64_t *d_instance, const uint64_t *rs, uint64_t *d_proofs, uint32_t *d_num_unsatisfied,
                          void *d_workspace, size_t workspace_bytes, void *stream);
/* The same with the blinding factors in DEVICE memory (d_rs: uint64_t[batch][2][4], any 256-bit values: taken modulo the group
 * order; their split by the curve's endomorphism, done on the host for the call above until round 4, happens on the device for
 * both).  Nothing waits on the host: the call is ordered on `stream` throughout and MAY be captured into a HIP graph and replayed
 * (one capture = one chunk: give it the workspace of the whole batch; the key's streams join the capture through its events and
 * leave it before the call returns).  A replay reads the factors that are in d_rs THEN: refresh them between replays -- or capture
 * frw_groth16_prove_seeded_dev (below, "drawing the factors on the device"), which draws them inside the graph. */
int frw_groth16_prove_rs_dev(const frw_groth16_pk *pk, const frw_r1cs *r, size_t batch, const uint64_t *d_witness,
                             const uint64_t *d_instance, const uint64_t *d_rs, uint64_t *d_proofs, uint32_t *d_num_unsatisfied,
                             void *d_workspace, size_t workspace_bytes, void *stream);

/* A key in slices (see frw_groth16_key_opts_t).  d_witness / d_instance: the WHOLE statement's vectors, on every rank; rs: host,
 * uint64_t[batch][2][4], the same on every rank; d_partial: uint64_t[batch][FRW_GROTH16_PARTIAL_WORDS]; workspace as frw_groth16_prove_dev
 * (frw_groth16_workspace_bytes).  A whole key (world == 1) may be used too: its "partial" sums are the sums. */
#define FRW_GROTH16_PARTIAL_WORDS 72
#define FRW_GROTH16_COMBINE_WORKSPACE 4096
int frw_groth16_prove_partial_dev(const frw_groth16_pk *pk, const frw_r1cs *r, size_t batch, const uint64_t *d_witness,
                                  const uint64_t *d_instance, const uint64_t *rs, uint64_t *d_partial, uint32_t *d_num_unsatisfied,
                                  void *d_workspace, size_t workspace_bytes, void *stream);
/* d_partials: uint64_t[world][FRW_GROTH16_PARTIAL_WORDS] in rank order (device memory); rs: host, uint64_t[2][4]; d_proof: uint64_t[48];
 * d_workspace: FRW_GROTH16_COMBINE_WORKSPACE bytes, 256-byte aligned.  `pk` names the device (any rank's handle). */
int frw_groth16_prove_combine_dev(const frw_groth16_pk *pk, size_t world, const uint64_t *d_partials, const uint64_t *rs, uint64_t *d_proof,
                                  void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Groth16 verification (examples/pok_sig.rs:34-47: Groth16::verify(&vk, &public_inputs, &proof)) --------------------------------
 * ark-groth16 0.3.0 verifier.rs: prepare_verifying_key (e(alpha_g1, beta_g2), -gamma_g2, -delta_g2), prepare_inputs
 * (gamma_abc_g1[0] + sum x_i gamma_abc_g1[i]) and verify_proof: e(A, B) e(inputs, -gamma_g2) e(C, -delta_g2) == e(alpha_g1, beta_g2)
 * as one product of three Miller loops and one final exponentiation.  HOST code like the reference's (about 15 ms per proof on
 * one core; a batch runs one proof per host thread); no device is needed (frw_groth16_verify_dev below: prepare_inputs on one).
 *     vk          the layout frw_groth16_setup writes: alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | gamma_abc_g1[num_instance]
 *                 (FRW_E_INVALID_ARG if a coordinate's limbs are not below the field modulus, a point is not on its curve or
 *                 not in the subgroup of order r -- every point, gamma_abc_g1 included: what ark's deserialiser checks)
 *     instance    uint64_t[batch][num_instance][4], encoding FRW_ENC_MONTGOMERY or FRW_ENC_CANONICAL: the instance vector AS THE
 *                 WITNESS ENTRY POINTS WRITE IT, i.e. the constant one first and then ark's public inputs (pk_ntt || hm_ntt)
 *     proofs      uint64_t[batch][48]: A | B | C as frw_groth16_prove_dev writes them
 *     flags       FRW_VERIFY_POINTS_ARE_CHECKED: skip the subgroup checks of A, B, C (ark checks them when it deserialises a proof;
 *                 these are raw limbs, so the check is made here unless the caller vouches for the points)
 *     accepted    int32_t[batch]: 1 the proof verifies, 0 it does not, -1 malformed: an instance value whose limbs (in either
 *                 encoding) are >= r, instance[0] != 1, a coordinate whose limbs are >= the field modulus (x + q is not accepted
 *                 for x), a point off its curve or outside the subgroup -- or, with FRW_VERIFY_POINTS_ARE_CHECKED, a point the
 *                 caller vouched for wrongly that drives the Miller loop into a vertical line */
#define FRW_VERIFY_POINTS_ARE_CHECKED 1
#define FRW_VERIFY_BATCHED 2          /* frw_groth16_verify_full_dev only: see there */
typedef struct frw_groth16_vk frw_groth16_vk;
int frw_groth16_vk_load(const uint64_t *vk, size_t num_instance, frw_groth16_vk **out);
/* flags: FRW_VK_POINTS_ARE_CHECKED -- the caller vouches for gamma_abc_g1 being on the curve and in the subgroup (a key it made itself a
 * moment ago: the 1,024-statement aggregate has 1.57 M of these points, a 255-bit ladder each); canonical limbs are still required and the
 * four fixed points are still checked. */
#define FRW_VK_POINTS_ARE_CHECKED 1
int frw_groth16_vk_load_opts(const uint64_t *vk, size_t num_instance, int flags, frw_groth16_vk **out);
void frw_groth16_vk_free(frw_groth16_vk *vk);
int frw_groth16_verify(const frw_groth16_vk *vk, size_t batch, const uint64_t *instance, int encoding, const uint64_t *proofs,
                       int flags, int32_t *accepted);
/* The same verifier with prepare_inputs ON THE DEVICE (round 6), for instance vectors and proofs that are in device memory already.
 * frw_groth16_vk_load_dev: the host key as frw_groth16_vk_load makes it, plus a copy of gamma_abc_g1 on `device` as a narrow MSM handle
 * (a table handle up to 2^18 points, a bare one beyond).  EVERY gamma_abc_g1 point is checked on the device: canonical limbs (< q), on
 * the curve, in the subgroup of order r (all zero = infinity is accepted, as on the host) -- the checks frw_groth16_vk_load makes, by the
 * same code; the four fixed points are checked on the host.  flags must be 0: FRW_VK_POINTS_ARE_CHECKED -> FRW_E_INVALID_ARG (vouching
 * is what this call makes unnecessary).  No device -> FRW_E_NO_DEVICE (no host fallback).  The handle serves frw_groth16_verify
 * unchanged too; frw_groth16_vk_free frees both parts. */
int frw_groth16_vk_load_dev(int device, const uint64_t *vk, size_t num_instance, int flags, frw_groth16_vk **out);
/* bytes of device workspace for `batch_in_flight` proofs (16-byte aligned; a smaller one runs a batch in chunks); 0 for a key without
 * a device part */
size_t frw_groth16_verify_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight);
/* prepare_inputs on the device: stream-ordered, allocates nothing.
 *     d_instance  uint64_t[batch][num_instance][4], FRW_ENC_MONTGOMERY or FRW_ENC_CANONICAL, as the witness entry points write it
 *     d_prepared  uint64_t[batch][12]: gamma_abc_g1[0] + sum_{i>=1} x_i gamma_abc_g1[i], affine, ark-ff's bytes (all zero = infinity;
 *                 all zero too where d_status is -1)
 *     d_status    int32_t[batch]: 0, or -1 malformed -- a value whose raw limbs are >= r (either encoding) or instance[0] != 1: exactly
 *                 the cases where frw_groth16_verify returns -1 because of the instance vector
 *     d_workspace at least frw_groth16_verify_workspace_bytes(vk, 1) bytes, 16-byte aligned
 * FRW_E_INVALID_ARG for a null pointer, a small or misaligned workspace, or a key without a device part. */
int frw_groth16_prepare_inputs_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, uint64_t *d_prepared,
                                   int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);
/* frw_groth16_verify with the instance vectors and the proofs in device memory (d_proofs: uint64_t[batch][48], as frw_groth16_prove_dev
 * writes them).  prepare_inputs runs on the device (above); one affine point, one status and the 384 proof bytes per proof are then
 * copied to the host, which does the rest -- the proof points' canonical / on-curve / subgroup checks, three Miller loops and the final
 * exponentiation, one proof per host thread, the code frw_groth16_verify runs.  accepted: HOST int32_t[batch], the values
 * frw_groth16_verify gives for the same bytes and flags.  Synchronises `stream`; not capture-safe.  Workspace as above: as many
 * proofs per pass as it holds.  A key without a device part -> FRW_E_INVALID_ARG. */
int frw_groth16_verify_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, const uint64_t *d_proofs,
                           int flags, int32_t *accepted, void *d_workspace, size_t workspace_bytes, void *stream);
/* diagnostics for the parity tests: the verifier's pairing of one pair (g1: 12, g2: 24 uint64_t), written as the twelve
 * coefficients of 1, w, ..., w^11 in Fq[w] / (w^12 - 2 w^6 + 2), 6 uint64_t each in ark-ff's form.  The value is the CUBE of the
 * reduced ate pairing (frw_pairing.h says why that is as good). */
int frw_diag_pairing(const uint64_t *g1, const uint64_t *g2, uint64_t *out);
/* The WHOLE verification on the device (frw_pairing_dev.hip): prepare_inputs as frw_groth16_prepare_inputs_dev, then the proof points'
 * checks, the three Miller loops, the final exponentiation and the comparison with e(alpha, beta)^3 -- no host round trip, verdicts in
 * device memory.  The key must come from frw_groth16_vk_load_dev (it uploads -gamma, -delta and beta's Miller-loop line tables,
 * e(alpha, beta)^3 and the Frobenius constants, computed on the host at load); any other key -> FRW_E_INVALID_ARG.
 *     d_accepted     DEVICE int32_t[batch]: what frw_groth16_verify returns for the same bytes and flags -- 1, 0 or -1 (an instance value
 *                    >= r or instance[0] != 1, a coordinate >= q, a point off its curve or outside the subgroup, a vertical line in the
 *                    Miller loop of a point vouched for wrongly)
 *     flags          FRW_VERIFY_POINTS_ARE_CHECKED and / or FRW_VERIFY_BATCHED; any other bit -> FRW_E_INVALID_ARG
 *     seed           HOST uint64_t[4], read with FRW_VERIFY_BATCHED (required then: NULL -> FRW_E_INVALID_ARG)
 *     d_batch_passed DEVICE int32_t (may be NULL): with FRW_VERIFY_BATCHED, 1 if the batched check passed in every pass, else 0
 *     d_workspace    at least frw_groth16_verify_full_workspace_bytes(vk, 1, flags) bytes, 16-byte aligned; a smaller one than the batch
 *                    needs runs it in chunks (about 26 KB per proof in flight besides prepare_inputs' share, 0.6 KB more batched)
 * FRW_VERIFY_BATCHED: the well-formed proofs of a pass (not -1) are checked together first.  rho_i = the first 128 bits of
 * SHAKE256(seed || le64(i) || proof i's 384 bytes), i the proof's index in the whole batch (one if they are all zero), and
 *     prod_i e(rho_i A_i, B_i) e(sum rho_i P_i, -gamma) e(sum rho_i C_i, -delta) e(-(sum rho_i) alpha, beta) == 1
 * (P_i the prepared inputs): N + 3 Miller loops, a product tree, ONE final exponentiation.  If it holds, every well-formed proof of the
 * pass gets 1; if not, the per-proof check decides each (its kernels are always launched and return at once when the batched check
 * passed).  Soundness: a pass holding a proof that the per-proof check rejects passes the batched check with probability at most about
 * 2^-128 over the choice of the rho_i -- PROVIDED the seed is chosen after the proofs and statements are fixed (unpredictable to whoever
 * made them; a fresh random seed per call).  A seed known in advance lets a prover craft proofs whose errors cancel.
 * Stream-ordered on `stream`, allocates nothing, does not synchronise: capture-safe.  batch = 0 is a no-op.  FRW_E_INVALID_ARG for a null
 * pointer, a bad encoding, a small or misaligned workspace. */
size_t frw_groth16_verify_full_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight, int flags);
int frw_groth16_verify_full_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, const uint64_t *d_proofs,
                                int flags, const uint64_t *seed, int32_t *d_accepted, int32_t *d_batch_passed, void *d_workspace,
                                size_t workspace_bytes, void *stream);

/* ---- proofs and verifying keys in arkworks' wire format (frw_wire.hip) ----------------------------------------------------------------
 * What ark-groth16's Proof and VerifyingKey are on disk, in a message or across a process boundary: ark-serialize's CanonicalSerialize
 * (ark-serialize / ark-ec 0.3, short-Weierstrass affine points over BLS12-381), restated here from the crates' sources (parity unpinned:
 * DESIGN.md).  Everything above takes and gives uint64_t limbs in ark-ff's Montgomery form; these calls convert, on the host or on the
 * device, by the same code.
 *   Fq            48 bytes, little-endian, the CANONICAL integer (not x 2^384); a value >= q is malformed
 *   Fq2           c0 then c1, 96 bytes
 *   flags         the top two bits of the last byte of the last field element written: bit 7 = "y is the greater one", bit 6 = infinity
 *                 (bit 5 of an Fq top byte is always 0; the flags are masked off before the >= q test)
 *   greater       y > -y as ark orders fields: Fq by canonical integer, Fq2 by c1 first, then c0
 *   compressed    x with flags -- G1 48 bytes, G2 96.  Infinity: x = 0, bit 6 set, bit 7 clear.  y = sqrt(x^3 + b), b = 4 (G1) or
 *                 4 (1 + u) (G2); no root -> malformed; the greater of y, -y if and only if bit 7 is set
 *   uncompressed  x, then y carrying only the infinity flag -- G1 96 bytes, G2 192.  Infinity: x = y = 0, bit 6 set.  The curve
 *                 equation is checked
 *   proof         A | B | C: 192 bytes compressed, 384 uncompressed
 *   key           alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | le64(n) | gamma_abc_g1[n]: 344 + 48 n bytes compressed, 680 + 96 n uncompressed
 * ONE encoding per point, as x + q is refused for x everywhere above: both flag bits set, infinity with a non-zero coordinate, and bit 7
 * set in an uncompressed point are malformed.  (ark 0.3 is laxer on the last two as far as this restatement goes: it ignores the
 * coordinates of a point flagged infinite and bit 7 of an uncompressed y.)  Subgroup membership is NOT the codec's business: the
 * verifier's own checks make it unless the caller sets FRW_VERIFY_POINTS_ARE_CHECKED, and the key loaders always make it. */
#define FRW_WIRE_COMPRESSED   0
#define FRW_WIRE_UNCOMPRESSED 1
/* bytes of one proof / of a key with num_instance gamma_abc_g1 points; 0 for a bad mode */
size_t frw_groth16_proof_wire_bytes(int mode);
size_t frw_groth16_vk_wire_bytes(size_t num_instance, int mode);
/* HOST codec (no device needed).  proofs: uint64_t[batch][48] as frw_groth16_prove_dev writes them; out / in: batch x
 * frw_groth16_proof_wire_bytes(mode) bytes, any alignment; status: int32_t[batch], 0 or -1 -- encoding: a coordinate's limbs are >= q
 * (nothing else is checked: a point off its curve is encoded as it stands, and compressed it comes back as another point or as
 * malformed); decoding: any malformed case above in any of the three points.  A refused proof's output is all zero bytes / limbs.  The
 * call itself returns FRW_OK; FRW_E_INVALID_ARG for a null pointer or a bad mode. */
int frw_groth16_proofs_to_wire(size_t batch, const uint64_t *proofs, int mode, uint8_t *out, int32_t *status);
int frw_groth16_proofs_from_wire(size_t batch, const uint8_t *in, int mode, uint64_t *proofs, int32_t *status);
/* The same with DEVICE pointers on `device`: stream-ordered on `stream`, allocates nothing, does not synchronise -- capture-safe; bytes,
 * limbs and statuses are bit-equal to the host functions'.  Decoding a compressed proof is four square roots in Fq (one each for A and
 * C, two for B) and an inversion.  No device -> FRW_E_NO_DEVICE (no host fallback). */
int frw_groth16_proofs_to_wire_dev(int device, size_t batch, const uint64_t *d_proofs, int mode, uint8_t *d_out, int32_t *d_status, void *stream);
int frw_groth16_proofs_from_wire_dev(int device, size_t batch, const uint8_t *d_in, int mode, uint64_t *d_proofs, int32_t *d_status, void *stream);
/* frw_groth16_verify_full_dev with the proofs as wire bytes (d_wire: batch x frw_groth16_proof_wire_bytes(mode) bytes in device memory,
 * any alignment): every pass decodes its proofs into the workspace and runs the chain above on them unchanged.  d_accepted[i] = -1 where
 * the decoder refused proof i; otherwise what frw_groth16_verify_full_dev gives for the decoded limbs and the same flags.  Same flags,
 * chunking, refusals and capture-safety as frw_groth16_verify_full_dev; a bad mode -> FRW_E_INVALID_ARG.  FRW_VERIFY_BATCHED: rho_i
 * hashes the DECODED 384 limb bytes of proof i, exactly as frw_groth16_verify_full_dev does -- not the wire bytes -- and a refused proof
 * is left out of the batched check like any other malformed one.
 * Workspace: frw_groth16_verify_wire_workspace_bytes(vk, batch_in_flight, flags, mode) bytes, 16-byte aligned: for k proofs in flight,
 * 384 k bytes of decoded limbs and 4 k of statuses rounded up to 16 on top of frw_groth16_verify_full_workspace_bytes(vk, k, flags)
 * (388 bytes a proof plus padding); 0 for a bad mode or where that function gives 0. */
size_t frw_groth16_verify_wire_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight, int flags, int mode);
int frw_groth16_verify_wire_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_instance, int encoding, const uint8_t *d_wire,
                                int mode, int flags, const uint64_t *seed, int32_t *d_accepted, int32_t *d_batch_passed, void *d_workspace,
                                size_t workspace_bytes, void *stream);
/* Keys.  frw_groth16_vk_to_wire (host): vk in the layout frw_groth16_setup writes -> frw_groth16_vk_wire_bytes(num_instance, mode) bytes;
 * FRW_E_INVALID_ARG (and zero bytes) if a coordinate's limbs are >= q, for num_instance = 0, a null pointer or a bad mode.
 * frw_groth16_vk_load_wire: decodes on the host and goes through frw_groth16_vk_load (every point checked).
 * frw_groth16_vk_load_wire_dev: the four fixed points decoded on the host, gamma_abc_g1 on `device` (a lane per point), then
 * everything frw_groth16_vk_load_dev does -- every point checked, no vouching flag; the handle serves every verifier above.
 * FRW_E_INVALID_ARG for both loaders: a length that is not frw_groth16_vk_wire_bytes(n, mode) for the embedded n (truncated, over-long),
 * n = 0, any malformed point, and whatever the limb loaders refuse.  No device -> FRW_E_NO_DEVICE (_dev only; no host fallback). */
int frw_groth16_vk_to_wire(const uint64_t *vk, size_t num_instance, int mode, uint8_t *out);
int frw_groth16_vk_load_wire(const uint8_t *bytes, size_t len, int mode, frw_groth16_vk **out);
int frw_groth16_vk_load_wire_dev(int device, const uint8_t *bytes, size_t len, int mode, frw_groth16_vk **out);
/* PROVING keys: what ark-groth16 0.3.0's ProvingKey<Bls12_381> is after pk.serialize(&mut file) (FRW_WIRE_COMPRESSED) or
 * pk.serialize_uncompressed(&mut file).  The struct derives CanonicalSerialize, so the bytes are its fields in order:
 *   vk            the VerifyingKey exactly as frw_groth16_vk_to_wire writes it:
 *                 alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | le64(I) | gamma_abc_g1[I]
 *   beta_g1       G1
 *   delta_g1      G1
 *   a_query       le64(len) | G1[len]        len = I + W
 *   b_g1_query    le64(len) | G1[len]        len = I + W
 *   b_g2_query    le64(len) | G2[len]        len = I + W
 *   h_query       le64(len) | G1[len]        len = n - 1
 *   l_query       le64(len) | G1[len]        len = W
 * with the point encodings, flag bits, "greater" rule and strictness of the block above.  Like the rest of that block this layout is
 * restated from the crate's source as recalled and is UNPINNED against ark-groth16: the independent check is a second
 * restatement in Python integers (tests/pk_wire_ref.py), not bytes that the crate wrote.
 * I (the constant one included), W and n are READ FROM THE BYTES: n = len(h_query) + 1 must be a power of two and at least 2, the three
 * I + W lengths must agree with each other, with len(l_query) + I and with the verifying key's I (I >= 1), and the total length must be
 * exactly what those counts imply.  Points at infinity (a variable on no A or B side) load as the all-zero rows the sums skip.
 *   frw_groth16_pk_wire_bytes   the size for (I, W, n); 0 for a bad mode, I = 0, n < 2 or not a power of two, or counts beyond 2^40
 *   frw_groth16_pk_wire_info    HOST only, no device, no point decoded: walks the framing, returns the counts and the byte offset of the
 *                               first point of each of the five runs (after its le64); FRW_E_INVALID_ARG for anything the rules above
 *                               exclude (truncated, over-long, disagreeing lengths, a length field larger than the buffer, ...) --
 *                               nothing beyond `len` is read
 *   frw_groth16_pk_load_wire_dev  `bytes`: host memory, any alignment.  opts: NULL = FRW_KEY_AUTO; FRW_KEY_TABLES / FRW_KEY_BARE are
 *                               honoured; world > 1 -> FRW_E_INVALID_ARG (a key in slices from wire bytes is OUT OF SCOPE: load the whole
 *                               key, or slice limbs with frw_groth16_pk_load_opts).  vk_out (optional): 84 + 12 I uint64_t, the embedded
 *                               verifying key in the layout frw_groth16_setup writes, ready for frw_groth16_vk_load*.  EVERY point of the
 *                               six runs (gamma_abc_g1 and the five queries) is decoded ON THE DEVICE, a lane per point -- canonical
 *                               coordinates, the flag rules, the curve equation or the root -- and, unless flags has
 *                               FRW_PK_POINTS_ARE_CHECKED, tested for membership of the subgroup of order r there too (the 255-bit
 *                               ladder every other loader runs); the seven fixed points are decoded and checked on the host by the same
 *                               code.  The bytes go through a device buffer of FRW_PK_WIRE_CHUNK_BYTES at a time and the decoded limbs
 *                               feed the key's tables in device memory: nothing decoded returns to the host but the verifying key.
 *                               Any malformed point, any point outside its subgroup, any framing error: FRW_E_INVALID_ARG, *pk_out ==
 *                               NULL, and frw_last_error() names the query and the first bad index.  No device -> FRW_E_NO_DEVICE (no
 *                               host fallback).  Allocates and frees its own device memory, takes no workspace, synchronises: NOT
 *                               capture-safe.
 *   FRW_PK_POINTS_ARE_CHECKED   skips the subgroup ladders ONLY; the decoder's checks are never skipped.  UNSAFE for a key the caller
 *                               did not make itself: a query point outside the subgroup makes proofs that leak or fail, and nothing
 *                               downstream notices.  For a file this process wrote a moment ago.
 *   frw_groth16_pk_to_wire_dev  the whole key into HOST memory `out` (out_len must be frw_groth16_pk_wire_bytes of the key's counts).
 *                               vk: the limb layout frw_groth16_setup returns, num_instance = the key's I -- gamma_g2 and gamma_abc_g1
 *                               are taken from it (the handle does not hold them); everything else, alpha_g1, beta_g2 and delta_g2
 *                               included, comes from the handle's own rows (window 0 of a table handle, a bare handle's row; the three
 *                               padding rows of the witness-side tables: frw_groth16_key_opts_t), encoded on the device a lane per row.
 *                               Table and bare keys, made by frw_groth16_setup* or loaded, alike; a slice of a key (world > 1), a wrong
 *                               out_len or num_instance -> FRW_E_INVALID_ARG.  Allocates, synchronises: not capture-safe. */
#define FRW_PK_POINTS_ARE_CHECKED 1
#define FRW_PK_WIRE_CHUNK_BYTES (32u << 20)
typedef struct {
    uint64_t num_instance, num_witness, domain_size;      /* I (with the constant one), W, n */
    uint64_t a_query_offset, b_g1_query_offset, b_g2_query_offset, h_query_offset, l_query_offset;
} frw_groth16_pk_wire_info_t;
size_t frw_groth16_pk_wire_bytes(uint64_t num_instance, uint64_t num_witness, uint64_t domain_size, int mode);
int frw_groth16_pk_wire_info(const uint8_t *bytes, size_t len, int mode, frw_groth16_pk_wire_info_t *out);
int frw_groth16_pk_load_wire_dev(int device, const uint8_t *bytes, size_t len, int mode, int flags, const frw_groth16_key_opts_t *opts,
                                 frw_groth16_pk **pk_out, uint64_t *vk_out);
int frw_groth16_pk_to_wire_dev(const frw_groth16_pk *pk, const uint64_t *vk, size_t num_instance, int mode, uint8_t *out, size_t out_len);
/* diagnostics for the codec's tests: the "greater" test on canonical integers (uint64_t[6] each; c1 NULL: the Fq order of c0, else
 * the Fq2 order, c1 first) -> 1 if y > -y, else 0; FRW_E_INVALID_ARG for a null c0 */
int frw_diag_wire_greater(const uint64_t *c0, const uint64_t *c1);
/* frw_diag_pairing for `count` pairs on `device` (host buffers: g1 count x 12, g2 count x 24, out count x 72 uint64_t, the same basis):
 * the device pairing's kernels, for the parity tests.  Allocates and synchronises.  A point off its curve -> FRW_E_INVALID_ARG; no
 * device -> FRW_E_NO_DEVICE (no host fallback). */
int frw_diag_pairing_dev(int device, size_t count, const uint64_t *g1, const uint64_t *g2, uint64_t *out);

/* ---- re-randomising proofs (frw_rerand.hip): ark-groth16 0.3.0 prover.rs, rerandomize_proof(rng, vk, proof) ---------------------------------
 * Restated from the crate's source (parity unpinned: DESIGN.md 5.11):
 *     A' = r1^-1 A          B' = r1 B + (r1 r2) delta_g2          C' = C + r2 A
 * A proof of the same statement that looks new: whoever holds (vk, proof) -- no signature, no witness, no proving key -- can present it
 * again, or forward it, without the 192 bytes being a stable identifier.  ark draws r1, r2 itself; here the CALLER supplies them, as with
 * the blinding factors of frw_groth16_prove_rs_dev: the new proof is unlinkable to the old one only if the pair is uniform, secret and
 * FRESH -- the same proof with the same pair gives the same bytes.  frw_groth16_rerandomize_seeded_dev / _wire_seeded_dev (below, "drawing
 * the factors on the device") draw the pair themselves, as ark does, from a seed and a counter in device memory.
 *     proofs      uint64_t[batch][48]: A | B | C as frw_groth16_prove_dev writes them.  Each of the three may be the point at infinity
 *                 (all zero): the formulas are defined for it, and so may each result be (written as all zero)
 *     factors     uint64_t[batch][2][4]: r1, r2 of every proof, ANY 256-bit values, taken modulo the group order r
 *     flags       0 or FRW_VERIFY_POINTS_ARE_CHECKED (any other bit -> FRW_E_INVALID_ARG): skips the subgroup ladders of A, B, C.  The
 *                 result for a point vouched for WRONGLY is unspecified -- the G1 multiples are computed through the endomorphism
 *                 phi(P) = lambda P, which holds in the subgroup only -- but the call stays memory-safe and deterministic (some point of the
 *                 curve, status 0)
 *     out         uint64_t[batch][48], affine points in ark-ff's limbs -- one representation per point, so equal across host, device, batch
 *                 size and chunking, bit for bit.  IN PLACE is allowed (out == proofs): a slot is read whole before any of it is written
 *     status      int32_t[batch]: 0 re-randomised; -1 malformed -- exactly what frw_groth16_verify calls malformed in a proof: a coordinate
 *                 >= q, a point off its curve, a point outside its subgroup (and, in the wire form, whatever the decoder refuses);
 *                 FRW_RERAND_ZERO_FACTOR: r1 or r2 is 0 modulo r (of a proof that is not malformed).  A refused slot's output is all
 *                 zero bytes; the call itself returns FRW_OK
 * A slot's output depends on its own proof and factors alone.  batch = 0 is a no-op that returns before anything else is looked at.
 * frw_groth16_rerandomize: HOST code, any handle from frw_groth16_vk_load*, one proof per host thread.  For a single proof it is the
 * faster route: a device call's time is that of its longest chain whatever the batch (DESIGN.md 5.11 has the figures).
 * The factors' arithmetic (r1^-1, r1 r2) is NOT constant-time, on the host or on the device: its branches and trip counts depend on r1, r2.
 * Where an observer of timing is part of the threat, draw the factors and call where that observer is not.
 * The _dev calls: the key must come from frw_groth16_vk_load_dev or frw_groth16_vk_load_wire_dev (they put delta_g2 on the device; any
 * other key -> FRW_E_INVALID_ARG, no device -> FRW_E_NO_DEVICE, no host fallback).  Stream-ordered on `stream` ALONE, nothing is
 * allocated or copied, nothing synchronises: capture-safe, and a captured graph has no parallel branches.  d_workspace:
 * frw_groth16_rerandomize_workspace_bytes(vk, batch_in_flight, wire_mode) bytes, 16-byte aligned -- 1,072 bytes a proof in flight (its
 * sixteen scalar words, A' and C' in XYZZ coordinates, B' likewise), with wire_mode FRW_WIRE_* 392 more (the decoded limbs and the two
 * codec statuses), each piece rounded up to 16; wire_mode -1: the limb form; 0 for a null key, batch_in_flight = 0 or a bad mode.  A
 * workspace smaller than the batch needs runs it in chunks.  FRW_E_INVALID_ARG: a null pointer, a bad flag or mode, a misaligned
 * workspace, one too small for one proof.
 * frw_groth16_rerandomize_wire_dev: d_wire_in, d_wire_out: batch x frw_groth16_proof_wire_bytes(mode) bytes, any alignment; every chunk is
 * decoded into the workspace (frw_groth16_proofs_from_wire_dev's kernels), re-randomised there and encoded
 * (frw_groth16_proofs_to_wire_dev's kernel).  In place is allowed (d_wire_out == d_wire_in). */
#define FRW_RERAND_ZERO_FACTOR (-2)
int frw_groth16_rerandomize(const frw_groth16_vk *vk, size_t batch, const uint64_t *proofs, const uint64_t *factors, int flags, uint64_t *out,
                            int32_t *status);
size_t frw_groth16_rerandomize_workspace_bytes(const frw_groth16_vk *vk, size_t batch_in_flight, int wire_mode);
int frw_groth16_rerandomize_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_proofs, const uint64_t *d_factors, int flags,
                                uint64_t *d_out, int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);
int frw_groth16_rerandomize_wire_dev(const frw_groth16_vk *vk, size_t batch, const uint8_t *d_wire_in, int mode, const uint64_t *d_factors,
                                     int flags, uint8_t *d_wire_out, int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- drawing the factors on the device (frw_drbg.h, frw_drbg.hip): the calls of ark-groth16 0.3.0 that take an `rng` ------------------------
 * create_random_proof draws (r, s) and rerandomize_proof draws (r1, r2); the calls above take them from the caller.  These derive them
 * from a 32-byte SEED and a 64-bit COUNTER, one exactly specified function for host and device:
 *     msg  = "FRW-FR-DRAW-001" (15 ASCII bytes) || tag (1 byte) || seed (32) || le64(counter) || le64(j)          64 bytes
 *     x_j  = int_le(first 64 bytes of SHAKE256(msg)) mod r        r: BLS12-381's group order; canonical, four little-endian uint64_t
 * for element j = 0 .. count - 1 of a call.  512 bits modulo r are within 2^-257 of uniform (256 bits "taken modulo r" are not: 2^256 is
 * some 2.2 r, and some residues would be 1.5 times as likely as others); there is no rejection loop.  tag separates the uses:
 * FRW_DRAW_BLINDING for (r, s), FRW_DRAW_RERANDOMIZE for (r1, r2), any value 0 .. 255 for a caller's own (else FRW_E_INVALID_ARG).
 *     frw_fr_draw      HOST code, no device: out = uint64_t[count][4].  The reference for the device calls, bit for bit, and the way to
 *                      audit or reproduce what a device call used.
 *     frw_fr_draw_dev  the same for (d_seed, *d_counter) in device memory (d_seed: 32 bytes, any alignment; d_counter: one uint64_t) into
 *                      d_out = uint64_t[count][4], then *d_counter += 1, modulo 2^64.  Two launches on `stream` ALONE -- one lane per
 *                      scalar, then one thread that steps the counter once every lane has read it -- nothing allocated, copied or
 *                      synchronised: capture-safe, no parallel branches, and a replayed graph draws with the counter it finds THEN.
 * count = 0 (batch = 0 below) is a no-op that returns FRW_OK before anything else is looked at and does NOT advance the counter.  A null
 * pointer -> FRW_E_INVALID_ARG; no device -> FRW_E_NO_DEVICE (no host fallback for the _dev forms).
 * The three composed calls are ONE draw followed by the existing call, unchanged: frw_groth16_prove_seeded_dev is
 * frw_groth16_prove_rs_dev, frw_groth16_rerandomize_seeded_dev / _wire_seeded_dev are frw_groth16_rerandomize_dev / _wire_dev, with
 * 2 x batch scalars drawn into the CALLER'S d_rs / d_factors (uint64_t[batch][2][4]: slot i gets j = 2 i and j = 2 i + 1) under
 * FRW_DRAW_BLINDING / FRW_DRAW_RERANDOMIZE -- the buffer stays the caller's, who can read back what was used.  Every other argument, the
 * workspace and every result are the wrapped call's.  The wrapped call's refusals come FIRST, and a refused call draws nothing and
 * leaves the counter alone; an accepted one advances it by exactly one, whatever the batch and however many chunks the workspace makes
 * of it.  A zero factor (probability 2^-255) is FRW_RERAND_ZERO_FACTOR for its slot, as above.  Captured into a HIP graph, each replay
 * gives fresh proofs with the host out of the loop (frw_groth16_prove_seeded_dev's capture is frw_groth16_prove_rs_dev's: one chunk).
 * frw_pok_prove_from_bytes_dev, frw_aggregate_prove_from_bytes_dev and frw_groth16_prove_partial_dev have no seeded form: fill their d_rs /
 * rs with frw_fr_draw_dev / frw_fr_draw first.  A key in SLICES needs the same factors on every rank: the same seed, counter and tag.
 * What stays the caller's:
 *   - the seed is SECRET and comes from the operating system's generator; whoever knows (seed, counter) knows every factor drawn from them
 *   - a pair (seed, counter) must NEVER recur under one tag -- not after 2^64 calls, and not after a restart of the process: persist the
 *     counter ahead of its use, or take a new seed on every start
 *   - the draw's reduction and the factors' arithmetic behind it are NOT constant-time (the caveat of the re-randomisation section):
 *     where an observer of timing is part of the threat, draw and call where that observer is not */
#define FRW_DRAW_BLINDING     1   /* (r, s) of create_random_proof */
#define FRW_DRAW_RERANDOMIZE  2   /* (r1, r2) of rerandomize_proof */
int frw_fr_draw(const uint8_t seed[32], uint64_t counter, int tag, size_t count, uint64_t *out);
int frw_fr_draw_dev(int device, const uint8_t *d_seed, uint64_t *d_counter, int tag, size_t count, uint64_t *d_out, void *stream);
int frw_groth16_prove_seeded_dev(const frw_groth16_pk *pk, const frw_r1cs *r, size_t batch, const uint64_t *d_witness,
                                 const uint64_t *d_instance, const uint8_t *d_seed, uint64_t *d_counter, uint64_t *d_rs,
                                 uint64_t *d_proofs, uint32_t *d_num_unsatisfied, void *d_workspace, size_t workspace_bytes, void *stream);
int frw_groth16_rerandomize_seeded_dev(const frw_groth16_vk *vk, size_t batch, const uint64_t *d_proofs, const uint8_t *d_seed,
                                       uint64_t *d_counter, uint64_t *d_factors, int flags, uint64_t *d_out, int32_t *d_status,
                                       void *d_workspace, size_t workspace_bytes, void *stream);
int frw_groth16_rerandomize_wire_seeded_dev(const frw_groth16_vk *vk, size_t batch, const uint8_t *d_wire_in, int mode, const uint8_t *d_seed,
                                            uint64_t *d_counter, uint64_t *d_factors, int flags, uint8_t *d_wire_out, int32_t *d_status,
                                            void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- input preparation (what the reference does with falcon-rust before any gadget runs) ---------------------
 * falcon_ntt.rs:27-28,44: sig_poly = Polynomial::from(&sig), pk_poly = Polynomial::from(&pk),
 * hm = Polynomial::from_hash_of_message(msg, sig.nonce()).  Formats are the Falcon specification's:
 *   public key  FRW_PK_LEN(logn)  = 1 + 14 N / 8 bytes: header 0x00 + logn, N x 14-bit coefficients (big-endian bits)
 *   signature   sig_len bytes (falcon.rs: 666 / 1280, the padded lengths): header 0x30 + logn, 40-byte nonce,
 *               compressed s2 (sign bit, 7 low bits, unary high part), zero padding
 *   hash        SHAKE256(nonce || msg) read as big-endian 16-bit words w, w < 5q accepted as w mod q
 * Messages are one byte blob plus batch+1 NON-DECREASING offsets (message i = msgs[msg_off[i] .. msg_off[i+1]));
 * frw_prepare_inputs returns FRW_E_INVALID_ARG for decreasing offsets, the _dev variant reads such a message as empty
 * and trusts the caller that msg_off[batch] does not exceed the blob.
 * status[i] = FRW_ST_DECODE for a malformed encoding (that signature must not be fed to the witness call). */
#define FRW_NONCE_LEN 40
#define FRW_PK_LEN(logn)  (1 + 14 * (1 << (logn)) / 8)
#define FRW_SIG_LEN(logn) ((logn) == 9 ? 666 : 1280)

int frw_hash_to_point_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_nonces /* batch x 40 */,
                          const uint8_t *d_msgs, const uint64_t *d_msg_off /* batch + 1 */, uint16_t *d_hm, void *stream);
int frw_decode_public_keys_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_pk_bytes, uint16_t *d_pk,
                               int32_t *d_status, void *stream);
int frw_decode_signatures_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_sig_bytes, size_t sig_len,
                              uint16_t *d_sig, uint8_t *d_nonce_out /* batch x 40, may be NULL */, int32_t *d_status,
                              void *stream);
/* host buffers: decode + hash for `batch` (pk, msg, sig) triples -> the three coefficient vectors the witness
 * entry points take.  status[i]: FRW_ST_OK or FRW_ST_DECODE. */
int frw_prepare_inputs(frw_ctx *ctx, int logn, size_t batch, const uint8_t *pk_bytes, const uint8_t *sig_bytes,
                       size_t sig_len, const uint8_t *msgs, const uint64_t *msg_off, uint16_t *sig, uint16_t *pk,
                       uint16_t *hm, int32_t *status);

/* ---- the verifier's statement: public inputs without a signature -------------------------------------------------
 * examples/pok_sig.rs:33-45 builds the public inputs from what a verifier holds -- the public key, and the message hashed with
 * the signature's nonce -- and lifts them into Fr; not knowing the signature is the point of a proof of knowledge.  These calls
 * write instance_assignment, 2 N + 1 field elements per statement, the exact bytes the witness entry points above write to
 * d_instance for the same pk and hm, from those alone: one launch of a kernel that does two mod-q NTTs per statement and
 * writes 33 / 66 KB (Falcon-512 / 1024) where the witness call writes 2.5 - 37 MB besides.
 *     circuit     FRW_CIRCUIT_NTT, FRW_CIRCUIT_DUAL_NTT: [1, NTT(pk), NTT(hm)]; FRW_CIRCUIT_SCHOOLBOOK: [1, pk, hm]
 *     encoding    FRW_ENC_CANONICAL or FRW_ENC_MONTGOMERY (there is no compact form of an instance vector)
 *     d_pk, d_hm  uint16_t[batch][N]
 *     d_instance  uint64_t[batch][2 N + 1][4]
 *     d_status    int32_t[batch]: FRW_ST_OK; FRW_ST_COEFF_RANGE for a pk or hm coefficient >= q (the witness kernels' rule);
 *                 from bytes also FRW_ST_DECODE for a malformed key (its header byte, or a 14-bit coefficient >= q)
 * A refused statement's slot is all zero bytes, its leading one included, never stale memory.  Nothing downstream needs to be
 * told: a zero-filled slot has instance[0] != 1, which frw_groth16_verify and every device verifier above report as -1
 * (malformed).
 * frw_statement_from_bytes_dev: frw_decode_public_keys_dev and frw_hash_to_point_dev into the caller's workspace, then the
 * kernel.  d_pk_bytes: batch x FRW_PK_LEN(logn); d_nonces: batch x FRW_NONCE_LEN (bytes 1 .. 40 of an encoded signature); the
 * messages as for frw_hash_to_point_dev.  d_workspace: frw_statement_workspace_bytes(logn, batch) bytes, 16-byte aligned -- pk
 * and hm as uint16_t[batch][N], each rounded up to 16 bytes, then the key decoder's int32_t[batch] statuses likewise (0 for a bad
 * logn).
 * The _dev forms are stream-ordered on `stream`, allocate nothing and do not synchronise: capture-safe.  The host-buffer forms
 * take host pointers, go through the context's arena 4,096 statements at a time, and with strict != 0 return FRW_E_RANGE if any
 * status is non-zero (the buffers are complete all the same).  batch = 0 is a no-op.  FRW_E_INVALID_ARG, before any device is
 * touched: FRW_ENC_COMPACT or another bad encoding, an unknown circuit, logn outside {9, 10}, a null pointer, a small or
 * misaligned workspace; host forms: decreasing message offsets.
 * frw_aggregate_statement_dev: instance_assignment of an aggregate (frw_r1cs_load_aggregate) -- [1, the public inputs of
 * statement 0, of statement 1, ...] -- from the statements' keys and hashed messages: statement i takes the next unused entry of
 * its parameter set's arrays, exactly as frw_aggregate_assign_dev does (either pair may be NULL if the aggregate has no such
 * statement).  The same bytes as frw_aggregate_assign_dev's d_instance after witness calls on the same inputs, in one launch per
 * parameter set and without a witness.  d_status: int32_t[num_statements], statement order.  The constant one is always
 * written; a refused statement leaves zeros in its 2 N slots (such an instance vector is well formed and verifies against no
 * proof).  ctx and the aggregate must be on the same device. */
int frw_statement_dev(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint16_t *d_pk, const uint16_t *d_hm,
                      int encoding, uint64_t *d_instance, int32_t *d_status, void *stream);
int frw_statement(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint16_t *pk, const uint16_t *hm,
                  int encoding, uint64_t *instance, int32_t *status, int strict);
size_t frw_statement_workspace_bytes(int logn, size_t batch);
int frw_statement_from_bytes_dev(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint8_t *d_pk_bytes,
                                 const uint8_t *d_nonces, const uint8_t *d_msgs, const uint64_t *d_msg_off, int encoding,
                                 uint64_t *d_instance, int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                                 void *stream);
int frw_statement_from_bytes(frw_ctx *ctx, int circuit, int logn, size_t batch, const uint8_t *pk_bytes,
                             const uint8_t *nonces, const uint8_t *msgs, const uint64_t *msg_off, int encoding,
                             uint64_t *instance, int32_t *status, int strict);
int frw_aggregate_statement_dev(const frw_r1cs *aggregate, frw_ctx *ctx, const uint16_t *d_pk_512, const uint16_t *d_hm_512,
                                const uint16_t *d_pk_1024, const uint16_t *d_hm_1024, int encoding, uint64_t *d_instance,
                                int32_t *d_status, void *stream);

/* ---- Falcon verification: batch verdicts without a witness --------------------------------------------------------
 * examples/pok_sig.rs:21 asserts keypair.public_key.verify(msg, &sig) before it builds a circuit.  These calls answer
 * that question for a batch and write nothing else: one status word and, if asked, one 64-bit squared norm per signature --
 * twelve bytes where the witness entry points write 2.5 / 5.1 MB (55 / 110 KB in compact form) to reach the same word.  One
 * kernel, one workgroup per signature: NTT(sig), NTT(pk), their product, one inverse NTT, v = hm - sig*pk, the squared norm
 * of v || sig over centred representatives.  A screen in front of frw_witness_*_dev and frw_groth16_prove_dev, and a plain
 * Falcon batch verifier.
 *     rule        how a coefficient a in [0, q) is centred and how the norm is compared:
 *                 FRW_RULE_CIRCUIT  what the three circuits prove and what the witness kernels report: r = a < 6144 ? a :
 *                                   q - a (is_less_than_6144: a = 6144 counts as 6145); refused when norm >= 34034726 /
 *                                   70265242 (Falcon-512 / 1024).  FRW_ST_OK under this rule: the signature can be proven;
 *                                   any other status: it cannot.  For every input the status word is the one
 *                                   frw_witness_ntt_verify_dev writes for the same (sig, pk, hm).
 *                 FRW_RULE_SPEC     the Falcon specification's Verify: r = a <= 6144 ? a : q - a; refused when norm >
 *                                   beta^2 (the same two numbers).
 *                 The two rules differ in exactly two cases: a norm equal to beta^2 (the specification accepts, the
 *                 circuits do not), and a coefficient equal to 6144 (6144^2 under the specification, 6145^2 under the
 *                 circuits) -- which can only decide a verdict at Falcon-1024, because 6144^2 > beta^2 at Falcon-512.
 *     d_sig, d_pk, d_hm   uint16_t[batch][N]
 *     d_status    int32_t[batch]: FRW_ST_OK, FRW_ST_COEFF_RANGE (a coefficient of sig, pk or hm >= q), FRW_ST_NORM_BOUND; from
 *                 bytes also FRW_ST_DECODE, raised by either decoder.  FRW_ST_DECODE beats FRW_ST_COEFF_RANGE beats
 *                 FRW_ST_NORM_BOUND.
 *     d_norm      (may be NULL) uint64_t[batch]: the squared norm under `rule`; all ones where the signature was refused
 *                 before a norm exists (FRW_ST_DECODE, FRW_ST_COEFF_RANGE); never stale memory.
 * frw_falcon_verify_from_bytes_dev: frw_decode_public_keys_dev, frw_decode_signatures_dev (the nonce goes to the workspace)
 * and frw_hash_to_point_dev into the caller's workspace, then the kernel, which takes the decoders' statuses as verdicts
 * already reached and reads no coefficient of such a signature.  d_pk_bytes: batch x FRW_PK_LEN(logn); d_sig_bytes: batch x
 * sig_len, as for frw_decode_signatures_dev; the messages as for frw_hash_to_point_dev.  d_workspace:
 * frw_falcon_verify_workspace_bytes(logn, batch) bytes, 16-byte aligned -- sig, pk, hm as uint16_t[batch][N], the nonces as
 * batch x 40 bytes, the two decoders' int32_t[batch] statuses, each piece rounded up to 16 bytes (0 for a bad logn).
 * The _dev forms are stream-ordered on `stream`, allocate nothing and do not synchronise: capture-safe.  The host-buffer forms
 * take host pointers, go through the context's arena 16,384 signatures at a time, and with strict != 0 return FRW_E_RANGE if
 * any status is non-zero (the buffers are complete all the same).  batch = 0 is a no-op.  FRW_E_INVALID_ARG, before any device
 * is touched: logn outside {9, 10}, an unknown rule, a null pointer other than d_norm / norm, a small or misaligned workspace,
 * sig_len <= 41; host forms: decreasing message offsets. */
#define FRW_RULE_CIRCUIT 0
#define FRW_RULE_SPEC    1
int frw_falcon_verify_dev(frw_ctx *ctx, int logn, size_t batch, const uint16_t *d_sig, const uint16_t *d_pk,
                          const uint16_t *d_hm, int rule, int32_t *d_status, uint64_t *d_norm, void *stream);
int frw_falcon_verify(frw_ctx *ctx, int logn, size_t batch, const uint16_t *sig, const uint16_t *pk, const uint16_t *hm,
                      int rule, int32_t *status, uint64_t *norm, int strict);
size_t frw_falcon_verify_workspace_bytes(int logn, size_t batch);
int frw_falcon_verify_from_bytes_dev(frw_ctx *ctx, int logn, size_t batch, const uint8_t *d_pk_bytes,
                                     const uint8_t *d_sig_bytes, size_t sig_len, const uint8_t *d_msgs,
                                     const uint64_t *d_msg_off, int rule, int32_t *d_status, uint64_t *d_norm,
                                     void *d_workspace, size_t workspace_bytes, void *stream);
int frw_falcon_verify_from_bytes(frw_ctx *ctx, int logn, size_t batch, const uint8_t *pk_bytes, const uint8_t *sig_bytes,
                                 size_t sig_len, const uint8_t *msgs, const uint64_t *msg_off, int rule, int32_t *status,
                                 uint64_t *norm, int strict);

/* ---- the prover from bytes: encoded Falcon signatures in, Groth16 proofs on the wire out -----------------------------------
 * The prover's half of examples/pok_sig.rs (:21-32 and Proof::serialize) as ONE call: what a caller otherwise chains from
 * frw_prepare_inputs, a screen, frw_witness_*_dev, frw_groth16_prove_rs_dev, frw_groth16_proofs_to_wire_dev and a statement call,
 * with the witness buffers, the compaction of the accepted signatures and the chunking done here.  For a batch, on `stream`:
 *   1. both decoders and SHAKE256 into the workspace, then the Falcon verification kernel under FRW_RULE_CIRCUIT with the
 *      decoders' statuses as verdicts already reached: d_status[i] is exactly the word frw_falcon_verify_from_bytes_dev writes;
 *   2. an order-preserving scan over the statuses lists the accepted slots (any batch: three small launches); every output of every
 *      refused slot is zero-filled;
 *   3. THE ONE HOST WAIT: the number of accepted slots is copied to the host and `stream` is synchronised (hipStreamSynchronize) --
 *      the chunk loop below is a host loop and the witness and prover launches are sized by it.  So the call also waits for
 *      whatever `stream` held before, and like frw_groth16_prove_dev it is NOT stream-capture safe;
 *   4. for each chunk of at most k accepted signatures: their (sig, pk, hm) rows are gathered, the circuit's witness kernel
 *      (FRW_ENC_MONTGOMERY) fills the workspace, then the prover of frw_groth16_prove_rs_dev and the wire encoder run on it, and
 *      a scatter writes every result into its slot.  k = the most proofs in flight the caller's workspace holds (at most 4,096).
 *     circuit, logn   FRW_CIRCUIT_*, 9 | 10: must be what `r` was loaded for, and `pk` a whole key over `r`
 *     d_pk_bytes, d_sig_bytes, sig_len, d_msgs, d_msg_off   as for frw_falcon_verify_from_bytes_dev
 *     d_rs            uint64_t[batch][2][4]: the blinding factors of slot i at d_rs[i], as for frw_groth16_prove_rs_dev (a refused
 *                     slot's are not read)
 *     d_wire          batch x frw_groth16_proof_wire_bytes(wire_mode) bytes, any alignment
 *     d_proofs        (may be NULL) uint64_t[batch][48], the limbs frw_groth16_prove_rs_dev writes
 *     d_instance      (may be NULL) uint64_t[batch][2 N + 1][4], FRW_ENC_MONTGOMERY: the verifier's statement
 *     d_status        int32_t[batch], FRW_ST_*; FRW_ST_OK: the slot holds a proof
 *     d_num_unsatisfied  (may be NULL) uint32_t[batch]: the prover's count of violated rows (0 for every accepted slot)
 *     d_workspace     256-byte aligned, at least frw_pok_prove_workspace_bytes(pk, r, circuit, logn, batch, 1) bytes; with
 *                     (..., batch, in_flight) bytes, in_flight proofs are in flight at a time.  The layout (csrc/frw_layout.h
 *                     pok_prove_layout): a part proportional to batch (the screen's workspace, the index list, the scan's words, the
 *                     count, the dense blinding factors), in_flight times a per-signature part (witness, instance, gathered inputs,
 *                     limbs, wire bytes, status words) and frw_groth16_workspace_bytes(pk, r, in_flight)
 * THE CONTRACT: the bytes written for slot i depend only on slot i's inputs and d_rs[i] -- not on the batch, on which neighbours
 * were refused, or on the workspace's size.  An accepted slot holds byte for byte what the chained calls give for that signature
 * alone with the same (r, s); a refused slot holds zero bytes in every output (a zero instance vector has instance[0] != 1 and
 * zero wire bytes are no encoding of a proof: every verifier above reports -1), never stale memory; nothing beyond `batch` entries
 * of any output is written.
 * A batch with nothing accepted launches no witness or prover kernel and returns FRW_OK.  Allocates nothing.
 * FRW_E_INVALID_ARG before any device work: logn outside {9, 10}, an unknown circuit or wire mode, sig_len <= 41, a null pointer
 * other than d_proofs / d_instance / d_num_unsatisfied, a workspace that is not 256-byte aligned; then batch = 0 is a no-op
 * (FRW_OK; the handles are not looked at); then: circuit / logn that are not the handle's (its I, W, C: frw_r1cs_info), an
 * aggregate handle, a key for another system or in slices (world > 1), ctx, pk and r on different devices, a workspace smaller
 * than that of one proof in flight.  frw_pok_prove_workspace_bytes returns 0 for the same mismatches, for a null handle and for
 * in_flight = 0.
 * frw_pok_prove_from_bytes: the same with HOST pointers for every array (rs, the outputs and the statuses too), through the
 * context's arena 256 slots at a time with up to 8 proofs in flight; decreasing message offsets -> FRW_E_INVALID_ARG; with
 * strict != 0 it returns FRW_E_RANGE if any status is non-zero (all outputs are complete all the same). */
size_t frw_pok_prove_workspace_bytes(const frw_groth16_pk *pk, const frw_r1cs *r, int circuit, int logn, size_t batch,
                                     size_t in_flight);
int frw_pok_prove_from_bytes_dev(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *r, int circuit, int logn, size_t batch,
                                 const uint8_t *d_pk_bytes, const uint8_t *d_sig_bytes, size_t sig_len, const uint8_t *d_msgs,
                                 const uint64_t *d_msg_off, const uint64_t *d_rs, int wire_mode, uint8_t *d_wire,
                                 uint64_t *d_proofs, uint64_t *d_instance, int32_t *d_status, uint32_t *d_num_unsatisfied,
                                 void *d_workspace, size_t workspace_bytes, void *stream);
int frw_pok_prove_from_bytes(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *r, int circuit, int logn, size_t batch,
                             const uint8_t *pk_bytes, const uint8_t *sig_bytes, size_t sig_len, const uint8_t *msgs,
                             const uint64_t *msg_off, const uint64_t *rs, int wire_mode, uint8_t *wire, uint64_t *proofs,
                             uint64_t *instance, int32_t *status, uint32_t *num_unsatisfied, int strict);

/* ---- an aggregate from bytes: encoded Falcon signatures of mixed parameter sets in, verdicts, the verifier's statement, ONE proof out ----
 * Both halves of examples/pok_sig.rs:21-47 for an aggregate handle (frw_r1cs_load_aggregate; its statements are FRW_CIRCUIT_NTT's),
 * from what a caller holds: a list of (pk, msg, sig) in STATEMENT order, Falcon-512 and Falcon-1024 mixed, not two sorted piles.
 *     d_pk_bytes      the encoded keys laid end to end in statement order: statement i takes FRW_PK_LEN(logn[i]) bytes (897 | 1,793), so
 *                     no key but the first is aligned to anything; nothing is assumed of the alignment of any input byte
 *     d_sig_bytes     likewise, FRW_SIG_LEN(logn[i]) bytes each (666 | 1,280)
 *     d_nonces        (the statement call, in place of the signatures) count x FRW_NONCE_LEN bytes, statement order
 *     d_msgs, d_msg_off   one blob and count + 1 non-decreasing offsets in statement order, as for frw_hash_to_point_dev
 * The device code reads every statement's bytes where they lie (csrc/frw_layout.h aggregate_route: k statements of its own set and s - k
 * of the other lie before the k-th statement of a set, statement s) and writes the decoded rows into its parameter set's dense arrays,
 * which the per-set kernels take: one launch per parameter set and stage.
 * frw_aggregate_falcon_verify_from_bytes_dev -- the screen: d_status[i] (int32_t[count]) and d_norm[i] (uint64_t[count], may be NULL) are
 *     word for word what frw_falcon_verify_from_bytes_dev writes for statement i alone under `rule`; FRW_ST_DECODE beats
 *     FRW_ST_COEFF_RANGE beats FRW_ST_NORM_BOUND.  d_workspace: frw_aggregate_screen_workspace_bytes(aggregate) bytes, 16-byte aligned
 *     (csrc/frw_layout.h aggregate_screen_layout).  Stream-ordered, allocates nothing, no host wait: capture-safe.
 * frw_aggregate_statement_from_bytes_dev -- the verifier's half: d_instance (uint64_t[I][4]) holds the bytes frw_aggregate_statement_dev
 *     writes for the decoded keys and the hashed messages of the same inputs, [1, NTT(pk_0), NTT(hm_0), ...].  The constant one is
 *     always written; a refused statement's 2 N slots are zero; d_status (int32_t[count]) is in statement order: FRW_ST_OK, FRW_ST_DECODE
 *     (a malformed key).  The same workspace size and alignment as the screen's.  Capture-safe.
 * frw_aggregate_prove_from_bytes_dev -- the prover's half as ONE call, on `stream`:
 *   1. the routed decoders and SHAKE256, then the screen under FRW_RULE_CIRCUIT: d_status is the screen's;
 *   2. d_instance (may be NULL; FRW_ENC_MONTGOMERY) and d_nonces_out (may be NULL; count x 40: bytes 1 .. 40 of every signature) are
 *      written: d_instance is exactly what frw_aggregate_statement_from_bytes_dev writes for these keys, nonces and messages -- the
 *      verifier's statement, which does not depend on the signatures;
 *   3. THE ONE HOST WAIT: the number of refused statements is copied to the host and `stream` is synchronised, so the call is NOT
 *      stream-capture safe, like frw_pok_prove_from_bytes_dev;
 *   4. if any statement is refused: d_wire (all bytes of the chosen mode) and d_proof are zero-filled, d_num_unsatisfied is all ones, no
 *      witness or prover kernel is launched, and the call returns FRW_E_RANGE -- an aggregate with a statement that cannot be proven has
 *      no proof; d_status says which one;
 *   5. else each parameter set's witness kernel (FRW_ENC_MONTGOMERY), frw_aggregate_assign_dev's copies into the workspace,
 *      frw_groth16_prove_rs_dev on the aggregate handle and the wire encoder; d_num_unsatisfied is the prover's count; FRW_OK.  Every
 *      statement was accepted, so the preconditions of frw_aggregate_assign_dev hold by construction.
 *     d_rs            uint64_t[2][4], as for frw_groth16_prove_rs_dev        d_wire   frw_groth16_proof_wire_bytes(wire_mode) bytes
 *     d_proof         (may be NULL) uint64_t[48]                              d_num_unsatisfied  (may be NULL) uint32_t[1]
 *     d_workspace     frw_aggregate_prove_workspace_bytes(pk, aggregate) bytes, 256-byte aligned (csrc/frw_layout.h aggregate_prove_layout:
 *                     the screen's pieces, the per-set witness and instance batches, the aggregate's vectors, limbs, wire bytes, status
 *                     words and frw_groth16_workspace_bytes(pk, aggregate, 1))
 * The proof's bytes depend only on the statements' inputs and d_rs, and are byte for byte what the chain of frw_prepare_inputs,
 * frw_witness_ntt_verify_dev, frw_aggregate_assign_dev, frw_groth16_prove_rs_dev and frw_groth16_proofs_to_wire_dev gives.  Nothing is
 * written beyond the stated sizes; nothing is left as stale memory.  Allocates nothing.
 * FRW_E_INVALID_ARG before any device work: a null pointer other than the ones marked, a handle that is not an aggregate, an unknown
 * rule, encoding (FRW_ENC_COMPACT too) or wire mode, a misaligned or small workspace, ctx, key and handle on different devices; a key
 * in slices (world > 1) or whose instance and witness counts are not the handle's.  The size functions return 0 for the same.
 * What the call CANNOT check: a key made for the same multiset of statements in another order has the same counts.  Pairing the key
 * with the handle it was set up from is the caller's responsibility (the proof of a mismatched pair verifies against nothing).
 * The host-buffer forms (no _dev) take the same arguments as host pointers and no workspace; an aggregate is not divisible, so each is
 * ONE pass through the context's arena (FRW_E_OUT_OF_MEMORY if the arena cannot hold the statement); decreasing message offsets ->
 * FRW_E_INVALID_ARG.  frw_aggregate_prove_from_bytes returns FRW_E_RANGE as the device form does, with every output complete. */
size_t frw_aggregate_screen_workspace_bytes(const frw_r1cs *aggregate);
int frw_aggregate_falcon_verify_from_bytes_dev(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *d_pk_bytes,
                                               const uint8_t *d_sig_bytes, const uint8_t *d_msgs, const uint64_t *d_msg_off, int rule,
                                               int32_t *d_status, uint64_t *d_norm, void *d_workspace, size_t workspace_bytes,
                                               void *stream);
int frw_aggregate_statement_from_bytes_dev(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *d_pk_bytes, const uint8_t *d_nonces,
                                           const uint8_t *d_msgs, const uint64_t *d_msg_off, int encoding, uint64_t *d_instance,
                                           int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);
size_t frw_aggregate_prove_workspace_bytes(const frw_groth16_pk *pk, const frw_r1cs *aggregate);
int frw_aggregate_prove_from_bytes_dev(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *aggregate, const uint8_t *d_pk_bytes,
                                       const uint8_t *d_sig_bytes, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint64_t *d_rs,
                                       int wire_mode, uint8_t *d_wire, uint64_t *d_proof, uint64_t *d_instance, uint8_t *d_nonces_out,
                                       int32_t *d_status, uint32_t *d_num_unsatisfied, void *d_workspace, size_t workspace_bytes,
                                       void *stream);
int frw_aggregate_falcon_verify_from_bytes(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *pk_bytes, const uint8_t *sig_bytes,
                                           const uint8_t *msgs, const uint64_t *msg_off, int rule, int32_t *status, uint64_t *norm);
int frw_aggregate_statement_from_bytes(const frw_r1cs *aggregate, frw_ctx *ctx, const uint8_t *pk_bytes, const uint8_t *nonces,
                                       const uint8_t *msgs, const uint64_t *msg_off, int encoding, uint64_t *instance, int32_t *status);
int frw_aggregate_prove_from_bytes(frw_ctx *ctx, const frw_groth16_pk *pk, const frw_r1cs *aggregate, const uint8_t *pk_bytes,
                                   const uint8_t *sig_bytes, const uint8_t *msgs, const uint64_t *msg_off, const uint64_t *rs,
                                   int wire_mode, uint8_t *wire, uint64_t *proof, uint64_t *instance, uint8_t *nonces_out,
                                   int32_t *status, uint32_t *num_unsatisfied);

/* ---- stand-alone gadget blocks ---------------------------------------------------------------
 * The reference's gadget functions are also called outside the full circuit (its unit tests do; so can any
 * other circuit built from them).  One call fills the witness block of `count` independent gadget invocations,
 * `frw_gadget_block_len(kind)` field elements each, in the order the gadget allocates them:
 *   FRW_G_LESS_THAN_Q     enforce_less_than_q(a)            range_proofs.rs:42-94     a: uint64_t[count]            27
 *   FRW_G_MOD_Q           mod_q(a, q) -> [t, b, ltq(b)]     arithmetics.rs:105-149    a: uint32_t[count][5] (LE limbs, a < 2^160)  29
 *   FRW_G_ADD_MOD         add_mod(a, b, q) -> [t, c, ltq(c)] arithmetics.rs:214-262   a, b: uint64_t[count], a+b < 2^64  29
 *   FRW_G_L2_ELEM         one l2_norm_var element -> [a0..a13, w0, w1, r, sq]  misc.rs:35-47, range_proofs.rs:289-333
 *                                                                                     a: uint64_t[count], a <= q     18
 *   FRW_G_NORM_BOUND_512  enforce_less_than_norm_bound      range_proofs.rs:100-186   a: uint64_t[count]            50
 *   FRW_G_NORM_BOUND_1024                                   range_proofs.rs:192-272   a: uint64_t[count]            52
 * As in the reference, bit decompositions take the LOW bits of the value (to_bits_le().take(k)); a value that does
 * not fit yields the block the reference's cfg(test) build assigns (an unsatisfied system), not an error.
 * status[i] = FRW_ST_COEFF_RANGE only where the input is outside the documented domain.  b is ignored (may be NULL)
 * unless kind == FRW_G_ADD_MOD. */
#define FRW_G_LESS_THAN_Q       0
#define FRW_G_MOD_Q             1
#define FRW_G_ADD_MOD           2
#define FRW_G_L2_ELEM           3
#define FRW_G_NORM_BOUND_512    4
#define FRW_G_NORM_BOUND_1024   5

int frw_gadget_block_len(int kind);   /* elements per block, or FRW_E_INVALID_ARG */
int frw_gadget_dev(frw_ctx *ctx, int kind, size_t count, const void *d_a, const uint64_t *d_b, int encoding,
                   uint64_t *d_out, int32_t *d_status, void *stream);
int frw_gadget(frw_ctx *ctx, int kind, size_t count, const void *a, const uint64_t *b, int encoding,
               uint64_t *out, int32_t *status);

/* ---- utilities ---------------------------------------------------------------------------- */
/* Per-item digest of a device buffer of `items` x `words_per_item` uint64_t:
 * d_out[i] = sum_j splitmix64(buf[i][j] + j * 0x9E3779B97F4A7C15) mod 2^64.
 * Lets a host compare whole HBM-resident witness batches without copying them back. */
int frw_digest_dev(frw_ctx *ctx, const uint64_t *d_buf, size_t words_per_item, size_t items,
                   uint64_t *d_out, void *stream);

/* What a witness launch of `batch` signatures looks like on this device: out = {workgroups launched, resident
 * workgroups per CU the grid was sized for, CUs, number of signatures (the ragged tail beyond the last full round of
 * the grid, or a whole small batch) that are cut into five work items each}.  Launches whose batch is a multiple of
 * out[0] run fastest (static striding, no tail). */
int frw_diag_launch_shape(frw_ctx *ctx, int logn, int encoding, size_t batch, int32_t out[4]);

/* Roofline calibration: overwrites d_buf[0, bytes) with a compute-free write stream of the witness kernel's store
 * shape (workgroup-contiguous slabs of slab_bytes, 16 B per lane).  Timed by bench.py on the same device and
 * stream as the witness kernel to report the write bandwidth the device's HBM actually sustains. */
int frw_diag_write_stream_dev(frw_ctx *ctx, void *d_buf, size_t bytes, size_t slab_bytes, void *stream);

/* Synthetic, always-valid inputs (host side; stands where the reference's tests call
 * KeyPair::keygen + sign, falcon_ntt.rs:134-138): sig, v ~ rounded Gaussian(sigma_logn),
 * pk uniform in [0,q), hm := v + sig*pk mod (x^N+1, q); triples whose norm reaches the bound are
 * redrawn.  Counter-based: triple i depends only on (seed, first_index + i). */
int frw_synth_triples(int logn, size_t batch, uint64_t seed, uint64_t first_index,
                      uint16_t *sig, uint16_t *pk, uint16_t *hm);

/* Issue rates of the vector instructions a BLS12-381 Fr product is built from, measured on this device (what the QAP
 * transforms' roofline is priced with; bench.py): out[0] = v_add_u32, out[1] = v_mad_u64_u32, both in wave-instructions
 * per SIMD per microsecond with four waves per SIMD; out[2] = field products per second of the bare multiplier loop
 * (frw_fr29.h f29_mul, no loads, no butterflies) over the whole chip; out[3] = number of SIMDs.  Synchronous, ~10 ms. */
int frw_diag_valu_rates(frw_ctx *ctx, double out[4]);

/* p(t) on the device for a polynomial in device memory: d_coeffs uint64_t[n][4] (ark-ff's Montgomery form, coefficient k at index k -- an
 * h of frw_qap_witness_map_dev), t host, canonical; out: host uint64_t[4], canonical.  For checks such as h_acc == (h(t) zt / delta) G1 on
 * domains of 2^27 coefficients.  Synchronous; allocates its own small scratch. */
int frw_diag_poly_eval_dev(int device, uint64_t n, const uint64_t *d_coeffs, const uint64_t *t, uint64_t *out);

/* What the four witness-side sums of a key of BARE handles add up for the scalars d_z (device, uint64_t[rows of this key's slice][4],
 * Montgomery: z ++ [1, r, s] from row z_lo on): out[0] = the rows in which b_g1_query / b_g2_query hold a point (a variable that no
 * constraint has on its B side has the point at infinity there, and the sums over those two tables skip it: frw_groth16_pk.b_index);
 * out[1], out[2] = non-zero 8-bit digits of the scalars that are not one, and scalars equal to one, over all rows (a_query, l_query);
 * out[3], out[4] = the same over the rows of out[0] (b_g1_query, b_g2_query).  One point addition each.  The benchmark prices the
 * aggregate proof's roofline with these.  d_workspace: 256-byte aligned, frw_groth16_workspace_bytes(pk, r, 1) is enough.  Synchronous. */
int frw_diag_groth16_side_counts(const frw_groth16_pk *pk, const uint64_t *d_z, void *d_workspace, size_t workspace_bytes, void *stream,
                                 uint64_t *out);

/* Page-locked host memory.  Output buffers of the host-buffer entry points allocated here are filled by
 * asynchronous DMA that overlaps with the kernels of the next chunk (pageable buffers work too, slower). */
int frw_host_alloc(frw_ctx *ctx, size_t bytes, void **ptr);
int frw_host_free(frw_ctx *ctx /* may be NULL */, void *ptr);

/* thin wrappers so that a host without a HIP binding can own device memory */
int frw_malloc(frw_ctx *ctx, size_t bytes, void **d_ptr);
int frw_free(frw_ctx *ctx, void *d_ptr);
int frw_memcpy_h2d(frw_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int frw_memcpy_d2h(frw_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int frw_synchronize(frw_ctx *ctx, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRW_H */
