//! Raw bindings of `include/frw.h`, one declaration per exported function, same order as the header.
//! Checked against the header by `tests/test_rust_binding.py` (names and parameter counts).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const FRW_OK: c_int = 0;
pub const FRW_E_INVALID_ARG: c_int = -1;
pub const FRW_E_NO_DEVICE: c_int = -2;
pub const FRW_E_HIP: c_int = -3;
pub const FRW_E_OUT_OF_MEMORY: c_int = -4;
pub const FRW_E_RANGE: c_int = -5;

pub const FRW_ENC_CANONICAL: c_int = 0;
/// x * 2^256 mod p: the in-memory limbs of `ark_ff::Fp256` (ark-ff 0.3)
pub const FRW_ENC_MONTGOMERY: c_int = 1;
pub const FRW_ENC_COMPACT: c_int = 2;

pub const FRW_ST_OK: i32 = 0;
pub const FRW_ST_COEFF_RANGE: i32 = 1;
pub const FRW_ST_NORM_BOUND: i32 = 2;
pub const FRW_ST_DECODE: i32 = 3;

pub const FRW_CIRCUIT_NTT: c_int = 0;
pub const FRW_CIRCUIT_DUAL_NTT: c_int = 1;
pub const FRW_CIRCUIT_SCHOOLBOOK: c_int = 2;
pub const FRW_RULE_CIRCUIT: c_int = 0;
pub const FRW_RULE_SPEC: c_int = 1;
pub const FRW_NONCE_LEN: usize = 40;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_layout_t {
    pub logn: i32,
    pub n: i32,
    pub num_witness: i32,
    pub num_instance: i32,
    pub num_constraints: i32,
    pub seg_off: [i32; 8],
    pub seg_len: [i32; 8],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_layout_schoolbook_t {
    pub logn: i32,
    pub n: i32,
    pub num_witness: i32,
    pub num_instance: i32,
    pub num_constraints: i32,
    pub column_len: i32,
    pub seg_off: [i32; 5],
    pub seg_len: [i32; 5],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_layout_dual_t {
    pub logn: i32,
    pub n: i32,
    pub num_witness: i32,
    pub num_instance: i32,
    pub num_constraints: i32,
    pub seg_off: [i32; 15],
    pub seg_len: [i32; 15],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_compact_layout_t {
    pub logn: i32,
    pub n: i32,
    pub bytes_per_signature: u64,
    pub small_off: u64,
    pub num_small: u64,
    pub t_off: u64,
    pub num_t: u64,
    pub bits_off: u64,
    pub num_bit_words: u64,
    pub bit_seg_off: [u64; 6],
    pub instance_off: u64,
    pub num_instance_values: u64,
    pub status_off: u64,
}

/// encodings 16 .. 16 + FRW_MAX_FIELDS - 1: a field registered on the context (`frw_ctx_field_encoding`)
pub const FRW_ENC_FIELD_BASE: c_int = 16;
pub const FRW_MAX_FIELDS: c_int = 8;
/// `frw_msmf_load`: the bases are known to be on the curve
pub const FRW_MSMF_POINTS_ARE_CHECKED: c_int = 1;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_field_info_t {
    pub modulus: [u64; 4],
    pub one: [u64; 4],
    pub r2: [u64; 4],
    pub ninv32: u32,
    pub bits: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_msm_info_t {
    pub num_points: u64,
    pub window_bits: i32,
    pub num_windows: i32,
    pub table_bytes: u64,
    pub workspace_bytes_per_signature: u64,
}

#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct frw_r1cs_info_t {
    pub num_statements: u64,
    pub count_logn9: u64,
    pub count_logn10: u64,
    pub num_instance: u64,
    pub num_witness: u64,
    pub num_constraints: u64,
    pub log_domain_size: i32,
    pub witness_map_on_device: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_r1csf_info_t {
    pub modulus: [u64; 4],
    pub num_instance: u64,
    pub num_witness: u64,
    pub num_constraints: u64,
    pub nnz: [u64; 3],
    pub scratch_bytes_per_statement: [u64; 2],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_fft_field_info_t {
    pub modulus: [u64; 4],
    pub generator: [u64; 4],
    pub two_adicity: u32,
    pub reserved: u32,
    pub two_adic_root: [u64; 4],
    pub two_adic_root_mont: [u64; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_qapf_domain_t {
    pub log_size: u32,
    pub reserved: u32,
    pub size: u64,
    pub group_gen: [u64; 4],
    pub group_gen_inv: [u64; 4],
    pub size_inv: [u64; 4],
    pub generator_inv: [u64; 4],
    pub vanishing_inv: [u64; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_qapf_info_t {
    pub domain: frw_qapf_domain_t,
    pub num_constraints: u64,
    pub num_instance: u64,
    pub num_passes: u32,
    pub reserved: u32,
    pub workspace_bytes_per_statement: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_curve_t {
    pub base_modulus: [u64; 4],
    pub scalar_modulus: [u64; 4],
    pub b: [u64; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_curve_info_t {
    pub base_bits: u32,
    pub scalar_bits: u32,
    pub b_mont: [u64; 4],
    pub one_mont: [u64; 4],
    pub scalar_one_mont: [u64; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_msmf_info_t {
    pub num_points: u64,
    pub window_bits: u32,
    pub num_windows: u32,
    pub reserved: u64,
    pub bases_bytes: u64,
    pub workspace_bytes_per_statement: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_curve2_t {
    pub base_modulus: [u64; 4],
    pub scalar_modulus: [u64; 4],
    pub nonresidue: [u64; 4],
    /// c0 then c1, canonical
    pub b: [u64; 8],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_curve2_info_t {
    pub base_bits: u32,
    pub scalar_bits: u32,
    pub b_mont: [u64; 8],
    pub one_mont: [u64; 4],
    pub nonresidue_mont: [u64; 4],
    pub scalar_one_mont: [u64; 4],
    pub nonresidue_is_minus_one: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_msmf2_info_t {
    pub num_points: u64,
    pub window_bits: u32,
    pub num_windows: u32,
    pub reserved: u64,
    pub bases_bytes: u64,
    pub workspace_bytes_per_statement: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct frw_qap_info_t {
    pub log_domain_size: i32,
    pub domain_size: u64,
    pub num_constraints: u64,
    pub num_instance: u64,
    pub workspace_bytes_per_signature: u64,
}

#[repr(C)]
pub struct frw_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_r1cs {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_r1csf {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_qapf {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_msmf {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_msmf2 {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_msm {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_groth16_pk {
    _private: [u8; 0],
}
#[repr(C)]
pub struct frw_groth16_vk {
    _private: [u8; 0],
}
pub const FRW_VERIFY_POINTS_ARE_CHECKED: c_int = 1;
pub const FRW_VERIFY_BATCHED: c_int = 2;
pub const FRW_WIRE_COMPRESSED: c_int = 0;
pub const FRW_WIRE_UNCOMPRESSED: c_int = 1;
pub const FRW_RERAND_ZERO_FACTOR: c_int = -2;
pub const FRW_DRAW_BLINDING: c_int = 1;
pub const FRW_DRAW_RERANDOMIZE: c_int = 2;
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct frw_groth16_pk_desc_t {
    pub num_instance: u64,
    pub num_witness: u64,
    pub domain_size: u64,
    pub alpha_g1: *const u64,
    pub beta_g1: *const u64,
    pub delta_g1: *const u64,
    pub beta_g2: *const u64,
    pub delta_g2: *const u64,
    pub a_query: *const u64,
    pub b_g1_query: *const u64,
    pub b_g2_query: *const u64,
    pub h_query: *const u64,
    pub l_query: *const u64,
}
/// round 5: keys beyond what window tables can hold (the points only), and keys in slices (frw.h FRW_KEY_*)
pub const FRW_KEY_AUTO: i32 = 0;
pub const FRW_KEY_TABLES: i32 = 1;
pub const FRW_KEY_BARE: i32 = 2;
pub const FRW_GROTH16_PARTIAL_WORDS: usize = 72;
pub const FRW_GROTH16_COMBINE_WORKSPACE: usize = 4096;
pub const FRW_VK_POINTS_ARE_CHECKED: c_int = 1;
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct frw_groth16_key_opts_t {
    pub mode: i32,
    pub rank: u32,
    pub world: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct frw_groth16_pk_info_t {
    pub mode: i32,
    pub rank: u32,
    pub world: u32,
    pub z_lo: u64,
    pub z_hi: u64,
    pub h_lo: u64,
    pub h_hi: u64,
    pub key_bytes: u64,
}
/// the subgroup ladders of frw_groth16_pk_load_wire_dev are skipped (the decoder's checks never are): unsafe for a key the caller did not make
pub const FRW_PK_POINTS_ARE_CHECKED: c_int = 1;
pub const FRW_PK_WIRE_CHUNK_BYTES: u32 = 32 << 20;
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct frw_groth16_pk_wire_info_t {
    pub num_instance: u64,
    pub num_witness: u64,
    pub domain_size: u64,
    pub a_query_offset: u64,
    pub b_g1_query_offset: u64,
    pub b_g2_query_offset: u64,
    pub h_query_offset: u64,
    pub l_query_offset: u64,
}

extern "C" {
    pub fn frw_layout(logn: c_int, out: *mut frw_layout_t) -> c_int;
    pub fn frw_strerror(code: c_int) -> *const c_char;
    pub fn frw_last_error() -> *const c_char;
    pub fn frw_device_count() -> c_int;
    pub fn frw_ctx_create(device: c_int, out: *mut *mut frw_ctx) -> c_int;
    pub fn frw_ctx_destroy(ctx: *mut frw_ctx);
    pub fn frw_witness_ntt_verify_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_sig: *const u16, d_pk: *const u16,
                                      d_hm: *const u16, encoding: c_int, d_witness: *mut u64, d_instance: *mut u64,
                                      d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_ntt_modq_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_poly: *const u16, encoding: c_int,
                            d_witness: *mut u64, d_ntt_out: *mut u16, d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_witness_ntt_verify(ctx: *mut frw_ctx, logn: c_int, batch: usize, sig: *const u16, pk: *const u16,
                                  hm: *const u16, encoding: c_int, witness: *mut u64, instance: *mut u64,
                                  status: *mut i32, strict: c_int) -> c_int;
    pub fn frw_ntt_modq(ctx: *mut frw_ctx, logn: c_int, batch: usize, poly: *const u16, encoding: c_int,
                        witness: *mut u64, ntt_out: *mut u16, status: *mut i32) -> c_int;
    pub fn frw_diag_host_allocations(ctx: *mut frw_ctx, count: *mut u64) -> c_int;
    pub fn frw_ctx_trim(ctx: *mut frw_ctx) -> c_int;
    pub fn frw_diag_valu_rates(ctx: *mut frw_ctx, out: *mut f64) -> c_int;
    pub fn frw_compact_layout(logn: c_int, out: *mut frw_compact_layout_t) -> c_int;
    pub fn frw_witness_ntt_verify_compact_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_sig: *const u16,
                                              d_pk: *const u16, d_hm: *const u16, d_compact: *mut c_void,
                                              d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_expand_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_compact: *const c_void, d_witness: *mut u64,
                          d_instance: *mut u64, stream: *mut c_void) -> c_int;
    pub fn frw_expand_host(logn: c_int, batch: usize, compact: *const c_void, witness: *mut u64,
                           instance: *mut u64) -> c_int;
    pub fn frw_field_info(modulus: *const u64, out: *mut frw_field_info_t) -> c_int;
    pub fn frw_ctx_field_encoding(ctx: *mut frw_ctx, modulus: *const u64, encoding: *mut c_int) -> c_int;
    pub fn frw_expand_field_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_compact: *const c_void, encoding: c_int,
                                d_witness: *mut u64, d_instance: *mut u64, stream: *mut c_void) -> c_int;
    pub fn frw_expand_field_host(modulus: *const u64, logn: c_int, batch: usize, compact: *const c_void, witness: *mut u64,
                                 instance: *mut u64) -> c_int;
    pub fn frw_layout_dual(logn: c_int, out: *mut frw_layout_dual_t) -> c_int;
    pub fn frw_witness_dual_ntt_verify_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_sig: *const u16,
                                           d_pk: *const u16, d_hm: *const u16, encoding: c_int, d_witness: *mut u64,
                                           d_instance: *mut u64, d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_witness_dual_ntt_verify(ctx: *mut frw_ctx, logn: c_int, batch: usize, sig: *const u16, pk: *const u16,
                                       hm: *const u16, encoding: c_int, witness: *mut u64, instance: *mut u64,
                                       status: *mut i32, strict: c_int) -> c_int;
    pub fn frw_layout_schoolbook(logn: c_int, out: *mut frw_layout_schoolbook_t) -> c_int;
    pub fn frw_witness_schoolbook_verify_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_sig: *const u16,
                                             d_pk: *const u16, d_hm: *const u16, encoding: c_int, d_witness: *mut u64,
                                             d_instance: *mut u64, d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_witness_schoolbook_verify(ctx: *mut frw_ctx, logn: c_int, batch: usize, sig: *const u16, pk: *const u16,
                                         hm: *const u16, encoding: c_int, witness: *mut u64, instance: *mut u64,
                                         status: *mut i32, strict: c_int) -> c_int;
    pub fn frw_r1cs_export(circuit: c_int, logn: c_int, path: *const c_char, counts: *mut u64) -> c_int;
    pub fn frw_r1cs_load(device: c_int, circuit: c_int, logn: c_int, out: *mut *mut frw_r1cs) -> c_int;
    pub fn frw_r1cs_load_csr(device: c_int, counts: *const u64, row_ptr: *const *const u64, col: *const *const u32, val: *const *const u64, out: *mut *mut frw_r1cs) -> c_int;
    pub fn frw_r1cs_load_file(device: c_int, path: *const c_char, out: *mut *mut frw_r1cs) -> c_int;
    pub fn frw_r1cs_free(r: *mut frw_r1cs);
    pub fn frw_r1cs_export_field(circuit: c_int, logn: c_int, modulus: *const u64, path: *const c_char, counts: *mut u64) -> c_int;
    pub fn frw_r1csf_load(device: c_int, circuit: c_int, logn: c_int, modulus: *const u64, out: *mut *mut frw_r1csf) -> c_int;
    pub fn frw_r1csf_load_csr(device: c_int, modulus: *const u64, counts: *const u64, row_ptr: *const *const u64, col: *const *const u32,
                              val: *const *const u64, out: *mut *mut frw_r1csf) -> c_int;
    pub fn frw_r1csf_load_file(device: c_int, modulus: *const u64, path: *const c_char, out: *mut *mut frw_r1csf) -> c_int;
    pub fn frw_r1csf_free(r: *mut frw_r1csf);
    pub fn frw_r1csf_info(r: *const frw_r1csf, out: *mut frw_r1csf_info_t) -> c_int;
    pub fn frw_r1csf_scratch_bytes(r: *const frw_r1csf, batch: usize, with_products: c_int) -> usize;
    pub fn frw_r1csf_check_dev(r: *const frw_r1csf, batch: usize, d_witness: *const u64, d_instance: *const u64,
                               d_num_unsatisfied: *mut u32, d_first_unsatisfied: *mut u32, d_abc: *mut u64, d_scratch: *mut c_void,
                               scratch_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_fft_field_info(modulus: *const u64, generator: *const u64, out: *mut frw_fft_field_info_t) -> c_int;
    pub fn frw_qapf_domain(modulus: *const u64, generator: *const u64, num_constraints: u64, num_instance: u64,
                           out: *mut frw_qapf_domain_t) -> c_int;
    pub fn frw_qapf_create(r: *const frw_r1csf, generator: *const u64, out: *mut *mut frw_qapf) -> c_int;
    pub fn frw_qapf_free(q: *mut frw_qapf);
    pub fn frw_qapf_info(q: *const frw_qapf, out: *mut frw_qapf_info_t) -> c_int;
    pub fn frw_qapf_witness_map_dev(q: *const frw_qapf, batch: usize, d_witness: *const u64, d_instance: *const u64, d_h: *mut u64,
                                    d_num_unsatisfied: *mut u32, d_workspace: *mut c_void, workspace_bytes: usize,
                                    stream: *mut c_void) -> c_int;
    pub fn frw_curve_info(c: *const frw_curve_t, out: *mut frw_curve_info_t) -> c_int;
    pub fn frw_curve_check_points(c: *const frw_curve_t, count: usize, points: *const u64, first_bad: *mut i64) -> c_int;
    pub fn frw_curve_scalar_mul(c: *const frw_curve_t, count: usize, points: *const u64, scalars: *const u64, out: *mut u64) -> c_int;
    pub fn frw_msmf_load(device: c_int, c: *const frw_curve_t, num_points: usize, bases: *const u64, flags: c_int,
                         out: *mut *mut frw_msmf) -> c_int;
    pub fn frw_msmf_free(m: *mut frw_msmf);
    pub fn frw_msmf_info(m: *const frw_msmf, out: *mut frw_msmf_info_t) -> c_int;
    pub fn frw_msmf_workspace_bytes(m: *const frw_msmf, batch_in_flight: usize) -> usize;
    pub fn frw_msmf_dev(m: *const frw_msmf, batch: usize, d_scalars: *const u64, scalar_stride: usize, num_scalars: usize,
                        montgomery: c_int, d_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_curve2_info(c: *const frw_curve2_t, out: *mut frw_curve2_info_t) -> c_int;
    pub fn frw_curve2_check_points(c: *const frw_curve2_t, count: usize, points: *const u64, first_bad: *mut i64) -> c_int;
    pub fn frw_curve2_scalar_mul(c: *const frw_curve2_t, count: usize, points: *const u64, scalars: *const u64, out: *mut u64) -> c_int;
    pub fn frw_msmf2_load(device: c_int, c: *const frw_curve2_t, num_points: usize, bases: *const u64, flags: c_int,
                          out: *mut *mut frw_msmf2) -> c_int;
    pub fn frw_msmf2_free(m: *mut frw_msmf2);
    pub fn frw_msmf2_info(m: *const frw_msmf2, out: *mut frw_msmf2_info_t) -> c_int;
    pub fn frw_msmf2_workspace_bytes(m: *const frw_msmf2, batch_in_flight: usize) -> usize;
    pub fn frw_msmf2_dev(m: *const frw_msmf2, batch: usize, d_scalars: *const u64, scalar_stride: usize, num_scalars: usize,
                         montgomery: c_int, d_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_r1cs_load_aggregate(device: c_int, count: usize, logn: *const i32, out: *mut *mut frw_r1cs) -> c_int;
    pub fn frw_r1cs_info(r: *const frw_r1cs, out: *mut frw_r1cs_info_t) -> c_int;
    pub fn frw_aggregate_assign_dev(aggregate: *const frw_r1cs, d_witness_512: *const u64, d_instance_512: *const u64,
                                    d_witness_1024: *const u64, d_instance_1024: *const u64, d_witness: *mut u64,
                                    d_instance: *mut u64, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_setup_r1cs(r: *const frw_r1cs, toxic: *const u64, pk_out: *mut *mut frw_groth16_pk,
                                  vk_out: *mut u64) -> c_int;
    pub fn frw_r1cs_check_dev(r: *const frw_r1cs, batch: usize, d_witness: *const u64, d_instance: *const u64,
                              d_num_unsatisfied: *mut u32, stream: *mut c_void) -> c_int;
    pub fn frw_r1cs_eval_dev(r: *const frw_r1cs, batch: usize, d_witness: *const u64, d_instance: *const u64,
                             d_num_unsatisfied: *mut u32, d_abc: *mut u64, stream: *mut c_void) -> c_int;
    pub fn frw_r1cs_eval_scratch_bytes(r: *const frw_r1cs, batch: usize, with_products: c_int) -> usize;
    pub fn frw_r1cs_eval_scratch_dev(r: *const frw_r1cs, batch: usize, d_witness: *const u64, d_instance: *const u64,
                                     d_num_unsatisfied: *mut u32, d_abc: *mut u64, d_scratch: *mut c_void,
                                     scratch_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_qap_info(r: *const frw_r1cs, out: *mut frw_qap_info_t) -> c_int;
    pub fn frw_qap_witness_map_dev(r: *const frw_r1cs, batch: usize, d_witness: *const u64, d_instance: *const u64,
                                   d_h: *mut u64, d_num_unsatisfied: *mut u32, d_workspace: *mut c_void,
                                   workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_qap_quotient_dev(r: *const frw_r1cs, batch: usize, d_witness: *const u64, d_instance: *const u64,
                                d_h: *mut u64, d_num_unsatisfied: *mut u32, d_workspace: *mut c_void, workspace_bytes: usize,
                                stream: *mut c_void) -> c_int;
    pub fn frw_qap_witness_map(r: *const frw_r1cs, batch: usize, witness: *const u64, instance: *const u64, h: *mut u64,
                               num_unsatisfied: *mut u32) -> c_int;
    pub fn frw_r1cs_diag_host_allocations(r: *const frw_r1cs, count: *mut u64) -> c_int;
    pub fn frw_msm_g1_load(device: c_int, num_points: usize, bases: *const u64, out: *mut *mut frw_msm) -> c_int;
    pub fn frw_msm_free(m: *mut frw_msm);
    pub fn frw_g1_fixed_base(device: c_int, count: usize, scalars: *const u64, out: *mut u64) -> c_int;
    pub fn frw_g2_fixed_base(device: c_int, count: usize, scalars: *const u64, out: *mut u64) -> c_int;
    pub fn frw_msm_g2_load(device: c_int, num_points: usize, bases: *const u64, out: *mut *mut frw_msm) -> c_int;
    pub fn frw_msm_g1_load_narrow(device: c_int, num_points: usize, bases: *const u64, out: *mut *mut frw_msm) -> c_int;
    pub fn frw_msm_g2_load_narrow(device: c_int, num_points: usize, bases: *const u64, out: *mut *mut frw_msm) -> c_int;
    pub fn frw_msm_g2_dev(m: *const frw_msm, batch: usize, d_scalars: *const u64, scalar_stride: usize, montgomery: c_int,
                          d_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_msm_info(m: *const frw_msm, out: *mut frw_msm_info_t) -> c_int;
    pub fn frw_msm_g1_dev(m: *const frw_msm, batch: usize, d_scalars: *const u64, scalar_stride: usize, montgomery: c_int,
                          d_out: *mut u64, d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_msm_h_dev(m: *const frw_msm, batch: usize, d_h: *const u64, domain_size: usize, d_out: *mut u64,
                                 d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_pk_load(device: c_int, desc: *const frw_groth16_pk_desc_t, out: *mut *mut frw_groth16_pk) -> c_int;
    pub fn frw_groth16_pk_load_opts(device: c_int, desc: *const frw_groth16_pk_desc_t, opts: *const frw_groth16_key_opts_t,
                                    out: *mut *mut frw_groth16_pk) -> c_int;
    pub fn frw_groth16_pk_info(pk: *const frw_groth16_pk, out: *mut frw_groth16_pk_info_t) -> c_int;
    pub fn frw_groth16_pk_query(pk: *const frw_groth16_pk, which: c_int) -> *const frw_msm;
    pub fn frw_groth16_setup_r1cs_opts(r: *const frw_r1cs, toxic: *const u64, opts: *const frw_groth16_key_opts_t,
                                       pk_out: *mut *mut frw_groth16_pk, vk_out: *mut u64) -> c_int;
    pub fn frw_groth16_prove_partial_dev(pk: *const frw_groth16_pk, r: *const frw_r1cs, batch: usize, d_witness: *const u64,
                                         d_instance: *const u64, rs: *const u64, d_partial: *mut u64, d_num_unsatisfied: *mut u32,
                                         d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_prove_combine_dev(pk: *const frw_groth16_pk, world: usize, d_partials: *const u64, rs: *const u64,
                                         d_proof: *mut u64, d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_msm_g1_load_bare(device: c_int, num_points: usize, bases: *const u64, narrow: c_int, out: *mut *mut frw_msm) -> c_int;
    pub fn frw_msm_g2_load_bare(device: c_int, num_points: usize, bases: *const u64, narrow: c_int, out: *mut *mut frw_msm) -> c_int;
    pub fn frw_diag_poly_eval_dev(device: c_int, n: u64, d_coeffs: *const u64, t: *const u64, out: *mut u64) -> c_int;
    pub fn frw_diag_groth16_side_counts(pk: *const frw_groth16_pk, d_z: *const u64, d_workspace: *mut c_void, workspace_bytes: usize,
                                        stream: *mut c_void, out: *mut u64) -> c_int;
    pub fn frw_groth16_pk_free(pk: *mut frw_groth16_pk);
    pub fn frw_groth16_setup(device: c_int, circuit: c_int, logn: c_int, toxic: *const u64, pk_out: *mut *mut frw_groth16_pk,
                             vk_out: *mut u64) -> c_int;
    pub fn frw_groth16_workspace_bytes(pk: *const frw_groth16_pk, r: *const frw_r1cs, batch_in_flight: usize) -> usize;
    pub fn frw_groth16_prove_dev(pk: *const frw_groth16_pk, r: *const frw_r1cs, batch: usize, d_witness: *const u64,
                                 d_instance: *const u64, rs: *const u64, d_proofs: *mut u64, d_num_unsatisfied: *mut u32,
                                 d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_prove_rs_dev(pk: *const frw_groth16_pk, r: *const frw_r1cs, batch: usize, d_witness: *const u64,
                                    d_instance: *const u64, d_rs: *const u64, d_proofs: *mut u64, d_num_unsatisfied: *mut u32,
                                    d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_vk_load(vk: *const u64, num_instance: usize, out: *mut *mut frw_groth16_vk) -> c_int;
    pub fn frw_groth16_vk_load_opts(vk: *const u64, num_instance: usize, flags: c_int, out: *mut *mut frw_groth16_vk) -> c_int;
    pub fn frw_groth16_vk_free(vk: *mut frw_groth16_vk);
    pub fn frw_groth16_verify(vk: *const frw_groth16_vk, batch: usize, instance: *const u64, encoding: c_int, proofs: *const u64,
                              flags: c_int, accepted: *mut i32) -> c_int;
    pub fn frw_groth16_vk_load_dev(device: c_int, vk: *const u64, num_instance: usize, flags: c_int,
                                   out: *mut *mut frw_groth16_vk) -> c_int;
    pub fn frw_groth16_verify_workspace_bytes(vk: *const frw_groth16_vk, batch_in_flight: usize) -> usize;
    pub fn frw_groth16_prepare_inputs_dev(vk: *const frw_groth16_vk, batch: usize, d_instance: *const u64, encoding: c_int,
                                          d_prepared: *mut u64, d_status: *mut i32, d_workspace: *mut c_void,
                                          workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_verify_dev(vk: *const frw_groth16_vk, batch: usize, d_instance: *const u64, encoding: c_int,
                                  d_proofs: *const u64, flags: c_int, accepted: *mut i32, d_workspace: *mut c_void,
                                  workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_diag_pairing(g1: *const u64, g2: *const u64, out: *mut u64) -> c_int;
    pub fn frw_groth16_verify_full_workspace_bytes(vk: *const frw_groth16_vk, batch_in_flight: usize, flags: c_int) -> usize;
    pub fn frw_groth16_verify_full_dev(vk: *const frw_groth16_vk, batch: usize, d_instance: *const u64, encoding: c_int,
                                       d_proofs: *const u64, flags: c_int, seed: *const u64, d_accepted: *mut i32,
                                       d_batch_passed: *mut i32, d_workspace: *mut c_void, workspace_bytes: usize,
                                       stream: *mut c_void) -> c_int;
    pub fn frw_groth16_proof_wire_bytes(mode: c_int) -> usize;
    pub fn frw_groth16_vk_wire_bytes(num_instance: usize, mode: c_int) -> usize;
    pub fn frw_groth16_proofs_to_wire(batch: usize, proofs: *const u64, mode: c_int, out: *mut u8, status: *mut i32) -> c_int;
    pub fn frw_groth16_proofs_from_wire(batch: usize, input: *const u8, mode: c_int, proofs: *mut u64, status: *mut i32) -> c_int;
    pub fn frw_groth16_proofs_to_wire_dev(device: c_int, batch: usize, d_proofs: *const u64, mode: c_int, d_out: *mut u8,
                                          d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_proofs_from_wire_dev(device: c_int, batch: usize, d_in: *const u8, mode: c_int, d_proofs: *mut u64,
                                            d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_verify_wire_workspace_bytes(vk: *const frw_groth16_vk, batch_in_flight: usize, flags: c_int, mode: c_int) -> usize;
    pub fn frw_groth16_verify_wire_dev(vk: *const frw_groth16_vk, batch: usize, d_instance: *const u64, encoding: c_int,
                                       d_wire: *const u8, mode: c_int, flags: c_int, seed: *const u64, d_accepted: *mut i32,
                                       d_batch_passed: *mut i32, d_workspace: *mut c_void, workspace_bytes: usize,
                                       stream: *mut c_void) -> c_int;
    pub fn frw_groth16_vk_to_wire(vk: *const u64, num_instance: usize, mode: c_int, out: *mut u8) -> c_int;
    pub fn frw_groth16_vk_load_wire(bytes: *const u8, len: usize, mode: c_int, out: *mut *mut frw_groth16_vk) -> c_int;
    pub fn frw_groth16_vk_load_wire_dev(device: c_int, bytes: *const u8, len: usize, mode: c_int, out: *mut *mut frw_groth16_vk) -> c_int;
    pub fn frw_groth16_pk_wire_bytes(num_instance: u64, num_witness: u64, domain_size: u64, mode: c_int) -> usize;
    pub fn frw_groth16_pk_wire_info(bytes: *const u8, len: usize, mode: c_int, out: *mut frw_groth16_pk_wire_info_t) -> c_int;
    pub fn frw_groth16_pk_load_wire_dev(device: c_int, bytes: *const u8, len: usize, mode: c_int, flags: c_int, opts: *const frw_groth16_key_opts_t,
                                        pk_out: *mut *mut frw_groth16_pk, vk_out: *mut u64) -> c_int;
    pub fn frw_groth16_pk_to_wire_dev(pk: *const frw_groth16_pk, vk: *const u64, num_instance: usize, mode: c_int, out: *mut u8, out_len: usize) -> c_int;
    pub fn frw_diag_wire_greater(c0: *const u64, c1: *const u64) -> c_int;
    pub fn frw_groth16_rerandomize(vk: *const frw_groth16_vk, batch: usize, proofs: *const u64, factors: *const u64, flags: c_int,
                                   out: *mut u64, status: *mut i32) -> c_int;
    pub fn frw_groth16_rerandomize_workspace_bytes(vk: *const frw_groth16_vk, batch_in_flight: usize, wire_mode: c_int) -> usize;
    pub fn frw_groth16_rerandomize_dev(vk: *const frw_groth16_vk, batch: usize, d_proofs: *const u64, d_factors: *const u64, flags: c_int,
                                       d_out: *mut u64, d_status: *mut i32, d_workspace: *mut c_void, workspace_bytes: usize,
                                       stream: *mut c_void) -> c_int;
    pub fn frw_groth16_rerandomize_wire_dev(vk: *const frw_groth16_vk, batch: usize, d_wire_in: *const u8, mode: c_int, d_factors: *const u64,
                                            flags: c_int, d_wire_out: *mut u8, d_status: *mut i32, d_workspace: *mut c_void,
                                            workspace_bytes: usize, stream: *mut c_void) -> c_int;
    // drawing the factors on the device (frw.h: seed secret, (seed, counter) never reused)
    pub fn frw_fr_draw(seed: *const u8, counter: u64, tag: c_int, count: usize, out: *mut u64) -> c_int;
    pub fn frw_fr_draw_dev(device: c_int, d_seed: *const u8, d_counter: *mut u64, tag: c_int, count: usize, d_out: *mut u64,
                           stream: *mut c_void) -> c_int;
    pub fn frw_groth16_prove_seeded_dev(pk: *const frw_groth16_pk, r: *const frw_r1cs, batch: usize, d_witness: *const u64,
                                        d_instance: *const u64, d_seed: *const u8, d_counter: *mut u64, d_rs: *mut u64,
                                        d_proofs: *mut u64, d_num_unsatisfied: *mut u32, d_workspace: *mut c_void,
                                        workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_groth16_rerandomize_seeded_dev(vk: *const frw_groth16_vk, batch: usize, d_proofs: *const u64, d_seed: *const u8,
                                              d_counter: *mut u64, d_factors: *mut u64, flags: c_int, d_out: *mut u64,
                                              d_status: *mut i32, d_workspace: *mut c_void, workspace_bytes: usize,
                                              stream: *mut c_void) -> c_int;
    pub fn frw_groth16_rerandomize_wire_seeded_dev(vk: *const frw_groth16_vk, batch: usize, d_wire_in: *const u8, mode: c_int,
                                                   d_seed: *const u8, d_counter: *mut u64, d_factors: *mut u64, flags: c_int,
                                                   d_wire_out: *mut u8, d_status: *mut i32, d_workspace: *mut c_void,
                                                   workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_diag_pairing_dev(device: c_int, count: usize, g1: *const u64, g2: *const u64, out: *mut u64) -> c_int;
    pub fn frw_hash_to_point_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_nonces: *const u8, d_msgs: *const u8,
                                 d_msg_off: *const u64, d_hm: *mut u16, stream: *mut c_void) -> c_int;
    pub fn frw_decode_public_keys_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_pk_bytes: *const u8,
                                      d_pk: *mut u16, d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_decode_signatures_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_sig_bytes: *const u8,
                                     sig_len: usize, d_sig: *mut u16, d_nonce_out: *mut u8, d_status: *mut i32,
                                     stream: *mut c_void) -> c_int;
    pub fn frw_prepare_inputs(ctx: *mut frw_ctx, logn: c_int, batch: usize, pk_bytes: *const u8, sig_bytes: *const u8,
                              sig_len: usize, msgs: *const u8, msg_off: *const u64, sig: *mut u16, pk: *mut u16,
                              hm: *mut u16, status: *mut i32) -> c_int;
    pub fn frw_statement_dev(ctx: *mut frw_ctx, circuit: c_int, logn: c_int, batch: usize, d_pk: *const u16, d_hm: *const u16,
                             encoding: c_int, d_instance: *mut u64, d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_statement(ctx: *mut frw_ctx, circuit: c_int, logn: c_int, batch: usize, pk: *const u16, hm: *const u16,
                         encoding: c_int, instance: *mut u64, status: *mut i32, strict: c_int) -> c_int;
    pub fn frw_statement_workspace_bytes(logn: c_int, batch: usize) -> usize;
    pub fn frw_statement_from_bytes_dev(ctx: *mut frw_ctx, circuit: c_int, logn: c_int, batch: usize, d_pk_bytes: *const u8,
                                        d_nonces: *const u8, d_msgs: *const u8, d_msg_off: *const u64, encoding: c_int,
                                        d_instance: *mut u64, d_status: *mut i32, d_workspace: *mut c_void,
                                        workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_statement_from_bytes(ctx: *mut frw_ctx, circuit: c_int, logn: c_int, batch: usize, pk_bytes: *const u8,
                                    nonces: *const u8, msgs: *const u8, msg_off: *const u64, encoding: c_int,
                                    instance: *mut u64, status: *mut i32, strict: c_int) -> c_int;
    pub fn frw_aggregate_statement_dev(aggregate: *const frw_r1cs, ctx: *mut frw_ctx, d_pk_512: *const u16, d_hm_512: *const u16,
                                       d_pk_1024: *const u16, d_hm_1024: *const u16, encoding: c_int, d_instance: *mut u64,
                                       d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_falcon_verify_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_sig: *const u16, d_pk: *const u16, d_hm: *const u16,
                                 rule: c_int, d_status: *mut i32, d_norm: *mut u64, stream: *mut c_void) -> c_int;
    pub fn frw_falcon_verify(ctx: *mut frw_ctx, logn: c_int, batch: usize, sig: *const u16, pk: *const u16, hm: *const u16,
                             rule: c_int, status: *mut i32, norm: *mut u64, strict: c_int) -> c_int;
    pub fn frw_falcon_verify_workspace_bytes(logn: c_int, batch: usize) -> usize;
    pub fn frw_falcon_verify_from_bytes_dev(ctx: *mut frw_ctx, logn: c_int, batch: usize, d_pk_bytes: *const u8,
                                            d_sig_bytes: *const u8, sig_len: usize, d_msgs: *const u8, d_msg_off: *const u64,
                                            rule: c_int, d_status: *mut i32, d_norm: *mut u64, d_workspace: *mut c_void,
                                            workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_falcon_verify_from_bytes(ctx: *mut frw_ctx, logn: c_int, batch: usize, pk_bytes: *const u8, sig_bytes: *const u8,
                                        sig_len: usize, msgs: *const u8, msg_off: *const u64, rule: c_int, status: *mut i32,
                                        norm: *mut u64, strict: c_int) -> c_int;
    pub fn frw_pok_prove_workspace_bytes(pk: *const frw_groth16_pk, r: *const frw_r1cs, circuit: c_int, logn: c_int, batch: usize,
                                         in_flight: usize) -> usize;
    pub fn frw_pok_prove_from_bytes_dev(ctx: *mut frw_ctx, pk: *const frw_groth16_pk, r: *const frw_r1cs, circuit: c_int, logn: c_int,
                                        batch: usize, d_pk_bytes: *const u8, d_sig_bytes: *const u8, sig_len: usize,
                                        d_msgs: *const u8, d_msg_off: *const u64, d_rs: *const u64, wire_mode: c_int,
                                        d_wire: *mut u8, d_proofs: *mut u64, d_instance: *mut u64, d_status: *mut i32,
                                        d_num_unsatisfied: *mut u32, d_workspace: *mut c_void, workspace_bytes: usize,
                                        stream: *mut c_void) -> c_int;
    pub fn frw_pok_prove_from_bytes(ctx: *mut frw_ctx, pk: *const frw_groth16_pk, r: *const frw_r1cs, circuit: c_int, logn: c_int,
                                    batch: usize, pk_bytes: *const u8, sig_bytes: *const u8, sig_len: usize, msgs: *const u8,
                                    msg_off: *const u64, rs: *const u64, wire_mode: c_int, wire: *mut u8, proofs: *mut u64,
                                    instance: *mut u64, status: *mut i32, num_unsatisfied: *mut u32, strict: c_int) -> c_int;
    pub fn frw_aggregate_screen_workspace_bytes(aggregate: *const frw_r1cs) -> usize;
    pub fn frw_aggregate_falcon_verify_from_bytes_dev(aggregate: *const frw_r1cs, ctx: *mut frw_ctx, d_pk_bytes: *const u8,
                                                      d_sig_bytes: *const u8, d_msgs: *const u8, d_msg_off: *const u64, rule: c_int,
                                                      d_status: *mut i32, d_norm: *mut u64, d_workspace: *mut c_void,
                                                      workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_aggregate_statement_from_bytes_dev(aggregate: *const frw_r1cs, ctx: *mut frw_ctx, d_pk_bytes: *const u8,
                                                  d_nonces: *const u8, d_msgs: *const u8, d_msg_off: *const u64, encoding: c_int,
                                                  d_instance: *mut u64, d_status: *mut i32, d_workspace: *mut c_void,
                                                  workspace_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn frw_aggregate_prove_workspace_bytes(pk: *const frw_groth16_pk, aggregate: *const frw_r1cs) -> usize;
    pub fn frw_aggregate_prove_from_bytes_dev(ctx: *mut frw_ctx, pk: *const frw_groth16_pk, aggregate: *const frw_r1cs,
                                              d_pk_bytes: *const u8, d_sig_bytes: *const u8, d_msgs: *const u8, d_msg_off: *const u64,
                                              d_rs: *const u64, wire_mode: c_int, d_wire: *mut u8, d_proof: *mut u64,
                                              d_instance: *mut u64, d_nonces_out: *mut u8, d_status: *mut i32,
                                              d_num_unsatisfied: *mut u32, d_workspace: *mut c_void, workspace_bytes: usize,
                                              stream: *mut c_void) -> c_int;
    pub fn frw_aggregate_falcon_verify_from_bytes(aggregate: *const frw_r1cs, ctx: *mut frw_ctx, pk_bytes: *const u8,
                                                  sig_bytes: *const u8, msgs: *const u8, msg_off: *const u64, rule: c_int,
                                                  status: *mut i32, norm: *mut u64) -> c_int;
    pub fn frw_aggregate_statement_from_bytes(aggregate: *const frw_r1cs, ctx: *mut frw_ctx, pk_bytes: *const u8, nonces: *const u8,
                                              msgs: *const u8, msg_off: *const u64, encoding: c_int, instance: *mut u64,
                                              status: *mut i32) -> c_int;
    pub fn frw_aggregate_prove_from_bytes(ctx: *mut frw_ctx, pk: *const frw_groth16_pk, aggregate: *const frw_r1cs, pk_bytes: *const u8,
                                          sig_bytes: *const u8, msgs: *const u8, msg_off: *const u64, rs: *const u64, wire_mode: c_int,
                                          wire: *mut u8, proof: *mut u64, instance: *mut u64, nonces_out: *mut u8, status: *mut i32,
                                          num_unsatisfied: *mut u32) -> c_int;
    pub fn frw_gadget_block_len(kind: c_int) -> c_int;
    pub fn frw_gadget_dev(ctx: *mut frw_ctx, kind: c_int, count: usize, d_a: *const c_void, d_b: *const u64,
                          encoding: c_int, d_out: *mut u64, d_status: *mut i32, stream: *mut c_void) -> c_int;
    pub fn frw_gadget(ctx: *mut frw_ctx, kind: c_int, count: usize, a: *const c_void, b: *const u64, encoding: c_int,
                      out: *mut u64, status: *mut i32) -> c_int;
    pub fn frw_digest_dev(ctx: *mut frw_ctx, d_buf: *const u64, words_per_item: usize, items: usize, d_out: *mut u64,
                          stream: *mut c_void) -> c_int;
    pub fn frw_diag_launch_shape(ctx: *mut frw_ctx, logn: c_int, encoding: c_int, batch: usize, out: *mut i32) -> c_int;
    pub fn frw_diag_write_stream_dev(ctx: *mut frw_ctx, d_buf: *mut c_void, bytes: usize, slab_bytes: usize,
                                     stream: *mut c_void) -> c_int;
    pub fn frw_synth_triples(logn: c_int, batch: usize, seed: u64, first_index: u64, sig: *mut u16, pk: *mut u16,
                             hm: *mut u16) -> c_int;
    pub fn frw_host_alloc(ctx: *mut frw_ctx, bytes: usize, ptr: *mut *mut c_void) -> c_int;
    pub fn frw_host_free(ctx: *mut frw_ctx, ptr: *mut c_void) -> c_int;
    pub fn frw_malloc(ctx: *mut frw_ctx, bytes: usize, d_ptr: *mut *mut c_void) -> c_int;
    pub fn frw_free(ctx: *mut frw_ctx, d_ptr: *mut c_void) -> c_int;
    pub fn frw_memcpy_h2d(ctx: *mut frw_ctx, d_dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;
    pub fn frw_memcpy_d2h(ctx: *mut frw_ctx, dst: *mut c_void, d_src: *const c_void, bytes: usize) -> c_int;
    pub fn frw_synchronize(ctx: *mut frw_ctx, stream: *mut c_void) -> c_int;
}
