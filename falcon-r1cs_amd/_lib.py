"""ctypes binding of libfrw.so (the C ABI declared in include/frw.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C falcon-r1cs_amd/csrc``.
There is no fallback: if the shared object is missing or no HIP device is usable, callers get
an exception, never a CPU-computed result.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class FrwError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__("%s failed: %d %s" % (where, code, detail))


def lib_path():
    return os.path.join(_HERE, "libfrw.so")


class LayoutStruct(C.Structure):
    _fields_ = [("logn", C.c_int32), ("n", C.c_int32), ("num_witness", C.c_int32),
                ("num_instance", C.c_int32), ("num_constraints", C.c_int32),
                ("seg_off", C.c_int32 * 8), ("seg_len", C.c_int32 * 8)]


class LayoutDualStruct(C.Structure):
    _fields_ = [("logn", C.c_int32), ("n", C.c_int32), ("num_witness", C.c_int32),
                ("num_instance", C.c_int32), ("num_constraints", C.c_int32),
                ("seg_off", C.c_int32 * 15), ("seg_len", C.c_int32 * 15)]


class LayoutSchoolbookStruct(C.Structure):
    _fields_ = [("logn", C.c_int32), ("n", C.c_int32), ("num_witness", C.c_int32),
                ("num_instance", C.c_int32), ("num_constraints", C.c_int32), ("column_len", C.c_int32),
                ("seg_off", C.c_int32 * 5), ("seg_len", C.c_int32 * 5)]


class CompactLayoutStruct(C.Structure):
    _fields_ = [("logn", C.c_int32), ("n", C.c_int32), ("bytes_per_signature", C.c_uint64),
                ("small_off", C.c_uint64), ("num_small", C.c_uint64), ("t_off", C.c_uint64), ("num_t", C.c_uint64),
                ("bits_off", C.c_uint64),
                ("num_bit_words", C.c_uint64), ("bit_seg_off", C.c_uint64 * 6), ("instance_off", C.c_uint64),
                ("num_instance_values", C.c_uint64), ("status_off", C.c_uint64)]


class FieldInfoStruct(C.Structure):
    _fields_ = [("modulus", C.c_uint64 * 4), ("one", C.c_uint64 * 4), ("r2", C.c_uint64 * 4), ("ninv32", C.c_uint32), ("bits", C.c_uint32)]


class MsmInfoStruct(C.Structure):
    _fields_ = [("num_points", C.c_uint64), ("window_bits", C.c_int32), ("num_windows", C.c_int32), ("table_bytes", C.c_uint64),
                ("workspace_bytes_per_signature", C.c_uint64)]


class Groth16PkDesc(C.Structure):
    _fields_ = [("num_instance", C.c_uint64), ("num_witness", C.c_uint64), ("domain_size", C.c_uint64),
                ("alpha_g1", C.c_void_p), ("beta_g1", C.c_void_p), ("delta_g1", C.c_void_p), ("beta_g2", C.c_void_p),
                ("delta_g2", C.c_void_p), ("a_query", C.c_void_p), ("b_g1_query", C.c_void_p), ("b_g2_query", C.c_void_p),
                ("h_query", C.c_void_p), ("l_query", C.c_void_p)]


class Groth16KeyOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("rank", C.c_uint32), ("world", C.c_uint32)]


class Groth16PkInfoStruct(C.Structure):
    _fields_ = [("mode", C.c_int32), ("rank", C.c_uint32), ("world", C.c_uint32), ("z_lo", C.c_uint64), ("z_hi", C.c_uint64),
                ("h_lo", C.c_uint64), ("h_hi", C.c_uint64), ("key_bytes", C.c_uint64)]


class Groth16PkWireInfoStruct(C.Structure):
    _fields_ = [("num_instance", C.c_uint64), ("num_witness", C.c_uint64), ("domain_size", C.c_uint64),
                ("a_query_offset", C.c_uint64), ("b_g1_query_offset", C.c_uint64), ("b_g2_query_offset", C.c_uint64),
                ("h_query_offset", C.c_uint64), ("l_query_offset", C.c_uint64)]


class R1csInfoStruct(C.Structure):
    _fields_ = [("num_statements", C.c_uint64), ("count_logn9", C.c_uint64), ("count_logn10", C.c_uint64),
                ("num_instance", C.c_uint64), ("num_witness", C.c_uint64), ("num_constraints", C.c_uint64),
                ("log_domain_size", C.c_int32), ("witness_map_on_device", C.c_int32)]


class R1csfInfoStruct(C.Structure):
    _fields_ = [("modulus", C.c_uint64 * 4), ("num_instance", C.c_uint64), ("num_witness", C.c_uint64), ("num_constraints", C.c_uint64),
                ("nnz", C.c_uint64 * 3), ("scratch_bytes_per_statement", C.c_uint64 * 2)]


class FftFieldInfoStruct(C.Structure):
    _fields_ = [("modulus", C.c_uint64 * 4), ("generator", C.c_uint64 * 4), ("two_adicity", C.c_uint32), ("reserved", C.c_uint32),
                ("two_adic_root", C.c_uint64 * 4), ("two_adic_root_mont", C.c_uint64 * 4)]


class QapfDomainStruct(C.Structure):
    _fields_ = [("log_size", C.c_uint32), ("reserved", C.c_uint32), ("size", C.c_uint64), ("group_gen", C.c_uint64 * 4),
                ("group_gen_inv", C.c_uint64 * 4), ("size_inv", C.c_uint64 * 4), ("generator_inv", C.c_uint64 * 4),
                ("vanishing_inv", C.c_uint64 * 4)]


class QapfInfoStruct(C.Structure):
    _fields_ = [("domain", QapfDomainStruct), ("num_constraints", C.c_uint64), ("num_instance", C.c_uint64), ("num_passes", C.c_uint32),
                ("reserved", C.c_uint32), ("workspace_bytes_per_statement", C.c_uint64)]


class CurveStruct(C.Structure):
    _fields_ = [("base_modulus", C.c_uint64 * 4), ("scalar_modulus", C.c_uint64 * 4), ("b", C.c_uint64 * 4)]


class CurveInfoStruct(C.Structure):
    _fields_ = [("base_bits", C.c_uint32), ("scalar_bits", C.c_uint32), ("b_mont", C.c_uint64 * 4), ("one_mont", C.c_uint64 * 4),
                ("scalar_one_mont", C.c_uint64 * 4)]


class MsmfInfoStruct(C.Structure):
    _fields_ = [("num_points", C.c_uint64), ("window_bits", C.c_uint32), ("num_windows", C.c_uint32), ("reserved", C.c_uint64),
                ("bases_bytes", C.c_uint64), ("workspace_bytes_per_statement", C.c_uint64)]


class Curve2Struct(C.Structure):
    _fields_ = [("base_modulus", C.c_uint64 * 4), ("scalar_modulus", C.c_uint64 * 4), ("nonresidue", C.c_uint64 * 4), ("b", C.c_uint64 * 8)]


class Curve2InfoStruct(C.Structure):
    _fields_ = [("base_bits", C.c_uint32), ("scalar_bits", C.c_uint32), ("b_mont", C.c_uint64 * 8), ("one_mont", C.c_uint64 * 4),
                ("nonresidue_mont", C.c_uint64 * 4), ("scalar_one_mont", C.c_uint64 * 4), ("nonresidue_is_minus_one", C.c_uint32),
                ("reserved", C.c_uint32)]


class Msmf2InfoStruct(C.Structure):
    _fields_ = [("num_points", C.c_uint64), ("window_bits", C.c_uint32), ("num_windows", C.c_uint32), ("reserved", C.c_uint64),
                ("bases_bytes", C.c_uint64), ("workspace_bytes_per_statement", C.c_uint64)]


class QapInfoStruct(C.Structure):
    _fields_ = [("log_domain_size", C.c_int32), ("domain_size", C.c_uint64), ("num_constraints", C.c_uint64),
                ("num_instance", C.c_uint64), ("workspace_bytes_per_signature", C.c_uint64)]


# name -> (restype, argtypes); must list every symbol include/frw.h declares
PROTOTYPES = {
    "frw_layout": (C.c_int, [C.c_int, C.POINTER(LayoutStruct)]),
    "frw_strerror": (C.c_char_p, [C.c_int]),
    "frw_last_error": (C.c_char_p, []),
    "frw_device_count": (C.c_int, []),
    "frw_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "frw_ctx_destroy": (None, [C.c_void_p]),
    "frw_witness_ntt_verify_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_ntt_modq_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "frw_witness_ntt_verify": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "frw_ntt_modq": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "frw_diag_host_allocations": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "frw_ctx_trim": (C.c_int, [C.c_void_p]),
    "frw_diag_valu_rates": (C.c_int, [C.c_void_p, C.POINTER(C.c_double * 4)]),
    "frw_r1cs_diag_host_allocations": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "frw_msm_g1_load": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "frw_msm_free": (None, [C.c_void_p]),
    "frw_g1_fixed_base": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "frw_g2_fixed_base": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "frw_msm_g2_load": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "frw_msm_g1_load_narrow": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "frw_msm_g2_load_narrow": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "frw_msm_g1_load_bare": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_msm_g2_load_bare": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_groth16_pk_load_opts": (C.c_int, [C.c_int, C.POINTER(Groth16PkDesc), C.POINTER(Groth16KeyOpts), C.POINTER(C.c_void_p)]),
    "frw_groth16_pk_query": (C.c_void_p, [C.c_void_p, C.c_int]),
    "frw_groth16_pk_info": (C.c_int, [C.c_void_p, C.POINTER(Groth16PkInfoStruct)]),
    "frw_groth16_setup_r1cs_opts": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Groth16KeyOpts), C.POINTER(C.c_void_p), C.c_void_p]),
    "frw_groth16_prove_partial_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_groth16_prove_combine_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_groth16_vk_load_opts": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_diag_poly_eval_dev": (C.c_int, [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_diag_groth16_side_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "frw_msm_g2_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "frw_msm_info": (C.c_int, [C.c_void_p, C.POINTER(MsmInfoStruct)]),
    "frw_msm_g1_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "frw_groth16_msm_h_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "frw_groth16_pk_load": (C.c_int, [C.c_int, C.POINTER(Groth16PkDesc), C.POINTER(C.c_void_p)]),
    "frw_groth16_pk_free": (None, [C.c_void_p]),
    "frw_groth16_setup": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "frw_groth16_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "frw_groth16_prove_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_groth16_prove_rs_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_groth16_vk_load": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "frw_groth16_vk_free": (None, [C.c_void_p]),
    "frw_groth16_verify": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "frw_groth16_vk_load_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_groth16_verify_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "frw_groth16_prepare_inputs_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                 C.c_void_p]),
    "frw_groth16_verify_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "frw_diag_pairing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_groth16_proof_wire_bytes": (C.c_size_t, [C.c_int]),
    "frw_groth16_vk_wire_bytes": (C.c_size_t, [C.c_size_t, C.c_int]),
    "frw_groth16_proofs_to_wire": (C.c_int, [C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "frw_groth16_proofs_from_wire": (C.c_int, [C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "frw_groth16_proofs_to_wire_dev": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_groth16_proofs_from_wire_dev": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_groth16_verify_wire_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "frw_groth16_verify_wire_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_groth16_vk_to_wire": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "frw_groth16_vk_load_wire": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_groth16_vk_load_wire_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_groth16_pk_wire_bytes": (C.c_size_t, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]),
    "frw_groth16_pk_wire_info": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Groth16PkWireInfoStruct)]),
    "frw_groth16_pk_load_wire_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(Groth16KeyOpts), C.POINTER(C.c_void_p),
                                               C.c_void_p]),
    "frw_groth16_pk_to_wire_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]),
    "frw_diag_wire_greater": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frw_groth16_verify_full_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_int]),
    "frw_groth16_verify_full_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_diag_pairing_dev": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_groth16_rerandomize": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "frw_groth16_rerandomize_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_int]),
    "frw_groth16_rerandomize_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]),
    "frw_groth16_rerandomize_wire_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_fr_draw": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_size_t, C.c_void_p]),
    "frw_fr_draw_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "frw_groth16_prove_seeded_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_groth16_rerandomize_seeded_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_groth16_rerandomize_wire_seeded_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_compact_layout": (C.c_int, [C.c_int, C.POINTER(CompactLayoutStruct)]),
    "frw_witness_ntt_verify_compact_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_expand_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_expand_host": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_field_info": (C.c_int, [C.c_void_p, C.POINTER(FieldInfoStruct)]),
    "frw_ctx_field_encoding": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "frw_expand_field_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_expand_field_host": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_diag_launch_shape": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int32 * 4)]),
    "frw_layout_dual": (C.c_int, [C.c_int, C.POINTER(LayoutDualStruct)]),
    "frw_witness_dual_ntt_verify_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_witness_dual_ntt_verify": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "frw_layout_schoolbook": (C.c_int, [C.c_int, C.POINTER(LayoutSchoolbookStruct)]),
    "frw_witness_schoolbook_verify_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_witness_schoolbook_verify": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "frw_r1cs_export": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_void_p]),
    "frw_r1cs_load": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_r1cs_load_csr": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "frw_r1cs_load_file": (C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]),
    "frw_r1cs_free": (None, [C.c_void_p]),
    "frw_r1cs_export_field": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p]),
    "frw_r1csf_load": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "frw_r1csf_load_csr": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "frw_r1csf_load_file": (C.c_int, [C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "frw_r1csf_free": (None, [C.c_void_p]),
    "frw_r1csf_info": (C.c_int, [C.c_void_p, C.POINTER(R1csfInfoStruct)]),
    "frw_r1csf_scratch_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_int]),
    "frw_r1csf_check_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "frw_fft_field_info": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FftFieldInfoStruct)]),
    "frw_qapf_domain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(QapfDomainStruct)]),
    "frw_qapf_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "frw_qapf_free": (None, [C.c_void_p]),
    "frw_qapf_info": (C.c_int, [C.c_void_p, C.POINTER(QapfInfoStruct)]),
    "frw_qapf_witness_map_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    "frw_curve_info": (C.c_int, [C.POINTER(CurveStruct), C.POINTER(CurveInfoStruct)]),
    "frw_curve_check_points": (C.c_int, [C.POINTER(CurveStruct), C.c_size_t, C.c_void_p, C.POINTER(C.c_int64)]),
    "frw_curve_scalar_mul": (C.c_int, [C.POINTER(CurveStruct), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_msmf_load": (C.c_int, [C.c_int, C.POINTER(CurveStruct), C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_msmf_free": (None, [C.c_void_p]),
    "frw_msmf_info": (C.c_int, [C.c_void_p, C.POINTER(MsmfInfoStruct)]),
    "frw_msmf_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "frw_msmf_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p]),
    "frw_curve2_info": (C.c_int, [C.POINTER(Curve2Struct), C.POINTER(Curve2InfoStruct)]),
    "frw_curve2_check_points": (C.c_int, [C.POINTER(Curve2Struct), C.c_size_t, C.c_void_p, C.POINTER(C.c_int64)]),
    "frw_curve2_scalar_mul": (C.c_int, [C.POINTER(Curve2Struct), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_msmf2_load": (C.c_int, [C.c_int, C.POINTER(Curve2Struct), C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "frw_msmf2_free": (None, [C.c_void_p]),
    "frw_msmf2_info": (C.c_int, [C.c_void_p, C.POINTER(Msmf2InfoStruct)]),
    "frw_msmf2_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "frw_msmf2_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p]),
    "frw_r1cs_load_aggregate": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "frw_r1cs_info": (C.c_int, [C.c_void_p, C.POINTER(R1csInfoStruct)]),
    "frw_aggregate_assign_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_groth16_setup_r1cs": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "frw_r1cs_check_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_r1cs_eval_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_r1cs_eval_scratch_bytes": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_int]),
    "frw_r1cs_eval_scratch_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p]),
    "frw_qap_info": (C.c_int, [C.c_void_p, C.POINTER(QapInfoStruct)]),
    "frw_qap_witness_map": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_qap_quotient_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "frw_qap_witness_map_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "frw_hash_to_point_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "frw_decode_public_keys_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "frw_decode_signatures_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_prepare_inputs": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_statement_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "frw_statement": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "frw_statement_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "frw_statement_from_bytes_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_statement_from_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int]),
    "frw_aggregate_statement_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "frw_falcon_verify_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "frw_falcon_verify": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "frw_falcon_verify_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "frw_falcon_verify_from_bytes_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_falcon_verify_from_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "frw_pok_prove_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t]),
    "frw_pok_prove_from_bytes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_pok_prove_from_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int]),
    "frw_aggregate_screen_workspace_bytes": (C.c_size_t, [C.c_void_p]),
    "frw_aggregate_falcon_verify_from_bytes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_aggregate_statement_from_bytes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_aggregate_prove_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p]),
    "frw_aggregate_prove_from_bytes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "frw_aggregate_falcon_verify_from_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                         C.c_void_p, C.c_void_p]),
    "frw_aggregate_statement_from_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                     C.c_void_p, C.c_void_p]),
    "frw_aggregate_prove_from_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "frw_gadget_block_len": (C.c_int, [C.c_int]),
    "frw_gadget_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "frw_gadget": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                             C.c_void_p]),
    "frw_digest_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "frw_diag_write_stream_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "frw_synth_triples": (C.c_int, [C.c_int, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frw_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "frw_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frw_malloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "frw_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frw_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "frw_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "frw_synchronize": (C.c_int, [C.c_void_p, C.c_void_p]),
}


def load_library():
    """Load libfrw.so; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise FrwError(-2, "load_library", "%s not built; run __graft_entry__.build()" % path)
        # One HIP runtime per process: torch wheels bundle their own libamdhip64.so.7.  If torch is going to
        # be used for device memory / streams / torch.distributed in this process, its runtime must be the one
        # already mapped when libfrw.so (NEEDED libamdhip64.so.7) is loaded, or torch later finds no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(path)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def check(code, where):
    if code != 0:
        lib = load_library()
        detail = "%s; %s" % (lib.frw_strerror(code).decode(), lib.frw_last_error().decode())
        raise FrwError(code, where, detail)
