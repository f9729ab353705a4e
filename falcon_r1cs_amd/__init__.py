"""Import alias: the package directory is ``falcon-r1cs_amd/`` (not a valid Python identifier),
so ``import falcon_r1cs_amd`` resolves its submodules from there."""
import os as _os

__path__.insert(0, _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "..", "falcon-r1cs_amd"))

from ._lib import FrwError, lib_path, load_library  # noqa: E402,F401
from .engine import (G_ADD_MOD, G_L2_ELEM, G_LESS_THAN_Q, G_MOD_Q, G_NORM_BOUND_512,  # noqa: E402,F401
                     G_NORM_BOUND_1024, ENC_CANONICAL, ENC_COMPACT, ENC_MONTGOMERY, ST_COEFF_RANGE, ST_DECODE, ST_NORM_BOUND, ST_OK, NONCE_LEN, PK_LEN, SIG_LEN,  # noqa: E402,F401
                     CompactLayout, Groth16Verifier, Layout, MI355X_BENCH_LAUNCH_SHAPES, VERIFY_BATCHED, VERIFY_POINTS_ARE_CHECKED, VK_POINTS_ARE_CHECKED,
                     KEY_AUTO, KEY_TABLES, KEY_BARE, GROTH16_PARTIAL_WORDS, GROTH16_COMBINE_WORKSPACE, WitnessEngine, diag_pairing, diag_pairing_dev, compact_layout, layout, layout_dual, layout_schoolbook, circuit_layout, LayoutSchoolbook, CIRCUIT_NTT, CIRCUIT_DUAL_NTT, CIRCUIT_SCHOOLBOOK, RULE_CIRCUIT, RULE_SPEC, synth_triples,
                     WIRE_COMPRESSED, WIRE_UNCOMPRESSED, proof_wire_bytes, proofs_from_wire, proofs_from_wire_dev, proofs_to_wire, proofs_to_wire_dev, vk_to_wire,
                     PK_POINTS_ARE_CHECKED, groth16_pk_wire_bytes, groth16_pk_wire_info,
                     ENC_FIELD_BASE, MAX_FIELDS, FieldInfo, field_info, expand_field_host, r1cs_export_field, FftFieldInfo, QapfDomain, fft_field_info, qapf_domain,
                     MSMF_POINTS_ARE_CHECKED, CurveInfo, curve_info, curve_check_points, curve_scalar_mul,
                     Curve2Info, curve2_info, curve2_check_points, curve2_scalar_mul,
                     DRAW_BLINDING, DRAW_RERANDOMIZE, fr_draw, fr_draw_dev)
