"""Host-side driver of the witness engine (Python face of the C ABI in include/frw.h).

Mirrors what a caller of the reference does around
``FalconNTTVerificationCircuit::generate_constraints`` (falcon-r1cs/src/circuits/falcon_ntt.rs:26-123):
hand over (sig, pk, hm) coefficient vectors, receive ``witness_assignment`` / ``instance_assignment``
of every signature in arkworks order.  torch is used only to own device memory and streams.
"""
import ctypes as C
import os
import weakref
from dataclasses import dataclass

import numpy as np

from ._lib import CompactLayoutStruct, FieldInfoStruct, FrwError, LayoutDualStruct, LayoutSchoolbookStruct, LayoutStruct, check, load_library

ENC_CANONICAL, ENC_MONTGOMERY, ENC_COMPACT = 0, 1, 2
ST_OK, ST_COEFF_RANGE, ST_NORM_BOUND, ST_DECODE = 0, 1, 2, 3
NONCE_LEN = 40
PK_LEN = {9: 897, 10: 1793}
SIG_LEN = {9: 666, 10: 1280}
E_RANGE = -5
G_LESS_THAN_Q, G_MOD_Q, G_ADD_MOD, G_L2_ELEM, G_NORM_BOUND_512, G_NORM_BOUND_1024 = range(6)
CIRCUIT_NTT, CIRCUIT_DUAL_NTT, CIRCUIT_SCHOOLBOOK = 0, 1, 2
RULE_CIRCUIT, RULE_SPEC = 0, 1          # FRW_RULE_*: how falcon_verify* centres a coefficient and compares the norm
WIRE_COMPRESSED, WIRE_UNCOMPRESSED = 0, 1      # frw.h FRW_WIRE_*
VERIFY_POINTS_ARE_CHECKED = 1
VERIFY_BATCHED = 2


# ---- what every entry point below does the same way: pointers, packed inputs, uploads, workspaces, refusals ------------------------
# torch is imported inside the helpers that own device memory, so that the host-only paths never need it.
def _p(x):
    """The one pointer rule: None, an address, a numpy array, or anything with data_ptr() (a torch tensor) -> a void* argument."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    return C.c_void_p(x.data_ptr())


def _wire_mode(compressed):
    return WIRE_COMPRESSED if compressed else WIRE_UNCOMPRESSED


def proof_wire_bytes(compressed=True):
    return 192 if compressed else 384


def _pack(keys, second, msgs):
    """Encoded inputs as the *_from_bytes calls read them: the keys end to end, the `second` items (signatures or nonces) end to end,
    the message blob (uint8 arrays; one zero byte for an empty join, so that each has an address) and the blob's uint64[batch + 1]
    offsets.  The callers check the lengths."""
    join = lambda items: np.frombuffer(b"".join(bytes(x) for x in items) or b"\0", dtype=np.uint8)
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return join(keys), join(second), join(msgs), off


def _empty(shape, dtype, device):
    """An uninitialised device tensor: dtype by name, device a torch.device or a HIP device index."""
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype), device=device if isinstance(device, torch.device) else torch.device("cuda", device))


def _upload(arrays, device):
    """numpy arrays -> tensors on HIP device `device`, each copied once; a uint64 array goes as int64, which torch has."""
    import torch
    dev = torch.device("cuda", device)
    return [torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).to(dev) for a in arrays]


def _encoded_dev(device, logn, pk_bytes, second, msgs, sig_len, pack):
    """The encoded inputs of a *_from_bytes_dev call -> (batch, sig_len, d_pkb, d_second, d_blob, d_off).  Device tensors (msgs a
    (blob, offsets) pair) pass through, a sig_len of None worked out from them; host lists go through `pack` (_statement_bytes, or
    _falcon_verify_bytes, which also says the sig_len) and are uploaded.  The caller holds the tensors until its C call has returned."""
    import torch
    if isinstance(pk_bytes, torch.Tensor):
        d_blob, d_off = msgs
        batch = pk_bytes.numel() // PK_LEN[logn]
        if sig_len is None:
            sig_len = second.numel() // batch if batch else SIG_LEN[logn]
        return batch, sig_len, pk_bytes, second, d_blob, d_off
    batch, *packed_len, pkb, sec, blob, off = pack(logn, pk_bytes, second, msgs)
    return (batch, packed_len[0] if packed_len else sig_len, *_upload((pkb, sec, blob, off), device))


def _wire_dev(wire, device):
    """Wire bytes (a tensor, bytes, or anything numpy reads as uint8) -> the flat uint8 tensor on HIP device `device`."""
    import torch
    dev = torch.device("cuda", device)
    if isinstance(wire, torch.Tensor):
        return wire.to(dev).contiguous().view(torch.uint8).reshape(-1)
    raw = wire if isinstance(wire, (bytes, bytearray)) else np.ascontiguousarray(wire, dtype=np.uint8).tobytes()
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)


def _wire_batch(d_wire, compressed, where):
    """The number of proofs in d_wire; FrwError in the name of `where` unless it is a contiguous uint8 tensor of whole proofs."""
    import torch
    per = proof_wire_bytes(compressed)
    if d_wire.dtype != torch.uint8 or not d_wire.is_contiguous() or d_wire.numel() % per:
        raise FrwError(-1, where, "d_wire: a contiguous uint8 tensor of %d bytes per proof" % per)
    return d_wire.numel() // per


def _workspace(workspace, device, floor, needed_bytes, *args):
    """(workspace tensor, its bytes): the caller's, or a fresh uint8 one of needed_bytes(*args) bytes, `floor` at the least."""
    if workspace is None:
        workspace = _empty(max(needed_bytes(*args), floor), "uint8", device)
    return workspace, workspace.numel() * workspace.element_size()


def _batched_seed(flags, batched, seed):
    """(flags with VERIFY_BATCHED where `batched`, the batched check's seed as 4 uint64 -- 32 fresh random bytes for None -- or None
    where that check is off)."""
    flags = int(flags) | (VERIFY_BATCHED if batched else 0)
    if not flags & VERIFY_BATCHED:
        return flags, None
    if seed is None:
        return flags, np.frombuffer(os.urandom(32), dtype=np.uint64).copy()
    return flags, np.ascontiguousarray(seed, dtype=np.uint64).reshape(4)


def _refusal(status, noun, verdict="refused", head="Invalid input"):
    """The message that names the first 8 slots of `status` (a numpy array or a tensor) that are not zero, and their statuses."""
    st = np.asarray(status.tolist())
    bad = np.nonzero(st)[0]
    return "%s: %s %s %s (status %s)" % (head, noun, bad[:8], verdict, st[bad][:8])


def _check_refusal(rc, where, status, noun, verdict="refused"):
    """check(rc, where), with FRW_E_RANGE raised as the FrwError that says which slots were refused."""
    if rc == E_RANGE:
        raise FrwError(rc, where, _refusal(status, noun, verdict))
    check(rc, where)


_VK_KEYS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")


def _vk_flat(vk, where):
    """A verifying key (the dict groth16_setup returns, or flat limbs) -> (the flat uint64 array of frw_groth16_setup's vk_out, its
    num_instance); FrwError in the name of `where` for a length no key has."""
    if isinstance(vk, dict):
        vk = np.concatenate([np.asarray(vk[k], dtype=np.uint64).reshape(-1) for k in _VK_KEYS])
    vk = np.ascontiguousarray(vk, dtype=np.uint64).reshape(-1)
    if vk.size < 96 or (vk.size - 84) % 12:
        raise FrwError(-1, where, "verifying key: expected 84 + 12 x num_instance uint64 values")
    return vk, (vk.size - 84) // 12


def _vk_dict(vk):
    return {"alpha_g1": vk[:12], "beta_g2": vk[12:36], "gamma_g2": vk[36:60], "delta_g2": vk[60:84], "gamma_abc_g1": vk[84:].reshape(-1, 12)}


@dataclass(frozen=True)
class Layout:
    logn: int
    n: int
    num_witness: int
    num_instance: int
    num_constraints: int
    seg_off: tuple
    seg_len: tuple


def layout(logn) -> Layout:
    s = LayoutStruct()
    check(load_library().frw_layout(int(logn), C.byref(s)), "frw_layout")
    return Layout(s.logn, s.n, s.num_witness, s.num_instance, s.num_constraints, tuple(s.seg_off), tuple(s.seg_len))


def layout_dual(logn) -> Layout:
    """Layout of FalconDualNTTVerificationCircuit's witness (frw_layout_dual; 15 segments)."""
    s = LayoutDualStruct()
    check(load_library().frw_layout_dual(int(logn), C.byref(s)), "frw_layout_dual")
    return Layout(s.logn, s.n, s.num_witness, s.num_instance, s.num_constraints, tuple(s.seg_off), tuple(s.seg_len))


@dataclass(frozen=True)
class LayoutSchoolbook(Layout):
    column_len: int = 0


def layout_schoolbook(logn) -> LayoutSchoolbook:
    """Layout of FalconSchoolBookVerificationCircuit's witness (frw_layout_schoolbook; 5 segments, columns of N + 34)."""
    s = LayoutSchoolbookStruct()
    check(load_library().frw_layout_schoolbook(int(logn), C.byref(s)), "frw_layout_schoolbook")
    return LayoutSchoolbook(s.logn, s.n, s.num_witness, s.num_instance, s.num_constraints, tuple(s.seg_off), tuple(s.seg_len), s.column_len)


def circuit_layout(circuit, logn) -> Layout:
    """The layout of circuit 0 (NTT), 1 (dual NTT) or 2 (schoolbook)."""
    return (layout, layout_dual, layout_schoolbook)[circuit](logn)


@dataclass(frozen=True)
class CompactLayout:
    logn: int
    n: int
    bytes_per_signature: int
    small_off: int
    num_small: int
    t_off: int
    num_t: int
    bits_off: int
    num_bit_words: int
    bit_seg_off: tuple
    instance_off: int
    num_instance_values: int
    status_off: int


# Launch shapes of the two launches bench.py times on an MI355X (256 CUs, 3 resident workgroups per CU, 4x
# over-subscription): (logn, signatures per launch) -> (grid, signatures beyond the last full round, cut into five work
# items each).  bench.py asserts its timed launches against this table and tests/test_gpu_parity.py asserts the table
# against the library, so the benchmark, its test and their descriptions cannot drift apart again.
MI355X_BENCH_LAUNCH_SHAPES = {(10, 32768): (3072, 2048), (9, 8192): (2048, 0)}


def compact_layout(logn) -> CompactLayout:
    """Layout of FRW_ENC_COMPACT (frw_compact_layout): 11N u32 values + 2N five-limb quotients + boolean bit array +
    2N u32 instance values."""
    s = CompactLayoutStruct()
    check(load_library().frw_compact_layout(int(logn), C.byref(s)), "frw_compact_layout")
    return CompactLayout(s.logn, s.n, s.bytes_per_signature, s.small_off, s.num_small, s.t_off, s.num_t, s.bits_off, s.num_bit_words,
                         tuple(s.bit_seg_off), s.instance_off, s.num_instance_values, s.status_off)


ENC_FIELD_BASE, MAX_FIELDS = 16, 8                 # frw.h FRW_ENC_FIELD_BASE, FRW_MAX_FIELDS


@dataclass(frozen=True)
class FieldInfo:
    modulus: int
    one: int            # 2^256 mod p
    r2: int             # 2^512 mod p
    ninv32: int         # -p^-1 mod 2^32
    bits: int


def _limbs4(x):
    return (C.c_uint64 * 4)(*[(int(x) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])


def _modulus(p, where):
    """A modulus as the four limbs the C ABI takes; one that does not fit them is refused here, as field_info refuses it."""
    if p < 0 or p >> 256:
        raise FrwError(-1, where, "the modulus does not fit four limbs")
    return _limbs4(p)


def _csr_arrays(num_instance, num_witness, matrices):
    """A, B, C as three (row_ptr, col, val) -> the counts, the three pointer arrays frw_r1cs_load_csr / frw_r1csf_load_csr take, and the
    numpy arrays those point into (the caller holds them for the duration of the call)."""
    if len(matrices) != 3:
        raise ValueError("three matrices: A, B, C")
    ptr = [np.ascontiguousarray(m[0], dtype=np.uint64) for m in matrices]
    col = [np.ascontiguousarray(m[1], dtype=np.uint32) for m in matrices]
    val = [np.ascontiguousarray(m[2], dtype=np.uint64).reshape(-1, 4) for m in matrices]
    if any(len(c) != len(v) for c, v in zip(col, val)) or any(len(p) != len(ptr[0]) or len(p) == 0 for p in ptr):
        raise ValueError("col and val of a matrix have one entry per term; the three row_ptr have C + 1 entries")
    counts = (C.c_uint64 * 6)(num_instance, num_witness, len(ptr[0]) - 1, len(col[0]), len(col[1]), len(col[2]))
    three = [(C.c_void_p * 3)(*map(_p, arrs)) for arrs in (ptr, col, val)]
    return counts, three, (ptr, col, val)


def r1cs_export_field(circuit, logn, p, path):
    """frw_r1cs_export_field (no device): the circuit's matrices over the modulus p as an FRWR1CS1 file -> the six header counts."""
    counts = (C.c_uint64 * 6)()
    check(load_library().frw_r1cs_export_field(int(circuit), int(logn), _modulus(p, "frw_r1cs_export_field"), os.fsencode(str(path)), counts),
          "frw_r1cs_export_field")
    return list(counts)


def field_info(p) -> FieldInfo:
    """frw_field_info: the Montgomery constants of an odd modulus 2^160 < p < 2^255 (no device needed)."""
    if p < 0 or p >> 256:
        raise FrwError(-1, "frw_field_info", "the modulus does not fit four limbs")
    s = FieldInfoStruct()
    check(load_library().frw_field_info(_limbs4(p), C.byref(s)), "frw_field_info")
    val = lambda l: sum(int(v) << (64 * i) for i, v in enumerate(l))
    return FieldInfo(val(s.modulus), val(s.one), val(s.r2), int(s.ninv32), int(s.bits))


def _val4(l):
    return sum(int(v) << (64 * i) for i, v in enumerate(l))


@dataclass(frozen=True)
class FftFieldInfo:
    modulus: int
    generator: int
    two_adicity: int         # s of p - 1 = 2^s t, t odd
    two_adic_root: int       # generator^t
    two_adic_root_mont: int  # ... x 2^256 mod p


@dataclass(frozen=True)
class QapfDomain:
    log_size: int
    size: int
    group_gen: int
    group_gen_inv: int
    size_inv: int
    generator_inv: int
    vanishing_inv: int       # (generator^size - 1)^-1


def _qapf_domain_of(s):
    return QapfDomain(int(s.log_size), int(s.size), _val4(s.group_gen), _val4(s.group_gen_inv), _val4(s.size_inv), _val4(s.generator_inv),
                      _val4(s.vanishing_inv))


def fft_field_info(p, generator) -> FftFieldInfo:
    """frw_fft_field_info (no device): the two-adicity of p and the root generator^t, what ark-ff's FftParameters lists; the generator
    is the caller's (ark-bn254: 5, ark-bls12-381: 7, ark-bls12-377: 22, Pallas / Vesta: 5)."""
    from ._lib import FftFieldInfoStruct
    s = FftFieldInfoStruct()
    check(load_library().frw_fft_field_info(_modulus(p, "frw_fft_field_info"), _modulus(generator, "frw_fft_field_info"), C.byref(s)),
          "frw_fft_field_info")
    return FftFieldInfo(_val4(s.modulus), _val4(s.generator), int(s.two_adicity), _val4(s.two_adic_root), _val4(s.two_adic_root_mont))


def qapf_domain(p, generator, num_constraints, num_instance) -> QapfDomain:
    """frw_qapf_domain (no device): ark-poly's Radix2EvaluationDomain::new(C + I) over p and the constants of the coset by the generator."""
    from ._lib import QapfDomainStruct
    s = QapfDomainStruct()
    check(load_library().frw_qapf_domain(_modulus(p, "frw_qapf_domain"), _modulus(generator, "frw_qapf_domain"), num_constraints, num_instance,
                                         C.byref(s)), "frw_qapf_domain")
    return _qapf_domain_of(s)


MSMF_POINTS_ARE_CHECKED = 1                         # frw.h FRW_MSMF_POINTS_ARE_CHECKED: skip the on-curve check of the bases at load


@dataclass(frozen=True)
class CurveInfo:
    base_modulus: int
    scalar_modulus: int
    b: int
    base_bits: int
    scalar_bits: int
    b_mont: int              # b 2^256 mod q
    one_mont: int            # 2^256 mod q
    scalar_one_mont: int     # 2^256 mod r


def _curve(q, r, b, where):
    from ._lib import CurveStruct
    if b < 0 or b >> 256:
        raise FrwError(-1, where, "b does not fit four limbs")
    return CurveStruct(_modulus(q, where), _modulus(r, where), _limbs4(b))


def curve_info(q, r, b) -> CurveInfo:
    """frw_curve_info (no device): the descriptor of y^2 = x^3 + b over F_q with scalar modulus r, refused as frw.h lists (an
    inadmissible q or r, b = 0, b >= q), and its Montgomery constants."""
    from ._lib import CurveInfoStruct
    s = CurveInfoStruct()
    check(load_library().frw_curve_info(C.byref(_curve(q, r, b, "frw_curve_info")), C.byref(s)), "frw_curve_info")
    return CurveInfo(int(q), int(r), int(b), int(s.base_bits), int(s.scalar_bits), _val4(s.b_mont), _val4(s.one_mont), _val4(s.scalar_one_mont))


def curve_check_points(q, r, b, points):
    """frw_curve_check_points (no device): points uint64[count, 8] (x then y, Montgomery limbs over q; all zero: infinity) -> the index
    of the first one with a coordinate >= q or off the curve, or -1."""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    bad = C.c_int64(0)
    check(load_library().frw_curve_check_points(C.byref(_curve(q, r, b, "frw_curve_check_points")), pts.shape[0], _p(pts), C.byref(bad)),
          "frw_curve_check_points")
    return int(bad.value)


def curve_scalar_mul(q, r, b, points, scalars):
    """frw_curve_scalar_mul (no device): out[i] = scalars[i] points[i] by double-and-add, scalars uint64[count, 4] plain integers (any
    value up to 2^256 - 1) -> uint64[count, 8]."""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    ks = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    if pts.shape[0] != ks.shape[0]:
        raise ValueError("one scalar per point")
    out = np.zeros_like(pts)
    check(load_library().frw_curve_scalar_mul(C.byref(_curve(q, r, b, "frw_curve_scalar_mul")), pts.shape[0], _p(pts), _p(ks), _p(out)),
          "frw_curve_scalar_mul")
    return out


@dataclass(frozen=True)
class Curve2Info:
    base_modulus: int
    scalar_modulus: int
    nonresidue: int
    b: tuple                 # (c0, c1)
    base_bits: int
    scalar_bits: int
    b_mont: tuple            # (c0 2^256 mod q, c1 2^256 mod q)
    one_mont: int            # 2^256 mod q
    nonresidue_mont: int     # nonresidue 2^256 mod q
    scalar_one_mont: int     # 2^256 mod r
    nonresidue_is_minus_one: bool


def _curve2(q, r, nonresidue, b, where):
    from ._lib import Curve2Struct
    b0, b1 = b
    if min(nonresidue, b0, b1) < 0 or max(nonresidue, b0, b1) >> 256:
        raise FrwError(-1, where, "the non-residue or a component of b does not fit four limbs")
    return Curve2Struct(_modulus(q, where), _modulus(r, where), _limbs4(nonresidue), (C.c_uint64 * 8)(*_limbs4(b0), *_limbs4(b1)))


def curve2_info(q, r, nonresidue, b) -> Curve2Info:
    """frw_curve2_info (no device): the descriptor of y^2 = x^3 + b over Fq2 = Fq[u] / (u^2 - nonresidue), b = (c0, c1), with scalar
    modulus r, refused as frw.h lists, and its Montgomery constants."""
    from ._lib import Curve2InfoStruct
    s = Curve2InfoStruct()
    check(load_library().frw_curve2_info(C.byref(_curve2(q, r, nonresidue, b, "frw_curve2_info")), C.byref(s)), "frw_curve2_info")
    return Curve2Info(int(q), int(r), int(nonresidue), (int(b[0]), int(b[1])), int(s.base_bits), int(s.scalar_bits),
                      (_val4(s.b_mont[:4]), _val4(s.b_mont[4:])), _val4(s.one_mont), _val4(s.nonresidue_mont), _val4(s.scalar_one_mont),
                      bool(s.nonresidue_is_minus_one))


def curve2_check_points(q, r, nonresidue, b, points):
    """frw_curve2_check_points (no device): points uint64[count, 16] (x.c0, x.c1, y.c0, y.c1, Montgomery limbs over q; all zero:
    infinity) -> the index of the first one with a component >= q or off the curve, or -1."""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 16)
    bad = C.c_int64(0)
    check(load_library().frw_curve2_check_points(C.byref(_curve2(q, r, nonresidue, b, "frw_curve2_check_points")), pts.shape[0], _p(pts),
                                                 C.byref(bad)), "frw_curve2_check_points")
    return int(bad.value)


def curve2_scalar_mul(q, r, nonresidue, b, points, scalars):
    """frw_curve2_scalar_mul (no device): out[i] = scalars[i] points[i] by double-and-add, scalars uint64[count, 4] plain integers (any
    value up to 2^256 - 1) -> uint64[count, 16]."""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 16)
    ks = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    if pts.shape[0] != ks.shape[0]:
        raise ValueError("one scalar per point")
    out = np.zeros_like(pts)
    check(load_library().frw_curve2_scalar_mul(C.byref(_curve2(q, r, nonresidue, b, "frw_curve2_scalar_mul")), pts.shape[0], _p(pts), _p(ks),
                                               _p(out)), "frw_curve2_scalar_mul")
    return out


def expand_field_host(p, logn, compact):
    """frw_expand_field_host (no device): compact u8[batch, bytes_per_signature] -> (witness u64[batch, W, 4], instance
    u64[batch, I, 4]) with every element in Montgomery form over the modulus p."""
    L = layout(logn)
    compact = np.ascontiguousarray(compact, dtype=np.uint8)
    batch = compact.shape[0]
    wit = np.empty((batch, L.num_witness, 4), dtype=np.uint64)
    inst = np.empty((batch, L.num_instance, 4), dtype=np.uint64)
    check(load_library().frw_expand_field_host(_limbs4(p), logn, batch, _p(compact), _p(wit), _p(inst)), "frw_expand_field_host")
    return wit, inst


def synth_triples(logn, batch, seed=0x46414C434F4E, first_index=0):
    """Synthetic valid (sig, pk, hm) -- frw_synth_triples; uint16 arrays of shape [batch, N]."""
    n = 1 << logn
    out = [np.empty((batch, n), dtype=np.uint16) for _ in range(3)]
    check(load_library().frw_synth_triples(int(logn), batch, seed, first_index, *[_p(a) for a in out]), "frw_synth_triples")
    return tuple(out)


RERAND_ZERO_FACTOR = -2                            # frw.h FRW_RERAND_ZERO_FACTOR
VK_POINTS_ARE_CHECKED = 1
KEY_AUTO, KEY_TABLES, KEY_BARE = 0, 1, 2           # frw.h FRW_KEY_*: window tables, or the points only (keys that would not fit)
GROTH16_PARTIAL_WORDS = 72
GROTH16_COMBINE_WORKSPACE = 4096
DRAW_BLINDING, DRAW_RERANDOMIZE = 1, 2             # frw.h FRW_DRAW_*: the tags of (r, s) and of (r1, r2)


def fr_draw(seed, counter, tag, count):
    """`count` scalars of BLS12-381's Fr for (seed, counter, tag) on the host (frw_fr_draw): element j is the first 64 bytes of
    SHAKE256("FRW-FR-DRAW-001" || tag || seed || le64(counter) || le64(j)) modulo the group order.  seed: 32 bytes; counter below
    2^64; tag 0 .. 255 (DRAW_BLINDING, DRAW_RERANDOMIZE, or a caller's own).  Returns uint64[count, 4], canonical.  What fr_draw_dev
    and the *_seeded_dev calls draw, bit for bit: the seed is a secret, and a (seed, counter) pair is used once."""
    seed = np.frombuffer(bytes(seed), dtype=np.uint8)
    if seed.size != 32:
        raise FrwError(-1, "frw_fr_draw", "seed: 32 bytes")
    out = np.zeros((int(count), 4), dtype=np.uint64)
    check(load_library().frw_fr_draw(_p(seed), C.c_uint64(int(counter)), int(tag), int(count), _p(out)), "frw_fr_draw")
    return out


def fr_draw_dev(d_seed, d_counter, tag, count, out=None, stream=0):
    """fr_draw on the device of `d_seed` (frw_fr_draw_dev): d_seed a device uint8 tensor of 32 bytes, d_counter a device int64 tensor
    of one element, read by the draw and then advanced by one (modulo 2^64).  Returns int64[count, 4] (`out`, or a fresh tensor),
    ordered on `stream`; with `out` given the call allocates nothing and is capture-safe: every replay draws with the counter it finds."""
    if out is None:
        out = _empty((int(count), 4), "int64", d_seed.device)
    check(load_library().frw_fr_draw_dev(d_seed.device.index or 0, _p(d_seed), _p(d_counter), int(tag), int(count), _p(out),
                                         C.c_void_p(stream)), "frw_fr_draw_dev")
    return out


class Groth16Verifier:
    """ark-groth16's prepared verifying key + verify_proof (examples/pok_sig.rs:34-47).  Host code: no device involved -- unless
    `device` is given: the key is then loaded with frw_groth16_vk_load_dev (every gamma_abc_g1 point checked on that device, no
    vouching: points_are_checked must stay False) and prepare_inputs_dev / verify_dev run prepare_inputs there.

    vk: the dict WitnessEngine.groth16_setup returns, or one flat uint64 array in frw_groth16_setup's vk_out layout."""

    def __init__(self, vk, points_are_checked=False, device=None):
        self._lib = load_library()
        vk, self.num_instance = _vk_flat(vk, "Groth16Verifier")
        self.device = device
        self._h = C.c_void_p()
        flags = VK_POINTS_ARE_CHECKED if points_are_checked else 0
        if device is None:
            check(self._lib.frw_groth16_vk_load_opts(_p(vk), self.num_instance, flags, C.byref(self._h)), "frw_groth16_vk_load")
        else:
            check(self._lib.frw_groth16_vk_load_dev(int(device), _p(vk), self.num_instance, flags, C.byref(self._h)),
                  "frw_groth16_vk_load_dev")

    def verify(self, instance, proofs, encoding=ENC_MONTGOMERY, flags=0):
        """instance: uint64[batch, num_instance, 4] as the witness entry points write it (the constant one first);
        proofs: uint64[batch, 48].  Returns int32[batch]: 1 accepted, 0 rejected, -1 malformed."""
        proofs = np.ascontiguousarray(proofs).view(np.uint64).reshape(-1, 48)
        instance = np.ascontiguousarray(instance).view(np.uint64).reshape(proofs.shape[0], self.num_instance, 4)
        out = np.zeros(proofs.shape[0], dtype=np.int32)
        check(self._lib.frw_groth16_verify(self._h, proofs.shape[0], _p(instance), int(encoding), _p(proofs), int(flags), _p(out)),
              "frw_groth16_verify")
        return out

    def workspace_bytes(self, batch_in_flight):
        """Device workspace for `batch_in_flight` proofs (frw_groth16_verify_workspace_bytes; 0 for a host-only key)."""
        return int(self._lib.frw_groth16_verify_workspace_bytes(self._h, int(batch_in_flight)))

    def prepare_inputs_dev(self, d_instance, encoding=ENC_MONTGOMERY, stream=0, workspace=None):
        """d_instance: device tensor [batch, num_instance, 4] of 64-bit limbs -> (prepared int64[batch, 12] in ark-ff's bytes,
        status int32[batch]: 0 or -1 malformed), device tensors, ordered on `stream`."""
        batch = d_instance.shape[0]
        dev = d_instance.device
        prepared = _empty((batch, 12), "int64", dev)
        status = _empty(batch, "int32", dev)
        ws, ws_bytes = _workspace(workspace, self.device, 16, self.workspace_bytes, batch)
        check(self._lib.frw_groth16_prepare_inputs_dev(self._h, batch, _p(d_instance), int(encoding), _p(prepared), _p(status), _p(ws),
                                                       ws_bytes, C.c_void_p(stream)), "frw_groth16_prepare_inputs_dev")
        return prepared, status

    def verify_dev(self, d_instance, d_proofs, encoding=ENC_MONTGOMERY, flags=0, stream=0, workspace=None):
        """verify() with the instance vectors [batch, num_instance, 4] and the proofs [batch, 48] in device memory (as the witness and
        prove entry points write them).  Returns numpy int32[batch], the values verify() gives for the same bytes; synchronises `stream`.
        workspace: a device tensor (16-byte aligned) or None for one of the whole batch."""
        batch = d_proofs.shape[0]
        out = np.zeros(batch, dtype=np.int32)
        ws, ws_bytes = _workspace(workspace, self.device, 16, self.workspace_bytes, batch)
        check(self._lib.frw_groth16_verify_dev(self._h, batch, _p(d_instance), int(encoding), _p(d_proofs), int(flags), _p(out), _p(ws),
                                               ws_bytes, C.c_void_p(stream)), "frw_groth16_verify_dev")
        return out

    def full_workspace_bytes(self, batch_in_flight, flags=0):
        """Device workspace of verify_full_dev for `batch_in_flight` proofs (0 for a host-only key)."""
        return int(self._lib.frw_groth16_verify_full_workspace_bytes(self._h, int(batch_in_flight), int(flags)))

    def verify_full_dev(self, d_instance, d_proofs, encoding=ENC_MONTGOMERY, flags=0, batched=False, seed=None, stream=0, workspace=None,
                        batch_passed=None):
        """The whole verification on the device (frw_groth16_verify_full_dev): prepare_inputs, the proof points' checks, the pairings.
        Returns a device int32 tensor [batch] with the values verify() gives for the same bytes, ordered on `stream`, without
        synchronising.  batched: the batched check first (FRW_VERIFY_BATCHED); seed: 4 uint64 (None: 32 fresh random bytes, drawn now,
        after the proofs); batch_passed: an optional device int32 tensor of one element that receives whether the batched check passed.
        workspace: a device tensor (16-byte aligned) or None for one of the whole batch."""
        batch = d_proofs.shape[0]
        out = _empty(batch, "int32", d_proofs.device)
        flags, seed_arr = _batched_seed(flags, batched, seed)
        ws, ws_bytes = _workspace(workspace, d_proofs.device, 16, self.full_workspace_bytes, batch, flags)
        check(self._lib.frw_groth16_verify_full_dev(self._h, batch, _p(d_instance), int(encoding), _p(d_proofs), flags, _p(seed_arr), _p(out),
                                                    _p(batch_passed), _p(ws), ws_bytes, C.c_void_p(stream)), "frw_groth16_verify_full_dev")
        return out

    @classmethod
    def from_wire(cls, data, device=None, compressed=True):
        """The key from ark-serialize's bytes (VerifyingKey::serialize / serialize_uncompressed; frw.h has the format): decoded and
        loaded with every point checked -- on the host (frw_groth16_vk_load_wire), or with `device` given gamma_abc_g1 decoded and
        checked there (frw_groth16_vk_load_wire_dev), the handle then serving the device verifiers too."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = C.c_void_p()
        self.device = device
        data = bytes(data)
        mode = _wire_mode(compressed)
        head = 336 if compressed else 672
        self.num_instance = int.from_bytes(data[head:head + 8], "little") if len(data) >= head + 8 else 0
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        if device is None:
            check(self._lib.frw_groth16_vk_load_wire(buf, len(data), mode, C.byref(self._h)), "frw_groth16_vk_load_wire")
        else:
            check(self._lib.frw_groth16_vk_load_wire_dev(int(device), buf, len(data), mode, C.byref(self._h)), "frw_groth16_vk_load_wire_dev")
        return self

    def wire_workspace_bytes(self, batch_in_flight, flags=0, compressed=True):
        """Device workspace of verify_wire_dev for `batch_in_flight` proofs (0 for a host-only key)."""
        return int(self._lib.frw_groth16_verify_wire_workspace_bytes(self._h, int(batch_in_flight), int(flags), _wire_mode(compressed)))

    def verify_wire_dev(self, d_instance, d_wire, compressed=True, encoding=ENC_MONTGOMERY, flags=0, batched=False, seed=None, stream=0,
                        workspace=None, batch_passed=None):
        """verify_full_dev with the proofs as ark-serialize's bytes (frw_groth16_verify_wire_dev): d_wire is a device uint8 tensor
        [batch, 192] (compressed) or [batch, 384]; decoded on the device, -1 where the bytes are malformed, otherwise
        verify_full_dev's verdict for the decoded proof.  Everything else as verify_full_dev."""
        batch = _wire_batch(d_wire, compressed, "verify_wire_dev")
        out = _empty(batch, "int32", d_wire.device)
        flags, seed_arr = _batched_seed(flags, batched, seed)
        ws, ws_bytes = _workspace(workspace, d_wire.device, 16, self.wire_workspace_bytes, batch, flags, compressed)
        check(self._lib.frw_groth16_verify_wire_dev(self._h, batch, _p(d_instance), int(encoding), _p(d_wire), _wire_mode(compressed), flags,
                                                    _p(seed_arr), _p(out), _p(batch_passed), _p(ws), ws_bytes, C.c_void_p(stream)),
              "frw_groth16_verify_wire_dev")
        return out

    def verify_statements_wire_dev(self, engine, logn, pk_bytes, nonces, msgs, wire, circuit=CIRCUIT_NTT, compressed=True, flags=0,
                                   batched=False, seed=None, stream=0):
        """Verification from what a verifier is sent and nothing else: the Falcon public keys' bytes, the signatures' 40-byte nonces
        (bytes 1 .. 40 of an encoded signature), the messages and the proofs' wire bytes (anything of batch x 192 or 384 bytes).  The
        statements are made on the device by `engine` (a WitnessEngine on this key's device: statement_from_bytes_dev) and go to
        verify_wire_dev as they are; batched / seed / flags are passed through.  Returns (statuses, verdicts), device int32 tensors
        [batch]: FRW_ST_* of the statement and 1 / 0 / -1 -- a refused statement is a zero-filled instance vector, hence -1."""
        d_wire = _wire_dev(wire, self.device)
        d_inst, d_status = engine.statement_from_bytes_dev(circuit, logn, pk_bytes, nonces, msgs, ENC_MONTGOMERY, stream)
        verdicts = self.verify_wire_dev(d_inst, d_wire, compressed, ENC_MONTGOMERY, flags, batched, seed, stream)
        return d_status, verdicts

    def verify_aggregate_wire_dev(self, engine, handle, pk_bytes, nonces, msgs, wire, compressed=True, flags=0, stream=0):
        """verify_statements_wire_dev for ONE aggregate proof: the statements' Falcon public keys, nonces and messages in statement
        order and the proof's wire bytes, nothing else.  The aggregate's instance vector is made on the device by `engine`
        (aggregate_statement_from_bytes_dev on `handle`, the constraint system this key was set up for) and goes to verify_wire_dev as
        it is.  Returns (statuses int32[count], verdict int32[1]) device tensors: a refused statement leaves zeros in its slots, an
        instance vector that is well formed and verifies against no proof."""
        d_wire = _wire_dev(wire, self.device)
        d_inst, d_status = engine.aggregate_statement_from_bytes_dev(handle, pk_bytes, nonces, msgs, ENC_MONTGOMERY, stream)
        verdict = self.verify_wire_dev(d_inst.reshape(1, -1, 4), d_wire, compressed, ENC_MONTGOMERY, flags, False, None, stream)
        return d_status, verdict

    def rerandomize(self, proofs, factors, flags=0):
        """ark-groth16's rerandomize_proof on the host (frw_groth16_rerandomize): A' = A / r1, B' = r1 B + r1 r2 delta_g2,
        C' = C + r2 A.  proofs: uint64[batch, 48]; factors: uint64[batch, 2, 4], r1 and r2 of every proof, any 256-bit values (taken
        modulo the group order).  Returns (proofs uint64[batch, 48], status int32[batch]): 0, -1 for a malformed proof, RERAND_ZERO_FACTOR
        where r1 or r2 is zero; a refused slot is all zero.  The new proofs are unlinkable to the old ones only for factors that are
        uniform, secret and fresh."""
        proofs = np.ascontiguousarray(proofs).view(np.uint64).reshape(-1, 48)
        batch = proofs.shape[0]
        factors = np.ascontiguousarray(factors).view(np.uint64).reshape(batch, 2, 4)
        out = np.zeros((batch, 48), dtype=np.uint64)
        status = np.zeros(batch, dtype=np.int32)
        check(self._lib.frw_groth16_rerandomize(self._h, batch, _p(proofs), _p(factors), int(flags), _p(out), _p(status)),
              "frw_groth16_rerandomize")
        return out, status

    def rerandomize_workspace_bytes(self, in_flight, wire_mode=None):
        """Device workspace of rerandomize_dev (wire_mode None) or rerandomize_wire_dev (WIRE_COMPRESSED / WIRE_UNCOMPRESSED) for
        `in_flight` proofs."""
        return int(self._lib.frw_groth16_rerandomize_workspace_bytes(self._h, int(in_flight), -1 if wire_mode is None else int(wire_mode)))

    def rerandomize_dev(self, d_proofs, d_factors, flags=0, out=None, stream=0, workspace=None):
        """rerandomize() on the device (frw_groth16_rerandomize_dev): d_proofs a device tensor [batch, 48] of 64-bit limbs, d_factors
        [batch, 2, 4].  Returns (proofs int64[batch, 48], status int32[batch]), device tensors, ordered on `stream`, nothing
        synchronised or allocated by the call itself: capture-safe when `out` and `workspace` are given.  out may be d_proofs (in
        place); workspace: a device tensor (16-byte aligned) or None for one of the whole batch -- a smaller one runs the batch in
        chunks."""
        batch = d_proofs.shape[0]
        if out is None:
            out = _empty((batch, 48), "int64", d_proofs.device)
        status = _empty(batch, "int32", d_proofs.device)
        ws, ws_bytes = _workspace(workspace, d_proofs.device, 16, self.rerandomize_workspace_bytes, batch)
        check(self._lib.frw_groth16_rerandomize_dev(self._h, batch, _p(d_proofs), _p(d_factors), int(flags), _p(out), _p(status), _p(ws),
                                                    ws_bytes, C.c_void_p(stream)), "frw_groth16_rerandomize_dev")
        return out, status

    def rerandomize_wire_dev(self, d_wire, d_factors, compressed=True, flags=0, out=None, stream=0, workspace=None):
        """rerandomize_dev with the proofs as ark-serialize's bytes, in and out (frw_groth16_rerandomize_wire_dev): d_wire a device
        uint8 tensor of batch x 192 (compressed) or 384 bytes.  Returns (bytes uint8[batch, 192 or 384], status int32[batch]); -1 also
        where the decoder refuses the bytes; a refused slot is all zero bytes.  out may be d_wire."""
        mode = _wire_mode(compressed)
        batch = _wire_batch(d_wire, compressed, "rerandomize_wire_dev")
        if out is None:
            out = _empty((batch, proof_wire_bytes(compressed)), "uint8", d_wire.device)
        status = _empty(batch, "int32", d_wire.device)
        ws, ws_bytes = _workspace(workspace, d_wire.device, 16, self.rerandomize_workspace_bytes, batch, mode)
        check(self._lib.frw_groth16_rerandomize_wire_dev(self._h, batch, _p(d_wire), mode, _p(d_factors), int(flags), _p(out), _p(status),
                                                         _p(ws), ws_bytes, C.c_void_p(stream)), "frw_groth16_rerandomize_wire_dev")
        return out, status

    def rerandomize_seeded_dev(self, d_proofs, d_seed, d_counter, d_factors=None, flags=0, out=None, stream=0, workspace=None):
        """rerandomize_dev with the factors drawn on the device (frw_groth16_rerandomize_seeded_dev): one draw of 2 x batch scalars
        for (d_seed, d_counter, DRAW_RERANDOMIZE) into d_factors (int64[batch, 2, 4]; None: a fresh tensor), the re-randomisation,
        and the counter advanced by one.  Returns (proofs, status, d_factors).  Capture-safe when d_factors, out and workspace are
        given: every replay is a fresh re-randomisation."""
        batch = d_proofs.shape[0]
        if d_factors is None:
            d_factors = _empty((batch, 2, 4), "int64", d_proofs.device)
        if out is None:
            out = _empty((batch, 48), "int64", d_proofs.device)
        status = _empty(batch, "int32", d_proofs.device)
        ws, ws_bytes = _workspace(workspace, d_proofs.device, 16, self.rerandomize_workspace_bytes, batch)
        check(self._lib.frw_groth16_rerandomize_seeded_dev(self._h, batch, _p(d_proofs), _p(d_seed), _p(d_counter), _p(d_factors), int(flags),
                                                           _p(out), _p(status), _p(ws), ws_bytes, C.c_void_p(stream)),
              "frw_groth16_rerandomize_seeded_dev")
        return out, status, d_factors

    def rerandomize_wire_seeded_dev(self, d_wire, d_seed, d_counter, d_factors=None, compressed=True, flags=0, out=None, stream=0, workspace=None):
        """rerandomize_wire_dev with the factors drawn on the device (frw_groth16_rerandomize_wire_seeded_dev), as
        rerandomize_seeded_dev.  Returns (bytes, status, d_factors)."""
        mode = _wire_mode(compressed)
        batch = _wire_batch(d_wire, compressed, "rerandomize_wire_seeded_dev")
        if d_factors is None:
            d_factors = _empty((batch, 2, 4), "int64", d_wire.device)
        if out is None:
            out = _empty((batch, proof_wire_bytes(compressed)), "uint8", d_wire.device)
        status = _empty(batch, "int32", d_wire.device)
        ws, ws_bytes = _workspace(workspace, d_wire.device, 16, self.rerandomize_workspace_bytes, batch, mode)
        check(self._lib.frw_groth16_rerandomize_wire_seeded_dev(self._h, batch, _p(d_wire), mode, _p(d_seed), _p(d_counter), _p(d_factors),
                                                                int(flags), _p(out), _p(status), _p(ws), ws_bytes, C.c_void_p(stream)),
              "frw_groth16_rerandomize_wire_seeded_dev")
        return out, status, d_factors

    def close(self):
        if self._h:
            self._lib.frw_groth16_vk_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def proofs_to_wire(proofs, compressed=True):
    """Proofs in limbs (uint64[batch, 48], as the prover writes them) -> (uint8[batch, 192 or 384] in ark-serialize's format, what
    Proof::deserialize / deserialize_uncompressed reads; int32[batch] status: -1 and zero bytes where a coordinate's limbs are >= q).
    Host code (frw_groth16_proofs_to_wire)."""
    proofs = np.ascontiguousarray(proofs).view(np.uint64).reshape(-1, 48)
    out = np.zeros((proofs.shape[0], proof_wire_bytes(compressed)), dtype=np.uint8)
    status = np.zeros(proofs.shape[0], dtype=np.int32)
    check(load_library().frw_groth16_proofs_to_wire(proofs.shape[0], _p(proofs), _wire_mode(compressed), _p(out), _p(status)),
          "frw_groth16_proofs_to_wire")
    return out, status


def proofs_from_wire(wire, compressed=True):
    """ark-serialize's bytes (anything of batch x 192 or 384 bytes) -> (uint64[batch, 48] limbs, int32[batch] status: -1 and zero limbs
    where the bytes are malformed).  Host code (frw_groth16_proofs_from_wire)."""
    per = proof_wire_bytes(compressed)
    wire = np.ascontiguousarray(np.frombuffer(wire, dtype=np.uint8) if isinstance(wire, (bytes, bytearray)) else wire, dtype=np.uint8).reshape(-1, per)
    out = np.zeros((wire.shape[0], 48), dtype=np.uint64)
    status = np.zeros(wire.shape[0], dtype=np.int32)
    check(load_library().frw_groth16_proofs_from_wire(wire.shape[0], _p(wire), _wire_mode(compressed), _p(out), _p(status)),
          "frw_groth16_proofs_from_wire")
    return out, status


def proofs_to_wire_dev(d_proofs, compressed=True, stream=0):
    """proofs_to_wire on the device of `d_proofs` (a device tensor [batch, 48] of 64-bit limbs): (uint8[batch, 192 or 384], int32[batch])
    device tensors, ordered on `stream`, the host function's bytes."""
    batch = d_proofs.shape[0]
    out = _empty((batch, proof_wire_bytes(compressed)), "uint8", d_proofs.device)
    status = _empty(batch, "int32", d_proofs.device)
    check(load_library().frw_groth16_proofs_to_wire_dev(d_proofs.device.index or 0, batch, _p(d_proofs), _wire_mode(compressed), _p(out),
                                                        _p(status), C.c_void_p(stream)), "frw_groth16_proofs_to_wire_dev")
    return out, status


def proofs_from_wire_dev(d_wire, compressed=True, stream=0):
    """proofs_from_wire on the device of `d_wire` (a contiguous device uint8 tensor of batch x 192 or 384 bytes): (int64[batch, 48] limbs,
    int32[batch] status) device tensors, ordered on `stream`, the host function's values."""
    batch = _wire_batch(d_wire, compressed, "proofs_from_wire_dev")
    out = _empty((batch, 48), "int64", d_wire.device)
    status = _empty(batch, "int32", d_wire.device)
    check(load_library().frw_groth16_proofs_from_wire_dev(d_wire.device.index or 0, batch, _p(d_wire), _wire_mode(compressed), _p(out),
                                                          _p(status), C.c_void_p(stream)), "frw_groth16_proofs_from_wire_dev")
    return out, status


def vk_to_wire(vk, compressed=True):
    """A verifying key in limbs (the dict WitnessEngine.groth16_setup returns, or the flat uint64 array of frw_groth16_setup's vk_out)
    -> bytes in ark-serialize's format (what VerifyingKey::deserialize reads): 344 + 48 n or 680 + 96 n bytes."""
    vk, n = _vk_flat(vk, "vk_to_wire")
    lib = load_library()
    out = np.zeros(lib.frw_groth16_vk_wire_bytes(n, _wire_mode(compressed)), dtype=np.uint8)
    check(lib.frw_groth16_vk_to_wire(_p(vk), n, _wire_mode(compressed), _p(out)), "frw_groth16_vk_to_wire")
    return out.tobytes()


PK_POINTS_ARE_CHECKED = 1                           # frw.h FRW_PK_POINTS_ARE_CHECKED: skip the subgroup ladders of a key the caller made itself


def groth16_pk_wire_bytes(num_instance, num_witness, domain_size, compressed=True):
    """Bytes of an ark-groth16 ProvingKey with these counts (I with the constant one, W, n) in ark-serialize's format; 0 for counts no key has."""
    return int(load_library().frw_groth16_pk_wire_bytes(int(num_instance), int(num_witness), int(domain_size), _wire_mode(compressed)))


def groth16_pk_wire_info(data, compressed=True):
    """The framing of a serialised ProvingKey, read on the host without decoding a point (frw_groth16_pk_wire_info): a dict of
    num_instance, num_witness, domain_size and the byte offset of the first point of each of the five queries.  FrwError
    (FRW_E_INVALID_ARG) for bytes that are no key: truncated, over-long, lengths that disagree."""
    from ._lib import Groth16PkWireInfoStruct
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = Groth16PkWireInfoStruct()
    check(load_library().frw_groth16_pk_wire_info(_p(buf), buf.size, _wire_mode(compressed), C.byref(info)), "frw_groth16_pk_wire_info")
    return {name: int(getattr(info, name)) for name, _ in Groth16PkWireInfoStruct._fields_}


def diag_pairing(g1, g2):
    """The verifier's pairing of one pair (ark-ff limbs: 12 and 24 uint64): uint64[12, 6], see frw.h."""
    g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(12)
    g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(24)
    out = np.zeros((12, 6), dtype=np.uint64)
    check(load_library().frw_diag_pairing(_p(g1), _p(g2), _p(out)), "frw_diag_pairing")
    return out


def diag_pairing_dev(g1, g2, device=0):
    """diag_pairing for many pairs at once on `device` (frw_diag_pairing_dev): g1 uint64[count, 12], g2 uint64[count, 24] ->
    uint64[count, 12, 6].  No device is an error (FrwError, FRW_E_NO_DEVICE), never a host fallback."""
    g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 12)
    g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(-1, 24)
    if g1.shape[0] != g2.shape[0]:
        raise FrwError("diag_pairing_dev: as many G1 as G2 points")
    out = np.zeros((g1.shape[0], 12, 6), dtype=np.uint64)
    check(load_library().frw_diag_pairing_dev(int(device), g1.shape[0], _p(g1), _p(g2), _p(out)), "frw_diag_pairing_dev")
    return out


def _u16(a, n):
    a = np.ascontiguousarray(a, dtype=np.uint16)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != n:
        raise ValueError("input length %s is not N=%d" % (a.shape, n))   # poly.rs:110-112 panics likewise
    return a


class WitnessEngine:
    """One context on one HIP device.  Raises FrwError when no device is usable."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        check(self._lib.frw_ctx_create(int(device), C.byref(h)), "frw_ctx_create")
        self._ctx = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.frw_ctx_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def host_allocations(self):
        """Device / page-locked allocations the host-buffer entry points of this context have made so far."""
        n = C.c_uint64()
        check(self._lib.frw_diag_host_allocations(self._ctx, C.byref(n)), "frw_diag_host_allocations")
        return int(n.value)

    def valu_rates(self):
        """{v_add_u32, v_mad_u64_u32: wave-instructions / SIMD / us; f29_mul_products_per_s; simds} measured now."""
        out = (C.c_double * 4)()
        check(self._lib.frw_diag_valu_rates(self._ctx, C.byref(out)), "frw_diag_valu_rates")
        return {"v_add_u32": out[0], "v_mad_u64_u32": out[1], "f29_mul_products_per_s": out[2], "simds": int(out[3])}

    def trim(self):
        """Gives the working memory of the host-buffer entry points back to the device (the next call allocates again)."""
        check(self._lib.frw_ctx_trim(self._ctx), "frw_ctx_trim")

    def pinned_empty(self, shape, dtype):
        """numpy array over page-locked host memory (frw_host_alloc); freed when the array is collected."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        ptr = C.c_void_p()
        check(self._lib.frw_host_alloc(self._ctx, nbytes, C.byref(ptr)), "frw_host_alloc")
        buf = (C.c_char * max(nbytes, 1)).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        weakref.finalize(buf, self._lib.frw_host_free, None, C.c_void_p(ptr.value))     # may outlive this engine
        return arr

    # ---- host buffers ------------------------------------------------------------------
    def witness_dual_ntt_verify(self, logn, sig, pk, hm, encoding=ENC_MONTGOMERY, strict=True):
        """FalconDualNTTVerificationCircuit (falcon_dual_ntt.rs:26-132); same conventions as witness_ntt_verify."""
        return self.witness_ntt_verify(logn, sig, pk, hm, encoding, strict, dual=True)

    def witness_schoolbook_verify(self, logn, sig, pk, hm, encoding=ENC_MONTGOMERY, strict=True):
        """FalconSchoolBookVerificationCircuit (falcon_schoolbook.rs:26-131); same conventions as witness_ntt_verify
        (instance = [1, pk, hm] coefficients; 10.0 / 36.8 MB of witness per signature)."""
        return self._witness_host(CIRCUIT_SCHOOLBOOK, logn, sig, pk, hm, encoding, strict, False)

    def witness_ntt_verify(self, logn, sig, pk, hm, encoding=ENC_MONTGOMERY, strict=True, dual=False, pinned=False):
        """-> (witness u64[batch, W, 4], instance u64[batch, I, 4], status i32[batch]).
        pinned=True puts the outputs in page-locked memory so that the D2H copies overlap with the kernels."""
        return self._witness_host(CIRCUIT_DUAL_NTT if dual else CIRCUIT_NTT, logn, sig, pk, hm, encoding, strict, pinned)

    def _witness_host(self, circuit, logn, sig, pk, hm, encoding, strict, pinned):
        L = circuit_layout(circuit, logn)
        sig, pk, hm = (_u16(a, L.n) for a in (sig, pk, hm))
        batch = sig.shape[0]
        if pk.shape[0] != batch or hm.shape[0] != batch:
            raise ValueError("batch mismatch")
        if pinned:
            wit = self.pinned_empty((batch, L.num_witness, 4), np.uint64)
            inst = self.pinned_empty((batch, L.num_instance, 4), np.uint64)
            st = self.pinned_empty((batch,), np.int32)
            st[:] = 0
        else:
            wit = np.zeros((batch, L.num_witness, 4), dtype=np.uint64)
            inst = np.zeros((batch, L.num_instance, 4), dtype=np.uint64)
            st = np.zeros(batch, dtype=np.int32)
        fn = (self._lib.frw_witness_ntt_verify, self._lib.frw_witness_dual_ntt_verify, self._lib.frw_witness_schoolbook_verify)[circuit]
        rc = fn(self._ctx, logn, batch, _p(sig), _p(pk), _p(hm), encoding, _p(wit), _p(inst), _p(st), 1 if strict else 0)
        _check_refusal(rc, "frw_witness_ntt_verify", st, "signature(s)", "failed range checks")
        return wit, inst, st

    def witness_ntt_verify_compact(self, logn, sig, pk, hm, strict=True, pinned=False):
        """Host-buffer entry point with FRW_ENC_COMPACT: -> (compact u8[batch, bytes_per_signature], status)."""
        CL = compact_layout(logn)
        sig, pk, hm = (_u16(a, CL.n) for a in (sig, pk, hm))
        batch = sig.shape[0]
        mk = (lambda shape, dt: self.pinned_empty(shape, dt)) if pinned else (lambda shape, dt: np.zeros(shape, dtype=dt))
        comp, st = mk((batch, CL.bytes_per_signature), np.uint8), mk((batch,), np.int32)
        rc = self._lib.frw_witness_ntt_verify(self._ctx, logn, batch, _p(sig), _p(pk), _p(hm), ENC_COMPACT, _p(comp), None, _p(st),
                                              1 if strict else 0)
        if rc == E_RANGE:
            raise FrwError(rc, "frw_witness_ntt_verify", "Invalid input: a signature failed its range checks")
        check(rc, "frw_witness_ntt_verify")
        return comp, st

    def expand_host(self, logn, compact):
        """frw_expand_host: compact u8[batch, bytes_per_signature] -> (witness u64[batch, W, 4], instance u64[batch, I, 4])."""
        L = layout(logn)
        compact = np.ascontiguousarray(compact, dtype=np.uint8)
        batch = compact.shape[0]
        wit = np.empty((batch, L.num_witness, 4), dtype=np.uint64)
        inst = np.empty((batch, L.num_instance, 4), dtype=np.uint64)
        check(self._lib.frw_expand_host(logn, batch, _p(compact), _p(wit), _p(inst)), "frw_expand_host")
        return wit, inst

    def field_encoding(self, p):
        """frw_ctx_field_encoding: registers the modulus p on this context (or finds it) -> the encoding to pass wherever
        ENC_MONTGOMERY goes in the witness, ntt_modq, gadget and statement calls: elements come out as x * 2^256 mod p."""
        if p < 0 or p >> 256:
            raise FrwError(-1, "frw_ctx_field_encoding", "the modulus does not fit four limbs")
        enc = C.c_int()
        check(self._lib.frw_ctx_field_encoding(self._ctx, _limbs4(p), C.byref(enc)), "frw_ctx_field_encoding")
        return int(enc.value)

    expand_field_host = staticmethod(expand_field_host)      # needs no device: also a module-level function

    def aggregate(self, items, encoding=ENC_MONTGOMERY, strict=True):
        """Aggregate driver (the reference's falcon-aggregate-sig is an empty stub, so the behaviour
        is defined here): a mixed batch of Falcon-512 / Falcon-1024 statements, each ``(logn, sig, pk, hm)``, is
        grouped by parameter set, each group goes through one batched engine call, and the results come back in
        input order as ``[(witness u64[W,4], instance u64[I,4], status)]``."""
        groups = {9: [], 10: []}
        for idx, (logn, sig, pk, hm) in enumerate(items):
            if logn not in groups:
                raise ValueError("logn must be 9 or 10")
            groups[logn].append((idx, sig, pk, hm))
        out = [None] * len(items)
        for logn, members in groups.items():
            if not members:
                continue
            sig, pk, hm = (np.stack([np.asarray(m[k], dtype=np.uint16) for m in members]) for k in (1, 2, 3))
            wit, inst, st = self.witness_ntt_verify(logn, sig, pk, hm, encoding, strict)
            for j, m in enumerate(members):
                out[m[0]] = (wit[j], inst[j], int(st[j]))
        return out

    def ntt_modq(self, logn, poly, encoding=ENC_MONTGOMERY):
        """NTTPolyVar::ntt_circuit alone -> (witness u64[batch, 29N, 4], ntt u16[batch, N], status)."""
        n = 1 << logn
        poly = _u16(poly, n)
        batch = poly.shape[0]
        wit = np.zeros((batch, 29 * n, 4), dtype=np.uint64)
        out = np.zeros((batch, n), dtype=np.uint16)
        st = np.zeros(batch, dtype=np.int32)
        check(self._lib.frw_ntt_modq(self._ctx, logn, batch, _p(poly), encoding, _p(wit), _p(out), _p(st)), "frw_ntt_modq")
        return wit, out, st

    def prepare_inputs(self, logn, pks, msgs, sigs):
        """(pk bytes, msg bytes, sig bytes) per signature -> (sig, pk, hm) uint16[batch, N] + status, i.e. what the
        reference derives with falcon-rust at falcon_ntt.rs:27-28,44 (decode + SHAKE256 hash-to-point, on the GPU)."""
        batch = len(pks)
        if len(msgs) != batch or len(sigs) != batch:
            raise ValueError("batch mismatch")
        sig_len = len(sigs[0]) if batch else SIG_LEN[logn]
        if any(len(p) != PK_LEN[logn] for p in pks) or any(len(s) != sig_len for s in sigs):
            raise ValueError("public keys must be %d bytes and signatures of one common length" % PK_LEN[logn])
        n = 1 << logn
        pkb, sgb, blob, off = _pack(pks, sigs, msgs)
        out = [np.zeros((batch, n), dtype=np.uint16) for _ in range(3)]
        st = np.zeros(batch, dtype=np.int32)
        check(self._lib.frw_prepare_inputs(self._ctx, logn, batch, _p(pkb), _p(sgb), sig_len, _p(blob), _p(off),
                                           _p(out[0]), _p(out[1]), _p(out[2]), _p(st)), "frw_prepare_inputs")
        return out[0], out[1], out[2], st

    # the three steps of prepare_inputs one by one, on device buffers (torch tensors or raw pointers); not synchronised
    def decode_signatures_dev(self, logn, batch, d_sig_bytes, sig_len, d_sig, d_nonce_out, d_status, stream=0):
        """frw_decode_signatures_dev: d_sig_bytes uint8[batch, sig_len] -> d_sig uint16[batch, N], d_nonce_out uint8[batch, 40] (or None),
        d_status int32[batch]: FRW_ST_OK or FRW_ST_DECODE.  The row of a refused signature is unspecified."""
        check(self._lib.frw_decode_signatures_dev(self._ctx, int(logn), batch, _p(d_sig_bytes), int(sig_len), _p(d_sig), _p(d_nonce_out),
                                                  _p(d_status), C.c_void_p(stream)), "frw_decode_signatures_dev")

    def decode_public_keys_dev(self, logn, batch, d_pk_bytes, d_pk, d_status, stream=0):
        """frw_decode_public_keys_dev: d_pk_bytes uint8[batch, PK_LEN[logn]] -> d_pk uint16[batch, N], d_status int32[batch]."""
        check(self._lib.frw_decode_public_keys_dev(self._ctx, int(logn), batch, _p(d_pk_bytes), _p(d_pk), _p(d_status), C.c_void_p(stream)),
              "frw_decode_public_keys_dev")

    def hash_to_point_dev(self, logn, batch, d_nonces, d_msgs, d_msg_off, d_hm, stream=0):
        """frw_hash_to_point_dev: d_nonces uint8[batch, 40], the messages as one blob d_msgs and its int64[batch + 1] non-decreasing offsets
        d_msg_off -> d_hm uint16[batch, N]."""
        check(self._lib.frw_hash_to_point_dev(self._ctx, int(logn), batch, _p(d_nonces), _p(d_msgs), _p(d_msg_off), _p(d_hm), C.c_void_p(stream)),
              "frw_hash_to_point_dev")

    def gadget(self, kind, a, b=None, encoding=ENC_MONTGOMERY):
        """Stand-alone gadget blocks (frw_gadget): a = python ints; returns (blocks u64[count, BLK, 4], status)."""
        blk = self._lib.frw_gadget_block_len(kind)
        if blk < 0:
            raise ValueError("unknown gadget kind %r" % (kind,))
        vals = [int(x) for x in a]
        count = len(vals)
        if kind == G_MOD_Q:
            if any(v >> 160 for v in vals):
                raise ValueError("mod_q input exceeds 160 bits (the ladder never produces more)")
            arr = np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(5)] for v in vals], dtype=np.uint32)
        else:
            arr = np.array(vals, dtype=np.uint64)
        barr = np.array([int(x) for x in b], dtype=np.uint64) if b is not None else None
        out = np.zeros((count, blk, 4), dtype=np.uint64)
        st = np.zeros(count, dtype=np.int32)
        check(self._lib.frw_gadget(self._ctx, kind, count, _p(arr), _p(barr), encoding, _p(out), _p(st)), "frw_gadget")
        return out, st

    # ---- device buffers (torch tensors or raw pointers) ---------------------------------
    _ptr = staticmethod(_p)

    def witness_ntt_verify_dev(self, logn, batch, d_sig, d_pk, d_hm, d_wit, d_inst, d_status,
                               encoding=ENC_MONTGOMERY, stream=0):
        check(self._lib.frw_witness_ntt_verify_dev(self._ctx, logn, batch, _p(d_sig), _p(d_pk), _p(d_hm), encoding, _p(d_wit), _p(d_inst),
                                                   _p(d_status), C.c_void_p(stream)), "frw_witness_ntt_verify_dev")

    def witness_ntt_verify_compact_dev(self, logn, batch, d_sig, d_pk, d_hm, d_compact, d_status, stream=0):
        """FRW_ENC_COMPACT producer: d_compact = batch x compact_layout(logn).bytes_per_signature bytes."""
        check(self._lib.frw_witness_ntt_verify_compact_dev(self._ctx, logn, batch, _p(d_sig), _p(d_pk), _p(d_hm), _p(d_compact),
                                                           _p(d_status), C.c_void_p(stream)), "frw_witness_ntt_verify_compact_dev")

    def expand_dev(self, logn, batch, d_compact, d_wit, d_inst, stream=0):
        """compact -> the arkworks witness / instance buffers (FRW_ENC_MONTGOMERY bytes)."""
        check(self._lib.frw_expand_dev(self._ctx, logn, batch, _p(d_compact), _p(d_wit), _p(d_inst), C.c_void_p(stream)), "frw_expand_dev")

    def expand_field_dev(self, logn, batch, d_compact, encoding, d_wit, d_inst, stream=0):
        """compact -> the witness / instance buffers over a field registered with field_encoding."""
        check(self._lib.frw_expand_field_dev(self._ctx, logn, batch, _p(d_compact), encoding, _p(d_wit), _p(d_inst), C.c_void_p(stream)),
              "frw_expand_field_dev")

    def launch_shape(self, logn, batch, encoding=ENC_MONTGOMERY):
        """{grid, resident workgroups per CU, CUs, split_signatures} of a witness launch of `batch` signatures
        (split_signatures = the ragged tail beyond the last full round of the grid, cut into five work items each)."""
        out = (C.c_int32 * 4)()
        check(self._lib.frw_diag_launch_shape(self._ctx, logn, encoding, batch, C.byref(out)), "frw_diag_launch_shape")
        return {"grid": out[0], "resident_per_cu": out[1], "cus": out[2], "split_signatures": out[3]}

    def witness_dual_ntt_verify_dev(self, logn, batch, d_sig, d_pk, d_hm, d_wit, d_inst, d_status,
                                    encoding=ENC_MONTGOMERY, stream=0):
        check(self._lib.frw_witness_dual_ntt_verify_dev(self._ctx, logn, batch, _p(d_sig), _p(d_pk), _p(d_hm), encoding, _p(d_wit),
                                                        _p(d_inst), _p(d_status), C.c_void_p(stream)), "frw_witness_dual_ntt_verify_dev")

    def witness_schoolbook_verify_dev(self, logn, batch, d_sig, d_pk, d_hm, d_wit, d_inst, d_status,
                                      encoding=ENC_MONTGOMERY, stream=0):
        check(self._lib.frw_witness_schoolbook_verify_dev(self._ctx, logn, batch, _p(d_sig), _p(d_pk), _p(d_hm), encoding, _p(d_wit),
                                                          _p(d_inst), _p(d_status), C.c_void_p(stream)), "frw_witness_schoolbook_verify_dev")

    def ntt_modq_dev(self, logn, batch, d_poly, d_wit, d_ntt, d_status, encoding=ENC_MONTGOMERY, stream=0):
        check(self._lib.frw_ntt_modq_dev(self._ctx, logn, batch, _p(d_poly), encoding, _p(d_wit), _p(d_ntt), _p(d_status),
                                         C.c_void_p(stream)), "frw_ntt_modq_dev")

    def diag_write_stream_dev(self, d_buf, nbytes, slab_bytes, stream=0):
        check(self._lib.frw_diag_write_stream_dev(self._ctx, _p(d_buf), nbytes, slab_bytes, C.c_void_p(stream)),
              "frw_diag_write_stream_dev")

    def r1cs_load(self, circuit, logn):
        """Device-resident A/B/C of circuit 0 (NTT) / 1 (dual NTT) / 2 (schoolbook) for r1cs_check_dev; free with r1cs_free."""
        h = C.c_void_p()
        check(self._lib.frw_r1cs_load(self.device, circuit, logn, C.byref(h)), "frw_r1cs_load")
        return h

    def r1cs_load_csr(self, num_instance, num_witness, matrices):
        """A handle for ANY constraint system: matrices = three (row_ptr uint64[C + 1], col uint32[nnz], val uint64[nnz][4] canonical)
        for A, B, C -- the arrays of the FRWR1CS1 file (column 0 the constant one, 1 .. I - 1 the public inputs, I + k witness k).  The
        handle goes wherever an r1cs_load handle goes but into the calls that start from Falcon signatures; free with r1cs_free."""
        counts, three, _arrays = _csr_arrays(num_instance, num_witness, matrices)
        h = C.c_void_p()
        check(self._lib.frw_r1cs_load_csr(self.device, counts, *three, C.byref(h)), "frw_r1cs_load_csr")
        return h

    def r1cs_load_file(self, path):
        """The same from an FRWR1CS1 file (what r1cs_export writes, or any system written in that layout)."""
        h = C.c_void_p()
        check(self._lib.frw_r1cs_load_file(self.device, os.fsencode(str(path)), C.byref(h)), "frw_r1cs_load_file")
        return h

    def r1cs_free(self, handle):
        self._lib.frw_r1cs_free(handle)

    # ---- the check and the products over any four-limb field (frw_r1csf_*): a handle made for a modulus ----
    def r1csf_load(self, circuit, logn, p):
        """The matrices of circuit 0 / 1 / 2 carried over to the modulus p (their centred lift, reduced), on the device; free with
        r1csf_free.  The handle goes into r1csf_check_dev only."""
        h = C.c_void_p()
        check(self._lib.frw_r1csf_load(self.device, circuit, logn, _modulus(p, "frw_r1csf_load"), C.byref(h)), "frw_r1csf_load")
        return h

    def r1csf_load_csr(self, p, num_instance, num_witness, matrices):
        """r1cs_load_csr over the modulus p: the values canonical mod p."""
        counts, three, _arrays = _csr_arrays(num_instance, num_witness, matrices)
        h = C.c_void_p()
        check(self._lib.frw_r1csf_load_csr(self.device, _modulus(p, "frw_r1csf_load_csr"), counts, *three, C.byref(h)), "frw_r1csf_load_csr")
        return h

    def r1csf_load_file(self, p, path):
        """The same from an FRWR1CS1 file (what r1cs_export_field writes; the file does not record the modulus)."""
        h = C.c_void_p()
        check(self._lib.frw_r1csf_load_file(self.device, _modulus(p, "frw_r1csf_load_file"), os.fsencode(str(path)), C.byref(h)),
              "frw_r1csf_load_file")
        return h

    def r1csf_free(self, handle):
        self._lib.frw_r1csf_free(handle)

    def r1csf_info(self, handle):
        from ._lib import R1csfInfoStruct
        q = R1csfInfoStruct()
        check(self._lib.frw_r1csf_info(handle, C.byref(q)), "frw_r1csf_info")
        return q

    def r1csf_scratch_bytes(self, handle, batch, with_products):
        return int(self._lib.frw_r1csf_scratch_bytes(handle, batch, 1 if with_products else 0))

    def r1csf_check_dev(self, handle, batch, d_wit, d_inst, d_num_unsatisfied, d_first_unsatisfied=None, d_abc=None, d_scratch=None,
                        scratch_bytes=0, stream=0):
        """is_satisfied() / which_is_unsatisfied() of every statement over the handle's field, and (d_abc: int64[batch, 3, C, 4]) A z, B z,
        C z in Montgomery form over it.  Allocates nothing: d_scratch holds r1csf_scratch_bytes(handle, batch, d_abc is not None)."""
        check(self._lib.frw_r1csf_check_dev(handle, batch, _p(d_wit), _p(d_inst), _p(d_num_unsatisfied), _p(d_first_unsatisfied), _p(d_abc),
                                            _p(d_scratch), scratch_bytes, C.c_void_p(stream)), "frw_r1csf_check_dev")

    # ---- the QAP witness map over the handle's field (frw_qapf_*) ----
    def qapf_create(self, r1csf_handle, generator):
        """The witness map of an r1csf_load* handle over its field's radix-2 domain, the coset by `generator`; the r1csf handle must
        outlive this one.  Free with qapf_free."""
        h = C.c_void_p()
        check(self._lib.frw_qapf_create(r1csf_handle, _modulus(generator, "frw_qapf_create"), C.byref(h)), "frw_qapf_create")
        return h

    def qapf_free(self, handle):
        self._lib.frw_qapf_free(handle)

    def qapf_info(self, handle):
        """-> the QapfInfoStruct: .domain (limbs; qapf_domain gives integers), num_constraints, num_instance, num_passes,
        workspace_bytes_per_statement"""
        from ._lib import QapfInfoStruct
        q = QapfInfoStruct()
        check(self._lib.frw_qapf_info(handle, C.byref(q)), "frw_qapf_info")
        return q

    def qapf_witness_map_dev(self, handle, batch, d_wit, d_inst, d_h, d_workspace, workspace_bytes, d_num_unsatisfied=None, stream=0):
        """h = (A B - C) / (X^n - 1) of every statement over the handle's field: d_h int64[batch, n, 4], Montgomery form over p.
        Allocates nothing; the batch goes through d_workspace in chunks of as many statements as it holds."""
        check(self._lib.frw_qapf_witness_map_dev(handle, batch, _p(d_wit), _p(d_inst), _p(d_h), _p(d_num_unsatisfied), _p(d_workspace),
                                                 workspace_bytes, C.c_void_p(stream)), "frw_qapf_witness_map_dev")

    # ---- the sum over a run-time curve y^2 = x^3 + b (frw_msmf_*) ----
    def msmf_load(self, q, r, b, bases, flags=0):
        """The bases of a multi-scalar multiplication on this engine's device: uint64[n, 8] affine points, Montgomery limbs over q, all
        zero the point at infinity; every base is checked to be on the curve unless flags has MSMF_POINTS_ARE_CHECKED.  Free with
        msmf_free."""
        pts = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
        h = C.c_void_p()
        check(self._lib.frw_msmf_load(self.device, C.byref(_curve(q, r, b, "frw_msmf_load")), pts.shape[0], _p(pts), int(flags), C.byref(h)),
              "frw_msmf_load")
        return h

    def msmf_free(self, handle):
        self._lib.frw_msmf_free(handle)

    def msmf_info(self, handle):
        """-> the MsmfInfoStruct: num_points, window_bits, num_windows, bases_bytes, workspace_bytes_per_statement"""
        from ._lib import MsmfInfoStruct
        m = MsmfInfoStruct()
        check(self._lib.frw_msmf_info(handle, C.byref(m)), "frw_msmf_info")
        return m

    def msmf_workspace_bytes(self, handle, batch_in_flight):
        return int(self._lib.frw_msmf_workspace_bytes(handle, int(batch_in_flight)))

    def msmf_dev(self, handle, batch, d_scalars, scalar_stride, num_scalars, montgomery, d_out, d_workspace, workspace_bytes, stream=0):
        """d_out[s] = sum_{i < num_scalars} k[s, i] P_i for every statement: d_scalars int64[batch, scalar_stride, 4] (plain integers, or with
        `montgomery` ark-ff's form over r, as qapf_witness_map_dev writes h), d_out int64[batch, 8].  Allocates nothing; the batch goes
        through d_workspace in chunks of as many statements as it holds."""
        check(self._lib.frw_msmf_dev(handle, batch, _p(d_scalars), scalar_stride, num_scalars, 1 if montgomery else 0, _p(d_out), _p(d_workspace),
                                     workspace_bytes, C.c_void_p(stream)), "frw_msmf_dev")

    # ---- the same sum over G2: a curve y^2 = x^3 + b' over a run-time Fq2 (frw_msmf2_*) ----
    def msmf2_load(self, q, r, nonresidue, b, bases, flags=0):
        """The bases of a multi-scalar multiplication over Fq2 = Fq[u] / (u^2 - nonresidue) on this engine's device: uint64[n, 16] affine
        points (x.c0, x.c1, y.c0, y.c1; Montgomery limbs over q), all zero the point at infinity; every base is checked to be on the curve
        unless flags has MSMF_POINTS_ARE_CHECKED.  There is no subgroup check.  Free with msmf2_free."""
        pts = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 16)
        h = C.c_void_p()
        check(self._lib.frw_msmf2_load(self.device, C.byref(_curve2(q, r, nonresidue, b, "frw_msmf2_load")), pts.shape[0], _p(pts), int(flags),
                                       C.byref(h)), "frw_msmf2_load")
        return h

    def msmf2_free(self, handle):
        self._lib.frw_msmf2_free(handle)

    def msmf2_info(self, handle):
        """-> the Msmf2InfoStruct: num_points, window_bits, num_windows, bases_bytes, workspace_bytes_per_statement"""
        from ._lib import Msmf2InfoStruct
        m = Msmf2InfoStruct()
        check(self._lib.frw_msmf2_info(handle, C.byref(m)), "frw_msmf2_info")
        return m

    def msmf2_workspace_bytes(self, handle, batch_in_flight):
        return int(self._lib.frw_msmf2_workspace_bytes(handle, int(batch_in_flight)))

    def msmf2_dev(self, handle, batch, d_scalars, scalar_stride, num_scalars, montgomery, d_out, d_workspace, workspace_bytes, stream=0):
        """d_out[s] = sum_{i < num_scalars} k[s, i] Q_i for every statement: msmf_dev's contract, d_out int64[batch, 16]."""
        check(self._lib.frw_msmf2_dev(handle, batch, _p(d_scalars), scalar_stride, num_scalars, 1 if montgomery else 0, _p(d_out), _p(d_workspace),
                                      workspace_bytes, C.c_void_p(stream)), "frw_msmf2_dev")

    def r1cs_load_aggregate(self, logns):
        """The constraint system of an aggregate statement: FalconNTTVerificationCircuit once per entry of `logns` (9 / 10, in
        order) on one system.  The handle goes wherever an r1cs_load handle goes; its witness / instance vectors are the
        aggregate's own (aggregate_assign_dev makes them).  Free with r1cs_free."""
        arr = np.ascontiguousarray(logns, dtype=np.int32)
        h = C.c_void_p()
        check(self._lib.frw_r1cs_load_aggregate(self.device, len(arr), _p(arr), C.byref(h)), "frw_r1cs_load_aggregate")
        return h

    def r1cs_info(self, handle):
        from ._lib import R1csInfoStruct
        q = R1csInfoStruct()
        check(self._lib.frw_r1cs_info(handle, C.byref(q)), "frw_r1cs_info")
        return q

    def aggregate_assign_dev(self, handle, d_wit512, d_inst512, d_wit1024, d_inst1024, d_wit, d_inst, stream=0):
        """instance_assignment / witness_assignment of the aggregate from the per-parameter-set batches of the witness entry points
        (either pair may be None when the aggregate has no such statement)."""
        check(self._lib.frw_aggregate_assign_dev(handle, _p(d_wit512), _p(d_inst512), _p(d_wit1024), _p(d_inst1024), _p(d_wit), _p(d_inst),
                                                 C.c_void_p(stream)), "frw_aggregate_assign_dev")

    # ---- the verifier's statement: instance vectors without a signature -----------------------------------------------------------
    def statement_dev(self, circuit, logn, batch, d_pk, d_hm, d_inst, d_status, encoding=ENC_MONTGOMERY, stream=0):
        """instance_assignment of `batch` statements from (pk, hm) in device memory (frw_statement_dev): the bytes the witness entry
        points write to d_inst for the same pk and hm, without a signature and without a witness."""
        check(self._lib.frw_statement_dev(self._ctx, int(circuit), int(logn), batch, _p(d_pk), _p(d_hm), int(encoding), _p(d_inst),
                                          _p(d_status), C.c_void_p(stream)), "frw_statement_dev")

    def statement(self, circuit, logn, pk, hm, encoding=ENC_MONTGOMERY, strict=True):
        """Host buffers (frw_statement): pk, hm uint16[batch, N] -> (instance u64[batch, 2 N + 1, 4], status i32[batch])."""
        n = 1 << logn
        pk, hm = _u16(pk, n), _u16(hm, n)
        batch = pk.shape[0]
        if hm.shape[0] != batch:
            raise ValueError("batch mismatch")
        inst = np.zeros((batch, 2 * n + 1, 4), dtype=np.uint64)
        st = np.zeros(batch, dtype=np.int32)
        rc = self._lib.frw_statement(self._ctx, int(circuit), int(logn), batch, _p(pk), _p(hm), int(encoding), _p(inst), _p(st),
                                     1 if strict else 0)
        _check_refusal(rc, "frw_statement", st, "statement(s)")
        return inst, st

    @staticmethod
    def _statement_bytes(logn, pk_bytes, nonces, msgs):
        batch = len(pk_bytes)
        if len(nonces) != batch or len(msgs) != batch:
            raise ValueError("batch mismatch")
        if any(len(k) != PK_LEN[logn] for k in pk_bytes) or any(len(x) != NONCE_LEN for x in nonces):
            raise ValueError("public keys must be %d bytes and nonces %d" % (PK_LEN[logn], NONCE_LEN))
        return (batch, *_pack(pk_bytes, nonces, msgs))

    def statement_workspace_bytes(self, logn, batch):
        return int(self._lib.frw_statement_workspace_bytes(int(logn), int(batch)))

    def statement_from_bytes(self, circuit, logn, pk_bytes, nonces, msgs, encoding=ENC_MONTGOMERY, strict=True):
        """Host buffers (frw_statement_from_bytes): lists of encoded public keys, 40-byte nonces and messages -> (instance, status);
        FRW_ST_DECODE and a zero-filled slot for a malformed key."""
        batch, pkb, non, blob, off = self._statement_bytes(logn, pk_bytes, nonces, msgs)
        n = 1 << logn
        inst = np.zeros((batch, 2 * n + 1, 4), dtype=np.uint64)
        st = np.zeros(batch, dtype=np.int32)
        rc = self._lib.frw_statement_from_bytes(self._ctx, int(circuit), int(logn), batch, _p(pkb), _p(non), _p(blob), _p(off), int(encoding),
                                                _p(inst), _p(st), 1 if strict else 0)
        _check_refusal(rc, "frw_statement_from_bytes", st, "statement(s)")
        return inst, st

    def statement_from_bytes_dev(self, circuit, logn, pk_bytes, nonces, msgs, encoding=ENC_MONTGOMERY, stream=0, workspace=None):
        """The same on the device (frw_statement_from_bytes_dev): the bytes are uploaded, the key decoder, SHAKE256 and the statement
        kernel run on `stream`.  -> (instance int64[batch, 2 N + 1, 4], status int32[batch]) device tensors, not synchronised.
        pk_bytes may be a device uint8 tensor [batch, PK_LEN] with nonces a device uint8 tensor [batch, 40], msgs a (blob, offsets)
        pair of device tensors (uint8, int64[batch + 1]): nothing is uploaded then."""
        batch, _, d_pkb, d_non, d_blob, d_off = _encoded_dev(self.device, logn, pk_bytes, nonces, msgs, NONCE_LEN, self._statement_bytes)
        n = 1 << logn
        d_inst = _empty((batch, 2 * n + 1, 4), "int64", self.device)
        d_status = _empty(batch, "int32", self.device)
        ws, ws_bytes = _workspace(workspace, self.device, 16, self.statement_workspace_bytes, logn, batch)
        check(self._lib.frw_statement_from_bytes_dev(self._ctx, int(circuit), int(logn), batch, _p(d_pkb), _p(d_non), _p(d_blob), _p(d_off),
                                                     int(encoding), _p(d_inst), _p(d_status), _p(ws), ws_bytes, C.c_void_p(stream)),
              "frw_statement_from_bytes_dev")
        return d_inst, d_status

    def aggregate_statement_dev(self, handle, d_pk512, d_hm512, d_pk1024, d_hm1024, d_inst, d_status, encoding=ENC_MONTGOMERY, stream=0):
        """instance_assignment of the aggregate from the statements' keys and hashed messages, per parameter set in statement order
        (either pair may be None): aggregate_assign_dev's d_inst without a witness.  d_status: int32[num_statements]."""
        check(self._lib.frw_aggregate_statement_dev(handle, self._ctx, _p(d_pk512), _p(d_hm512), _p(d_pk1024), _p(d_hm1024), int(encoding),
                                                    _p(d_inst), _p(d_status), C.c_void_p(stream)), "frw_aggregate_statement_dev")

    # ---- Falcon verification: verdicts and norms without a witness -------------------------------------------------------------------
    def falcon_verify_dev(self, logn, batch, d_sig, d_pk, d_hm, d_status, d_norm=None, rule=RULE_CIRCUIT, stream=0):
        """The verdicts of `batch` signatures from (sig, pk, hm) in device memory (frw_falcon_verify_dev): d_status int32[batch] is FRW_ST_*
        -- under RULE_CIRCUIT the word the witness entry points write for the same inputs --, d_norm (int64[batch] or None) the squared
        norm under `rule`, all ones where none exists.  Not synchronised."""
        check(self._lib.frw_falcon_verify_dev(self._ctx, int(logn), batch, _p(d_sig), _p(d_pk), _p(d_hm), int(rule), _p(d_status), _p(d_norm),
                                              C.c_void_p(stream)), "frw_falcon_verify_dev")

    def falcon_verify(self, logn, sig, pk, hm, rule=RULE_CIRCUIT, strict=True, want_norm=True):
        """Host buffers (frw_falcon_verify): sig, pk, hm uint16[batch, N] -> (status i32[batch], norm u64[batch] or None)."""
        n = 1 << logn
        sig, pk, hm = _u16(sig, n), _u16(pk, n), _u16(hm, n)
        batch = sig.shape[0]
        if pk.shape[0] != batch or hm.shape[0] != batch:
            raise ValueError("batch mismatch")
        st = np.zeros(batch, dtype=np.int32)
        norm = np.zeros(batch, dtype=np.uint64) if want_norm else None
        rc = self._lib.frw_falcon_verify(self._ctx, int(logn), batch, _p(sig), _p(pk), _p(hm), int(rule), _p(st), _p(norm), 1 if strict else 0)
        _check_refusal(rc, "frw_falcon_verify", st, "signature(s)")
        return st, norm

    @staticmethod
    def _falcon_verify_bytes(logn, pk_bytes, sig_bytes, msgs):
        batch = len(pk_bytes)
        if len(sig_bytes) != batch or len(msgs) != batch:
            raise ValueError("batch mismatch")
        sig_len = len(sig_bytes[0]) if batch else SIG_LEN[logn]
        if any(len(k) != PK_LEN[logn] for k in pk_bytes) or any(len(x) != sig_len for x in sig_bytes):
            raise ValueError("public keys must be %d bytes and signatures of one common length" % PK_LEN[logn])
        return (batch, sig_len, *_pack(pk_bytes, sig_bytes, msgs))

    def falcon_verify_workspace_bytes(self, logn, batch):
        return int(self._lib.frw_falcon_verify_workspace_bytes(int(logn), int(batch)))

    def falcon_verify_from_bytes(self, logn, pk_bytes, sig_bytes, msgs, rule=RULE_CIRCUIT, strict=True, want_norm=True):
        """Host buffers (frw_falcon_verify_from_bytes): lists of encoded public keys, encoded signatures of one common length and messages
        -> (status, norm or None); FRW_ST_DECODE for a malformed key or signature."""
        batch, sig_len, pkb, sgb, blob, off = self._falcon_verify_bytes(logn, pk_bytes, sig_bytes, msgs)
        st = np.zeros(batch, dtype=np.int32)
        norm = np.zeros(batch, dtype=np.uint64) if want_norm else None
        rc = self._lib.frw_falcon_verify_from_bytes(self._ctx, int(logn), batch, _p(pkb), _p(sgb), sig_len, _p(blob), _p(off), int(rule),
                                                    _p(st), _p(norm), 1 if strict else 0)
        _check_refusal(rc, "frw_falcon_verify_from_bytes", st, "signature(s)")
        return st, norm

    def falcon_verify_from_bytes_dev(self, logn, pk_bytes, sig_bytes, msgs, rule=RULE_CIRCUIT, stream=0, workspace=None, sig_len=None):
        """The same on the device (frw_falcon_verify_from_bytes_dev): the bytes are uploaded, both decoders, SHAKE256 and the kernel run
        on `stream`.  -> (status int32[batch], norm int64[batch]) device tensors, not synchronised.  pk_bytes may be a device uint8
        tensor [batch, PK_LEN] with sig_bytes a device uint8 tensor [batch, sig_len], msgs a (blob, offsets) pair of device tensors
        (uint8, int64[batch + 1]): nothing is uploaded then.  The uploaded inputs and a workspace made here are torch's and go back
        to its allocator when this method returns, with the four kernels possibly still queued: pass torch's current stream (or 0 while
        that is the default stream), or pass device tensors and a `workspace` of your own and keep them until `stream` has run."""
        batch, sig_len, d_pkb, d_sgb, d_blob, d_off = _encoded_dev(self.device, logn, pk_bytes, sig_bytes, msgs, sig_len,
                                                                   self._falcon_verify_bytes)
        d_status = _empty(batch, "int32", self.device)
        d_norm = _empty(batch, "int64", self.device)
        ws, ws_bytes = _workspace(workspace, self.device, 16, self.falcon_verify_workspace_bytes, logn, batch)
        check(self._lib.frw_falcon_verify_from_bytes_dev(self._ctx, int(logn), batch, _p(d_pkb), _p(d_sgb), int(sig_len), _p(d_blob),
                                                         _p(d_off), int(rule), _p(d_status), _p(d_norm), _p(ws), ws_bytes,
                                                         C.c_void_p(stream)), "frw_falcon_verify_from_bytes_dev")
        return d_status, d_norm

    # ---- the prover from bytes: encoded signatures in, proofs on the wire out ---------------------------------------------------------
    def pok_prove_workspace_bytes(self, pk, r1cs, circuit, logn, batch, in_flight):
        """Bytes of frw_pok_prove_from_bytes_dev's workspace for `batch` slots with `in_flight` proofs in flight (0: the handles are not
        that circuit's, or a bad argument)."""
        return int(self._lib.frw_pok_prove_workspace_bytes(pk, r1cs, int(circuit), int(logn), int(batch), int(in_flight)))

    def pok_prove_from_bytes(self, pk, r1cs, circuit, logn, pk_bytes, sig_bytes, msgs, rs, compressed=True, strict=True, want_proofs=True,
                             want_instance=True):
        """Host buffers (frw_pok_prove_from_bytes): lists of encoded public keys, encoded signatures of one common length and messages,
        rs uint64[batch, 2, 4] -> dict(wire uint8[batch, 192 | 384], proofs uint64[batch, 48] or None, instance uint64[batch, 2 N + 1, 4]
        or None, status int32[batch], num_unsatisfied uint32[batch]).  A refused slot (status != 0) is all zeros in every output."""
        batch, sig_len, pkb, sgb, blob, off = self._falcon_verify_bytes(logn, pk_bytes, sig_bytes, msgs)
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(batch, 2, 4)
        out = {"wire": np.zeros((batch, proof_wire_bytes(compressed)), dtype=np.uint8),
               "proofs": np.zeros((batch, 48), dtype=np.uint64) if want_proofs else None,
               "instance": np.zeros((batch, (2 << logn) + 1, 4), dtype=np.uint64) if want_instance else None,
               "status": np.zeros(batch, dtype=np.int32), "num_unsatisfied": np.zeros(batch, dtype=np.uint32)}
        rc = self._lib.frw_pok_prove_from_bytes(self._ctx, pk, r1cs, int(circuit), int(logn), batch, _p(pkb), _p(sgb), sig_len, _p(blob),
                                                _p(off), _p(rs), _wire_mode(compressed), _p(out["wire"]), _p(out["proofs"]),
                                                _p(out["instance"]), _p(out["status"]), _p(out["num_unsatisfied"]), 1 if strict else 0)
        _check_refusal(rc, "frw_pok_prove_from_bytes", out["status"], "signature(s)")
        return out

    def pok_prove_from_bytes_dev(self, pk, r1cs, circuit, logn, pk_bytes, sig_bytes, msgs, rs, compressed=True, in_flight=None, workspace=None,
                                 want_proofs=True, want_instance=True, want_unsatisfied=True, stream=0, sig_len=None):
        """The same on the device (frw_pok_prove_from_bytes_dev) -> dict of device tensors: wire uint8[batch, 192 | 384], proofs
        int64[batch, 48], instance int64[batch, 2 N + 1, 4], status int32[batch], num_unsatisfied int32[batch] (None where not asked
        for).  The inputs as for falcon_verify_from_bytes_dev (lists of bytes, or device tensors with msgs a (blob, offsets) pair); rs:
        uint64[batch, 2, 4] on the host or an int64 device tensor.  workspace: a uint8 device tensor (256-byte aligned, as torch's
        are), or None for one that holds `in_flight` proofs (default: min(batch, 4)).  The call waits on `stream` once, for the number
        of accepted signatures; its results are ordered on `stream` and not synchronised."""
        import torch
        dev = self.device
        batch, sig_len, d_pkb, d_sgb, d_blob, d_off = _encoded_dev(dev, logn, pk_bytes, sig_bytes, msgs, sig_len, self._falcon_verify_bytes)
        if isinstance(rs, torch.Tensor):
            d_rs = rs
        elif batch:
            d_rs, = _upload((np.ascontiguousarray(rs, dtype=np.uint64).reshape(batch, 2, 4),), dev)
        else:
            d_rs = torch.zeros(8, dtype=torch.int64, device=torch.device("cuda", dev))
        rows = max(batch, 1)                    # (an empty tensor has no address: the call refuses null pointers whatever the batch)
        out = {"wire": _empty((rows, proof_wire_bytes(compressed)), "uint8", dev),
               "proofs": _empty((rows, 48), "int64", dev) if want_proofs else None,
               "instance": _empty((rows, (2 << logn) + 1, 4), "int64", dev) if want_instance else None,
               "status": _empty(rows, "int32", dev),
               "num_unsatisfied": _empty(rows, "int32", dev) if want_unsatisfied else None}
        k = max(1, min(batch, 4) if in_flight is None else int(in_flight))
        ws, ws_bytes = _workspace(workspace, dev, 256, self.pok_prove_workspace_bytes, pk, r1cs, circuit, logn, batch, k)
        check(self._lib.frw_pok_prove_from_bytes_dev(self._ctx, pk, r1cs, int(circuit), int(logn), batch, _p(d_pkb), _p(d_sgb), int(sig_len),
                                                     _p(d_blob), _p(d_off), _p(d_rs), _wire_mode(compressed), _p(out["wire"]),
                                                     _p(out["proofs"]), _p(out["instance"]), _p(out["status"]), _p(out["num_unsatisfied"]),
                                                     _p(ws), ws_bytes, C.c_void_p(stream)), "frw_pok_prove_from_bytes_dev")
        return {k: (v[:batch] if v is not None else None) for k, v in out.items()}

    # ---- an aggregate from bytes: triples of mixed parameter sets in statement order -> verdicts, the statement, ONE proof ------------
    @staticmethod
    def _aggregate_bytes(triples, nonces=None):
        """[(pk_bytes, msg, sig_bytes)] in statement order (with `nonces`: [(pk_bytes, msg)] and the 40-byte nonces) -> the keys end to
        end, the signatures (or nonces) end to end, the message blob and its offsets.  The lengths say which parameter set a statement
        is of; the handle says which it must be, and the library reads the bytes by the handle."""
        keys = [bytes(t[0]) for t in triples]
        msgs = [bytes(t[1]) for t in triples]
        second = [bytes(x) for x in nonces] if nonces is not None else [bytes(t[2]) for t in triples]
        if len(second) != len(keys):
            raise ValueError("one nonce per statement")
        for i, k in enumerate(keys):
            logn = {PK_LEN[9]: 9, PK_LEN[10]: 10}.get(len(k))
            if logn is None or len(second[i]) != (NONCE_LEN if nonces is not None else SIG_LEN[logn]):
                raise ValueError("statement %d: a key of %d or %d bytes and a signature of %d or %d (a nonce of %d)"
                                 % (i, PK_LEN[9], PK_LEN[10], SIG_LEN[9], SIG_LEN[10], NONCE_LEN))
        return (len(keys), *_pack(keys, second, msgs))

    def _aggregate_count(self, handle, count, where):
        info = self.r1cs_info(handle)
        if int(info.num_statements) != count:
            raise FrwError(-1, where, "%d statements given, the aggregate has %d" % (count, int(info.num_statements)))
        return info

    def aggregate_screen_workspace_bytes(self, handle):
        return int(self._lib.frw_aggregate_screen_workspace_bytes(handle))

    def aggregate_falcon_verify_from_bytes(self, handle, triples, rule=RULE_CIRCUIT, want_norm=True):
        """Host buffers (frw_aggregate_falcon_verify_from_bytes): [(pk_bytes, msg, sig_bytes)] in statement order -> (status i32[count],
        norm u64[count] or None), statement by statement what falcon_verify_from_bytes gives."""
        count, pkb, sgb, blob, off = self._aggregate_bytes(triples)
        self._aggregate_count(handle, count, "frw_aggregate_falcon_verify_from_bytes")
        st = np.zeros(count, dtype=np.int32)
        norm = np.zeros(count, dtype=np.uint64) if want_norm else None
        check(self._lib.frw_aggregate_falcon_verify_from_bytes(handle, self._ctx, _p(pkb), _p(sgb), _p(blob), _p(off), int(rule), _p(st),
                                                               _p(norm)), "frw_aggregate_falcon_verify_from_bytes")
        return st, norm

    def aggregate_falcon_verify_from_bytes_dev(self, handle, triples, rule=RULE_CIRCUIT, stream=0, workspace=None):
        """The same on the device (frw_aggregate_falcon_verify_from_bytes_dev) -> (status int32[count], norm int64[count]) device
        tensors, not synchronised.  Capture-safe once the inputs are on the device."""
        count, pkb, sgb, blob, off = self._aggregate_bytes(triples)
        self._aggregate_count(handle, count, "frw_aggregate_falcon_verify_from_bytes_dev")
        d_pkb, d_sgb, d_blob, d_off = _upload((pkb, sgb, blob, off), self.device)
        d_status = _empty(count, "int32", self.device)
        d_norm = _empty(count, "int64", self.device)
        ws, ws_bytes = _workspace(workspace, self.device, 16, self.aggregate_screen_workspace_bytes, handle)
        check(self._lib.frw_aggregate_falcon_verify_from_bytes_dev(handle, self._ctx, _p(d_pkb), _p(d_sgb), _p(d_blob), _p(d_off), int(rule),
                                                                   _p(d_status), _p(d_norm), _p(ws), ws_bytes, C.c_void_p(stream)),
              "frw_aggregate_falcon_verify_from_bytes_dev")
        return d_status, d_norm

    def aggregate_statement_from_bytes(self, handle, pk_bytes, nonces, msgs, encoding=ENC_MONTGOMERY):
        """Host buffers (frw_aggregate_statement_from_bytes): the verifier's side -- keys, 40-byte nonces and messages in statement
        order -> (instance u64[I, 4], status i32[count])."""
        count, pkb, non, blob, off = self._aggregate_bytes(list(zip(pk_bytes, msgs)), nonces)
        info = self._aggregate_count(handle, count, "frw_aggregate_statement_from_bytes")
        inst = np.zeros((int(info.num_instance), 4), dtype=np.uint64)
        st = np.zeros(count, dtype=np.int32)
        check(self._lib.frw_aggregate_statement_from_bytes(handle, self._ctx, _p(pkb), _p(non), _p(blob), _p(off), int(encoding), _p(inst),
                                                           _p(st)), "frw_aggregate_statement_from_bytes")
        return inst, st

    def aggregate_statement_from_bytes_dev(self, handle, pk_bytes, nonces, msgs, encoding=ENC_MONTGOMERY, stream=0, workspace=None):
        """The same on the device (frw_aggregate_statement_from_bytes_dev) -> (instance int64[I, 4], status int32[count]) device
        tensors, not synchronised."""
        count, pkb, non, blob, off = self._aggregate_bytes(list(zip(pk_bytes, msgs)), nonces)
        info = self._aggregate_count(handle, count, "frw_aggregate_statement_from_bytes_dev")
        d_pkb, d_non, d_blob, d_off = _upload((pkb, non, blob, off), self.device)
        d_inst = _empty((int(info.num_instance), 4), "int64", self.device)
        d_status = _empty(count, "int32", self.device)
        ws, ws_bytes = _workspace(workspace, self.device, 16, self.aggregate_screen_workspace_bytes, handle)
        check(self._lib.frw_aggregate_statement_from_bytes_dev(handle, self._ctx, _p(d_pkb), _p(d_non), _p(d_blob), _p(d_off), int(encoding),
                                                               _p(d_inst), _p(d_status), _p(ws), ws_bytes, C.c_void_p(stream)),
              "frw_aggregate_statement_from_bytes_dev")
        return d_inst, d_status

    def aggregate_prove_workspace_bytes(self, pk, handle):
        """Bytes of frw_aggregate_prove_from_bytes_dev's workspace (0: not an aggregate, or a key that is not this handle's)."""
        return int(self._lib.frw_aggregate_prove_workspace_bytes(pk, handle))

    def aggregate_prove_from_bytes(self, pk, handle, triples, rs, compressed=True, strict=True):
        """Host buffers (frw_aggregate_prove_from_bytes): [(pk_bytes, msg, sig_bytes)] in statement order, rs uint64[2, 4] -> dict(rc,
        wire uint8[192 | 384], proof uint64[48], instance uint64[I, 4], nonces uint8[count, 40], status int32[count],
        num_unsatisfied).  A refused statement means NO proof: rc = E_RANGE, wire and proof all zero, num_unsatisfied all ones, status
        says which statement; with strict that is raised as FrwError."""
        count, pkb, sgb, blob, off = self._aggregate_bytes(triples)
        info = self._aggregate_count(handle, count, "frw_aggregate_prove_from_bytes")
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(2, 4)
        out = {"wire": np.zeros(proof_wire_bytes(compressed), dtype=np.uint8), "proof": np.zeros(48, dtype=np.uint64),
               "instance": np.zeros((int(info.num_instance), 4), dtype=np.uint64), "nonces": np.zeros((count, NONCE_LEN), dtype=np.uint8),
               "status": np.zeros(count, dtype=np.int32), "num_unsatisfied": np.zeros(1, dtype=np.uint32)}
        rc = self._lib.frw_aggregate_prove_from_bytes(self._ctx, pk, handle, _p(pkb), _p(sgb), _p(blob), _p(off), _p(rs),
                                                      _wire_mode(compressed), _p(out["wire"]), _p(out["proof"]), _p(out["instance"]),
                                                      _p(out["nonces"]), _p(out["status"]), _p(out["num_unsatisfied"]))
        return self._aggregate_verdict(rc, out, out["status"], strict, "frw_aggregate_prove_from_bytes")

    @staticmethod
    def _aggregate_verdict(rc, out, status, strict, where):
        if rc == E_RANGE and strict:
            raise FrwError(rc, where, _refusal(status, "statement(s)", head="no proof"))
        if rc != E_RANGE:
            check(rc, where)
        out["rc"] = rc
        return out

    def aggregate_prove_from_bytes_dev(self, pk, handle, triples, rs, compressed=True, strict=True, workspace=None, stream=0):
        """The same on the device (frw_aggregate_prove_from_bytes_dev) -> dict of device tensors (wire uint8, proof int64[48], instance
        int64[I, 4], nonces uint8[count, 40], status int32[count], num_unsatisfied int32[1]) and rc.  rs: uint64[2, 4] on the host or an
        int64 device tensor.  The call waits on `stream` once, for the number of refused statements."""
        import torch
        dev = self.device
        count, pkb, sgb, blob, off = self._aggregate_bytes(triples)
        info = self._aggregate_count(handle, count, "frw_aggregate_prove_from_bytes_dev")
        d_pkb, d_sgb, d_blob, d_off = _upload((pkb, sgb, blob, off), dev)
        d_rs = rs if isinstance(rs, torch.Tensor) else _upload((np.ascontiguousarray(rs, dtype=np.uint64).reshape(8),), dev)[0]
        out = {"wire": _empty(proof_wire_bytes(compressed), "uint8", dev),
               "proof": _empty(48, "int64", dev),
               "instance": _empty((int(info.num_instance), 4), "int64", dev),
               "nonces": _empty((count, NONCE_LEN), "uint8", dev),
               "status": _empty(count, "int32", dev),
               "num_unsatisfied": _empty(1, "int32", dev)}
        ws, ws_bytes = _workspace(workspace, dev, 256, self.aggregate_prove_workspace_bytes, pk, handle)
        rc = self._lib.frw_aggregate_prove_from_bytes_dev(self._ctx, pk, handle, _p(d_pkb), _p(d_sgb), _p(d_blob), _p(d_off), _p(d_rs),
                                                          _wire_mode(compressed), _p(out["wire"]), _p(out["proof"]), _p(out["instance"]),
                                                          _p(out["nonces"]), _p(out["status"]), _p(out["num_unsatisfied"]), _p(ws),
                                                          ws_bytes, C.c_void_p(stream))
        return self._aggregate_verdict(rc, out, out["status"], strict, "frw_aggregate_prove_from_bytes_dev")

    def groth16_setup_r1cs(self, handle, alpha, beta, gamma, delta, t, mode=KEY_AUTO, rank=0, world=1, want_vk=True):
        """groth16_setup for the system behind an r1cs handle (a per-signature circuit or an aggregate statement).
        mode: KEY_TABLES (window tables), KEY_BARE (the points only, made on the device end to end), KEY_AUTO by size;
        rank / world: one slice of a key in slices (bare)."""
        from ._lib import Groth16KeyOpts
        tox = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in (alpha, beta, gamma, delta, t)), dtype=np.uint64).copy()
        ni = int(self.r1cs_info(handle).num_instance)
        vk = np.zeros(84 + 12 * ni, dtype=np.uint64)
        h = C.c_void_p()
        opts = Groth16KeyOpts(int(mode), int(rank), int(world))
        check(self._lib.frw_groth16_setup_r1cs_opts(handle, _p(tox), C.byref(opts), C.byref(h), _p(vk) if want_vk else None),
              "frw_groth16_setup_r1cs")
        return h, (_vk_dict(vk) if want_vk else None)

    def r1cs_check_dev(self, handle, batch, d_wit, d_inst, d_num_unsatisfied, stream=0):
        check(self._lib.frw_r1cs_check_dev(handle, batch, _p(d_wit), _p(d_inst), _p(d_num_unsatisfied), C.c_void_p(stream)),
              "frw_r1cs_check_dev")

    def r1cs_eval_dev(self, handle, batch, d_wit, d_inst, d_num_unsatisfied, d_abc, stream=0):
        """r1cs_check_dev + A z, B z, C z into d_abc (int64[batch, 3, C, 4], Montgomery)."""
        check(self._lib.frw_r1cs_eval_dev(handle, batch, _p(d_wit), _p(d_inst), _p(d_num_unsatisfied), _p(d_abc), C.c_void_p(stream)),
              "frw_r1cs_eval_dev")

    def r1cs_eval_scratch_bytes(self, handle, batch, with_products):
        return int(self._lib.frw_r1cs_eval_scratch_bytes(handle, batch, 1 if with_products else 0))

    def r1cs_eval_scratch_dev(self, handle, batch, d_wit, d_inst, d_num_unsatisfied, d_abc, d_scratch, scratch_bytes, stream=0):
        """frw_r1cs_eval_dev / frw_r1cs_check_dev (d_abc=None) with the caller's scratch: allocates nothing, capture-safe."""
        check(self._lib.frw_r1cs_eval_scratch_dev(handle, batch, _p(d_wit), _p(d_inst), _p(d_num_unsatisfied), _p(d_abc), _p(d_scratch),
                                                  scratch_bytes, C.c_void_p(stream)), "frw_r1cs_eval_scratch_dev")

    # ---- multi-scalar multiplication over BLS12-381 G1 (frw_msm.hip) --------------------------------------------------
    def msm_g1_load(self, bases, narrow=False, bare=False, wide=False):
        """bases: uint64[n, 12] (ark-ff's bytes of n affine points, zeros = infinity) -> handle; free with msm_free.
        narrow: 8-bit windows (128 buckets) instead of 16-bit ones: for scalars that are mostly zero, one or small.
        bare: the points only, no window table (the sums run window by window); wide: a dense bare handle on thirteen 20-bit windows
        whatever its size (what handles of 2^23 points and more run on anyway)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
        h = C.c_void_p()
        if bare:
            check(self._lib.frw_msm_g1_load_bare(self.device, bases.shape[0], _p(bases), 2 if wide else 1 if narrow else 0, C.byref(h)),
                  "frw_msm_g1_load_bare")
            return h
        fn = self._lib.frw_msm_g1_load_narrow if narrow else self._lib.frw_msm_g1_load
        check(fn(self.device, bases.shape[0], _p(bases), C.byref(h)), "frw_msm_g1_load")
        return h

    def g1_fixed_base(self, scalars):
        """k_i G1 on the device: canonical scalars uint64[count, 4] -> uint64[count, 12] (ark-ff's bytes)."""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((scalars.shape[0], 12), dtype=np.uint64)
        check(self._lib.frw_g1_fixed_base(self.device, scalars.shape[0], _p(scalars), _p(out)), "frw_g1_fixed_base")
        return out

    def g2_fixed_base(self, scalars):
        """k_i G2 on the device: canonical scalars uint64[count, 4] -> uint64[count, 24] (ark-ff's bytes)."""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((scalars.shape[0], 24), dtype=np.uint64)
        check(self._lib.frw_g2_fixed_base(self.device, scalars.shape[0], _p(scalars), _p(out)), "frw_g2_fixed_base")
        return out

    def msm_g2_load(self, bases, narrow=False, bare=False, wide=False):
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 24)
        h = C.c_void_p()
        if bare:
            check(self._lib.frw_msm_g2_load_bare(self.device, bases.shape[0], _p(bases), 2 if wide else 1 if narrow else 0, C.byref(h)),
                  "frw_msm_g2_load_bare")
            return h
        fn = self._lib.frw_msm_g2_load_narrow if narrow else self._lib.frw_msm_g2_load
        check(fn(self.device, bases.shape[0], _p(bases), C.byref(h)), "frw_msm_g2_load")
        return h

    def msm_g2_dev(self, handle, batch, d_scalars, scalar_stride, montgomery, d_out, d_workspace, workspace_bytes, stream=0):
        check(self._lib.frw_msm_g2_dev(handle, batch, _p(d_scalars), scalar_stride, 1 if montgomery else 0, _p(d_out), _p(d_workspace),
                                       workspace_bytes, C.c_void_p(stream)), "frw_msm_g2_dev")

    def msm_free(self, handle):
        self._lib.frw_msm_free(handle)

    def msm_info(self, handle):
        from ._lib import MsmInfoStruct
        info = MsmInfoStruct()
        check(self._lib.frw_msm_info(handle, C.byref(info)), "frw_msm_info")
        return info

    def msm_g1_dev(self, handle, batch, d_scalars, scalar_stride, montgomery, d_out, d_workspace, workspace_bytes, stream=0):
        check(self._lib.frw_msm_g1_dev(handle, batch, _p(d_scalars), scalar_stride, 1 if montgomery else 0, _p(d_out), _p(d_workspace),
                                       workspace_bytes, C.c_void_p(stream)), "frw_msm_g1_dev")

    def groth16_msm_h_dev(self, handle, batch, d_h, domain_size, d_out, d_workspace, workspace_bytes, stream=0):
        check(self._lib.frw_groth16_msm_h_dev(handle, batch, _p(d_h), domain_size, _p(d_out), _p(d_workspace), workspace_bytes,
                                              C.c_void_p(stream)), "frw_groth16_msm_h_dev")

    # ---- a whole Groth16 proof per signature ---------------------------------------------------------------------------
    def groth16_pk_load(self, num_instance, num_witness, domain_size, alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query,
                        b_g1_query, b_g2_query, h_query, l_query, mode=KEY_TABLES, rank=0, world=1):
        """The proving key's elements as uint64 arrays in ark-ff's bytes (G1 rows of 12, G2 rows of 24) -> handle.
        mode / rank / world: as groth16_setup_r1cs (every rank passes the WHOLE key and keeps its slice)."""
        from ._lib import Groth16PkDesc, Groth16KeyOpts
        arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in (alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query, b_g1_query,
                                                                   b_g2_query, h_query, l_query)]
        nv = num_instance + num_witness
        want = [12, 12, 12, 24, 24, nv * 12, nv * 12, nv * 24, (domain_size - 1) * 12, num_witness * 12]
        if [a.size for a in arrs] != want:
            raise ValueError("proving key: wrong array sizes")
        d = Groth16PkDesc(num_instance, num_witness, domain_size, *[_p(a) for a in arrs])
        h = C.c_void_p()
        opts = Groth16KeyOpts(int(mode), int(rank), int(world))
        check(self._lib.frw_groth16_pk_load_opts(self.device, C.byref(d), C.byref(opts), C.byref(h)), "frw_groth16_pk_load")
        return h

    groth16_pk_wire_bytes = staticmethod(groth16_pk_wire_bytes)
    groth16_pk_wire_info = staticmethod(groth16_pk_wire_info)

    def groth16_pk_load_wire(self, data, compressed=True, checked=True, mode=KEY_AUTO):
        """A ProvingKey as ark-groth16 serialises it (pk.serialize / serialize_uncompressed) -> (handle, verifying key dict as groth16_setup
        returns it).  Every point is decoded on the device and, if `checked`, tested for subgroup membership there; checked=False
        (FRW_PK_POINTS_ARE_CHECKED) skips those ladders only and is unsafe for a key this process did not make.  FrwError
        (FRW_E_INVALID_ARG) for a malformed or off-subgroup point or bad framing: the message names the query and the first bad index."""
        from ._lib import Groth16KeyOpts
        data = bytes(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        info = groth16_pk_wire_info(data, compressed)
        vk = np.zeros(84 + 12 * info["num_instance"], dtype=np.uint64)
        h = C.c_void_p()
        opts = Groth16KeyOpts(int(mode), 0, 1)
        check(self._lib.frw_groth16_pk_load_wire_dev(self.device, _p(buf), buf.size, _wire_mode(compressed),
                                                     0 if checked else PK_POINTS_ARE_CHECKED, C.byref(opts), C.byref(h), _p(vk)),
              "frw_groth16_pk_load_wire_dev")
        return h, _vk_dict(vk)

    def groth16_pk_to_wire(self, pk, vk, compressed=True):
        """The whole proving key behind a handle (table or bare, made by groth16_setup* or loaded) as the bytes ProvingKey::deserialize
        reads.  vk: the verifying key that came with the handle (dict or flat limbs): gamma_g2 and gamma_abc_g1 are taken from it."""
        vk, ni = _vk_flat(vk, "groth16_pk_to_wire")
        info = self.groth16_pk_info(pk)
        nv = int(info.z_hi) - int(info.z_lo) - 3
        out = np.zeros(max(groth16_pk_wire_bytes(ni, nv - ni, int(info.h_hi) - int(info.h_lo) + 1, compressed), 1), dtype=np.uint8)
        check(self._lib.frw_groth16_pk_to_wire_dev(pk, _p(vk), ni, _wire_mode(compressed), _p(out), out.size), "frw_groth16_pk_to_wire_dev")
        return out.tobytes()

    def groth16_pk_info(self, pk):
        from ._lib import Groth16PkInfoStruct
        info = Groth16PkInfoStruct()
        check(self._lib.frw_groth16_pk_info(pk, C.byref(info)), "frw_groth16_pk_info")
        return info

    def groth16_pk_query(self, pk, which):
        """One of the key's five tables (0: h_query, 1: a, 2: b_g1, 3: l, 4: b_g2) as a BORROWED msm handle (never msm_free it)."""
        h = self._lib.frw_groth16_pk_query(pk, int(which))
        if not h:
            raise FrwError(-1, "frw_groth16_pk_query", "no such query")
        return C.c_void_p(h)

    def groth16_prove_partial_dev(self, pk, r1cs, batch, d_wit, d_inst, rs, d_partial, d_workspace, workspace_bytes, d_num_unsatisfied=None, stream=0):
        """One rank's partial sums of a key in slices: d_partial int64[batch, 72] = A | B1' | L | H | B (ark-ff's affine bytes)."""
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(batch, 2, 4)
        check(self._lib.frw_groth16_prove_partial_dev(pk, r1cs, batch, _p(d_wit), _p(d_inst), _p(rs), _p(d_partial), _p(d_num_unsatisfied),
                                                      _p(d_workspace), workspace_bytes, C.c_void_p(stream)), "frw_groth16_prove_partial_dev")

    def groth16_prove_combine_dev(self, pk, world, d_partials, rs, d_proof, d_workspace, workspace_bytes, stream=0):
        """All ranks' partial sums (int64[world, 72], rank order) -> the proof int64[48]."""
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(2, 4)
        check(self._lib.frw_groth16_prove_combine_dev(pk, world, _p(d_partials), _p(rs), _p(d_proof), _p(d_workspace), workspace_bytes,
                                                      C.c_void_p(stream)), "frw_groth16_prove_combine_dev")

    def diag_groth16_side_counts(self, pk, d_z, d_workspace, workspace_bytes, stream=0):
        """(rows of b_g1_query / b_g2_query that hold a point, digits and ones over all rows, digits and ones over those rows): the point
        additions of the witness-side sums of a key of bare handles for the scalars d_z (z ++ [1, r, s] of the key's slice)."""
        out = np.zeros(5, dtype=np.uint64)
        check(self._lib.frw_diag_groth16_side_counts(pk, _p(d_z), _p(d_workspace), workspace_bytes, C.c_void_p(stream), _p(out)),
              "frw_diag_groth16_side_counts")
        return [int(v) for v in out]

    def diag_poly_eval_dev(self, d_coeffs, n, t):
        """p(t) for the polynomial whose n coefficients (ark-ff's Montgomery form) are in device memory; t, result: Python integers."""
        tt = np.frombuffer(int(t).to_bytes(32, "little"), dtype=np.uint64).copy()
        out = np.zeros(4, dtype=np.uint64)
        check(self._lib.frw_diag_poly_eval_dev(self.device, n, _p(d_coeffs), _p(tt), _p(out)), "frw_diag_poly_eval_dev")
        return int.from_bytes(out.tobytes(), "little")

    def groth16_setup(self, circuit, logn, alpha, beta, gamma, delta, t):
        """generate_parameters with the given toxic waste (Python integers) -> (proving-key handle, verifying key dict of uint64 arrays)."""
        tox = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in (alpha, beta, gamma, delta, t)), dtype=np.uint64).copy()
        L = circuit_layout(circuit, logn)
        vk = np.zeros(84 + 12 * L.num_instance, dtype=np.uint64)
        h = C.c_void_p()
        check(self._lib.frw_groth16_setup(self.device, circuit, logn, _p(tox), C.byref(h), _p(vk)), "frw_groth16_setup")
        return h, _vk_dict(vk)

    def groth16_pk_free(self, handle):
        self._lib.frw_groth16_pk_free(handle)

    def groth16_workspace_bytes(self, pk, r1cs, in_flight):
        return int(self._lib.frw_groth16_workspace_bytes(pk, r1cs, in_flight))

    def groth16_prove_dev(self, pk, r1cs, batch, d_wit, d_inst, rs, d_proofs, d_workspace, workspace_bytes, d_num_unsatisfied=None, stream=0):
        """rs: host uint64[batch, 2, 4] (r, s per proof, canonical); d_proofs: int64[batch, 48] = A | B | C in ark-ff's bytes."""
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(batch, 2, 4)
        check(self._lib.frw_groth16_prove_dev(pk, r1cs, batch, _p(d_wit), _p(d_inst), _p(rs), _p(d_proofs), _p(d_num_unsatisfied),
                                              _p(d_workspace), workspace_bytes, C.c_void_p(stream)), "frw_groth16_prove_dev")

    def groth16_prove_rs_dev(self, pk, r1cs, batch, d_wit, d_inst, d_rs, d_proofs, d_workspace, workspace_bytes, d_num_unsatisfied=None, stream=0):
        """The same with the blinding factors in device memory (d_rs: int64[batch, 2, 4]): stream-ordered throughout, capturable."""
        check(self._lib.frw_groth16_prove_rs_dev(pk, r1cs, batch, _p(d_wit), _p(d_inst), _p(d_rs), _p(d_proofs), _p(d_num_unsatisfied),
                                                 _p(d_workspace), workspace_bytes, C.c_void_p(stream)), "frw_groth16_prove_rs_dev")

    def groth16_prove_seeded_dev(self, pk, r1cs, batch, d_wit, d_inst, d_seed, d_counter, d_rs, d_proofs, d_workspace, workspace_bytes,
                                 d_num_unsatisfied=None, stream=0):
        """groth16_prove_rs_dev with the blinding factors drawn on the device (frw_groth16_prove_seeded_dev): one draw of 2 x batch
        scalars for (d_seed uint8[32], d_counter int64[1], DRAW_BLINDING) into d_rs (int64[batch, 2, 4], the caller's: it holds what
        was used), the proofs, and the counter advanced by one.  Capturable as groth16_prove_rs_dev is: every replay is a fresh proof."""
        check(self._lib.frw_groth16_prove_seeded_dev(pk, r1cs, batch, _p(d_wit), _p(d_inst), _p(d_seed), _p(d_counter), _p(d_rs), _p(d_proofs),
                                                     _p(d_num_unsatisfied), _p(d_workspace), workspace_bytes, C.c_void_p(stream)),
              "frw_groth16_prove_seeded_dev")

    def qap_info(self, handle):
        """Domain of the QAP witness map for the loaded matrices: (log n, n, C, I, workspace bytes per signature)."""
        from ._lib import QapInfoStruct
        q = QapInfoStruct()
        check(self._lib.frw_qap_info(handle, C.byref(q)), "frw_qap_info")
        return q

    def qap_witness_map_dev(self, handle, batch, d_wit, d_inst, d_h, d_workspace, workspace_bytes, d_num_unsatisfied=None,
                            stream=0):
        """ark-groth16's R1CStoQAP::witness_map for every signature of a resident batch: d_h = int64[batch, n, 4]
        (Montgomery), coefficient k of h(X) = (A B - C)(X) / (X^n - 1) at index k."""
        check(self._lib.frw_qap_witness_map_dev(handle, batch, _p(d_wit), _p(d_inst), _p(d_h), _p(d_num_unsatisfied), _p(d_workspace),
                                                workspace_bytes, C.c_void_p(stream)), "frw_qap_witness_map_dev")

    def qap_quotient_dev(self, handle, batch, d_wit, d_inst, d_h, d_workspace, workspace_bytes, d_num_unsatisfied=None, stream=0):
        """h with six transforms instead of seven: equal to qap_witness_map_dev's wherever d_num_unsatisfied is 0."""
        check(self._lib.frw_qap_quotient_dev(handle, batch, _p(d_wit), _p(d_inst), _p(d_h), _p(d_num_unsatisfied), _p(d_workspace),
                                             workspace_bytes, C.c_void_p(stream)), "frw_qap_quotient_dev")

    def qap_witness_map(self, handle, witness, instance):
        """Host arrays (uint64[batch, W, 4], uint64[batch, I, 4], Montgomery, as witness_ntt_verify returns them) ->
        (h uint64[batch, n, 4], unsatisfied rows uint32[batch])."""
        witness = np.ascontiguousarray(witness, dtype=np.uint64)
        instance = np.ascontiguousarray(instance, dtype=np.uint64)
        batch = witness.shape[0]
        n = int(self.qap_info(handle).domain_size)
        h = np.empty((batch, n, 4), dtype=np.uint64)
        bad = np.empty(batch, dtype=np.uint32)
        check(self._lib.frw_qap_witness_map(handle, batch, _p(witness), _p(instance), _p(h), _p(bad)), "frw_qap_witness_map")
        return h, bad

    def digest_dev(self, d_buf, words_per_item, items, d_out, stream=0):
        check(self._lib.frw_digest_dev(self._ctx, _p(d_buf), words_per_item, items, _p(d_out), C.c_void_p(stream)), "frw_digest_dev")
