"""Falcon verification on the device without a witness (falcon_verify_kernel in frw_kernels.hip; frw_falcon_verify_dev,
frw_falcon_verify_from_bytes_dev and their host-buffer forms): the status words held to the compact witness call's on the same inputs,
the norms to a numpy negacyclic product, the two rules to the bound and to the coefficient 6144 exactly, the bytes path to the genuine
signatures and to oracle/falcon_sign.py's Verify on tampered ones, and the verdicts of an aggregate's statements to r1cs_check_dev."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import falcon_verify_cases as FV
from oracle import falcon_codec as FC
from oracle import falcon_sign as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = FV.Q
SENTINEL = 0x5A5AA5A53C3CC3C3                        # (fits int64)
OK, COEFF_RANGE, NORM_BOUND, DECODE = 0, 1, 2, 3
RULES = (FV.RULE_CIRCUIT, FV.RULE_SPEC)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(torch.device("cuda:0"))


def _verify(engine, logn, sig, pk, hm, rule, want_norm=True):
    """frw_falcon_verify_dev with a sentinel word in front of and behind each output -> (status, norm) as numpy, the sentinels checked"""
    import torch
    dev = torch.device("cuda:0")
    batch = sig.shape[0]
    st = torch.full((batch + 2,), -7, dtype=torch.int32, device=dev)
    nrm = torch.full((batch + 2,), SENTINEL, dtype=torch.int64, device=dev)
    engine.falcon_verify_dev(logn, batch, _dev(sig), _dev(pk), _dev(hm), st[1:], nrm[1:] if want_norm else None, rule,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st, nrm = st.cpu().numpy(), nrm.cpu().numpy()
    assert st[0] == -7 and st[-1] == -7 and nrm[0] == SENTINEL and nrm[-1] == SENTINEL
    if not want_norm:
        assert (nrm == SENTINEL).all()
    return st[1:-1], nrm[1:-1]


def _compact_status(engine, logn, sig, pk, hm):
    """the status words of frw_witness_ntt_verify_compact_dev: the cheapest route to them before this entry point"""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    batch = sig.shape[0]
    compact = torch.empty(batch * frw.compact_layout(logn).bytes_per_signature, dtype=torch.uint8, device=dev)
    st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
    engine.witness_ntt_verify_compact_dev(logn, batch, _dev(sig), _dev(pk), _dev(hm), compact, st, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st.cpu().numpy()


_MIXED = {}


def _mixed(engine, logn):
    """130 triples: every third one's hm uniform (its v is uniform: NORM_BOUND), a coefficient >= q planted in sig of 1, in pk of 4 and
    in hm of 7 (and in sig of 9, whose hm is uniform too: COEFF_RANGE comes first) -> (sig, pk, hm, the compact witness call's statuses,
    the CPU norms per rule).  Made once per logn and shared; nobody writes to it."""
    if logn not in _MIXED:
        import falcon_r1cs_amd as frw
        n = 1 << logn
        sig, pk, hm = (a.copy() for a in frw.synth_triples(logn, 130, seed=1200 + logn))
        rng = np.random.default_rng(logn)
        hm[0::3] = rng.integers(0, Q, (len(hm[0::3]), n), dtype=np.uint16)
        sig[1, 17] = Q
        pk[4, n - 1] = Q + 1
        hm[7, 0] = 0xFFFF
        sig[9, n - 1] = 0x8000
        for a in (sig, pk, hm):
            a.setflags(write=False)
        want = _compact_status(engine, logn, sig, pk, hm)
        ok = np.ones(130, dtype=bool)
        ok[[1, 4, 7, 9]] = False
        cpu = {rule: FV.norms(np.where(ok[:, None], sig, 0), np.where(ok[:, None], pk, 0), np.where(ok[:, None], hm, 0), rule) for rule in RULES}
        _MIXED[logn] = (sig, pk, hm, want, ok, cpu)
    return _MIXED[logn]


# ---- 1. equality with the witness kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [9, 10])
def test_status_equals_the_compact_witness_call_word_for_word(engine, logn):
    sig, pk, hm, want, ok, _ = _mixed(engine, logn)
    assert want[:3].tolist() == [NORM_BOUND, COEFF_RANGE, OK]                   # the smallest batch that can hold all three does
    assert want[[1, 4, 7, 9]].tolist() == [COEFF_RANGE] * 4
    for batch in (1, 3, 37, 130):
        got, _ = _verify(engine, logn, sig[:batch], pk[:batch], hm[:batch], FV.RULE_CIRCUIT)
        assert np.array_equal(got, want[:batch]), batch
        if batch >= 3:                                                          # (one signature has one status)
            assert {OK, COEFF_RANGE, NORM_BOUND} <= set(got.tolist()), batch
    # the witness call on its own prefix gives the same words as on the whole batch
    assert np.array_equal(_compact_status(engine, logn, sig[:37], pk[:37], hm[:37]), want[:37])


# ---- 2. norms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("logn", [9, 10])
def test_norms_equal_the_numpy_negacyclic_product(engine, logn, rule):
    sig, pk, hm, want, ok, cpu = _mixed(engine, logn)
    st, nrm = _verify(engine, logn, sig, pk, hm, rule)
    assert np.array_equal(nrm[ok], cpu[rule][ok])
    assert (nrm[~ok] == -1).all() and (~ok).sum() == 4                          # all ones where no norm exists
    assert np.array_equal(st[ok], FV.verdicts(cpu[rule][ok], logn, rule)) and (st[~ok] == COEFF_RANGE).all()
    assert (st[ok] == OK).any() and (st[ok] == NORM_BOUND).any()
    # without d_norm: the same statuses, nothing written anywhere else
    st2, _ = _verify(engine, logn, sig, pk, hm, rule, want_norm=False)
    assert np.array_equal(st2, st)


# ---- 3. the bound, exactly -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [9, 10])
def test_the_bound_exactly(engine, logn):
    """norms beta^2 - 1, beta^2, beta^2 + 1 from four non-zero coefficients (tests/test_falcon_verify_rules.py: the oracle's circuit is
    satisfied by the first of these and by neither of the others)"""
    import falcon_r1cs_amd as frw
    _, pk, _ = frw.synth_triples(logn, 3, seed=5)
    sig, pk, hm, want = FV.bound_triples(logn, pk)
    st, nrm = _verify(engine, logn, sig, pk, hm, FV.RULE_CIRCUIT)
    assert st.tolist() == [OK, NORM_BOUND, NORM_BOUND] and nrm.tolist() == want
    assert np.array_equal(st, _compact_status(engine, logn, sig, pk, hm))
    st, nrm = _verify(engine, logn, sig, pk, hm, FV.RULE_SPEC)
    assert st.tolist() == [OK, OK, NORM_BOUND] and nrm.tolist() == want


# ---- 4. the coefficient 6144 -----------------------------------------------------------------------------------------------------------
def test_the_coefficient_6144(engine):
    import falcon_r1cs_amd as frw
    beta2 = FV.BETA2[10]
    sig, pk, hm, _ = FV.coeff_6144_triple(10, frw.synth_triples(10, 1, seed=6)[1][0])
    st, nrm = _verify(engine, 10, sig, pk, hm, FV.RULE_SPEC)
    assert st.tolist() == [OK] and nrm.tolist() == [beta2 - 1]
    st, nrm = _verify(engine, 10, sig, pk, hm, FV.RULE_CIRCUIT)
    assert st.tolist() == [NORM_BOUND] and nrm.tolist() == [beta2 + 12288]
    assert _compact_status(engine, 10, sig, pk, hm).tolist() == [NORM_BOUND]
    sig, pk, hm, _ = FV.coeff_6144_triple(9, frw.synth_triples(9, 1, seed=6)[1][0])
    for rule in RULES:
        assert _verify(engine, 9, sig, pk, hm, rule)[0].tolist() == [NORM_BOUND]


# ---- 5. the stride loop ----------------------------------------------------------------------------------------------------------------
def test_more_signatures_than_the_grid(engine):
    """4,099 Falcon-512 triples: a prime number, more than any grid the launcher picks (at most half the batch); every seventh invalid"""
    import torch
    import falcon_r1cs_amd as frw
    logn, batch = 9, 4099
    sig, pk, hm = (a.copy() for a in frw.synth_triples(logn, batch, seed=4099))
    rng = np.random.default_rng(4099)
    hm[0::14] = rng.integers(0, Q, (len(hm[0::14]), 512), dtype=np.uint16)       # NORM_BOUND
    pk[7::14, 100] = Q + 3                                                       # COEFF_RANGE
    want = torch.from_numpy(_compact_status(engine, logn, sig, pk, hm))
    got, nrm = _verify(engine, logn, sig, pk, hm, FV.RULE_CIRCUIT)
    got, nrm = torch.from_numpy(got), torch.from_numpy(nrm)
    assert torch.equal(got, want)
    bad = torch.arange(batch) % 7 == 0
    assert bool((want[bad] != OK).all()) and bool((want[~bad] == OK).all())
    assert torch.equal(nrm == -1, want == COEFF_RANGE) and int((want == COEFF_RANGE).sum()) == 293 and int((want == NORM_BOUND).sum()) == 293


# ---- 6. / 7. from bytes ----------------------------------------------------------------------------------------------------------------
def _cases(logn=None):
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        cases = json.load(f)["cases"]
    return [c for c in cases if logn is None or c["logn"] == logn]


def _spec_sum(pkb, msg, sgb, logn):
    """the sum oracle/falcon_sign.py's verify compares with beta^2, from its own pieces"""
    h = FC.modq_decode(pkb, logn)
    nonce, s2 = FC.comp_decode(sgb, logn)
    c = FC.hash_to_point(nonce, msg, logn)
    s1 = [(ci - x) % Q for ci, x in zip(c, S.mul_mod_q(s2, h))]
    centre = lambda x: x if x <= Q // 2 else x - Q
    return sum(centre(x) ** 2 for x in s1) + sum(centre(x) ** 2 for x in s2)


def _cpu_norm(pkb, msg, sgb, logn, rule):
    """the squared norm under `rule` from the oracle's codec and the numpy product (a refused message leaves v uniform, and a uniform
    v holds a coefficient of 6144 more often than not at N = 1024: the two rules' sums differ there)"""
    nonce, s2 = FC.comp_decode(sgb, logn)
    return int(FV.norms(np.array(s2), np.array(FC.modq_decode(pkb, logn)), np.array(FC.hash_to_point(nonce, msg, logn)), rule)[0])


def _from_bytes(engine, logn, pkb, sgb, msgs, rule):
    import torch
    d_st, d_nrm = engine.falcon_verify_from_bytes_dev(logn, pkb, sgb, msgs, rule, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_nrm.cpu().numpy()


def test_genuine_signatures_from_bytes_are_accepted_under_both_rules(engine):
    assert len(_cases()) == 4
    for logn in (9, 10):
        sel = _cases(logn)
        pkb, msgs, sgb = ([bytes.fromhex(c[k]) for c in sel] for k in ("pk_bytes", "msg", "sig_bytes"))
        want = [_spec_sum(*t, logn) for t in zip(pkb, msgs, sgb)]
        assert all(S.verify(*t, logn) for t in zip(pkb, msgs, sgb)) and all(w <= FV.BETA2[logn] for w in want)
        for rule in RULES:
            st, nrm = _from_bytes(engine, logn, pkb, sgb, msgs, rule)
            assert st.tolist() == [OK, OK] and nrm.tolist() == want, (logn, rule)
            h_st, h_nrm = engine.falcon_verify_from_bytes(logn, pkb, sgb, msgs, rule)       # strict: nothing to refuse
            assert h_st.tolist() == [OK, OK] and h_nrm.tolist() == want


@pytest.mark.parametrize("logn", [9, 10])
def test_tampered_bytes_are_refused_and_their_neighbours_are_not(engine, logn):
    import torch
    a, b = _cases(logn)
    pk_a, msg_a, sg_a = (bytes.fromhex(a[k]) for k in ("pk_bytes", "msg", "sig_bytes"))
    pk_b, msg_b, sg_b = (bytes.fromhex(b[k]) for k in ("pk_bytes", "msg", "sig_bytes"))
    msg_t = msg_a[:3] + bytes([msg_a[3] ^ 1]) + msg_a[4:]
    assert sg_a[-1] == 0                                                        # the padding the next line spoils
    key_12289 = pk_a[:1] + bytes([12289 >> 6, (12289 & 63) << 2 | (pk_a[2] & 3)]) + pk_a[3:]
    assert FC.modq_decode(key_12289, logn) is None
    good_a, good_b = (pk_a, sg_a, msg_a), (pk_b, sg_b, msg_b)
    tampered = [((pk_a, sg_a, msg_t), NORM_BOUND),                              # one message byte flipped
                ((pk_b, sg_a, msg_a), NORM_BOUND),                              # the other key of the same logn
                ((pk_a, bytes([sg_a[0] ^ 1]) + sg_a[1:], msg_a), DECODE),       # signature header
                ((pk_a, sg_a[:-1] + b"\x01", msg_a), DECODE),                   # a non-zero padding byte
                ((key_12289, sg_a, msg_a), DECODE),                             # a key coefficient of 12289
                ((bytes([pk_a[0] ^ 0x10]) + pk_a[1:], sg_a, msg_a), DECODE)]    # key header
    entries, want = [good_a], [OK]
    for k, (t, status) in enumerate(tampered):
        entries += [t, good_b if k % 2 else good_a]
        want += [status, OK]
    pkb, sgb, msgs = ([e[k] for e in entries] for k in range(3))
    oracle_accepts = [S.verify(p, m, s, logn) for p, s, m in entries]
    assert oracle_accepts == [w == OK for w in want]
    for rule in RULES:
        st, nrm = _from_bytes(engine, logn, pkb, sgb, msgs, rule)
        assert st.tolist() == want, rule
        assert ((nrm == -1) == (st == DECODE)).all()
        assert [int(x) for x in nrm[st != DECODE]] == [_cpu_norm(p, m, s, logn, rule) for (p, s, m), w in zip(entries, want) if w != DECODE]
        if rule == FV.RULE_SPEC:
            assert [int(x) for x in nrm[st != DECODE]] == [_spec_sum(p, m, s, logn) for (p, s, m), w in zip(entries, want) if w != DECODE]
            assert [s == OK for s in st.tolist()] == oracle_accepts
            # the host-buffer form: the same answers
            h_st, h_nrm = engine.falcon_verify_from_bytes(logn, pkb, sgb, msgs, rule, strict=False)
            assert np.array_equal(h_st, st) and np.array_equal(h_nrm.view(np.int64), nrm)
    # strict refuses the batch
    import falcon_r1cs_amd as frw
    with pytest.raises(frw.FrwError) as ei:
        engine.falcon_verify_from_bytes(logn, pkb, sgb, msgs)
    assert ei.value.code == -5
    # sig_len cut to 100: one length holds for a whole call, so every signature of that call is truncated and refused
    dev = torch.device("cuda:0")
    up = lambda blob: torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(np.cumsum([0, len(msg_a), len(msg_b)]).astype(np.int64)).to(dev)
    d_st, d_nrm = engine.falcon_verify_from_bytes_dev(logn, up(pk_a + pk_b), up(sg_a[:100] + sg_b[:100]), (up(msg_a + msg_b + b"\0"), d_off),
                                                      FV.RULE_SPEC, torch.cuda.current_stream().cuda_stream, sig_len=100)
    torch.cuda.synchronize()
    assert d_st.tolist() == [DECODE, DECODE] and d_nrm.tolist() == [-1, -1]
    assert FC.comp_decode(sg_a[:100], logn) is None


_AROUND_THE_RATE = []


def _signed_around_the_rate():
    """Falcon-512 signatures of messages of 0, 95, 96, 97 and 200 bytes under the first fixture key -> (pk_bytes, msgs, sigs); signed once"""
    if not _AROUND_THE_RATE:
        logn = 9
        case = _cases(logn)[0]
        seed = bytes.fromhex(case["key_seed"])
        sk = S.keygen(logn, seed)
        pk_bytes = sk.public_key_bytes()
        assert pk_bytes.hex() == case["pk_bytes"]
        lengths = [0, 95, 96, 97, 200]
        msgs = [bytes((7 * i + k) & 255 for i in range(k)) for k in lengths]
        sigs = [S.sign(sk, m, seed + bytes([k & 255])) for m, k in zip(msgs, lengths)]
        assert all(S.verify(pk_bytes, m, s, logn) for m, s in zip(msgs, sigs))
        _AROUND_THE_RATE.append((pk_bytes, msgs, sigs))
    return _AROUND_THE_RATE[0]


# ---- 8. message lengths around the SHAKE rate ------------------------------------------------------------------------------------------
def test_message_lengths_around_the_shake_rate(engine):
    """nonce || msg is 136 bytes, SHAKE256's rate, at a 96-byte message: 95, 96 and 97 straddle the block boundary; 0 is the empty
    message, 200 a third block.  Signed here with oracle/falcon_sign.py from the first fixture key's seed."""
    logn = 9
    pk_bytes, msgs, sigs = _signed_around_the_rate()
    want = [_spec_sum(pk_bytes, m, s, logn) for m, s in zip(msgs, sigs)]
    for rule in RULES:
        st, nrm = _from_bytes(engine, logn, [pk_bytes] * 5, sigs, msgs, rule)
        assert st.tolist() == [OK] * 5 and nrm.tolist() == want
    # each signature against its neighbour's message: one byte more or less moves the block boundary
    st, _ = _from_bytes(engine, logn, [pk_bytes] * 5, sigs, msgs[1:] + msgs[:1], FV.RULE_SPEC)
    assert st.tolist() == [NORM_BOUND] * 5


# ---- 9. host-buffer forms --------------------------------------------------------------------------------------------------------------
def test_host_buffer_forms_and_strict(engine):
    import falcon_r1cs_amd as frw
    logn = 10
    sig, pk, hm, want, ok, cpu = _mixed(engine, logn)
    sig, pk, hm = sig[:37], pk[:37], hm[:37]
    for rule in RULES:
        d_st, d_nrm = _verify(engine, logn, sig, pk, hm, rule)
        st, nrm = engine.falcon_verify(logn, sig, pk, hm, rule, strict=False)
        assert np.array_equal(st, d_st) and np.array_equal(nrm.view(np.int64), d_nrm)
    st, nrm = engine.falcon_verify(logn, sig, pk, hm, FV.RULE_SPEC, strict=False)                           # the rest: the specification's rule
    assert np.array_equal(st != OK, ~(ok[:37] & (FV.verdicts(cpu[FV.RULE_SPEC][:37], logn, FV.RULE_SPEC) == OK)))
    st2, none = engine.falcon_verify(logn, sig, pk, hm, FV.RULE_SPEC, strict=False, want_norm=False)        # norm = NULL
    assert none is None and np.array_equal(st2, st)
    with pytest.raises(frw.FrwError) as ei:
        engine.falcon_verify(logn, sig, pk, hm, FV.RULE_SPEC)
    assert ei.value.code == -5
    # strict through the C entry point itself: FRW_E_RANGE, and the buffers are complete all the same
    h_st = np.full(37, -7, dtype=np.int32)
    h_nrm = np.full(37, 5, dtype=np.uint64)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    s_, p_, h_ = (np.ascontiguousarray(a) for a in (sig, pk, hm))
    rc = engine._lib.frw_falcon_verify(engine._ctx, logn, 37, p(s_), p(p_), p(h_), FV.RULE_SPEC, p(h_st), p(h_nrm), 1)
    assert rc == -5 and np.array_equal(h_st, st) and np.array_equal(h_nrm, nrm)
    good = np.nonzero(st == OK)[0]
    st3, _ = engine.falcon_verify(logn, sig[good], pk[good], hm[good], FV.RULE_SPEC)                        # strict, nothing refused
    assert not st3.any()


# ---- 9b. the host-buffer forms past their first pass -----------------------------------------------------------------------------------
PASS = 16384                                         # signatures of one pass of the host-buffer forms (FALCON_VERIFY_CHUNK in frw_capi.cpp)


def _strict_is_e_range(rc, got, want):
    assert rc == -5
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_host_form_in_two_passes_equals_the_device_form(engine):
    """16,387 Falcon-512 triples = one full pass and three more, tiled from 131 valid ones (131 does not divide 16,384).  The device form
    does not chunk: its statuses and norms over the whole batch are the reference.  Slot 16,385 (second pass) has another hm."""
    import falcon_r1cs_amd as frw
    logn, batch, bad = 9, PASS + 3, PASS + 1
    tile = np.arange(batch) % 131
    sig, pk, hm = (a[tile] for a in frw.synth_triples(logn, 131, seed=16387))
    hm[bad] = np.random.default_rng(16387).integers(0, Q, 512, dtype=np.uint16)
    want_st, want_nrm = _verify(engine, logn, sig, pk, hm, FV.RULE_CIRCUIT)
    assert np.nonzero(want_st)[0].tolist() == [bad] and want_st[bad] == NORM_BOUND
    st, nrm = engine.falcon_verify(logn, sig, pk, hm, FV.RULE_CIRCUIT, strict=False)
    assert np.array_equal(st, want_st) and np.array_equal(nrm.view(np.int64), want_nrm)
    assert nrm[PASS] != nrm[0] and nrm[PASS] == nrm[PASS % 131]             # (the second pass is not the first one again)
    st2, none = engine.falcon_verify(logn, sig, pk, hm, FV.RULE_CIRCUIT, strict=False, want_norm=False)     # norm = NULL
    assert none is None and np.array_equal(st2, want_st)
    # strict through the C entry point itself: FRW_E_RANGE, and the buffers are complete all the same
    h_st, h_nrm = np.full(batch, -7, dtype=np.int32), np.full(batch, 5, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    s_, p_, h_ = (np.ascontiguousarray(a) for a in (sig, pk, hm))
    rc = engine._lib.frw_falcon_verify(engine._ctx, logn, batch, p(s_), p(p_), p(h_), FV.RULE_CIRCUIT, p(h_st), p(h_nrm), 1)
    _strict_is_e_range(rc, (h_st, h_nrm.view(np.int64)), (want_st, want_nrm))


def test_host_form_from_bytes_in_two_passes_equals_the_device_form(engine):
    """16,387 encoded Falcon-512 signatures tiled from the two genuine cases and five signed here over messages of 0, 95, 96, 97 and 200
    bytes: a period of 7, which does not divide 16,384, so the second pass's messages differ from those at the same positions of the
    first and their offsets have to be rebased.  Slot 16,385 has one message byte flipped."""
    import falcon_r1cs_amd as frw
    logn, batch, bad = 9, PASS + 3, PASS + 1
    pk_a, msgs_a, sigs_a = _signed_around_the_rate()
    seven = [(pk_a, m, s) for m, s in zip(msgs_a, sigs_a)] + [tuple(bytes.fromhex(c[k]) for k in ("pk_bytes", "msg", "sig_bytes")) for c in _cases(logn)]
    assert len(seven) == 7 and PASS % 7 and {len(t[1]) for t in seven} >= {0, 95, 96, 97, 200}
    entries = [seven[i % 7] for i in range(batch)]
    assert [e[1] for e in entries[PASS:PASS + 3]] != [e[1] for e in entries[:3]]
    k, m, s = entries[bad]
    assert len(m) > 3
    entries[bad] = (k, m[:3] + bytes([m[3] ^ 1]) + m[4:], s)
    pkb, msgs, sgb = ([e[j] for e in entries] for j in range(3))
    want_st, want_nrm = _from_bytes(engine, logn, pkb, sgb, msgs, FV.RULE_SPEC)
    assert np.nonzero(want_st)[0].tolist() == [bad] and want_st[bad] == NORM_BOUND
    assert want_nrm[:7].tolist() == [_spec_sum(*t, logn) for t in ((e[0], e[1], e[2]) for e in seven)]
    st, nrm = engine.falcon_verify_from_bytes(logn, pkb, sgb, msgs, FV.RULE_SPEC, strict=False)
    assert np.array_equal(st, want_st) and np.array_equal(nrm.view(np.int64), want_nrm)
    st2, none = engine.falcon_verify_from_bytes(logn, pkb, sgb, msgs, FV.RULE_SPEC, strict=False, want_norm=False)      # norm = NULL
    assert none is None and np.array_equal(st2, want_st)
    # strict through the C entry point itself: FRW_E_RANGE, and the buffers are complete all the same
    _, sig_len, a_pk, a_sg, blob, off = engine._falcon_verify_bytes(logn, pkb, sgb, msgs)
    h_st, h_nrm = np.full(batch, -7, dtype=np.int32), np.full(batch, 5, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = engine._lib.frw_falcon_verify_from_bytes(engine._ctx, logn, batch, p(a_pk), p(a_sg), sig_len, p(blob), p(off), FV.RULE_SPEC, p(h_st),
                                                  p(h_nrm), 1)
    _strict_is_e_range(rc, (h_st, h_nrm.view(np.int64)), (want_st, want_nrm))


# ---- 10. screening an aggregate --------------------------------------------------------------------------------------------------------
def test_screening_names_the_unprovable_statement_of_an_aggregate(engine):
    import torch
    import falcon_r1cs_amd as frw
    from test_gpu_aggregate import Aggregate
    dev = torch.device("cuda:0")
    logns = [9, 10, 9, 10]
    agg = Aggregate(engine, logns, seed=712)
    singles = {g: engine.r1cs_load(0, g) for g in (9, 10)}
    try:
        # the second Falcon-512 statement (statement 2) gets another message's hash
        triples = {g: [a.copy() for a in agg.triples[g]] for g in (9, 10)}
        triples[9][2][1] = np.random.default_rng(2).integers(0, Q, 512, dtype=np.uint16)
        per_set = {}
        for g in (9, 10):
            sig, pk, hm = triples[g]
            wit, inst = agg.batches[g]
            st = torch.empty(2, dtype=torch.int32, device=dev)
            engine.witness_ntt_verify_dev(g, 2, _dev(sig), _dev(pk), _dev(hm), wit, inst, st, 1, agg.s0)
            rows = torch.empty(2, dtype=torch.int32, device=dev)
            engine.r1cs_check_dev(singles[g], 2, wit, inst, rows, agg.s0)
            per_set[g] = (_verify(engine, g, sig, pk, hm, FV.RULE_CIRCUIT)[0], rows.cpu().numpy(), st.cpu().numpy())
        engine.aggregate_assign_dev(agg.handle, agg.batches[9][0], agg.batches[9][1], agg.batches[10][0], agg.batches[10][1], agg.wit, agg.inst, agg.s0)
        total = torch.empty(1, dtype=torch.int32, device=dev)
        engine.r1cs_check_dev(agg.handle, 1, agg.wit, agg.inst, total, agg.s0)
        torch.cuda.synchronize()
        # statement order: statement i takes the next unused entry of its parameter set
        used = {9: 0, 10: 0}
        screened, unsatisfied = [], []
        for g in logns:
            k = used[g]
            used[g] += 1
            screened.append(int(per_set[g][0][k]))
            unsatisfied.append(int(per_set[g][1][k]))
            assert per_set[g][0][k] == per_set[g][2][k]
        assert screened == [OK, OK, NORM_BOUND, OK]
        assert [u > 0 for u in unsatisfied] == [s != OK for s in screened]
        assert int(total[0]) == sum(unsatisfied) > 0        # the aggregate's unsatisfied rows are that statement's
    finally:
        for h in singles.values():
            engine.r1cs_free(h)
        agg.close()


# ---- 11. the example -------------------------------------------------------------------------------------------------------------------
def test_falcon_verify_example_exits_zero():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "falcon_verify.py"), os.path.join(ROOT, "tests", "golden", "falcon_signed.json")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "accepted" in out.stdout and "refused" in out.stdout
