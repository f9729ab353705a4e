"""The aggregate from bytes on the device (frw_aggregate_falcon_verify_from_bytes_dev, frw_aggregate_statement_from_bytes_dev,
frw_aggregate_prove_from_bytes_dev and their host-buffer forms): encoded (pk, msg, sig) triples of mixed parameter sets in statement
order -> verdicts, the verifier's statement, ONE proof on the wire.

Every comparison is against calls that were there before these: frw_falcon_verify_from_bytes_dev per parameter set for the screen;
frw_prepare_inputs per set and frw_aggregate_statement_dev for the statement; and for the proof the chain frw_prepare_inputs,
frw_witness_ntt_verify_dev, frw_aggregate_assign_dev, frw_groth16_prove_rs_dev, frw_groth16_proofs_to_wire_dev with the same (r, s).
Every output and every workspace is followed by 4,096 guard bytes of 0xA5 that must come back untouched.

The triples are tests/pok_prove_cases.py's, from the two golden genuine triples per parameter set only (repeated where more are needed):
nothing is signed here.  A refused statement's message may be anything -- its verdict is reached before the message matters -- so those
carry the messages of 0, 95, 96 and 97 bytes (nonce || msg fills SHAKE256's rate exactly at 96); a bad signature header leaves the key
intact, so such a statement's hashed message is still seen in the verifier's statement."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pok_prove_cases as PC

pytestmark = pytest.mark.gpu

GUARD = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_RANGE = -5
RULE_CIRCUIT, RULE_SPEC = 0, 1


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _logn(triple):
    return {897: 9, 1793: 10}[len(triple[0])]


def _with_msg(triple, length, tag):
    return triple[0], bytes((tag + 7 * i) & 255 for i in range(length)), triple[2]


def _restored(triple):
    """a bad_header triple with its header byte put back: the same key, nonce and message -- the verifier's statement of it"""
    pkb, msg, sgb = triple
    return (pkb, msg, bytes([0x30 + _logn(triple)]) + sgb[1:])


# ---- raw calls with guard regions -------------------------------------------------------------------------------------------------------
class Guarded:
    def __init__(self, sizes):
        import torch
        self.sizes = sizes
        self.bufs = {k: torch.full((v + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0") for k, v in sizes.items()}
        assert all(b.data_ptr() % 256 == 0 for b in self.bufs.values())

    def p(self, k):
        return C.c_void_p(self.bufs[k].data_ptr())

    def host(self):
        import torch
        torch.cuda.synchronize()
        out = {}
        for k, b in self.bufs.items():
            h = b.cpu().numpy()
            assert (h[self.sizes[k]:] == 0xA5).all(), "the guard region behind %s was written" % k
            out[k] = h[:self.sizes[k]]
        return out


def _upload(triples, nonces=None):
    import torch
    import falcon_r1cs_amd as frw
    arrays = frw.WitnessEngine._aggregate_bytes(triples, nonces)[1:]
    return [torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).to("cuda:0") for a in arrays]


def raw_screen(engine, handle, triples, rule):
    count = len(triples)
    ws_bytes = engine.aggregate_screen_workspace_bytes(handle)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    g = Guarded({"status": 4 * count, "norm": 8 * count, "workspace": ws_bytes})
    d = _upload(triples)
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = engine._lib.frw_aggregate_falcon_verify_from_bytes_dev(handle, engine._ctx, P(d[0]), P(d[1]), P(d[2]), P(d[3]), rule, g.p("status"),
                                                                g.p("norm"), g.p("workspace"), ws_bytes, C.c_void_p(_stream()))
    assert rc == 0, (rc, engine._lib.frw_last_error())
    h = g.host()
    # the one word the prover's host side reads: the last 16-byte piece of the layout (frw_layout.h aggregate_screen_layout)
    refused = int(h["workspace"][ws_bytes - 16:ws_bytes - 12].view(np.uint32)[0])
    return h["status"].view(np.int32).tolist(), h["norm"].view(np.uint64).tolist(), refused


def raw_statement(engine, handle, triples, encoding):
    count = len(triples)
    ni = int(engine.r1cs_info(handle).num_instance)
    ws_bytes = engine.aggregate_screen_workspace_bytes(handle)
    g = Guarded({"instance": 32 * ni, "status": 4 * count, "workspace": ws_bytes})
    d = _upload([(t[0], t[1]) for t in triples], [t[2][1:41] for t in triples])
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = engine._lib.frw_aggregate_statement_from_bytes_dev(handle, engine._ctx, P(d[0]), P(d[1]), P(d[2]), P(d[3]), encoding, g.p("instance"),
                                                            g.p("status"), g.p("workspace"), ws_bytes, C.c_void_p(_stream()))
    assert rc == 0, (rc, engine._lib.frw_last_error())
    h = g.host()
    return h["instance"].view(np.uint64).reshape(ni, 4), h["status"].view(np.int32).tolist()


def raw_prove(engine, key, handle, triples, rs, compressed=True):
    import torch
    import falcon_r1cs_amd as frw
    count = len(triples)
    ni = int(engine.r1cs_info(handle).num_instance)
    wire_len = frw.proof_wire_bytes(compressed)
    ws_bytes = engine.aggregate_prove_workspace_bytes(key, handle)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    g = Guarded({"wire": wire_len, "proof": 384, "instance": 32 * ni, "nonces": 40 * count, "status": 4 * count, "num_unsatisfied": 4,
                 "workspace": ws_bytes})
    d = _upload(triples)
    d_rs = torch.from_numpy(rs.reshape(8).view(np.int64).copy()).to("cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = engine._lib.frw_aggregate_prove_from_bytes_dev(engine._ctx, key, handle, P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d_rs),
                                                        0 if compressed else 1, g.p("wire"), g.p("proof"), g.p("instance"), g.p("nonces"),
                                                        g.p("status"), g.p("num_unsatisfied"), g.p("workspace"), ws_bytes, C.c_void_p(_stream()))
    assert rc in (0, E_RANGE), (rc, engine._lib.frw_last_error())
    h = g.host()
    return {"rc": rc, "wire": h["wire"], "proof": h["proof"].view(np.uint64), "instance": h["instance"].view(np.uint64).reshape(ni, 4),
            "nonces": h["nonces"].reshape(count, 40), "status": h["status"].view(np.int32).tolist(),
            "num_unsatisfied": int(h["num_unsatisfied"].view(np.uint32)[0])}


# ---- the references: calls that were there before -------------------------------------------------------------------------------------
def by_set(triples):
    """{logn: (the statements' indices, their triples)} in statement order"""
    out = {}
    for i, t in enumerate(triples):
        idx, ts = out.setdefault(_logn(t), ([], []))
        idx.append(i)
        ts.append(t)
    return out


def screen_reference(engine, triples, rule):
    import torch
    status, norm = [None] * len(triples), [None] * len(triples)
    for logn, (idx, ts) in by_set(triples).items():
        st, nm = engine.falcon_verify_from_bytes_dev(logn, [t[0] for t in ts], [t[2] for t in ts], [t[1] for t in ts], rule, _stream())
        torch.cuda.synchronize()
        for i, s, n in zip(idx, st.tolist(), nm.cpu().numpy().view(np.uint64).tolist()):
            status[i], norm[i] = s, n
    return status, norm


def statement_reference(engine, handle, triples, encoding):
    """frw_aggregate_statement_dev on frw_prepare_inputs' decoded keys and hashed messages -> instance uint64[I, 4]"""
    import torch
    dev = torch.device("cuda:0")
    d = {9: (None, None), 10: (None, None)}
    for logn, (idx, ts) in by_set(triples).items():
        _, pk, hm, _ = engine.prepare_inputs(logn, [t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts])
        d[logn] = tuple(torch.from_numpy(a.view(np.int16)).to(dev) for a in (pk, hm))
    ni = int(engine.r1cs_info(handle).num_instance)
    inst = torch.full((ni, 4), -1, dtype=torch.int64, device=dev)
    st = torch.full((len(triples),), -1, dtype=torch.int32, device=dev)
    engine.aggregate_statement_dev(handle, d[9][0], d[9][1], d[10][0], d[10][1], inst, st, encoding, _stream())
    torch.cuda.synchronize()
    return inst.cpu().numpy().view(np.uint64), st.tolist()


def slots(triples):
    """[(first element, elements)] of every statement's public inputs in the aggregate's instance vector"""
    out, at = [], 1
    for t in triples:
        n = 2 << _logn(t)
        out.append((at, n))
        at += n
    return out


def check_screen_and_statement(engine, handle, triples, want_status, through_host):
    refused = sum(s != PC.OK for s in want_status)
    for rule in (RULE_CIRCUIT, RULE_SPEC):
        ref_status, ref_norm = screen_reference(engine, triples, rule)
        if through_host:
            st, nm = engine.aggregate_falcon_verify_from_bytes(handle, triples, rule)
            st, nm = st.tolist(), nm.tolist()
        else:
            st, nm, cnt = raw_screen(engine, handle, triples, rule)
            assert cnt == sum(s != PC.OK for s in ref_status), "the refused count in the workspace"
        if rule == RULE_CIRCUIT:
            assert st == want_status
            assert through_host or cnt == refused
        assert st == ref_status and nm == ref_norm, "rule %d: not the per-set call's words" % rule
    # the verifier's statement: the same keys, nonces and messages, whatever became of the signatures
    as_sent = [_restored(t) if s == PC.DECODE and t[2][0] != 0x30 + _logn(t) else t for t, s in zip(triples, want_status)]
    for encoding in (0, 1):
        ref_inst, _ = statement_reference(engine, handle, as_sent, encoding)
        if through_host:
            inst, st = engine.aggregate_statement_from_bytes(handle, [t[0] for t in triples], [t[2][1:41] for t in triples],
                                                             [t[1] for t in triples], encoding)
            st = st.tolist()
        else:
            inst, st = raw_statement(engine, handle, triples, encoding)
        assert inst.tobytes() == ref_inst.tobytes(), "encoding %d: not frw_aggregate_statement_dev's bytes" % encoding
        one = [1, 0, 0, 0] if encoding == 0 else np.frombuffer(((1 << 256) % PC.R).to_bytes(32, "little"), dtype=np.uint64).tolist()
        assert inst[0].tolist() == one, "the constant one"
        bad_key = [i for i, t in enumerate(triples) if (t[0][1] << 6 | t[0][2] >> 2) >= 12289]
        assert st == [PC.DECODE if i in bad_key else PC.OK for i in range(len(triples))]
        for i, (at, n) in enumerate(slots(triples)):
            assert inst[at:at + n].any() == (i not in bad_key), "statement %d" % i


# ---- 1. routing: seven statements, no key --------------------------------------------------------------------------------------------
def seven():
    g9, g10 = PC.genuine(9, 2), PC.genuine(10, 2)
    triples = [g10[0], _with_msg(PC.bad_header(g9[0]), 97, 1), g9[0], PC.at_the_bound(10), _with_msg(PC.bad_key(g9[1]), 96, 2), g10[1], g9[1]]
    return triples, [PC.OK, PC.DECODE, PC.OK, PC.NORM_BOUND, PC.DECODE, PC.OK, PC.OK]


@pytest.fixture(scope="module")
def handle7(engine):
    triples, _ = seven()
    h = engine.r1cs_load_aggregate([_logn(t) for t in triples])
    assert int(engine.r1cs_info(h).log_domain_size) == 20
    yield h
    engine.r1cs_free(h)


@pytest.mark.parametrize("through_host", [False, True])
def test_seven_mixed_statements_are_routed_to_their_sets_and_back(engine, handle7, through_host):
    triples, want = seven()
    check_screen_and_statement(engine, handle7, triples, want, through_host)


# ---- 2. beyond one workgroup: 300 statements, no key -----------------------------------------------------------------------------------
def test_three_hundred_statements_beyond_one_workgroup(engine):
    g9, g10 = PC.genuine(9, 2), PC.genuine(10, 2)
    rng = random.Random(300)
    pool = [i for i in range(1, 299) if i not in (254, 255, 256, 257)]
    at10 = sorted(rng.sample(pool, 8) + [254, 257])             # Falcon-1024 statements on both sides of the workgroup's edge
    triples, want = [], []
    for i in range(300):
        t = g10[i & 1] if i in at10 else g9[i & 1]
        triples.append(t)
        want.append(PC.OK)
    assert [_logn(t) for t in triples].count(10) == 10 and not {0, 255, 256, 299} & set(at10)
    for pos, length, kind in ((0, 0, PC.bad_header), (255, 95, PC.bad_header), (256, 96, PC.bad_header), (299, 97, PC.bad_key)):
        triples[pos] = _with_msg(kind(triples[pos]), length, pos)
        want[pos] = PC.DECODE
    handle = engine.r1cs_load_aggregate([_logn(t) for t in triples])
    try:
        info = engine.r1cs_info(handle)
        assert int(info.num_constraints) + int(info.num_instance) < 1 << 25
        check_screen_and_statement(engine, handle, triples, want, False)
    finally:
        engine.r1cs_free(handle)


# ---- 3 - 5. the proof: handle (9, 10, 9), one key and one verifier ---------------------------------------------------------------------
class Proving:
    def __init__(self, engine):
        import falcon_r1cs_amd as frw
        self.engine = engine
        self.handle = engine.r1cs_load_aggregate([9, 10, 9])
        self.info = engine.r1cs_info(self.handle)
        assert int(self.info.log_domain_size) == 19
        rng = random.Random(9109)
        self.key, vk = engine.groth16_setup_r1cs(self.handle, *(rng.randrange(2, PC.R) for _ in range(5)))
        self.ver = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
        self.chains = {}

    def chain(self, triples, rs, compressed):
        """the existing calls -> dict(wire, proof, instance); the prover's part is cached per (order, rs)"""
        import torch
        import falcon_r1cs_amd as frw
        engine, dev, s0 = self.engine, torch.device("cuda:0"), _stream()
        tag = (tuple(triples), rs.tobytes())
        if tag not in self.chains:
            b = {9: (None, None), 10: (None, None)}
            for logn, (idx, ts) in by_set(triples).items():
                sig, pk, hm, st = engine.prepare_inputs(logn, [t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts])
                assert not st.any()
                L = frw.layout(logn)
                d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
                wit = torch.empty((len(ts), L.num_witness, 4), dtype=torch.int64, device=dev)
                inst = torch.empty((len(ts), L.num_instance, 4), dtype=torch.int64, device=dev)
                wst = torch.empty(len(ts), dtype=torch.int32, device=dev)
                engine.witness_ntt_verify_dev(logn, len(ts), d[0], d[1], d[2], wit, inst, wst, frw.ENC_MONTGOMERY, s0)
                torch.cuda.synchronize()
                assert not wst.any()
                b[logn] = (wit, inst)
            awit = torch.empty((1, int(self.info.num_witness), 4), dtype=torch.int64, device=dev)
            ainst = torch.empty((1, int(self.info.num_instance), 4), dtype=torch.int64, device=dev)
            engine.aggregate_assign_dev(self.handle, b[9][0], b[9][1], b[10][0], b[10][1], awit, ainst, s0)
            ws_bytes = engine.groth16_workspace_bytes(self.key, self.handle, 1)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            proof = torch.empty((1, 48), dtype=torch.int64, device=dev)
            bad = torch.empty(1, dtype=torch.int32, device=dev)
            d_rs = torch.from_numpy(rs.reshape(1, 2, 4).view(np.int64).copy()).to(dev)
            engine.groth16_prove_rs_dev(self.key, self.handle, 1, awit, ainst, d_rs, proof, ws, ws_bytes, bad, s0)
            torch.cuda.synchronize()
            assert bad.tolist() == [0]
            self.chains[tag] = (proof, ainst[0].cpu().numpy().view(np.uint64))
        proof, inst = self.chains[tag]
        wire, wire_status = frw.proofs_to_wire_dev(proof, compressed, s0)
        torch.cuda.synchronize()
        assert wire_status.tolist() == [0]
        return {"wire": wire[0].cpu().numpy(), "proof": proof[0].cpu().numpy().view(np.uint64), "instance": inst}

    def close(self):
        self.ver.close()
        self.engine.groth16_pk_free(self.key)
        self.engine.r1cs_free(self.handle)


@pytest.fixture(scope="module")
def proving(engine):
    p = Proving(engine)
    yield p
    p.close()


def three():
    g9, g10 = PC.genuine(9, 2), PC.genuine(10, 2)
    return [g9[1], g10[0], g9[0]]                               # (the golden file's second Falcon-512 message is the empty one: not last)


def test_one_call_gives_the_chains_proof_and_the_verifier_accepts_it(engine, proving):
    import torch
    triples, rs = three(), PC.blinding("aggregate 9 10 9")
    first = None
    for compressed in (True, False):
        out = raw_prove(engine, proving.key, proving.handle, triples, rs, compressed)
        ref = proving.chain(triples, rs, compressed)
        assert out["rc"] == 0 and out["status"] == [0, 0, 0] and out["num_unsatisfied"] == 0
        assert out["wire"].tobytes() == ref["wire"].tobytes(), "wire bytes differ from the chain's"
        assert out["proof"].tolist() == ref["proof"].tolist(), "limbs differ from the chain's"
        assert out["instance"].tobytes() == ref["instance"].tobytes(), "instance differs from the chain's"
        assert out["nonces"].tobytes() == b"".join(t[2][1:41] for t in triples)
        first = first or out
    # the verifier's half: key bytes, nonces, messages and wire bytes alone
    pks, nonces, msgs = [t[0] for t in triples], [bytes(n) for n in first["nonces"]], [t[1] for t in triples]
    st, verdict = proving.ver.verify_aggregate_wire_dev(engine, proving.handle, pks, nonces, msgs, first["wire"].tobytes(), True, stream=_stream())
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0, 0] and verdict.tolist() == [1]
    changed = msgs[:2] + [msgs[2][:-1] + bytes([msgs[2][-1] ^ 1])]
    st, verdict = proving.ver.verify_aggregate_wire_dev(engine, proving.handle, pks, nonces, changed, first["wire"].tobytes(), True, stream=_stream())
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0, 0] and verdict.tolist() == [0]
    # statements 0 and 2 exchanged: the chain's proof for that order, and another proof than the first
    swapped = [triples[2], triples[1], triples[0]]
    out = raw_prove(engine, proving.key, proving.handle, swapped, rs, True)
    ref = proving.chain(swapped, rs, True)
    assert out["rc"] == 0 and out["status"] == [0, 0, 0] and out["num_unsatisfied"] == 0
    assert out["wire"].tobytes() == ref["wire"].tobytes() and out["proof"].tolist() == ref["proof"].tolist()
    assert out["instance"].tobytes() == ref["instance"].tobytes()
    assert out["wire"].tobytes() != first["wire"].tobytes()


def refusals():
    t = three()
    return {"bad_header at 2": ([t[0], t[1], PC.bad_header(t[2])], [PC.OK, PC.OK, PC.DECODE]),
            "bad_key at 1": ([t[0], PC.bad_key(t[1]), t[2]], [PC.OK, PC.DECODE, PC.OK]),
            "at_the_bound at 0": ([PC.at_the_bound(9), t[1], t[2]], [PC.NORM_BOUND, PC.OK, PC.OK])}


@pytest.mark.parametrize("case", sorted(refusals()))
def test_a_refused_statement_means_no_proof(engine, proving, case):
    triples, want = refusals()[case]
    out = raw_prove(engine, proving.key, proving.handle, triples, PC.blinding(case), True)
    assert out["rc"] == E_RANGE
    assert out["status"] == want
    assert not out["wire"].any() and not out["proof"].any()
    assert out["num_unsatisfied"] == 0xFFFFFFFF
    inst, _ = raw_statement(engine, proving.handle, triples, 1)
    assert out["instance"].tobytes() == inst.tobytes(), "the instance vector is the statement call's"
    assert out["nonces"].tobytes() == b"".join(t[2][1:41] for t in triples)


def test_the_host_form_equals_the_device_form(engine, proving):
    accepted, rs = three(), PC.blinding("aggregate host")
    refused, want = refusals()["bad_header at 2"]
    for triples, rc, status in ((accepted, 0, [0, 0, 0]), (refused, E_RANGE, want)):
        dev = raw_prove(engine, proving.key, proving.handle, triples, rs, True)
        host = engine.aggregate_prove_from_bytes(proving.key, proving.handle, triples, rs, compressed=True, strict=False)
        assert host["rc"] == dev["rc"] == rc and host["status"].tolist() == dev["status"] == status
        assert host["wire"].tobytes() == dev["wire"].tobytes() and host["proof"].tolist() == dev["proof"].tolist()
        assert host["instance"].tobytes() == dev["instance"].tobytes() and host["nonces"].tobytes() == dev["nonces"].tobytes()
        assert int(host["num_unsatisfied"][0]) == dev["num_unsatisfied"]


# ---- 6. the example --------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_to_exit_status_zero():
    """examples/aggregate_pok.py in a fresh child process: setup, ONE call to the proof bytes, the verifier accepts them from (pk bytes,
    nonces, msgs, proof bytes) alone and rejects them with one message byte changed."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "aggregate_pok.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-4000:]
    assert "accepted" in res.stdout and "rejected" in res.stdout, res.stdout[-4000:]
