"""The codec kernels of falcon-r1cs_amd/csrc/frw_prepare.hip on the catalogue of tests/falcon_codec_cases.py, against oracle/falcon_codec.py:
frw_decode_signatures_dev (with and without a nonce output), frw_decode_public_keys_dev and frw_hash_to_point_dev on their own, then the
calls that chain them -- frw_prepare_inputs, frw_falcon_verify_from_bytes_dev and the routed kernels of
frw_aggregate_falcon_verify_from_bytes_dev.  Every comparison is exact: status words, uint16 coefficients, nonce bytes, norms (a numpy
negacyclic product of the oracle's decoded vectors, tests/falcon_verify_cases.py).

Every output buffer is pre-filled with a sentinel (0xFFFF coefficient rows, 0x7F7F7F7F status words, 0xEE nonce rows) and followed by
4,096 guard bytes of 0xA5 that must come back intact.  A refused signature's own row is unspecified and is not compared; the rows of
its neighbours are.  That the catalogue holds what it should is tests/test_falcon_codec_cases.py's business, without a device."""
import ctypes as C
import random

import numpy as np
import pytest

import falcon_codec_cases as CC
import falcon_verify_cases as FV
import frw_testlib as T
import pok_prove_cases as PC
from oracle import falcon_codec as FC

pytestmark = pytest.mark.gpu

OK, DECODE = 0, 3
E_INVALID_ARG = -1
ROW, STATUS, NONCE, NORM = 0xFF, 0x7F, 0xEE, 0x5C          # the sentinels, byte by byte
RULES = (FV.RULE_CIRCUIT, FV.RULE_SPEC)


@pytest.fixture(scope="module")
def cat():
    return CC.catalogue()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).to("cuda:0")


def _bytes_dev(items):
    return _dev(np.frombuffer(b"".join(bytes(x) for x in items) or b"\0", dtype=np.uint8))


class Out:
    """An output of `nbytes` bytes, every byte the sentinel, with T.GUARD_BYTES of 0xA5 right behind it"""

    def __init__(self, nbytes, sentinel):
        self.nbytes, self.sentinel = nbytes, sentinel
        self.buf, self.t = T.guarded_workspace(nbytes, "cuda:0")
        self.t.fill_(sentinel)

    def host(self, dtype=np.uint8):
        import torch
        torch.cuda.synchronize()
        assert T.guard_intact(self.buf), "the guard region behind an output was written"
        return self.buf[:self.nbytes].cpu().numpy().view(dtype)

    def untouched(self):
        return bool((self.host() == self.sentinel).all())


def _rows_equal(got, want_rows, names):
    """got[i] == want_rows[i] wherever want_rows[i] is not None; the first case that differs is named"""
    for i, w in enumerate(want_rows):
        if w is not None and got[i].tolist() != list(w):
            k = next(j for j in range(len(w)) if got[i, j] != w[j])
            raise AssertionError("%s (item %d): coefficient %d is %d, the oracle says %d" % (names[i], i, k, got[i, k], w[k]))


# ---- frw_decode_signatures_dev --------------------------------------------------------------------------------------------------------------
def decode_signatures(engine, logn, cases, with_nonce=True):
    n, batch, sig_len = 1 << logn, len(cases), cases[0].sig_len
    assert all(c.sig_len == sig_len for c in cases)
    rows, st, nonce = Out(batch * n * 2, ROW), Out(batch * 4, STATUS), Out(batch * 40, NONCE)
    d_in = _bytes_dev([c.data for c in cases])
    engine.decode_signatures_dev(logn, batch, d_in, sig_len, rows.t, nonce.t if with_nonce else None, st.t, _stream())
    return rows.host(np.uint16).reshape(batch, n), st.host(np.int32), nonce.host().reshape(batch, 40)


def check_signatures(engine, logn, cases, with_nonce=True):
    rows, st, nonce = decode_signatures(engine, logn, cases, with_nonce)
    names = [c.name for c in cases]
    want = [OK if c.accepted else DECODE for c in cases]
    assert st.tolist() == want, [(c.name, int(s)) for c, s, w in zip(cases, st, want) if s != w][:8]
    _rows_equal(rows, [c.want[1] if c.accepted else None for c in cases], names)
    if not with_nonce:
        assert (nonce == NONCE).all()
        return
    for i, c in enumerate(cases):
        if c.accepted:
            assert nonce[i].tobytes() == c.data[1:41] == c.want[0], c.name
        if c.data[0] != 0x30 + logn:                            # the nonce is copied out only behind the expected header
            assert (nonce[i] == NONCE).all(), c.name


@pytest.mark.parametrize("with_nonce", [True, False])
@pytest.mark.parametrize("logn", CC.LOGNS)
def test_decode_signatures_every_sig_len_group(engine, cat, logn, with_nonce):
    """one call per sig_len, accepted and refused cases shuffled so that the lanes of a wavefront diverge"""
    seen = 0
    for sig_len, cases in sorted(cat.groups(logn).items()):
        cases = [c for c in cases if c.on_device]
        if not cases:
            continue
        random.Random(1000 * logn + sig_len).shuffle(cases)
        check_signatures(engine, logn, cases, with_nonce)
        seen += len(cases)
    assert seen == len(cat.signatures(logn)) - 1                # all but the case without a body (sig_len 41: an argument error, below)


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_decode_signatures_batches_around_a_wavefront_and_a_workgroup(engine, cat, logn):
    cases = list(cat.standard(logn))
    random.Random(77 + logn).shuffle(cases)
    assert len(cases) >= 257
    for batch in (1, 63, 64, 65, 257):
        part = cases[:batch]
        assert batch == 1 or {c.accepted for c in part} == {True, False}
        check_signatures(engine, logn, part)
    check_signatures(engine, logn, [next(c for c in cases if not c.accepted)])
    check_signatures(engine, logn, [next(c for c in cases if c.accepted)])


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_a_sig_len_without_a_body_is_an_argument_error_and_writes_nothing(engine, logn):
    import falcon_r1cs_amd as frw
    n = 1 << logn
    for sig_len in (0, 1, 40, 41):
        rows, st, nonce = Out(4 * n * 2, ROW), Out(4 * 4, STATUS), Out(4 * 40, NONCE)
        d_in = _bytes_dev([bytes([0x30 + logn]) + bytes(63)] * 4)
        with pytest.raises(frw.FrwError) as e:
            engine.decode_signatures_dev(logn, 4, d_in, sig_len, rows.t, nonce.t, st.t, _stream())
        assert e.value.code == E_INVALID_ARG
        assert rows.untouched() and st.untouched() and nonce.untouched()


# ---- frw_decode_public_keys_dev -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", CC.LOGNS)
def test_decode_public_keys(engine, cat, logn):
    n = 1 << logn
    ks = list(cat.keys[logn])
    random.Random(31 + logn).shuffle(ks)
    batch = len(ks)
    assert batch >= 70 and batch * n > 4 * 256                  # several workgroups, a key spread over more than one
    rows, st = Out(batch * n * 2, ROW), Out(batch * 4, STATUS)
    engine.decode_public_keys_dev(logn, batch, _bytes_dev([k.data for k in ks]), rows.t, st.t, _stream())
    got, status = rows.host(np.uint16).reshape(batch, n), st.host(np.int32)
    want = [OK if k.accepted else DECODE for k in ks]
    assert status.tolist() == want, [(k.name, int(s)) for k, s, w in zip(ks, status, want) if s != w][:8]
    _rows_equal(got, [k.want for k in ks], [k.name for k in ks])
    # a refused key next to accepted ones on both sides somewhere: it taints neither
    assert any(not ks[i].accepted and ks[i - 1].accepted and ks[i + 1].accepted for i in range(1, batch - 1))


# ---- frw_hash_to_point_dev --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", CC.LOGNS)
def test_hash_to_point(engine, cat, logn):
    n = 1 << logn
    hs = cat.hashes[logn]
    batch = len(hs)
    off = np.zeros(batch + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(h.msg) for h in hs])
    rows = Out(batch * n * 2, ROW)
    engine.hash_to_point_dev(logn, batch, _bytes_dev([h.nonce for h in hs]), _bytes_dev([h.msg for h in hs]), _dev(off), rows.t, _stream())
    _rows_equal(rows.host(np.uint16).reshape(batch, n), [h.want for h in hs], [h.name for h in hs])


# ---- the calls that chain the three ---------------------------------------------------------------------------------------------------------
class Triple:
    """(key case or genuine key bytes, message, signature case or genuine signature bytes) with the oracle's view of it"""

    def __init__(self, logn, key, msg, sig):
        self.logn, self.msg = logn, bytes(msg)
        self.pk_bytes, self.sig_bytes = bytes(getattr(key, "data", key)), bytes(getattr(sig, "data", sig))
        self.pk = FC.modq_decode(self.pk_bytes, logn)
        decoded = FC.comp_decode(self.sig_bytes, logn)
        self.sig = decoded[1] if decoded else None
        self.accepted = self.pk is not None and self.sig is not None
        self.hm = FC.hash_to_point(decoded[0], self.msg, logn) if decoded else None
        self.name = "%s | %s" % (getattr(key, "name", "genuine key"), getattr(sig, "name", "genuine signature"))

    def norm(self, rule):
        return int(FV.norms([self.sig], [self.pk], [self.hm], rule)[0]) if self.accepted else -1

    def status(self, rule):
        return int(FV.verdicts([self.norm(rule)], self.logn, rule)[0]) if self.accepted else DECODE


_QUADRANTS = {}


def quadrants(cat, logn, per):
    """`per` triples in each combination of good or bad key and accepted or refused standard-length signature, shuffled; the two genuine
    triples of tests/golden/falcon_signed.json among the good ones, so that FRW_ST_OK occurs.  Built once per (logn, per), never written."""
    if (logn, per) not in _QUADRANTS:
        rng = random.Random(500 + logn)
        good_k, bad_k = ([k for k in cat.keys[logn] if k.accepted == a] for a in (True, False))
        good_s, bad_s = ([c for c in cat.standard(logn) if c.accepted == a] for a in (True, False))
        out = [Triple(logn, *g) for g in PC.genuine(logn, 2)]
        for ks, ss, count in ((good_k, good_s, per - 2), (good_k, bad_s, per), (bad_k, good_s, per), (bad_k, bad_s, per)):
            for i, (k, s) in enumerate(zip(rng.sample(ks, count), rng.sample(ss, count))):
                out.append(Triple(logn, k, bytes(rng.randrange(256) for _ in range((0, 95, 96, 97, 200)[i % 5])), s))
        rng.shuffle(out)
        _QUADRANTS[logn, per] = out
    return _QUADRANTS[logn, per]


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_prepare_inputs_host_form(engine, cat, logn):
    """frw_prepare_inputs: status is the signature's where that is non-zero, else the key's (both FRW_ST_DECODE); the three rows of
    every accepted item"""
    import falcon_r1cs_amd as frw
    n = 1 << logn
    ts = quadrants(cat, logn, 16)
    batch, sig_len, pkb, sgb, blob, off = frw.WitnessEngine._falcon_verify_bytes(logn, [t.pk_bytes for t in ts], [t.sig_bytes for t in ts],
                                                                                 [t.msg for t in ts])
    guard = T.GUARD_BYTES
    outs = [np.concatenate([np.full(batch * n * 2, ROW, dtype=np.uint8), np.full(guard, 0xA5, dtype=np.uint8)]) for _ in range(3)]
    st = np.concatenate([np.full(batch * 4, STATUS, dtype=np.uint8), np.full(guard, 0xA5, dtype=np.uint8)])
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = engine._lib.frw_prepare_inputs(engine._ctx, logn, batch, P(pkb), P(sgb), sig_len, P(blob), P(off), P(outs[0]), P(outs[1]), P(outs[2]), P(st))
    assert rc == 0, (rc, engine._lib.frw_last_error())
    assert all((a[-guard:] == 0xA5).all() for a in outs + [st])
    status = st[:-guard].view(np.int32)
    assert status.tolist() == [OK if t.accepted else DECODE for t in ts]
    assert {(t.pk is None, t.sig is None) for t in ts} == {(a, b) for a in (False, True) for b in (False, True)}
    sig, pk, hm = (a[:-guard].view(np.uint16).reshape(batch, n) for a in outs)
    names = [t.name for t in ts]
    for got, field in ((sig, "sig"), (pk, "pk"), (hm, "hm")):
        _rows_equal(got, [getattr(t, field) if t.accepted else None for t in ts], names)


def _screen_outputs(count, ws_bytes):
    import torch
    st, norm = Out(count * 4, STATUS), Out(count * 8, NORM)
    ws_buf, ws = T.guarded_workspace(ws_bytes, torch.device("cuda:0"))
    return st, norm, ws_buf, ws


def _check_screen(ts, st, norm, ws_buf, rule):
    status, norms = st.host(np.int32).tolist(), norm.host(np.int64).tolist()
    assert T.guard_intact(ws_buf), "the guard region behind the workspace was written"
    want_status, want_norm = [t.status(rule) for t in ts], [t.norm(rule) for t in ts]
    assert status == want_status, [(t.name, s, w) for t, s, w in zip(ts, status, want_status) if s != w][:8]
    assert norms == want_norm, [(t.name, s, w) for t, s, w in zip(ts, norms, want_norm) if s != w][:8]
    assert {OK, DECODE, 2} <= set(want_status)                  # a genuine one, refused ones, and norms beyond the bound


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("logn", CC.LOGNS)
def test_falcon_verify_from_bytes_dev(engine, cat, logn, rule):
    """64 triples: FRW_ST_DECODE and norm -1 where the key or the signature is refused, else the verdict and the norm of the oracle's
    decoded vectors"""
    import falcon_r1cs_amd as frw
    ts = quadrants(cat, logn, 16)
    assert len(ts) == 64
    batch, sig_len, pkb, sgb, blob, off = frw.WitnessEngine._falcon_verify_bytes(logn, [t.pk_bytes for t in ts], [t.sig_bytes for t in ts],
                                                                                 [t.msg for t in ts])
    d = [_dev(a) for a in (pkb, sgb, blob, off)]
    ws_bytes = engine.falcon_verify_workspace_bytes(logn, batch)
    st, norm, ws_buf, ws = _screen_outputs(batch, ws_bytes)
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = engine._lib.frw_falcon_verify_from_bytes_dev(engine._ctx, logn, batch, P(d[0]), P(d[1]), sig_len, P(d[2]), P(d[3]), rule, P(st.t), P(norm.t),
                                                      P(ws), ws_bytes, C.c_void_p(_stream()))
    assert rc == 0, (rc, engine._lib.frw_last_error())
    _check_screen(ts, st, norm, ws_buf, rule)


@pytest.fixture(scope="module")
def handle12(engine):
    h = engine.r1cs_load_aggregate([9, 10] * 6)
    yield h
    engine.r1cs_free(h)


@pytest.mark.parametrize("rule", RULES)
def test_aggregate_falcon_verify_from_bytes_dev(engine, cat, handle12, rule):
    """twelve statements alternating the two parameter sets: the routed kernels read keys (897 / 1793 bytes) and signatures (666 / 1280)
    laid end to end, so at byte offsets of every residue mod 4; refused signatures and refused keys of both sets among them.  Held to
    the oracle and numpy statement by statement, not to the per-set device call."""
    import falcon_r1cs_amd as frw
    pick = {g: {} for g in CC.LOGNS}
    for g in CC.LOGNS:
        for t in quadrants(cat, g, 16):
            kind = "ok" if t.accepted and t.status(rule) == OK else "norm" if t.accepted else "bad-key" if t.sig is not None else "bad-sig" if t.pk is not None else "both"
            pick[g].setdefault(kind, []).append(t)
    order = ("ok", "bad-sig", "norm", "bad-key", "both", "ok")
    ts = [pick[g][kind][-1 if i == 5 else 0] for i, kind in enumerate(order) for g in CC.LOGNS]
    assert [t.logn for t in ts] == [9, 10] * 6
    count, pkb, sgb, blob, off = frw.WitnessEngine._aggregate_bytes([(t.pk_bytes, t.msg, t.sig_bytes) for t in ts])
    pk_at = np.cumsum([0] + [len(t.pk_bytes) for t in ts[:-1]])
    sig_at = np.cumsum([0] + [len(t.sig_bytes) for t in ts[:-1]])
    assert {int(x) % 4 for x in pk_at} == {0, 1, 2, 3} and len({int(x) % 4 for x in sig_at}) >= 2
    d = [_dev(a) for a in (pkb, sgb, blob, off)]
    ws_bytes = engine.aggregate_screen_workspace_bytes(handle12)
    st, norm, ws_buf, ws = _screen_outputs(count, ws_bytes)
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = engine._lib.frw_aggregate_falcon_verify_from_bytes_dev(handle12, engine._ctx, P(d[0]), P(d[1]), P(d[2]), P(d[3]), rule, P(st.t), P(norm.t),
                                                                P(ws), ws_bytes, C.c_void_p(_stream()))
    assert rc == 0, (rc, engine._lib.frw_last_error())
    _check_screen(ts, st, norm, ws_buf, rule)
