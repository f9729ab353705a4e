"""The Python binding's own work, without a device: how the encoded inputs of the *_from_bytes calls are packed (the joined keys,
the joined signatures or nonces, the message blob and its offsets), which lengths are refused with which words, what the pointer
rule makes of an address and of a tensor, and the error a verifying key of a wrong length raises.  The expected arrays are written
out from the format, not computed by the code under test."""
import numpy as np
import pytest

import falcon_r1cs_amd as frw

E = frw.WitnessEngine
ZERO = [0]                                             # an empty join is one zero byte, so that the array has an address


def key(logn, fill):
    return bytes([fill]) * frw.PK_LEN[logn]


def sig(logn, fill):
    return bytes([fill]) * frw.SIG_LEN[logn]


def nonce(fill):
    return bytes([fill]) * frw.NONCE_LEN


def same(got, want, dtype):
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.ndim == 1, (got.dtype, got.shape)
    assert got.tolist() == list(want)


# (messages, the blob's bytes, the offsets), written out by hand
PACK_CASES = [
    ([], ZERO, [0]),                                                           # batch 0
    ([b"abc"], [97, 98, 99], [0, 3]),                                          # batch 1
    ([b"ab", b"", b"xyz"], [97, 98, 120, 121, 122], [0, 2, 2, 5]),             # batch 3, the middle message empty
    ([b"", b""], ZERO, [0, 0, 0]),                                             # batch 2, both messages empty: the placeholder blob
]


@pytest.mark.parametrize("logn", [9, 10])
@pytest.mark.parametrize("msgs,blob,offsets", PACK_CASES)
def test_statement_bytes_packs_keys_nonces_and_messages(logn, msgs, blob, offsets):
    batch = len(msgs)
    got = E._statement_bytes(logn, [key(logn, 1 + i) for i in range(batch)], [nonce(101 + i) for i in range(batch)], msgs)
    assert isinstance(got, tuple) and len(got) == 5 and got[0] == batch
    same(got[1], sum(([1 + i] * frw.PK_LEN[logn] for i in range(batch)), []) or ZERO, np.uint8)
    same(got[2], sum(([101 + i] * 40 for i in range(batch)), []) or ZERO, np.uint8)
    same(got[3], blob, np.uint8)
    same(got[4], offsets, np.uint64)


@pytest.mark.parametrize("logn", [9, 10])
@pytest.mark.parametrize("msgs,blob,offsets", PACK_CASES)
def test_falcon_verify_bytes_packs_keys_signatures_and_messages(logn, msgs, blob, offsets):
    batch = len(msgs)
    got = E._falcon_verify_bytes(logn, [key(logn, 1 + i) for i in range(batch)], [sig(logn, 201 + i) for i in range(batch)], msgs)
    assert isinstance(got, tuple) and len(got) == 6 and got[0] == batch
    assert got[1] == frw.SIG_LEN[logn]                  # the common length; the parameter set's own for an empty batch
    same(got[2], sum(([1 + i] * frw.PK_LEN[logn] for i in range(batch)), []) or ZERO, np.uint8)
    same(got[3], sum(([201 + i] * frw.SIG_LEN[logn] for i in range(batch)), []) or ZERO, np.uint8)
    same(got[4], blob, np.uint8)
    same(got[5], offsets, np.uint64)


def test_falcon_verify_bytes_takes_the_common_signature_length_from_the_signatures():
    got = E._falcon_verify_bytes(9, [key(9, 7)], [b"\x39" + bytes(49)], [b"m"])
    assert got[1] == 50
    same(got[3], [0x39] + [0] * 49, np.uint8)


def test_aggregate_bytes_mixed_parameter_sets_in_statement_order():
    logns = [9, 10, 9]
    msgs = [b"one", b"", b"three"]
    triples = [(key(g, 1 + i), msgs[i], sig(g, 201 + i)) for i, g in enumerate(logns)]
    keys = [1] * 897 + [2] * 1793 + [3] * 897
    blob = [111, 110, 101, 116, 104, 114, 101, 101]    # "one" + "" + "three"
    got = E._aggregate_bytes(triples)
    assert isinstance(got, tuple) and len(got) == 5 and got[0] == 3
    same(got[1], keys, np.uint8)
    same(got[2], [201] * 666 + [202] * 1280 + [203] * 666, np.uint8)
    same(got[3], blob, np.uint8)
    same(got[4], [0, 3, 3, 8], np.uint64)
    got = E._aggregate_bytes([t[:2] for t in triples], [nonce(101 + i) for i in range(3)])
    assert isinstance(got, tuple) and len(got) == 5 and got[0] == 3
    same(got[1], keys, np.uint8)
    same(got[2], [101] * 40 + [102] * 40 + [103] * 40, np.uint8)
    same(got[3], blob, np.uint8)
    same(got[4], [0, 3, 3, 8], np.uint64)


def test_aggregate_bytes_of_no_statement():
    got = E._aggregate_bytes([])
    assert got[0] == 0
    for arr in got[1:4]:
        same(arr, ZERO, np.uint8)
    same(got[4], [0], np.uint64)


def test_aggregate_bytes_refusals():
    pairs = [(key(9, 1), b"a"), (key(10, 2), b"b")]
    with pytest.raises(ValueError) as e:
        E._aggregate_bytes(pairs, [nonce(5)])
    assert str(e.value) == "one nonce per statement"
    with pytest.raises(ValueError) as e:
        E._aggregate_bytes([(key(9, 1), b"a", sig(9, 3)), (key(10, 2), b"b", sig(9, 4))])
    assert str(e.value) == "statement 1: a key of 897 or 1793 bytes and a signature of 666 or 1280 (a nonce of 40)"
    with pytest.raises(ValueError) as e:
        E._aggregate_bytes([(key(9, 1)[:-1], b"a", sig(9, 3))])
    assert str(e.value) == "statement 0: a key of 897 or 1793 bytes and a signature of 666 or 1280 (a nonce of 40)"
    with pytest.raises(ValueError) as e:
        E._aggregate_bytes(pairs, [nonce(5), nonce(6) + b"\0"])
    assert str(e.value) == "statement 1: a key of 897 or 1793 bytes and a signature of 666 or 1280 (a nonce of 40)"


@pytest.mark.parametrize("logn,klen", [(9, 897), (10, 1793)])
def test_statement_bytes_refusals(logn, klen):
    lengths = "public keys must be %d bytes and nonces 40" % klen
    for args, text in ((([key(logn, 1)], [], [b"m"]), "batch mismatch"),
                       (([key(logn, 1)], [nonce(2)], []), "batch mismatch"),
                       (([key(logn, 1) + b"\0"], [nonce(2)], [b"m"]), lengths),
                       (([key(logn, 1)], [nonce(2)[:-1]], [b"m"]), lengths)):
        with pytest.raises(ValueError) as e:
            E._statement_bytes(logn, *args)
        assert str(e.value) == text


@pytest.mark.parametrize("logn,klen", [(9, 897), (10, 1793)])
def test_falcon_verify_bytes_refusals(logn, klen):
    lengths = "public keys must be %d bytes and signatures of one common length" % klen
    for args, text in ((([key(logn, 1)], [], [b"m"]), "batch mismatch"),
                       (([key(logn, 1)], [sig(logn, 2)], []), "batch mismatch"),
                       (([key(logn, 1)[:-1]], [sig(logn, 2)], [b"m"]), lengths),
                       (([key(logn, 1), key(logn, 3)], [sig(logn, 2), sig(logn, 4) + b"\0"], [b"m", b"n"]), lengths)):
        with pytest.raises(ValueError) as e:
            E._falcon_verify_bytes(logn, *args)
        assert str(e.value) == text


def test_ptr_of_an_address_and_of_a_tensor():
    import torch
    assert E._ptr(0x1234_5678_9ABC).value == 0x1234_5678_9ABC
    t = torch.arange(8, dtype=torch.int64)
    assert E._ptr(t).value == t.data_ptr() != 0
    assert E._ptr(t[3:]).value == t.data_ptr() + 24


def test_a_verifying_key_of_a_wrong_length_is_an_frw_error():
    # Before the binding got its one pointer rule and one refusal path this raised TypeError: FrwError was given one argument of
    # the two it needs.  It is the one case of this file that the earlier engine.py does not pass.
    with pytest.raises(frw.FrwError) as e:
        frw.Groth16Verifier(np.zeros(95, dtype=np.uint64))
    assert "verifying key: expected 84 + 12 x num_instance uint64 values" in str(e.value)
    with pytest.raises(frw.FrwError):
        frw.vk_to_wire(np.zeros(95, dtype=np.uint64))
