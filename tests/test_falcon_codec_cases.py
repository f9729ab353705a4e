"""The catalogue of tests/falcon_codec_cases.py held to its own conditions by oracle/falcon_codec.py alone, where no device is involved:
the GPU tests and the host harness compare against these cases, so they must not be able to pass by having nothing to compare."""
from collections import Counter

import pytest

import falcon_codec_cases as CC
from oracle import falcon_codec as FC


@pytest.fixture(scope="module")
def cat():
    return CC.catalogue()


_DECODED = {}


def decode(data, logn):
    key = (logn, data)
    if key not in _DECODED:
        _DECODED[key] = FC.comp_decode(data, logn)
    return _DECODED[key]


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_well_formed_signatures_round_trip(cat, logn):
    n = 1 << logn
    names = {c.name for c in cat.well[logn]}
    assert {"zeros-exact", "zeros-std", "plus-minus-one", "all-plus-2047", "all-minus-2047", "unary-cycle", "exact-end"} <= names
    for c in cat.well[logn]:
        assert c.want is not None, c.name
        assert c.want[0] == c.data[1:41] and c.want[1] == [x % CC.Q for x in c.built] and len(c.built) == n, c.name
    by = {c.name: c for c in cat.well[logn]}
    assert by["all-plus-2047"].sig_len == by["all-minus-2047"].sig_len == 41 + 3 * n
    assert by["zeros-exact"].sig_len == 41 + 9 * n // 8
    cyc = by["unary-cycle"].built
    assert [abs(x) >> 7 for x in cyc[:32]] == list(range(16)) * 2 and any(x < 0 for x in cyc) and any(x > 0 for x in cyc)
    # a coefficient of 24 bits, a unary run over two byte boundaries, and bodies without padding with 0 .. 7 unused bits
    assert any(abs(x) >> 7 >= 15 for x in cyc)
    used = lambda c: sum(9 + (abs(x) >> 7) for x in c.built)
    assert 8 * (by["exact-end"].sig_len - 41) == used(by["exact-end"])
    for unused in range(1, 8):
        c = by["unused-%d-no-padding" % unused]
        assert 8 * (c.sig_len - 41) - used(c) == unused
    assert sum(c.sig_len == CC.SIG_LEN[logn] for c in cat.well[logn]) >= 8


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_refused_signatures_are_refused_for_their_rule_and_no_other(cat, logn):
    n = 1 << logn
    rules = Counter()
    for c in cat.refused[logn]:
        assert c.want is None, c.name
        assert CC.diagnose(c.data, logn) == (c.rule, None), c.name
        assert decode(c.twin, logn) is not None, "the repaired twin of %s" % c.name
        rules[c.rule] += 1
    assert set(rules) == set(CC.RULES)
    names = {c.name for c in cat.refused[logn]}
    for k in CC.POSITIONS(n):
        assert {"minus-zero@%d" % k, "high-2048-plus@%d" % k, "high-2048-minus@%d" % k, "exactly-2048-plus@%d" % k, "exactly-2048-minus@%d" % k, "cut-in-fixed-bits@%d" % k, "cut-in-unary@%d" % k} <= names
    assert {"cut-before-last-terminator", "one-short-standard", "one-short-3-padding", "one-short-2-padding", "one-short-0-padding"} <= names
    assert {"padding-%s-%02x" % (w, v) for w in ("first", "middle", "last") for v in (1, 0x80)} <= names
    assert {"header-%02x" % h for h in (0x30 + 19 - logn, logn, 0x30, 0xFF)} <= names
    assert {"unused-bit-%d-of-7" % j for j in range(7)} <= names
    # a cut case differs from its twin by its length alone
    for c in cat.refused[logn]:
        if c.name.startswith("cut-"):
            assert c.twin[:c.sig_len] == c.data and len(c.twin) > c.sig_len, c.name


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_mutant_floors(cat, logn):
    ms = cat.mutants[logn]
    assert len({m.data for m in ms}) == len(ms)
    assert all(m.sig_len == CC.SIG_LEN[logn] and m.parent.want is not None and m.data != m.parent.data for m in ms)
    changed = [m for m in ms if m.want is not None and m.want[1] != m.parent.want[1]]
    refused = [m for m in ms if m.want is None]
    assert len(changed) >= CC.FLOOR_CHANGED and len(refused) >= CC.FLOOR_REFUSED, (len(changed), len(refused))
    for m in ms:                                             # the search's decoder and the oracle agree on every mutant
        rule, coeffs = CC.diagnose(m.data, logn)
        assert (rule is None) == (m.want is not None) and rule == m.rule and (m.want is None or coeffs == m.want[1]), m.name
    hit = Counter(m.rule for m in refused)
    assert all(hit[r] >= CC.FLOOR_PER_RULE for r in CC.RULES), hit
    assert {m.how[0] for m in ms} == set(CC.MUTANT_KINDS)
    assert any(m.want is not None and m.want[1] == m.parent.want[1] and m.want[0] != m.parent.want[0] for m in ms)     # a nonce bit


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_the_search_decoder_is_the_oracle_on_every_signature(cat, logn):
    for c in cat.signatures(logn):
        rule, coeffs = CC.diagnose(c.data, logn)
        assert (None if rule else coeffs) == (c.want[1] if c.want else None), c.name


def test_signature_groups(cat):
    for logn in CC.LOGNS:
        groups = cat.groups(logn)
        assert any(L % 2 == 1 and len(g) >= 17 for L, g in groups.items()), "an odd sig_len in a batch of at least 17"
        assert len(groups[CC.SIG_LEN[logn]]) >= 257
        # every case but the one without a body can go to the device; that one is the host harness's alone
        assert [c.name for c in cat.signatures(logn) if not c.on_device] == ["cut-in-fixed-bits@0"]


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_keys(cat, logn):
    n = 1 << logn
    ks = cat.keys[logn]
    assert len(ks) >= 70
    for k in ks:
        assert len(k.data) == CC.PK_LEN[logn]
        if k.rule is None:
            assert k.want == k.built and k.data == FC.modq_encode(k.built, logn), k.name
        else:
            assert k.want is None and FC.modq_decode(k.twin, logn) is not None and k.rule in CC.KEY_RULES, k.name
            assert sum(a != b for a, b in zip(k.data, k.twin)) <= 3, k.name          # one coefficient or the header byte
    names = {k.name for k in ks}
    at = (0, 1, 2, 3, n // 2, n // 2 + 1, n - 4, n - 3, n - 2, n - 1)
    assert {14 * k % 8 for k in at} == {0, 6, 4, 2}
    assert {"%s@%d" % (v, k) for v in ("q-minus-1", "q", "3fff") for k in at} <= names
    assert {"zeros", "all-q-minus-1", "header-own", "header-%02x" % (19 - logn), "header-%02x" % (0x30 + logn), "header-%02x" % (0x80 | logn)} <= names


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_hash_inputs(cat, logn):
    hs = cat.hashes[logn]
    for h in hs:
        assert CC.squeeze(h.nonce, h.msg, logn)[0] == h.want and len(h.nonce) == 40, h.name
    lens = [len(h.msg) for h in hs]
    assert set(range(301)) | {1000, 5000, 65539} <= set(lens)
    assert len({h.nonce for h in hs if len(h.msg) <= 300 and h.name.startswith("len-")}) == 1
    assert any(lens[i] == 0 and lens[i - 1] > 0 and lens[i + 1] > 0 for i in range(1, len(hs) - 1))
    assert any(lens[i] == 0 and lens[i + 1] == 0 for i in range(len(hs) - 1)) and lens[-3] == 0
    # the N-th accepted word: the last of a squeeze block, the first of a fresh one; found by counter below 500
    last, first = hs[-2], hs[-1]
    assert last.words % CC.RATE_WORDS == 0 and first.words % CC.RATE_WORDS == 1
    assert last.nonce == first.nonce == bytes(40) and len(last.msg) == len(first.msg) == 4
    assert int.from_bytes(last.msg, "little") == {9: 6, 10: 39}[logn] and int.from_bytes(first.msg, "little") == {9: 2, 10: 3}[logn]
    assert {h.blocks for h in hs} == ({8, 9} if logn == 9 else {16, 17})
    # the acceptance bound itself: streams that hold the word 5 q - 1 (accepted, as q - 1) and the word 5 q (not accepted)
    assert set().union(*(h.edges for h in hs)) == {5 * CC.Q - 1, 5 * CC.Q}
