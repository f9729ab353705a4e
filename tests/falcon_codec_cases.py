"""The case catalogue of the Falcon codec tests: encoded signatures, public keys and hash inputs with what oracle/falcon_codec.py alone says
about each.  Shared by tests/test_falcon_codec_cases.py (the catalogue held to its own conditions, no device), tests/test_codec_host.py
(the host build of falcon-r1cs_amd/csrc/frw_codec.h) and tests/test_gpu_codec.py (the kernels), built once from fixed seeds and cached.
No GPU, no product import.

A signature is built bit by bit -- a list of bits per coefficient, packed into header | nonce | body of a chosen sig_len -- because
falcon_codec.comp_encode cannot emit a malformed stream.  Every case carries the oracle's verdict (`want`: None, or (nonce, coefficients)
for a signature, the coefficients for a key); a refused case also names the rule it was built to break (RULES) and carries a repaired
twin that undoes that one defect and that the oracle accepts, so it is refused for the intended reason and no other.

`diagnose` is a second, fast decoder that also says WHICH rule refuses a stream.  It only steers the search for mutants; every verdict
in the catalogue is comp_decode's, and tests/test_falcon_codec_cases.py holds diagnose to comp_decode on every case."""
import hashlib
import random
import time
from collections import Counter

import frw_testlib as T
from oracle import falcon_codec as FC

Q = FC.Q
NONCE_LEN = FC.NONCE_LEN
HEAD = 1 + NONCE_LEN
SIG_LEN, PK_LEN = FC.SIG_LEN, FC.PK_LEN
LOGNS = (9, 10)
RATE_WORDS = 68                                    # 16-bit words per SHAKE256 squeeze block
# the refusal rules of the signature decoder, in the order it meets them
RULES = ("header", "minus_zero", "high_2048", "ends_in_fixed_bits", "ends_in_unary", "unused_bits", "padding")
KEY_RULES = ("header", "coeff_not_reduced")
MUTANT_KINDS = ("bit", "tail_bit", "two_bits", "byte")
FLOOR_CHANGED, FLOOR_REFUSED, FLOOR_PER_RULE = 150, 150, 5


# ---- the bit-level builder ---------------------------------------------------------------------------------------------------------------
def raw_bits(sign, low, zeros, terminate=True):
    """one coefficient as the decoder reads it: the sign bit, seven low bits, `zeros` unary zeros, the terminating 1"""
    return [sign] + [(low >> i) & 1 for i in range(6, -1, -1)] + [0] * zeros + ([1] if terminate else [])


def coeff_bits(x):
    return raw_bits(1 if x < 0 else 0, abs(x) & 127, abs(x) >> 7)


def starts_of(coeffs):
    """the bit offset of every coefficient in the body, and the number of bits used"""
    out, at = [], 0
    for c in coeffs:
        out.append(at)
        at += len(c)
    return out, at


def pack(logn, nonce, coeffs, sig_len=None, header=None, cut=False):
    """header | nonce | the coefficients' bits, zero bits up to sig_len (the shortest that holds them for None); cut: a sig_len that
    ends the stream early is meant"""
    bits = [b for c in coeffs for b in c]
    if sig_len is None:
        sig_len = HEAD + (len(bits) + 7) // 8
    room = 8 * (sig_len - HEAD)
    assert room >= 0 and (cut or len(bits) <= room), "the stream does not fit sig_len"
    bits = (bits + [0] * room)[:room]
    body = int("".join(map(str, bits)), 2).to_bytes(room // 8, "big") if room else b""
    return bytes([0x30 + logn if header is None else header]) + bytes(nonce) + body


def diagnose(data, logn):
    """(None, coefficients mod q) or (the rule that refuses the stream, None): Falcon spec Alg. 18 with the codec's strictness rules,
    written apart from comp_decode (a bit string and str.find where that walks bit by bit)"""
    n = 1 << logn
    if len(data) < HEAD or data[0] != 0x30 + logn:
        return "header", None
    body = data[HEAD:]
    total = 8 * len(body)
    s = bin(int.from_bytes(b"\x01" + body, "big"))[3:]
    pos, out = 0, []
    for _ in range(n):
        if pos + 8 > total:
            return "ends_in_fixed_bits", None
        sign, m = s[pos] == "1", int(s[pos + 1:pos + 8], 2)
        pos += 8
        one = s.find("1", pos)
        run = (one if one >= 0 else total) - pos
        if run >= 16:
            return "high_2048", None
        if one < 0:
            return "ends_in_unary", None
        m += 128 * run
        pos = one + 1
        if sign and m == 0:
            return "minus_zero", None
        out.append(Q - m if sign else m)
    one = s.find("1", pos)
    if one >= 0:
        return ("unused_bits" if one < (pos + 7) // 8 * 8 else "padding"), None
    return None, out


# ---- signatures --------------------------------------------------------------------------------------------------------------------------
class SigCase:
    """kind: "well" (built from `built`, signed coefficients), "refused" (rule, twin) or "mutant" (of `parent`, by `how`)"""

    def __init__(self, name, logn, data, kind, built=None, rule=None, twin=None, parent=None, how=None):
        self.name, self.logn, self.data, self.kind = name, logn, bytes(data), kind
        self.built, self.rule, self.twin, self.parent, self.how = built, rule, twin, parent, how
        self.want = FC.comp_decode(self.data, logn)

    sig_len = property(lambda self: len(self.data))
    accepted = property(lambda self: self.want is not None)
    on_device = property(lambda self: len(self.data) > HEAD)        # the entry points refuse sig_len <= 41 as an argument


def gauss(rng, logn, scale=1.0):
    s = T.SIGMA[logn] * scale
    return [max(-2047, min(2047, round(rng.gauss(0, s)))) for _ in range(1 << logn)]


def gauss_fit(rng, logn, slack_bits, scale=1.0):
    """a Gaussian vector whose stream leaves at least slack_bits of the standard length unused"""
    while True:
        x = gauss(rng, logn, scale)
        if sum(9 + (abs(v) >> 7) for v in x) + slack_bits <= 8 * (SIG_LEN[logn] - HEAD):
            return x


def tail_mod(x, mod8):
    """x with its last coefficient's high part chosen so that the stream's bit count is mod8 modulo 8"""
    x = list(x)
    x[-1] = (abs(x[-1]) & 127) * (-1 if x[-1] < 0 else 1)
    used = sum(9 + (abs(v) >> 7) for v in x)
    add = (mod8 - used) % 8
    x[-1] = (abs(x[-1]) + 128 * add) * (-1 if x[-1] < 0 else 1) if x[-1] else 128 * add
    return x


def _nonce(rng):
    return bytes(rng.randrange(256) for _ in range(NONCE_LEN))


def _set_bit(data, bit, value=None):
    """data with body bit `bit` (0 = the first bit of the body) flipped, or set to value"""
    b = bytearray(data)
    mask = 0x80 >> (bit & 7)
    i = HEAD + (bit >> 3)
    b[i] = b[i] ^ mask if value is None else (b[i] | mask if value else b[i] & ~mask)
    return bytes(b)


def well_formed(logn):
    rng = random.Random(9100 + logn)
    n, std = 1 << logn, SIG_LEN[logn]
    out = []

    def add(name, x, sig_len=None):
        c = SigCase(name, logn, pack(logn, _nonce(rng), [coeff_bits(v) for v in x], sig_len), "well", built=list(x))
        c.starts = starts_of([coeff_bits(v) for v in x])[0]
        out.append(c)
        return c

    add("zeros-exact", [0] * n)                                                   # 9 bits each: every bit phase, no padding (9 N / 8 bytes)
    add("zeros-std", [0] * n, std)
    add("plus-minus-one", [1 if i % 2 == 0 else -1 for i in range(n)], std)
    add("all-plus-2047", [2047] * n)                                              # 24 bits each: sig_len = 41 + 3 N
    add("all-minus-2047", [-2047] * n)
    assert out[-1].sig_len == HEAD + 3 * n
    cyc = []
    for i in range(n):                                                            # unary lengths 0 .. 15 cycling, mixed signs, no "-0"
        m = 128 * (i % 16) + rng.randrange(128)
        cyc.append(-m if rng.randrange(2) and m else m)
    add("unary-cycle", cyc)
    for k in range(6):
        add("gauss-std-%d" % k, gauss_fit(rng, logn, 0), std)
    for k in range(2):                                                            # a narrower Gaussian with zeros and |x| >= 1920 planted
        x = gauss_fit(rng, logn, 200, 0.6)
        for j, pos in enumerate(rng.sample(range(n), 12)):
            x[pos] = 0 if j < 6 else (1920 + rng.randrange(128)) * (1 if j % 2 else -1)
        add("spiked-std-%d" % k, x, std)
    for k in range(6):                                                            # a body that fills the standard length but for k bits
        x = gauss_fit(rng, logn, 0)
        spare = 8 * (std - HEAD) - sum(9 + (abs(v) >> 7) for v in x) - k
        for pos in rng.sample(range(n), spare):                                   # one more unary zero each
            x[pos] += 128 if x[pos] >= 0 else -128
        add("tight-std-%d" % k, x, std)
    add("exact-end", tail_mod(gauss(rng, logn), 0))                               # the body ends on the last byte of sig_len
    for unused in range(1, 8):
        add("unused-%d-no-padding" % unused, tail_mod(gauss(rng, logn), 8 - unused))
    for k in range(17):                                                           # an odd sig_len: signature s starts at every residue mod 16
        add("gauss-odd-%d" % k, gauss_fit(rng, logn, 0), std + 1)
    return out


POSITIONS = lambda n: (0, 1, n // 2, n - 1)


def refused(logn):
    rng = random.Random(9200 + logn)
    n, std = 1 << logn, SIG_LEN[logn]
    out = []

    def add(name, rule, data, twin):
        out.append(SigCase(name, logn, data, "refused", rule=rule, twin=bytes(twin)))

    def base(slack=40):
        return [coeff_bits(v) for v in gauss_fit(rng, logn, slack)], _nonce(rng)

    for k in POSITIONS(n):
        c, nonce = base()
        low = rng.randrange(1, 128)
        for name, rule, bad, good in (("minus-zero", "minus_zero", raw_bits(1, 0, 0), raw_bits(0, 0, 0)),
                                      ("high-2048-plus", "high_2048", raw_bits(0, low, 16), raw_bits(0, low, 15)),
                                      ("high-2048-minus", "high_2048", raw_bits(1, low, 16), raw_bits(1, low, 15)),
                                      # |x| = 2048 exactly: the low bits are zero, so the sixteenth zero alone makes it too large
                                      ("exactly-2048-plus", "high_2048", raw_bits(0, 0, 16), raw_bits(0, 0, 15)),
                                      ("exactly-2048-minus", "high_2048", raw_bits(1, 0, 16), raw_bits(1, 0, 15))):
            add("%s@%d" % (name, k), rule, pack(logn, nonce, c[:k] + [bad] + c[k + 1:], std), pack(logn, nonce, c[:k] + [good] + c[k + 1:], std))
    # sig_len cut: the stream ends inside the eight fixed bits of coefficient k (k = 0: no body at all), inside its unary run, and
    # just before the last coefficient's terminating 1.  The twin is the whole stream.
    for k in POSITIONS(n):
        c, nonce = base()
        st, used = starts_of(c)
        if k and st[k] % 8 == 0:                                                   # no byte boundary strictly inside: one more unary zero in front
            c[k - 1] = c[k - 1][:-1] + [0, 1]
            st, used = starts_of(c)
        cut = (st[k] + 7) // 8
        assert k == 0 or st[k] < 8 * cut < st[k] + 8
        add("cut-in-fixed-bits@%d" % k, "ends_in_fixed_bits", pack(logn, nonce, c, HEAD + cut, cut=True), pack(logn, nonce, c))
        c, nonce = base()
        c[k] = raw_bits(rng.randrange(2), rng.randrange(128), 9)
        st, used = starts_of(c)
        cut = (st[k] + 8 + 7) // 8
        assert st[k] + 8 <= 8 * cut <= st[k] + 8 + 9
        add("cut-in-unary@%d" % k, "ends_in_unary", pack(logn, nonce, c, HEAD + cut, cut=True), pack(logn, nonce, c))
    c, nonce = base()
    st, used = starts_of(c)
    c[n - 1] = raw_bits(0, rng.randrange(128), (-(st[n - 1] + 8)) % 8)
    st, used = starts_of(c)
    assert (used - 1) % 8 == 0
    add("cut-before-last-terminator", "ends_in_unary", pack(logn, nonce, c, HEAD + (used - 1) // 8, cut=True), pack(logn, nonce, c))
    # each single unused bit of the last used byte: seven of them at the standard length (padding behind), and the first and the last
    # unused bit of bodies that end without a padding byte
    x = tail_mod(gauss_fit(rng, logn, 40), 1)
    c, nonce = [coeff_bits(v) for v in x], _nonce(rng)
    used = starts_of(c)[1]
    good = pack(logn, nonce, c, std)
    for j in range(7):
        add("unused-bit-%d-of-7" % j, "unused_bits", _set_bit(good, used + j, 1), good)
    for unused in range(1, 8):
        c, nonce = [coeff_bits(v) for v in tail_mod(gauss(rng, logn), 8 - unused)], _nonce(rng)
        used = starts_of(c)[1]
        good = pack(logn, nonce, c)
        assert 8 * (len(good) - HEAD) - used == unused
        for j in sorted({0, unused - 1}):
            add("unused-bit-%d-of-%d-no-padding" % (j, unused), "unused_bits", _set_bit(good, used + j, 1), good)
    # a non-zero padding byte: the first, a middle one, the last byte of sig_len
    c, nonce = base(40)
    good = pack(logn, nonce, c, std)
    first = HEAD + (starts_of(c)[1] + 7) // 8
    assert std - first >= 3
    for where, at in (("first", first), ("middle", (first + std - 1) // 2), ("last", std - 1)):
        for value in (0x01, 0x80):
            bad = bytearray(good)
            bad[at] = value
            add("padding-%s-%02x" % (where, value), "padding", bad, good)
    # N - 1 coefficients, then zeros only: the N-th coefficient runs into the padding
    c, nonce = base(40)
    c = c[:n - 1]
    if starts_of(c)[1] % 8 == 0:
        c[-1] = c[-1][:-1] + [0, 1]
    used = starts_of(c)[1]
    full = HEAD + (used + 7) // 8
    twin = pack(logn, nonce, c + [raw_bits(0, 0, 0)], full + 3)
    assert 8 * (std - HEAD) - used >= 24
    add("one-short-standard", "high_2048", pack(logn, nonce, c, std), pack(logn, nonce, c + [raw_bits(0, 0, 0)], std))
    add("one-short-3-padding", "high_2048", pack(logn, nonce, c, full + 3), twin)
    add("one-short-2-padding", "ends_in_unary", pack(logn, nonce, c, full + 2), twin)
    add("one-short-0-padding", "ends_in_fixed_bits", pack(logn, nonce, c, full), twin)
    c, nonce = base(0)
    good = pack(logn, nonce, c, std)
    for h in (0x30 + (19 - logn), logn, 0x30, 0xFF):
        add("header-%02x" % h, "header", bytes([h]) + good[1:], good)
    return out


def mutants(logn, parents):
    """Mutants of the well-formed standard-length signatures, the kinds mixed until the floors hold: FLOOR_CHANGED accepted with other
    coefficients than the parent's, FLOOR_REFUSED refused, every rule hit FLOOR_PER_RULE times.  Flips aimed at what a uniform flip
    rarely finds come first: a header bit, the sign of a zero coefficient, the terminating 1 behind fifteen unary zeros."""
    rng = random.Random(9300 + logn)
    out, seen, rules = [], set(), Counter()
    changed = refused_n = 0
    std = SIG_LEN[logn]

    def consider(parent, how, data):
        nonlocal changed, refused_n
        if data in seen or data == parent.data:
            return
        rule, coeffs = diagnose(data, logn)
        if rule is None:
            if changed >= FLOOR_CHANGED + 30:
                return
        elif refused_n >= FLOOR_REFUSED + 30 and rules[rule] >= FLOOR_PER_RULE + 3:
            return
        seen.add(data)
        c = SigCase("mutant-%d-of-%s" % (len(out), parent.name), logn, data, "mutant", rule=rule, twin=parent.data, parent=parent, how=how)
        out.append(c)
        if rule is None:
            changed += coeffs != parent.want[1]
        else:
            refused_n += 1
            rules[rule] += 1

    for i, p in enumerate(parents):
        consider(p, ("bit", -1), bytes([p.data[0] ^ (1 << (i % 8))]) + p.data[1:])
        consider(p, ("bit", -1), _set_bit(p.data, 8 * (rng.randrange(1, HEAD) - HEAD) + rng.randrange(8)))      # a nonce bit: accepted, same coefficients
        last = p.starts[-1] + 8 + (abs(p.built[-1]) >> 7)                            # the last terminating 1: the run goes on into the padding
        consider(p, ("tail_bit", last), _set_bit(p.data, last))
        for k, x in enumerate(p.built):
            if x == 0:
                consider(p, ("bit", p.starts[k]), _set_bit(p.data, p.starts[k]))
            if abs(x) >> 7 == 15:
                consider(p, ("bit", p.starts[k] + 23), _set_bit(p.data, p.starts[k] + 23))
    done = lambda: changed >= FLOOR_CHANGED and refused_n >= FLOOR_REFUSED and all(rules[r] >= FLOOR_PER_RULE for r in RULES)
    tries = 0
    while not done() and tries < 6000:
        p = parents[tries % len(parents)]
        kind = MUTANT_KINDS[(tries // len(parents)) % len(MUTANT_KINDS)]
        tries += 1
        used = p.starts[-1] + 9 + (abs(p.built[-1]) >> 7)
        room = 8 * (std - HEAD)
        if kind == "bit":
            data = _set_bit(p.data, rng.randrange(room))
        elif kind == "tail_bit":                                                  # the last 30 used bytes and the padding
            data = _set_bit(p.data, rng.randrange(max(0, (used + 7) // 8 * 8 - 240), room))
        elif kind == "two_bits":
            a = rng.randrange(room)
            data = _set_bit(_set_bit(p.data, a), rng.choice([b for b in (a + rng.randrange(1, 40), rng.randrange(room)) if b < room and b != a] or [0]))
        else:
            b = bytearray(p.data)
            b[rng.randrange(HEAD, std)] = rng.choice((0x00, 0xFF))
            data = bytes(b)
        consider(p, (kind, tries), data)
    return out


# ---- public keys ---------------------------------------------------------------------------------------------------------------------------
class KeyCase:
    def __init__(self, name, logn, data, built=None, rule=None, twin=None):
        self.name, self.logn, self.data, self.built, self.rule, self.twin = name, logn, bytes(data), built, rule, twin
        self.want = FC.modq_decode(self.data, logn)

    accepted = property(lambda self: self.want is not None)


def encode_key(coeffs, logn, header=None):
    """modq_encode without its range check: 14 bits per coefficient, whatever they hold"""
    acc = 0
    for c in coeffs:
        assert 0 <= c < 1 << 14
        acc = (acc << 14) | c
    return bytes([logn if header is None else header]) + acc.to_bytes(14 * len(coeffs) // 8, "big")


def keys(logn):
    rng = random.Random(9400 + logn)
    n = 1 << logn
    out = []
    rand = lambda: [rng.randrange(Q) for _ in range(n)]
    out.append(KeyCase("zeros", logn, encode_key([0] * n, logn), built=[0] * n))
    out.append(KeyCase("all-q-minus-1", logn, encode_key([Q - 1] * n, logn), built=[Q - 1] * n))
    for k in range(36):
        x = rand()
        out.append(KeyCase("random-%d" % k, logn, encode_key(x, logn), built=x))
    x = rand()
    good = encode_key(x, logn)
    for k in (0, 1, 2, 3, n // 2, n // 2 + 1, n - 4, n - 3, n - 2, n - 1):      # all four bit alignments (14 k mod 8), both ends
        y = list(x)
        y[k] = Q - 1
        out.append(KeyCase("q-minus-1@%d" % k, logn, encode_key(y, logn), built=y))
        for name, v in (("q", Q), ("3fff", 0x3FFF)):
            z = list(x)
            z[k] = v
            out.append(KeyCase("%s@%d" % (name, k), logn, encode_key(z, logn), rule="coeff_not_reduced", twin=encode_key(y, logn)))
    out.append(KeyCase("header-own", logn, good, built=x))
    for h in (19 - logn, 0x30 + logn, 0x80 | logn):
        out.append(KeyCase("header-%02x" % h, logn, bytes([h]) + good[1:], rule="header", twin=good))
    return out


# ---- hash inputs ---------------------------------------------------------------------------------------------------------------------------
def squeeze(nonce, msg, logn):
    """(the coefficients, the 16-bit words read to find them): HashToPoint with the place it stopped"""
    n = 1 << logn
    stream = hashlib.shake_256(bytes(nonce) + bytes(msg)).digest(2 * RATE_WORDS * (3 << (logn - 5)))
    out = []
    for i in range(0, len(stream), 2):
        w = stream[i] << 8 | stream[i + 1]
        if w < 5 * Q:
            out.append(w % Q)
            if len(out) == n:
                return out, i // 2 + 1
    raise AssertionError("SHAKE256 stream too short")


def words_read(nonce, msg, count):
    stream = hashlib.shake_256(bytes(nonce) + bytes(msg)).digest(2 * count)
    return [stream[i] << 8 | stream[i + 1] for i in range(0, 2 * count, 2)]


class HashCase:
    def __init__(self, name, logn, nonce, msg):
        self.name, self.logn, self.nonce, self.msg = name, logn, bytes(nonce), bytes(msg)
        self.want = FC.hash_to_point(self.nonce, self.msg, logn)
        self.words = squeeze(self.nonce, self.msg, logn)[1]
        self.blocks = (self.words + RATE_WORDS - 1) // RATE_WORDS
        self.edges = {w for w in words_read(self.nonce, self.msg, self.words) if w in (5 * Q - 1, 5 * Q)}     # the last word accepted, the first not


def hashes(logn):
    """In batch order: the empty messages sit between non-empty ones (a message's bytes start where the previous one's end)."""
    rng = random.Random(9500 + logn)
    nonce = _nonce(rng)
    blob = bytes(rng.randrange(256) for _ in range(65539))
    out = [HashCase("len-%d" % k, logn, nonce, blob[:k]) for k in range(1, 301)]               # nonce || msg crosses 136 and 272 bytes
    out.insert(0, HashCase("len-0", logn, nonce, b""))
    for at in (150, 151, 200):                                                                  # two empties side by side, one alone
        out.insert(at, HashCase("empty-between@%d" % at, logn, _nonce(rng), b""))
    for k in (1000, 5000, 65539):
        out.append(HashCase("len-%d" % k, logn, _nonce(rng), blob[:k]))
    out.append(HashCase("empty-last", logn, _nonce(rng), b""))
    # the N-th accepted word as the last word of a squeeze block (no further permutation is needed) and as the first of a fresh one
    zero = bytes(NONCE_LEN)
    found = {}
    for k in range(500):
        msg = k.to_bytes(4, "little")
        where = squeeze(zero, msg, logn)[1] % RATE_WORDS
        if where in (0, 1) and where not in found:
            found[where] = HashCase("ends-on-%s-word-k%d" % ("last" if where == 0 else "first", k), logn, zero, msg)
    assert set(found) == {0, 1}, "the counter search found %s" % sorted(found)
    out += [found[0], found[1]]
    return out


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------------
class Catalogue:
    def __init__(self):
        t0 = time.time()
        self.well = {g: well_formed(g) for g in LOGNS}
        self.refused = {g: refused(g) for g in LOGNS}
        self.parents = {g: [c for c in self.well[g] if c.sig_len == SIG_LEN[g] and c.name.startswith(("gauss-std", "spiked-std", "tight-std"))] for g in LOGNS}
        self.mutants = {g: mutants(g, self.parents[g]) for g in LOGNS}
        self.keys = {g: keys(g) for g in LOGNS}
        self.hashes = {g: hashes(g) for g in LOGNS}
        self.build_seconds = time.time() - t0

    def signatures(self, logn):
        return self.well[logn] + self.refused[logn] + self.mutants[logn]

    def groups(self, logn):
        """{sig_len: the signature cases of that length} -- a device call takes one sig_len for all its signatures"""
        out = {}
        for c in self.signatures(logn):
            out.setdefault(c.sig_len, []).append(c)
        return out

    def standard(self, logn):
        return self.groups(logn)[SIG_LEN[logn]]

    def sizes(self):
        return {g: {"well-formed": len(self.well[g]), "refused": len(self.refused[g]), "mutants": len(self.mutants[g]),
                    "keys": len(self.keys[g]), "hashes": len(self.hashes[g]), "sig_len groups": len(self.groups(g))} for g in LOGNS}


_CATALOGUE = []


def catalogue():
    if not _CATALOGUE:
        _CATALOGUE.append(Catalogue())
    return _CATALOGUE[0]
