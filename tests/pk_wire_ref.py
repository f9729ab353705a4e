"""ark-groth16 0.3.0's ProvingKey<Bls12_381> in ark-serialize's wire format, restated in Python integers for the tests of
frw_groth16_pk_*wire* (a helper, not a test).  Written from the format table, not from the C code: the struct derives
CanonicalSerialize, so the bytes are its fields in order,

    vk            alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | le64(I) | gamma_abc_g1[I]        (wire_ref.vk_encode)
    beta_g1       G1
    delta_g1      G1
    a_query       le64(len) | G1[len]        len = I + W
    b_g1_query    le64(len) | G1[len]        len = I + W
    b_g2_query    le64(len) | G2[len]        len = I + W
    h_query       le64(len) | G1[len]        len = n - 1
    l_query       le64(len) | G1[len]        len = W

with the points as tests/wire_ref.py encodes them ((x, y) tuples of Python integers, None = infinity).  Unpinned against the crate,
like wire_ref.py itself."""
import wire_ref as W

QUERIES = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")


def _le64(v):
    return int(v).to_bytes(8, "little")


def pk_encode(key, compressed=True, length_fields=None):
    """key: {"vk": the dict wire_ref.vk_encode takes, "beta_g1", "delta_g1": G1 points, and the five queries as lists of points}.
    The length fields are the lists' own lengths (a key whose lists disagree is encoded as it stands: the framing tests want such bytes)
    unless length_fields names another value for a query."""
    out = W.vk_encode(key["vk"], compressed)
    out += W.g1_encode(key["beta_g1"], compressed) + W.g1_encode(key["delta_g1"], compressed)
    for name in QUERIES:
        enc = W.g2_encode if name == "b_g2_query" else W.g1_encode
        out += _le64((length_fields or {}).get(name, len(key[name])))
        out += b"".join(enc(p, compressed) for p in key[name])
    return out


def pk_bytes(num_instance, num_witness, domain_size, compressed=True):
    """the size the counts imply"""
    g1, g2 = W.g1_len(compressed), W.g2_len(compressed)
    nv = num_instance + num_witness
    vk = g1 + 3 * g2 + 8 + num_instance * g1
    return vk + 2 * g1 + 5 * 8 + (2 * nv + (domain_size - 1) + num_witness) * g1 + nv * g2


def pk_offsets(key, compressed=True):
    """byte offset of the first point of each query (after its length field), by the queries' own lengths"""
    g1, g2 = W.g1_len(compressed), W.g2_len(compressed)
    pos = g1 + 3 * g2 + 8 + len(key["vk"]["gamma_abc_g1"]) * g1 + 2 * g1
    offs = {}
    for name in QUERIES:
        pos += 8
        offs[name] = pos
        pos += len(key[name]) * (g2 if name == "b_g2_query" else g1)
    return offs
