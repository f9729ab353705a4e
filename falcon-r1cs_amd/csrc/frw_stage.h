// frw_stage.h -- what the host-buffer entry points know before they touch the device: the three circuits' sizes, and how the encoded
// inputs of the bytes paths (frw_prepare_inputs, frw_statement_from_bytes, frw_falcon_verify_from_bytes, frw_pok_prove_from_bytes; the
// mixed-length ones of frw_aggregate_*_from_bytes) are staged.  Host code only, nothing of the HIP runtime is called:
// tests/cpp/test_stage_host.cpp and tests/cpp/test_aggregate_bytes.cpp fill real memory by it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include "../../include/frw.h"
#include "frw_layout.h"       // frw::Carve

namespace frw {

inline bool known_circuit(int circuit) { return circuit == FRW_CIRCUIT_NTT || circuit == FRW_CIRCUIT_DUAL_NTT || circuit == FRW_CIRCUIT_SCHOOLBOOK; }

// The counts of one signature's constraint system (logn = 9 | 10; an unknown circuit: all zero).  The reference's own figures are held
// to these through frw_layout* (tests/test_capi.py, tests/test_schoolbook_host.py).
struct CircuitShape { size_t n, nb, num_instance, num_witness, num_constraints; };
inline CircuitShape circuit_shape(int circuit, int logn)
{
    const size_t n = (size_t)1 << logn, nb = logn == 9 ? 50 : 52;       // nb: the bits of the norm bound's comparison
    switch (circuit) {
    case FRW_CIRCUIT_NTT: return {n, nb, 2 * n + 1, 153 * n + nb, 159 * n + nb + 2};
    case FRW_CIRCUIT_DUAL_NTT: return {n, nb, 2 * n + 1, 186 * n + 4 + nb, 189 * n + 10 + nb};
    case FRW_CIRCUIT_SCHOOLBOOK: return {n, nb, 2 * n + 1, n * n + 99 * n + nb, n * n + 105 * n + nb + 2};
    default: return {0, 0, 0, 0, 0};
    }
}

// msg_off[0 .. batch] is non-decreasing, and msgs == NULL only where there is no message byte at all
inline bool message_offsets_ok(const uint8_t *msgs, const uint64_t *msg_off, size_t batch)
{
    for (size_t i = 0; i < batch; i++)
        if (msg_off[i + 1] < msg_off[i]) return false;
    return msgs || batch == 0 || msg_off[batch] == msg_off[0];
}

// The encoded inputs of a pass of `chunk` slots at most: pk bytes | signature bytes or nonces | messages | rebased offsets (| r, s), each
// piece 256-byte aligned.  The staged layout IS the device layout, which is why a pass has ONE copy in: fill() a page-locked buffer of
// `bytes`, copy `bytes` to a device base, and take the kernels' pointers from that base.
struct StagedInputs {
    const uint8_t *pk_bytes, *second, *msgs;      // second: the signatures' bytes, or the nonces
    const uint64_t *msg_off, *rs;                 // rs: 64 bytes a slot, or NULL
    size_t pk_len, second_len;
    size_t max_msg = 1;                           // the longest pass's message bytes (1 where there are none: no empty piece)
    size_t o_pk, o_second, o_msgs, o_off, o_rs, bytes;

    StagedInputs(int logn, size_t batch, size_t chunk, const uint8_t *pk_bytes_, const uint8_t *second_, size_t second_len_,
                 const uint8_t *msgs_, const uint64_t *msg_off_, const uint64_t *rs_ = nullptr)
        : pk_bytes(pk_bytes_), second(second_), msgs(msgs_), msg_off(msg_off_), rs(rs_), pk_len(FRW_PK_LEN(logn)), second_len(second_len_)
    {
        for (size_t lo = 0; lo < batch; lo += chunk) max_msg = std::max(max_msg, msg_bytes(lo, std::min(chunk, batch - lo)));
        Carve c(nullptr);
        o_pk = c.off;     c.take(chunk * pk_len);
        o_second = c.off; c.take(chunk * second_len);
        o_msgs = c.off;   c.take(max_msg);
        o_off = c.off;    c.take((chunk + 1) * sizeof(uint64_t));
        o_rs = c.off;     if (rs) c.take(chunk * 64);
        bytes = c.off;
    }
    size_t msg_bytes(size_t lo, size_t cnt) const { return (size_t)(msg_off[lo + cnt] - msg_off[lo]); }
    // slots lo .. lo + cnt - 1 into `stage`: the slices of the sources, and the offsets rebased to the pass's first message
    void fill(void *stage, size_t lo, size_t cnt) const
    {
        char *h = (char *)stage;
        memcpy(h + o_pk, pk_bytes + lo * pk_len, cnt * pk_len);
        memcpy(h + o_second, second + lo * second_len, cnt * second_len);
        if (msg_bytes(lo, cnt)) memcpy(h + o_msgs, msgs + msg_off[lo], msg_bytes(lo, cnt));
        uint64_t *off = (uint64_t *)(h + o_off);
        for (size_t i = 0; i <= cnt; i++) off[i] = msg_off[lo + i] - msg_off[lo];
        if (rs) memcpy(h + o_rs, rs + lo * 8, cnt * 64);
    }
    // the pieces of a pass copied to `base`
    const uint8_t *d_pk(const void *base) const { return (const uint8_t *)base + o_pk; }
    const uint8_t *d_second(const void *base) const { return (const uint8_t *)base + o_second; }
    const uint8_t *d_msgs(const void *base) const { return (const uint8_t *)base + o_msgs; }
    const uint64_t *d_off(const void *base) const { return (const uint64_t *)((const char *)base + o_off); }
    const uint64_t *d_rs(const void *base) const { return (const uint64_t *)((const char *)base + o_rs); }
};

// The encoded inputs of ONE aggregate (frw_aggregate_*_from_bytes): the same pieces, but the statements' keys and signatures are of two
// lengths, mixed, in statement order -- the layout the device entry points read in place, so the pieces are the caller's arrays whole
// (aggregate_pk_bytes / aggregate_sig_bytes of frw_layout.h say how long), and an aggregate is one pass: it is not divisible.  `nonces`:
// the second piece is the statements' nonces (40 bytes each), not their signatures.  rs: the proof's r and s, 64 bytes, or NULL.
struct StagedAggregate {
    const uint8_t *pk_bytes, *second, *msgs;
    const uint64_t *msg_off, *rs;
    size_t count, pk_total, second_total, msg_total;
    size_t o_pk, o_second, o_msgs, o_off, o_rs, bytes;

    StagedAggregate(size_t count9, size_t count10, bool nonces, const uint8_t *pk_bytes_, const uint8_t *second_, const uint8_t *msgs_,
                    const uint64_t *msg_off_, const uint64_t *rs_ = nullptr)
        : pk_bytes(pk_bytes_), second(second_), msgs(msgs_), msg_off(msg_off_), rs(rs_), count(count9 + count10),
          pk_total(aggregate_pk_bytes(count9, count10)),
          second_total(nonces ? (count9 + count10) * FRW_NONCE_LEN : aggregate_sig_bytes(count9, count10)),
          msg_total((size_t)(msg_off_[count9 + count10] - msg_off_[0]))
    {
        Carve c(nullptr);
        o_pk = c.off;     c.take(pk_total);
        o_second = c.off; c.take(second_total);
        o_msgs = c.off;   c.take(msg_total ? msg_total : 1);
        o_off = c.off;    c.take((count + 1) * sizeof(uint64_t));
        o_rs = c.off;     if (rs) c.take(64);
        bytes = c.off;
    }
    void fill(void *stage) const
    {
        char *h = (char *)stage;
        memcpy(h + o_pk, pk_bytes, pk_total);
        memcpy(h + o_second, second, second_total);
        if (msg_total) memcpy(h + o_msgs, msgs + msg_off[0], msg_total);
        uint64_t *off = (uint64_t *)(h + o_off);
        for (size_t i = 0; i <= count; i++) off[i] = msg_off[i] - msg_off[0];
        if (rs) memcpy(h + o_rs, rs, 64);
    }
    const uint8_t *d_pk(const void *base) const { return (const uint8_t *)base + o_pk; }
    const uint8_t *d_second(const void *base) const { return (const uint8_t *)base + o_second; }
    const uint8_t *d_msgs(const void *base) const { return (const uint8_t *)base + o_msgs; }
    const uint64_t *d_off(const void *base) const { return (const uint64_t *)((const char *)base + o_off); }
    const uint64_t *d_rs(const void *base) const { return (const uint64_t *)((const char *)base + o_rs); }
};

}  // namespace frw
