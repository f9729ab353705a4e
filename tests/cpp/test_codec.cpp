// Host harness (shared library, ctypes) around the per-item functions of Falcon's encodings (falcon-r1cs_amd/csrc/frw_codec.h): one
// signature, one public key, one hash-to-point, compiled with g++ through tests/cpp/hip_host.  tests/test_codec_host.py drives the
// catalogue of tests/falcon_codec_cases.py through it against oracle/falcon_codec.py; tests/cpp/codec_sanitize_main.cpp includes this
// file and calls the same three functions on heap buffers of exactly their inputs' lengths.
#include <cstddef>
#include <cstdint>
#include "frw_codec.h"

using namespace frw::codec;

// -> 1: well formed.  out: N coefficients; nonce_out: 40 bytes or null
extern "C" int t_decode_signature(int logn, const uint8_t *p, size_t sig_len, uint16_t *out, uint8_t *nonce_out)
{
    return decode_signature_one(logn, p, sig_len, out, nonce_out) ? 1 : 0;
}

// the key at p, coefficient by coefficient as decode_public_keys_kernel's lanes take it -> 1: well formed.  out: N coefficients, all written
extern "C" int t_decode_public_key(int logn, const uint8_t *p, uint16_t *out)
{
    bool refused = false;
    for (int k = 0; k < 1 << logn; k++) {
        const uint32_t c = public_key_coeff(p, k);
        out[k] = (uint16_t)c;
        if (public_key_coeff_refused(c) || (k == 0 && public_key_header_refused(p, logn))) refused = true;
    }
    return refused ? 0 : 1;
}

// msg: the message's first byte (never read where o1 <= o0)
extern "C" void t_hash_to_point(int logn, const uint8_t *nonce, const uint8_t *msg, uint64_t o0, uint64_t o1, uint16_t *out)
{
    hash_to_point_one(logn, nonce, msg, o0, o1, out);
}
