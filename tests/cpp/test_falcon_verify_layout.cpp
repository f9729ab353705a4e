// Test-only: the workspace of frw_falcon_verify_from_bytes_dev (frw_layout.h falcon_verify_layout) as plain numbers for
// tests/test_falcon_verify_abi.py, walked from a null base, so a pointer IS its offset.
#include <hip/hip_runtime.h>
#include "frw_layout.h"

extern "C" {
// sig, pk, hm, nonce, sig_status, pk_status; returns .bytes
uint64_t t_falcon_verify(int logn, uint64_t batch, uint64_t *out)
{
    const frw::FalconVerifyBufs b = frw::falcon_verify_layout(nullptr, logn, batch);
    out[0] = (uint64_t)(uintptr_t)b.sig; out[1] = (uint64_t)(uintptr_t)b.pk; out[2] = (uint64_t)(uintptr_t)b.hm;
    out[3] = (uint64_t)(uintptr_t)b.nonce; out[4] = (uint64_t)(uintptr_t)b.sig_status; out[5] = (uint64_t)(uintptr_t)b.pk_status;
    return b.bytes;
}
}
