// Test-only: the workspace of frw_statement_from_bytes_dev (frw_layout.h statement_layout) as plain numbers for tests/test_statement_abi.py,
// walked from a null base, so a pointer IS its offset.
#include <hip/hip_runtime.h>
#include "frw_layout.h"

extern "C" {
// pk, hm, decode_status; returns .bytes
uint64_t t_statement(int logn, uint64_t batch, uint64_t *out)
{
    const frw::StatementBufs b = frw::statement_layout(nullptr, logn, batch);
    out[0] = (uint64_t)(uintptr_t)b.pk; out[1] = (uint64_t)(uintptr_t)b.hm; out[2] = (uint64_t)(uintptr_t)b.decode_status;
    return b.bytes;
}
}
