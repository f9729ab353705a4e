// frw_arena.h -- working memory of the host-buffer entry points (frw_witness_ntt_verify, frw_ntt_modq, frw_gadget,
// frw_prepare_inputs, frw_qap_witness_map): device buffers, a page-locked bounce buffer, two streams and four events that
// belong to the context (or the R1CS handle) and only ever grow.
//
// Why: the reference's consumer calls generate_constraints once per signature (examples/constraint_counts.rs:61-63,
// examples/pok_sig.rs:24-32), so the drop-in entry point is called with batch = 1 over and over.  Allocating and freeing
// five device buffers per call (hipFree synchronises the device) cost more than the 43 us the kernel takes for one
// signature; with the arena a call after the first allocates nothing (frw_diag_host_allocations counts).
//
// host_passes() below is the one loop that takes a batch through the arena in chunks; every chunked entry point is a caller of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <initializer_list>
#include <mutex>
#include "../../include/frw.h"
#include "frw_layout.h"       // frw::Carve: a slot is carved into 256-byte aligned pieces (run once with base = nullptr to size it)

namespace frw {

struct HostArena {
    static constexpr int SLOTS = 2;       // chunk k is copied out while chunk k+1 is computed
    std::mutex mu;                        // the host-buffer entry points of one owner run one at a time
    void *d_slot[SLOTS] = {nullptr, nullptr};
    size_t d_cap[SLOTS] = {0, 0};
    void *h_pin = nullptr;                // page-locked: inputs on their way in, status words on their way out
    size_t h_cap = 0;
    hipStream_t compute = nullptr, copy = nullptr;
    hipEvent_t done[SLOTS] = {nullptr, nullptr}, drained[SLOTS] = {nullptr, nullptr};
    uint64_t allocations = 0;             // hipMalloc + hipHostMalloc calls made so far

    hipError_t init()
    {
        hipError_t e = hipStreamCreateWithFlags(&compute, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking);
        for (int b = 0; b < SLOTS && e == hipSuccess; b++) {
            e = hipEventCreateWithFlags(&done[b], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&drained[b], hipEventDisableTiming);
        }
        return e;
    }
    // everything the arena holds goes back to the device; the arena stays usable (the next call allocates again)
    void trim()
    {
        for (int b = 0; b < SLOTS; b++) {
            if (d_slot[b]) (void)hipFree(d_slot[b]);
            d_slot[b] = nullptr;
            d_cap[b] = 0;
        }
        if (h_pin) (void)hipHostFree(h_pin);
        h_pin = nullptr;
        h_cap = 0;
    }
    void destroy()
    {
        trim();
        for (int b = 0; b < SLOTS; b++) {
            if (done[b]) (void)hipEventDestroy(done[b]);
            if (drained[b]) (void)hipEventDestroy(drained[b]);
            done[b] = drained[b] = nullptr;
        }
        if (compute) (void)hipStreamDestroy(compute);
        if (copy) (void)hipStreamDestroy(copy);
        compute = copy = nullptr;
    }
    hipError_t reserve_device(int slot, size_t bytes)
    {
        if (d_cap[slot] >= bytes) return hipSuccess;
        if (d_slot[slot]) (void)hipFree(d_slot[slot]);      // no call is in flight: the entry points synchronise before they return, DrainOnExit on every other way out
        d_slot[slot] = nullptr;
        d_cap[slot] = 0;
        const hipError_t e = hipMalloc(&d_slot[slot], bytes);
        if (e == hipSuccess) {
            d_cap[slot] = bytes;
            allocations++;
        }
        return e;
    }
    hipError_t reserve_pinned(size_t bytes)
    {
        if (h_cap >= bytes) return hipSuccess;
        if (h_pin) (void)hipHostFree(h_pin);
        h_pin = nullptr;
        h_cap = 0;
        const hipError_t e = hipHostMalloc(&h_pin, bytes, hipHostMallocDefault);
        if (e == hipSuccess) {
            h_cap = bytes;
            allocations++;
        }
        return e;
    }
};

// An entry point that gives up half way through its pipeline (a HIP error after the first enqueue) must not hand the caller's
// buffers back while copies into them, or kernels on the arena's slots, are still running -- the caller may free them, and the
// next call reuses the slot.  Declared right after the lock; `settled` is set once the call's own final synchronisations have
// been made, so the successful path pays nothing.
struct DrainOnExit {
    HostArena &a;
    bool settled = false;
    explicit DrainOnExit(HostArena &arena) : a(arena) {}
    ~DrainOnExit()
    {
        if (settled) return;
        if (a.compute) (void)hipStreamSynchronize(a.compute);
        if (a.copy) (void)hipStreamSynchronize(a.copy);
    }
};

int record_hip_error(hipError_t e, const char *what);      // (frw_capi.cpp: frw_last_error's text and the FRW_E_* code)

// One result of a pass on its way out: `item` bytes per slot of the batch, from the piece at `dev_off` of the device slot to `host`, the
// caller's array for the whole batch.  A null `host` (an output the caller did not ask for) is skipped.
struct PassOut { void *host; size_t dev_off, item; };

// A batch through the arena in passes of `chunk`: everything about order and lifetime, nothing about what a pass computes.
//     slots        1: every pass uses device slot 0 and the page-locked buffer, and the host waits for the pass before the next one
//                  overwrites either.  2: pass k uses slot k & 1 and that half of the page-locked buffer; its results leave on the copy
//                  stream while the compute stream already fills the other slot with pass k + 1 (a witness is 5 MB per signature over
//                  PCIe).  With output buffers from frw_host_alloc (pinned) every copy out is a true asynchronous DMA; with pageable
//                  memory the runtime stages the copies itself and the overlap degrades gracefully, the results are the same.
//     slot_bytes   the carved size of a device slot; stage_bytes: page-locked bytes of a pass (0: the pass copies in from the caller's
//                  memory itself).  Both only ever grow the arena: a call after the first of its shape allocates nothing.
//     pass(d_slot, stage, lo, cnt, stream) -> FRW_*: fill `stage`, enqueue the copy in and the kernels of slots lo .. lo + cnt - 1 on
//                  `stream`.  A code other than FRW_OK ends the call with that code.
// Every way out but the last goes through DrainOnExit; the last has made the call's own synchronisations.
template <class Pass>
int host_passes(HostArena &A, int device, size_t batch, size_t chunk, int slots, size_t slot_bytes, size_t stage_bytes,
                std::initializer_list<PassOut> outs, Pass pass)
{
    std::lock_guard<std::mutex> lock(A.mu);
    DrainOnExit drain(A);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return record_hip_error(e, "host passes: hipSetDevice");
    for (int b = 0; b < slots; b++)
        if ((e = A.reserve_device(b, slot_bytes)) != hipSuccess) return record_hip_error(e, "host passes: device memory");
    if ((e = A.reserve_pinned((size_t)slots * stage_bytes)) != hipSuccess) return record_hip_error(e, "host passes: page-locked memory");
    size_t k = 0;
    for (size_t lo = 0; lo < batch; lo += chunk, k++) {
        const size_t cnt = std::min(chunk, batch - lo);
        const int b = slots == 2 ? (int)(k & 1) : 0;
        // slot b was last used by pass k - 2: its copies out have finished before its memory is written again (the host waits too:
        // the pass is about to overwrite the page-locked inputs that pass's copy in read)
        if (slots == 2 && k >= 2 && (e = hipEventSynchronize(A.drained[b])) != hipSuccess)
            return record_hip_error(e, "host passes: waiting for a slot to drain");
        const int rc = pass((char *)A.d_slot[b], (char *)A.h_pin + (size_t)b * stage_bytes, lo, cnt, A.compute);
        if (rc != FRW_OK) return rc;
        hipStream_t out = A.compute;
        if (slots == 2) {
            if ((e = hipEventRecord(A.done[b], A.compute)) == hipSuccess) e = hipStreamWaitEvent(A.copy, A.done[b], 0);
            if (e != hipSuccess) return record_hip_error(e, "host passes: handing a pass to the copy stream");
            out = A.copy;
        }
        for (const PassOut &o : outs)
            if (o.host && (e = hipMemcpyAsync((char *)o.host + lo * o.item, (char *)A.d_slot[b] + o.dev_off, cnt * o.item,
                                              hipMemcpyDeviceToHost, out)) != hipSuccess)
                return record_hip_error(e, "host passes: copy out");
        // one slot: the staged inputs and the slot are reused by the next pass
        e = slots == 2 ? hipEventRecord(A.drained[b], A.copy) : hipStreamSynchronize(A.compute);
        if (e != hipSuccess) return record_hip_error(e, "host passes: end of a pass");
    }
    if (slots == 2) {
        if ((e = hipStreamSynchronize(A.compute)) == hipSuccess) e = hipStreamSynchronize(A.copy);
        if (e != hipSuccess) return record_hip_error(e, "host passes: final synchronisation");
    }
    drain.settled = true;
    return FRW_OK;
}

}  // namespace frw
