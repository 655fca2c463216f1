// mgx_bgzf_internal.h -- what the record store (mgx_store.hip) reaches of the compressor (mgx_bgzf.hip): a batch whose
// input a kernel of the store's writes in device memory, in place of pinned input that is copied up.  Internal to
// libmgx.so: the two functions have hidden visibility, nothing here is part of the C ABI.
#pragma once
#include "../../include/mgx_bgzf.h"
#include "mgx_bgzf_ctx.h"

struct mgx_bgzf_batch {
    uint64_t in_cap = 0; uint32_t max_blocks = 0;
    mgx_hip::Owner own;                                // of every buffer and event below
    uint8_t* h_in = nullptr; uint64_t* h_off = nullptr;          // pinned, filled by the caller
    uint8_t* h_out = nullptr; uint64_t* h_out_off = nullptr;     // pinned, results
    uint8_t* d_in = nullptr; uint64_t* d_off = nullptr; uint8_t* d_slots = nullptr; uint32_t* d_sizes = nullptr; uint64_t* d_out_off = nullptr;
    uint64_t out_cap = 0;
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr, ev_p0 = nullptr, ev_out = nullptr, ev_in = nullptr;
    uint8_t* h_out_dev = nullptr;                      // the pinned output buffer as the device addresses it
    uint32_t n_blocks = 0; uint64_t n_in = 0;
    bool submitted = false;
};

#pragma GCC visibility push(hidden)
namespace mgx_internal {
// mgx_bgzf_batch_create; pinned_input == false: no h_in, the input is written to d_in on the device
int bgzf_batch_create(mgx_bgzf_t* c, uint64_t in_capacity, uint32_t max_blocks, bool pinned_input, mgx_bgzf_batch_t** out);
// mgx_bgzf_batch_submit; input_resident: d_in was filled by a kernel on the context's stream, nothing is copied up
int bgzf_batch_submit(mgx_bgzf_t* c, mgx_bgzf_batch_t* b, uint32_t n_blocks, bool input_resident);
}  // namespace mgx_internal
#pragma GCC visibility pop
