// mgx_bgzf_ctx.h -- the BGZF context (include/mgx_bgzf.h) as its translation units see it: the compressor
// (mgx_bgzf.hip), the record store (mgx_store.hip), the inflater (mgx_bgzf_inflate.hip), BAM input (mgx_bam.hip) and SAM
// text input (mgx_sam.hip) share its device and streams, and BAM input reads an inflate batch's output where the inflate
// kernel left it.  What the record store reaches of the compressor's batches is in mgx_bgzf_internal.h.
#pragma once
#include <cstdint>
#include <mutex>

#include "mgx_hip_util.h"

struct mgx_bgzf {
    mgx_hip::Owner own;                        // of the streams and the compressor's device state; the first member: the streams go last
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr;              // all batches of a context run in order on one stream
    hipStream_t copy = nullptr;                // packed blocks travel back on a stream of their own, behind their batch's kernels only
    hipStream_t up = nullptr;                  // ... and a batch's input travels up on a third one, under the kernels of the batch before
    std::mutex prep_mu; bool prepared = false; // the compressor's scratch and kernel attributes: set up at first use (or mgx_bgzf_prepare)
    uint32_t* d_scratch = nullptr; uint32_t grid = 0;
    uint32_t* d_n_stored = nullptr;
    unsigned long long* d_prof = nullptr;
    uint32_t lazy = 1, cost_base = 10, cost_rle = 6;
    uint64_t n_blocks = 0, bytes_in = 0, bytes_out = 0;
    float ms_kernels = 0, ms_pack = 0;
    // inflate (mgx_bgzf_inflate.hip)
    std::mutex inf_mu;
    uint64_t inf_blocks = 0, inf_bytes_in = 0, inf_bytes_out = 0;
    float inf_ms_kernel = 0;
    // BAM input (mgx_bam.hip): the last batch waited for
    std::mutex bam_mu;
    uint64_t bam_tiles = 0, bam_rewalked = 0, bam_redo = 0;
    uint32_t bam_rounds = 0;
    float bam_ms_index = 0, bam_ms_keys = 0;
    // SAM text input (mgx_sam.hip): the last batch waited for
    std::mutex sam_mu;
    uint64_t sam_lines = 0, sam_declined = 0, sam_bytes_in = 0, sam_bytes_out = 0, sam_tiles = 0;
    float sam_ms_lines = 0, sam_ms_encode = 0, sam_ms_keys = 0;
};

struct mgx_bgzf_inflate {
    uint64_t in_cap = 0, out_cap = 0; uint32_t max_blocks = 0;
    mgx_hip::Owner own;                        // of every buffer and event below
    uint8_t* h_in = nullptr; uint64_t* h_off = nullptr; uint8_t* h_out = nullptr; uint32_t* h_status = nullptr;      // pinned
    uint8_t* d_in = nullptr; uint64_t* d_off = nullptr; uint8_t* d_out = nullptr; uint32_t* d_status = nullptr;
    hipEvent_t ev_in = nullptr, ev_k0 = nullptr, ev_k1 = nullptr, ev_done = nullptr;
    uint32_t n_blocks = 0; uint64_t n_in = 0, n_out = 0;
    bool submitted = false;
};
