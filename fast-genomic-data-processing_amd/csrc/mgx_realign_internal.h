// mgx_realign_internal.h -- what mgx_realign.hip reaches of the PairHMM and Smith-Waterman contexts (mgx_pairhmm.hip,
// mgx_smithwaterman.hip).  Internal to libmgx.so: every declaration has hidden visibility, nothing here is part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/mgx_pairhmm.h"
#include "../../include/mgx_smithwaterman.h"

#pragma GCC visibility push(hidden)
namespace mgx_internal {

// ---- PairHMM side -------------------------------------------------------------------------------------------------
// One extension object per context, owned by the context (mgx_pairhmm_destroy calls free_fn on it with the device set).
struct PairhmmExt { void* p = nullptr; void (*free_fn)(void*) = nullptr; };
struct PairhmmView { int device; unsigned flags; hipStream_t compute, d2h; PairhmmExt* ext; };
PairhmmView pairhmm_view(mgx_pairhmm_t* c);

// The stages of mgx_pairhmm_regions.  begin: validation, the cross-product batch (create_cross) and its run (mgx_pairhmm_batch_run);
// batch == nullptr afterwards when the regions hold no test case.  The pointers are the batch's device-resident arrays: sequences as
// the caller gave them, region after region; row r of `out` (global read order) starts at row_off[r] and holds row_nh[r] values.
struct RegionBatch {
    mgx_pairhmm_batch_t* batch = nullptr;
    std::vector<uint64_t> base;          // every region's first test case in the batch
    uint64_t n_pairs = 0;
    uint32_t n_reads = 0;
    const uint8_t *d_bases = nullptr, *d_hap = nullptr, *d_keep = nullptr;
    const double* d_out = nullptr;
    const uint32_t *d_row_off = nullptr, *d_row_nh = nullptr;
    hipEvent_t done = nullptr;           // behind the epilogue on the compute stream
};
int regions_begin(mgx_pairhmm_t* c, uint32_t n_regions, const mgx_pairhmm_input_t* regions, const uint8_t* const* mapq,
                  const mgx_read_model_t* model, double* const* out_log10, RegionBatch* rb);
// values and keep flags into the batch's pinned mirror, one copy queued on `s` behind the batch's last kernel
int regions_queue_download(mgx_pairhmm_t* c, const RegionBatch& rb, hipStream_t s);
// ... and, once that copy has completed, out of the mirror into the caller's arrays
void regions_scatter(const RegionBatch& rb, const mgx_pairhmm_input_t* regions, uint32_t n_regions, double* const* out_log10,
                     uint8_t* const* out_keep);
void regions_end(mgx_pairhmm_t* c, RegionBatch* rb);

// pairhmm_best_allele_rows (pairhmm_kernels.hip.inc) on stream s; pri_off == nullptr: priorities are indexed like the values
void launch_best_allele_rows(hipStream_t s, const double* d_values, const uint32_t* d_row_off, const uint32_t* d_row_nh,
                             const double* d_priority, const uint32_t* d_pri_off, uint32_t n_rows, int32_t* d_best);

// ---- Smith-Waterman side ------------------------------------------------------------------------------------------
// mgx_sw_align_batch with the sequences already in device memory: in->ref and in->alt are ignored, and per chunk of pairs [lo, hi)
// the context's stream waits for `ready` and `gather` is called in place of the upload; it queues on stream s whatever writes the
// chunk's references to d_ref and its alternates to d_alt, densely and in pair order (pair p of the chunk at in->ref_off[p] -
// in->ref_off[lo], likewise alt).  Everything behind that is mgx_sw_align_batch's.
struct SwDeviceSource {
    hipEvent_t ready;
    int (*gather)(void* user, hipStream_t s, uint64_t lo, uint64_t hi, uint8_t* d_ref, uint8_t* d_alt);
    void* user;
};
// The aligner's CIGAR of every pair in binary beside its text: pair p's elements, BAM-encoded (length << 4 | M I D S = 0 1 2 4) and
// in text order, are el[off[p] .. off[p] + n[p]); exactly the elements the text holds (one the text has no room for is absent here
// too; without a text buffer the capacity is the reference's 2 * max(lengths)).  nullptr: the aligner behaves as without it.
struct SwElementSink { std::vector<uint64_t> off; std::vector<uint32_t> n, el; };
int sw_align_from_device(mgx_sw_t* c, const mgx_sw_params_t* params, const mgx_sw_input_t* in, const SwDeviceSource& src,
                         int32_t* out_offset, char* out_cigar, uint32_t cigar_stride, int32_t* out_score, SwElementSink* sink = nullptr);
struct SwView { int device; int max_ref, max_alt; };
SwView sw_view(mgx_sw_t* c);

}  // namespace mgx_internal
#pragma GCC visibility pop
