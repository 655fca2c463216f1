// mgx_activity_internal.h -- the context behind mgx_activity_t, shared by mgx_activity.hip (the per-locus value) and
// mgx_activity_regions.hip (band-pass profile and region cutting).  Internal to libmgx.so, HIP only.
#pragma once
#include "../../include/mgx_activity.h"
#include "mgx_hip_util.h"      // HIP_TRY, Owner, Mirror, DevArray

// what the region calls keep between calls: [weights | probabilities] up, [counts | state values] down, the regions down, and the
// device-only arrays (flags, piece ends, run heads, scan output and its partial sums) in one block
struct mgx_activity_regions_work {
    mgx_hip::Mirror up, down, out;
    mgx_hip::DevArray<uint8_t> work;
    mgx_activity_region_stats_t stats{};
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // band-pass: 0-1, run heads + cutter + compaction: 1-2
    ~mgx_activity_regions_work() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
};

struct mgx_activity {
    mgx_hip::Owner own;                                  // of the stream, the events and the tables; the first member: the stream goes last
    int device = 0;
    uint32_t max_depth = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // elements: 0-1, loci: 1-2
    double* d_tables = nullptr;                          // [digamma | log10 factorial] (max_depth + 3 each) | eps | logEps | logOneMinusEps (128 each)
    mgx_hip::DevArray<uint8_t> elem; uint64_t n_elem = 0;                     // n_elem: what the last run wrote
    mgx_hip::Mirror up, down;                                     // [ReadJob | Window | running max | elements | bases | quals | reference] up | [log-odds | depth | active | too deep] down
    mgx_activity_stats_t stats{};
    mgx_activity_regions_work regions;                   // mgx_activity_regions.hip
};

// mgx_activity.hip's two halves of a call, for the fused call of mgx_activity_regions.hip: where the per-locus arrays lie in ctx->down.dev
struct mgx_activity_loci { uint32_t n_loci; size_t o_depth, o_active, o_deep, down_bytes; };      // [log-odds | depth | active | too deep]
#pragma GCC visibility push(hidden)
int mgx_activity_launch_loci(mgx_activity* c, const mgx_activity_input_t* in, const mgx_activity_params_t* p, bool has_out_active, mgx_activity_loci* o);
int mgx_activity_collect_loci(mgx_activity* c, const mgx_activity_loci& o, const mgx_activity_params_t* p, bool all, uint8_t* out_active, double* out_log_odds,
                              uint32_t* out_depth);
#pragma GCC visibility pop
