// pairhmm_plan.h -- the batch plan of the PairHMM library (mgx_pairhmm.hip): everything the host decides about a batch
// before it talks to the device.  Read length -> (G, RPL) class, the folding of small classes, the counting sort of the
// jobs, launch geometry and LDS bytes, where every array lies in the slab, the tables the device enumerates a
// cross-product batch from, the wire expansion's grid, the cutter of region lists and which classes share a launch.
// Plain C++17, no HIP and no environment: tests/cpp/pairhmm_plan_driver.cpp runs it on the CPU under sanitizers, and
// tests/test_pairhmm_plan_host.py checks what it prints against what the kernels index.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mgx_pairhmm.h"
#include "mgx_common.h"
#include "pairhmm_wire.h"

#pragma GCC visibility push(hidden)      // internal to libmgx.so
namespace mgx_hmm_plan {

// ---- what the host writes and the kernels (pairhmm_kernels.hip.inc) read ---------------------------------------------

struct Job {
    uint64_t read_off;
    uint64_t hap_off;
    uint32_t R;
    uint32_t H;
    uint32_t pair;
    uint32_t pad_;
};
static_assert(sizeof(Job) == 32, "Job is 32 bytes");

// Cross-product batches (every read against every haplotype of a region, the shape
// VectorLoglessPairHMM builds): job descriptors are generated on the device from two small tables
// instead of being written one by one on the host.
struct SeqRef {
    uint64_t off;
    uint32_t len;
    uint32_t id;
};

// One or several active regions (row F1) in ONE batch.  Every read is paired with the
// haplotypes of its own region; job q belongs to the read whose prefix range holds q, so neighbouring jobs
// are the same read against haplotypes of similar length.
struct RegionRef {
    uint32_t hap_begin;    // first entry of the region's (length-sorted) haplotypes in the hap table
    uint32_t n_haps;
    uint32_t read_base;    // global index of the region's first read
    uint32_t out_base;     // where the region's [reads][haps] block starts in the output
};

constexpr int kMaxCodes = 5;       // code columns of the emission table: A C T G N (pairhmm_kernels.hip.inc)
constexpr int kMultiBins = 16;     // classes one multi-class launch takes

using mgx::set_error;

// Row classes: a read of R rows is owned by G lanes with RPL = ceil(R / G) rows each.  Few rows per lane waste
// issue slots on the per-step overhead (3 DPP moves, the haplotype byte, loop control are paid per step, not per
// cell), many lanes waste steps on fill/drain (G - 1 per pair) and lanes on padding (up to G - 1 rows), so short
// reads take narrow groups: G = 4 up to 32 bases, G = 8 up to 64, G = 16 up to 192 (1..12 rows per lane: the
// common 100-151 bp reads), G = 64 with 4..16 rows per lane beyond that (up to 1024 bases).
// (Giving 8 lanes up to 16 rows each -- reads up to 128 bases -- was measured and lost: 128 x 256 test cases 6019 ->
// 5642 GCUPS, ragged 4429 -> 3835; profiles/r02_pairhmm_g8_rows.txt.)
constexpr int kNarrowMaxRPL = 8, kG8MaxRPL = 8, kG16MaxRPL = 12, kG64MinRPL = 4, kG64MaxRPL = 16;
constexpr int kMaxRowsG4 = 4 * kNarrowMaxRPL, kMaxRowsG8 = 8 * kG8MaxRPL;
constexpr int kMaxRowsG16 = 16 * kG16MaxRPL;
constexpr int kMaxRowsG64 = 64 * kG64MaxRPL;
// the five-operation cell (pairhmm_cell.h) is the first fp32 launch of the classes of up to 16 lanes: reads of at most 192 bases
constexpr int kFiveOpMaxG = 16, kFiveOpMaxRows = kMaxRowsG16;
// Longer reads are strip-mined: 64 lanes x 16 rows per strip, the strips sweep the haplotype one after the other
// (pairhmm_fwd_strip).  The limit below only keeps row indices and the boundary scratch in 32 bits.
constexpr int kMaxRowsStrip = 1 << 20;
constexpr int kStripMarkRPL = kG64MaxRPL + 1;      // shape_of's RPL value for the strip-mined class
constexpr uint32_t kMaxLdsPerBlock = 64 * 1024;
constexpr uint32_t kMaxLdsPerLaunch = 160 * 1024;
constexpr size_t kStageLimit = 256u << 20;         // inputs + results beyond this are not staged through a pinned mirror
constexpr size_t kSlabAlign = 256;                 // every array of a slab starts on a multiple of this and owns the bytes up to the next
constexpr uint64_t kMergeBelow = 4096;             // classes with fewer test cases are folded into the next one (default of the limit)
constexpr uint32_t kExpandBlock = 256;             // threads per workgroup of pairhmm_expand_wire, 8 positions each
// the last thread of an array stores its full 8 bytes, up to 7 past the array's length: they fall into the array's own
// slab slot, which align_up rounds to a multiple of 8
static_assert(kSlabAlign % 8 == 0, "pairhmm_expand_wire stores whole 8-byte groups into slab slots");

inline size_t align_up(size_t x, size_t a = kSlabAlign) { return (x + a - 1) / a * a; }

struct Bin {
    int G = 0, RPL = 0;              // fp32 kernel shape
    int Gd = 0, RPLd = 0;            // fp64 re-run kernel shape (fewer registers per row class)
    uint32_t job_begin = 0, job_count = 0;
    uint32_t max_h = 0;
    uint64_t cells = 0, alg_bytes = 0;
    // launch geometry
    uint32_t block = 256, lds_stride = 0, grid_f32 = 0, grid_f64 = 0, grid_f64_all = 0, grid_nhap = 0;
    bool strip = false;              // reads longer than 1024 bases: the strip-mined kernel, one test case per workgroup
};

// (G, RPL) class of a read of R rows; G = 0 if unsupported.  min_g = 16 switches the narrow groups off (MGX_PAIRHMM_MIN_G).
inline void shape_of(uint32_t R, int min_g, int* G, int* RPL) {
    if (R <= (uint32_t)kMaxRowsG4 && min_g <= 4) { *G = 4; *RPL = (int)((R + 3) / 4); }
    else if (R <= (uint32_t)kMaxRowsG8 && min_g <= 8) { *G = 8; *RPL = (int)((R + 7) / 8); }
    else if (R <= (uint32_t)kMaxRowsG16) { *G = 16; *RPL = (int)((R + 15) / 16); }
    else if (R <= (uint32_t)kMaxRowsG64) { *G = 64; *RPL = std::max(kG64MinRPL, (int)((R + 63) / 64)); }
    else if (R <= (uint32_t)kMaxRowsStrip) { *G = 64; *RPL = kStripMarkRPL; }
    else { *G = 0; *RPL = 0; }
}
// LDS bytes of one group's haplotype codes: G pad + codes + G pad + prefetch slack (see the kernel's staging loop)
inline uint32_t hap_stride(uint32_t max_h, int G) { return (max_h + 2u * (uint32_t)G + 8u + 15u) & ~15u; }
// dynamic LDS of one block: per-wavefront emission table (fp32 only, `codes` columns) + per-group haplotype codes
inline uint32_t lds_bytes(const Bin& bin, bool f32, int codes = kMaxCodes) {
    const uint32_t waves = bin.block / 64u, groups = bin.block / (uint32_t)(f32 ? bin.G : bin.Gd);
    const uint32_t etab = f32 ? (uint32_t)((bin.RPL + 1) / 2) * (uint32_t)codes * 512u : 0u;
    return waves * etab + groups * bin.lds_stride;
}
// bins in order of (G, RPL): [G=4: 1..8][G=8: 1..8][G=16: 1..12][G=64: 4..16]
constexpr int kBinG8 = kNarrowMaxRPL, kBinG16 = kBinG8 + kG8MaxRPL, kBinG64 = kBinG16 + kG16MaxRPL;
constexpr int kBinStrip = kBinG64 + (kG64MaxRPL - kG64MinRPL + 1);      // the strip-mined class comes last
constexpr int kBins = kBinStrip + 1;
inline int bin_index(int G, int RPL) {
    if (G == 64 && RPL == kStripMarkRPL) return kBinStrip;
    return G == 4 ? RPL - 1 : G == 8 ? kBinG8 + RPL - 1 : G == 16 ? kBinG16 + RPL - 1 : kBinG64 + RPL - kG64MinRPL;
}
inline void bin_shape(int k, Bin* b) {
    if (k == kBinStrip) { b->G = 64; b->RPL = kG64MaxRPL; b->Gd = 64; b->RPLd = kG64MaxRPL; b->strip = true; return; }
    if (k < kBinG8) { b->G = 4; b->RPL = k + 1; }
    else if (k < kBinG16) { b->G = 8; b->RPL = k - kBinG8 + 1; }
    else if (k < kBinG64) { b->G = 16; b->RPL = k - kBinG16 + 1; }
    else { b->G = 64; b->RPL = k - kBinG64 + kG64MinRPL; }
    // the fp64 kernel keeps twice the registers per row: beyond 8 rows per lane of 16 it runs one
    // pair per wavefront instead
    if (b->G == 16 && b->RPL > 8) { b->Gd = 64; b->RPLd = (16 * b->RPL + 63) / 64; }
    else { b->Gd = b->G; b->RPLd = b->RPL; }
}
// device counters of a batch: [0, kBins) every class's own fp64 re-run list, kExactCount the exact tier's list (the
// second half of the re-run list), kSharedCount the narrow classes' shared fp64 list, [kNhapCount, kNhapCount + kBins)
// every class's N-haplotype list, kFormDeferCount how many entries of those lists (all classes) hold no N: test cases the
// five-operation cell of the first launch deferred
constexpr int kFormDeferCount = 61, kExactCount = 62, kSharedCount = 63, kNhapCount = 64, kCounters = 128;
static_assert(kBins <= kFormDeferCount && kNhapCount + kBins <= kCounters, "counter slots");

// launch geometry of a bin once job_count and max_h are known; `block` is 64, 128 or 256 threads (MGX_PAIRHMM_BLOCK)
inline int finalize_bin(Bin& bin, int n_cu, uint32_t block) {
    bin.lds_stride = hap_stride(bin.max_h, std::max(bin.G, bin.Gd));
    bin.block = block;
    while (bin.block > 64u && lds_bytes(bin, true) > kMaxLdsPerBlock) bin.block /= 2;
    if (lds_bytes(bin, true) > kMaxLdsPerLaunch) {
        set_error("haplotype of %u bases does not fit the LDS staging buffer", bin.max_h);
        return -E2BIG;
    }
    if (bin.strip) {
        // one test case per workgroup, a bounded grid walking the job list: the boundary rows between strips live in
        // a scratch array indexed by workgroup
        bin.block = 64;
        bin.grid_f32 = bin.grid_f64 = bin.grid_f64_all = std::min<uint32_t>(bin.job_count, (uint32_t)n_cu * 4u);
        return 0;
    }
    const uint32_t gpb = bin.block / bin.G, gpbd = bin.block / bin.Gd;
    bin.grid_f32 = (bin.job_count + gpb - 1) / gpb;
    bin.grid_f64_all = (bin.job_count + gpbd - 1) / gpbd;
    bin.grid_f64 = std::min<uint32_t>(bin.grid_f64_all, (uint32_t)n_cu * 8u);
    bin.grid_nhap = std::min<uint32_t>(bin.grid_f32, (uint32_t)n_cu * 8u);
    return 0;
}
// Fold sparsely populated bins into the next larger row class of the same group width (any RPL >= ceil(R / G) is
// valid, it only leaves lanes unused): a region-sized batch then needs one fp32 + one fp64 launch instead of one pair
// per read-length class.  merge_below: classes of fewer test cases are folded; kMergeBelow unless MGX_PAIRHMM_MERGE_BELOW
// says otherwise, and 1 folds none.  (The limit is the last parameter here and in classify_pairs and cross_bins, with kMergeBelow
// as its default: the library passes it everywhere, a driver written before it existed still compiles and plans as before.)
inline void merge_small_bins(uint64_t (&count)[kBins], int (&remap)[kBins], uint64_t merge_below = kMergeBelow) {
    for (int k = 0; k < kBins; ++k) remap[k] = k;
    for (int k = 0; k + 1 < kBins; ++k) {
        if (k + 1 == kBinG8 || k + 1 == kBinG16 || k + 1 == kBinG64 || k + 1 == kBinStrip) continue;   // never across a group-width boundary
        if (count[k] && count[k] < merge_below) { count[k + 1] += count[k]; count[k] = 0; remap[k] = k + 1; }
    }
    for (int k = 0; k < kBins; ++k) { int t = k; while (remap[t] != t) t = remap[t]; remap[k] = t; }
}

// what a test case of R x H costs: cells of the recurrence, and the bytes an implementation has to move for it
inline uint64_t pair_cells(uint64_t R, uint64_t H) { return R * H; }
inline uint64_t pair_bytes(uint64_t R, uint64_t H) { return 5 * R + H + 4; }

// ---- pair-list batches ---------------------------------------------------------------------------------------------
struct PairView {                    // the test cases of a batch and the offset tables they index
    uint64_t n = 0, n_reads = 0, n_haps = 0;
    const uint32_t *pr = nullptr, *ph = nullptr;
    const uint64_t *roff = nullptr, *hoff = nullptr;
    uint64_t R(uint64_t i) const { return roff[pr[i] + 1] - roff[pr[i]]; }
    uint64_t H(uint64_t i) const { return hoff[ph[i] + 1] - hoff[ph[i]]; }
};
struct PairClasses {
    std::vector<uint32_t> bin_of;    // every test case's class, after the folding of small classes
    uint64_t count[kBins] = {0};
    uint32_t max_h = 0;
};

// bin by (G, RPL), small classes folded
inline int classify_pairs(const PairView& v, int min_g, PairClasses* pc, uint64_t merge_below = kMergeBelow) {
    pc->bin_of.resize(v.n);
    for (uint64_t i = 0; i < v.n; ++i) {
        if (v.pr[i] >= v.n_reads || v.ph[i] >= v.n_haps) { set_error("test case %llu: index out of range", (unsigned long long)i); return -EINVAL; }
        const uint64_t R = v.R(i), H = v.H(i);
        if (R == 0 || H == 0) { set_error("test case %llu: empty read or haplotype", (unsigned long long)i); return -EINVAL; }
        int G, RPL;
        shape_of((uint32_t)std::min<uint64_t>(R, 0xFFFFFFFFull), min_g, &G, &RPL);
        if (G == 0) { set_error("test case %llu: read of %llu bases exceeds the %d-row limit", (unsigned long long)i, (unsigned long long)R, kMaxRowsStrip); return -E2BIG; }
        if (H > 0x7FFFFFF0ull) { set_error("haplotype too long"); return -E2BIG; }
        const int bi = bin_index(G, RPL);
        pc->bin_of[i] = (uint32_t)bi;
        pc->count[bi]++;
        pc->max_h = std::max<uint32_t>(pc->max_h, (uint32_t)H);
    }
    int remap[kBins];
    merge_small_bins(pc->count, remap, merge_below);
    for (uint64_t i = 0; i < v.n; ++i) pc->bin_of[i] = (uint32_t)remap[pc->bin_of[i]];
    return 0;
}

// The jobs in launch order, into jobs[0, n), and the classes that hold any.  key = (bin, H descending): counting sort
// on H inside each bin keeps the wavefront's groups (consecutive jobs) at near-equal step counts, and longest first
// means the last workgroups of a launch -- its drain -- are the shortest jobs.
inline int sort_pairs(const PairView& v, const PairClasses& pc, int n_cu, uint32_t block, Job* jobs, std::vector<Bin>* bins) {
    const uint32_t max_h = pc.max_h;
    uint64_t bin_start[kBins + 1] = {0};
    for (int k = 0; k < kBins; ++k) bin_start[k + 1] = bin_start[k] + pc.count[k];
    std::vector<std::vector<uint32_t>> hist(kBins);
    for (int k = 0; k < kBins; ++k) if (pc.count[k]) hist[k].assign((size_t)max_h + 2, 0);
    for (uint64_t i = 0; i < v.n; ++i) hist[pc.bin_of[i]][(max_h - (uint32_t)v.H(i)) + 1]++;
    for (int k = 0; k < kBins; ++k)
        for (size_t x = 1; x < hist[k].size(); ++x) hist[k][x] += hist[k][x - 1];
    for (uint64_t i = 0; i < v.n; ++i) {
        const uint32_t H = (uint32_t)v.H(i);
        const int k = (int)pc.bin_of[i];
        Job& jb = jobs[bin_start[k] + hist[k][max_h - H]++];
        jb.read_off = v.roff[v.pr[i]]; jb.hap_off = v.hoff[v.ph[i]];
        jb.R = (uint32_t)v.R(i); jb.H = H; jb.pair = (uint32_t)i; jb.pad_ = 0;
    }
    for (int k = 0; k < kBins; ++k) {
        if (!pc.count[k]) continue;
        Bin bin;
        bin_shape(k, &bin);
        bin.job_begin = (uint32_t)bin_start[k];
        bin.job_count = (uint32_t)pc.count[k];
        for (uint64_t q = bin_start[k]; q < bin_start[k + 1]; ++q) {
            bin.max_h = std::max(bin.max_h, jobs[q].H);
            bin.cells += pair_cells(jobs[q].R, jobs[q].H);
            bin.alg_bytes += pair_bytes(jobs[q].R, jobs[q].H);
        }
        if (const int rc = finalize_bin(bin, n_cu, block)) return rc;
        bins->push_back(bin);
    }
    return 0;
}

// ---- the slab ------------------------------------------------------------------------------------------------------
// The six sequence arrays of a batch, in the order every table of them goes by.
enum { kSeqBases, kSeqQual, kSeqIns, kSeqDel, kSeqGcp, kSeqHap, kSeqArrays };

// Where the arrays of a batch lie in its slab.  The inputs are written once (one H2D copy when staged through the
// pinned mirror), [out | used | keep] is read back with one D2H copy, what follows is device scratch.  The pair-list
// form writes its jobs on the host, first in the mirror; the cross-product form uploads the tables that the device
// enumerates them from and keeps the jobs in scratch.
struct SlabLayout {
    // sizes: set by the caller
    uint64_t n = 0, n_reads = 0, n_haps = 0, n_regions = 0, read_bytes = 0, hap_bytes = 0;
    bool cross = false, model = false;
    // the wire form (pair-list batches of a context with MGX_PAIRHMM_WIRE): the uploaded prefix is [jobs | bases4 | qual |
    // ins | del | gcp | hap4] at wseq[], and seq[] lies in device scratch.  Asked for by the caller, decided by plan_slab.
    bool wire = false;
    mgx::wire::Widths ww;
    // offsets: set by plan_slab
    size_t rtab = 0, rreg = 0, rpre = 0, gtab = 0, htab = 0;      // cross-product form: what the jobs are enumerated from
    size_t jobs = 0, seq[kSeqArrays] = {0}, wseq[kSeqArrays] = {0};
    size_t mapq = 0, rlen = 0, roff = 0, rnh = 0;                 // with a read model: per read, for the model and the epilogue
    size_t in_bytes = 0, o_out = 0, o_used = 0, o_keep = 0, result_bytes = 0;
    size_t pin_bytes = 0;                                         // the pinned mirror covers the inputs and the results only
    size_t rlist = 0, nlist = 0, rcount = 0, total = 0;
    bool staged = true;

    uint64_t seq_len(int k) const { return k == kSeqHap ? hap_bytes : read_bytes; }
    // 4: nibble codes; 6 / 7: bit stream; 0: every byte is ww.gcp_const
    uint32_t wire_width(int k) const { return k == kSeqBases || k == kSeqHap ? 4u : k == kSeqQual ? ww.qual : k == kSeqIns ? ww.ins : k == kSeqDel ? ww.del : ww.gcp; }
    uint64_t wire_len(int k) const { return wire_width(k) == 4 ? mgx::wire::nibble_bytes(seq_len(k)) : mgx::wire::stream_bytes(seq_len(k), wire_width(k)); }
};

// Decides the offsets; the batch is staged through a pinned mirror if always_stage or if inputs and results fit kStageLimit.
inline void plan_slab(bool always_stage, SlabLayout* L) {
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off = align_up(off + bytes); return at; };
    const uint64_t n = L->n, per_read = L->model ? L->n_reads : 0;
    if (L->cross) {
        L->rtab = take(L->n_reads * sizeof(SeqRef));
        L->rreg = take(L->n_reads * sizeof(uint32_t));
        L->rpre = take((L->n_reads + 1) * sizeof(uint32_t));
        L->gtab = take(L->n_regions * sizeof(RegionRef));
        L->htab = take(L->n_haps * sizeof(SeqRef));
    } else {
        L->jobs = take(n * sizeof(Job));
    }
    auto take_expanded = [&] { for (int k = 0; k < kSeqArrays; ++k) L->seq[k] = take(L->seq_len(k)); };
    // the wire form is for batches that go through the pinned mirror: those the plain form would stage
    if (L->wire && (L->cross || (!always_stage && align_up(n * sizeof(Job)) + 5 * align_up(L->read_bytes) + align_up(L->hap_bytes) +
                                                       align_up(n * sizeof(double)) + align_up(n) > kStageLimit))) L->wire = false;
    if (L->wire) for (int k = 0; k < kSeqArrays; ++k) L->wseq[k] = take(L->wire_len(k));
    else take_expanded();
    L->mapq = take(per_read);
    L->rlen = take(per_read * sizeof(uint64_t));
    L->roff = take(per_read * sizeof(uint32_t));
    L->rnh = take(per_read * sizeof(uint32_t));
    L->in_bytes = off;
    L->o_out = take(n * sizeof(double));
    L->o_used = take(n);
    L->o_keep = take(per_read);
    L->result_bytes = off - L->o_out;
    L->pin_bytes = off;
    if (L->cross) L->jobs = take(n * sizeof(Job));
    if (L->wire) take_expanded();                    // what pairhmm_expand_wire writes
    L->rlist = take(2 * n * sizeof(uint32_t));       // fp64 re-run lists | exact-tier list
    L->nlist = take(n * sizeof(uint32_t));           // N-haplotype lists of the four-code fp32 launches
    L->rcount = take(kCounters * sizeof(uint32_t));
    L->total = off;
    L->staged = always_stage || L->pin_bytes <= kStageLimit;
}

// The grid of pairhmm_expand_wire, laid over the concatenated work of the six arrays, one thread per 8 positions: per array
// its positions (= output bytes), its width and its first workgroup; block_first[6] is the grid.
inline int expand_grid(const SlabLayout& L, uint64_t (&n)[kSeqArrays], uint32_t (&w)[kSeqArrays], uint32_t (&block_first)[kSeqArrays + 1]) {
    uint64_t blocks = 0;
    for (int k = 0; k < kSeqArrays; ++k) {
        w[k] = L.wire_width(k);
        n[k] = L.seq_len(k);
        block_first[k] = (uint32_t)blocks;
        blocks += ((n[k] + 7) / 8 + kExpandBlock - 1) / kExpandBlock;
        if (blocks > 0x7FFFFFFFull) { set_error("batch too large for one expansion launch"); return -E2BIG; }
    }
    block_first[kSeqArrays] = (uint32_t)blocks;
    return 0;
}

// ---- cross-product batches -------------------------------------------------------------------------------------------
// Row F1: the cross-product test cases (pair_read == pair_hap == NULL: every read against every haplotype,
// out[r * n_haps + h]) of one or several regions in one batch -- one upload, one set of launches, one download.
// Host work is linear in reads + haplotypes (the test cases are enumerated on the device), so coalescing a
// thousand small regions costs microseconds, not a pair list.
struct CrossRead { uint64_t off; uint32_t len, region; uint8_t bin; };
struct CrossPlan {
    uint64_t nr = 0, nh = 0, n = 0, read_bytes = 0, hap_bytes = 0;
    std::vector<CrossRead> reads;          // in global read order: offsets rebased to the batch's concatenated arrays
    std::vector<RegionRef> regions;
    std::vector<SeqRef> haps;              // region by region, each in stable order of decreasing length
    uint32_t max_h = 0;
    uint64_t rstart[kBins + 1] = {0};      // where every class starts in the read table
};

// totals of the batch, and where every region's [reads][haps] block starts in the output
inline int cross_totals(uint32_t n_regions, const mgx_pairhmm_input_t* regs, CrossPlan* p, std::vector<uint64_t>* out_base) {
    out_base->assign(n_regions + 1, 0);
    for (uint32_t g = 0; g < n_regions; ++g) {
        const mgx_pairhmm_input_t& in = regs[g];
        if (in.pair_read || in.pair_hap) { set_error("region %u: regions are given in the cross-product form (pair arrays NULL)", g); return -EINVAL; }
        p->nr += in.n_reads; p->nh += in.n_haps; p->n += in.n_reads * in.n_haps;
        if (in.n_reads) p->read_bytes += in.read_off[in.n_reads] - in.read_off[0];
        if (in.n_haps) p->hap_bytes += in.hap_off[in.n_haps] - in.hap_off[0];
        (*out_base)[g + 1] = p->n;
    }
    if (p->n > 0xFFFFFFF0ull || p->nr > 0xFFFFFFF0ull) { set_error("more than 2^32 test cases in one batch"); return -E2BIG; }
    return 0;
}

// read, region and haplotype tables; job counts per read-length class in count[]
inline int cross_tables(uint32_t n_regions, const mgx_pairhmm_input_t* regs, const std::vector<uint64_t>& out_base, int min_g, CrossPlan* p,
                        uint64_t (&count)[kBins]) {
    p->reads.resize(p->nr); p->regions.resize(n_regions); p->haps.resize(p->nh);
    uint64_t r_at = 0, h_at = 0, rb = 0, hb = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        const mgx_pairhmm_input_t& in = regs[g];
        RegionRef& R = p->regions[g];
        R.hap_begin = (uint32_t)h_at; R.n_haps = (uint32_t)in.n_haps; R.read_base = (uint32_t)r_at; R.out_base = (uint32_t)out_base[g];
        for (uint64_t h = 0; h < in.n_haps; ++h) {
            const uint64_t H = in.hap_off[h + 1] - in.hap_off[h];
            if (H == 0) { set_error("region %u: haplotype %llu is empty", g, (unsigned long long)h); return -EINVAL; }
            if (H > 0x7FFFFFF0ull) { set_error("haplotype too long"); return -E2BIG; }
            p->haps[h_at + h] = SeqRef{hb + (in.hap_off[h] - in.hap_off[0]), (uint32_t)H, (uint32_t)h};
            p->max_h = std::max<uint32_t>(p->max_h, (uint32_t)H);
        }
        std::stable_sort(p->haps.begin() + h_at, p->haps.begin() + h_at + in.n_haps, [](const SeqRef& a, const SeqRef& b2) { return a.len > b2.len; });
        for (uint64_t r = 0; r < in.n_reads; ++r) {
            const uint64_t Rl = in.read_off[r + 1] - in.read_off[r];
            if (Rl == 0) { set_error("region %u: read %llu is empty", g, (unsigned long long)r); return -EINVAL; }
            int G, RPL;
            shape_of((uint32_t)std::min<uint64_t>(Rl, 0xFFFFFFFFull), min_g, &G, &RPL);
            if (G == 0) { set_error("region %u: read of %llu bases exceeds the %d-row limit", g, (unsigned long long)Rl, kMaxRowsStrip); return -E2BIG; }
            CrossRead& ri = p->reads[r_at + r];
            ri.off = rb + (in.read_off[r] - in.read_off[0]); ri.len = (uint32_t)Rl; ri.region = g; ri.bin = (uint8_t)bin_index(G, RPL);
            count[ri.bin] += in.n_haps;
        }
        if (in.n_reads) rb += in.read_off[in.n_reads] - in.read_off[0];
        if (in.n_haps) hb += in.hap_off[in.n_haps] - in.hap_off[0];
        r_at += in.n_reads; h_at += in.n_haps;
    }
    return 0;
}

// Folds the small classes and makes the classes that hold any test case, in job order: jobs are laid out in read-table order,
// which is class order.
inline int cross_bins(CrossPlan* p, uint64_t (&count)[kBins], int n_cu, uint32_t block, std::vector<Bin>* bins, uint64_t merge_below = kMergeBelow) {
    int remap[kBins];
    merge_small_bins(count, remap, merge_below);
    std::vector<uint64_t> sumH(p->regions.size(), 0);
    for (size_t g = 0; g < p->regions.size(); ++g)
        for (uint32_t h = 0; h < p->regions[g].n_haps; ++h) sumH[g] += p->haps[p->regions[g].hap_begin + h].len;
    uint64_t reads_in[kBins] = {0}, jobs_in[kBins] = {0}, cells_in[kBins] = {0}, bytes_in[kBins] = {0}, job_begin = 0;
    for (CrossRead& ri : p->reads) {
        ri.bin = (uint8_t)remap[ri.bin];
        const RegionRef& R = p->regions[ri.region];
        // the read against every haplotype of its region: pair_cells and pair_bytes summed over them
        reads_in[ri.bin]++; jobs_in[ri.bin] += R.n_haps; cells_in[ri.bin] += pair_cells(ri.len, sumH[ri.region]);
        bytes_in[ri.bin] += R.n_haps * pair_bytes(ri.len, 0) + sumH[ri.region];
    }
    for (int k = 0; k < kBins; ++k) {
        p->rstart[k + 1] = p->rstart[k] + reads_in[k];
        if (!jobs_in[k]) continue;      // no read, or only reads of regions without haplotypes: they stay in the read table, nothing is launched
        Bin bin;
        bin_shape(k, &bin);
        bin.job_begin = (uint32_t)job_begin;
        bin.job_count = (uint32_t)jobs_in[k];
        bin.max_h = p->max_h;
        bin.cells = cells_in[k];
        bin.alg_bytes = bytes_in[k];
        if (const int rc = finalize_bin(bin, n_cu, block)) return rc;
        bins->push_back(bin);
        job_begin += bin.job_count;
    }
    return 0;
}

// what pairhmm_make_jobs_multi enumerates from: the read table in (class, input) order, every entry's region, and the
// first job of every entry (nr + 1 values)
inline void cross_write_tables(const CrossPlan& p, SeqRef* rtab, uint32_t* rreg, uint32_t* rpre) {
    uint64_t cur[kBins];
    for (int k = 0; k < kBins; ++k) cur[k] = p.rstart[k];
    for (uint64_t r = 0; r < p.nr; ++r) {
        const CrossRead& ri = p.reads[r];
        const uint64_t at = cur[ri.bin]++;
        rtab[at] = SeqRef{ri.off, ri.len, (uint32_t)r};
        rreg[at] = ri.region;
    }
    uint32_t run = 0;
    for (uint64_t at = 0; at < p.nr; ++at) { rpre[at] = run; run += p.regions[rreg[at]].n_haps; }
    rpre[p.nr] = run;
}

// per read, in global read order: length, where its row of the output starts and how many haplotypes it holds
inline void cross_write_rows(uint32_t n_regions, const mgx_pairhmm_input_t* regs, const std::vector<uint64_t>& out_base,
                             uint64_t* rlen, uint32_t* roff, uint32_t* rnh) {
    uint64_t r_at = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        const mgx_pairhmm_input_t& in = regs[g];
        for (uint64_t r = 0; r < in.n_reads; ++r) {
            rlen[r_at + r] = in.read_off[r + 1] - in.read_off[r];
            roff[r_at + r] = (uint32_t)(out_base[g] + r * in.n_haps);
            rnh[r_at + r] = (uint32_t)in.n_haps;
        }
        r_at += in.n_reads;
    }
}

// ---- region lists ----------------------------------------------------------------------------------------------------
// Cuts a list of regions into runs of whole regions of about `limit` test cases: a run ends in front of the region
// that would take it past the limit (a region larger than the limit is a run of its own).  cut: the boundaries.
inline void cut_regions(const mgx_pairhmm_input_t* regions, uint32_t n_regions, uint64_t limit, std::vector<uint32_t>* cut) {
    cut->assign(1, 0);
    uint64_t in_run = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        const uint64_t n = regions[g].n_reads * regions[g].n_haps;
        if (in_run && in_run + n > limit) { cut->push_back(g); in_run = 0; }
        in_run += n;
    }
    if (n_regions) cut->push_back(n_regions);
}
// Test cases per chunk of mgx_pairhmm_compute_regions: a sixth of the job, from 196 608 to 393 216.
// (tools/dev_regions_chunk.py, 1000 regions of 40 x 25 on an MI355X: 65 536 test cases per chunk 2 430 GCUPS, 131 072 3 035,
// 196 608 3 193, 262 144 2 980-3 190, 524 288 2 610, one chunk 2 090: larger chunks mean larger class launches, fewer of them
// mean less of the flattening hidden behind the kernels)
// Larger jobs take larger chunks: 1000 regions of 100 x 50 (5 M test cases) 3 440 GCUPS with 131 072 per chunk, 3 790 with
// 196 608, 4 160 with 393 216, 3 960 with 524 288; 200 regions of 300 x 100: 3 640 / 4 050 / 4 560 / 4 370; 4000 regions of
// 40 x 25: 3 460 with 196 608, 3 620 with 393 216 (tools/dev_regions_chunk_shapes.py)
inline uint64_t region_chunk_pairs(uint64_t total) { return std::min<uint64_t>(6u << 16, std::max<uint64_t>(3u << 16, total / 6)); }

// ---- the run -----------------------------------------------------------------------------------------------------------
// Re-runs in double precision: the "narrow" classes (at most 16 lanes x 8 rows: every read up to 128 bases) append
// to ONE list (their jobs are a prefix of the job array) that ONE fp64 launch of the 16 x RPLd shape processes --
// a test case's value does not depend on the shape that computes it; wider classes keep a list and a launch each.
inline bool is_narrow(const Bin& bn) { return bn.G <= 16 && bn.G * bn.RPL <= 16 * kNarrowMaxRPL; }

// extent of the narrow classes: what the shared fp64 launch has to cover
struct NarrowExtent {
    size_t first = 0;                  // books the shared fp64 launch; bins.size() if there is no narrow class
    uint32_t n_jobs = 0, max_h = 0, rows = 0;
};
inline NarrowExtent survey_narrow(const std::vector<Bin>& bins) {
    NarrowExtent e;
    e.first = bins.size();
    for (size_t k = 0; k < bins.size(); ++k) {
        const Bin& bn = bins[k];
        if (!is_narrow(bn)) continue;
        if (e.first == bins.size()) e.first = k;
        e.n_jobs = std::max(e.n_jobs, bn.job_begin + bn.job_count);
        e.max_h = std::max(e.max_h, bn.max_h);
        e.rows = std::max(e.rows, (uint32_t)(bn.G * bn.RPL));
    }
    return e;
}

// Several narrow classes: one multi-class launch per lane-width set (0: G = 16, 1: G < 16) instead of one launch per class.
// Only SMALL classes share a launch: measured on an MI355X (profiles/r02_pairhmm_multi_ab.txt) the common launch
// costs every class the register budget of the hungriest one (131-149 VGPRs: 3 wavefronts per SIMD; 4 when forced,
// with spills), which outweighs the saved drains for classes that fill the device on their own (ragged 1 M test
// cases, nine classes of ~29 000 workgroups: 4462 -> 4343 GCUPS) but not for classes of a few thousand workgroups
// (reads of 20-32 bases: 2764 -> 3009; region-sized batches).  (The same build forced to 4 wavefronts per SIMD, and
// sharing a launch among all narrow classes whatever their size, were measured too and lost: DESIGN.md 3.5.)
struct MultiSet {
    std::vector<size_t> members;       // in launch order; empty if the classes do not make a set
    uint32_t block_first[kMultiBins + 1] = {0};      // every member's first workgroup (of 64 threads); [members.size()]: the grid
    uint32_t lds = 0;                                // the members' largest four-code footprint
};
inline MultiSet multi_set(const std::vector<Bin>& bins, int gset, int n_cu) {
    const uint32_t multi_below = (uint32_t)n_cu * 64u;     // workgroups; ~5 device fills
    MultiSet ms;
    std::vector<size_t>& set = ms.members;
    for (size_t k = 0; k < bins.size(); ++k) {
        const Bin& bn = bins[k];
        if (is_narrow(bn) && bn.RPL <= kNarrowMaxRPL && bn.block == 64 && bn.grid_f32 < multi_below && (gset == 0 ? bn.G == 16 : bn.G < 16)) set.push_back(k);
    }
    if (set.size() < 2 || set.size() > (size_t)kMultiBins) set.clear();
    // most rows per lane first (the costliest workgroups), wider groups first among equals
    std::stable_sort(set.begin(), set.end(), [&](size_t x, size_t y) {
        const Bin &bx = bins[x], &by = bins[y];
        return bx.RPL != by.RPL ? bx.RPL > by.RPL : bx.G > by.G;
    });
    for (size_t q = 0; q < set.size(); ++q) {
        ms.block_first[q + 1] = ms.block_first[q] + bins[set[q]].grid_f32;
        ms.lds = std::max(ms.lds, lds_bytes(bins[set[q]], true, 4));
    }
    return ms;
}

// the order the classes launch in: largest first
inline std::vector<size_t> class_order(const std::vector<Bin>& bins) {
    std::vector<size_t> order(bins.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return bins[x].cells > bins[y].cells; });
    return order;
}


}  // namespace mgx_hmm_plan
#pragma GCC visibility pop
