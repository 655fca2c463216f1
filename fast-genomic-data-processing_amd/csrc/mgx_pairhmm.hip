// mgx_pairhmm.hip -- host side of the PairHMM C ABI (include/mgx_pairhmm.h) for MI355X.
//
// Replaces, behind a plain C boundary, the reference's native PairHMM layer
// (deepmutect/Mutect2Cpp-master/src/intel/pairhmm/IntelPairHmm.cc:202-351): table set-up,
// float-first / double-fallback policy and the per-test-case loop.  The per-test-case loop
// becomes: bin test cases by read-length class, sort each bin by haplotype length, launch one
// fp32 kernel per bin, then one fp64 kernel per bin over the device-side re-run list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <vector>

#include "../../include/mgx_pairhmm.h"
#include "../../include/mgx_realign.h"
#include "mgx_common.h"
#include "mgx_realign_internal.h"
#include "mgx_tables.h"
#include "pairhmm_pack.h"
#include "pairhmm_wire.h"
#include "pairhmm_kernels.hip.inc"

using mgx::set_error;

namespace {

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
// Longer reads are strip-mined: 64 lanes x 16 rows per strip, the strips sweep the haplotype one after the other
// (pairhmm_fwd_strip).  The limit below only keeps row indices and the boundary scratch in 32 bits.
constexpr int kMaxRowsStrip = 1 << 20;
constexpr int kStripMarkRPL = kG64MaxRPL + 1;      // shape_of's RPL value for the strip-mined class
constexpr uint32_t kMaxLdsPerBlock = 64 * 1024;

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


// One device allocation + (for batches up to kStageLimit) a pinned host mirror of the same size.
// Slabs are recycled through the context, so a stream of region-sized batches does no hipMalloc.
struct Slab {
    uint8_t* dev = nullptr;
    uint8_t* pin = nullptr;     // mirrors the first pin_cap bytes only: inputs and results, never device scratch
    size_t cap = 0, pin_cap = 0;
};
constexpr size_t kStageLimit = 256u << 20;
constexpr size_t kMaxEventSets = 64;       // runs whose kernel durations a timed batch remembers
constexpr size_t kMinSlab = 1u << 20;
}  // namespace

struct mgx_pairhmm {
    int device = 0;
    unsigned flags = 0;
    hipStream_t compute = nullptr, copy = nullptr, d2h = nullptr;   // kernels | uploads | result downloads
    // a batch with several read-length classes launches one kernel per class: they are dealt to the compute
    // stream and these side streams so that the drain of one launch overlaps the body of the others
    static constexpr int kAux = 3;
    hipStream_t aux[kAux] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kAux] = {nullptr, nullptr, nullptr};
    int n_streams = 1;
    float* d_ph2pr_f = nullptr; float* d_mm_f = nullptr; float* d_div3_f = nullptr; float* d_ratio_f = nullptr;
    double* d_ph2pr_d = nullptr; double* d_mm_d = nullptr; double* d_div3_d = nullptr; double* d_ratio_d = nullptr;
    float log10_initial_f = 0; double log10_initial_d = 0;
    int n_cu = 256;
    bool wire = false;           // MGX_PAIRHMM_WIRE, or its environment override: staged pair-list batches upload the wire form
    std::vector<Slab> free_slabs;
    void* d_strip = nullptr; size_t strip_cap = 0;      // boundary rows of the strip-mined class (one compute stream: launches do not overlap)
    mgx_internal::PairhmmExt ext;                       // mgx_realign.hip's buffers and statistics
};

struct mgx_pairhmm_batch {
    uint64_t n_pairs = 0;
    std::vector<Bin> bins;
    // everything lives in one slab: [jobs | bases | qual | ins | del | gcp | hap] is written once
    // (one H2D copy when staged through the pinned mirror), [out | used] is read back with one
    // D2H copy, [rerun_list | rerun_count] is device scratch.  In the wire form the written prefix is
    // [jobs | bases4 | qual | ins | del | gcp | hap4] and the six arrays are expanded into device scratch.
    Slab slab;
    size_t in_bytes = 0, o_out = 0, o_used = 0, result_bytes = 0;
    uint64_t read_bytes = 0, hap_bytes = 0;      // lengths of the five read arrays and of the haplotype array
    uint8_t *d_bases = nullptr, *d_qual = nullptr, *d_ins = nullptr, *d_del = nullptr,
            *d_gcp = nullptr, *d_hap = nullptr, *d_used = nullptr;
    Job* d_jobs = nullptr;
    uint32_t* d_rerun_list = nullptr;
    uint32_t* d_rerun_count = nullptr;
    uint32_t* d_nhap_list = nullptr;   // N-haplotype test cases of the four-code launches, every class at its job_begin
    double* d_out = nullptr;
    std::vector<Job> host_jobs;    // only kept for unstaged (very large) batches
    // whole-region form (mgx_pairhmm_regions): normalise / filter epilogue over every read's row of the output
    bool has_model = false;
    uint32_t n_reads = 0;
    uint64_t* d_read_len = nullptr;
    uint8_t* d_keep = nullptr;
    uint32_t *d_row_off = nullptr, *d_row_nh = nullptr;   // per read: where its row starts and how many haplotypes it holds
    size_t o_keep = 0;
    double log10_rate = 0, max_err = 0;
    hipEvent_t uploaded = nullptr;
    // timing: a ring of event sets, one set per run (4 per bin: f32 start/stop, f64 start/stop), so that
    // every run of a timed loop is measured and batch_stats can average them after the final sync
    std::vector<hipEvent_t> ev;
    // what every class's fp32 event pair covers in the last run: its own launch, a whole multi-class launch (booked on
    // the member with the most cells) or nothing (the other members)
    std::vector<uint64_t> acct_cells, acct_bytes;
    std::vector<int8_t> acct_multi;    // 0: single-class kernel, 1 + GSET: multi-class kernel
    uint32_t ev_sets = 0;          // sets allocated
    uint32_t runs_timed = 0;       // runs recorded since the last batch_stats
    hipEvent_t done = nullptr;     // recorded on the compute stream behind the last kernel of a run
    bool ran = false;
    mgx_pairhmm_stats_t stats{};
};

namespace {

using BatchPtr = std::unique_ptr<mgx_pairhmm_batch, void (*)(mgx_pairhmm_batch*)>;
BatchPtr new_batch() {
    // (on an error path the slab is freed, not pooled: destroy is called without the context)
    return BatchPtr(new (std::nothrow) mgx_pairhmm_batch, [](mgx_pairhmm_batch* p) { mgx_pairhmm_batch_destroy(nullptr, p); });
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,     \
                      __LINE__);                                                           \
            return -EIO;                                                                   \
        }                                                                                  \
    } while (0)

template <typename T>
int upload(T** dst, const void* src, size_t bytes, hipStream_t s) {
    *dst = nullptr;
    if (bytes == 0) bytes = 16;
    HIP_TRY(hipMalloc((void**)dst, bytes));
    if (src) HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, s));
    return 0;
}

// (G, RPL) class of a read of R rows; G = 0 if unsupported.  MGX_PAIRHMM_MIN_G=16 switches the narrow groups off.
inline void shape_of(uint32_t R, int* G, int* RPL) {
    static const int min_g = [] { const char* e = getenv("MGX_PAIRHMM_MIN_G"); const int v = e ? atoi(e) : 4; return v; }();
    const uint32_t g8_rows = (uint32_t)kMaxRowsG8;
    if (R <= (uint32_t)kMaxRowsG4 && min_g <= 4) { *G = 4; *RPL = (int)((R + 3) / 4); }
    else if (R <= g8_rows && min_g <= 8) { *G = 8; *RPL = (int)((R + 7) / 8); }
    else if (R <= (uint32_t)kMaxRowsG16) { *G = 16; *RPL = (int)((R + 15) / 16); }
    else if (R <= (uint32_t)kMaxRowsG64) { *G = 64; *RPL = std::max(kG64MinRPL, (int)((R + 63) / 64)); }
    else if (R <= (uint32_t)kMaxRowsStrip) { *G = 64; *RPL = kStripMarkRPL; }
    else { *G = 0; *RPL = 0; }
}
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
constexpr uint64_t kMergeBelow = 4096;
// device counters of a batch: [0, kBins) every class's own fp64 re-run list, 62 the exact tier's list, 63 the narrow
// classes' shared fp64 list, [kNhapCount, kNhapCount + kBins) every class's N-haplotype list
constexpr int kNhapCount = 64, kCounters = 128;
static_assert(kBins <= 62 && kNhapCount + kBins <= kCounters, "counter slots");

// launch geometry of a bin once job_count and max_h are known
int finalize_bin(Bin& bin, int n_cu) {
    // LDS per group: G pad + codes + G pad + prefetch slack (see the kernel's staging loop)
    bin.lds_stride = (bin.max_h + 2u * (uint32_t)std::max(bin.G, bin.Gd) + 8u + 15u) & ~15u;
    bin.block = 64;                   // one wavefront per workgroup: finest LDS/VGPR packing per CU, no cross-wave
                                      // barriers; in-process A/B at 1 M pairs: 5.48 ms (64), 5.65 (128), 5.46 (256)
    if (const char* e = getenv("MGX_PAIRHMM_BLOCK")) { const int v = atoi(e); if (v == 64 || v == 128 || v == 256) bin.block = (uint32_t)v; }
    while (bin.block > 64u && lds_bytes(bin, true) > kMaxLdsPerBlock) bin.block /= 2;
    if (lds_bytes(bin, true) > 160u * 1024u) {
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
// fold sparsely populated bins into the next larger row class of the same group width
void merge_small_bins(uint64_t (&count)[kBins], int (&remap)[kBins]) {
    for (int k = 0; k < kBins; ++k) remap[k] = k;
    for (int k = 0; k + 1 < kBins; ++k) {
        if (k + 1 == kBinG8 || k + 1 == kBinG16 || k + 1 == kBinG64 || k + 1 == kBinStrip) continue;   // never across a group-width boundary
        if (count[k] && count[k] < kMergeBelow) { count[k + 1] += count[k]; count[k] = 0; remap[k] = k + 1; }
    }
    for (int k = 0; k < kBins; ++k) { int t = k; while (remap[t] != t) t = remap[t]; remap[k] = t; }
}

constexpr size_t kSlabAlign = 256;          // every array of a slab starts on a multiple of this and owns the bytes up to the next
inline size_t align_up(size_t x, size_t a = kSlabAlign) { return (x + a - 1) / a * a; }

// ---- the wire form's device side (pairhmm_wire.h): one launch on the copy stream, right behind the H2D copy, turns
// [bases4 | qual | ins | del | gcp | hap4] back into the six byte arrays the PairHMM kernels read.  The grid is laid
// over the concatenated work of the six arrays; which array a workgroup serves is uniform over it.  One thread
// produces 8 output bytes with one 8-byte store: of a bit stream it reads the group's w bytes at byte offset w t, of
// nibble codes 4 bytes, which two byte permutes map through "ACTGN".  No LDS, nothing shared between threads.
constexpr uint32_t kExpandBlock = 256;
// the last thread of an array stores its full 8 bytes, up to 7 past the array's length: they fall into the array's own
// slab slot, which align_up rounds to a multiple of 8
static_assert(kSlabAlign % 8 == 0, "pairhmm_expand_wire stores whole 8-byte groups into slab slots");
struct ExpandWireArgs {
    const uint8_t* src[6];       // bases4, qual, ins, del, gcp, hap4
    uint8_t* dst[6];             // bases, qual, ins, del, gcp, hap
    uint64_t n[6];               // positions = output bytes
    uint32_t block_first[7];     // the first workgroup of every array; [6]: the grid
    uint32_t w[6];               // 4: nibble codes; 6 / 7: bit stream; 0: every byte is `fill`
    uint32_t fill;
};
__device__ __forceinline__ uint32_t nibbles_to_letters(uint32_t h) {      // four codes in 16 bits -> four ASCII bytes
    h = (h | (h << 8)) & 0x00FF00FFu;
    h = (h | (h << 4)) & 0x0F0F0F0Fu;
    return __builtin_amdgcn_perm(0x0000004Eu, 0x47544341u, h & 0x07070707u);      // idx 0..7 -> A C T G N 0 0 0 (mgx::wire::kLetters)
}
__global__ __launch_bounds__(kExpandBlock) void pairhmm_expand_wire(const ExpandWireArgs a) {
    const uint32_t blk = blockIdx.x;
    const uint8_t* src = a.src[0];
    uint8_t* dst = a.dst[0];
    uint64_t n = a.n[0];
    uint32_t first = 0, w = a.w[0];
#pragma unroll
    for (int k = 1; k < 6; ++k)
        if (blk >= a.block_first[k]) { src = a.src[k]; dst = a.dst[k]; n = a.n[k]; first = a.block_first[k]; w = a.w[k]; }
    const uint64_t t = (uint64_t)(blk - first) * kExpandBlock + threadIdx.x;      // this thread's group of eight positions
    if (8 * t >= n) return;
    uint64_t out;
    if (w == 4) {
        const uint64_t n_bytes = (n + 1) / 2;
        const uint8_t* p = src + 4 * t;
        uint32_t v = 0;
        if (4 * t + 4 <= n_bytes) v = *reinterpret_cast<const uint32_t*>(p);
        else for (uint64_t k = 0; 4 * t + k < n_bytes; ++k) v |= (uint32_t)p[k] << (8 * k);      // the array's last thread: nothing past ceil(n / 2) bytes
        out = nibbles_to_letters(v & 0xFFFFu) | (uint64_t)nibbles_to_letters(v >> 16) << 32;
    } else if (w == 0) {
        out = (uint64_t)a.fill * 0x0101010101010101ull;
    } else {
        const uint8_t* p = src + (uint64_t)w * t;      // whole groups only: the packer zero-fills the last one
        uint32_t lo;
        uint16_t mid;
        __builtin_memcpy(&lo, p, 4);
        __builtin_memcpy(&mid, p + 4, 2);
        const uint64_t v = lo | (uint64_t)mid << 32;
        out = w == 7 ? mgx::wire::spread8<7>(v | (uint64_t)p[6] << 48) : mgx::wire::spread8<6>(v);
    }
    *reinterpret_cast<uint64_t*>(dst + 8 * t) = out;
}

int acquire_slab(mgx_pairhmm* c, size_t bytes, size_t pin_bytes, Slab* out) {
    int best = -1;
    for (size_t i = 0; i < c->free_slabs.size(); ++i) {
        const Slab& f = c->free_slabs[i];
        if (f.cap >= bytes && f.pin_cap >= pin_bytes && (best < 0 || f.cap < c->free_slabs[best].cap)) best = (int)i;
    }
    if (best >= 0) { *out = c->free_slabs[best]; c->free_slabs.erase(c->free_slabs.begin() + best); return 0; }
    auto round = [](size_t want) {
        size_t cap = kMinSlab;
        while (cap < want) cap *= 2;
        if (cap > want + (want >> 2) && want > (64u << 20)) cap = align_up(want, 1u << 20);   // no 2x waste on big batches
        return cap;
    };
    Slab sl;
    sl.cap = round(bytes);
    HIP_TRY(hipMalloc((void**)&sl.dev, sl.cap));
    if (pin_bytes) {
        sl.pin_cap = std::min(sl.cap, round(pin_bytes));
        if (hipHostMalloc((void**)&sl.pin, sl.pin_cap, hipHostMallocDefault) != hipSuccess) {
            (void)hipFree(sl.dev);
            set_error("hipHostMalloc of %zu bytes failed", sl.pin_cap);
            return -ENOMEM;
        }
    }
    *out = sl;
    return 0;
}
void release_slab(mgx_pairhmm* c, Slab sl) {
    if (!sl.dev) return;
    if (c && c->free_slabs.size() < 16) { c->free_slabs.push_back(sl); return; }
    (void)hipFree(sl.dev);
    if (sl.pin) (void)hipHostFree(sl.pin);
}

using mgx::validate;

}  // namespace

extern "C" {

int mgx_pairhmm_table_f32(int which, const float** out) {
    const auto& t = mgx::tables<float>();
    if (which == 0) { *out = t.ph2pr.data(); return mgx::kPh2prSize; }
    if (which == 1) { *out = t.mm.data(); return mgx::kMmSize; }
    return -EINVAL;
}
int mgx_pairhmm_table_f64(int which, const double** out) {
    const auto& t = mgx::tables<double>();
    if (which == 0) { *out = t.ph2pr.data(); return mgx::kPh2prSize; }
    if (which == 1) { *out = t.mm.data(); return mgx::kMmSize; }
    return -EINVAL;
}

int mgx_pairhmm_create(int device, unsigned flags, mgx_pairhmm_t** out) {
    if (!out) { set_error("out is NULL"); return -EINVAL; }
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        set_error("no HIP device is visible (this library has no CPU fallback)");
        return -ENODEV;
    }
    if (device == -1) {                 // MGX_DEVICE_AUTO: contexts are dealt round-robin over the visible GPUs
        static std::atomic<unsigned> next{0};
        device = (int)(next.fetch_add(1) % (unsigned)n_dev);
    }
    if (device < 0 || device >= n_dev) { set_error("device %d out of range (0..%d)", device, n_dev - 1); return -EINVAL; }
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<mgx_pairhmm> c(new (std::nothrow) mgx_pairhmm);
    if (!c) return -ENOMEM;
    c->device = device;
    c->flags = flags;
    c->wire = (flags & MGX_PAIRHMM_WIRE) != 0;
    if (const char* e = getenv("MGX_PAIRHMM_WIRE")) { if (*e) c->wire = atoi(e) != 0; }      // A/B: read per context, not once per process
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount;
    {
        // optional CU partition (flags bits 8..15: an 8-bit pattern repeated over the CU index): lets a
        // VALU-bound PairHMM context and an HBM-bound sort context share one GPU side by side instead
        // of queueing behind each other (BASELINE.json configs[4])
        const unsigned pat = (flags >> 8) & 0xFFu;
        if (pat != 0 && pat != 0xFFu) {
            const int n_words = (c->n_cu + 31) / 32;
            std::vector<uint32_t> mask(n_words, 0);
            for (int cu = 0; cu < c->n_cu; ++cu) if ((pat >> (cu & 7)) & 1u) mask[cu >> 5] |= 1u << (cu & 31);
            HIP_TRY(hipExtStreamCreateWithCUMask(&c->compute, (uint32_t)n_words, mask.data()));
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking));
        }
    }
    HIP_TRY(hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->d2h, hipStreamNonBlocking));
    {
        const unsigned pat = (flags >> 8) & 0xFFu;
        const char* e = getenv("MGX_PAIRHMM_STREAMS");
        // default 1: measured on an MI355X (profiles/r02_pairhmm_streams_ab.txt) two streams gain 2 % on resident ragged
        // batches (4529 -> 4610 GCUPS) but lose 20 % for region batches through a 4-lane queue (3089 -> 2431: lanes x
        // streams oversubscribe the device); three and four streams lose everywhere (ragged 3865 / 3895)
        c->n_streams = e ? std::max(1, std::min(1 + mgx_pairhmm::kAux, atoi(e))) : 1;
        if (pat != 0 && pat != 0xFFu) c->n_streams = 1;          // a CU-masked context keeps to its masked stream
        for (int a = 0; a + 1 < c->n_streams; ++a) {
            HIP_TRY(hipStreamCreateWithFlags(&c->aux[a], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_join[a], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    }
    const auto& tf = mgx::tables<float>();
    const auto& td = mgx::tables<double>();
    int rc;
    if ((rc = upload(&c->d_ph2pr_f, tf.ph2pr.data(), tf.ph2pr.size() * 4, c->compute))) return rc;
    if ((rc = upload(&c->d_mm_f, tf.mm.data(), tf.mm.size() * 4, c->compute))) return rc;
    if ((rc = upload(&c->d_ph2pr_d, td.ph2pr.data(), td.ph2pr.size() * 8, c->compute))) return rc;
    if ((rc = upload(&c->d_mm_d, td.mm.data(), td.mm.size() * 8, c->compute))) return rc;
    if ((rc = upload(&c->d_div3_f, tf.ph2pr_div3.data(), tf.ph2pr_div3.size() * 4, c->compute))) return rc;
    if ((rc = upload(&c->d_ratio_f, tf.gap_ratio.data(), tf.gap_ratio.size() * 4, c->compute))) return rc;
    if ((rc = upload(&c->d_div3_d, td.ph2pr_div3.data(), td.ph2pr_div3.size() * 8, c->compute))) return rc;
    if ((rc = upload(&c->d_ratio_d, td.gap_ratio.data(), td.gap_ratio.size() * 8, c->compute))) return rc;
    c->log10_initial_f = tf.log10_initial;
    c->log10_initial_d = td.log10_initial;
    HIP_TRY(hipStreamSynchronize(c->compute));
    *out = c.release();
    return 0;
}

void mgx_pairhmm_destroy(mgx_pairhmm_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->ext.p && c->ext.free_fn) c->ext.free_fn(c->ext.p);
    (void)hipFree(c->d_ph2pr_f); (void)hipFree(c->d_mm_f);
    (void)hipFree(c->d_ph2pr_d); (void)hipFree(c->d_mm_d);
    (void)hipFree(c->d_div3_f); (void)hipFree(c->d_ratio_f); (void)hipFree(c->d_div3_d); (void)hipFree(c->d_ratio_d);
    for (auto& sl : c->free_slabs) { (void)hipFree(sl.dev); if (sl.pin) (void)hipHostFree(sl.pin); }
    (void)hipFree(c->d_strip);
    if (c->compute) (void)hipStreamDestroy(c->compute);
    if (c->copy) (void)hipStreamDestroy(c->copy);
    if (c->d2h) (void)hipStreamDestroy(c->d2h);
    for (int a = 0; a < mgx_pairhmm::kAux; ++a) { if (c->aux[a]) (void)hipStreamDestroy(c->aux[a]); if (c->ev_join[a]) (void)hipEventDestroy(c->ev_join[a]); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    delete c;
}

void mgx_pairhmm_batch_destroy(mgx_pairhmm_t* c, mgx_pairhmm_batch_t* b) {
    if (!b) return;
    if (c) {
        (void)hipSetDevice(c->device);
        // the slab goes back to the pool: nothing may still be reading or writing it.  Only THIS batch's
        // work is waited for (its last run, or its upload if it never ran; result downloads are
        // synchronous), so retiring one batch does not stall on the batches queued behind it.
        if (b->done) (void)hipEventSynchronize(b->done);
        else if (b->uploaded) (void)hipEventSynchronize(b->uploaded);
    }
    release_slab(c, b->slab);
    if (b->uploaded) (void)hipEventDestroy(b->uploaded);
    if (b->done) (void)hipEventDestroy(b->done);
    for (auto e : b->ev) (void)hipEventDestroy(e);
    delete b;
}

namespace {

// Where the arrays of a batch lie in its slab.  The inputs are written once (one H2D copy when staged through the
// pinned mirror), [out | used | keep] is read back with one D2H copy, what follows is device scratch.  The pair-list
// form writes its jobs on the host, first in the mirror; the cross-product form uploads the tables that the device
// enumerates them from and keeps the jobs in scratch.
struct SlabLayout {
    // sizes: set by the caller
    uint64_t n = 0, n_reads = 0, n_haps = 0, n_regions = 0, read_bytes = 0, hap_bytes = 0;
    bool cross = false, model = false;
    // offsets: set by lay_out_slab (the results' offsets go to the batch: o_out, o_used, o_keep)
    size_t rtab = 0, rreg = 0, rpre = 0, gtab = 0, htab = 0;      // cross-product form: what the jobs are enumerated from
    size_t jobs = 0, bases = 0, qual = 0, ins = 0, del = 0, gcp = 0, hap = 0;
    size_t mapq = 0, rlen = 0, roff = 0, rnh = 0;                 // with a read model: per read, for the model and the epilogue
    size_t rlist = 0, nlist = 0, rcount = 0;
    size_t pin_bytes = 0;                                         // the pinned mirror covers the inputs and the results only
    bool staged = true;
    // the wire form (pair-list batches of a context with MGX_PAIRHMM_WIRE): the uploaded prefix is [jobs | bases4 | qual |
    // ins | del | gcp | hap4] at these offsets, and bases ... hap above lie in device scratch
    bool wire = false;
    mgx::wire::Widths ww;
    size_t w_bases4 = 0, w_qual = 0, w_ins = 0, w_del = 0, w_gcp = 0, w_hap4 = 0;
};

// Decides the offsets, takes a slab of that size -- with a pinned mirror if always_stage or if inputs and results fit
// kStageLimit -- and points the batch into it.
int lay_out_slab(mgx_pairhmm* c, bool always_stage, SlabLayout* L, mgx_pairhmm_batch* b) {
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
    auto take_expanded = [&] {
        L->bases = take(L->read_bytes);
        L->qual = take(L->read_bytes);
        L->ins = take(L->read_bytes);
        L->del = take(L->read_bytes);
        L->gcp = take(L->read_bytes);
        L->hap = take(L->hap_bytes);
    };
    // the wire form is for batches that go through the pinned mirror: those the plain form would stage
    if (L->wire && (L->cross || (!always_stage && align_up(n * sizeof(Job)) + 5 * align_up(L->read_bytes) + align_up(L->hap_bytes) +
                                                       align_up(n * sizeof(double)) + align_up(n) > kStageLimit))) L->wire = false;
    if (L->wire) {
        namespace W = mgx::wire;
        L->w_bases4 = take(W::nibble_bytes(L->read_bytes));
        L->w_qual = take(W::stream_bytes(L->read_bytes, L->ww.qual));
        L->w_ins = take(W::stream_bytes(L->read_bytes, L->ww.ins));
        L->w_del = take(W::stream_bytes(L->read_bytes, L->ww.del));
        L->w_gcp = take(W::stream_bytes(L->read_bytes, L->ww.gcp));
        L->w_hap4 = take(W::nibble_bytes(L->hap_bytes));
    } else {
        take_expanded();
    }
    L->mapq = take(per_read);
    L->rlen = take(per_read * sizeof(uint64_t));
    L->roff = take(per_read * sizeof(uint32_t));
    L->rnh = take(per_read * sizeof(uint32_t));
    b->in_bytes = off;
    b->o_out = take(n * sizeof(double));
    b->o_used = take(n);
    b->o_keep = take(per_read);
    b->result_bytes = off - b->o_out;
    L->pin_bytes = off;
    if (L->cross) L->jobs = take(n * sizeof(Job));
    if (L->wire) take_expanded();                    // what pairhmm_expand_wire writes
    L->rlist = take(2 * n * sizeof(uint32_t));       // fp64 re-run lists | exact-tier list
    L->nlist = take(n * sizeof(uint32_t));           // N-haplotype lists of the four-code fp32 launches
    L->rcount = take(kCounters * sizeof(uint32_t));
    L->staged = always_stage || L->pin_bytes <= kStageLimit;
    if (const int rc = acquire_slab(c, off, L->staged ? L->pin_bytes : 0, &b->slab)) return rc;
    uint8_t* dv = b->slab.dev;
    b->read_bytes = L->read_bytes; b->hap_bytes = L->hap_bytes;
    b->d_jobs = (Job*)(dv + L->jobs);
    b->d_bases = dv + L->bases; b->d_qual = dv + L->qual; b->d_ins = dv + L->ins; b->d_del = dv + L->del;
    b->d_gcp = dv + L->gcp; b->d_hap = dv + L->hap;
    b->d_out = (double*)(dv + b->o_out); b->d_used = dv + b->o_used;
    b->d_rerun_list = (uint32_t*)(dv + L->rlist); b->d_rerun_count = (uint32_t*)(dv + L->rcount);
    b->d_nhap_list = (uint32_t*)(dv + L->nlist);
    if (L->model) {
        b->d_read_len = (uint64_t*)(dv + L->rlen); b->d_keep = dv + b->o_keep;
        b->d_row_off = (uint32_t*)(dv + L->roff); b->d_row_nh = (uint32_t*)(dv + L->rnh);
    }
    return 0;
}

// modifyReadQualities + gap continuation penalties as the device applies them (pairhmm_read_model)
ReadModel make_read_model(const mgx_read_model_t& model) {
    ReadModel rm{};
    rm.rate_factor = model.pcr_rate_factor; rm.bq_threshold = model.base_quality_threshold;
    rm.constant_gcp = model.constant_gcp;
    for (int i = 0; i <= 20; ++i) {      // PairHMMLikelihoodCalculationEngine.cpp:45-61
        const double d = 40.0 - std::exp((double)i / ((double)std::max(rm.rate_factor, 1) * M_PI));
        const int v = (d > 0.0 ? (int)(d + 0.5) : (int)(d - 0.5)) + 1;
        rm.pcr_cache[i] = (uint8_t)(char)std::max(10, v);
    }
    return rm;
}

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
    uint64_t reads_in[kBins] = {0}, rstart[kBins + 1] = {0}, jobs_in[kBins] = {0}, cells_in[kBins] = {0}, bytes_in[kBins] = {0};
};

// totals of the batch, and where every region's [reads][haps] block starts in the output
int cross_totals(uint32_t n_regions, const mgx_pairhmm_input_t* regs, CrossPlan* p, std::vector<uint64_t>* out_base) {
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
int cross_tables(uint32_t n_regions, const mgx_pairhmm_input_t* regs, const std::vector<uint64_t>& out_base, CrossPlan* p,
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
            shape_of((uint32_t)std::min<uint64_t>(Rl, 0xFFFFFFFFull), &G, &RPL);
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

// folds the small classes and sums, per class, reads, jobs, cells and bytes
void cross_bins(CrossPlan* p, uint64_t (&count)[kBins]) {
    int remap[kBins];
    merge_small_bins(count, remap);
    std::vector<uint64_t> sumH(p->regions.size(), 0);
    for (size_t g = 0; g < p->regions.size(); ++g)
        for (uint32_t h = 0; h < p->regions[g].n_haps; ++h) sumH[g] += p->haps[p->regions[g].hap_begin + h].len;
    for (CrossRead& ri : p->reads) {
        ri.bin = (uint8_t)remap[ri.bin];
        const RegionRef& R = p->regions[ri.region];
        p->reads_in[ri.bin]++; p->jobs_in[ri.bin] += R.n_haps; p->cells_in[ri.bin] += (uint64_t)ri.len * sumH[ri.region];
        p->bytes_in[ri.bin] += 5ull * ri.len * R.n_haps + sumH[ri.region] + 4ull * R.n_haps;
    }
    for (int k = 0; k < kBins; ++k) p->rstart[k + 1] = p->rstart[k] + p->reads_in[k];
}

// the enumeration tables and the sequences, into the pinned mirror
void cross_stage(const CrossPlan& p, uint32_t n_regions, const mgx_pairhmm_input_t* regs, const SlabLayout& L, uint8_t* pin) {
    SeqRef* rtab = (SeqRef*)(pin + L.rtab);
    uint32_t* rreg = (uint32_t*)(pin + L.rreg);
    uint32_t* rpre = (uint32_t*)(pin + L.rpre);
    uint64_t cur[kBins];
    for (int k = 0; k < kBins; ++k) cur[k] = p.rstart[k];
    for (uint64_t r = 0; r < p.nr; ++r) {          // read table in (class, input) order
        const CrossRead& ri = p.reads[r];
        const uint64_t at = cur[ri.bin]++;
        rtab[at] = SeqRef{ri.off, ri.len, (uint32_t)r};
        rreg[at] = ri.region;
    }
    uint32_t run = 0;
    for (uint64_t at = 0; at < p.nr; ++at) { rpre[at] = run; run += p.regions[rreg[at]].n_haps; }
    rpre[p.nr] = run;
    memcpy(pin + L.gtab, p.regions.data(), n_regions * sizeof(RegionRef));
    memcpy(pin + L.htab, p.haps.data(), p.nh * sizeof(SeqRef));
    size_t rb = 0, hb = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        const mgx_pairhmm_input_t& in = regs[g];
        if (in.n_reads) {
            const uint64_t o0 = in.read_off[0], len = in.read_off[in.n_reads] - o0;
            memcpy(pin + L.bases + rb, in.bases + o0, len); memcpy(pin + L.qual + rb, in.qual + o0, len);
            memcpy(pin + L.ins + rb, in.ins + o0, len);     memcpy(pin + L.del + rb, in.del + o0, len);
            memcpy(pin + L.gcp + rb, in.gcp + o0, len);
            rb += len;
        }
        if (in.n_haps) {
            const uint64_t o0 = in.hap_off[0], len = in.hap_off[in.n_haps] - o0;
            memcpy(pin + L.hap + hb, in.hap_bases + o0, len);
            hb += len;
        }
    }
}

// per read, in global read order: MAPQ, length, and its row of the output
int cross_stage_model(uint32_t n_regions, const mgx_pairhmm_input_t* regs, const uint8_t* const* mapq,
                      const std::vector<uint64_t>& out_base, const SlabLayout& L, uint8_t* pin) {
    uint64_t* rlen = (uint64_t*)(pin + L.rlen);
    uint32_t* roff = (uint32_t*)(pin + L.roff);
    uint32_t* rnh = (uint32_t*)(pin + L.rnh);
    uint64_t r_at = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        const mgx_pairhmm_input_t& in = regs[g];
        if (in.n_reads && !mapq[g]) { set_error("region %u: mapq is NULL", g); return -EINVAL; }
        for (uint64_t r = 0; r < in.n_reads; ++r) {
            rlen[r_at + r] = in.read_off[r + 1] - in.read_off[r];
            roff[r_at + r] = (uint32_t)(out_base[g] + r * in.n_haps);
            rnh[r_at + r] = (uint32_t)in.n_haps;
        }
        if (in.n_reads) memcpy(pin + L.mapq + r_at, mapq[g], in.n_reads);
        r_at += in.n_reads;
    }
    return 0;
}

int create_cross(mgx_pairhmm_t* c, uint32_t n_regions, const mgx_pairhmm_input_t* regs, mgx_pairhmm_batch* b,
                 std::vector<uint64_t>* out_base, const uint8_t* const* mapq = nullptr, const mgx_read_model_t* model = nullptr) {
    CrossPlan p;
    int rc;
    if ((rc = cross_totals(n_regions, regs, &p, out_base))) return rc;
    b->n_pairs = p.n;
    b->stats.n_pairs = p.n;
    if (p.n == 0) return 0;
    uint64_t count[kBins] = {0};
    if ((rc = cross_tables(n_regions, regs, *out_base, &p, count))) return rc;
    cross_bins(&p, count);
    SlabLayout L;
    L.n = p.n; L.n_reads = p.nr; L.n_haps = p.nh; L.n_regions = n_regions; L.read_bytes = p.read_bytes; L.hap_bytes = p.hap_bytes;
    L.cross = true; L.model = model != nullptr;
    if ((rc = lay_out_slab(c, true, &L, b))) return rc;
    uint8_t* dv = b->slab.dev; uint8_t* pin = b->slab.pin;
    cross_stage(p, n_regions, regs, L, pin);
    hipStream_t s = c->copy;
    if (model) {
        if ((rc = cross_stage_model(n_regions, regs, mapq, *out_base, L, pin))) return rc;
        b->has_model = true; b->n_reads = (uint32_t)p.nr;
        b->log10_rate = model->log10_mismapping_rate; b->max_err = model->max_error_per_base;
    }
    HIP_TRY(hipMemcpyAsync(dv, pin, b->in_bytes, hipMemcpyHostToDevice, s));
    if (model)      // modifyReadQualities + gap continuation penalties, in place on the uploaded arrays
        hipLaunchKernelGGL(pairhmm_read_model, dim3((uint32_t)p.nr), dim3(128), 0, s, (const SeqRef*)(dv + L.rtab),
                           b->d_bases, b->d_qual, b->d_ins, b->d_del, b->d_gcp, (const uint8_t*)(dv + L.mapq), make_read_model(*model));
    uint64_t job_begin = 0;
    for (int k = 0; k < kBins; ++k) {
        if (!p.reads_in[k]) continue;
        Bin bin;
        bin_shape(k, &bin);
        bin.job_begin = (uint32_t)job_begin;
        bin.job_count = (uint32_t)p.jobs_in[k];
        bin.max_h = p.max_h;
        bin.cells = p.cells_in[k];
        bin.alg_bytes = p.bytes_in[k];
        if ((rc = finalize_bin(bin, c->n_cu))) return rc;
        b->stats.cells += bin.cells; b->stats.alg_bytes += bin.alg_bytes;
        b->bins.push_back(bin);
        job_begin += bin.job_count;
    }
    // one enumeration launch for all bins: jobs are laid out in read-table order, which is bin order
    hipLaunchKernelGGL(pairhmm_make_jobs_multi, dim3((uint32_t)((p.n + 255) / 256)), dim3(256), 0, s, (const SeqRef*)(dv + L.rtab),
                       (const uint32_t*)(dv + L.rreg), (const uint32_t*)(dv + L.rpre), (uint32_t)p.nr, (const RegionRef*)(dv + L.gtab),
                       (const SeqRef*)(dv + L.htab), (uint32_t)p.n, b->d_jobs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventCreateWithFlags(&b->uploaded, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->uploaded, s));
    return 0;
}

// The six arrays of a pair-list batch in the wire form, straight from the caller's arrays into the pinned mirror
// (the gather and the bit-packing are one pass; the widths come from create_pairs' pre-pass).
void stage_wire(const mgx_pairhmm_input_t* in, const mgx::PackPlan* plan, const SlabLayout& L, uint8_t* pin) {
    namespace W = mgx::wire;
    if (plan || L.read_bytes + L.hap_bytes < (32u << 20)) {
        W::pack_arrays(in, plan, L.ww, pin + L.w_bases4, pin + L.w_qual, pin + L.w_ins, pin + L.w_del, pin + L.w_gcp, pin + L.w_hap4);
        return;
    }
    // a large one-shot batch: one thread per array, as the plain form stages it
    std::thread th[6];
    th[0] = std::thread([=] { W::pack_nibbles(in, plan, true, pin + L.w_bases4); });
    th[1] = std::thread([=] { W::pack_stream(in, plan, in->qual, L.ww.qual, pin + L.w_qual); });
    th[2] = std::thread([=] { W::pack_stream(in, plan, in->ins, L.ww.ins, pin + L.w_ins); });
    th[3] = std::thread([=] { W::pack_stream(in, plan, in->del, L.ww.del, pin + L.w_del); });
    th[4] = std::thread([=] { if (L.ww.gcp) W::pack_stream(in, plan, in->gcp, L.ww.gcp, pin + L.w_gcp); });
    th[5] = std::thread([=] { W::pack_nibbles(in, plan, false, pin + L.w_hap4); });
    for (auto& t : th) t.join();
}

// pairhmm_expand_wire behind the copy, on the same stream: d_bases ... d_hap are whole before `uploaded` is recorded
int launch_expand_wire(hipStream_t s, const SlabLayout& L, mgx_pairhmm_batch* b) {
    ExpandWireArgs a{};
    const size_t src[6] = {L.w_bases4, L.w_qual, L.w_ins, L.w_del, L.w_gcp, L.w_hap4};
    uint8_t* const dst[6] = {b->d_bases, b->d_qual, b->d_ins, b->d_del, b->d_gcp, b->d_hap};
    const uint32_t w[6] = {4, L.ww.qual, L.ww.ins, L.ww.del, L.ww.gcp, 4};
    uint64_t blocks = 0;
    for (int k = 0; k < 6; ++k) {
        a.src[k] = b->slab.dev + src[k]; a.dst[k] = dst[k]; a.w[k] = w[k];
        a.n[k] = k == 5 ? L.hap_bytes : L.read_bytes;
        a.block_first[k] = (uint32_t)blocks;
        blocks += ((a.n[k] + 7) / 8 + kExpandBlock - 1) / kExpandBlock;
        if (blocks > 0x7FFFFFFFull) { set_error("batch too large for one expansion launch"); return -E2BIG; }
    }
    a.block_first[6] = (uint32_t)blocks;
    a.fill = L.ww.gcp_const;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(pairhmm_expand_wire, dim3((uint32_t)blocks), dim3(kExpandBlock), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Upload of a pair-list batch: one copy out of the pinned mirror, or (very large batches) one per array.
int upload_pairs(mgx_pairhmm_t* c, const mgx_pairhmm_input_t* in, const mgx::PackPlan* plan, const SlabLayout& L, const Job* jobs,
                 mgx_pairhmm_batch* b) {
    const uint64_t read_bytes = L.read_bytes, hap_bytes = L.hap_bytes;
    uint8_t* dv = b->slab.dev;
    hipStream_t s = c->copy;
    if (L.wire) {
        stage_wire(in, plan, L, b->slab.pin);
        HIP_TRY(hipMemcpyAsync(dv, b->slab.pin, b->in_bytes, hipMemcpyHostToDevice, s));
        if (const int rc = launch_expand_wire(s, L, b)) return rc;
    } else if (L.staged) {
        uint8_t* pin = b->slab.pin;
        if (plan) {
            mgx::pack_copy(in, *plan, pin + L.bases, pin + L.qual, pin + L.ins, pin + L.del, pin + L.gcp, pin + L.hap);
        } else if (read_bytes + hap_bytes < (32u << 20)) {
            memcpy(pin + L.bases, in->bases, read_bytes); memcpy(pin + L.qual, in->qual, read_bytes);
            memcpy(pin + L.ins, in->ins, read_bytes);     memcpy(pin + L.del, in->del, read_bytes);
            memcpy(pin + L.gcp, in->gcp, read_bytes);     memcpy(pin + L.hap, in->hap_bases, hap_bytes);
        } else {
            // a large one-shot batch: the six arrays are staged by six threads (one core copies ~10 GB/s)
            const void* src[6] = {in->bases, in->qual, in->ins, in->del, in->gcp, in->hap_bases};
            uint8_t* dst[6] = {pin + L.bases, pin + L.qual, pin + L.ins, pin + L.del, pin + L.gcp, pin + L.hap};
            const size_t len[6] = {(size_t)read_bytes, (size_t)read_bytes, (size_t)read_bytes, (size_t)read_bytes, (size_t)read_bytes, (size_t)hap_bytes};
            std::thread th[6];
            for (int k = 0; k < 6; ++k) th[k] = std::thread([=] { memcpy(dst[k], src[k], len[k]); });
            for (auto& t : th) t.join();
        }
        HIP_TRY(hipMemcpyAsync(dv, pin, b->in_bytes, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(hipMemcpyAsync(b->d_jobs, jobs, L.n * sizeof(Job), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->d_bases, in->bases, read_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->d_qual, in->qual, read_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->d_ins, in->ins, read_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->d_del, in->del, read_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->d_gcp, in->gcp, read_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->d_hap, in->hap_bases, hap_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));          // the caller's buffers may go away after we return
        b->host_jobs.clear(); b->host_jobs.shrink_to_fit();
    }
    HIP_TRY(hipEventCreateWithFlags(&b->uploaded, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->uploaded, s));       // batch_run makes the compute stream wait on this
    return 0;
}

// Pair-list batch.  plan == nullptr: the test cases of `in` with its read / haplotype arrays copied as
// they are.  plan != nullptr: test cases [plan->lo, plan->hi) of `in`, only the sequences they reference
// (gathered by the packer, pairhmm_pack.h) -- the form the host work queue uploads.
int create_pairs(mgx_pairhmm_t* c, const mgx_pairhmm_input_t* in, const mgx::PackPlan* plan, mgx_pairhmm_batch* b) {
    const uint64_t n = plan ? plan->hi - plan->lo : in->n_pairs;
    const uint32_t* pr = plan ? plan->pair_read.data() : in->pair_read;
    const uint32_t* ph = plan ? plan->pair_hap.data() : in->pair_hap;
    const uint64_t* roff = plan ? plan->roff.data() : in->read_off;
    const uint64_t* hoff = plan ? plan->hoff.data() : in->hap_off;
    const uint64_t n_reads = plan ? plan->lread.size() : in->n_reads, n_haps = plan ? plan->lhap.size() : in->n_haps;
    int rc;
    b->n_pairs = n;
    b->stats.n_pairs = n;

    // ---- bin by (G, RPL), then counting-sort every bin by haplotype length -------------
    std::vector<uint32_t> bin_of(n);
    uint64_t count[kBins] = {0};
    uint32_t max_h = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t r = pr[i], h = ph[i];
        if (r >= n_reads || h >= n_haps) { set_error("test case %llu: index out of range", (unsigned long long)i); return -EINVAL; }
        const uint64_t R = roff[r + 1] - roff[r];
        const uint64_t H = hoff[h + 1] - hoff[h];
        if (R == 0 || H == 0) { set_error("test case %llu: empty read or haplotype", (unsigned long long)i); return -EINVAL; }
        int G, RPL;
        shape_of((uint32_t)std::min<uint64_t>(R, 0xFFFFFFFFull), &G, &RPL);
        if (G == 0) { set_error("test case %llu: read of %llu bases exceeds the %d-row limit", (unsigned long long)i, (unsigned long long)R, kMaxRowsStrip); return -E2BIG; }
        if (H > 0x7FFFFFF0ull) { set_error("haplotype too long"); return -E2BIG; }
        const int bi = bin_index(G, RPL);
        bin_of[i] = (uint32_t)bi;
        count[bi]++;
        max_h = std::max<uint32_t>(max_h, (uint32_t)H);
        b->stats.cells += R * H;
        b->stats.alg_bytes += 5 * R + H + 4;
    }
    // A bin with few jobs is folded into the next larger row class of the same group width (any
    // RPL >= ceil(R/G) is valid, it only leaves lanes unused): a region-sized batch then needs one
    // fp32 + one fp64 launch instead of one pair per read-length class.
    {
        int remap[kBins];
        merge_small_bins(count, remap);
        for (uint64_t i = 0; i < n; ++i) bin_of[i] = (uint32_t)remap[bin_of[i]];
    }
    // ---- one slab for everything; layout decided before the jobs are written so that they can be
    //      built directly in the pinned mirror
    SlabLayout L;
    L.n = n; L.n_reads = n_reads; L.n_haps = n_haps; L.read_bytes = roff[n_reads]; L.hap_bytes = hoff[n_haps];
    if (c->wire) { L.wire = true; L.ww = mgx::wire::scan_widths(in, plan); }      // the widths decide the layout
    if ((rc = lay_out_slab(c, plan != nullptr, &L, b))) return rc;
    if (!L.staged) b->host_jobs.resize(n);
    Job* jobs = L.staged ? (Job*)(b->slab.pin + L.jobs) : b->host_jobs.data();
    {
        // key = (bin, H descending): counting sort on H inside each bin keeps the wavefront's groups
        // (consecutive jobs) at near-equal step counts, and longest first means the last workgroups of a
        // launch -- its drain -- are the shortest jobs.
        std::vector<uint64_t> bin_start(kBins + 1, 0);
        for (int k = 0; k < kBins; ++k) bin_start[k + 1] = bin_start[k] + count[k];
        std::vector<std::vector<uint32_t>> hist(kBins);
        for (int k = 0; k < kBins; ++k) if (count[k]) hist[k].assign((size_t)max_h + 2, 0);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t h = ph[i];
            const uint32_t H = (uint32_t)(hoff[h + 1] - hoff[h]);
            hist[bin_of[i]][(max_h - H) + 1]++;
        }
        for (int k = 0; k < kBins; ++k)
            for (size_t x = 1; x < hist[k].size(); ++x) hist[k][x] += hist[k][x - 1];
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t r = pr[i], h = ph[i];
            const uint32_t R = (uint32_t)(roff[r + 1] - roff[r]);
            const uint32_t H = (uint32_t)(hoff[h + 1] - hoff[h]);
            const int k = (int)bin_of[i];
            Job& jb = jobs[bin_start[k] + hist[k][max_h - H]++];
            jb.read_off = roff[r]; jb.hap_off = hoff[h];
            jb.R = R; jb.H = H; jb.pair = (uint32_t)i; jb.pad_ = 0;
        }
        for (int k = 0; k < kBins; ++k) {
            if (!count[k]) continue;
            Bin bin;
            bin_shape(k, &bin);
            bin.job_begin = (uint32_t)bin_start[k];
            bin.job_count = (uint32_t)count[k];
            for (uint64_t q = bin_start[k]; q < bin_start[k + 1]; ++q) {
                bin.max_h = std::max(bin.max_h, jobs[q].H);
                bin.cells += (uint64_t)jobs[q].R * jobs[q].H;
                bin.alg_bytes += 5ull * jobs[q].R + jobs[q].H + 4;
            }
            if ((rc = finalize_bin(bin, c->n_cu))) return rc;
            b->bins.push_back(bin);
        }
    }
    return upload_pairs(c, in, plan, L, jobs, b);
}

}  // namespace

int mgx_pairhmm_batch_create(mgx_pairhmm_t* c, const mgx_pairhmm_input_t* in,
                             mgx_pairhmm_batch_t** out) {
    if (!c || !out) { set_error("ctx/out is NULL"); return -EINVAL; }
    *out = nullptr;
    int rc = validate(in);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    BatchPtr b = new_batch();
    if (!b) return -ENOMEM;
    std::vector<uint64_t> base;
    if (!in->pair_read && !in->pair_hap && in->n_reads && in->n_haps) rc = create_cross(c, 1, in, b.get(), &base);   // cross-product form: one region
    else rc = create_pairs(c, in, nullptr, b.get());
    if (rc) return rc;
    *out = b.release();
    return 0;
}

namespace {

constexpr int kSharedCount = 63;      // counter slot of the narrow classes' shared fp64 re-run list
constexpr int kExactCount = 62;       // ... and of the exact tier's list (second half of d_rerun_list)

// Re-runs in double precision: the "narrow" classes (at most 16 lanes x 8 rows: every read up to 128 bases) append
// to ONE list (their jobs are a prefix of the job array) that ONE fp64 launch of the 16 x RPLd shape processes --
// a test case's value does not depend on the shape that computes it; wider classes keep a list and a launch each.
inline bool is_narrow(const Bin& bn) { return bn.G <= 16 && bn.G * bn.RPL <= 16 * kNarrowMaxRPL; }

// what the steps of one mgx_pairhmm_batch_run share
struct Run {
    mgx_pairhmm* c = nullptr;
    mgx_pairhmm_batch* b = nullptr;
    hipStream_t s = nullptr;                   // the compute stream
    bool timing = false, force_f64 = false;
    hipEvent_t* ev = nullptr;                  // this run's event set (timing only)
    int n_str = 1;                             // streams the classes are dealt to
    KernelArgs base{};                         // the arguments every launch starts from
    std::vector<char> in_multi;                // classes that a multi-class launch has computed
    size_t first_narrow = 0;                   // books the shared fp64 launch; bins.size() if there is no narrow class
    uint32_t n_narrow_jobs = 0, narrow_max_h = 0, narrow_rows = 0;
};

// boundary rows of the strip-mined class and of the exact tier: one array per context, grown on demand
int ensure_strip_scratch(mgx_pairhmm* c, size_t bytes) {
    if (bytes <= c->strip_cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->compute));           // an earlier launch may still be using the old array
    (void)hipFree(c->d_strip); c->d_strip = nullptr; c->strip_cap = 0;
    HIP_TRY(hipMalloc(&c->d_strip, bytes));
    c->strip_cap = bytes;
    return 0;
}

// this run's event set out of the batch's ring
int pick_event_set(Run& r) {
    mgx_pairhmm_batch* b = r.b;
    if (!r.timing) return 0;
    if (b->ev.empty()) {                   // whichever entry point made the batch: allocated on first use
        const size_t per = b->bins.size() * 4;
        b->ev_sets = (uint32_t)std::max<size_t>(1, std::min<size_t>(kMaxEventSets, 1024 / per));
        b->ev.resize(per * b->ev_sets);
        for (auto& e : b->ev) HIP_TRY(hipEventCreate(&e));
    }
    r.ev = b->ev.data() + (size_t)(b->runs_timed % b->ev_sets) * b->bins.size() * 4;
    return 0;
}

// the compute stream waits for the upload, the counters and flags are cleared, the side streams fork
int begin_run(Run& r) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    if (b->uploaded) HIP_TRY(hipStreamWaitEvent(r.s, b->uploaded, 0));
    HIP_TRY(hipMemsetAsync(b->d_rerun_count, 0, kCounters * sizeof(uint32_t), r.s));
    HIP_TRY(hipMemsetAsync(b->d_used, 0, b->n_pairs, r.s));
    r.n_str = (int)std::min<size_t>((size_t)c->n_streams, b->bins.size());
    if (r.n_str > 1) {
        HIP_TRY(hipEventRecord(c->ev_fork, r.s));
        for (int q = 0; q + 1 < r.n_str; ++q) HIP_TRY(hipStreamWaitEvent(c->aux[q], c->ev_fork, 0));
    }
    KernelArgs& base = r.base;
    base.jobs = b->d_jobs;
    base.bases = b->d_bases; base.qual = b->d_qual; base.ins = b->d_ins; base.del = b->d_del;
    base.gcp = b->d_gcp; base.hap_bases = b->d_hap;
    base.out_log10 = b->d_out; base.used_f64 = b->d_used;
    base.nhap_list = b->d_nhap_list; base.nhap_count = b->d_rerun_count + kNhapCount;
    base.log10_initial_f = c->log10_initial_f;
    base.log10_initial_d = c->log10_initial_d;
    return 0;
}

// extent of the narrow classes: what the shared fp64 launch has to cover
void survey_narrow(Run& r) {
    const std::vector<Bin>& bins = r.b->bins;
    r.first_narrow = bins.size();
    for (size_t k = 0; k < bins.size(); ++k) {
        const Bin& bn = bins[k];
        if (!is_narrow(bn)) continue;
        if (r.first_narrow == bins.size()) r.first_narrow = k;
        r.n_narrow_jobs = std::max(r.n_narrow_jobs, bn.job_begin + bn.job_count);
        r.narrow_max_h = std::max(r.narrow_max_h, bn.max_h);
        r.narrow_rows = std::max(r.narrow_rows, (uint32_t)(bn.G * bn.RPL));
    }
}

// an fp64 launch over a job list or a class; what it leaves near the flush-to-zero threshold goes to the exact tier's list
int launch_f64(const Run& r, KernelArgs a, int Gd, int RPLd, uint32_t grid, uint32_t block, uint32_t lds, hipStream_t sk) {
    const mgx_pairhmm* c = r.c;
    a.ph2pr = c->d_ph2pr_d; a.mm = c->d_mm_d; a.ph2pr_div3 = c->d_div3_d; a.gap_ratio = c->d_ratio_d;
    a.rerun_list = r.b->d_rerun_list + r.b->n_pairs; a.rerun_count = r.b->d_rerun_count + kExactCount;      // job_list / n_dyn are set: the fp64 tier appends here
    KernelFn f = a.strip_scratch ? (KernelFn)pairhmm_fwd_strip<double> : pick_kernel<double>(Gd, RPLd);
    if (!f) { set_error("no fp64 kernel for G=%d RPL=%d", Gd, RPLd); return -ENOSYS; }
    hipLaunchKernelGGL(f, dim3(grid), dim3(block), lds, sk, a);
    return 0;
}

// one multi-class launch over the classes `set` (lane-width set gset), booked on the member with the most cells
int launch_multi(Run& r, int gset, std::vector<size_t>& set) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    // most rows per lane first (the costliest workgroups), wider groups first among equals
    std::stable_sort(set.begin(), set.end(), [&](size_t x, size_t y) {
        const Bin &bx = b->bins[x], &by = b->bins[y];
        return bx.RPL != by.RPL ? bx.RPL > by.RPL : bx.G > by.G;
    });
    MultiArgs m{};
    m.a = r.base;
    m.a.rerun_list = b->d_rerun_list; m.a.rerun_count = b->d_rerun_count + kSharedCount;
    m.a.job_list = nullptr; m.a.n_dyn = nullptr;
    m.a.ph2pr = c->d_ph2pr_f; m.a.mm = c->d_mm_f; m.a.ph2pr_div3 = c->d_div3_f; m.a.gap_ratio = c->d_ratio_f;
    m.n_bins = (uint32_t)set.size();
    uint32_t blocks = 0, lds = 0;
    size_t book = set[0];
    uint64_t cells = 0, bytes = 0;
    for (size_t q = 0; q < set.size(); ++q) {
        const Bin& bn = b->bins[set[q]];
        m.block_first[q] = blocks; blocks += bn.grid_f32;
        m.job_first[q] = bn.job_begin; m.job_count[q] = bn.job_count; m.lds_stride[q] = bn.lds_stride;
        m.G[q] = (uint8_t)bn.G; m.RPL[q] = (uint8_t)bn.RPL; m.bin[q] = (uint8_t)set[q];
        lds = std::max(lds, lds_bytes(bn, true, 4));
        if (bn.cells > b->bins[book].cells) book = set[q];
        cells += bn.cells; bytes += bn.alg_bytes;
        r.in_multi[set[q]] = 1;
        b->acct_cells[set[q]] = 0; b->acct_bytes[set[q]] = 0;
    }
    m.block_first[set.size()] = blocks;
    b->acct_cells[book] = cells; b->acct_bytes[book] = bytes; b->acct_multi[book] = (int8_t)(1 + gset);
    if (r.timing) for (size_t q : set) if (q != book) { HIP_TRY(hipEventRecord(r.ev[4 * q + 0], r.s)); HIP_TRY(hipEventRecord(r.ev[4 * q + 1], r.s)); }
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * book + 0], r.s));
    if (gset == 0) hipLaunchKernelGGL(pairhmm_fwd_multi<0>, dim3(blocks), dim3(64), lds, r.s, m);
    else           hipLaunchKernelGGL(pairhmm_fwd_multi<1>, dim3(blocks), dim3(64), lds, r.s, m);
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * book + 1], r.s));
    return 0;
}

// Several narrow classes: one multi-class launch per lane-width set instead of one launch per class.
// Only SMALL classes share a launch: measured on an MI355X (profiles/r02_pairhmm_multi_ab.txt) the common launch
// costs every class the register budget of the hungriest one (131-149 VGPRs: 3 wavefronts per SIMD; 4 when forced,
// with spills), which outweighs the saved drains for classes that fill the device on their own (ragged 1 M test
// cases, nine classes of ~29 000 workgroups: 4462 -> 4343 GCUPS) but not for classes of a few thousand workgroups
// (reads of 20-32 bases: 2764 -> 3009; region-sized batches).  MGX_PAIRHMM_MULTI=0 keeps the per-class launches; any
// other value is the default.  (The same build forced to 4 wavefronts per SIMD, and sharing a launch among all narrow
// classes whatever their size, were measured too and lost: DESIGN.md 3.5.)
int launch_multi_classes(Run& r) {
    mgx_pairhmm_batch* b = r.b;
    static const bool multi_ok = [] { const char* e = getenv("MGX_PAIRHMM_MULTI"); return !e || atoi(e) != 0; }();
    const uint32_t multi_below = (uint32_t)r.c->n_cu * 64u;     // workgroups; ~5 device fills
    r.in_multi.assign(b->bins.size(), 0);
    b->acct_cells.assign(b->bins.size(), 0); b->acct_bytes.assign(b->bins.size(), 0); b->acct_multi.assign(b->bins.size(), 0);
    for (size_t k = 0; k < b->bins.size(); ++k) { b->acct_cells[k] = b->bins[k].cells; b->acct_bytes[k] = b->bins[k].alg_bytes; }
    if (!multi_ok || r.force_f64) return 0;
    for (int gset = 0; gset < 2; ++gset) {
        std::vector<size_t> set;
        for (size_t k = 0; k < b->bins.size(); ++k) {
            const Bin& bn = b->bins[k];
            if (is_narrow(bn) && bn.RPL <= kNarrowMaxRPL && bn.block == 64 && bn.grid_f32 < multi_below && (gset == 0 ? bn.G == 16 : bn.G < 16)) set.push_back(k);
        }
        if (set.size() < 2 || set.size() > (size_t)kMultiBins) continue;
        if (const int rc = launch_multi(r, gset, set)) return rc;
    }
    return 0;
}

// class k on stream sk: its fp32 launch unless a multi-class launch has done it, then the fp64 re-run of its own list
// (the narrow classes share one, launch_shared_f64)
int launch_class(Run& r, size_t k, hipStream_t sk) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    hipEvent_t* ev = r.ev;
    const Bin& bin = b->bins[k];
    const bool shared = is_narrow(bin) && !r.force_f64;
    KernelArgs a = r.base;
    if (bin.strip) {
        a.strip_stride = (bin.max_h + 63u) & ~63u;
        if (const int rc = ensure_strip_scratch(c, (size_t)bin.grid_f32 * 6u * a.strip_stride * sizeof(double))) return rc;
        a.strip_scratch = c->d_strip;
    }
    a.rerun_list = shared ? b->d_rerun_list : b->d_rerun_list + bin.job_begin;
    a.rerun_count = b->d_rerun_count + (shared ? kSharedCount : (int)k);
    a.lds_stride = bin.lds_stride;
    a.job_first = bin.job_begin;
    a.nhap_list = b->d_nhap_list + bin.job_begin;
    a.nhap_count = b->d_rerun_count + kNhapCount + (int)k;
    if (!r.force_f64) {
        // four code columns first (the strip-mined class: five), then the class's N-haplotype list with five; both
        // append their underflows to the same fp64 list.  A multi-class launch has done the first of the two.
        a.ph2pr = c->d_ph2pr_f; a.mm = c->d_mm_f; a.ph2pr_div3 = c->d_div3_f; a.gap_ratio = c->d_ratio_f;
        const bool first = !r.in_multi[k];
        if (first) {
            a.job_list = nullptr; a.n_dyn = nullptr; a.n_static = bin.job_count;
            KernelFn f = bin.strip ? (KernelFn)pairhmm_fwd_strip<float> : pick_kernel<float, 4>(bin.G, bin.RPL);
            if (!f) { set_error("no fp32 kernel for G=%d RPL=%d", bin.G, bin.RPL); return -ENOSYS; }
            if (r.timing) HIP_TRY(hipEventRecord(ev[4 * k + 0], sk));
            hipLaunchKernelGGL(f, dim3(bin.grid_f32), dim3(bin.block), lds_bytes(bin, true, bin.strip ? kMaxCodes : 4), sk, a);
        }
        if (!bin.strip) {
            KernelFn f5 = pick_kernel<float, kMaxCodes>(bin.G, bin.RPL);
            if (!f5) { set_error("no fp32 kernel for G=%d RPL=%d", bin.G, bin.RPL); return -ENOSYS; }
            a.job_list = a.nhap_list; a.n_dyn = a.nhap_count; a.n_static = 0;
            hipLaunchKernelGGL(f5, dim3(bin.grid_nhap), dim3(bin.block), lds_bytes(bin, true, kMaxCodes), sk, a);
        }
        if (r.timing && first) HIP_TRY(hipEventRecord(ev[4 * k + 1], sk));
    }
    const bool books_shared = shared && k == r.first_narrow;      // the shared launch is booked on the first narrow class
    if (r.timing && !books_shared) HIP_TRY(hipEventRecord(ev[4 * k + 2], sk));
    if (!shared) {
        if (r.force_f64) { a.job_list = nullptr; a.n_dyn = nullptr; a.n_static = bin.job_count; }
        else { a.job_list = a.rerun_list; a.n_dyn = a.rerun_count; a.n_static = 0; }
        const int rc = launch_f64(r, a, bin.Gd, bin.RPLd, r.force_f64 ? bin.grid_f64_all : bin.grid_f64, bin.block, lds_bytes(bin, false), sk);
        if (rc) return rc;
    }
    if (r.timing && !books_shared) HIP_TRY(hipEventRecord(ev[4 * k + 3], sk));
    return 0;
}

// largest class first, classes dealt round-robin to the compute stream and the side streams, which then join it
int launch_classes(Run& r) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    std::vector<size_t> order(b->bins.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return b->bins[x].cells > b->bins[y].cells; });
    for (size_t at = 0; at < order.size(); ++at) {
        hipStream_t sk = (int)(at % (size_t)r.n_str) == 0 ? r.s : c->aux[at % (size_t)r.n_str - 1];
        if (r.in_multi[order[at]]) sk = r.s;      // its five-code launch follows the multi-class launch, which ran there
        if (const int rc = launch_class(r, order[at], sk)) return rc;
    }
    for (int q = 0; q + 1 < r.n_str; ++q) {
        HIP_TRY(hipEventRecord(c->ev_join[q], c->aux[q]));
        HIP_TRY(hipStreamWaitEvent(r.s, c->ev_join[q], 0));
    }
    return 0;
}

// the narrow classes' shared re-run list in one fp64 launch
int launch_shared_f64(Run& r) {
    if (!r.n_narrow_jobs || r.force_f64) return 0;
    KernelArgs a = r.base;
    a.job_list = r.b->d_rerun_list; a.n_dyn = r.b->d_rerun_count + kSharedCount; a.n_static = 0; a.job_first = 0;
    a.lds_stride = (r.narrow_max_h + 2u * 16u + 8u + 15u) & ~15u;
    const int RPLd = (int)((r.narrow_rows + 15) / 16);
    const uint32_t grid = std::min<uint32_t>((r.n_narrow_jobs + 3) / 4, (uint32_t)r.c->n_cu * 8u);
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * r.first_narrow + 2], r.s));
    if (const int rc = launch_f64(r, a, 16, RPLd, grid, 64, 4u * a.lds_stride, r.s)) return rc;
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * r.first_narrow + 3], r.s));
    return 0;
}

// The exact tier: whatever the fp64 launches left within reach of the flush-to-zero threshold (next to nothing
// on real data: log10 likelihoods below about -587), one test case per wavefront, the reference's operation order.
int launch_exact(Run& r) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    uint32_t max_h = 0;
    for (const Bin& bn : b->bins) max_h = std::max(max_h, bn.max_h);
    KernelArgs a = r.base;
    a.ph2pr = c->d_ph2pr_d; a.mm = c->d_mm_d; a.ph2pr_div3 = c->d_div3_d; a.gap_ratio = c->d_ratio_d;
    a.job_list = b->d_rerun_list + b->n_pairs; a.n_dyn = b->d_rerun_count + kExactCount; a.n_static = 0; a.job_first = 0;
    a.rerun_list = nullptr; a.rerun_count = nullptr;
    a.lds_stride = (max_h + 2u * 64u + 8u + 15u) & ~15u;
    a.strip_stride = (max_h + 63u) & ~63u;
    const size_t per_wg = 6u * (size_t)a.strip_stride * sizeof(double);
    const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)b->n_pairs, (size_t)c->n_cu * 2u, (size_t)(256u << 20) / per_wg}));
    if (const int rc = ensure_strip_scratch(c, (size_t)grid * per_wg)) return rc;
    a.strip_scratch = c->d_strip;
    hipLaunchKernelGGL(pairhmm_fwd_exact, dim3(grid), dim3(64), a.lds_stride, r.s, a);
    return 0;
}

// whole-region batches: normalise / filter every read's row of the output
void launch_epilogue(Run& r) {
    const mgx_pairhmm_batch* b = r.b;
    if (!b->has_model) return;
    hipLaunchKernelGGL(pairhmm_normalize_filter_rows, dim3((b->n_reads + 3) / 4), dim3(256), 0, r.s, b->d_out, b->d_read_len,
                       b->d_row_off, b->d_row_nh, b->n_reads, b->log10_rate, b->max_err, b->d_keep);
}

}  // namespace

int mgx_pairhmm_batch_run(mgx_pairhmm_t* c, mgx_pairhmm_batch_t* b) {
    if (!c || !b) { set_error("ctx/batch is NULL"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (b->n_pairs == 0) { b->ran = true; return 0; }
    Run r;
    r.c = c; r.b = b; r.s = c->compute;
    r.timing = (c->flags & MGX_PAIRHMM_TIMING) != 0 && !b->bins.empty();
    r.force_f64 = (c->flags & MGX_PAIRHMM_FORCE_DOUBLE) != 0;
    int rc;
    if ((rc = pick_event_set(r))) return rc;
    if ((rc = begin_run(r))) return rc;
    survey_narrow(r);
    if ((rc = launch_multi_classes(r))) return rc;
    if ((rc = launch_classes(r))) return rc;
    if ((rc = launch_shared_f64(r))) return rc;
    if ((rc = launch_exact(r))) return rc;
    launch_epilogue(r);
    HIP_TRY(hipGetLastError());
    if (r.timing) b->runs_timed++;
    if (!b->done) HIP_TRY(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->done, r.s));
    b->ran = true;
    return 0;
}

int mgx_pairhmm_batch_read_inputs(mgx_pairhmm_t* c, mgx_pairhmm_batch_t* b, uint8_t* bases, uint8_t* qual, uint8_t* ins,
                                  uint8_t* del, uint8_t* gcp, uint8_t* hap) {
    if (!c || !b) { set_error("ctx/batch is NULL"); return -EINVAL; }
    if ((b->read_bytes && (!bases || !qual || !ins || !del || !gcp)) || (b->hap_bytes && !hap)) { set_error("NULL argument"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (b->n_pairs == 0) return 0;
    if (b->uploaded) HIP_TRY(hipEventSynchronize(b->uploaded));      // the copy and, in the wire form, the expansion behind it
    uint8_t* const host[6] = {bases, qual, ins, del, gcp, hap};
    const uint8_t* const dev[6] = {b->d_bases, b->d_qual, b->d_ins, b->d_del, b->d_gcp, b->d_hap};
    for (int k = 0; k < 6; ++k) {
        const uint64_t len = k == 5 ? b->hap_bytes : b->read_bytes;
        if (len) HIP_TRY(hipMemcpy(host[k], dev[k], len, hipMemcpyDeviceToHost));
    }
    return 0;
}

int mgx_pairhmm_sync(mgx_pairhmm_t* c) {
    if (!c) { set_error("ctx is NULL"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->compute));
    return 0;
}

int mgx_pairhmm_batch_stats(mgx_pairhmm_t* c, mgx_pairhmm_batch_t* b, mgx_pairhmm_stats_t* out) {
    if (!c || !b || !out) { set_error("NULL argument"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->compute));
    mgx_pairhmm_stats_t st = b->stats;
    const bool force_f64 = (c->flags & MGX_PAIRHMM_FORCE_DOUBLE) != 0;
    st.n_launches_f32 = force_f64 ? 0 : (uint32_t)b->bins.size();
    st.n_launches_f64 = (uint32_t)b->bins.size();
    st.n_rerun_f64 = 0;
    st.n_nhap_f32 = 0;
    if (b->ran && b->n_pairs) {
        std::vector<uint32_t> cnt(kCounters);
        HIP_TRY(hipMemcpy(cnt.data(), b->d_rerun_count, kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < b->bins.size(); ++k) st.n_nhap_f32 += cnt[kNhapCount + k];
        for (size_t k = 0; k < b->bins.size(); ++k) st.n_rerun_f64 += force_f64 ? b->bins[k].job_count : cnt[k];
        if (!force_f64) st.n_rerun_f64 += cnt[63];          // the narrow classes' shared list
        st.n_exact = cnt[62];
    }
    st.ms_f32 = st.ms_f64 = st.ms_f32_dominant = 0;
    st.dominant_cells = st.dominant_alg_bytes = 0;
    st.dominant_kernel[0] = 0;
    st.n_runs_timed = 0;
    if ((c->flags & MGX_PAIRHMM_TIMING) && b->ran && !b->ev.empty() && b->runs_timed) {
        // mean over the runs recorded since the previous call (the ring keeps the last ev_sets of them)
        const uint32_t n_sets = std::min(b->runs_timed, b->ev_sets);
        const bool acct = b->acct_cells.size() == b->bins.size();
        auto cells_of = [&](size_t k) { return acct ? b->acct_cells[k] : b->bins[k].cells; };
        size_t dom = 0;
        for (size_t k = 0; k < b->bins.size(); ++k) if (cells_of(k) >= cells_of(dom)) dom = k;
        double f32 = 0, f64 = 0, domms = 0;
        for (uint32_t q = 0; q < n_sets; ++q) {
            const uint32_t set = (b->runs_timed - 1 - q) % b->ev_sets;
            hipEvent_t* ev = b->ev.data() + (size_t)set * b->bins.size() * 4;
            for (size_t k = 0; k < b->bins.size(); ++k) {
                float ms = 0;
                if (!force_f64) {
                    HIP_TRY(hipEventElapsedTime(&ms, ev[4 * k + 0], ev[4 * k + 1]));
                    f32 += ms;
                    if (k == dom) domms += ms;
                }
                float ms2 = 0;
                HIP_TRY(hipEventElapsedTime(&ms2, ev[4 * k + 2], ev[4 * k + 3]));
                f64 += ms2;
            }
        }
        st.n_runs_timed = n_sets;
        st.ms_f32 = (float)(f32 / n_sets); st.ms_f64 = (float)(f64 / n_sets);
        if (!force_f64) {
            st.ms_f32_dominant = (float)(domms / n_sets);
            st.dominant_cells = cells_of(dom);
            st.dominant_alg_bytes = acct ? b->acct_bytes[dom] : b->bins[dom].alg_bytes;
            if (acct && b->acct_multi[dom]) snprintf(st.dominant_kernel, sizeof st.dominant_kernel, "pairhmm_fwd_multi<%d>", b->acct_multi[dom] - 1);
            else snprintf(st.dominant_kernel, sizeof st.dominant_kernel, "pairhmm_fwd<float, %d, %d>", b->bins[dom].G, b->bins[dom].RPL);
        }
        b->runs_timed = 0;
    }
    *out = st;
    return 0;
}

namespace {
// Results of a batch that has been run, into its pinned mirror (staged batches): waits for this batch's last
// kernel only.  Downloads run on their own stream, so the results of batch k do not queue behind the kernels of
// batch k+1 that were enqueued in the meantime.
int fetch_results(mgx_pairhmm_t* c, mgx_pairhmm_batch_t* b, size_t bytes) {
    hipStream_t s = c->d2h;
    if (b->done) HIP_TRY(hipStreamWaitEvent(s, b->done, 0));
    HIP_TRY(hipMemcpyAsync(b->slab.pin + b->o_out, b->d_out, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// The results of a batch made of regions [g0, g1) (base: every region's first test case in the batch, as create_cross
// returns it), out of the pinned mirror into the caller's array of each region; keep may be NULL, and so may its entries.
void scatter_region_results(const mgx_pairhmm_batch* b, const std::vector<uint64_t>& base, const mgx_pairhmm_input_t* regions,
                            uint32_t g0, uint32_t g1, double* const* out, uint8_t* const* keep) {
    const double* all = (const double*)(b->slab.pin + b->o_out);
    const uint8_t* kept = b->slab.pin + b->o_keep;
    uint64_t r_at = 0;
    for (uint32_t g = g0; g < g1; ++g) {
        const uint64_t a = base[g - g0], e = base[g - g0 + 1];
        if (e > a) memcpy(out[g], all + a, (e - a) * sizeof(double));
        if (keep && keep[g] && e > a) memcpy(keep[g], kept + r_at, regions[g].n_reads);
        r_at += regions[g].n_reads;
    }
}

// Cuts a list of regions into runs of whole regions of about `limit` test cases: a run ends in front of the region
// that would take it past the limit (a region larger than the limit is a run of its own).  cut: the boundaries.
void cut_regions(const mgx_pairhmm_input_t* regions, uint32_t n_regions, uint64_t limit, std::vector<uint32_t>* cut) {
    cut->assign(1, 0);
    uint64_t in_run = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        const uint64_t n = regions[g].n_reads * regions[g].n_haps;
        if (in_run && in_run + n > limit) { cut->push_back(g); in_run = 0; }
        in_run += n;
    }
    if (n_regions) cut->push_back(n_regions);
}
}  // namespace

// The stages of a whole-region call (mgx_realign_internal.h): mgx_pairhmm_regions below runs them back to back, mgx_realign_regions
// (mgx_realign.hip) puts the best-haplotype and verbatim kernels between the run and the download.
extern "C++" {
namespace mgx_internal {
PairhmmView pairhmm_view(mgx_pairhmm_t* c) { return PairhmmView{c->device, c->flags, c->compute, c->d2h, &c->ext}; }

int regions_begin(mgx_pairhmm_t* c, uint32_t n_regions, const mgx_pairhmm_input_t* regions, const uint8_t* const* mapq,
                  const mgx_read_model_t* model, double* const* out_log10, RegionBatch* rb) {
    if (n_regions == 0) return 0;
    int rc;
    for (uint32_t g = 0; g < n_regions; ++g) {
        if ((rc = validate(&regions[g]))) return rc;
        if (regions[g].n_reads * regions[g].n_haps && !out_log10[g]) { set_error("region %u: output pointer is NULL", g); return -EINVAL; }
    }
    HIP_TRY(hipSetDevice(c->device));
    BatchPtr b = new_batch();
    if (!b) return -ENOMEM;
    if ((rc = create_cross(c, n_regions, regions, b.get(), &rb->base, mapq, model))) return rc;
    if (b->n_pairs == 0) return 0;
    mgx_pairhmm_batch* raw = b.release();
    if ((rc = mgx_pairhmm_batch_run(c, raw))) { mgx_pairhmm_batch_destroy(c, raw); return rc; }
    rb->batch = raw; rb->n_pairs = raw->n_pairs; rb->n_reads = raw->n_reads;
    rb->d_bases = raw->d_bases; rb->d_hap = raw->d_hap; rb->d_keep = raw->d_keep; rb->d_out = raw->d_out;
    rb->d_row_off = raw->d_row_off; rb->d_row_nh = raw->d_row_nh; rb->done = raw->done;
    return 0;
}

int regions_queue_download(mgx_pairhmm_t* c, const RegionBatch& rb, hipStream_t s) {
    const mgx_pairhmm_batch* b = rb.batch;
    if (s != c->compute) HIP_TRY(hipStreamWaitEvent(s, b->done, 0));
    HIP_TRY(hipMemcpyAsync(b->slab.pin + b->o_out, b->d_out, b->result_bytes, hipMemcpyDeviceToHost, s));
    return 0;
}

void regions_scatter(const RegionBatch& rb, const mgx_pairhmm_input_t* regions, uint32_t n_regions, double* const* out_log10,
                     uint8_t* const* out_keep) {
    scatter_region_results(rb.batch, rb.base, regions, 0, n_regions, out_log10, out_keep);
}

void regions_end(mgx_pairhmm_t* c, RegionBatch* rb) {
    mgx_pairhmm_batch_destroy(c, rb->batch);
    rb->batch = nullptr;
}

void launch_best_allele_rows(hipStream_t s, const double* d_values, const uint32_t* d_row_off, const uint32_t* d_row_nh,
                             const double* d_priority, const uint32_t* d_pri_off, uint32_t n_rows, int32_t* d_best) {
    hipLaunchKernelGGL(pairhmm_best_allele_rows, dim3((n_rows + 3) / 4), dim3(256), 0, s, d_values, d_row_off, d_row_nh, d_priority, d_pri_off,
                       n_rows, d_best);
}
}  // namespace mgx_internal
}  // extern "C++"

int mgx_pairhmm_batch_results(mgx_pairhmm_t* c, mgx_pairhmm_batch_t* b, double* out_log10,
                              uint8_t* used_f64) {
    if (!c || !b) { set_error("ctx/batch is NULL"); return -EINVAL; }
    if (!b->ran) { set_error("batch has not been run"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (b->n_pairs == 0) return 0;
    if (!out_log10) { set_error("out_log10 is NULL"); return -EINVAL; }
    if (b->slab.pin) {
        const int rc = fetch_results(c, b, used_f64 ? b->o_used + b->n_pairs - b->o_out : b->n_pairs * sizeof(double));
        if (rc) return rc;
        memcpy(out_log10, b->slab.pin + b->o_out, b->n_pairs * sizeof(double));
        if (used_f64) memcpy(used_f64, b->slab.pin + b->o_used, b->n_pairs);
        return 0;
    }
    hipStream_t s = c->d2h;
    if (b->done) HIP_TRY(hipStreamWaitEvent(s, b->done, 0));
    HIP_TRY(hipMemcpyAsync(out_log10, b->d_out, b->n_pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (used_f64) HIP_TRY(hipMemcpyAsync(used_f64, b->d_used, b->n_pairs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

void mgx_read_model_defaults(mgx_read_model_t* m) {
    if (!m) return;
    m->pcr_rate_factor = 3;             // CONSERVATIVE, LikelihoodEngineArgumentCollection.h:30
    m->base_quality_threshold = 18;     // PairHMM::BASE_QUALITY_SCORE_THRESHOLD, PairHMM.h:18
    m->constant_gcp = 10;               // gcpHMM
    m->log10_mismapping_rate = -4.5;    // phredScaledGlobalReadMismappingRate = 45
    m->max_error_per_base = 0.02;       // EXPECTED_ERROR_RATE_PER_BASE
}

int mgx_pairhmm_compute(mgx_pairhmm_t* c, const mgx_pairhmm_input_t* in, double* out_log10) {
    mgx_pairhmm_batch_t* b = nullptr;
    int rc = mgx_pairhmm_batch_create(c, in, &b);
    if (rc) return rc;
    rc = mgx_pairhmm_batch_run(c, b);
    if (!rc) rc = mgx_pairhmm_batch_results(c, b, out_log10, nullptr);
    mgx_pairhmm_batch_destroy(c, b);
    return rc;
}

int mgx_pairhmm_regions(mgx_pairhmm_t* c, uint32_t n_regions, const mgx_pairhmm_input_t* regions, const uint8_t* const* mapq,
                        const mgx_read_model_t* model, double* const* out_log10, uint8_t* const* out_keep) {
    if (!c || !model || (n_regions && (!regions || !mapq || !out_log10))) { set_error("NULL argument"); return -EINVAL; }
    // the stages below are shared with mgx_realign_regions (mgx_realign.hip), which puts its own between the run and the download
    mgx_internal::RegionBatch rb;
    int rc = mgx_internal::regions_begin(c, n_regions, regions, mapq, model, out_log10, &rb);
    if (rc || !rb.batch) return rc;
    rc = [&]() -> int {           // values and keep flags in one copy, behind the kernels on their own stream
        if (const int e = mgx_internal::regions_queue_download(c, rb, c->compute)) return e;
        HIP_TRY(hipStreamSynchronize(c->compute));
        return 0;
    }();
    if (!rc) mgx_internal::regions_scatter(rb, regions, n_regions, out_log10, out_keep);
    mgx_internal::regions_end(c, &rb);
    return rc;
}

int mgx_pairhmm_best_alleles(mgx_pairhmm_t* c, uint64_t n_rows, const uint64_t* row_off, const uint32_t* row_nh, const double* values_log10,
                             const double* priority, int32_t* out_best) {
    if (!c || (n_rows && (!row_off || !row_nh || !out_best))) { set_error("NULL argument"); return -EINVAL; }
    if (n_rows == 0) return 0;
    if (n_rows > 0xFFFFFFF0ull) { set_error("more than 2^32 rows"); return -E2BIG; }
    uint64_t n_values = 0;
    std::vector<uint32_t> off32(n_rows);
    for (uint64_t r = 0; r < n_rows; ++r) {
        if (row_off[r] + row_nh[r] > 0xFFFFFFF0ull) { set_error("row %llu ends beyond 2^32 values", (unsigned long long)r); return -E2BIG; }
        off32[r] = (uint32_t)row_off[r];
        n_values = std::max(n_values, row_off[r] + row_nh[r]);
    }
    if (n_values && !values_log10) { set_error("NULL argument"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    // [values | priorities | row_off | row_nh | best] in one allocation of the call's own
    const size_t vb = align_up(n_values * sizeof(double)), ib = align_up(n_rows * sizeof(uint32_t));
    uint8_t* dv = nullptr;
    HIP_TRY(hipMalloc((void**)&dv, 2 * vb + 3 * ib + 16));
    std::unique_ptr<uint8_t, void (*)(uint8_t*)> hold(dv, [](uint8_t* p) { (void)hipFree(p); });
    double* d_val = (double*)dv; double* d_pri = (double*)(dv + vb);
    uint32_t* d_off = (uint32_t*)(dv + 2 * vb); uint32_t* d_nh = (uint32_t*)(dv + 2 * vb + ib);
    int32_t* d_best = (int32_t*)(dv + 2 * vb + 2 * ib);
    hipStream_t s = c->compute;
    if (n_values) HIP_TRY(hipMemcpyAsync(d_val, values_log10, n_values * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_values && priority) HIP_TRY(hipMemcpyAsync(d_pri, priority, n_values * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_off, off32.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_nh, row_nh, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    mgx_internal::launch_best_allele_rows(s, d_val, d_off, d_nh, priority ? d_pri : nullptr, nullptr, (uint32_t)n_rows, d_best);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_best, d_best, n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int mgx_pairhmm_region(mgx_pairhmm_t* c, const mgx_pairhmm_input_t* in, const uint8_t* mapq,
                       const mgx_read_model_t* model, double* out_log10, uint8_t* out_keep) {
    if (!c || !in || !mapq || !model || !out_log10) { set_error("NULL argument"); return -EINVAL; }
    if (in->pair_read || in->pair_hap) { set_error("mgx_pairhmm_region takes the cross-product form (pair arrays NULL)"); return -EINVAL; }
    int rc = validate(in);
    if (rc) return rc;
    if (in->n_reads == 0 || in->n_haps == 0) return 0;
    return mgx_pairhmm_regions(c, 1, in, &mapq, model, &out_log10, out_keep ? &out_keep : nullptr);
}

int mgx_pairhmm_compute_regions(mgx_pairhmm_t* c, uint32_t n_regions, const mgx_pairhmm_input_t* regions, double* const* out_log10) {
    if (!c || (n_regions && (!regions || !out_log10))) { set_error("NULL argument"); return -EINVAL; }
    if (n_regions == 0) return 0;
    int rc;
    for (uint32_t g = 0; g < n_regions; ++g) {
        if ((rc = validate(&regions[g]))) return rc;
        if (regions[g].n_reads * regions[g].n_haps && !out_log10[g]) { set_error("region %u: output pointer is NULL", g); return -EINVAL; }
    }
    HIP_TRY(hipSetDevice(c->device));
    // A large call is cut into runs of whole regions of about kChunkPairs (196 608 to 393 216) test cases that go through the context two
    // at a time: while one chunk computes, the next is flattened and uploaded and the previous one's results are
    // scattered -- the queue's pipelining (mgx_pairhmm_queue_run_regions) on the caller's thread alone.
    // (tools/dev_regions_chunk.py, 1000 regions of 40 x 25 on an MI355X: 65 536 test cases per chunk 2 430 GCUPS, 131 072 3 035,
    // 196 608 3 193, 262 144 2 980-3 190, 524 288 2 610, one chunk 2 090: larger chunks mean larger class launches, fewer of them
    // mean less of the flattening hidden behind the kernels)
    // Larger jobs take larger chunks (a sixth of the job, at most 393 216 test cases): 1000 regions of 100 x 50 (5 M test cases)
    // 3 440 GCUPS with 131 072 per chunk, 3 790 with 196 608, 4 160 with 393 216, 3 960 with 524 288; 200 regions of 300 x 100:
    // 3 640 / 4 050 / 4 560 / 4 370; 4000 regions of 40 x 25: 3 460 with 196 608, 3 620 with 393 216 (tools/dev_regions_chunk_shapes.py)
    uint64_t kChunkPairs = 3u << 16;
    {
        uint64_t total = 0;
        for (uint32_t g = 0; g < n_regions; ++g) total += regions[g].n_reads * regions[g].n_haps;
        kChunkPairs = std::min<uint64_t>(6u << 16, std::max<uint64_t>(kChunkPairs, total / 6));
    }
    if (const char* e = getenv("MGX_PAIRHMM_REGION_CHUNK")) { const long long v = atoll(e); if (v > 0) kChunkPairs = (uint64_t)v; }      // A/B
    std::vector<uint32_t> cut;
    cut_regions(regions, n_regions, kChunkPairs, &cut);
    struct InFlight { mgx_pairhmm_batch_t* b = nullptr; uint32_t g0 = 0, g1 = 0; std::vector<uint64_t> base; };
    InFlight fl[2];
    auto retire = [&](InFlight& f) -> int {
        if (!f.b) return 0;
        const int r = fetch_results(c, f.b, f.b->n_pairs * sizeof(double));
        if (!r) scatter_region_results(f.b, f.base, regions, f.g0, f.g1, out_log10, nullptr);
        mgx_pairhmm_batch_destroy(c, f.b);
        f.b = nullptr;
        return r;
    };
    rc = 0;
    for (size_t k = 0; k + 1 < cut.size() && !rc; ++k) {
        InFlight& f = fl[k & 1];
        rc = retire(f);                                  // the chunk launched two iterations ago
        if (rc) break;
        BatchPtr b = new_batch();
        if (!b) { rc = -ENOMEM; break; }
        f.g0 = cut[k]; f.g1 = cut[k + 1];
        if ((rc = create_cross(c, f.g1 - f.g0, regions + f.g0, b.get(), &f.base))) break;
        if (b->n_pairs == 0) continue;
        f.b = b.release();
        rc = mgx_pairhmm_batch_run(c, f.b);
    }
    for (int q = 0; q < 2; ++q) { const int r = retire(fl[(cut.size() - 1 + q) & 1]); if (!rc) rc = r; }   // oldest first
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Host work queue (BASELINE.json configs[2]).  The reference's worker threads pull the next active
// region off one atomic index (deepmutect/Mutect2Cpp-master/src/main.cpp:254) and share the tail of the
// work at the end (main.cpp:302-315, IntelPairHmm.cc:296-330).  Here the unit pulled is a BATCH of test
// cases: every lane -- a host thread with its own context, i.e. its own streams and recycled pinned
// slabs -- takes the next batch index, plans and packs it (pairhmm_pack.h), uploads, launches and moves on
// to the next one while the device works; a batch's results are fetched when its slot comes round
// again, `depth` batches later.  Several lanes per device keep the PCIe link busy (one core packs
// ~10 GB/s, the link takes ~55); lanes of different devices share the same counter, so a faster GPU
// simply takes more batches.  No collective, no device-to-device traffic.
// ---------------------------------------------------------------------------------------------
struct mgx_pairhmm_queue {
    struct Lane {
        mgx_pairhmm* ctx = nullptr;
        uint32_t dev_slot = 0;
        double pack_s = 0, wait_s = 0;
        uint64_t batches = 0, bytes_h2d = 0, bytes_d2h = 0, cells = 0;
    };
    std::vector<Lane> lanes;
    uint32_t n_devices = 1, depth = 2, batch_pairs = 65536;
    mgx_pairhmm_queue_stats_t stats{};
};

namespace {

struct QueueRun {
    const mgx_pairhmm_input_t* in = nullptr;      // pair-stream mode: one long stream, batches are test-case ranges
    uint64_t lo = 0, hi = 0, n_batches = 0;
    double* out = nullptr;
    uint8_t* used = nullptr;
    // region mode (row F1): many active regions in the cross-product form, batches are runs of whole regions
    const mgx_pairhmm_input_t* regions = nullptr;
    double* const* region_out = nullptr;
    std::vector<uint32_t> chunk;                   // [n_batches + 1] region index boundaries
    std::atomic<uint64_t> next{0};
    std::atomic<int> failed{0};
    std::mutex err_mu;
    int rc = 0;
    std::string err;
    void fail(int code) {
        std::lock_guard<std::mutex> g(err_mu);
        if (!rc) { rc = code; err = mgx_last_error(); }
        failed.store(1);
    }
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void queue_lane(mgx_pairhmm_queue* q, mgx_pairhmm_queue::Lane* ln, QueueRun* run) {
    struct Slot { mgx_pairhmm_batch* b = nullptr; uint64_t lo = 0; uint32_t g0 = 0, g1 = 0; std::vector<uint64_t> base; };
    std::vector<Slot> slots(q->depth);
    mgx::PackPlan plan;
    mgx_pairhmm* c = ln->ctx;
    if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); run->fail(-EIO); return; }
    auto retire = [&](Slot& sl) {
        if (!sl.b) return;
        const double t0 = now_s();
        if (!run->failed.load()) {
            int rc = 0;
            if (run->regions) {
                rc = fetch_results(c, sl.b, sl.b->n_pairs * sizeof(double));
                if (!rc) scatter_region_results(sl.b, sl.base, run->regions, sl.g0, sl.g1, run->region_out, nullptr);
                ln->bytes_d2h += sl.b->n_pairs * 8;
            } else {
                const uint64_t at = sl.lo - run->lo;
                rc = mgx_pairhmm_batch_results(c, sl.b, run->out + at, run->used ? run->used + at : nullptr);
                ln->bytes_d2h += sl.b->n_pairs * (run->used ? 9 : 8);
            }
            if (rc) run->fail(rc);
        }
        mgx_pairhmm_batch_destroy(c, sl.b);
        sl.b = nullptr;
        ln->wait_s += now_s() - t0;
    };
    size_t turn = 0;
    while (!run->failed.load()) {
        const uint64_t k = run->next.fetch_add(1);
        if (k >= run->n_batches) break;
        Slot& sl = slots[turn++ % slots.size()];
        retire(sl);
        if (run->failed.load()) break;
        const double t0 = now_s();
        BatchPtr b = new_batch();
        int rc = b ? 0 : -ENOMEM;
        if (!rc && run->regions) {
            sl.g0 = run->chunk[k]; sl.g1 = run->chunk[k + 1];
            rc = create_cross(c, sl.g1 - sl.g0, run->regions + sl.g0, b.get(), &sl.base);
        } else if (!rc) {
            sl.lo = run->lo + k * q->batch_pairs;
            const uint64_t hi = std::min(run->hi, sl.lo + q->batch_pairs);
            const uint64_t bad = mgx::pack_plan(run->in, sl.lo, hi, &plan);
            if (bad) { set_error("test case %llu: index out of range", (unsigned long long)(sl.lo + bad - 1)); run->fail(-EINVAL); break; }
            rc = create_pairs(c, run->in, &plan, b.get());
        }
        ln->pack_s += now_s() - t0;
        if (!rc && b->n_pairs) rc = mgx_pairhmm_batch_run(c, b.get());
        if (rc) { run->fail(rc); break; }
        if (!b->n_pairs) continue;                  // a chunk of empty regions
        ln->batches++; ln->bytes_h2d += b->in_bytes; ln->cells += b->stats.cells;
        sl.b = b.release();
    }
    for (size_t j = 0; j < slots.size(); ++j) retire(slots[(turn + j) % slots.size()]);    // oldest first
}

int queue_execute(mgx_pairhmm_queue* q, QueueRun& run, uint64_t n_pairs) {
    for (auto& ln : q->lanes) { ln.pack_s = ln.wait_s = 0; ln.batches = ln.bytes_h2d = ln.bytes_d2h = ln.cells = 0; }
    const double t0 = now_s();
    const size_t n_thr = (size_t)std::min<uint64_t>(q->lanes.size(), run.n_batches);
    std::vector<std::thread> th;
    for (size_t i = 1; i < n_thr; ++i) th.emplace_back(queue_lane, q, &q->lanes[i], &run);
    queue_lane(q, &q->lanes[0], &run);               // the caller's thread is lane 0
    for (auto& t : th) t.join();
    q->stats.seconds = now_s() - t0;
    q->stats.n_pairs = n_pairs;
    q->stats.n_batches = run.n_batches;
    for (auto& ln : q->lanes) {
        q->stats.cells += ln.cells; q->stats.bytes_h2d += ln.bytes_h2d; q->stats.bytes_d2h += ln.bytes_d2h;
        q->stats.pack_seconds += ln.pack_s; q->stats.wait_seconds += ln.wait_s;
        q->stats.batches_per_device[ln.dev_slot] += ln.batches;
    }
    if (run.rc) { set_error("%s", run.err.c_str()); return run.rc; }
    return 0;
}

}  // namespace

int mgx_pairhmm_queue_create(const mgx_pairhmm_queue_config_t* cfg, mgx_pairhmm_queue_t** out) {
    if (!out) { set_error("out is NULL"); return -EINVAL; }
    *out = nullptr;
    mgx_pairhmm_queue_config_t d{};
    if (cfg) d = *cfg;
    const int dev0 = 0;
    const uint32_t n_dev = d.n_devices && d.devices ? d.n_devices : 1;
    if (n_dev > 16) { set_error("at most 16 devices per queue"); return -EINVAL; }
    const uint32_t lanes = d.lanes_per_device ? d.lanes_per_device : 4;
    if (lanes > 32) { set_error("at most 32 lanes per device"); return -EINVAL; }
    std::unique_ptr<mgx_pairhmm_queue> q(new (std::nothrow) mgx_pairhmm_queue);
    if (!q) return -ENOMEM;
    q->n_devices = n_dev;
    q->depth = d.depth ? std::min<uint32_t>(d.depth, 8) : 2;
    q->batch_pairs = d.batch_pairs ? d.batch_pairs : 65536;
    for (uint32_t v = 0; v < n_dev; ++v)
        for (uint32_t l = 0; l < lanes; ++l) {
            mgx_pairhmm_queue::Lane ln;
            ln.dev_slot = v;
            const int rc = mgx_pairhmm_create(d.n_devices && d.devices ? d.devices[v] : dev0, d.flags, &ln.ctx);
            if (rc) { for (auto& x : q->lanes) mgx_pairhmm_destroy(x.ctx); return rc; }
            q->lanes.push_back(ln);
        }
    *out = q.release();
    return 0;
}

void mgx_pairhmm_queue_destroy(mgx_pairhmm_queue_t* q) {
    if (!q) return;
    for (auto& ln : q->lanes) mgx_pairhmm_destroy(ln.ctx);
    delete q;
}

int mgx_pairhmm_queue_run_range(mgx_pairhmm_queue_t* q, const mgx_pairhmm_input_t* in, uint64_t pair_begin, uint64_t pair_end,
                                double* out_log10, uint8_t* used_f64) {
    if (!q) { set_error("queue is NULL"); return -EINVAL; }
    int rc = validate(in);
    if (rc) return rc;
    const uint64_t total = mgx::pack_n_pairs(in);
    if (pair_begin > pair_end || pair_end > total) { set_error("test-case range [%llu, %llu) outside the stream of %llu", (unsigned long long)pair_begin, (unsigned long long)pair_end, (unsigned long long)total); return -EINVAL; }
    q->stats = mgx_pairhmm_queue_stats_t{};
    q->stats.n_lanes = (uint32_t)q->lanes.size();
    if (pair_begin == pair_end) return 0;
    if (!out_log10) { set_error("out_log10 is NULL"); return -EINVAL; }
    QueueRun run;
    run.in = in; run.lo = pair_begin; run.hi = pair_end; run.out = out_log10; run.used = used_f64;
    run.n_batches = (pair_end - pair_begin + q->batch_pairs - 1) / q->batch_pairs;
    return queue_execute(q, run, pair_end - pair_begin);
}

int mgx_pairhmm_queue_run_regions(mgx_pairhmm_queue_t* q, uint32_t n_regions, const mgx_pairhmm_input_t* regions, double* const* out_log10) {
    if (!q || (n_regions && (!regions || !out_log10))) { set_error("NULL argument"); return -EINVAL; }
    q->stats = mgx_pairhmm_queue_stats_t{};
    q->stats.n_lanes = (uint32_t)q->lanes.size();
    QueueRun run;
    run.regions = regions; run.region_out = out_log10;
    uint64_t total = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        int rc = validate(&regions[g]);
        if (rc) return rc;
        if (regions[g].pair_read || regions[g].pair_hap) { set_error("region %u: regions are given in the cross-product form (pair arrays NULL)", g); return -EINVAL; }
        const uint64_t n = regions[g].n_reads * regions[g].n_haps;
        if (n && !out_log10[g]) { set_error("region %u: output pointer is NULL", g); return -EINVAL; }
        total += n;
    }
    cut_regions(regions, n_regions, q->batch_pairs, &run.chunk);      // batches are runs of whole regions holding about batch_pairs test cases
    run.n_batches = run.chunk.size() - 1;
    if (total == 0) return 0;
    return queue_execute(q, run, total);
}

int mgx_pairhmm_queue_run(mgx_pairhmm_queue_t* q, const mgx_pairhmm_input_t* in, double* out_log10, uint8_t* used_f64) {
    if (!in) { set_error("input is NULL"); return -EINVAL; }
    return mgx_pairhmm_queue_run_range(q, in, 0, mgx::pack_n_pairs(in), out_log10, used_f64);
}

int mgx_pairhmm_queue_stats(mgx_pairhmm_queue_t* q, mgx_pairhmm_queue_stats_t* out) {
    if (!q || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = q->stats;
    return 0;
}

}  // extern "C"
