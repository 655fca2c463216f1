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
#include "mgx_hip_util.h"
#include "mgx_realign_internal.h"
#include "mgx_tables.h"
#include "pairhmm_pack.h"
#include "pairhmm_plan.h"
#include "pairhmm_wire.h"
#include "pairhmm_kernels.hip.inc"

using mgx::set_error;
using namespace mgx_hmm_plan;

namespace {

// One device allocation + (for batches up to kStageLimit) a pinned host mirror of the same size.
// Slabs are recycled through the context, so a stream of region-sized batches does no hipMalloc.
struct Slab {
    uint8_t* dev = nullptr;
    uint8_t* pin = nullptr;     // mirrors the first pin_cap bytes only: inputs and results, never device scratch
    size_t cap = 0, pin_cap = 0;
};
constexpr size_t kMaxEventSets = 64;       // runs whose kernel durations a timed batch remembers
constexpr size_t kMinSlab = 1u << 20;
}  // namespace

struct mgx_pairhmm {
    mgx_hip::Owner own;          // of the streams and the tables below; the first member: the streams go last
    int device = 0;
    unsigned flags = 0;
    hipStream_t compute = nullptr, copy = nullptr, d2h = nullptr;   // kernels | uploads | result downloads
    float* d_ph2pr_f = nullptr; float* d_mm_f = nullptr; float* d_div3_f = nullptr; float* d_ratio_f = nullptr;
    double* d_ph2pr_d = nullptr; double* d_mm_d = nullptr; double* d_div3_d = nullptr; double* d_ratio_d = nullptr;
    float log10_initial_f = 0; double log10_initial_d = 0;
    int n_cu = 256;
    bool wire = false;           // MGX_PAIRHMM_WIRE, or its environment override: staged pair-list batches upload the wire form
    std::vector<Slab> free_slabs;
    mgx_hip::DevArray<uint8_t> strip;                   // boundary rows of the strip-mined class (one compute stream: launches do not overlap)
    mgx_internal::PairhmmExt ext;                       // mgx_realign.hip's buffers and statistics
    ~mgx_pairhmm() {
        if (ext.p && ext.free_fn) ext.free_fn(ext.p);
        for (auto& sl : free_slabs) { (void)hipFree(sl.dev); if (sl.pin) (void)hipHostFree(sl.pin); }
    }
};

struct mgx_pairhmm_batch {
    uint64_t n_pairs = 0;
    std::vector<Bin> bins;
    Slab slab;                                   // everything lives in one slab ...
    SlabLayout lay;                              // ... laid out by the plan (SlabLayout, pairhmm_plan.h): inputs | results | device scratch
    template <typename T = uint8_t> T* dev(size_t off) const { return (T*)(slab.dev + off); }
    uint32_t* rerun_list() const { return dev<uint32_t>(lay.rlist); }
    uint32_t* counters() const { return dev<uint32_t>(lay.rcount); }
    std::vector<Job> host_jobs;    // only kept for unstaged (very large) batches
    // whole-region form (mgx_pairhmm_regions): normalise / filter epilogue over every read's row of the output
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

// a table of the context, owned by `own`; the copy is queued on s
template <typename T>
void upload(mgx_hip::Owner& own, T** dst, const std::vector<T>& src, hipStream_t s) {
    if (own.device(dst, src.size() * sizeof(T))) own.note(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
}

// ---- the wire form's device side (pairhmm_wire.h): one launch on the copy stream, right behind the H2D copy, turns
// [bases4 | qual | ins | del | gcp | hap4] back into the six byte arrays the PairHMM kernels read.  The grid is laid
// over the concatenated work of the six arrays; which array a workgroup serves is uniform over it.  One thread
// produces 8 output bytes with one 8-byte store: of a bit stream it reads the group's w bytes at byte offset w t, of
// nibble codes 4 bytes, which two byte permutes map through "ACTGN".  No LDS, nothing shared between threads.
// (the grid: expand_grid in pairhmm_plan.h)
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

template <typename T>
int host_table(int which, const T** out) {
    const auto& t = mgx::tables<T>();
    if (which == 0) { *out = t.ph2pr.data(); return mgx::kPh2prSize; }
    if (which == 1) { *out = t.mm.data(); return mgx::kMmSize; }
    return -EINVAL;
}

}  // namespace

extern "C" {

int mgx_pairhmm_table_f32(int which, const float** out) { return host_table(which, out); }
int mgx_pairhmm_table_f64(int which, const double** out) { return host_table(which, out); }

int mgx_pairhmm_create(int device, unsigned flags, mgx_pairhmm_t** out) {
    if (!out) { set_error("out is NULL"); return -EINVAL; }
    *out = nullptr;
    static std::atomic<unsigned> next{0};      // MGX_DEVICE_AUTO: contexts are dealt round-robin over the visible GPUs
    if (const int rc = mgx_hip::pick_device(&device, &next)) return rc;
    std::unique_ptr<mgx_pairhmm> c(new (std::nothrow) mgx_pairhmm);
    if (!c) return -ENOMEM;
    c->device = device;
    c->flags = flags;
    c->wire = (flags & MGX_PAIRHMM_WIRE) != 0;
    if (const char* e = getenv("MGX_PAIRHMM_WIRE")) { if (*e) c->wire = atoi(e) != 0; }      // A/B: read per context, not once per process
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount;
    mgx_hip::Owner& m = c->own;
    m.stream(&c->compute, c->n_cu, (flags >> 8) & 0xFFu);
    m.stream(&c->copy); m.stream(&c->d2h);
    const auto& tf = mgx::tables<float>();
    const auto& td = mgx::tables<double>();
    upload(m, &c->d_ph2pr_f, tf.ph2pr, c->compute); upload(m, &c->d_mm_f, tf.mm, c->compute);
    upload(m, &c->d_ph2pr_d, td.ph2pr, c->compute); upload(m, &c->d_mm_d, td.mm, c->compute);
    upload(m, &c->d_div3_f, tf.ph2pr_div3, c->compute); upload(m, &c->d_ratio_f, tf.gap_ratio, c->compute);
    upload(m, &c->d_div3_d, td.ph2pr_div3, c->compute); upload(m, &c->d_ratio_d, td.gap_ratio, c->compute);
    c->log10_initial_f = tf.log10_initial;
    c->log10_initial_d = td.log10_initial;
    if (m.ok()) m.note(hipStreamSynchronize(c->compute), "hipStreamSynchronize");
    if (!m.ok()) return m.error("a PairHMM context");
    *out = c.release();
    return 0;
}

void mgx_pairhmm_destroy(mgx_pairhmm_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
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

// The plan's three environment knobs.  MGX_PAIRHMM_MIN_G=16 switches the narrow groups off (read once).  MGX_PAIRHMM_BLOCK is the
// workgroup size of the single-class launches; 64, one wavefront per workgroup, packs LDS and VGPRs finest and needs no
// cross-wave barriers (in-process A/B at 1 M pairs: 5.48 ms (64), 5.65 (128), 5.46 (256)).  MGX_PAIRHMM_MERGE_BELOW, 1 to 4096,
// is the number of test cases below which a class is folded into the next one (merge_small_bins; anything else: kMergeBelow).
// With 1 no class is folded, so that a test reaches the kernel of a class with a handful of test cases.  Like the workgroup
// size it is read per batch.
// (static, as every helper below that is new: in this file's extern "C" block a plain function of an unnamed namespace is exported)
static int env_min_g() { static const int v = [] { const char* e = getenv("MGX_PAIRHMM_MIN_G"); return e ? atoi(e) : 4; }(); return v; }
static uint32_t env_block() { const char* e = getenv("MGX_PAIRHMM_BLOCK"); const int v = e ? atoi(e) : 64; return v == 128 || v == 256 ? (uint32_t)v : 64u; }
static uint64_t env_merge_below() { const char* e = getenv("MGX_PAIRHMM_MERGE_BELOW"); const long long v = e ? atoll(e) : 0; return v >= 1 && v <= (long long)kMergeBelow ? (uint64_t)v : kMergeBelow; }

// the caller's six sequence arrays, in the order of SlabLayout::seq, wseq and mgx_pairhmm_batch::lay.seq
static const uint8_t* seq_src(const mgx_pairhmm_input_t* in, int k) {
    const uint8_t* const src[kSeqArrays] = {in->bases, in->qual, in->ins, in->del, in->gcp, in->hap_bases};
    return src[k];
}

// cells and bytes of a batch: the sum over its classes
static void sum_stats(mgx_pairhmm_batch* b) {
    for (const Bin& bin : b->bins) { b->stats.cells += bin.cells; b->stats.alg_bytes += bin.alg_bytes; }
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

// the enumeration tables (pairhmm_plan.h) and the sequences, into the pinned mirror
void cross_stage(const CrossPlan& p, uint32_t n_regions, const mgx_pairhmm_input_t* regs, const SlabLayout& L, uint8_t* pin) {
    cross_write_tables(p, (SeqRef*)(pin + L.rtab), (uint32_t*)(pin + L.rreg), (uint32_t*)(pin + L.rpre));
    memcpy(pin + L.gtab, p.regions.data(), n_regions * sizeof(RegionRef));
    memcpy(pin + L.htab, p.haps.data(), p.nh * sizeof(SeqRef));
    size_t rb = 0, hb = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        const mgx_pairhmm_input_t& in = regs[g];
        const uint64_t r0 = in.n_reads ? in.read_off[0] : 0, rlen = in.n_reads ? in.read_off[in.n_reads] - r0 : 0;
        const uint64_t h0 = in.n_haps ? in.hap_off[0] : 0, hlen = in.n_haps ? in.hap_off[in.n_haps] - h0 : 0;
        for (int k = 0; k < kSeqArrays; ++k) {
            if (k == kSeqHap) { if (hlen) memcpy(pin + L.seq[k] + hb, seq_src(&in, k) + h0, hlen); }
            else if (rlen) memcpy(pin + L.seq[k] + rb, seq_src(&in, k) + r0, rlen);
        }
        rb += rlen; hb += hlen;
    }
}

// per read, in global read order: MAPQ, length, and its row of the output
int cross_stage_model(uint32_t n_regions, const mgx_pairhmm_input_t* regs, const uint8_t* const* mapq,
                      const std::vector<uint64_t>& out_base, const SlabLayout& L, uint8_t* pin) {
    uint64_t r_at = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        if (regs[g].n_reads && !mapq[g]) { set_error("region %u: mapq is NULL", g); return -EINVAL; }
        if (regs[g].n_reads) memcpy(pin + L.mapq + r_at, mapq[g], regs[g].n_reads);
        r_at += regs[g].n_reads;
    }
    cross_write_rows(n_regions, regs, out_base, (uint64_t*)(pin + L.rlen), (uint32_t*)(pin + L.roff), (uint32_t*)(pin + L.rnh));
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
    if ((rc = cross_tables(n_regions, regs, *out_base, env_min_g(), &p, count))) return rc;
    if ((rc = cross_bins(&p, count, c->n_cu, env_block(), &b->bins, env_merge_below()))) return rc;      // before anything is enqueued
    sum_stats(b);
    SlabLayout& L = b->lay;
    L.n = p.n; L.n_reads = p.nr; L.n_haps = p.nh; L.n_regions = n_regions; L.read_bytes = p.read_bytes; L.hap_bytes = p.hap_bytes;
    L.cross = true; L.model = model != nullptr;
    plan_slab(true, &L);
    if ((rc = acquire_slab(c, L.total, L.pin_bytes, &b->slab))) return rc;
    uint8_t* dv = b->slab.dev; uint8_t* pin = b->slab.pin;
    cross_stage(p, n_regions, regs, L, pin);
    hipStream_t s = c->copy;
    if (model) {
        if ((rc = cross_stage_model(n_regions, regs, mapq, *out_base, L, pin))) return rc;
        b->log10_rate = model->log10_mismapping_rate; b->max_err = model->max_error_per_base;
    }
    HIP_TRY(hipMemcpyAsync(dv, pin, b->lay.in_bytes, hipMemcpyHostToDevice, s));
    if (model)      // modifyReadQualities + gap continuation penalties, in place on the uploaded arrays
        hipLaunchKernelGGL(pairhmm_read_model, dim3((uint32_t)p.nr), dim3(128), 0, s, (const SeqRef*)(dv + L.rtab), b->dev(b->lay.seq[kSeqBases]),
                           b->dev(b->lay.seq[kSeqQual]), b->dev(b->lay.seq[kSeqIns]), b->dev(b->lay.seq[kSeqDel]), b->dev(b->lay.seq[kSeqGcp]), (const uint8_t*)(dv + L.mapq), make_read_model(*model));
    // one enumeration launch for all bins: jobs are laid out in read-table order, which is bin order
    hipLaunchKernelGGL(pairhmm_make_jobs_multi, dim3((uint32_t)((p.n + 255) / 256)), dim3(256), 0, s, (const SeqRef*)(dv + L.rtab),
                       (const uint32_t*)(dv + L.rreg), (const uint32_t*)(dv + L.rpre), (uint32_t)p.nr, (const RegionRef*)(dv + L.gtab),
                       (const SeqRef*)(dv + L.htab), (uint32_t)p.n, b->dev<Job>(b->lay.jobs));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventCreateWithFlags(&b->uploaded, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->uploaded, s));
    return 0;
}

// The six arrays of a pair-list batch in the wire form, straight from the caller's arrays into the pinned mirror
// (the gather and the bit-packing are one pass; the widths come from create_pairs' pre-pass).
void stage_wire(const mgx_pairhmm_input_t* in, const mgx::PackPlan* plan, const SlabLayout& L, uint8_t* pin) {
    namespace W = mgx::wire;
    uint8_t* dst[kSeqArrays];
    for (int k = 0; k < kSeqArrays; ++k) dst[k] = pin + L.wseq[k];
    if (plan || L.read_bytes + L.hap_bytes < (32u << 20)) {
        W::pack_arrays(in, plan, L.ww, dst[kSeqBases], dst[kSeqQual], dst[kSeqIns], dst[kSeqDel], dst[kSeqGcp], dst[kSeqHap]);
        return;
    }
    // a large one-shot batch: one thread per array, as the plain form stages it
    std::thread th[kSeqArrays];
    for (int k = 0; k < kSeqArrays; ++k) {
        const uint32_t w = L.wire_width(k);
        uint8_t* const to = dst[k];
        th[k] = std::thread([=] {
            if (w == 4) W::pack_nibbles(in, plan, k == kSeqBases, to);
            else if (w) W::pack_stream(in, plan, seq_src(in, k), w, to);       // w == 0: a constant gcp travels in the widths
        });
    }
    for (auto& t : th) t.join();
}

// pairhmm_expand_wire behind the copy, on the same stream: the six arrays are whole before `uploaded` is recorded
int launch_expand_wire(hipStream_t s, const SlabLayout& L, mgx_pairhmm_batch* b) {
    ExpandWireArgs a{};
    if (const int rc = expand_grid(L, a.n, a.w, a.block_first)) return rc;
    for (int k = 0; k < kSeqArrays; ++k) { a.src[k] = b->slab.dev + L.wseq[k]; a.dst[k] = b->dev(b->lay.seq[k]); }
    a.fill = L.ww.gcp_const;
    if (a.block_first[kSeqArrays] == 0) return 0;
    hipLaunchKernelGGL(pairhmm_expand_wire, dim3(a.block_first[kSeqArrays]), dim3(kExpandBlock), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Upload of a pair-list batch: one copy out of the pinned mirror, or (very large batches) one per array.
int upload_pairs(mgx_pairhmm_t* c, const mgx_pairhmm_input_t* in, const mgx::PackPlan* plan, const SlabLayout& L, const Job* jobs,
                 mgx_pairhmm_batch* b) {
    uint8_t* dv = b->slab.dev;
    uint8_t* pin = b->slab.pin;
    hipStream_t s = c->copy;
    if (L.wire) {
        stage_wire(in, plan, L, pin);
        HIP_TRY(hipMemcpyAsync(dv, pin, b->lay.in_bytes, hipMemcpyHostToDevice, s));
        if (const int rc = launch_expand_wire(s, L, b)) return rc;
    } else if (L.staged) {
        if (plan) {
            mgx::pack_copy(in, *plan, pin + L.seq[kSeqBases], pin + L.seq[kSeqQual], pin + L.seq[kSeqIns], pin + L.seq[kSeqDel],
                           pin + L.seq[kSeqGcp], pin + L.seq[kSeqHap]);
        } else {
            // a large one-shot batch: the six arrays are staged by six threads (one core copies ~10 GB/s)
            const bool threaded = L.read_bytes + L.hap_bytes >= (32u << 20);
            std::thread th[kSeqArrays];
            for (int k = 0; k < kSeqArrays; ++k) {
                uint8_t* const to = pin + L.seq[k];
                const size_t len = L.seq_len(k);
                if (threaded) th[k] = std::thread([=] { memcpy(to, seq_src(in, k), len); });
                else memcpy(to, seq_src(in, k), len);
            }
            if (threaded) for (auto& t : th) t.join();
        }
        HIP_TRY(hipMemcpyAsync(dv, pin, b->lay.in_bytes, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(hipMemcpyAsync(b->dev<Job>(b->lay.jobs), jobs, L.n * sizeof(Job), hipMemcpyHostToDevice, s));
        for (int k = 0; k < kSeqArrays; ++k) HIP_TRY(hipMemcpyAsync(b->dev(b->lay.seq[k]), seq_src(in, k), L.seq_len(k), hipMemcpyHostToDevice, s));
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
    PairView v;
    v.n = plan ? plan->hi - plan->lo : in->n_pairs;
    v.pr = plan ? plan->pair_read.data() : in->pair_read;
    v.ph = plan ? plan->pair_hap.data() : in->pair_hap;
    v.roff = plan ? plan->roff.data() : in->read_off;
    v.hoff = plan ? plan->hoff.data() : in->hap_off;
    v.n_reads = plan ? plan->lread.size() : in->n_reads; v.n_haps = plan ? plan->lhap.size() : in->n_haps;
    int rc;
    b->n_pairs = v.n;
    b->stats.n_pairs = v.n;
    PairClasses pc;
    if ((rc = classify_pairs(v, env_min_g(), &pc, env_merge_below()))) return rc;
    // one slab for everything; the layout is decided before the jobs are written so that they can be built directly in
    // the pinned mirror
    SlabLayout& L = b->lay;
    L.n = v.n; L.n_reads = v.n_reads; L.n_haps = v.n_haps; L.read_bytes = v.roff[v.n_reads]; L.hap_bytes = v.hoff[v.n_haps];
    if (c->wire) { L.wire = true; L.ww = mgx::wire::scan_widths(in, plan); }      // the widths decide the layout
    plan_slab(plan != nullptr, &L);
    if ((rc = acquire_slab(c, L.total, L.staged ? L.pin_bytes : 0, &b->slab))) return rc;
    if (!L.staged) b->host_jobs.resize(v.n);
    Job* jobs = L.staged ? (Job*)(b->slab.pin + L.jobs) : b->host_jobs.data();
    if ((rc = sort_pairs(v, pc, c->n_cu, env_block(), jobs, &b->bins))) return rc;
    sum_stats(b);
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

// what the steps of one mgx_pairhmm_batch_run share
struct Run {
    mgx_pairhmm* c = nullptr;
    mgx_pairhmm_batch* b = nullptr;
    hipStream_t s = nullptr;                   // the compute stream
    bool timing = false, force_f64 = false;
    hipEvent_t* ev = nullptr;                  // this run's event set (timing only)
    KernelArgs base{};                         // the arguments every launch starts from
    std::vector<char> in_multi;                // classes that a multi-class launch has computed
    NarrowExtent narrow;                       // what the shared fp64 launch covers; narrow.first books it
};

// boundary rows of the strip-mined class and of the exact tier: one array per context, grown on demand
int ensure_strip_scratch(mgx_pairhmm* c, size_t bytes) {
    if (bytes <= c->strip.cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->compute));           // an earlier launch may still be using the old array
    return c->strip.reserve(bytes);
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

// the compute stream waits for the upload, the counters and flags are cleared
int begin_run(Run& r) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    if (b->uploaded) HIP_TRY(hipStreamWaitEvent(r.s, b->uploaded, 0));
    HIP_TRY(hipMemsetAsync(b->counters(), 0, kCounters * sizeof(uint32_t), r.s));
    HIP_TRY(hipMemsetAsync(b->dev(b->lay.o_used), 0, b->n_pairs, r.s));
    KernelArgs& base = r.base;
    base.jobs = b->dev<Job>(b->lay.jobs);
    base.bases = b->dev(b->lay.seq[kSeqBases]); base.qual = b->dev(b->lay.seq[kSeqQual]); base.ins = b->dev(b->lay.seq[kSeqIns]); base.del = b->dev(b->lay.seq[kSeqDel]);
    base.gcp = b->dev(b->lay.seq[kSeqGcp]); base.hap_bases = b->dev(b->lay.seq[kSeqHap]);
    base.out_log10 = b->dev<double>(b->lay.o_out); base.used_f64 = b->dev(b->lay.o_used);
    base.nhap_list = b->dev<uint32_t>(b->lay.nlist); base.nhap_count = b->counters() + kNhapCount;
    base.form_count = b->counters() + kFormDeferCount;
    base.log10_initial_f = c->log10_initial_f;
    base.log10_initial_d = c->log10_initial_d;
    return 0;
}

// an fp64 launch over a job list or a class; what it leaves near the flush-to-zero threshold goes to the exact tier's list
int launch_f64(const Run& r, KernelArgs a, int Gd, int RPLd, uint32_t grid, uint32_t block, uint32_t lds) {
    const mgx_pairhmm* c = r.c;
    a.ph2pr = c->d_ph2pr_d; a.mm = c->d_mm_d; a.ph2pr_div3 = c->d_div3_d; a.gap_ratio = c->d_ratio_d;
    a.rerun_list = r.b->rerun_list() + r.b->n_pairs; a.rerun_count = r.b->counters() + kExactCount;      // job_list / n_dyn are set: the fp64 tier appends here
    KernelFn f = a.strip_scratch ? (KernelFn)pairhmm_fwd_strip<double> : pick_kernel<double>(Gd, RPLd);
    if (!f) { set_error("no fp64 kernel for G=%d RPL=%d", Gd, RPLd); return -ENOSYS; }
    hipLaunchKernelGGL(f, dim3(grid), dim3(block), lds, r.s, a);
    return 0;
}

// one multi-class launch over the classes `set` (lane-width set gset), booked on the member with the most cells
int launch_multi(Run& r, int gset, const MultiSet& ms) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    const std::vector<size_t>& set = ms.members;
    MultiArgs m{};
    m.a = r.base;
    m.a.rerun_list = b->rerun_list(); m.a.rerun_count = b->counters() + kSharedCount;
    m.a.job_list = nullptr; m.a.n_dyn = nullptr;
    m.a.ph2pr = c->d_ph2pr_f; m.a.mm = c->d_mm_f; m.a.ph2pr_div3 = c->d_div3_f; m.a.gap_ratio = c->d_ratio_f;
    m.n_bins = (uint32_t)set.size();
    size_t book = set[0];
    uint64_t cells = 0, bytes = 0;
    for (size_t q = 0; q < set.size(); ++q) {
        const Bin& bn = b->bins[set[q]];
        m.job_first[q] = bn.job_begin; m.job_count[q] = bn.job_count; m.lds_stride[q] = bn.lds_stride;
        m.G[q] = (uint8_t)bn.G; m.RPL[q] = (uint8_t)bn.RPL; m.bin[q] = (uint8_t)set[q];
        if (bn.cells > b->bins[book].cells) book = set[q];
        cells += bn.cells; bytes += bn.alg_bytes;
        r.in_multi[set[q]] = 1;
        b->acct_cells[set[q]] = 0; b->acct_bytes[set[q]] = 0;
    }
    memcpy(m.block_first, ms.block_first, sizeof m.block_first);
    b->acct_cells[book] = cells; b->acct_bytes[book] = bytes; b->acct_multi[book] = (int8_t)(1 + gset);
    if (r.timing) for (size_t q : set) if (q != book) { HIP_TRY(hipEventRecord(r.ev[4 * q + 0], r.s)); HIP_TRY(hipEventRecord(r.ev[4 * q + 1], r.s)); }
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * book + 0], r.s));
    if (gset == 0) hipLaunchKernelGGL(pairhmm_fwd_multi<0>, dim3(ms.block_first[set.size()]), dim3(64), ms.lds, r.s, m);
    else           hipLaunchKernelGGL(pairhmm_fwd_multi<1>, dim3(ms.block_first[set.size()]), dim3(64), ms.lds, r.s, m);
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * book + 1], r.s));
    return 0;
}

// Several small narrow classes: one multi-class launch per lane-width set instead of one launch per class (multi_set,
// pairhmm_plan.h).  MGX_PAIRHMM_MULTI=0 keeps the per-class launches; any other value is the default.
int launch_multi_classes(Run& r) {
    mgx_pairhmm_batch* b = r.b;
    static const bool multi_ok = [] { const char* e = getenv("MGX_PAIRHMM_MULTI"); return !e || atoi(e) != 0; }();
    r.in_multi.assign(b->bins.size(), 0);
    b->acct_cells.assign(b->bins.size(), 0); b->acct_bytes.assign(b->bins.size(), 0); b->acct_multi.assign(b->bins.size(), 0);
    for (size_t k = 0; k < b->bins.size(); ++k) { b->acct_cells[k] = b->bins[k].cells; b->acct_bytes[k] = b->bins[k].alg_bytes; }
    if (!multi_ok || r.force_f64) return 0;
    for (int gset = 0; gset < 2; ++gset) {
        const MultiSet ms = multi_set(b->bins, gset, r.c->n_cu);
        if (ms.members.empty()) continue;
        if (const int rc = launch_multi(r, gset, ms)) return rc;
    }
    return 0;
}

// class k: its fp32 launch unless a multi-class launch has done it, then the fp64 re-run of its own list
// (the narrow classes share one, launch_shared_f64)
int launch_class(Run& r, size_t k) {
    mgx_pairhmm* c = r.c; mgx_pairhmm_batch* b = r.b;
    hipEvent_t* ev = r.ev;
    const Bin& bin = b->bins[k];
    const bool shared = is_narrow(bin) && !r.force_f64;
    KernelArgs a = r.base;
    if (bin.strip) {
        a.strip_stride = (bin.max_h + 63u) & ~63u;
        if (const int rc = ensure_strip_scratch(c, (size_t)bin.grid_f32 * 6u * a.strip_stride * sizeof(double))) return rc;
        a.strip_scratch = c->strip.p;
    }
    a.rerun_list = shared ? b->rerun_list() : b->rerun_list() + bin.job_begin;
    a.rerun_count = b->counters() + (shared ? kSharedCount : (int)k);
    a.lds_stride = bin.lds_stride;
    a.job_first = bin.job_begin;
    a.nhap_list = b->dev<uint32_t>(b->lay.nlist) + bin.job_begin;
    a.nhap_count = b->counters() + kNhapCount + (int)k;
    if (!r.force_f64) {
        // four code columns first (the strip-mined class: five), then the class's N-haplotype list with five; both
        // append their underflows to the same fp64 list.  A multi-class launch has done the first of the two.
        a.ph2pr = c->d_ph2pr_f; a.mm = c->d_mm_f; a.ph2pr_div3 = c->d_div3_f; a.gap_ratio = c->d_ratio_f;
        const bool first = !r.in_multi[k];
        if (first) {
            a.job_list = nullptr; a.n_dyn = nullptr; a.n_static = bin.job_count;
            KernelFn f = bin.strip ? (KernelFn)pairhmm_fwd_strip<float> : pick_kernel<float, 4>(bin.G, bin.RPL);
            if (!f) { set_error("no fp32 kernel for G=%d RPL=%d", bin.G, bin.RPL); return -ENOSYS; }
            if (r.timing) HIP_TRY(hipEventRecord(ev[4 * k + 0], r.s));
            hipLaunchKernelGGL(f, dim3(bin.grid_f32), dim3(bin.block), lds_bytes(bin, true, bin.strip ? kMaxCodes : 4), r.s, a);
        }
        if (!bin.strip) {
            KernelFn f5 = pick_kernel<float, kMaxCodes>(bin.G, bin.RPL);
            if (!f5) { set_error("no fp32 kernel for G=%d RPL=%d", bin.G, bin.RPL); return -ENOSYS; }
            a.job_list = a.nhap_list; a.n_dyn = a.nhap_count; a.n_static = 0;
            hipLaunchKernelGGL(f5, dim3(bin.grid_nhap), dim3(bin.block), lds_bytes(bin, true, kMaxCodes), r.s, a);
        }
        if (r.timing && first) HIP_TRY(hipEventRecord(ev[4 * k + 1], r.s));
    }
    const bool books_shared = shared && k == r.narrow.first;      // the shared launch is booked on the first narrow class
    if (r.timing && !books_shared) HIP_TRY(hipEventRecord(ev[4 * k + 2], r.s));
    if (!shared) {
        if (r.force_f64) { a.job_list = nullptr; a.n_dyn = nullptr; a.n_static = bin.job_count; }
        else { a.job_list = a.rerun_list; a.n_dyn = a.rerun_count; a.n_static = 0; }
        const int rc = launch_f64(r, a, bin.Gd, bin.RPLd, r.force_f64 ? bin.grid_f64_all : bin.grid_f64, bin.block, lds_bytes(bin, false));
        if (rc) return rc;
    }
    if (r.timing && !books_shared) HIP_TRY(hipEventRecord(ev[4 * k + 3], r.s));
    return 0;
}

// every class on the compute stream, largest first
int launch_classes(Run& r) {
    for (size_t k : class_order(r.b->bins))
        if (const int rc = launch_class(r, k)) return rc;
    return 0;
}

// the narrow classes' shared re-run list in one fp64 launch
int launch_shared_f64(Run& r) {
    const NarrowExtent& nw = r.narrow;
    if (!nw.n_jobs || r.force_f64) return 0;
    KernelArgs a = r.base;
    a.job_list = r.b->rerun_list(); a.n_dyn = r.b->counters() + kSharedCount; a.n_static = 0; a.job_first = 0;
    a.lds_stride = hap_stride(nw.max_h, 16);
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * nw.first + 2], r.s));
    const uint32_t grid = std::min<uint32_t>((nw.n_jobs + 3) / 4, (uint32_t)r.c->n_cu * 8u);      // 16 lanes: four test cases per workgroup
    if (const int rc = launch_f64(r, a, 16, (int)((nw.rows + 15) / 16), grid, 64, 4u * a.lds_stride)) return rc;
    if (r.timing) HIP_TRY(hipEventRecord(r.ev[4 * nw.first + 3], r.s));
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
    a.job_list = b->rerun_list() + b->n_pairs; a.n_dyn = b->counters() + kExactCount; a.n_static = 0; a.job_first = 0;
    a.rerun_list = nullptr; a.rerun_count = nullptr;
    a.lds_stride = hap_stride(max_h, 64);
    a.strip_stride = (max_h + 63u) & ~63u;
    const size_t per_wg = 6u * (size_t)a.strip_stride * sizeof(double);
    const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)b->n_pairs, (size_t)c->n_cu * 2u, (size_t)(256u << 20) / per_wg}));
    if (const int rc = ensure_strip_scratch(c, (size_t)grid * per_wg)) return rc;
    a.strip_scratch = c->strip.p;
    hipLaunchKernelGGL(pairhmm_fwd_exact, dim3(grid), dim3(64), a.lds_stride, r.s, a);
    return 0;
}

// whole-region batches: normalise / filter every read's row of the output
void launch_epilogue(Run& r) {
    const mgx_pairhmm_batch* b = r.b;
    if (!b->lay.model) return;
    hipLaunchKernelGGL(pairhmm_normalize_filter_rows, dim3(((uint32_t)b->lay.n_reads + 3) / 4), dim3(256), 0, r.s, b->dev<double>(b->lay.o_out), b->dev<uint64_t>(b->lay.rlen),
                       b->dev<uint32_t>(b->lay.roff), b->dev<uint32_t>(b->lay.rnh), (uint32_t)b->lay.n_reads, b->log10_rate, b->max_err, b->dev(b->lay.o_keep));
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
    r.narrow = survey_narrow(b->bins);
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
    if ((b->lay.read_bytes && (!bases || !qual || !ins || !del || !gcp)) || (b->lay.hap_bytes && !hap)) { set_error("NULL argument"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (b->n_pairs == 0) return 0;
    if (b->uploaded) HIP_TRY(hipEventSynchronize(b->uploaded));      // the copy and, in the wire form, the expansion behind it
    uint8_t* const host[kSeqArrays] = {bases, qual, ins, del, gcp, hap};
    for (int k = 0; k < kSeqArrays; ++k) {
        const uint64_t len = k == kSeqHap ? b->lay.hap_bytes : b->lay.read_bytes;
        if (len) HIP_TRY(hipMemcpy(host[k], b->dev(b->lay.seq[k]), len, hipMemcpyDeviceToHost));
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
    st.n_form_deferred_f32 = 0;
    if (b->ran && b->n_pairs) {
        std::vector<uint32_t> cnt(kCounters);
        HIP_TRY(hipMemcpy(cnt.data(), b->counters(), kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < b->bins.size(); ++k) st.n_nhap_f32 += cnt[kNhapCount + k];
        st.n_form_deferred_f32 = cnt[kFormDeferCount];      // on the same lists, without an N
        st.n_nhap_f32 -= st.n_form_deferred_f32;
        for (size_t k = 0; k < b->bins.size(); ++k) st.n_rerun_f64 += force_f64 ? b->bins[k].job_count : cnt[k];
        if (!force_f64) st.n_rerun_f64 += cnt[kSharedCount];          // the narrow classes' shared list
        st.n_exact = cnt[kExactCount];
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
        st.dominant_cells = cells_of(dom);
        st.dominant_alg_bytes = acct ? b->acct_bytes[dom] : b->bins[dom].alg_bytes;
        if (force_f64) {
            // every class in its own fp64 launch (launch_class): no fp32 time
            if (b->bins[dom].strip) snprintf(st.dominant_kernel, sizeof st.dominant_kernel, "pairhmm_fwd_strip<double>");
            else snprintf(st.dominant_kernel, sizeof st.dominant_kernel, "pairhmm_fwd<double, %d, %d>", b->bins[dom].Gd, b->bins[dom].RPLd);
        } else {
            st.ms_f32_dominant = (float)(domms / n_sets);
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
    HIP_TRY(hipMemcpyAsync(b->slab.pin + b->lay.o_out, b->dev<double>(b->lay.o_out), bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// The results of a batch made of regions [g0, g1) (base: every region's first test case in the batch, as create_cross
// returns it), out of the pinned mirror into the caller's array of each region; keep may be NULL, and so may its entries.
void scatter_region_results(const mgx_pairhmm_batch* b, const std::vector<uint64_t>& base, const mgx_pairhmm_input_t* regions,
                            uint32_t g0, uint32_t g1, double* const* out, uint8_t* const* keep) {
    const double* all = (const double*)(b->slab.pin + b->lay.o_out);
    const uint8_t* kept = b->slab.pin + b->lay.o_keep;
    uint64_t r_at = 0;
    for (uint32_t g = g0; g < g1; ++g) {
        const uint64_t a = base[g - g0], e = base[g - g0 + 1];
        if (e > a) memcpy(out[g], all + a, (e - a) * sizeof(double));
        if (keep && keep[g] && e > a) memcpy(keep[g], kept + r_at, regions[g].n_reads);
        r_at += regions[g].n_reads;
    }
}

// every region of a whole-region call: valid, in the cross-product form, with an output if it holds test cases (total: of the call;
// out_log10 == nullptr: a call without outputs per test case)
static int validate_regions(uint32_t n_regions, const mgx_pairhmm_input_t* regions, double* const* out_log10, uint64_t* total) {
    *total = 0;
    for (uint32_t g = 0; g < n_regions; ++g) {
        if (const int rc = validate(&regions[g])) return rc;
        if (regions[g].pair_read || regions[g].pair_hap) { set_error("region %u: regions are given in the cross-product form (pair arrays NULL)", g); return -EINVAL; }
        const uint64_t n = regions[g].n_reads * regions[g].n_haps;
        if (n && out_log10 && !out_log10[g]) { set_error("region %u: output pointer is NULL", g); return -EINVAL; }
        *total += n;
    }
    return 0;
}

// ---- a stream of batches through lanes: mgx_pairhmm_compute_regions is one lane on the caller's context, the host work
// queue (below) several, each a host thread with a context of its own
struct LaneStats {
    double pack_s = 0, wait_s = 0;
    uint64_t batches = 0, bytes_h2d = 0, bytes_d2h = 0, cells = 0;
};

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
    int result() const { if (rc) set_error("%s", err.c_str()); return rc; }      // on the caller's thread, after the lanes have ended
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One lane on context c: at most `depth` batches in flight, pair-stream batches of batch_pairs test cases.  Per batch:
// retire the slot's previous batch, create, run; at the end the slots are retired oldest first.
static void run_lane(mgx_pairhmm* c, uint32_t depth, uint32_t batch_pairs, QueueRun* run, LaneStats* ln) {
    struct Slot { mgx_pairhmm_batch* b = nullptr; uint64_t lo = 0; uint32_t g0 = 0, g1 = 0; std::vector<uint64_t> base; };
    std::vector<Slot> slots(depth);
    mgx::PackPlan plan;
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
            sl.lo = run->lo + k * batch_pairs;
            const uint64_t hi = std::min(run->hi, sl.lo + batch_pairs);
            const uint64_t bad = mgx::pack_plan(run->in, sl.lo, hi, &plan);
            if (bad) { set_error("test case %llu: index out of range", (unsigned long long)(sl.lo + bad - 1)); run->fail(-EINVAL); break; }
            rc = create_pairs(c, run->in, &plan, b.get());
        }
        ln->pack_s += now_s() - t0;
        if (!rc && b->n_pairs) rc = mgx_pairhmm_batch_run(c, b.get());
        if (rc) { run->fail(rc); break; }
        if (!b->n_pairs) continue;                  // a chunk of empty regions
        ln->batches++; ln->bytes_h2d += b->lay.in_bytes; ln->cells += b->stats.cells;
        sl.b = b.release();
    }
    for (size_t j = 0; j < slots.size(); ++j) retire(slots[(turn + j) % slots.size()]);    // oldest first
}
}  // namespace

// The stages of a whole-region call (mgx_realign_internal.h): mgx_pairhmm_regions below runs them back to back, mgx_realign_regions
// (mgx_realign.hip) puts the best-haplotype and verbatim kernels between the run and the download.
extern "C++" {
namespace mgx_internal {
PairhmmView pairhmm_view(mgx_pairhmm_t* c) { return PairhmmView{c->device, c->flags, c->compute, c->d2h, &c->ext}; }

int regions_begin(mgx_pairhmm_t* c, uint32_t n_regions, const mgx_pairhmm_input_t* regions, const uint8_t* const* mapq,
                  const mgx_read_model_t* model, double* const* out_log10, RegionBatch* rb) {
    int rc;
    uint64_t total;
    if ((rc = validate_regions(n_regions, regions, out_log10, &total)) || total == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    BatchPtr b = new_batch();
    if (!b) return -ENOMEM;
    if ((rc = create_cross(c, n_regions, regions, b.get(), &rb->base, mapq, model))) return rc;
    if (b->n_pairs == 0) return 0;
    mgx_pairhmm_batch* raw = b.release();
    if ((rc = mgx_pairhmm_batch_run(c, raw))) { mgx_pairhmm_batch_destroy(c, raw); return rc; }
    rb->batch = raw; rb->n_pairs = raw->n_pairs; rb->n_reads = raw->lay.model ? (uint32_t)raw->lay.n_reads : 0;
    rb->d_bases = raw->dev(raw->lay.seq[kSeqBases]); rb->d_hap = raw->dev(raw->lay.seq[kSeqHap]); rb->d_keep = raw->dev(raw->lay.o_keep); rb->d_out = raw->dev<double>(raw->lay.o_out);
    rb->d_row_off = raw->dev<uint32_t>(raw->lay.roff); rb->d_row_nh = raw->dev<uint32_t>(raw->lay.rnh); rb->done = raw->done;
    return 0;
}

int regions_queue_download(mgx_pairhmm_t* c, const RegionBatch& rb, hipStream_t s) {
    const mgx_pairhmm_batch* b = rb.batch;
    if (s != c->compute) HIP_TRY(hipStreamWaitEvent(s, b->done, 0));
    HIP_TRY(hipMemcpyAsync(b->slab.pin + b->lay.o_out, b->dev<double>(b->lay.o_out), b->lay.result_bytes, hipMemcpyDeviceToHost, s));
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
        const int rc = fetch_results(c, b, used_f64 ? b->lay.o_used + b->n_pairs - b->lay.o_out : b->n_pairs * sizeof(double));
        if (rc) return rc;
        memcpy(out_log10, b->slab.pin + b->lay.o_out, b->n_pairs * sizeof(double));
        if (used_f64) memcpy(used_f64, b->slab.pin + b->lay.o_used, b->n_pairs);
        return 0;
    }
    hipStream_t s = c->d2h;
    if (b->done) HIP_TRY(hipStreamWaitEvent(s, b->done, 0));
    HIP_TRY(hipMemcpyAsync(out_log10, b->dev<double>(b->lay.o_out), b->n_pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (used_f64) HIP_TRY(hipMemcpyAsync(used_f64, b->dev(b->lay.o_used), b->n_pairs, hipMemcpyDeviceToHost, s));
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

int mgx_pairhmm_regions_modified_inputs(mgx_pairhmm_t* c, uint32_t n_regions, const mgx_pairhmm_input_t* regions, const uint8_t* const* mapq,
                                        const mgx_read_model_t* model, uint8_t* const* out_qual, uint8_t* const* out_ins, uint8_t* const* out_del,
                                        uint8_t* const* out_gcp) {
    if (!c || !model || (n_regions && (!regions || !mapq || !out_qual || !out_ins || !out_del || !out_gcp))) { set_error("NULL argument"); return -EINVAL; }
    int rc;
    uint64_t total;
    if ((rc = validate_regions(n_regions, regions, nullptr, &total)) || total == 0) return rc;
    uint8_t* const* const out[4] = {out_qual, out_ins, out_del, out_gcp};
    const int seq[4] = {kSeqQual, kSeqIns, kSeqDel, kSeqGcp};
    for (uint32_t g = 0; g < n_regions; ++g)      // every region with reads is staged and copied back, with or without haplotypes
        for (int k = 0; k < 4 && regions[g].n_reads; ++k)
            if (!out[k][g]) { set_error("region %u: output pointer is NULL", g); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    BatchPtr b = new_batch();
    if (!b) return -ENOMEM;
    std::vector<uint64_t> base;
    if ((rc = create_cross(c, n_regions, regions, b.get(), &base, mapq, model))) return rc;      // the upload and the read model, as regions_begin
    HIP_TRY(hipEventSynchronize(b->uploaded));
    uint64_t rb = 0;          // regions lie back to back in the batch's read arrays, each in the caller's read order (cross_stage)
    for (uint32_t g = 0; g < n_regions; ++g) {
        const uint64_t len = regions[g].n_reads ? regions[g].read_off[regions[g].n_reads] - regions[g].read_off[0] : 0;
        for (int k = 0; k < 4 && len; ++k) HIP_TRY(hipMemcpy(out[k][g], b->dev(b->lay.seq[seq[k]]) + rb, len, hipMemcpyDeviceToHost));
        rb += len;
    }
    mgx_pairhmm_batch_destroy(c, b.release());      // the slab goes back to the pool
    return 0;
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
    uint64_t total;
    if (const int rc = validate_regions(n_regions, regions, out_log10, &total)) return rc;
    if (total == 0) return 0;
    // runs of whole regions of region_chunk_pairs test cases (pairhmm_plan.h), two in flight: the queue's pipelining on the caller's thread
    uint64_t chunk_pairs = region_chunk_pairs(total);
    if (const char* e = getenv("MGX_PAIRHMM_REGION_CHUNK")) { const long long v = atoll(e); if (v > 0) chunk_pairs = (uint64_t)v; }      // A/B
    QueueRun run;
    run.regions = regions; run.region_out = out_log10;
    cut_regions(regions, n_regions, chunk_pairs, &run.chunk);
    run.n_batches = run.chunk.size() - 1;
    LaneStats st;
    run_lane(c, 2, 0, &run, &st);
    return run.result();
}

// ---------------------------------------------------------------------------------------------
// Host work queue (BASELINE.json configs[2]).  The reference's worker threads pull the next active
// region off one atomic index (deepmutect/Mutect2Cpp-master/src/main.cpp:254) and share the tail of the
// work at the end (main.cpp:302-315, IntelPairHmm.cc:296-330).  Here the unit pulled is a BATCH of test
// cases: every lane (run_lane) -- a host thread with its own context, i.e. its own streams and recycled pinned
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
        LaneStats st;
    };
    std::vector<Lane> lanes;
    uint32_t n_devices = 1, depth = 2, batch_pairs = 65536;
    mgx_pairhmm_queue_stats_t stats{};
};

namespace {

int queue_execute(mgx_pairhmm_queue* q, QueueRun& run, uint64_t n_pairs) {
    for (auto& ln : q->lanes) ln.st = LaneStats{};
    const double t0 = now_s();
    const size_t n_thr = (size_t)std::min<uint64_t>(q->lanes.size(), run.n_batches);
    std::vector<std::thread> th;
    for (size_t i = 1; i < n_thr; ++i) th.emplace_back(run_lane, q->lanes[i].ctx, q->depth, q->batch_pairs, &run, &q->lanes[i].st);
    run_lane(q->lanes[0].ctx, q->depth, q->batch_pairs, &run, &q->lanes[0].st);               // the caller's thread is lane 0
    for (auto& t : th) t.join();
    q->stats.seconds = now_s() - t0;
    q->stats.n_pairs = n_pairs;
    q->stats.n_batches = run.n_batches;
    for (auto& ln : q->lanes) {
        q->stats.cells += ln.st.cells; q->stats.bytes_h2d += ln.st.bytes_h2d; q->stats.bytes_d2h += ln.st.bytes_d2h;
        q->stats.pack_seconds += ln.st.pack_s; q->stats.wait_seconds += ln.st.wait_s;
        q->stats.batches_per_device[ln.dev_slot] += ln.st.batches;
    }
    return run.result();
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
    uint64_t total;
    if (const int rc = validate_regions(n_regions, regions, out_log10, &total)) return rc;
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
