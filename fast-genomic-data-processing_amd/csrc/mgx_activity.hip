// mgx_activity.hip -- Mutect2Engine::isActive for every locus of an interval (C ABI: include/mgx_activity.h; the rule: activity_rule.h).
//
// The reference walks each read's position map per (read, locus) inside a per-locus loop on host threads (M2/main.cpp:254-300).  Here the
// two halves are two launches on one stream:
//   k_pileup_elements  read-parallel, one wavefront per read: rule 1's byte for every position of the read's pileup window into a dense
//                      array (elem_off is the host's prefix over window lengths).  Lanes take consecutive positions; each finds its CIGAR
//                      element among 64 elements held one per lane (inclusive scan of the reference lengths, binary search by shuffle);
//                      a longer CIGAR goes round again.  Bases, qualities and the reference byte are read where they lie.
//   k_locus_activity   locus-parallel, one lane per locus, 64 consecutive loci per wavefront.  The reads that can cover the wavefront's
//                      loci are [lo, hi): hi = reads with act_start <= the last locus, lo = the first read whose running maximum of
//                      act_stop reaches the first locus, both by binary search in arrays that do not decrease.  The wavefront walks that
//                      range once to count and once more for the fp64 sum; each lane tests its own window and loads
//                      elem[elem_off[i] + p - act_start[i]], so neighbouring lanes read neighbouring bytes.
// No atomics, no order that depends on scheduling: a locus' sum runs over the reads that cover it in input order, whatever interval they
// were passed with.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

#include "../../include/mgx_activity.h"
#include "activity_rule.h"
#include "mgx_activity_internal.h"      // struct mgx_activity; HIP_TRY, Mirror
#include "mgx_tables.h"

using mgx::set_error;
using mgx_hip::Mirror;
namespace R = mgx_activity_rule;

namespace {
typedef uint8_t u8; typedef uint32_t u32; typedef uint64_t u64;

// one read of k_pileup_elements: where its elements, bases and qualities lie in the upload, and its window's first byte in elem
struct ReadJob { u64 base_at; u32 cigar_at, n_cigar; int32_t read_start, act_start, act_stop, mate_start; u32 elem_off, n_bases, flags, pad_; };
// one read of k_locus_activity
struct Window { int32_t act_start, act_stop; u32 elem_off, sample; };
static_assert(sizeof(ReadJob) == 48 && sizeof(Window) == 16, "table entries");

__device__ __forceinline__ u32 wave_scan_inclusive(u32 v, u32 lane) {
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) { const u32 o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}

// 64 elements of a read from k on, one per lane: the inclusive ends of their reference and read spans within the chunk
__device__ __forceinline__ void scan_chunk(const u32* cg, u32 n_cigar, u32 k, u32 lane, u32* ref_end, u32* read_end) {
    const u32 el = k + lane < n_cigar ? cg[k + lane] : 0u;
    *ref_end = wave_scan_inclusive(R::ref_len(el), lane);
    *read_end = wave_scan_inclusive(R::read_len(el), lane);
}

__global__ __launch_bounds__(256) void k_pileup_elements(const ReadJob* __restrict__ jobs, const u32* __restrict__ cigar, const u8* __restrict__ bases,
                                                         const u8* __restrict__ quals, const u8* __restrict__ ref, int32_t interval_start,
                                                         u32 n_loci, u32 n_reads, R::ElementParams P, u8* __restrict__ elem) {
    const u32 r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const u32 lane = threadIdx.x & 63;
    if (r >= n_reads) return;
    const ReadJob J = jobs[r];
    if (J.act_stop < J.act_start) return;
    const u32* cg = cigar + J.cigar_at;
    const R::Read rd{cg, J.n_cigar, bases + J.base_at, quals + J.base_at, J.n_bases, J.read_start, J.mate_start, (uint16_t)J.flags};
    const u32 n_pos = (u32)(J.act_stop - J.act_start) + 1;
    u32 ref_end0, read_end0;
    scan_chunk(cg, J.n_cigar, 0, lane, &ref_end0, &read_end0);
    for (u32 at = 0; at < n_pos; at += 64) {
        const bool on = at + lane < n_pos;
        const int32_t pos = J.act_start + (int32_t)(on ? at + lane : 0);
        const u32 rel = (u32)(pos - J.read_start);
        u32 ref_end = ref_end0, read_end = read_end0, ref_base = 0, read_base = 0;
        R::Where w{0, 0, 0};
        bool found = false;
        for (u32 k = 0;; k += 64) {                     // every lane runs every shuffle
            if (k) {
                scan_chunk(cg, J.n_cigar, k, lane, &ref_end, &read_end);
                ref_end += ref_base; read_end += read_base;
            }
            const u32 j = R::first_end_above([&](u32 l) { return (u32)__shfl((int)ref_end, (int)l); }, rel);
            const int before = j == 0 || j == 64 ? 0 : (int)j - 1;
            const u32 ref_before = (u32)__shfl((int)ref_end, before), read_before = (u32)__shfl((int)read_end, before);
            if (!found && j < 64) { found = true; w = R::Where{k + j, j ? ref_before : ref_base, j ? read_before : read_base}; }
            ref_base = (u32)__shfl((int)ref_end, 63); read_base = (u32)__shfl((int)read_end, 63);
            if (__ballot(!found) == 0 || k + 64 >= J.n_cigar) break;
        }
        if (!on) continue;
        const int64_t l = (int64_t)pos - interval_start;                    // outside the interval no reference byte exists and no locus reads the element
        u8 b = 0;
        if (found && l >= 0 && l < (int64_t)n_loci) b = R::element_byte(rd, w, pos, ref[l], P);
        elem[J.elem_off + at + lane] = b;
    }
}

__global__ __launch_bounds__(256) void k_locus_activity(const Window* __restrict__ win, const int32_t* __restrict__ run_max_stop, u32 n_reads,
                                                        const u8* __restrict__ elem, int32_t interval_start, u32 n_loci, R::Tables T,
                                                        R::LocusParams P, u32 max_depth, u8* __restrict__ out_active,
                                                        double* __restrict__ out_log_odds, u32* __restrict__ out_depth, u32* __restrict__ too_deep) {
    const u32 l0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + (threadIdx.x >> 6)) * 64);
    const u32 lane = threadIdx.x & 63;
    if (l0 >= n_loci) return;
    const u32 l = l0 + lane;
    const bool on = l < n_loci;
    const int32_t p_first = interval_start + (int32_t)l0, p_last = interval_start + (int32_t)(l0 + 63 < n_loci ? l0 + 63 : n_loci - 1);
    u32 lo = 0, hi = 0;
    for (u32 b = n_reads; lo < b;) { const u32 m = lo + (b - lo) / 2; if (run_max_stop[m] < p_first) lo = m + 1; else b = m; }
    for (u32 b = n_reads; hi < b;) { const u32 m = hi + (b - hi) / 2; if (win[m].act_start <= p_last) hi = m + 1; else b = m; }
    const int32_t p = interval_start + (int32_t)l;
    // f(sample, byte) for every read whose window holds the lane's locus, in input order
    const auto walk = [&](auto f) __attribute__((always_inline)) {
        for (u32 i = lo; i < hi; ++i) {
            const Window W = win[i];
            if (on && W.act_start <= p && p <= W.act_stop) f(W.sample, elem[W.elem_off + (u32)(p - W.act_start)]);
        }
    };
    R::Counts c{0, 0, 0, 0, 0};
    walk([&](u32 sample, u8 b) __attribute__((always_inline)) { R::count(c, sample, b); });
    double sum = 0;
    if (R::has_sum(c, max_depth)) {
        const double f_tilde = R::f_tilde_ratio(T, c.tumour - c.alt, c.alt);
        walk([&](u32 sample, u8 b) __attribute__((always_inline)) { if (sample == 0 && b) sum += R::alt_term(T, b, f_tilde); });
    }
    const R::Locus L = R::locus_of(T, P, c, max_depth, sum);
    if (!on) return;
    out_active[l] = L.active; out_log_odds[l] = L.log_odds; out_depth[l] = L.depth;
    if (L.depth > max_depth) *too_deep = 1;          // every writer stores the same value
}

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

namespace {

// ---- before anything is launched: the arguments, and per read its spans and its window
struct Checked { u64 n_elements, n_cigar, n_bases; };
int check(const mgx_activity_input_t* in, const mgx_activity_params_t* p, bool has_out_active, Checked* c) {
    if (!in || !p || (in->n_loci && (!has_out_active || !in->ref_bases))) { set_error("NULL argument"); return -EINVAL; }
    const u64 n = in->n_reads;
    if (n && (!in->read_start || !in->cigar_off || !in->base_off || !in->flags || !in->mate_start || !in->sample || !in->act_start || !in->act_stop)) { set_error("NULL array"); return -EINVAL; }
    if (p->pcr_error_qual < 2 || p->pcr_error_qual > 254 || p->min_base_quality < 0 || p->min_base_quality > 127) { set_error("pcr_error_qual must lie in 2..254 and min_base_quality in 0..127"); return -EINVAL; }
    if (in->interval_start < 0 || (u64)in->interval_start + in->n_loci > (1ull << 31)) { set_error("the interval ends beyond 2^31"); return -E2BIG; }
    if (n > 0x7FFFFFF0ull) { set_error("more than 2^31 reads in one call"); return -E2BIG; }
    *c = Checked{0, 0, 0};
    if (n == 0) return 0;
    for (u64 r = 0; r < n; ++r)
        if (in->cigar_off[r + 1] < in->cigar_off[r] || in->base_off[r + 1] < in->base_off[r]) { set_error("read %llu: offsets decrease", (unsigned long long)r); return -EINVAL; }
    c->n_cigar = in->cigar_off[n] - in->cigar_off[0]; c->n_bases = in->base_off[n] - in->base_off[0];
    if (c->n_cigar >= (1ull << 32)) { set_error("2^32 CIGAR elements or more"); return -E2BIG; }
    if ((c->n_cigar && !in->cigar) || (c->n_bases && (!in->bases || !in->quals))) { set_error("NULL array"); return -EINVAL; }
    for (u64 r = 0; r < n; ++r) {
        const unsigned long long R_ = r;
        u64 ref_span = 0, read_span = 0;
        for (u64 k = in->cigar_off[r]; k < in->cigar_off[r + 1]; ++k) {
            const u32 el = in->cigar[k], op = el & 15;
            if (op > 8 || op == R::kOpN) { set_error("read %llu: element %llu has operator code %u", R_, (unsigned long long)(k - in->cigar_off[r]), op); return -EINVAL; }
            if ((el >> 4) == 0) { set_error("read %llu: element %llu has length 0", R_, (unsigned long long)(k - in->cigar_off[r])); return -EINVAL; }
            ref_span += R::ref_len(el); read_span += R::read_len(el);
        }
        if (read_span != in->base_off[r + 1] - in->base_off[r]) { set_error("read %llu: its CIGAR covers %llu bases, the read has %llu", R_, (unsigned long long)read_span, (unsigned long long)(in->base_off[r + 1] - in->base_off[r])); return -EINVAL; }
        if (in->read_start[r] < 0 || (u64)in->read_start[r] + ref_span > (1ull << 31)) { set_error("read %llu ends beyond 2^31 or starts below 0", R_); return -E2BIG; }
        if (in->sample[r] > 1) { set_error("read %llu: sample %u", R_, in->sample[r]); return -EINVAL; }
        if (r && in->act_start[r] < in->act_start[r - 1]) { set_error("read %llu: act_start decreases", R_); return -EINVAL; }
        if (in->act_stop[r] >= in->act_start[r]) {
            if (in->act_start[r] < in->read_start[r] || (u64)in->act_stop[r] >= (u64)in->read_start[r] + ref_span) { set_error("read %llu: its window leaves its reference span", R_); return -EINVAL; }
            c->n_elements += (u64)((int64_t)in->act_stop[r] - in->act_start[r] + 1);
        }
    }
    for (u64 k = in->base_off[0]; k < in->base_off[n]; ++k) if (in->quals[k] > 127) { set_error("quality %u above 127", in->quals[k]); return -EINVAL; }
    if (c->n_elements >= (1ull << 32)) { set_error("2^32 pileup elements or more"); return -E2BIG; }
    return 0;
}

// ---- the host prefixes and the caller's arrays into the pinned mirror, one upload
struct Layout { size_t o_win, o_max, o_cigar, o_bases, o_quals, o_ref, bytes; };
int stage(mgx_activity* c, const mgx_activity_input_t* in, const Checked& k, Layout* L) {
    const u64 n = in->n_reads;
    L->o_win = up256(n * sizeof(ReadJob)); L->o_max = L->o_win + up256(n * sizeof(Window)); L->o_cigar = L->o_max + up256(n * 4);
    L->o_bases = L->o_cigar + up256(k.n_cigar * 4); L->o_quals = L->o_bases + up256(k.n_bases); L->o_ref = L->o_quals + up256(k.n_bases);
    L->bytes = L->o_ref + up256(in->n_loci);
    if (int rc = c->up.reserve(L->bytes)) return rc;
    u8* pin = c->up.pin;
    ReadJob* jobs = (ReadJob*)pin; Window* win = (Window*)(pin + L->o_win); int32_t* run_max = (int32_t*)(pin + L->o_max);
    u32 elem_off = 0;
    int32_t top = INT32_MIN;
    for (u64 r = 0; r < n; ++r) {
        const bool empty = in->act_stop[r] < in->act_start[r];
        jobs[r] = ReadJob{in->base_off[r] - in->base_off[0], (u32)(in->cigar_off[r] - in->cigar_off[0]), (u32)(in->cigar_off[r + 1] - in->cigar_off[r]),
                          in->read_start[r], in->act_start[r], in->act_stop[r], in->mate_start[r], elem_off, (u32)(in->base_off[r + 1] - in->base_off[r]),
                          in->flags[r], 0};
        win[r] = Window{in->act_start[r], in->act_stop[r], elem_off, in->sample[r]};
        if (!empty) { top = in->act_stop[r] > top ? in->act_stop[r] : top; elem_off += (u32)(in->act_stop[r] - in->act_start[r]) + 1; }
        run_max[r] = top;
    }
    if (k.n_cigar) memcpy(pin + L->o_cigar, in->cigar + in->cigar_off[0], k.n_cigar * 4);
    if (k.n_bases) { memcpy(pin + L->o_bases, in->bases + in->base_off[0], k.n_bases); memcpy(pin + L->o_quals, in->quals + in->base_off[0], k.n_bases); }
    memcpy(pin + L->o_ref, in->ref_bases, in->n_loci);
    return 0;
}

}  // namespace

// validate -> host prefixes and the inputs into one pinned buffer -> one upload -> two launches on c->stream; nothing is downloaded
int mgx_activity_launch_loci(mgx_activity* c, const mgx_activity_input_t* in, const mgx_activity_params_t* p, bool has_out_active, mgx_activity_loci* o) {
    if (!c) { set_error("NULL argument"); return -EINVAL; }
    c->stats = mgx_activity_stats_t{};
    *o = mgx_activity_loci{};
    // 1. validate
    Checked k;
    if (int rc = check(in, p, has_out_active, &k)) return rc;
    const u32 n_loci = in->n_loci, n_reads = (u32)in->n_reads;
    c->stats.n_loci = n_loci; c->stats.n_elements = k.n_elements;
    if (n_loci == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // 2. host prefixes and the inputs into one pinned buffer
    Layout L;
    if (int rc = stage(c, in, k, &L)) return rc;
    const size_t o_depth = up256((size_t)n_loci * 8), o_active = o_depth + up256((size_t)n_loci * 4), o_deep = o_active + up256(n_loci), down_bytes = o_deep + 256;
    if (int rc = c->down.reserve(down_bytes)) return rc;
    if (int rc = c->elem.reserve(k.n_elements, k.n_elements + k.n_elements / 4 + 256)) return rc;
    // 3. one upload
    hipStream_t s = c->stream;
    const bool timing = (p->flags & MGX_PAIRHMM_TIMING) != 0;
    u8* up = c->up.dev; u8* down = c->down.dev;
    HIP_TRY(hipMemcpyAsync(up, c->up.pin, L.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(down + o_deep, 0, 4, s));
    // 4. two launches on one stream
    if (timing) HIP_TRY(hipEventRecord(c->ev[0], s));
    if (k.n_elements) {
        hipLaunchKernelGGL(k_pileup_elements, dim3((n_reads + 3) / 4), dim3(256), 0, s, (const ReadJob*)up, (const u32*)(up + L.o_cigar), up + L.o_bases,
                           up + L.o_quals, up + L.o_ref, in->interval_start, n_loci, n_reads, R::ElementParams{p->pcr_error_qual, p->min_base_quality}, c->elem.p);
        c->stats.n_launches++;
    }
    if (timing) HIP_TRY(hipEventRecord(c->ev[1], s));
    const u32 n_counts = c->max_depth + 3;
    const R::Tables T{c->d_tables, c->d_tables + n_counts, c->d_tables + 2 * (size_t)n_counts, c->d_tables + 2 * (size_t)n_counts + 128, c->d_tables + 2 * (size_t)n_counts + 256};
    hipLaunchKernelGGL(k_locus_activity, dim3((n_loci + 255) / 256), dim3(256), 0, s, (const Window*)(up + L.o_win), (const int32_t*)(up + L.o_max), n_reads,
                       c->elem.p, in->interval_start, n_loci, T, R::LocusParams{p->has_normal, p->genotype_germline_sites, p->initial_log_odds}, c->max_depth,
                       down + o_active, (double*)down, (u32*)(down + o_depth), (u32*)(down + o_deep));
    c->stats.n_launches++;
    c->n_elem = k.n_elements;
    if (timing) HIP_TRY(hipEventRecord(c->ev[2], s));
    HIP_TRY(hipGetLastError());
    *o = mgx_activity_loci{n_loci, o_depth, o_active, o_deep, down_bytes};
    return 0;
}

// 5. one download: everything (`all`), or the depth flag alone; the outputs that were asked for.  n_active and n_callable are counted on the
// host from the download, so they stay 0 without it.
int mgx_activity_collect_loci(mgx_activity* c, const mgx_activity_loci& o, const mgx_activity_params_t* p, bool all, u8* out_active, double* out_log_odds,
                              u32* out_depth) {
    if (o.n_loci == 0) return 0;
    hipStream_t s = c->stream;
    const bool timing = (p->flags & MGX_PAIRHMM_TIMING) != 0;
    if (all) HIP_TRY(hipMemcpyAsync(c->down.pin, c->down.dev, o.down_bytes, hipMemcpyDeviceToHost, s));
    else HIP_TRY(hipMemcpyAsync(c->down.pin + o.o_deep, c->down.dev + o.o_deep, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (timing) { HIP_TRY(hipEventElapsedTime(&c->stats.ms_elements, c->ev[0], c->ev[1])); HIP_TRY(hipEventElapsedTime(&c->stats.ms_locus, c->ev[1], c->ev[2])); }
    const u8* pin = c->down.pin;
    if (*(const u32*)(pin + o.o_deep)) { set_error("a locus is deeper than max_depth %u", c->max_depth); return -E2BIG; }
    if (!all) return 0;
    const u32* depth = (const u32*)(pin + o.o_depth);
    for (u32 l = 0; l < o.n_loci; ++l) { c->stats.n_active += pin[o.o_active + l]; c->stats.n_callable += (int64_t)depth[l] > (int64_t)p->min_callable_depth; }
    if (out_active) memcpy(out_active, pin + o.o_active, o.n_loci);
    if (out_log_odds) memcpy(out_log_odds, pin, (size_t)o.n_loci * 8);
    if (out_depth) memcpy(out_depth, depth, (size_t)o.n_loci * 4);
    return 0;
}

extern "C" {

int mgx_activity_create(int device, uint32_t max_depth, mgx_activity_t** out) {
    if (!out) { set_error("out is NULL"); return -EINVAL; }
    *out = nullptr;
    if (const int rc = mgx_hip::pick_device(&device, nullptr)) return rc;
    if (max_depth == 0) max_depth = MGX_ACTIVITY_DEFAULT_MAX_DEPTH;
    if (max_depth > (1u << 24)) { set_error("max_depth above 2^24"); return -E2BIG; }
    std::unique_ptr<mgx_activity> c(new (std::nothrow) mgx_activity);
    if (!c) return -ENOMEM;
    c->device = device; c->max_depth = max_depth;
    mgx_hip::Owner& m = c->own;
    m.stream(&c->stream);
    for (auto& e : c->ev) m.event(&e);
    mgx::ActivityTables t;
    const u32 n_counts = max_depth + 3;
    mgx::build_activity_tables(n_counts, &t);
    if (!m.device(&c->d_tables, (2 * (size_t)n_counts + 3 * 128) * sizeof(double))) return m.error("an activity context");
    HIP_TRY(hipMemcpy(c->d_tables, t.digamma.data(), n_counts * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_tables + n_counts, t.log10_factorial.data(), n_counts * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_tables + 2 * (size_t)n_counts, t.eps, 128 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_tables + 2 * (size_t)n_counts + 128, t.log_eps, 128 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_tables + 2 * (size_t)n_counts + 256, t.log_one_minus_eps, 128 * sizeof(double), hipMemcpyHostToDevice));
    *out = c.release();
    return 0;
}

void mgx_activity_destroy(mgx_activity_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

void mgx_activity_params_defaults(mgx_activity_params_t* p) {
    if (p) *p = mgx_activity_params_t{0, 0, 10, 40, 6, 0u, 4.605170185988092};
}

int mgx_activity_interval(mgx_activity_t* c, const mgx_activity_input_t* in, const mgx_activity_params_t* p, uint8_t* out_active,
                          double* out_log_odds, uint32_t* out_depth) {
    mgx_activity_loci o;
    if (int rc = mgx_activity_launch_loci(c, in, p, out_active != nullptr, &o)) return rc;
    return mgx_activity_collect_loci(c, o, p, true, out_active, out_log_odds, out_depth);
}

int mgx_activity_stats(mgx_activity_t* c, mgx_activity_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = c->stats;
    return 0;
}

int mgx_activity_last_elements(mgx_activity_t* c, uint8_t* out, uint64_t n) {
    if (!c || (n && !out)) { set_error("NULL argument"); return -EINVAL; }
    if (n != c->n_elem) { set_error("the last call wrote %llu elements, not %llu", (unsigned long long)c->n_elem, (unsigned long long)n); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (n) HIP_TRY(hipMemcpy(out, c->elem.p, n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
