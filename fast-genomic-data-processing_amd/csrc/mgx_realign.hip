// mgx_realign.hip -- realignReadsToTheirBestHaplotype in one device call (C ABI: include/mgx_realign.h).
//
// The reference runs computeReadLikelihoods, then per read bestAllelesBreakingTies and createReadAlignedToRef's aligner call
// (M2/Mutect2Engine.cpp:223-231).  Here the PairHMM batch stays in HBM between the two: the best haplotype of every read
// (pairhmm_best_allele_rows, pairhmm_kernels.hip.inc) and SWNativeAlignerWrapper's verbatim shortcut (k_realign_verbatim) run behind
// the PairHMM epilogue, 9 bytes per read come back, and the reads that still need the aligner are gathered out of the batch's slab
// into the Smith-Waterman context's sequence arrays (k_realign_gather) instead of being assembled and uploaded by the host.
//   * Mutect2Utils::lastIndexOf (Mutect2Utils.cpp:69-82): the LAST verbatim occurrence, bytes compared as the aligner compares them.
//   * The aligner's jobs derive their score and element offsets from the sequence offsets (sw_layout.h: sc_off = off1 + off2 + 2q),
//     so its sequences must be dense and in pair order: hence a gather, not pointers into the slab.
//   * Region batches upload the caller's bytes unchanged (the wire form is for staged pair lists only): the slab's bases are the caller's.
//   * createReadAlignedToRef behind the aligner call (read -> reference CIGAR and start, read_to_ref_rule.h) is k_read_to_ref: one
//     wavefront per read runs the rule wave-uniform on what already lies in HBM (read bases, the reference haplotype's bases);
//     only the CIGAR tables go up and the element rows come down.
// The two contexts' internals are reached through mgx_realign_internal.h; both keep their own code paths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/mgx_realign.h"
#include "mgx_hip_util.h"      // HIP_TRY
#include "mgx_realign_internal.h"
#include "pairhmm_pack.h"
#include "read_to_ref_rule.h"
#include "sw_trace_rule.h"

using mgx::set_error;
using mgx_hip::Mirror;
using namespace mgx_internal;

namespace {
typedef uint8_t u8; typedef uint32_t u32; typedef uint64_t u64;

// per read, in global read order: its bases in the slab and where its region's haplotypes start in the haplotype table
struct ReadRef { u64 off; u32 len, hap_base; };
struct HapRef { u64 off; u32 len, pad_; };                 // in input order, region after region
// one read that needs the aligner: sources in the slab, destinations as the aligner's offsets (the chunk's first is subtracted)
struct GatherJob { u64 src_ref, src_alt, dst_ref, dst_alt; u32 len_ref, len_alt; };
static_assert(sizeof(ReadRef) == 16 && sizeof(HapRef) == 16 && sizeof(GatherJob) == 40, "table entries");

// One wavefront per kept read: does the read occur verbatim in its best haplotype, and where last?  Lanes take the start positions
// from H - R downwards, 64 at a time, and compare with an early exit; a ballot picks the highest matching start of the first block
// that has one.  R > H: no start at all, -1.  Lane 0 also copies the keep flag next to the result, so that the host fetches
// [best | match | keep] in one copy.
__global__ __launch_bounds__(256) void k_realign_verbatim(const ReadRef* __restrict__ reads, const HapRef* __restrict__ haps,
                                                          const u8* __restrict__ bases, const u8* __restrict__ hap_bases,
                                                          const int32_t* __restrict__ best, const u8* __restrict__ keep, u32 n_reads,
                                                          int enabled, int32_t* __restrict__ match, u8* __restrict__ keep_out) {
    const u32 r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_reads) return;
    const bool kept = keep[r] != 0;
    int found = -1;
    if (kept && enabled) {
        const ReadRef R = reads[r];
        const HapRef H = haps[R.hap_base + (u32)best[r]];
        const u8* rd = bases + R.off;
        const u8* hp = hap_bases + H.off;
        const int n = (int)R.len;
        for (int top = (int)H.len - n; top >= 0; top -= 64) {          // the block's highest start; every start s has s + n <= H
            const int start = top - lane;
            bool ok = start >= 0;
            if (ok) {
                const u8* w = hp + start;
                int i = 0;
                while (i < n && w[i] == rd[i]) ++i;
                ok = i == n;
            }
            const unsigned long long m = __ballot(ok);
            if (m) { found = top - (__ffsll((long long)m) - 1); break; }
        }
    }
    if (lane == 0) { match[r] = found; keep_out[r] = kept ? 1 : 0; }
}

// One wavefront per read that needs the aligner: its best haplotype and its bases out of the slab into the aligner's dense arrays.
__global__ __launch_bounds__(256) void k_realign_gather(const GatherJob* __restrict__ jobs, u32 n_jobs, u64 base_ref, u64 base_alt,
                                                        const u8* __restrict__ bases, const u8* __restrict__ hap_bases,
                                                        u8* __restrict__ d_ref, u8* __restrict__ d_alt) {
    const u32 q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63;
    if (q >= n_jobs) return;
    const GatherJob J = jobs[q];
    const u8* s1 = hap_bases + J.src_ref; u8* d1 = d_ref + (J.dst_ref - base_ref);
    const u8* s2 = bases + J.src_alt;     u8* d2 = d_alt + (J.dst_alt - base_alt);
    for (u32 x = lane; x < J.len_ref; x += 64) d1[x] = s1[x];
    for (u32 x = lane; x < J.len_alt; x += 64) d2[x] = s2[x];
}

// ---- read -> reference ------------------------------------------------------------------------------------------------------------
// one read of k_read_to_ref: where its bases, its reference haplotype and its two element lists lie.  kVerbatim: no aligner list, the
// rule takes <read_len>M (the shortcut's result); kDropped: the filter dropped the read, nothing is computed.
struct ToRefJob {
    u64 read_at, ref_at;
    u32 read_len, ref_len, sw_at, n_sw, hap_at, n_hap;
    int32_t offset, hap_start, reference_start;
    u32 hard_lead, hard_trail, flags;
};
constexpr u32 kVerbatim = 1, kDropped = 2;
static_assert(sizeof(ToRefJob) == 64, "table entry");

struct LaneStore {          // lane 0 alone stores elements, inside the row
    u32* row; u32 room; bool on;
    __device__ void operator()(u32 k, u32 e) const { if (on && k < room) row[k] = e; }
};
struct WaveAny {            // the byte comparison of a left-alignment step: lanes stride the window, a ballot of "differs" decides
    int lane;
    template <class P> __device__ bool operator()(int64_t lo, int64_t hi, P pred) const {
        for (int64_t at = lo; at < hi; at += 64) {
            const int64_t j = at + lane;
            if (__ballot(j < hi && pred(j))) return true;
        }
        return false;
    }
};

// One wavefront per read, four per workgroup.  The read index goes through readfirstlane, so everything the rule loads by it (the
// job, the elements) is loaded once per wavefront and every branch of the merge is uniform; the lanes differ only inside WaveAny.
__global__ __launch_bounds__(256) void k_read_to_ref(const ToRefJob* __restrict__ jobs, const u32* __restrict__ sw_el,
                                                     const u32* __restrict__ hap_el, const u8* __restrict__ read_bases,
                                                     const u8* __restrict__ ref_bases, u32 n_reads, u32 stride,
                                                     int32_t* __restrict__ out_start, u32* __restrict__ out_rows,
                                                     u32* __restrict__ out_n, u8* __restrict__ out_status) {
    namespace R = mgx_to_ref_rule;
    const u32 r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (r >= n_reads) return;
    const ToRefJob J = jobs[r];
    R::Result res{0, 0, R::kDropped};
    if (!(J.flags & kDropped)) {
        const R::Input in{(J.flags & kVerbatim) ? nullptr : sw_el + J.sw_at, J.n_sw, J.offset, hap_el + J.hap_at, J.n_hap, J.hap_start,
                          ref_bases + J.ref_at, J.ref_len, read_bases + J.read_at, J.read_len, J.reference_start, J.hard_lead, J.hard_trail};
        res = R::read_to_ref(in, stride, LaneStore{out_rows + (u64)r * stride, stride, lane == 0}, WaveAny{lane});
    }
    if (lane == 0) {
        const bool placed = res.status == R::kOk || res.status == R::kNoRoom;
        out_start[r] = res.status == R::kOk ? res.start : 0;
        out_n[r] = placed ? res.n : 0;
        out_status[r] = res.status;
    }
}

// what a PairHMM context keeps for this call (mgx_internal::PairhmmExt)
struct Realign {
    Mirror tables, small, gjobs;      // [ReadRef | HapRef | priority | pri_off] up | [best | match | keep] down | GatherJob up
    Mirror to_ref_up, to_ref_down;    // [ToRefJob | aligner elements | haplotype elements | (bases)] up | [start | n | status | rows] down
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};     // best: 0-1, verbatim: 1-2, gather: 3-4, to-reference: 5-6
    mgx_realign_stats_t stats{};
    mgx_realign_to_ref_stats_t to_ref_stats{};
    ~Realign() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
};
int realign_of(const PairhmmView& v, Realign** out) {
    if (!v.ext->p) {
        std::unique_ptr<Realign> r(new (std::nothrow) Realign);      // whole before the context sees it
        if (!r) return -ENOMEM;
        for (auto& e : r->ev) HIP_TRY(hipEventCreate(&e));
        v.ext->p = r.release(); v.ext->free_fn = [](void* p) { delete static_cast<Realign*>(p); };
    }
    *out = static_cast<Realign*>(v.ext->p);
    return 0;
}
size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- read -> reference: one launch over all reads on the PairHMM compute stream, one download
struct ToRefOut { size_t o_n, o_status, o_rows, bytes; };           // [start | n | status | rows] in Realign::to_ref_down
int launch_to_ref(const PairhmmView& v, Realign* st, size_t o_sw, size_t o_hap, size_t up_bytes, const u8* d_reads, const u8* d_refs, u32 n,
                  u32 stride, ToRefOut* L) {
    L->o_n = up256((size_t)n * 4); L->o_status = 2 * L->o_n; L->o_rows = L->o_status + up256(n);
    L->bytes = L->o_rows + (size_t)n * stride * 4;
    if (int rc = st->to_ref_down.reserve(L->bytes)) return rc;
    hipStream_t s = v.compute;
    u8* up = st->to_ref_up.dev; u8* down = st->to_ref_down.dev;
    HIP_TRY(hipMemcpyAsync(up, st->to_ref_up.pin, up_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(st->ev[5], s));
    hipLaunchKernelGGL(k_read_to_ref, dim3((n + 3) / 4), dim3(256), 0, s, (const ToRefJob*)up, (const u32*)(up + o_sw), (const u32*)(up + o_hap),
                       d_reads ? d_reads : up, d_refs ? d_refs : up, n, stride, (int32_t*)down, (u32*)(down + L->o_rows), (u32*)(down + L->o_n),
                       down + L->o_status);
    HIP_TRY(hipEventRecord(st->ev[6], s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(st->to_ref_down.pin, down, L->bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (v.flags & MGX_PAIRHMM_TIMING) HIP_TRY(hipEventElapsedTime(&st->to_ref_stats.ms_to_ref, st->ev[5], st->ev[6]));
    const u8* status = st->to_ref_down.pin + L->o_status;
    for (u32 r = 0; r < n; ++r) st->to_ref_stats.n_status[status[r] < MGX_TO_REF_N_STATUS ? status[r] : MGX_TO_REF_UNDEFINED]++;
    return 0;
}

// BAM-encoded element lists of a caller: CSR offsets that do not decrease, fewer than 2^32 elements, operator codes 0..8
int check_elements(const char* what, u64 n_lists, const u64* off, const u32* el) {
    if (!off || (n_lists && off[n_lists] > off[0] && !el)) { set_error("%s: NULL array", what); return -EINVAL; }
    for (u64 i = 0; i < n_lists; ++i) if (off[i + 1] < off[i]) { set_error("%s: offsets decrease at %llu", what, (unsigned long long)i); return -EINVAL; }
    if (n_lists && off[n_lists] - off[0] >= (1ull << 32)) { set_error("%s: 2^32 elements or more", what); return -E2BIG; }
    for (u64 k = n_lists ? off[0] : 0, e = n_lists ? off[n_lists] : 0; k < e; ++k)
        if ((el[k] & 15) > 8) { set_error("%s: element %llu has operator code %u", what, (unsigned long long)k, el[k] & 15); return -EINVAL; }
    return 0;
}
constexpr u64 kToRefMaxLen = 1ull << 28;

int read_to_ref_call(mgx_pairhmm_t* c, const mgx_to_ref_input_t* in, int32_t* out_start, u32* out_cigar, u32 stride, u32* out_n, u8* out_status) {
    if (!c || !in) { set_error("NULL argument"); return -EINVAL; }
    const u64 n = in->n_reads;
    if (n && (!out_start || !out_cigar || !out_n || !out_status || !in->read_off || !in->sw_offset || !in->read_hap || !in->hap_start ||
              !in->read_ref || !in->ref_off || !in->reference_start)) { set_error("NULL argument"); return -EINVAL; }
    if (n && stride == 0) { set_error("cigar_stride must be at least 1"); return -EINVAL; }
    if (n > 0x7FFFFFF0ull) { set_error("more than 2^31 reads in one call"); return -E2BIG; }
    if (int rc = check_elements("sw_cigar", n, in->sw_cigar_off, in->sw_cigar)) return rc;
    if (n) if (int rc = check_elements("hap_cigar", in->n_haps, in->hap_cigar_off, in->hap_cigar)) return rc;
    for (u64 r = 0; r < n; ++r) {
        if (in->read_off[r + 1] < in->read_off[r]) { set_error("read_off decreases at %llu", (unsigned long long)r); return -EINVAL; }
        if (in->read_off[r + 1] - in->read_off[r] >= kToRefMaxLen) { set_error("read %llu has 2^28 bases or more", (unsigned long long)r); return -E2BIG; }
        if (in->read_hap[r] >= in->n_haps || in->read_ref[r] >= in->n_refs) { set_error("read %llu: haplotype or reference index out of range", (unsigned long long)r); return -EINVAL; }
    }
    for (u64 h = 0; n && h < in->n_refs; ++h) {
        if (in->ref_off[h + 1] < in->ref_off[h]) { set_error("ref_off decreases at %llu", (unsigned long long)h); return -EINVAL; }
        if (in->ref_off[h + 1] - in->ref_off[h] >= kToRefMaxLen) { set_error("reference haplotype %llu has 2^28 bases or more", (unsigned long long)h); return -E2BIG; }
    }
    const u64 read_bytes = n ? in->read_off[n] - in->read_off[0] : 0, ref_bytes = n && in->n_refs ? in->ref_off[in->n_refs] - in->ref_off[0] : 0;
    if (n && ((read_bytes && !in->read_bases) || (ref_bytes && !in->ref_bases))) { set_error("NULL argument"); return -EINVAL; }
    const PairhmmView v = pairhmm_view(c);
    HIP_TRY(hipSetDevice(v.device));
    Realign* st = nullptr;
    if (int rc = realign_of(v, &st)) return rc;
    st->to_ref_stats = mgx_realign_to_ref_stats_t{};
    if (n == 0) return 0;
    // everything the kernel reads, in one upload: [jobs | aligner elements | haplotype elements | read bases | reference bases]
    const u64 sw0 = in->sw_cigar_off[0], hap0 = in->n_haps ? in->hap_cigar_off[0] : 0, n_sw = in->sw_cigar_off[n] - sw0,
              n_hap = in->n_haps ? in->hap_cigar_off[in->n_haps] - hap0 : 0;
    const size_t o_sw = up256(n * sizeof(ToRefJob)), o_hap = o_sw + up256(n_sw * 4), o_reads = o_hap + up256(n_hap * 4),
                 o_refs = o_reads + up256(read_bytes), bytes = o_refs + up256(ref_bytes);
    if (int rc = st->to_ref_up.reserve(bytes)) return rc;
    u8* pin = st->to_ref_up.pin;
    ToRefJob* jobs = (ToRefJob*)pin;
    for (u64 r = 0; r < n; ++r) {
        const u32 h = in->read_hap[r], f = in->read_ref[r];
        jobs[r] = ToRefJob{o_reads + (in->read_off[r] - in->read_off[0]), o_refs + (in->ref_off[f] - in->ref_off[0]),
                           (u32)(in->read_off[r + 1] - in->read_off[r]), (u32)(in->ref_off[f + 1] - in->ref_off[f]),
                           (u32)(in->sw_cigar_off[r] - sw0), (u32)(in->sw_cigar_off[r + 1] - in->sw_cigar_off[r]),
                           (u32)(in->hap_cigar_off[h] - hap0), (u32)(in->hap_cigar_off[h + 1] - in->hap_cigar_off[h]),
                           in->sw_offset[r], in->hap_start[h], in->reference_start[r],
                           in->hard_clips ? in->hard_clips[2 * r] : 0u, in->hard_clips ? in->hard_clips[2 * r + 1] : 0u, 0u};
        if (jobs[r].hard_lead >= kToRefMaxLen || jobs[r].hard_trail >= kToRefMaxLen) { set_error("read %llu: hard clip of 2^28 bases or more", (unsigned long long)r); return -E2BIG; }
    }
    if (n_sw) memcpy(pin + o_sw, in->sw_cigar + sw0, n_sw * 4);
    if (n_hap) memcpy(pin + o_hap, in->hap_cigar + hap0, n_hap * 4);
    if (read_bytes) memcpy(pin + o_reads, in->read_bases + in->read_off[0], read_bytes);
    if (ref_bytes) memcpy(pin + o_refs, in->ref_bases + in->ref_off[0], ref_bytes);
    ToRefOut L;
    if (int rc = launch_to_ref(v, st, o_sw, o_hap, bytes, nullptr, nullptr, (u32)n, stride, &L)) return rc;
    const u8* down = st->to_ref_down.pin;
    memcpy(out_start, down, n * 4); memcpy(out_n, down + L.o_n, n * 4); memcpy(out_status, down + L.o_status, n);
    memcpy(out_cigar, down + L.o_rows, n * (size_t)stride * 4);
    return 0;
}

struct Args {
    mgx_pairhmm_t* c; mgx_sw_t* sw; u32 n_regions; const mgx_pairhmm_input_t* regions; const double* const* hap_priority;
    mgx_sw_params_t params; u8 strategy;
    int32_t* const* out_best; int32_t* const* out_offset; char* const* out_cigar; u32 stride; int32_t* const* out_score;
    // mgx_realign_regions_to_ref alone
    bool with_to_ref; const mgx_to_ref_region_t* to_ref; int32_t* const* out_start; u32* const* out_rows; u32 row_stride; u32* const* out_n; u8* const* out_status;
};
bool shortcut_applies(u8 strategy) { return strategy == MGX_SW_SOFTCLIP || strategy == MGX_SW_IGNORE; }      // SWNativeAlignerWrapper.cpp:14

// ---- before anything is launched: arguments, devices, lengths
int check(const Args& a, const uint8_t* const* mapq, const mgx_read_model_t* model, double* const* out_log10, u64* n_reads) {
    if (!a.c || !a.sw || !model || (a.n_regions && (!a.regions || !mapq || !out_log10 || !a.out_best || !a.out_offset))) { set_error("NULL argument"); return -EINVAL; }
    if (a.with_to_ref && a.n_regions && (a.row_stride == 0 || !a.to_ref || !a.out_start || !a.out_rows || !a.out_n || !a.out_status)) { set_error("NULL to-reference argument or ref_cigar_stride 0"); return -EINVAL; }
    if (a.out_cigar && a.stride < 2) { set_error("cigar_stride must be at least 2"); return -EINVAL; }
    if (a.strategy < MGX_SW_SOFTCLIP || a.strategy > MGX_SW_IGNORE) { set_error("unknown overhang strategy %d", (int)a.strategy); return -EINVAL; }
    const SwView sv = sw_view(a.sw);
    if (pairhmm_view(a.c).device != sv.device) { set_error("the PairHMM context is on device %d, the Smith-Waterman context on %d", pairhmm_view(a.c).device, sv.device); return -EINVAL; }
    *n_reads = 0;
    for (u32 g = 0; g < a.n_regions; ++g) {
        const mgx_pairhmm_input_t& in = a.regions[g];
        if (in.pair_read || in.pair_hap) { set_error("region %u: regions are given in the cross-product form (pair arrays NULL)", g); return -EINVAL; }
        if (int rc = mgx::validate(&in)) return rc;
        *n_reads += in.n_reads;
        if (in.n_reads == 0) continue;
        if (a.with_to_ref) {
            const mgx_to_ref_region_t& tr = a.to_ref[g];
            if (!a.out_start[g] || !a.out_rows[g] || !a.out_n[g] || !a.out_status[g] || (in.n_haps && !tr.hap_start)) { set_error("region %u: to-reference pointer is NULL", g); return -EINVAL; }
            if (int rc = check_elements("hap_cigar", in.n_haps, tr.hap_cigar_off, tr.hap_cigar)) return rc;
            if (in.n_haps && tr.ref_hap >= in.n_haps) { set_error("region %u: ref_hap %u of %llu haplotypes", g, tr.ref_hap, (unsigned long long)in.n_haps); return -EINVAL; }
        }
        if (!a.out_best[g] || !a.out_offset[g] || (a.out_cigar && !a.out_cigar[g]) || (a.out_score && !a.out_score[g])) { set_error("region %u: output pointer is NULL", g); return -EINVAL; }
        if (in.n_haps == 0) continue;
        // every haplotype of a region that has reads may come out best
        for (u64 h = 0; h < in.n_haps; ++h)
            if (in.hap_off[h + 1] - in.hap_off[h] > (u64)sv.max_ref) {
                set_error("region %u: haplotype %llu of %llu bases exceeds the aligner's reference limit %d", g, (unsigned long long)h,
                          (unsigned long long)(in.hap_off[h + 1] - in.hap_off[h]), sv.max_ref);
                return -E2BIG;
            }
        for (u64 r = 0; r < in.n_reads; ++r)
            if (in.read_off[r + 1] - in.read_off[r] > (u64)sv.max_alt) { set_error("region %u: read %llu exceeds the aligner's alternate limit %d", g, (unsigned long long)r, sv.max_alt); return -E2BIG; }
    }
    if (*n_reads > 0x7FFFFFF0ull) { set_error("more than 2^31 reads in one call"); return -E2BIG; }
    return 0;
}

// ---- the tables of the two kernels, into the pinned mirror: reads and haplotypes as create_cross lays them out in the slab
// (region after region, offsets rebased to each region's first byte), priorities per haplotype (0 where a region has none)
struct Tables { size_t o_reads, o_haps, o_pri, o_prioff, bytes; u64 n_reads, n_haps; bool has_pri; };
int stage_tables(const Args& a, u64 n_reads, Realign* st, Tables* t) {
    u64 n_haps = 0;
    bool has_pri = false;
    for (u32 g = 0; g < a.n_regions; ++g) { n_haps += a.regions[g].n_haps; has_pri |= a.hap_priority && a.hap_priority[g]; }
    t->n_reads = n_reads; t->n_haps = n_haps; t->has_pri = has_pri;
    t->o_reads = 0; t->o_haps = up256(n_reads * sizeof(ReadRef)); t->o_pri = t->o_haps + up256(n_haps * sizeof(HapRef));
    t->o_prioff = t->o_pri + up256(n_haps * sizeof(double)); t->bytes = t->o_prioff + up256(n_reads * sizeof(u32));
    if (int rc = st->tables.reserve(t->bytes)) return rc;
    ReadRef* reads = (ReadRef*)(st->tables.pin + t->o_reads); HapRef* haps = (HapRef*)(st->tables.pin + t->o_haps);
    double* pri = (double*)(st->tables.pin + t->o_pri); u32* prioff = (u32*)(st->tables.pin + t->o_prioff);
    u64 r_at = 0, h_at = 0, rb = 0, hb = 0;
    for (u32 g = 0; g < a.n_regions; ++g) {
        const mgx_pairhmm_input_t& in = a.regions[g];
        for (u64 r = 0; r < in.n_reads; ++r) {
            reads[r_at + r] = ReadRef{rb + (in.read_off[r] - in.read_off[0]), (u32)(in.read_off[r + 1] - in.read_off[r]), (u32)h_at};
            prioff[r_at + r] = (u32)h_at;
        }
        for (u64 h = 0; h < in.n_haps; ++h) {
            haps[h_at + h] = HapRef{hb + (in.hap_off[h] - in.hap_off[0]), (u32)(in.hap_off[h + 1] - in.hap_off[h]), 0};
            pri[h_at + h] = (a.hap_priority && a.hap_priority[g]) ? a.hap_priority[g][h] : 0.0;
        }
        if (in.n_reads) rb += in.read_off[in.n_reads] - in.read_off[0];
        if (in.n_haps) hb += in.hap_off[in.n_haps] - in.hap_off[0];
        r_at += in.n_reads; h_at += in.n_haps;
    }
    return 0;
}

// ---- behind the epilogue on the PairHMM compute stream: best haplotype and verbatim search of every read; 9 bytes per read come back
struct Small { const int32_t* best; const int32_t* match; const u8* keep; };
int launch_best_and_verbatim(const Args& a, const PairhmmView& v, const RegionBatch& rb, const Tables& t, Realign* st, Small* out) {
    hipStream_t s = v.compute;
    const u32 n = rb.n_reads;
    const size_t o_match = up256((size_t)n * 4), o_keep = 2 * o_match, bytes = o_keep + up256(n);
    if (int rc = st->small.reserve(bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(st->tables.dev, st->tables.pin, t.bytes, hipMemcpyHostToDevice, s));
    int32_t* d_best = (int32_t*)st->small.dev; int32_t* d_match = (int32_t*)(st->small.dev + o_match);
    HIP_TRY(hipEventRecord(st->ev[0], s));
    launch_best_allele_rows(s, rb.d_out, rb.d_row_off, rb.d_row_nh, t.has_pri ? (const double*)(st->tables.dev + t.o_pri) : nullptr,
                            (const u32*)(st->tables.dev + t.o_prioff), n, d_best);
    HIP_TRY(hipEventRecord(st->ev[1], s));
    hipLaunchKernelGGL(k_realign_verbatim, dim3((n + 3) / 4), dim3(256), 0, s, (const ReadRef*)(st->tables.dev + t.o_reads),
                       (const HapRef*)(st->tables.dev + t.o_haps), rb.d_bases, rb.d_hap, d_best, rb.d_keep, n, shortcut_applies(a.strategy) ? 1 : 0,
                       d_match, st->small.dev + o_keep);
    HIP_TRY(hipEventRecord(st->ev[2], s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(st->small.pin, st->small.dev, bytes, hipMemcpyDeviceToHost, s));
    out->best = (const int32_t*)st->small.pin; out->match = (const int32_t*)(st->small.pin + o_match); out->keep = st->small.pin + o_keep;
    return 0;
}

// ---- the aligner's input over the reads that still need it: offset prefixes on the host, the bytes stay on the device
struct Pairs { std::vector<u64> ref_off, alt_off; std::vector<u8> strategy; u64 n = 0; };
int plan_pairs(const Args& a, const Tables& t, const Small& sm, Realign* st, Pairs* p) {
    const ReadRef* reads = (const ReadRef*)(st->tables.pin + t.o_reads); const HapRef* haps = (const HapRef*)(st->tables.pin + t.o_haps);
    u64 n = 0;
    for (u64 r = 0; r < t.n_reads; ++r) {
        st->stats.n_kept += sm.keep[r] != 0;
        if (sm.keep[r] && sm.match[r] >= 0) st->stats.n_verbatim++;
        n += sm.keep[r] && sm.match[r] < 0;
    }
    st->stats.n_sw_pairs = n;
    p->n = n;
    p->ref_off.assign(n + 1, 0); p->alt_off.assign(n + 1, 0); p->strategy.assign(n, a.strategy);
    if (int rc = st->gjobs.reserve(n * sizeof(GatherJob))) return rc;
    GatherJob* jobs = (GatherJob*)st->gjobs.pin;
    u64 q = 0;
    for (u64 r = 0; r < t.n_reads; ++r) {
        if (!sm.keep[r] || sm.match[r] >= 0) continue;
        const ReadRef& R = reads[r];
        const HapRef& H = haps[R.hap_base + (u32)sm.best[r]];
        jobs[q] = GatherJob{H.off, R.off, p->ref_off[q], p->alt_off[q], H.len, R.len};
        p->ref_off[q + 1] = p->ref_off[q] + H.len; p->alt_off[q + 1] = p->alt_off[q] + R.len;
        ++q;
    }
    return 0;
}

// the aligner's callback, per chunk in place of its upload (mgx_internal::SwDeviceSource)
struct GatherCtx { Realign* st; const RegionBatch* rb; const Pairs* pairs; bool timing, pending; };
int gather_chunk(void* user, hipStream_t s, u64 lo, u64 hi, u8* d_ref, u8* d_alt) {
    GatherCtx* g = static_cast<GatherCtx*>(user);
    Realign* st = g->st;
    float ms = 0;
    if (g->pending) { HIP_TRY(hipEventElapsedTime(&ms, st->ev[3], st->ev[4])); st->stats.ms_gather += ms; g->pending = false; }   // the chunk before has been fetched
    const u32 n = (u32)(hi - lo);
    HIP_TRY(hipMemcpyAsync(st->gjobs.dev + lo * sizeof(GatherJob), st->gjobs.pin + lo * sizeof(GatherJob), n * sizeof(GatherJob), hipMemcpyHostToDevice, s));
    if (g->timing) HIP_TRY(hipEventRecord(st->ev[3], s));
    hipLaunchKernelGGL(k_realign_gather, dim3((n + 3) / 4), dim3(256), 0, s, (const GatherJob*)st->gjobs.dev + lo, n, g->pairs->ref_off[lo],
                       g->pairs->alt_off[lo], g->rb->d_bases, g->rb->d_hap, d_ref, d_alt);
    if (g->timing) { HIP_TRY(hipEventRecord(st->ev[4], s)); g->pending = true; }
    HIP_TRY(hipGetLastError());
    return 0;
}

// "<len>M" as the aligner writes a one-element list (sw_trace_rule.h: an element whose text does not fit is skipped; a read is at most max_alt bases)
void verbatim_text(u32 len, u64 hap_len, char* dst, u32 stride) {
    const int16_t el[2] = {(int16_t)mgx_sw_trace::kOpMatch, (int16_t)len};
    dst[mgx_sw_trace::render(el, 1, dst, mgx_sw_trace::text_cap(hap_len, len, stride))] = 0;
}

// ---- the per-read results into the caller's arrays of every region: dropped, verbatim, aligned
struct Aligned { std::vector<int32_t> offset, score; std::vector<char> cigar; };
void scatter_reads(const Args& a, const Tables* t, const Small* sm, const Realign* st, const Aligned& al) {
    u64 r_at = 0, q = 0;
    for (u32 g = 0; g < a.n_regions; ++g) {
        const u64 nr = a.regions[g].n_reads;
        for (u64 r = 0; r < nr; ++r) {
            const u64 R = r_at + r;
            char* text = a.out_cigar ? a.out_cigar[g] + r * a.stride : nullptr;
            const bool kept = sm && sm->keep[R];
            a.out_best[g][r] = sm ? sm->best[R] : 0;
            if (!kept) {
                a.out_offset[g][r] = MGX_REALIGN_NOT_ALIGNED;
                if (text) text[0] = 0;
                if (a.out_score) a.out_score[g][r] = 0;
            } else if (sm->match[R] >= 0) {
                const ReadRef& rd = ((const ReadRef*)(st->tables.pin + t->o_reads))[R];
                const HapRef& hp = ((const HapRef*)(st->tables.pin + t->o_haps))[rd.hap_base + (u32)sm->best[R]];
                a.out_offset[g][r] = sm->match[R];
                if (text) verbatim_text(rd.len, hp.len, text, a.stride);
                if (a.out_score) a.out_score[g][r] = (int32_t)rd.len * a.params.match;
            } else {
                a.out_offset[g][r] = al.offset[q];
                if (text) memcpy(text, al.cigar.data() + q * a.stride, a.stride);
                if (a.out_score) a.out_score[g][r] = al.score[q];
                ++q;
            }
        }
        r_at += nr;
    }
}

// ---- between aligner and scatter (mgx_realign_regions_to_ref): every read's alignment mapped onto the reference.  Up go the jobs, the
// aligner's elements of the reads that went through it and the haplotype CIGAR tables; bases and haplotypes are read in the batch's slab.
int to_ref_stage(const Args& a, const PairhmmView& v, const RegionBatch& rb, const Tables& t, const Small& sm, const Aligned& al,
                 const SwElementSink& sink, Realign* st, ToRefOut* L) {
    const ReadRef* reads = (const ReadRef*)(st->tables.pin + t.o_reads); const HapRef* haps = (const HapRef*)(st->tables.pin + t.o_haps);
    u64 n_hap_el = 0;
    for (u32 g = 0; g < a.n_regions; ++g)
        if (a.regions[g].n_reads && a.regions[g].n_haps) n_hap_el += a.to_ref[g].hap_cigar_off[a.regions[g].n_haps] - a.to_ref[g].hap_cigar_off[0];
    if (n_hap_el >= (1ull << 32) || sink.el.size() >= (1ull << 32)) { set_error("2^32 CIGAR elements or more in one call"); return -E2BIG; }
    const size_t o_sw = up256(t.n_reads * sizeof(ToRefJob)), o_hap = o_sw + up256(sink.el.size() * 4), bytes = o_hap + up256(n_hap_el * 4);
    if (int rc = st->to_ref_up.reserve(bytes)) return rc;
    u8* pin = st->to_ref_up.pin;
    ToRefJob* jobs = (ToRefJob*)pin;
    u32* hap_el = (u32*)(pin + o_hap);
    if (!sink.el.empty()) memcpy(pin + o_sw, sink.el.data(), sink.el.size() * 4);
    u64 r_at = 0, q = 0, el_at = 0;
    for (u32 g = 0; g < a.n_regions; ++g) {
        const mgx_pairhmm_input_t& in = a.regions[g];
        const mgx_to_ref_region_t& tr = a.to_ref[g];
        const u64 nr = in.n_reads;
        if (nr && in.n_haps) memcpy(hap_el + el_at, tr.hap_cigar + tr.hap_cigar_off[0], (tr.hap_cigar_off[in.n_haps] - tr.hap_cigar_off[0]) * 4);
        for (u64 r = 0; r < nr; ++r) {
            const u64 R = r_at + r;
            ToRefJob J{};
            if (!sm.keep[R]) J.flags = kDropped;      // (a region without haplotypes keeps no read)
            else {
                const ReadRef& rd = reads[R];
                const u32 h = (u32)sm.best[R];
                const HapRef& ref = haps[rd.hap_base + tr.ref_hap];
                J = ToRefJob{rd.off, ref.off, rd.len, ref.len, 0, 0, (u32)(el_at + (tr.hap_cigar_off[h] - tr.hap_cigar_off[0])),
                             (u32)(tr.hap_cigar_off[h + 1] - tr.hap_cigar_off[h]), sm.match[R], tr.hap_start[h], tr.reference_start,
                             tr.hard_clips ? tr.hard_clips[2 * r] : 0u, tr.hard_clips ? tr.hard_clips[2 * r + 1] : 0u, kVerbatim};
                if (sm.match[R] < 0) { J.flags = 0; J.offset = al.offset[q]; J.sw_at = (u32)sink.off[q]; J.n_sw = sink.n[q]; ++q; }
            }
            jobs[R] = J;
        }
        if (nr && in.n_haps) el_at += tr.hap_cigar_off[in.n_haps] - tr.hap_cigar_off[0];
        r_at += nr;
    }
    return launch_to_ref(v, st, o_sw, o_hap, bytes, rb.d_bases, rb.d_hap, (u32)t.n_reads, a.row_stride, L);
}
// ... and its results to the caller's arrays; L == nullptr: no read was kept
void scatter_to_ref(const Args& a, const Realign* st, const ToRefOut* L) {
    u64 r_at = 0;
    const u8* down = st->to_ref_down.pin;
    for (u32 g = 0; g < a.n_regions; ++g) {
        const u64 nr = a.regions[g].n_reads;
        if (!nr) continue;
        if (L) {
            memcpy(a.out_start[g], down + r_at * 4, nr * 4); memcpy(a.out_n[g], down + L->o_n + r_at * 4, nr * 4);
            memcpy(a.out_status[g], down + L->o_status + r_at, nr); memcpy(a.out_rows[g], down + L->o_rows + r_at * a.row_stride * 4, nr * (size_t)a.row_stride * 4);
        } else {
            memset(a.out_start[g], 0, nr * 4); memset(a.out_n[g], 0, nr * 4); memset(a.out_status[g], MGX_TO_REF_DROPPED, nr);
        }
        r_at += nr;
    }
}

int run(const Args& a, const uint8_t* const* mapq, const mgx_read_model_t* model, double* const* out_log10, uint8_t* const* out_keep) {
    u64 n_reads = 0;
    if (int rc = check(a, mapq, model, out_log10, &n_reads)) return rc;
    const PairhmmView v = pairhmm_view(a.c);
    HIP_TRY(hipSetDevice(v.device));
    Realign* st = nullptr;
    if (int rc = realign_of(v, &st)) return rc;
    st->stats = mgx_realign_stats_t{};
    st->stats.n_reads = n_reads;
    if (a.with_to_ref) st->to_ref_stats = mgx_realign_to_ref_stats_t{};
    // 1. the cross-product batch and its run
    RegionBatch rb;
    if (int rc = regions_begin(a.c, a.n_regions, a.regions, mapq, model, out_log10, &rb)) return rc;
    if (!rb.batch) {                                                                     // no test case: no read is kept
        scatter_reads(a, nullptr, nullptr, st, Aligned{});
        if (a.with_to_ref) { scatter_to_ref(a, st, nullptr); st->to_ref_stats.n_status[MGX_TO_REF_DROPPED] = n_reads; }
        return 0;
    }
    const int rc = [&]() -> int {
        Tables t; Small sm; Pairs pairs; Aligned al; SwElementSink sink; ToRefOut tr;
        int e;
        // 2. best haplotype and verbatim search behind the epilogue  3. their 9 bytes per read  4. the matrix, on the d2h stream
        if ((e = stage_tables(a, n_reads, st, &t)) || (e = launch_best_and_verbatim(a, v, rb, t, st, &sm))) return e;
        if ((e = regions_queue_download(a.c, rb, v.d2h))) return e;
        HIP_TRY(hipStreamSynchronize(v.compute));
        if (v.flags & MGX_PAIRHMM_TIMING) {
            HIP_TRY(hipEventElapsedTime(&st->stats.ms_best, st->ev[0], st->ev[1]));
            HIP_TRY(hipEventElapsedTime(&st->stats.ms_verbatim, st->ev[1], st->ev[2]));
        }
        // 5. the aligner's offsets  6. its chunks, each fed by the gather
        if ((e = plan_pairs(a, t, sm, st, &pairs))) return e;
        al.offset.assign(pairs.n, 0); al.score.assign(pairs.n, 0);
        if (a.out_cigar) al.cigar.assign(pairs.n * a.stride, 0);
        if (pairs.n) {
            GatherCtx gc{st, &rb, &pairs, (v.flags & MGX_PAIRHMM_TIMING) != 0, false};
            const SwDeviceSource src{rb.done, gather_chunk, &gc};
            const mgx_sw_input_t in{pairs.n, pairs.ref_off.data(), nullptr, pairs.alt_off.data(), nullptr, pairs.strategy.data()};
            if ((e = sw_align_from_device(a.sw, &a.params, &in, src, al.offset.data(), a.out_cigar ? al.cigar.data() : nullptr, a.stride, al.score.data(),
                                          a.with_to_ref ? &sink : nullptr))) return e;
            float ms = 0;
            if (gc.pending) { HIP_TRY(hipEventElapsedTime(&ms, st->ev[3], st->ev[4])); st->stats.ms_gather += ms; }
        }
        // 6b. read -> reference of every read, one launch behind the aligner
        if (a.with_to_ref && (e = to_ref_stage(a, v, rb, t, sm, al, sink, st, &tr))) return e;
        // 7. everything to the per-region outputs
        HIP_TRY(hipStreamSynchronize(v.d2h));
        regions_scatter(rb, a.regions, a.n_regions, out_log10, out_keep);
        scatter_reads(a, &t, &sm, st, al);
        if (a.with_to_ref) scatter_to_ref(a, st, &tr);
        return 0;
    }();
    if (rc) { (void)hipStreamSynchronize(v.compute); (void)hipStreamSynchronize(v.d2h); }     // nothing of the batch in flight when its slab goes back
    regions_end(a.c, &rb);
    return rc;
}

}  // namespace

extern "C" {

int mgx_realign_regions(mgx_pairhmm_t* c, mgx_sw_t* sw, uint32_t n_regions, const mgx_pairhmm_input_t* regions, const uint8_t* const* mapq,
                        const mgx_read_model_t* model, const double* const* hap_priority, const mgx_sw_params_t* sw_params, uint8_t strategy,
                        double* const* out_log10, uint8_t* const* out_keep, int32_t* const* out_best, int32_t* const* out_offset,
                        char* const* out_cigar, uint32_t cigar_stride, int32_t* const* out_score) {
    const mgx_sw_params_t to_best_haplotype{10, -15, -30, -5};      // ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS, read/CigarUtils.cpp:15
    const Args a{c, sw, n_regions, regions, hap_priority, sw_params ? *sw_params : to_best_haplotype, strategy,
                 out_best, out_offset, out_cigar, cigar_stride, out_score, false, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
    return run(a, mapq, model, out_log10, out_keep);
}

int mgx_realign_regions_to_ref(mgx_pairhmm_t* c, mgx_sw_t* sw, uint32_t n_regions, const mgx_pairhmm_input_t* regions, const uint8_t* const* mapq,
                               const mgx_read_model_t* model, const double* const* hap_priority, const mgx_sw_params_t* sw_params, uint8_t strategy,
                               double* const* out_log10, uint8_t* const* out_keep, int32_t* const* out_best, int32_t* const* out_offset,
                               char* const* out_cigar, uint32_t cigar_stride, int32_t* const* out_score, const mgx_to_ref_region_t* to_ref,
                               int32_t* const* out_start, uint32_t* const* out_ref_cigar, uint32_t ref_cigar_stride,
                               uint32_t* const* out_n_ref_cigar, uint8_t* const* out_status) {
    const mgx_sw_params_t to_best_haplotype{10, -15, -30, -5};
    const Args a{c, sw, n_regions, regions, hap_priority, sw_params ? *sw_params : to_best_haplotype, strategy,
                 out_best, out_offset, out_cigar, cigar_stride, out_score, true, to_ref, out_start, out_ref_cigar, ref_cigar_stride,
                 out_n_ref_cigar, out_status};
    return run(a, mapq, model, out_log10, out_keep);
}

int mgx_read_to_ref(mgx_pairhmm_t* c, const mgx_to_ref_input_t* in, int32_t* out_start, uint32_t* out_cigar, uint32_t cigar_stride,
                    uint32_t* out_n_cigar, uint8_t* out_status) {
    return read_to_ref_call(c, in, out_start, out_cigar, cigar_stride, out_n_cigar, out_status);
}

int mgx_realign_to_ref_stats(mgx_pairhmm_t* c, mgx_realign_to_ref_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    const PairhmmView v = pairhmm_view(c);
    *out = v.ext->p ? static_cast<Realign*>(v.ext->p)->to_ref_stats : mgx_realign_to_ref_stats_t{};
    return 0;
}

int mgx_realign_stats(mgx_pairhmm_t* c, mgx_realign_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    const PairhmmView v = pairhmm_view(c);
    *out = v.ext->p ? static_cast<Realign*>(v.ext->p)->stats : mgx_realign_stats_t{};
    return 0;
}

}  // extern "C"
