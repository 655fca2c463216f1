// mgx_activity_regions.hip -- per-locus activity values to active regions on the device (C ABI: include/mgx_activity.h; the rule:
// activity_profile_rule.h).  On one stream:
//   k_band_pass     one lane per state, 256 states per workgroup.  The workgroup stages its tile of probabilities plus F on either side and
//                   the 2F + 1 weights in LDS; each lane folds its sources in ascending order (the reference's order of accumulation) and
//                   writes the value, a flag byte (bit 0: value > threshold, bit 1: the state exists) and "no piece starts here".
//   runs            the first and last state of every run, compacted in position order: mgx_scan.h's exclusive scan over "the flag rises
//                   here", then k_scatter_runs.
//   k_cut_runs      one wavefront per chain of runs (a run with 2F + 2 inactive states in front starts one: no piece further back can
//                   delay its pops; the rule header says why), pieces cut one after another.  A piece's next max_region_size flags by
//                   ballot; the candidates of findBestCutSite spread over the lanes from the top index down, each lane keeping its
//                   smallest local minimum, then a butterfly reduction: smaller value, at equal values the larger index.  The pop times
//                   and the value of state s + max_region_size at the pop are the rule header's, computed by every lane alike.  A
//                   piece's end goes to the slot of its start state.
//   (the fused call runs the same kernels on the 0 / 1 bytes k_locus_activity left on the device: k_band_pass<u8>, k_cut_runs<u8>)
//   regions         the slots that hold an end, compacted in position order by the same scan, then k_emit_regions.
// No atomics, no order that depends on scheduling; every lane runs every cross-lane operation.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "activity_profile_rule.h"
#include "mgx_activity_internal.h"
#include "mgx_scan.h"

using mgx::set_error;
namespace PR = mgx_activity_profile_rule;

static_assert(PR::kBandTile == MGX_ACTIVITY_BAND_TILE && PR::kFilterCap == MGX_ACTIVITY_MAX_FILTER, "the header's constants");
static_assert(sizeof(PR::Region) == sizeof(mgx_activity_region_t), "region layout");

namespace {
typedef uint8_t u8; typedef uint32_t u32; typedef uint64_t u64;
constexpr u8 kActive = 1, kExists = 2;
constexpr u32 kCutBlocks = 1024;          // the cutter's grid: 4 wavefronts each, runs dealt round-robin

struct Shape { int64_t first_abs, n_loci, n_upper, contig_length; };      // n_upper: PR::states_upper

template <typename Src>
__global__ __launch_bounds__(PR::kBandTile) void k_band_pass(const Src* __restrict__ prob, const double* __restrict__ weights, Shape S, int filter,
                                                             double threshold, double* __restrict__ value, u8* __restrict__ flag,
                                                             int32_t* __restrict__ piece_end) {
    __shared__ double s_w[2 * PR::kFilterCap + 1];
    __shared__ double s_p[PR::kBandTile + 2 * PR::kFilterCap];
    const int64_t q0 = (int64_t)blockIdx.x * PR::kBandTile;
    const int tid = (int)threadIdx.x;
    for (int k = tid; k <= 2 * filter; k += PR::kBandTile) s_w[k] = weights[k];
    for (int k = tid; k < PR::kBandTile + 2 * filter; k += PR::kBandTile) {
        const int64_t p = q0 - filter + k;
        s_p[k] = p >= 0 && p < S.n_loci ? (double)prob[p] : 0.0;
    }
    __syncthreads();
    const int64_t q = q0 + tid;
    if (q > S.n_upper) return;
    if (q == S.n_upper) { flag[q] = 0; return; }          // the sentinel behind the last state
    const PR::Fold f = PR::fold_state(q, S.n_loci, filter, [&](int64_t p) { return s_p[p - q0 + filter]; }, [&](int64_t k) { return s_w[k]; }, S.n_loci - 1);
    const bool exists = q < S.n_loci || f.any_positive;
    value[q] = f.value;
    flag[q] = exists ? (u8)(kExists | (f.value > threshold ? kActive : 0)) : (u8)0;
    piece_end[q] = -1;
}

struct RisingFlag { const u8* flag; __device__ u64 operator()(u64 i) const { return (flag[i] & kActive) && !(i && (flag[i - 1] & kActive)); } };
struct HoldsPiece { const int32_t* piece_end; __device__ u64 operator()(u64 i) const { return piece_end[i] >= 0; } };

__global__ __launch_bounds__(256) void k_scatter_runs(const u8* __restrict__ flag, const u64* __restrict__ rank, u64 n, u32* __restrict__ heads,
                                                      u32* __restrict__ tails, u64* __restrict__ counts) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) counts[0] = rank[n];
    if (i >= n || !(flag[i] & kActive)) return;
    if (RisingFlag{flag}(i)) heads[rank[i]] = (u32)i;
    if (!(flag[i + 1] & kActive)) tails[rank[i + 1] - 1] = (u32)i;          // flag[n] is the sentinel; rank[i + 1]: the runs that start at or before i
}

template <typename Src>
__global__ __launch_bounds__(256) void k_cut_runs(const u32* __restrict__ heads, const u32* __restrict__ tails, const u64* __restrict__ counts,
                                                  const u8* __restrict__ flag, const double* __restrict__ value, const Src* __restrict__ prob,
                                                  const double* __restrict__ weights, Shape S, PR::CutParams C, int32_t* __restrict__ piece_end) {
    const u64 wave = (u64)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * 4;
    const int lane = (int)(threadIdx.x & 63);
    const u64 n_runs = counts[0];
    const auto p_at = [&](int64_t p) { return (double)prob[p]; };
    const auto w_at = [&](int64_t k) { return weights[k]; };
    const auto final_value = [&](int64_t q) { return value[q]; };
    const auto state_exists = [&](int64_t q) { return q < S.n_upper && (flag[q] & kExists) != 0; };
    // the active states from s on, max_region at the most, by ballot (flag[n_upper] is 0)
    const auto count_active = [&](int64_t s) {
        int64_t e = 0;
        for (; e < C.max_region; e += 64) {
            const int64_t q = s + e + lane;
            const bool on = e + lane < C.max_region && q < S.n_upper && (flag[q] & kActive);
            const u64 off = ~__ballot(on);
            if (off) { e += __builtin_ctzll(off); break; }
        }
        return e < C.max_region ? e : C.max_region;
    };
    // findBestCutSite: the candidates spread over the lanes from the top index down, then smaller value, at equal values the larger index
    const auto cut = [&](int64_t s, int64_t e, double next) {
        const auto v_at = [&](int64_t i) { return i == e ? next : value[s + i]; };
        const auto exists = [&](int64_t i) { return state_exists(s + i); };
        double best = 1.7976931348623157e308;
        int64_t best_i = -1;
        for (int64_t i = e - 1 - lane; i >= C.min_region - 1; i -= 64) {
            const double cur = v_at(i);
            if (cur < best && PR::is_minimum(i, v_at, exists)) { best = cur; best_i = i; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double o = __shfl_xor(best, d);
            const int64_t oi = __shfl_xor((long long)best_i, d);
            if (o < best || (o == best && oi > best_i)) { best = o; best_i = oi; }
        }
        return best_i >= 0 ? best_i : e - 1;
    };
    const auto emit = [&](int64_t a, int64_t b) { if (lane == 0) piece_end[a] = (int32_t)b; };
    for (u64 r = wave; r < n_runs; r += n_waves)          // uniform over the wavefront
        if (PR::starts_chain((int64_t)r, heads, tails, C))
            PR::cut_chain((int64_t)r, heads, tails, (int64_t)n_runs, S.first_abs, S.n_loci, C, S.contig_length, p_at, w_at, final_value, state_exists, count_active, cut, emit);
}

__global__ __launch_bounds__(256) void k_emit_regions(const int32_t* __restrict__ piece_end, const u64* __restrict__ rank, u64 n, Shape S, int64_t padding,
                                                      PR::Region* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n && piece_end[i] >= 0) out[rank[i]] = PR::region_of(S.first_abs + (int64_t)i, S.first_abs + piece_end[i], padding, S.contig_length);
}

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- before anything is launched: the parameters, the weights (into w, 2 * kFilterCap + 1 of room), the probabilities
int resolve_weights(const mgx_activity_region_params_t* rp, double* w, int* filter) {
    if (!rp) { set_error("NULL argument"); return -EINVAL; }
    if (rp->band_weights) {
        if (rp->n_band_weights % 2 == 0 || rp->n_band_weights > 2u * PR::kFilterCap + 1) { set_error("n_band_weights must be odd and at most %d", 2 * PR::kFilterCap + 1); return -EINVAL; }
        for (u32 k = 0; k < rp->n_band_weights; ++k) {
            if (!std::isfinite(rp->band_weights[k])) { set_error("weight %u is not finite", k); return -EINVAL; }
            w[k] = rp->band_weights[k];
        }
        *filter = (int)(rp->n_band_weights / 2);
        return 0;
    }
    if (!(rp->sigma > 0) || !std::isfinite(rp->sigma)) { set_error("sigma must be positive and finite"); return -EINVAL; }
    if (rp->max_filter_size < 0 || rp->max_filter_size > PR::kFilterCap) { set_error("max_filter_size must lie in 0..%d", PR::kFilterCap); return -EINVAL; }
    *filter = PR::band_weights(rp->max_filter_size, rp->sigma, rp->adaptive_filter_size != 0, w);
    for (int k = 0; k <= 2 * *filter; ++k) if (!std::isfinite(w[k])) { set_error("sigma %g gives a weight that is not finite", rp->sigma); return -EINVAL; }
    return 0;
}

int check(int32_t interval_start, u32 n_loci, const double* prob, int64_t contig_length, const mgx_activity_region_params_t* rp, int filter,
          const void* out_regions, u64 cap, const u64* n_regions, const u64* n_states) {
    if (!n_regions || !n_states || (cap && !out_regions)) { set_error("NULL argument"); return -EINVAL; }
    if (rp->max_prob_propagation < filter) { set_error("max_prob_propagation %d is below the filter size %d", rp->max_prob_propagation, filter); return -EINVAL; }
    if (rp->min_region_size < 1 || rp->max_region_size < rp->min_region_size) { set_error("region sizes: 1 <= min <= max"); return -EINVAL; }
    if (rp->padding < 0) { set_error("padding is negative"); return -EINVAL; }
    if (!std::isfinite(rp->active_prob_threshold)) { set_error("active_prob_threshold is not finite"); return -EINVAL; }
    if (interval_start < 0 || (u64)interval_start + n_loci > (1ull << 31) || contig_length > (1ll << 31)) { set_error("the interval or the contig ends beyond 2^31"); return -E2BIG; }
    if (contig_length < (int64_t)interval_start + n_loci || contig_length < 1) { set_error("contig_length %lld does not reach beyond the last locus", (long long)contig_length); return -EINVAL; }
    for (u32 l = 0; prob && l < n_loci; ++l)
        if (!(prob[l] >= 0.0 && prob[l] <= 1.0)) { set_error("probability %u is NaN or outside [0, 1]", l); return -EINVAL; }
    return 0;
}

}  // namespace

extern "C" {

void mgx_activity_region_params_defaults(mgx_activity_region_params_t* rp) {
    if (rp) *rp = mgx_activity_region_params_t{50, 100, 50, 300, 50, 1, 0u, 0u, 0.002, 17.0, nullptr};
}

int mgx_activity_band_weights(const mgx_activity_region_params_t* rp, double* out, uint32_t cap, int32_t* filter_size) {
    double w[2 * PR::kFilterCap + 1];
    int filter = 0;
    if (int rc = resolve_weights(rp, w, &filter)) return rc;
    if (filter_size) *filter_size = filter;
    if (cap < 2u * filter + 1) { set_error("%d weights, room for %u", 2 * filter + 1, cap); return -ENOSPC; }
    if (!out) { set_error("NULL argument"); return -EINVAL; }
    memcpy(out, w, (2 * (size_t)filter + 1) * sizeof(double));
    return 0;
}

namespace {
// the regions of one stretch whose values are `prob` on the host or, prob NULL, the 0 / 1 bytes at d_active on the device; validated by the caller
int regions_of(mgx_activity* c, int32_t interval_start, u32 n_loci, const double* prob, const u8* d_active, int64_t contig_length, const mgx_activity_region_params_t* rp,
               const double* w, int filter, mgx_activity_region_t* out_regions, u64 cap, u64* n_regions, double* out_profile, u64 profile_cap, u64* n_states) {
    mgx_activity_regions_work& W = c->regions;
    HIP_TRY(hipSetDevice(c->device));
    for (auto& e : W.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    const Shape S{interval_start, n_loci, PR::states_upper(interval_start, n_loci, filter, contig_length), contig_length};
    const PR::CutParams C{rp->min_region_size, rp->max_region_size, rp->max_prob_propagation, filter};
    const u64 n = (u64)S.n_upper;
    // 2. the layouts: [weights | probabilities] up; [counts: runs, regions | tail flags | values] down; device-only work
    const size_t n_w = 2 * (size_t)filter + 1, o_prob = up256(n_w * 8), up_bytes = o_prob + (prob ? up256((size_t)n_loci * 8) : 0);
    const size_t n_tail = (size_t)(S.n_upper - S.n_loci), o_tail = 256, o_value = o_tail + up256(n_tail + 1), down_bytes = o_value + up256(n * 8);
    const size_t o_piece = up256(n + 1), o_heads = o_piece + up256(n * 4), o_tails = o_heads + up256((n / 2 + 1) * 4), o_rank = o_tails + up256((n / 2 + 1) * 4), o_part = o_rank + up256((n + 1) * 8),
                 work_bytes = o_part + up256((n / mgx_hip::kScanChunk + 2) * 8);
    if (int rc = W.up.reserve(up_bytes)) return rc;
    if (int rc = W.down.reserve(down_bytes)) return rc;
    if (int rc = W.work.reserve(work_bytes, work_bytes + work_bytes / 4)) return rc;
    memcpy(W.up.pin, w, n_w * 8);
    if (prob) memcpy(W.up.pin + o_prob, prob, (size_t)n_loci * 8);
    // 3. one upload, then the kernels on one stream
    hipStream_t s = c->stream;
    const bool timing = (rp->flags & MGX_PAIRHMM_TIMING) != 0;
    const double* d_w = (const double*)W.up.dev; const double* d_prob = (const double*)(W.up.dev + o_prob);          // d_active: the fused call's source
    u64* d_counts = (u64*)W.down.dev; double* d_value = (double*)(W.down.dev + o_value);
    u8* d_flag = W.work.p; int32_t* d_piece = (int32_t*)(W.work.p + o_piece); u32* d_heads = (u32*)(W.work.p + o_heads); u32* d_tails = (u32*)(W.work.p + o_tails);
    u64* d_rank = (u64*)(W.work.p + o_rank); u64* d_part = (u64*)(W.work.p + o_part);
    HIP_TRY(hipMemcpyAsync(W.up.dev, W.up.pin, up_bytes, hipMemcpyHostToDevice, s));
    if (timing) HIP_TRY(hipEventRecord(W.ev[0], s));
    const dim3 tiles((u32)((n + 1 + PR::kBandTile - 1) / PR::kBandTile));
    if (prob) hipLaunchKernelGGL(k_band_pass<double>, tiles, dim3(PR::kBandTile), 0, s, d_prob, d_w, S, filter, rp->active_prob_threshold, d_value, d_flag, d_piece);
    else hipLaunchKernelGGL(k_band_pass<u8>, tiles, dim3(PR::kBandTile), 0, s, d_active, d_w, S, filter, rp->active_prob_threshold, d_value, d_flag, d_piece);
    if (timing) HIP_TRY(hipEventRecord(W.ev[1], s));
    const dim3 per_state((u32)((n + 255) / 256));
    mgx_hip::scan_exclusive(s, RisingFlag{d_flag}, nullptr, n, d_part, d_rank);
    hipLaunchKernelGGL(k_scatter_runs, per_state, dim3(256), 0, s, (const u8*)d_flag, (const u64*)d_rank, n, d_heads, d_tails, d_counts);
    const u32 cut_blocks = (u32)((n / 2 + 1 + 3) / 4 < kCutBlocks ? (n / 2 + 1 + 3) / 4 : kCutBlocks);
    if (prob) hipLaunchKernelGGL(k_cut_runs<double>, dim3(cut_blocks), dim3(256), 0, s, (const u32*)d_heads, (const u32*)d_tails, (const u64*)d_counts, (const u8*)d_flag,
                                 (const double*)d_value, d_prob, d_w, S, C, d_piece);
    else hipLaunchKernelGGL(k_cut_runs<u8>, dim3(cut_blocks), dim3(256), 0, s, (const u32*)d_heads, (const u32*)d_tails, (const u64*)d_counts, (const u8*)d_flag,
                            (const double*)d_value, d_active, d_w, S, C, d_piece);
    mgx_hip::scan_exclusive(s, HoldsPiece{d_piece}, nullptr, n, d_part, d_rank);
    W.stats.n_launches = 9;
    HIP_TRY(hipGetLastError());
    // 4. the counts and the flags of the states behind the last locus
    HIP_TRY(hipMemcpyAsync(d_counts + 1, d_rank + n, 8, hipMemcpyDeviceToDevice, s));
    if (n_tail) HIP_TRY(hipMemcpyAsync(W.down.dev + o_tail, d_flag + S.n_loci, n_tail, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(W.down.pin, W.down.dev, o_value, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const u64 runs = ((const u64*)W.down.pin)[0], regions = ((const u64*)W.down.pin)[1];
    u64 states = n_loci;
    for (size_t k = 0; k < n_tail; ++k) states += (W.down.pin[o_tail + k] & kExists) != 0;
    W.stats.n_states = states; W.stats.n_runs = runs; W.stats.n_regions = regions;
    *n_regions = regions; *n_states = states;
    // 5. the regions, and the values if asked for
    const bool too_many = regions > cap, too_long = out_profile && states > profile_cap;
    if (regions && !too_many && !too_long) {
        if (int rc = W.out.reserve(regions * sizeof(PR::Region))) return rc;
        hipLaunchKernelGGL(k_emit_regions, per_state, dim3(256), 0, s, (const int32_t*)d_piece, (const u64*)d_rank, n, S, (int64_t)rp->padding, (PR::Region*)W.out.dev);
        W.stats.n_launches++;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(W.out.pin, W.out.dev, regions * sizeof(PR::Region), hipMemcpyDeviceToHost, s));
    }
    if (timing) HIP_TRY(hipEventRecord(W.ev[2], s));
    if (out_profile && !too_many && !too_long) HIP_TRY(hipMemcpyAsync(W.down.pin + o_value, d_value, states * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (timing) { HIP_TRY(hipEventElapsedTime(&W.stats.ms_band, W.ev[0], W.ev[1])); HIP_TRY(hipEventElapsedTime(&W.stats.ms_cut, W.ev[1], W.ev[2])); }
    if (too_many) { set_error("%llu regions, room for %llu", (unsigned long long)regions, (unsigned long long)cap); return -ENOSPC; }
    if (too_long) { set_error("%llu states, room for %llu", (unsigned long long)states, (unsigned long long)profile_cap); return -ENOSPC; }
    if (regions) memcpy(out_regions, W.out.pin, regions * sizeof(PR::Region));
    if (out_profile) memcpy(out_profile, W.down.pin + o_value, states * 8);
    return 0;
}
}  // namespace

int mgx_activity_profile_regions(mgx_activity_t* c, int32_t interval_start, uint32_t n_loci, const double* prob, int64_t contig_length,
                                 const mgx_activity_region_params_t* rp, mgx_activity_region_t* out_regions, uint64_t cap, uint64_t* n_regions,
                                 double* out_profile, uint64_t profile_cap, uint64_t* n_states) {
    if (!c) { set_error("NULL argument"); return -EINVAL; }
    c->regions.stats = mgx_activity_region_stats_t{};
    double w[2 * PR::kFilterCap + 1];
    int filter = 0;
    if (int rc = resolve_weights(rp, w, &filter)) return rc;
    if (n_loci && !prob) { set_error("NULL argument"); return -EINVAL; }
    if (int rc = check(interval_start, n_loci, prob, contig_length, rp, filter, out_regions, cap, n_regions, n_states)) return rc;
    *n_regions = 0; *n_states = 0;
    if (n_loci == 0) return 0;
    return regions_of(c, interval_start, n_loci, prob, nullptr, contig_length, rp, w, filter, out_regions, cap, n_regions, out_profile, profile_cap, n_states);
}

int mgx_activity_interval_regions(mgx_activity_t* c, const mgx_activity_input_t* in, const mgx_activity_params_t* p, int64_t contig_length,
                                  const mgx_activity_region_params_t* rp, mgx_activity_region_t* out_regions, uint64_t cap, uint64_t* n_regions,
                                  double* out_profile, uint64_t profile_cap, uint64_t* n_states, uint8_t* out_active, double* out_log_odds, uint32_t* out_depth) {
    if (!c || !in) { set_error("NULL argument"); return -EINVAL; }
    c->regions.stats = mgx_activity_region_stats_t{};
    c->stats = mgx_activity_stats_t{};
    // every argument error of either half before anything is launched
    double w[2 * PR::kFilterCap + 1];
    int filter = 0;
    if (int rc = resolve_weights(rp, w, &filter)) return rc;
    if (int rc = check(in->interval_start, in->n_loci, nullptr, contig_length, rp, filter, out_regions, cap, n_regions, n_states)) return rc;
    *n_regions = 0; *n_states = 0;
    mgx_activity_loci o;
    if (int rc = mgx_activity_launch_loci(c, in, p, true, &o)) return rc;
    if (o.n_loci == 0) return 0;
    // the depth flag, and the per-locus arrays only when one of them is asked for
    if (int rc = mgx_activity_collect_loci(c, o, p, out_active || out_log_odds || out_depth, out_active, out_log_odds, out_depth)) return rc;
    return regions_of(c, in->interval_start, o.n_loci, nullptr, c->down.dev + o.o_active, contig_length, rp, w, filter, out_regions, cap, n_regions, out_profile,
                      profile_cap, n_states);
}

int mgx_activity_region_stats(mgx_activity_t* c, mgx_activity_region_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = c->regions.stats;
    return 0;
}

}  // extern "C"
