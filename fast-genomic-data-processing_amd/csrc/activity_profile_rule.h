// activity_profile_rule.h -- BandPassActivityProfile + ActivityProfile::popReadyAssemblyRegions (M2/BandPassActivityProfile.cpp,
// M2/ActivityProfile.cpp, driven as M2/main.cpp:267-328 drives them over one contiguous locus sequence), stated once for the kernels of
// mgx_activity_regions.hip and for the CPU tests (tests/cpp/activity_profile_rule_driver.cpp, ASan + UBSan).  No HIP, no heap, no
// environment.  Indices are relative to the first locus of the call unless a name says `abs`.
//
// Weights.  makeKernel(F, sigma)[i] = exp(-(i - F)(i - F) / (2 sigma sigma)) / (sigma sqrt(2 pi)), i = 0..2F, each divided by their sum
//   taken in index order (MathUtils.cpp:29-52).  Adaptive: F = determineFilterSize(makeKernel(max_filter_size, sigma), 1e-5), the distance
//   from the middle down to the first weight below 1e-5.
// State q exists for q in [0, n_states): n_states - 1 = min(contig_length - 1 - first, max(n_loci - 1, last locus with prob > 0 + F)).
//   Its value is a left fold over the source loci p in ascending order: prob[p] > 0 and |q - p| <= F adds prob[p] * K[q - p + F] (the
//   product rounded, then the sum); prob[p] <= 0 adds prob[p] at p == q alone.  The first term of a state is stored, not added to 0.0
//   (ActivityProfile.cpp:56-68), so a -0.0 stays -0.0.  The translation units that include this header are built with -ffp-contract=off.
// Regions.  Maximal runs of states with value > threshold, each cut from its head: e = min(states left in the run, max_region_size);
//   e == max_region_size -> findBestCutSite: i = e - 1 down to min_region_size - 1, the smallest value that is a local minimum (strict <,
//   so the largest index among equal values); isMinimum(i): i >= 1, i is not the last state of the list, P[i] <= P[i + 1] and
//   P[i] < P[i - 1].  The piece is [head, head + minI].
// The pop clock.  The reference pops a piece that starts at s as soon as the state list holds max_region_size + max_prob_propagation + F
//   states, i.e. after the first locus t with min(contig end, max(t, last locus <= t with prob > 0 + F)) >= s + that - 1 was added.  With
//   max_prob_propagation >= F every state the cut reads is final then except the one at s + max_region_size, read by
//   isMinimum(max_region_size - 1) alone: its value is the same fold over the sources <= t.  max(t, a(t) + F) >= T first holds at
//   t = min(T, first locus >= T - F with prob > 0), so the clock needs F + 1 probabilities and no array.  No such t among the loci: the
//   pop is the forced one behind the last locus and all values are final.  "Last state of the list" is then the last state of the
//   profile; in a clocked pop the list reaches beyond s + max_region_size, so one test serves both: state s + i + 1 does not exist.
//   popReadyAssemblyRegions also returns after it drops an inactive piece, so the piece behind it is popped a locus later: pop_time below.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MGX_APR_FN __host__ __device__ inline
#else
#define MGX_APR_FN inline
#endif

namespace mgx_activity_profile_rule {

constexpr int kFilterCap = 256;          // the largest filter size F a call takes (the band-pass tile holds 2F + 1 weights and a halo of F in LDS)
constexpr int kBandTile = 256;           // states per workgroup of the band-pass kernel
constexpr double kMinProbToKeepInFilter = 1e-5;      // BandPassActivityProfile::MIN_PROB_TO_KEEP_IN_FILTER

struct CutParams { int64_t min_region, max_region, max_prob_propagation; int32_t filter; };

// ---- weights (host: libm)
inline double normal_distribution(double mean, double sd, double x) {      // MathUtils::normalDistribution; M_PI
    return std::exp(-(x - mean) * (x - mean) / (2.0 * sd * sd)) / (sd * std::sqrt(2.0 * 3.14159265358979323846));
}
inline void make_kernel(int filter, double sigma, double* out) {            // out: 2 * filter + 1
    const int band = (filter << 1) + 1;
    for (int i = 0; i < band; ++i) out[i] = normal_distribution(filter, sigma, i);
    double sum = 0.0;
    for (int i = 0; i < band; ++i) sum += out[i];
    for (int i = 0; i < band; ++i) out[i] = out[i] / sum;
}
inline int determine_filter_size(const double* kernel, int band, double min_prob) {
    const int middle = (band - 1) >> 1;
    int end = middle;
    while (end > 0) {
        if (kernel[end - 1] < min_prob) break;
        end--;
    }
    return middle - end;
}
// the weights of BandPassActivityProfile's constructor; max_filter in 0..kFilterCap.  Returns F; out holds 2F + 1 weights (room: 2 * max_filter + 1).
inline int band_weights(int max_filter, double sigma, bool adaptive, double* out) {
    make_kernel(max_filter, sigma, out);
    const int filter = adaptive ? determine_filter_size(out, 2 * max_filter + 1, kMinProbToKeepInFilter) : max_filter;
    make_kernel(filter, sigma, out);
    return filter;
}

// ---- the profile
// one more than the last index a state can have: the states of [n_loci, upper) exist where a source with prob > 0 reaches them
MGX_APR_FN int64_t states_upper(int64_t first_abs, int64_t n_loci, int filter, int64_t contig_length) {
    const int64_t last = first_abs + n_loci - 1 + filter;
    return (last < contig_length - 1 ? last : contig_length - 1) - first_abs + 1;
}
MGX_APR_FN int64_t n_states_of(int64_t first_abs, int64_t n_loci, int64_t last_positive /* -1: none */, int filter, int64_t contig_length) {
    int64_t last = n_loci - 1;
    if (last_positive >= 0 && last_positive + filter > last) last = last_positive + filter;
    const int64_t room = contig_length - 1 - first_abs;
    return (last < room ? last : room) + 1;
}

struct Fold { double value; bool any_positive; };
// prob(p) for p in [0, n_loci), weight(k) for k in [0, 2F]; sources above `limit` are left out
template <typename P, typename W>
MGX_APR_FN Fold fold_state(int64_t q, int64_t n_loci, int filter, P prob, W weight, int64_t limit) {
    int64_t lo = q - filter, hi = q + filter;
    if (lo < 0) lo = 0;
    if (hi > n_loci - 1) hi = n_loci - 1;
    if (hi > limit) hi = limit;
    Fold f{0.0, false};
    bool first = true;
    for (int64_t p = lo; p <= hi; ++p) {
        const double pr = prob(p);
        if (pr > 0.0) {
            const double term = pr * weight(q - p + filter);
            f.value = first ? term : f.value + term;
            first = false; f.any_positive = true;
        } else if (p == q) {
            f.value = first ? pr : f.value + pr;
            first = false;
        }
    }
    return f;
}

// the last locus added before the piece that starts at state s is popped, or -1: the forced pop behind the last locus
template <typename P>
MGX_APR_FN int64_t pop_clock(int64_t s, int64_t first_abs, int64_t n_loci, const CutParams& c, int64_t contig_length, P prob) {
    const int64_t target = s + c.max_region + c.max_prob_propagation + c.filter - 1;      // the list's last state, at the least
    if (first_abs + target > contig_length - 1) return -1;
    int64_t t = target;
    for (int64_t p = target - c.filter; p < target && p < n_loci; ++p)
        if (p >= 0 && prob(p) > 0.0) { t = p; break; }
    return t < n_loci ? t : -1;
}

// value(i): the state at list index i as the cut sees it; exists(i): the list holds index i
template <typename V, typename E>
MGX_APR_FN bool is_minimum(int64_t i, V value, E exists) {
    if (!exists(i + 1) || i < 1) return false;
    const double x = value(i);
    return x <= value(i + 1) && x < value(i - 1);
}
// findBestCutSite(e, min_region) - 1: the last list index of the piece
template <typename V, typename E>
MGX_APR_FN int64_t best_cut(int64_t e, int64_t min_region, V value, E exists) {
    int64_t min_i = e - 1;
    double min_p = 1.7976931348623157e308;      // numeric_limits<double>::max()
    for (int64_t i = min_i; i >= min_region - 1; --i) {
        const double cur = value(i);
        if (cur < min_p && is_minimum(i, value, exists)) { min_p = cur; min_i = i; }
    }
    return min_i;
}

struct Region { int32_t start, end, ext_start, ext_end; };      // absolute, ends inclusive: mgx_activity_region_t
MGX_APR_FN Region region_of(int64_t start_abs, int64_t end_abs, int64_t padding, int64_t contig_length) {      // IntervalUtils::trimIntervalToContig
    const int64_t a = start_abs - padding, b = end_abs + padding;
    return Region{(int32_t)start_abs, (int32_t)end_abs, (int32_t)(a > 0 ? a : 0), (int32_t)(b < contig_length - 1 ? b : contig_length - 1)};
}

// ---- when a piece is popped.  popReadyAssemblyRegions stops after it has dropped an INACTIVE piece (popReadyAssemblyRegion returns
// nullptr for it, ActivityProfile.cpp:126-127), so the piece behind it waits for the next call, one locus later: with tau the last
// locus added before a piece's pop, tau_k = max(ready_k, tau_(k-1) + (piece k - 1 inactive ? 1 : 0)), ready = pop_clock.
constexpr int64_t kForced = INT64_MAX / 4;      // popped behind the last locus: every source is in
struct Clock { int64_t tau; bool prev_inactive; };      // of the piece before; tau -2: there is none
MGX_APR_FN Clock no_piece_before() { return Clock{-2, false}; }
template <typename P>
MGX_APR_FN int64_t pop_time(Clock& k, int64_t s, bool active, int64_t first_abs, int64_t n_loci, const CutParams& c, int64_t contig_length, P prob) {
    const int64_t ready = pop_clock(s, first_abs, n_loci, c, contig_length, prob);
    int64_t t = ready < 0 ? kForced : ready;
    const int64_t after = k.tau >= kForced ? kForced : k.tau + (k.prev_inactive ? 1 : 0);
    if (after > t) t = after;
    if (t >= n_loci - 1) t = kForced;
    k.tau = t; k.prev_inactive = !active;
    return t;
}
// The value of state q as a pop after locus t sees it.  final_value(q): the whole fold, already computed.
template <typename P, typename W, typename V>
MGX_APR_FN double value_at_pop(int64_t q, int64_t t, int64_t n_loci, const CutParams& c, P prob, W weight, V final_value) {
    if (t >= q + c.filter || t >= n_loci - 1) return final_value(q);
    return fold_state(q, n_loci, c.filter, prob, weight, t).value;
}

// Runs as chains.  tau_k = max over j <= k of ready_j + (inactive pieces among j .. k - 1), and ready_j <= x_j + C - 1 while
// ready_k >= x_k + C - 1 - F (x: a piece's first state, C = max_region + max_prob_propagation + F).  With max_region >= 2 an inactive
// piece and its successor cover two states or more, so the pieces that start 2F + 1 states or more before x_k cannot delay piece k: a
// run whose inactive stretch in front is chain_window() long starts a chain that is cut without looking further back.  With
// max_region 1 every state is a piece and a delay never drains: one chain.
MGX_APR_FN int64_t chain_window(const CutParams& c) { return c.max_region >= 2 ? 2 * (int64_t)c.filter + 2 : kForced; }
MGX_APR_FN bool starts_chain(int64_t r, const uint32_t* heads, const uint32_t* tails, const CutParams& c) {
    return r == 0 || (int64_t)heads[r] - ((int64_t)tails[r - 1] + 1) >= chain_window(c);
}
// the inactive pieces of [z, s) are cut at z + k max_region: the first of them that a chain starting at s has to look at
MGX_APR_FN int64_t first_inactive_piece(int64_t z, int64_t s, const CutParams& c) {
    const int64_t w = chain_window(c);
    return s - z <= w ? z : z + (s - w - z) / c.max_region * c.max_region;
}
// The chain that run r0 starts.  heads / tails: first and last state of every run, in order.  count_active(s): the active states from s
// on, max_region at the most; cut(s, e, next): best_cut over the piece at s whose state e has the value next; exists(q); emit(first
// state, last state).  The kernel passes wave-wide count_active and cut; every other step is the same on every lane.
template <typename P, typename W, typename V, typename X, typename N, typename K, typename Emit>
MGX_APR_FN void cut_chain(int64_t r0, const uint32_t* heads, const uint32_t* tails, int64_t n_runs, int64_t first_abs, int64_t n_loci, const CutParams& c,
                          int64_t contig_length, P prob, W weight, V final_value, X exists, N count_active, K cut, Emit emit) {
    Clock k = no_piece_before();
    for (int64_t r = r0; r < n_runs; ++r) {
        const int64_t z = r ? (int64_t)tails[r - 1] + 1 : 0;
        int64_t s = heads[r];
        if (r > r0 && s - z >= chain_window(c)) break;          // the next chain
        for (int64_t x = r == r0 ? first_inactive_piece(z, s, c) : z; x < s; x += c.max_region) pop_time(k, x, false, first_abs, n_loci, c, contig_length, prob);
        for (;;) {
            const int64_t e = count_active(s);
            if (e == 0) break;
            const int64_t t = pop_time(k, s, true, first_abs, n_loci, c, contig_length, prob);
            int64_t len = e;
            if (e == c.max_region) {
                const double next = exists(s + e) ? value_at_pop(s + e, t, n_loci, c, prob, weight, final_value) : 0.0;
                len = cut(s, e, next) + 1;
            }
            emit(s, s + len - 1);
            s += len;
        }
    }
}

// ---- the serial pass: values[n_states], then the regions in order.  emit(Region) per region.  Returns the number of states.
// chains false: one clock from the first state on, every piece in turn.  chains true: as the kernels group the work.
template <typename P, typename W, typename Emit>
inline int64_t serial_pass(int64_t first_abs, int64_t n_loci, P prob, W weight, const CutParams& c, double threshold, int64_t padding, int64_t contig_length,
                           double* values /* states_upper() of them */, uint32_t* heads, uint32_t* tails /* room for a run at every other state */, bool chains,
                           Emit emit) {
    int64_t last_positive = -1;
    for (int64_t p = 0; p < n_loci; ++p) if (prob(p) > 0.0) last_positive = p;
    const int64_t n = n_loci ? n_states_of(first_abs, n_loci, last_positive, c.filter, contig_length) : 0;
    for (int64_t q = 0; q < n; ++q) values[q] = fold_state(q, n_loci, c.filter, prob, weight, n_loci - 1).value;
    const auto active = [&](int64_t q) { return q < n && values[q] > threshold; };
    const auto exists = [&](int64_t q) { return q < n; };
    const auto final_value = [&](int64_t q) { return values[q]; };
    const auto count = [&](int64_t s, bool on) { int64_t e = 0; while (e < c.max_region && s + e < n && active(s + e) == on) ++e; return e; };
    const auto cut = [&](int64_t s, int64_t e, double next) {
        return best_cut(e, c.min_region, [&](int64_t i) { return i == e ? next : values[s + i]; }, [&](int64_t i) { return s + i < n; });
    };
    const auto out = [&](int64_t a, int64_t b) { emit(region_of(first_abs + a, first_abs + b, padding, contig_length)); };
    if (!chains) {
        Clock k = no_piece_before();
        for (int64_t s = 0; s < n;) {
            const bool on = active(s);
            const int64_t e = count(s, on), t = pop_time(k, s, on, first_abs, n_loci, c, contig_length, prob);
            int64_t len = e;
            if (on && e == c.max_region) len = cut(s, e, exists(s + e) ? value_at_pop(s + e, t, n_loci, c, prob, weight, final_value) : 0.0) + 1;
            if (on) out(s, s + len - 1);
            s += len;
        }
        return n;
    }
    int64_t n_runs = 0;
    for (int64_t q = 0; q < n; ++q) {
        if (active(q) && !(q && active(q - 1))) heads[n_runs] = (uint32_t)q;
        if (active(q) && !active(q + 1)) tails[n_runs++] = (uint32_t)q;
    }
    for (int64_t r = 0; r < n_runs; ++r)
        if (starts_chain(r, heads, tails, c))
            cut_chain(r, heads, tails, n_runs, first_abs, n_loci, c, contig_length, prob, weight, final_value, exists, [&](int64_t s) { return count(s, true); }, cut, out);
    return n;
}

}  // namespace mgx_activity_profile_rule
