// activity_host_pass.cpp -- csrc/activity_rule.h over one mgx_activity_input_t serially on one host thread: the yardstick tools/dev_activity.py
// prints next to the device call (scale only; the input is taken as mgx_activity_interval has validated it).  Built by that tool into
// tools/bin/; not part of libmgx.so.  activity_profile_host_pass is the same yardstick for the step behind it: csrc/activity_profile_rule.h's
// serial pass over the 0 / 1 values with the default band.
#include <cstdint>
#include <vector>

#include "activity_profile_rule.h"
#include "activity_rule.h"
#include "mgx_activity.h"
#include "mgx_tables.h"

namespace R = mgx_activity_rule;

extern "C" int activity_host_pass(const mgx_activity_input_t* in, const mgx_activity_params_t* p, uint32_t max_depth, uint8_t* out_active,
                                  double* out_log_odds, uint32_t* out_depth) {
    static mgx::ActivityTables tables;
    if (tables.digamma.size() != max_depth + 3) mgx::build_activity_tables(max_depth + 3, &tables);
    const R::Tables T{tables.digamma.data(), tables.log10_factorial.data(), tables.eps, tables.log_eps, tables.log_one_minus_eps};
    const R::ElementParams ep{p->pcr_error_qual, p->min_base_quality};
    const R::LocusParams lp{p->has_normal, p->genotype_germline_sites, p->initial_log_odds};
    const uint64_t n = in->n_reads;
    std::vector<uint64_t> elem_off(n + 1, 0);
    std::vector<int32_t> run_max(n);
    int32_t top = INT32_MIN;
    for (uint64_t r = 0; r < n; ++r) {
        const bool empty = in->act_stop[r] < in->act_start[r];
        elem_off[r + 1] = elem_off[r] + (empty ? 0 : (uint64_t)(in->act_stop[r] - in->act_start[r]) + 1);
        if (!empty && in->act_stop[r] > top) top = in->act_stop[r];
        run_max[r] = top;
    }
    std::vector<uint8_t> elem(elem_off[n], 0);
    for (uint64_t r = 0; r < n; ++r) {
        const uint32_t* cg = in->cigar + in->cigar_off[r];
        const uint32_t n_cigar = (uint32_t)(in->cigar_off[r + 1] - in->cigar_off[r]);
        const R::Read rd{cg, n_cigar, in->bases + in->base_off[r], in->quals + in->base_off[r], (uint32_t)(in->base_off[r + 1] - in->base_off[r]),
                         in->read_start[r], in->mate_start[r], in->flags[r]};
        for (int32_t pos = in->act_start[r]; pos <= in->act_stop[r]; ++pos) {
            const int64_t l = (int64_t)pos - in->interval_start;
            if (l < 0 || l >= (int64_t)in->n_loci) continue;
            elem[elem_off[r] + (uint64_t)(pos - in->act_start[r])] = R::element_byte(rd, R::locate(cg, n_cigar, (uint32_t)(pos - rd.start)), pos, in->ref_bases[l], ep);
        }
    }
    uint64_t lo = 0, hi = 0;
    for (uint32_t l = 0; l < in->n_loci; ++l) {
        const int32_t pos = in->interval_start + (int32_t)l;
        while (lo < n && run_max[lo] < pos) ++lo;
        while (hi < n && in->act_start[hi] <= pos) ++hi;
        const auto walk = [&](auto f) {
            for (uint64_t i = lo; i < hi; ++i)
                if (in->act_start[i] <= pos && pos <= in->act_stop[i]) f(in->sample[i], elem[elem_off[i] + (uint64_t)(pos - in->act_start[i])]);
        };
        R::Counts c{0, 0, 0, 0, 0};
        walk([&](uint32_t sample, uint8_t b) { R::count(c, sample, b); });
        double sum = 0;
        if (R::has_sum(c, max_depth)) {
            const double f_tilde = R::f_tilde_ratio(T, c.tumour - c.alt, c.alt);
            walk([&](uint32_t sample, uint8_t b) { if (sample == 0 && b) sum += R::alt_term(T, b, f_tilde); });
        }
        const R::Locus L = R::locus_of(T, lp, c, max_depth, sum);
        out_active[l] = L.active; out_log_odds[l] = L.log_odds; out_depth[l] = L.depth;
    }
    return 0;
}

// out_regions: room for n_loci + 1 regions.  Returns the number of regions.
extern "C" int64_t activity_profile_host_pass(int32_t interval_start, uint32_t n_loci, const uint8_t* active, int64_t contig_length,
                                              const mgx_activity_region_params_t* rp, mgx_activity_region_t* out_regions) {
    namespace PR = mgx_activity_profile_rule;
    std::vector<double> w(2 * (size_t)rp->max_filter_size + 1);
    const int filter = PR::band_weights(rp->max_filter_size, rp->sigma, rp->adaptive_filter_size != 0, w.data());
    const PR::CutParams c{rp->min_region_size, rp->max_region_size, rp->max_prob_propagation, filter};
    const int64_t upper = PR::states_upper(interval_start, n_loci, filter, contig_length);
    std::vector<double> values((size_t)upper);
    std::vector<uint32_t> heads((size_t)upper / 2 + 1), tails((size_t)upper / 2 + 1);
    int64_t n = 0;
    PR::serial_pass(interval_start, n_loci, [&](int64_t p) { return (double)active[p]; }, [&](int64_t k) { return w[k]; }, c, rp->active_prob_threshold, rp->padding,
                    contig_length, values.data(), heads.data(), tails.data(), false, [&](const PR::Region& r) { out_regions[n++] = mgx_activity_region_t{r.start, r.end, r.ext_start, r.ext_end}; });
    return n;
}
