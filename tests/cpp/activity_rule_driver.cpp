// activity_rule_driver.cpp -- runs csrc/activity_rule.h on the CPU in two ways, with the product's own tables (csrc/mgx_tables.cpp):
//   serial     the element of every (read, position) by locate(), every locus over all reads
//   64 lanes   as the kernels group the work: 64 CIGAR elements per round held one per "lane" (inclusive scans, first_end_above over
//              the lane array), and per 64 loci the candidate range [lo, hi) from the running maximum of act_stop and act_start
// Every array lives in a heap block of its exact size, so AddressSanitizer sees any read past an end.  Built and run by
// tests/test_activity_host.py (ASan + UBSan, -Werror).
//   activity_rule_driver cases <file>      input as tests/activity_cases.py::to_text writes it; per case and way: "E <hex bytes>", "L <n>",
//                                          n lines "active depth log_odds" (hex float or nan), then "end"
//   activity_rule_driver tables <n>        n lines "digamma(k) log10_factorial(k)", then 128 lines "eps logEps logOneMinusEps", hex floats
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "activity_rule.h"
#include "mgx_tables.h"

namespace R = mgx_activity_rule;

namespace {
template <typename T> std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}
struct ReadRow {
    int32_t start, mate_start, act_start, act_stop; uint32_t flags, sample, n_cigar, n_bases;
    std::unique_ptr<uint32_t[]> cigar; std::unique_ptr<uint8_t[]> bases, quals;
    size_t elem_off;
    R::Read view() const { return R::Read{cigar.get(), n_cigar, bases.get(), quals.get(), n_bases, start, mate_start, (uint16_t)flags}; }
};

R::Where locate_64_lanes(const ReadRow& rd, uint32_t rel) {
    uint32_t ref_base = 0, read_base = 0;
    for (uint32_t k = 0; k < rd.n_cigar; k += 64) {
        uint32_t ref_end[64], read_end[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t el = k + lane < rd.n_cigar ? rd.cigar[k + lane] : 0u;
            ref_end[lane] = (lane ? ref_end[lane - 1] : ref_base) + R::ref_len(el);
            read_end[lane] = (lane ? read_end[lane - 1] : read_base) + R::read_len(el);
        }
        const uint32_t j = R::first_end_above([&](uint32_t l) { if (l >= 64) abort(); return ref_end[l]; }, rel);
        if (j < 64) return R::Where{k + j, j ? ref_end[j - 1] : ref_base, j ? read_end[j - 1] : read_base};
        ref_base = ref_end[63]; read_base = read_end[63];
    }
    abort();
}

void print_double(double v) { if (std::isnan(v)) printf("nan"); else printf("%a", v); }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    if (!strcmp(argv[1], "tables")) {
        const unsigned n = (unsigned)atoi(argv[2]);
        mgx::ActivityTables t;
        mgx::build_activity_tables(n, &t);
        for (unsigned k = 0; k < n; ++k) { print_double(t.digamma[k]); printf(" "); print_double(t.log10_factorial[k]); printf("\n"); }
        for (int q = 0; q < 128; ++q) { print_double(t.eps[q]); printf(" "); print_double(t.log_eps[q]); printf(" "); print_double(t.log_one_minus_eps[q]); printf("\n"); }
        return 0;
    }
    const uint32_t max_depth = 65535;
    mgx::ActivityTables tables;
    mgx::build_activity_tables(max_depth + 3, &tables);
    const auto dig = exact(tables.digamma), l10 = exact(tables.log10_factorial);
    const R::Tables T{dig.get(), l10.get(), tables.eps, tables.log_eps, tables.log_one_minus_eps};
    std::ifstream f(argv[2]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string word, ref_text;
        int32_t interval_start; uint32_t n_loci; size_t n_reads; R::LocusParams lp; R::ElementParams ep; int min_callable;
        ss >> word >> interval_start >> n_loci >> ref_text >> n_reads >> lp.has_normal >> lp.genotype_germline_sites >> min_callable >> ep.pcr_error_qual >>
            ep.min_base_quality >> lp.initial_log_odds;
        if (!ss || word != "case") { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        const auto ref = exact(std::vector<uint8_t>(ref_text.begin(), ref_text.begin() + n_loci));
        std::vector<ReadRow> reads(n_reads);
        size_t n_elements = 0;
        for (auto& rd : reads) {
            if (!std::getline(f, line)) return 2;
            std::istringstream rs(line);
            std::string bases, quals;
            rs >> rd.start >> rd.mate_start >> rd.flags >> rd.sample >> rd.act_start >> rd.act_stop >> rd.n_cigar;
            std::vector<uint32_t> cg(rd.n_cigar);
            for (auto& e : cg) rs >> e;
            rs >> bases >> quals;
            if (!rs) { fprintf(stderr, "bad read: %s\n", line.c_str()); return 2; }
            if (bases == "-") { bases.clear(); quals.clear(); }
            std::vector<uint8_t> q(bases.size());
            for (size_t i = 0; i < q.size(); ++i) q[i] = (uint8_t)strtoul(quals.substr(2 * i, 2).c_str(), nullptr, 16);
            rd.n_bases = (uint32_t)bases.size();
            rd.cigar = exact(cg); rd.bases = exact(std::vector<uint8_t>(bases.begin(), bases.end())); rd.quals = exact(q);
            rd.elem_off = n_elements;
            if (rd.act_stop >= rd.act_start) n_elements += (size_t)(rd.act_stop - rd.act_start) + 1;
        }
        for (int way = 0; way < 2; ++way) {
            // rule 1
            const auto elem = exact(std::vector<uint8_t>(n_elements, 0));
            for (const auto& rd : reads)
                for (int32_t pos = rd.act_start; pos <= rd.act_stop; ++pos) {
                    const int64_t l = (int64_t)pos - interval_start;
                    if (l < 0 || l >= (int64_t)n_loci) continue;
                    const uint32_t rel = (uint32_t)(pos - rd.start);
                    const R::Where w = way == 0 ? R::locate(rd.cigar.get(), rd.n_cigar, rel) : locate_64_lanes(rd, rel);
                    elem[rd.elem_off + (size_t)(pos - rd.act_start)] = R::element_byte(rd.view(), w, pos, ref[l], ep);
                }
            printf("E ");
            for (size_t i = 0; i < n_elements; ++i) printf("%02x", elem[i]);
            printf("\nL %u\n", n_loci);
            // rule 2
            std::vector<int32_t> run_max(n_reads);
            int32_t top = INT32_MIN;
            for (size_t r = 0; r < n_reads; ++r) { if (reads[r].act_stop >= reads[r].act_start && reads[r].act_stop > top) top = reads[r].act_stop; run_max[r] = top; }
            for (uint32_t l = 0; l < n_loci; ++l) {
                const int32_t p = interval_start + (int32_t)l;
                size_t lo = 0, hi = n_reads;
                if (way == 1) {
                    const uint32_t l0 = l & ~63u;
                    const int32_t p_first = interval_start + (int32_t)l0, p_last = interval_start + (int32_t)(l0 + 63 < n_loci ? l0 + 63 : n_loci - 1);
                    hi = 0;
                    for (size_t b = n_reads; lo < b;) { const size_t m = lo + (b - lo) / 2; if (run_max[m] < p_first) lo = m + 1; else b = m; }
                    for (size_t b = n_reads; hi < b;) { const size_t m = hi + (b - hi) / 2; if (reads[m].act_start <= p_last) hi = m + 1; else b = m; }
                }
                const auto walk = [&](auto fn) {
                    for (size_t i = lo; i < hi; ++i)
                        if (reads[i].act_start <= p && p <= reads[i].act_stop) fn(reads[i].sample, elem[reads[i].elem_off + (size_t)(p - reads[i].act_start)]);
                };
                R::Counts c{0, 0, 0, 0, 0};
                walk([&](uint32_t sample, uint8_t b) { R::count(c, sample, b); });
                double sum = 0;
                if (R::has_sum(c, max_depth)) {
                    const double f_tilde = R::f_tilde_ratio(T, c.tumour - c.alt, c.alt);
                    walk([&](uint32_t sample, uint8_t b) { if (sample == 0 && b) sum += R::alt_term(T, b, f_tilde); });
                }
                const R::Locus L = R::locus_of(T, lp, c, max_depth, sum);
                printf("%u %u ", L.active, L.depth); print_double(L.log_odds); printf("\n");
            }
        }
        printf("end\n");
    }
    return 0;
}
