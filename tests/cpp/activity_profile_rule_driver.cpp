// activity_profile_rule_driver.cpp -- csrc/activity_profile_rule.h's serial pass on the CPU over the cases tests/activity_region_cases.py
// writes.  Every array lives in a heap block of its exact size, so AddressSanitizer sees any read past an end.  Built and run by
// tests/test_activity_regions_host.py (ASan + UBSan, -Werror, -ffp-contract=off).
//   activity_profile_rule_driver cases <file>     per case "R n", n lines "start end ext_start ext_end", "V values", "K weights", "end":
//                                                 one clock from the first state on, every piece in turn
//   activity_profile_rule_driver chains <file>    the same, cut as the kernels group the work: run heads and tails, one chain of runs
//                                                 after the other, each without a look further back than its window
//   activity_profile_rule_driver weights          the default band: "K weights" (hex floats) and "F filter_size"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "activity_profile_rule.h"

namespace PR = mgx_activity_profile_rule;

namespace {
std::vector<double> numbers(const std::string& line, char tag) {
    std::istringstream ss(line);
    std::string word;
    ss >> word;
    if (word.size() != 1 || word[0] != tag) { fprintf(stderr, "expected %c: %.40s\n", tag, line.c_str()); exit(2); }
    std::vector<double> out;
    while (ss >> word) out.push_back(strtod(word.c_str(), nullptr));
    return out;
}
template <typename T> std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}
void print_row(char tag, const double* v, size_t n) {
    printf("%c", tag);
    for (size_t i = 0; i < n; ++i) printf(" %a", v[i]);
    printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "weights")) {
        std::unique_ptr<double[]> w(new double[2 * 50 + 1]);
        const int f = PR::band_weights(50, 17.0, true, w.get());
        print_row('K', w.get(), 2 * (size_t)f + 1);
        printf("F %d\n", f);
        return 0;
    }
    if (argc != 3 || (strcmp(argv[1], "cases") && strcmp(argv[1], "chains"))) return 2;
    const bool chains = !strcmp(argv[1], "chains");
    std::ifstream in(argv[2]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string word, thr;
        long long first, n_loci, contig, prop, padding, mn, mx, n_w;
        ss >> word >> first >> n_loci >> contig >> prop >> thr >> padding >> mn >> mx >> n_w;
        if (!ss || word != "case") { fprintf(stderr, "bad line: %.60s\n", line.c_str()); return 2; }
        std::getline(in, line);
        std::vector<double> wv = numbers(line, 'W');
        std::getline(in, line);
        const std::vector<double> pv = numbers(line, 'P');
        if ((long long)wv.size() != n_w || (long long)pv.size() != n_loci) { fprintf(stderr, "counts\n"); return 2; }
        if (wv.empty()) {
            wv.resize(2 * 50 + 1);
            wv.resize(2 * (size_t)PR::band_weights(50, 17.0, true, wv.data()) + 1);
        }
        const auto w = exact(wv);
        const auto p = exact(pv);
        const int filter = (int)(wv.size() / 2);
        const PR::CutParams c{mn, mx, prop, filter};
        const int64_t upper = n_loci ? PR::states_upper(first, n_loci, filter, contig) : 0;
        std::unique_ptr<double[]> values(new double[(size_t)upper]);
        std::unique_ptr<uint32_t[]> heads(new uint32_t[(size_t)upper / 2 + 1]), tails(new uint32_t[(size_t)upper / 2 + 1]);
        std::vector<PR::Region> regions;
        const int64_t n = PR::serial_pass(first, n_loci, [&](int64_t k) { if (k < 0 || k >= n_loci) abort(); return p[k]; },
                                          [&](int64_t k) { if (k < 0 || k > 2 * filter) abort(); return w[k]; }, c, strtod(thr.c_str(), nullptr), padding, contig,
                                          values.get(), heads.get(), tails.get(), chains, [&](const PR::Region& r) { regions.push_back(r); });
        printf("R %zu\n", regions.size());
        for (const auto& r : regions) printf("%d %d %d %d\n", r.start, r.end, r.ext_start, r.ext_end);
        print_row('V', values.get(), (size_t)n);
        print_row('K', w.get(), wv.size());
        printf("end\n");
    }
    return 0;
}
