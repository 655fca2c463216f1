// sw_layout_driver.cpp -- csrc/sw_layout.h on the CPU, for tests/test_sw_layout_host.py (built with -Wall -Wextra -Werror under ASan + UBSan).
//   sw_layout_driver FILE
// FILE: "params match mismatch open extend", "paired 0|1", "use16 0|1", "limit BYTES", "slices K", then one "pair len1 len2 strategy" per pair.
// Prints, for the whole batch as one chunk:
//   layout n_jobs bt_bytes n_pairs_i16 n_pairs_strip n_strips
//   job index out_index g rpl len1 len2 bt_off lr_off lc_off sc_off el_off        (launch order; out_index -1: a filler)
//   launch first end max_len2
// and for the chunks the cutter makes of it under the limit, each laid out on its own:
//   cut lo hi sum_of_bounds bt_bytes n_jobs
// and the same for consecutive slices of K pairs (lane groups of chosen partners):
//   slice lo hi sum_of_bounds bt_bytes n_jobs
// The job array holds max_jobs(n) entries and not one more: a layout that needs more runs into the sanitizer.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "sw_layout.h"

using namespace mgx_sw_layout;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: sw_layout_driver FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int P[4] = {25, -50, -110, -6}, paired = 0, use16 = 1;
    unsigned long long limit = 0, slices = 0;
    std::vector<u64> ref_off{0}, alt_off{0};
    std::vector<u8> strategy;
    char key[32];
    while (fscanf(f, "%31s", key) == 1) {
        unsigned long long a, b; int st;
        if (!strcmp(key, "params") && fscanf(f, "%d %d %d %d", &P[0], &P[1], &P[2], &P[3]) == 4) continue;
        if (!strcmp(key, "paired") && fscanf(f, "%d", &paired) == 1) continue;
        if (!strcmp(key, "use16") && fscanf(f, "%d", &use16) == 1) continue;
        if (!strcmp(key, "limit") && fscanf(f, "%llu", &limit) == 1) continue;
        if (!strcmp(key, "slices") && fscanf(f, "%llu", &slices) == 1) continue;
        if (!strcmp(key, "pair") && fscanf(f, "%llu %llu %d", &a, &b, &st) == 3 && a >= 1 && a <= (u64)kMaxLen && b >= 1 && b <= (u64)kMaxLen) {
            ref_off.push_back(ref_off.back() + a); alt_off.push_back(alt_off.back() + b); strategy.push_back((u8)st);
            continue;
        }
        fprintf(stderr, "bad input at '%s'\n", key);
        fclose(f);
        return 2;
    }
    fclose(f);
    const u64 n = strategy.size();
    const mgx_sw16::I16Rule rule(P[0], P[1], P[2], P[3]);
    auto lay_out = [&](u64 lo, u64 hi, std::unique_ptr<SwJob[]>& jobs) {
        jobs.reset(new SwJob[max_jobs((u32)(hi - lo))]);
        return build_jobs(ref_off.data(), alt_off.data(), strategy.data(), lo, hi, paired != 0, use16 != 0, rule, jobs.get());
    };
    std::unique_ptr<SwJob[]> jobs;
    const Layout L = lay_out(0, n, jobs);
    printf("layout %u %llu %llu %llu %llu\n", L.n_jobs, (unsigned long long)L.bt_bytes, (unsigned long long)L.n_pairs_i16,
           (unsigned long long)L.n_pairs_strip, (unsigned long long)L.n_strips);
    for (u32 x = 0; x < L.n_jobs; ++x) {
        const SwJob& J = jobs[x];
        printf("job %u %lld %u %u %u %u %llu %llu %llu %llu %llu\n", x, J.out_index == kNoOutput ? -1ll : (long long)J.out_index, J.g, J.rpl, J.len1, J.len2,
               (unsigned long long)J.bt_off, (unsigned long long)J.lr_off, (unsigned long long)J.lc_off, (unsigned long long)J.sc_off,
               (unsigned long long)J.el_off);
    }
    for (u32 a = 0; a < L.n_jobs;) {
        const Launch l = next_launch(jobs.get(), L.n_jobs, a);
        printf("launch %u %u %u\n", a, l.end, l.max_len2);
        if (l.end <= a) { fprintf(stderr, "next_launch does not advance at %u\n", a); return 1; }
        a = l.end;
    }
    auto report = [&](const char* kind, u64 lo, u64 hi) {
        u64 bound = 0;
        for (u64 p = lo; p < hi; ++p) { const Lens l = pair_lens(ref_off.data(), alt_off.data(), p); bound += chunk_bound(l.l1, l.l2); }
        std::unique_ptr<SwJob[]> part;
        const Layout C = lay_out(lo, hi, part);
        printf("%s %llu %llu %llu %llu %u\n", kind, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)bound, (unsigned long long)C.bt_bytes, C.n_jobs);
    };
    for (u64 lo = 0, hi; limit && lo < n; lo = hi) {
        hi = chunk_end(ref_off.data(), alt_off.data(), n, lo, limit);
        if (hi <= lo) { fprintf(stderr, "chunk_end does not advance at %llu\n", (unsigned long long)lo); return 1; }
        report("cut", lo, hi);
    }
    for (u64 lo = 0; slices && lo < n; lo += slices) report("slice", lo, std::min<u64>(lo + slices, n));
    return 0;
}
