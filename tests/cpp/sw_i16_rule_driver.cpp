// sw_i16_rule_driver.cpp -- the admission rule of the packed 16-bit Smith-Waterman fill (csrc/sw_i16_rule.h) on the CPU, next to a
// 64-bit restatement of what k_sw_fill16 computes (csrc/mgx_smithwaterman.hip, sw_fill16_body).  Meant to be run under
// AddressSanitizer + UBSan (tests/test_sw_i16_rule_host.py); the GPU tests take every expected admission from it.
//
//   sw_i16_rule_driver admits [FILE]   lines `match mismatch open extend n m`
//       -> `A low16 lh u0 pad up ll`   A = 1 admitted / 0 refused; the rest are the rule's own names (low16 = 0 where refused)
//   sw_i16_rule_driver model [FILE]    lines `pair match mismatch open extend strategy REF ALT`
//                                         or `rand match mismatch open extend strategy n m count seed`   (count random pairs, half of
//                                                                                 them an alternate that is a mutated copy of the reference)
//       -> `ok rmin rmax amin amax dmin dmax margin wrong`  or  `refused`
//          rmin / rmax  extrema of every REAL value below (nothing derived from low16)
//          amin / amax  the same with low16, low16 + extend and the four parameters included: all of it sits in 16-bit halves
//          dmin / dmax  extrema of the four differences whose sign bit the kernel takes
//          margin       min of (H + open) - (low16 + extend) where the two meet; > 0 means low16 loses strictly
//          wrong        cells whose H or decision nibble differ from the same recurrence with LOW_INIT_VALUE = INT32_MIN / 2
//   FILE defaults to stdin.
//
// What the kernel forms for cell (i, j) of a pair's own matrix, i = 1 .. n (rows: reference), j = 1 .. m (columns: alternate), by the
// statement of sw_fill16_body it stands for.  All are 16-bit halves; sums wrap silently, pk_max and the sign bits read them as signed.
//   boundaries   hl[k] = H(i, 0), diag_in = H(r0, 0), bnd / bstep = H(0, j): open + (x - 1) * extend under INDEL / LEADING_INDEL, else 0;
//                H(0, 0) = 0; gs[k] = E(i, 0) = low16; lane 0's up_g = F(0, j) = low16; vopen, vext, vmatch from pk2(): the parameters
//   open_s = hl[k] + vopen            H(i, j-1) + open
//   ext_s  = gs[k] + vext             E(i, j-1) + extend         (j = 1: low16 + extend)
//   ee     = pk_max(open_s, ext_s)    E(i, j)
//   open_c = up_h + vopen             H(i-1, j) + open
//   ext_c  = up_g + vext              F(i-1, j) + extend         (i = 1: low16 + extend)
//   ff     = pk_max(ext_c, open_c)    F(i, j)
//   h0     = diag + pk_mad(ne, vdelta, vmatch)    H(i-1, j-1) + (match | mismatch).  vdelta = mismatch - match may itself wrap: the
//                                     multiply-add is modular and its result, match or mismatch, is what has to fit
//   m1     = pk_max(h0, ee)
//   h      = pk_max(m1, ff)           H(i, j)
//   t1 = ext_s - open_s   sign: E opened            t2 = ext_c - open_c   sign: F opened
//   t3 = h0 - ee          sign: E beats the diagonal        t4 = m1 - ff          sign: F beats max(diagonal, E)
// The kernel has no MATRIX_MIN_CUTOFF: inside 16 bits it cannot bind.  Cells beyond (n, m) -- the partner's columns, padding rows -- are
// not modelled: nothing real reads them.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "sw_i16_rule.h"

using mgx_sw16::I16Rule;

namespace {

constexpr int kIndel = 10, kLeadingIndel = 11;      // MGX_SW_INDEL, MGX_SW_LEADING_INDEL (include/mgx_smithwaterman.h)
constexpr int64_t kLowInit = INT32_MIN / 2;

struct Extrema {
    int64_t rmin = INT64_MAX, rmax = INT64_MIN, amin = INT64_MAX, amax = INT64_MIN, dmin = INT64_MAX, dmax = INT64_MIN, margin = INT64_MAX;
    long wrong = 0;
    void real(int64_t v) { rmin = std::min(rmin, v); rmax = std::max(rmax, v); any(v); }
    void any(int64_t v) { amin = std::min(amin, v); amax = std::max(amax, v); }
    void diff(int64_t v) { dmin = std::min(dmin, v); dmax = std::max(dmax, v); }
};

struct Cell { int64_t h, e, f; int nib; };

// one cell with `low` standing in for LOW_INIT_VALUE; X (may be null) collects what the kernel forms
Cell cell(int64_t hl, int64_t el, bool el_real, int64_t hu, int64_t fu, bool fu_real, int64_t hd, bool eq, int match, int mismatch, int open,
          int extend, Extrema* X) {
    const int64_t open_s = hl + open, ext_s = el + extend, ee = std::max(open_s, ext_s);
    const int64_t open_c = hu + open, ext_c = fu + extend, ff = std::max(ext_c, open_c);
    const int64_t h0 = hd + (eq ? match : mismatch), m1 = std::max(h0, ee), h = std::max(m1, ff);
    const int64_t t1 = ext_s - open_s, t2 = ext_c - open_c, t3 = h0 - ee, t4 = m1 - ff;
    if (X) {
        for (int64_t v : {hl, hu, hd, open_s, open_c, ee, ff, h0, m1, h}) X->real(v);
        if (el_real) X->real(ext_s); else { X->any(el); X->any(ext_s); X->margin = std::min(X->margin, open_s - ext_s); }
        if (fu_real) X->real(ext_c); else { X->any(fu); X->any(ext_c); X->margin = std::min(X->margin, open_c - ext_c); }
        for (int64_t v : {t1, t2, t3, t4}) X->diff(v);
    }
    return Cell{h, ee, ff, (t1 < 0 ? 8 : 0) | (t2 < 0 ? 4 : 0) | (t3 < 0 ? 2 : 0) | (t4 < 0 ? 1 : 0)};
}

void model_pair(const std::string& ref, const std::string& alt, int strategy, int match, int mismatch, int open, int extend, int64_t low16, Extrema& X) {
    const size_t n = ref.size(), m = alt.size();
    const bool indel = strategy == kIndel || strategy == kLeadingIndel;
    auto bnd = [&](size_t x) -> int64_t { return x == 0 ? 0 : indel ? (int64_t)open + (int64_t)(x - 1) * extend : 0; };
    for (int64_t v : {(int64_t)match, (int64_t)mismatch, (int64_t)open, (int64_t)extend}) X.any(v);
    // row i - 1 of both recurrences: [0] with low16, [1] with LOW_INIT_VALUE
    std::vector<int64_t> hp[2], fp[2];
    for (int w = 0; w < 2; ++w) {
        hp[w].resize(m + 1); fp[w].assign(m + 1, w ? kLowInit : low16);
        for (size_t j = 0; j <= m; ++j) hp[w][j] = bnd(j);
    }
    for (size_t i = 1; i <= n; ++i) {
        int64_t hl[2] = {bnd(i), bnd(i)}, el[2] = {low16, kLowInit}, hd[2] = {bnd(i - 1), bnd(i - 1)};
        for (size_t j = 1; j <= m; ++j) {
            const bool eq = ref[i - 1] == alt[j - 1];
            Cell c[2];
            for (int w = 0; w < 2; ++w) {
                c[w] = cell(hl[w], el[w], j > 1, hp[w][j], fp[w][j], i > 1, hd[w], eq, match, mismatch, open, extend, w ? nullptr : &X);
                hd[w] = hp[w][j]; hp[w][j] = c[w].h; fp[w][j] = c[w].f; hl[w] = c[w].h; el[w] = c[w].e;
            }
            if (c[0].h != c[1].h || c[0].nib != c[1].nib) X.wrong++;
        }
    }
}

bool next_line(std::istream& in, std::string& line) {
    while (std::getline(in, line)) if (!line.empty() && line[0] != '#') return true;
    return false;
}

int run_admits(std::istream& in) {
    std::string line;
    while (next_line(in, line)) {
        std::istringstream ss(line);
        long long match, mismatch, open, extend, n, m;
        if (!(ss >> match >> mismatch >> open >> extend >> n >> m) || n < 1 || m < 1) { fprintf(stderr, "bad admits line: %s\n", line.c_str()); return 2; }
        const I16Rule rule((int)match, (int)mismatch, (int)open, (int)extend);
        int32_t low16 = 0;
        const bool ok = rule.admits(n, m, &low16);
        const I16Rule::Bounds b = rule.bounds(n, m);
        printf("%d %d %lld %lld %lld %lld %lld\n", ok ? 1 : 0, ok ? low16 : 0, (long long)b.lh, (long long)b.u0, (long long)rule.pad, (long long)b.up, (long long)b.ll);
    }
    return 0;
}

int run_model(std::istream& in) {
    std::string line;
    while (next_line(in, line)) {
        std::istringstream ss(line);
        std::string kind;
        long long match, mismatch, open, extend, strategy;
        if (!(ss >> kind >> match >> mismatch >> open >> extend >> strategy) || (kind != "pair" && kind != "rand")) { fprintf(stderr, "bad model line: %.80s\n", line.c_str()); return 2; }
        const I16Rule rule((int)match, (int)mismatch, (int)open, (int)extend);
        Extrema X;
        int32_t low16 = 0;
        if (kind == "pair") {
            std::string ref, alt;
            if (!(ss >> ref >> alt)) { fprintf(stderr, "bad pair line: %.80s\n", line.c_str()); return 2; }
            if (!rule.admits((int64_t)ref.size(), (int64_t)alt.size(), &low16)) { printf("refused\n"); continue; }
            model_pair(ref, alt, (int)strategy, (int)match, (int)mismatch, (int)open, (int)extend, low16, X);
        } else {
            long long n, m, count, seed;
            if (!(ss >> n >> m >> count >> seed) || n < 1 || m < 1) { fprintf(stderr, "bad rand line: %.80s\n", line.c_str()); return 2; }
            if (!rule.admits(n, m, &low16)) { printf("refused\n"); continue; }
            std::mt19937_64 rng((uint64_t)seed);
            std::string ref((size_t)n, 'A'), alt((size_t)m, 'A');
            for (long long c = 0; c < count; ++c) {
                for (auto& ch : ref) ch = "ACGT"[rng() & 3];
                for (auto& ch : alt) ch = "ACGT"[rng() & 3];
                if (c & 1) {                                            // the alternate follows the reference from a random start, one base in eight changed
                    const size_t s = (size_t)(rng() % (uint64_t)n);
                    for (size_t j = 0; j < (size_t)m && s + j < (size_t)n; ++j) if (rng() & 7) alt[j] = ref[s + j];
                }
                model_pair(ref, alt, (int)strategy, (int)match, (int)mismatch, (int)open, (int)extend, low16, X);
            }
        }
        printf("ok %lld %lld %lld %lld %lld %lld %lld %ld\n", (long long)X.rmin, (long long)X.rmax, (long long)X.amin, (long long)X.amax, (long long)X.dmin,
               (long long)X.dmax, (long long)X.margin, X.wrong);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || argc > 3) { fprintf(stderr, "usage: %s admits|model [FILE]\n", argv[0]); return 2; }
    const std::string cmd = argv[1];
    std::ifstream file;
    if (argc == 3) {
        file.open(argv[2]);
        if (!file) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    }
    std::istream& in = argc == 3 ? static_cast<std::istream&>(file) : std::cin;
    if (cmd == "admits") return run_admits(in);
    if (cmd == "model") return run_model(in);
    fprintf(stderr, "unknown command %s\n", cmd.c_str());
    return 2;
}
