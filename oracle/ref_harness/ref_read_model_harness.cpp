/*
 * oracle/ref_harness/ref_read_model_harness.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Pins the repeat search of the PCR indel model to the reference.  Compiled and linked from the reference where
 * they lie (oracle/Makefile, target _ref/ref_read_model; unresolved symbols of the rest of those translation units are
 * ignored at link time, nothing of them runs):
 *   utils/variant/GATKVariantContextUtils.cpp   findNumberOfRepetitions, both overloads (:59-106)
 *   utils/Utils.cpp                             equalRange (:9-17)
 * MathUtils::fastRound (MathUtils.cpp:65-68) does not link the same way: MathUtils.h reaches boost/multi_array.hpp through
 * read/ReadCache.h, which this build does not have.  It is restated below, one line.
 * The lines around the search cannot be compiled: their translation unit needs the SAMRecord model
 * (haplotypecaller/PairHMMLikelihoodCalculationEngine.cpp).  They are stated below in this project's own words -- the cache table
 * (:45-61), the PCR cap on ins / del (:149-157), the search for the repeat unit behind and ahead of a base (:175-254) and the
 * floors (:256-272) -- keeping what the reference's algorithm does: units are copied byte vectors compared for equality, and
 * every count comes from the linked findNumberOfRepetitions: the 9-argument overload, and the 5-argument one in the units-differ
 * branch (:244).  Two additions that the reference does not have, as include/mgx_pairhmm.h defines them: a rate factor
 * of 0 leaves ins / del to the floor alone, and a constant gap-continuation byte < 0 keeps the caller's bytes.
 *
 * Text in (a file), text out (stdout); byte strings are lower-case hex, "-" is the empty string.
 *   ref_read_model reps FILE    lines "leading unit test" -> lines "n9 n5": the count through the 9-argument overload
 *                               (unit and test string as sub-ranges of padded arrays) and through the 5-argument one
 *   ref_read_model reads FILE   cases "case RATE THRESHOLD GCP N_READS" followed by N_READS lines "mapq bases qual ins del gcp"
 *                               -> per case "cache c0 .. c20" ("cache -" with RATE 0), per read "rl qual ins del gcp": the
 *                               repeat length at every offset, then the modified arrays
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "utils/Utils.h"
#include "utils/variant/GATKVariantContextUtils.h"

using std::vector;

using Bytes = vector<uint8_t>;

// the model's constants (PairHMMLikelihoodCalculationEngine.h:29-31, .cpp:19, QualityUtils.h:17)
constexpr int kLongestUnit = 8, kRepeatCap = 20, kCacheFloor = 10;
constexpr double kCacheStart = 40.0;
constexpr uint8_t kQualityFloor = 6;

static vector<uint8_t> unhex(const std::string& s) {
    vector<uint8_t> v;
    if (s == "-") return v;
    auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)(nib(s[i]) * 16 + nib(s[i + 1])));
    return v;
}
static std::string hex(const vector<uint8_t>& v) {
    if (v.empty()) return "-";
    static const char* d = "0123456789abcdef";
    std::string s;
    for (uint8_t b : v) { s.push_back(d[b >> 4]); s.push_back(d[b & 15]); }
    return s;
}

// ---- this project's own statement of PairHMMLikelihoodCalculationEngine.cpp:45-61, 149-272 around the linked search -------

// MathUtils::fastRound (MathUtils.cpp:65-68): to the nearest integer, halves away from zero
static int round_half_away(double x) { return (int)(x > 0.0 ? x + 0.5 : x - 0.5); }

// the quality that a repeat of 0..20 units caps ins / del at
static Bytes cache_table(int rate) {
    Bytes table(kRepeatCap + 1);
    for (int units = 0; units <= kRepeatCap; ++units) {
        const double q = kCacheStart - std::exp(units / (rate * M_PI));
        table[units] = (uint8_t)std::max(kCacheFloor, round_half_away(q) + 1);
    }
    return table;
}

// the linked 9-argument overload with unit and test string both ranges of one read
static int count_in_read(Bytes& read, int unit_at, int unit_len, int test_at, int test_len, bool leading) {
    const int n = (int)read.size();
    return GATKVariantContextUtils::findNumberOfRepetitions(read.data(), n, unit_at, unit_len, read.data(), n, test_at, test_len, leading);
}

// One direction of the search at base `at`: units of 1, 2, .. 8 bases that end at `at` (behind, counted backwards over
// read[0 .. at]) or start behind it (ahead, counted forwards over the rest).  The first unit found twice or more ends the
// search and is kept as a copy; otherwise the unit stays the single neighbouring base, and the count is that of the last length
// that still fitted into the read.
struct Found { Bytes unit; int count; };
static Found search(Bytes& read, int at, bool ahead) {
    const int n = (int)read.size();
    Found f{Bytes(1, read[ahead ? at + 1 : at]), 0};
    for (int len = 1; len <= kLongestUnit; ++len) {
        const int begin = ahead ? at + 1 : at + 1 - len;
        if (begin < 0 || begin + len > n) break;
        f.count = ahead ? count_in_read(read, begin, len, at + 1, n - at - 1, true) : count_in_read(read, begin, len, 0, at + 1, false);
        if (f.count >= 2) {
            f.unit.assign(read.begin() + begin, read.begin() + begin + len);
            break;
        }
    }
    return f;
}

// the repeat length the PCR model sees at base `at`: behind + ahead where the two units are the same bytes; otherwise the unit
// ahead is counted again behind, through the linked 5-argument overload; at most 20
static int repeat_length_at(Bytes& read, int at) {
    const Found behind = search(read, at, false);
    int total = behind.count;
    if (at + 1 < (int)read.size()) {
        Found ahead = search(read, at, true);
        const int back = ahead.unit == behind.unit
                             ? behind.count
                             : GATKVariantContextUtils::findNumberOfRepetitions(ahead.unit.data(), (int)ahead.unit.size(), read.data(), at + 1, false);
        total = ahead.count + back;
    }
    return std::min(total, kRepeatCap);
}

// every base but the last: ins / del at most the cache value of its repeat length
static void cap_gap_opens(const Bytes& table, Bytes& read, Bytes& ins, Bytes& del) {
    for (int at = 0; at + 1 < (int)read.size(); ++at) {
        const uint8_t c = table[repeat_length_at(read, at)];
        ins[at] = std::min(ins[at], c);
        del[at] = std::min(del[at], c);
    }
}

// base quality at most MAPQ and, below the threshold, 6; ins / del at least 6
static void floor_qualities(int mapq, uint8_t threshold, Bytes& qual, Bytes& ins, Bytes& del) {
    for (size_t at = 0; at < qual.size(); ++at) {
        const uint8_t q = (uint8_t)std::min<int>(qual[at], mapq);
        qual[at] = q < threshold ? kQualityFloor : q;
        ins[at] = std::max(ins[at], kQualityFloor);
        del[at] = std::max(del[at], kQualityFloor);
    }
}

static int run_reps(std::istream& in) {
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        int leading; std::string u, t;
        ls >> leading >> u >> t;
        vector<uint8_t> unit = unhex(u), test = unhex(t);
        // the 9-argument overload on sub-ranges: three bytes of padding on either side that no answer may depend on
        vector<uint8_t> uf(3, 'x'), tf(3, 'y');
        uf.insert(uf.end(), unit.begin(), unit.end()); uf.insert(uf.end(), 3, 'x');
        tf.insert(tf.end(), test.begin(), test.end()); tf.insert(tf.end(), 3, 'y');
        const int n9 = GATKVariantContextUtils::findNumberOfRepetitions(uf.data(), (int)uf.size(), 3, (int)unit.size(), tf.data(), (int)tf.size(), 3,
                                                                        (int)test.size(), leading != 0);
        const int n5 = GATKVariantContextUtils::findNumberOfRepetitions(unit.data(), (int)unit.size(), test.data(), (int)test.size(), leading != 0);
        printf("%d %d\n", n9, n5);
    }
    return 0;
}

static int run_reads(std::istream& in) {
    std::string word;
    while (in >> word) {
        if (word != "case") { fprintf(stderr, "expected 'case', got '%s'\n", word.c_str()); return 2; }
        int rate, thr, gcp_const, n_reads;
        in >> rate >> thr >> gcp_const >> n_reads;
        Bytes table;
        if (rate != 0) {
            table = cache_table(rate);
            printf("cache");
            for (uint8_t c : table) printf(" %d", (int)c);
            printf("\n");
        } else {
            printf("cache -\n");
        }
        for (int r = 0; r < n_reads; r++) {
            int mapq; std::string sb, sq, si, sd, sg;
            in >> mapq >> sb >> sq >> si >> sd >> sg;
            Bytes bases = unhex(sb), qual = unhex(sq), ins = unhex(si), del = unhex(sd), gcp = unhex(sg);
            Bytes rl(bases.size());
            for (size_t at = 0; at < bases.size(); ++at) rl[at] = (uint8_t)repeat_length_at(bases, (int)at);
            if (rate != 0) cap_gap_opens(table, bases, ins, del);
            floor_qualities(mapq, (uint8_t)thr, qual, ins, del);
            if (gcp_const >= 0) std::fill(gcp.begin(), gcp.end(), (uint8_t)gcp_const);      // one constant byte per base (:284-292)
            printf("%s %s %s %s %s\n", hex(rl).c_str(), hex(qual).c_str(), hex(ins).c_str(), hex(del).c_str(), hex(gcp).c_str());
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s reps|reads FILE\n", argv[0]); return 2; }
    std::ifstream in(argv[2]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    const std::string mode = argv[1];
    if (mode == "reps") return run_reps(in);
    if (mode == "reads") return run_reads(in);
    fprintf(stderr, "unknown mode %s\n", argv[1]);
    return 2;
}
