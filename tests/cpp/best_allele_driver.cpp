// best_allele_driver.cpp -- folds csrc/best_allele_rule.h in several groupings for tests/test_best_allele_host.py (CPU, ASan + UBSan).
// Input (a file): one row per line, "<has_priorities> <n> v[0] .. v[n-1] [p[0] .. p[n-1]]", doubles as strtod reads them (hex floats,
// -inf).  Output: per row "<serial> <lanes> <tree> <tree> <tree>" -- the best allele by a serial left fold, by 64 strided lanes folded
// across with a butterfly (what pairhmm_best_allele_rows does; every lane must end with the same result) and by three random split
// trees with randomly swapped operands.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "best_allele_rule.h"

namespace BA = mgx_best_allele;

struct Row { std::vector<double> v, p; bool has_pri; };

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

static BA::Top top_at(const Row& r, uint32_t a) { return BA::top_of(r.v[a], a); }
static BA::Cand cand_at(const Row& r, const BA::Top& best, uint32_t a) { return BA::cand_of(best, BA::top_of(r.v[a], a).v, r.p[a], a); }
static uint32_t finish(const Row& r, const BA::Top& best, const BA::Cand& c) {
    if (!r.has_pri || r.v.size() < 2) return best.at == BA::kNone ? 0u : best.at;
    return BA::result(best, r.p[best.at], c);
}

static uint32_t serial(const Row& r) {
    const uint32_t n = (uint32_t)r.v.size();
    BA::Top top = BA::top_identity();
    for (uint32_t a = 0; a < n; ++a) top = BA::merge(top, top_at(r, a));
    BA::Cand c = BA::cand_identity();
    if (r.has_pri) for (uint32_t a = 0; a < n; ++a) c = BA::merge(c, cand_at(r, top, a));
    return finish(r, top, c);
}

template <typename T>
static bool butterfly(std::vector<T>& lane, bool (*same)(const T&, const T&)) {
    for (int off = 32; off > 0; off >>= 1) {
        std::vector<T> next(64);
        for (int l = 0; l < 64; ++l) next[l] = BA::merge(lane[l], lane[l ^ off]);
        lane = next;
    }
    for (int l = 1; l < 64; ++l) if (!same(lane[0], lane[l])) return false;
    return true;
}
static bool same_top(const BA::Top& a, const BA::Top& b) { return a.at == b.at && (a.v == b.v || (a.v != a.v && b.v != b.v)); }
static bool same_cand(const BA::Cand& a, const BA::Cand& b) { return a.at == b.at && a.entered == b.entered && (a.at == BA::kNone || a.pri == b.pri); }

static uint32_t lanes(const Row& r) {
    const uint32_t n = (uint32_t)r.v.size();
    std::vector<BA::Top> top(64, BA::top_identity());
    for (uint32_t l = 0; l < 64; ++l) for (uint32_t a = l; a < n; a += 64) top[l] = BA::merge(top[l], top_at(r, a));
    if (!butterfly(top, same_top)) { fprintf(stderr, "the lanes disagree after the first butterfly\n"); exit(2); }
    std::vector<BA::Cand> c(64, BA::cand_identity());
    if (r.has_pri) {
        for (uint32_t l = 0; l < 64; ++l) for (uint32_t a = l; a < n; a += 64) c[l] = BA::merge(c[l], cand_at(r, top[0], a));
        if (!butterfly(c, same_cand)) { fprintf(stderr, "the lanes disagree after the second butterfly\n"); exit(2); }
    }
    return finish(r, top[0], c[0]);
}

template <typename T, typename Leaf>
static T tree_fold(uint32_t lo, uint32_t hi, T identity, const Leaf& leaf) {
    if (hi == lo) return identity;
    if (hi - lo == 1) return leaf(lo);
    const uint32_t mid = lo + 1 + rnd() % (hi - lo - 1);
    const T a = tree_fold(lo, mid, identity, leaf), b = tree_fold(mid, hi, identity, leaf);
    return (rnd() & 1) ? BA::merge(a, b) : BA::merge(b, a);
}
static uint32_t tree(const Row& r) {
    const uint32_t n = (uint32_t)r.v.size();
    const BA::Top top = tree_fold(0u, n, BA::top_identity(), [&](uint32_t a) { return top_at(r, a); });
    BA::Cand c = BA::cand_identity();
    if (r.has_pri) c = tree_fold(0u, n, BA::cand_identity(), [&](uint32_t a) { return cand_at(r, top, a); });
    return finish(r, top, c);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s rows.txt\n", argv[0]); return 1; }
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        int has_pri; size_t n;
        if (!(ss >> has_pri >> n)) { fprintf(stderr, "bad line\n"); return 1; }
        Row r; r.has_pri = has_pri != 0;
        std::string tok;
        for (size_t k = 0; k < n * (r.has_pri ? 2 : 1); ++k) {
            if (!(ss >> tok)) { fprintf(stderr, "short line\n"); return 1; }
            (k < n ? r.v : r.p).push_back(strtod(tok.c_str(), nullptr));
        }
        printf("%u %u %u %u %u\n", serial(r), lanes(r), tree(r), tree(r), tree(r));
    }
    return 0;
}
