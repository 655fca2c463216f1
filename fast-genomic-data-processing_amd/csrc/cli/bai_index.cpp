// bai_index.cpp -- see bai_index.h.
#include "bai_index.h"

#include <cstdlib>

namespace bamout {

size_t bai_parts(size_t n, int threads) {
    size_t T = n >= (1u << 20) ? (size_t)std::max(1, std::min(threads, 32)) : 1;
    if (threads > 1) if (const char* e = getenv("MGX_CLI_BAI_PARTS")) T = (size_t)std::max(1, std::min(atoi(e), 64));
    return std::min(T, std::max<size_t>(n, 1));
}

void merge_part(RefIndex& to, RefIndex& from) {
    for (auto& kv : from.bins) {
        auto& dst = to.bins[kv.first]; auto& src = kv.second;
        size_t first = 0;
        if (!dst.empty() && !src.empty() && dst.back().second == src[0].first) { dst.back().second = src[0].second; first = 1; }
        dst.insert(dst.end(), src.begin() + (std::ptrdiff_t)first, src.end());
    }
    if (to.linear.size() < from.linear.size()) to.linear.resize(from.linear.size(), 0);
    for (size_t w = 0; w < from.linear.size(); ++w)
        if (from.linear[w] != 0 && (to.linear[w] == 0 || from.linear[w] < to.linear[w])) to.linear[w] = from.linear[w];
    to.off_beg = std::min(to.off_beg, from.off_beg); to.off_end = std::max(to.off_end, from.off_end);
    to.n_mapped += from.n_mapped; to.n_unmapped += from.n_unmapped;
}

std::vector<uint8_t> serialise_bai(std::vector<RefIndex>& idx, uint64_t n_no_coor) {
    std::vector<uint8_t> bai;
    bai.insert(bai.end(), {'B', 'A', 'I', 1});
    put<int32_t>(bai, (int32_t)idx.size());
    for (RefIndex& ri : idx) {
        const bool any = !ri.bins.empty();
        put<int32_t>(bai, (int32_t)(ri.bins.size() + (any ? 1 : 0)));
        for (auto& kv : ri.bins) {
            put<uint32_t>(bai, kv.first);
            put<int32_t>(bai, (int32_t)kv.second.size());
            for (auto& c : kv.second) { put<uint64_t>(bai, c.first); put<uint64_t>(bai, c.second); }
        }
        if (any) {                                  // metadata pseudo-bin
            put<uint32_t>(bai, 37450u); put<int32_t>(bai, 2);
            put<uint64_t>(bai, ri.off_beg); put<uint64_t>(bai, ri.off_end);
            put<uint64_t>(bai, ri.n_mapped); put<uint64_t>(bai, ri.n_unmapped);
        }
        // empty windows inherit the previous non-empty offset, as htslib's index does
        uint64_t last = 0;
        for (auto& v : ri.linear) { if (v == 0) v = last; else last = v; }
        put<int32_t>(bai, (int32_t)ri.linear.size());
        for (uint64_t v : ri.linear) put<uint64_t>(bai, v);
    }
    put<uint64_t>(bai, n_no_coor);
    return bai;
}

}  // namespace bamout
