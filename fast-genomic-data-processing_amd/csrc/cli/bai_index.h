// bai_index.h -- the BAI index (SAMv1 5.2) of records in output order, as bytes.  Host code only: no file, no device.
#pragma once

#include <algorithm>
#include <map>

#include "bam_writer.h"
#include "gang.h"

namespace bamout {

// appends v as it lies in memory (little-endian hosts): the index's and the BAM header's fields
template <typename T>
inline void put(std::vector<uint8_t>& a, T v) { const uint8_t* p = (const uint8_t*)&v; a.insert(a.end(), p, p + sizeof(T)); }

struct RefIndex {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> linear;
    uint64_t off_beg = ~0ull, off_end = 0, n_mapped = 0, n_unmapped = 0;
};

// One contiguous part of the records (output order) into a fresh index, record by record.
template <typename VOff>
void index_part(const RecordRefs& recs, size_t k0, size_t k1, VOff& voff, std::vector<RefIndex>& idx, uint64_t* n_no_coor) {
    int32_t last_tid = -2; uint32_t last_bin = 0; std::vector<std::pair<uint64_t, uint64_t>>* last_chunks = nullptr;
    for (size_t k = k0; k < k1; ++k) {
        const RecordRef& r = recs[k];
        uint64_t vb, ve;
        voff(k, &vb, &ve);
        if (r.tid < 0 || (size_t)r.tid >= idx.size()) { ++*n_no_coor; continue; }
        RefIndex& ri = idx[r.tid];
        const int64_t beg = std::max<int64_t>(r.beg, 0), end = std::max<int64_t>(r.end, beg + 1);
        // the records are coordinate-sorted: neighbours almost always share their bin, so the map is asked once per run
        const uint32_t bin = (uint32_t)reg2bin(beg, end);
        if (r.tid != last_tid || bin != last_bin) { last_chunks = &ri.bins[bin]; last_tid = r.tid; last_bin = bin; }
        auto& chunks = *last_chunks;
        if (!chunks.empty() && chunks.back().second == vb) chunks.back().second = ve;   // contiguous: extend
        else chunks.emplace_back(vb, ve);
        const size_t w0 = (size_t)(beg >> 14), w1 = (size_t)((end - 1) >> 14);
        if (ri.linear.size() <= w1) ri.linear.resize(w1 + 1, 0);
        for (size_t w = w0; w <= w1; ++w) if (ri.linear[w] == 0 || vb < ri.linear[w]) ri.linear[w] = vb;
        ri.off_beg = std::min(ri.off_beg, vb); ri.off_end = std::max(ri.off_end, ve);
        if (r.mapped) ++ri.n_mapped; else ++ri.n_unmapped;
    }
}

// How many parts index `n` records on `threads` threads (MGX_CLI_BAI_PARTS, for tests: parts on small inputs).
size_t bai_parts(size_t n, int threads);
// Part `from` follows `to` in output order: a bin's chunk lists concatenated, the seam joined where the serial loop would have
// extended a chunk (a part starts every bin with a new chunk, which is contiguous with the previous part's last one exactly when the
// serial rule applies), linear windows by minimum, counters by sum.
void merge_part(RefIndex& to, RefIndex& from);
std::vector<uint8_t> serialise_bai(std::vector<RefIndex>& idx, uint64_t n_no_coor);

// The .bai bytes of the records in output order; voff(k, &vbeg, &vend) gives record k's virtual offsets.  threads > 1 (only for a voff
// that may be called from several threads in any order): the records are indexed in contiguous parts and the parts merged in
// order: the same bytes as the serial index (200 M records: 1.0 s -> 0.15 s).
template <typename VOff>
std::vector<uint8_t> bai_bytes(size_t n_ref, const RecordRefs& recs, VOff&& voff, int threads = 1) {
    std::vector<RefIndex> idx(n_ref);
    uint64_t n_no_coor = 0;
    const size_t T = bai_parts(recs.size(), threads);
    if (T == 1) index_part(recs, 0, recs.size(), voff, idx, &n_no_coor);
    else {
        std::vector<std::vector<RefIndex>> part(T, std::vector<RefIndex>(n_ref));
        std::vector<uint64_t> part_no(T, 0);
        gang::run_gang(T, [&](size_t t) { auto v = voff; const auto r = gang::gang_range(recs.size(), t, T); index_part(recs, r.begin, r.end, v, part[t], &part_no[t]); });
        for (size_t t = 0; t < T; ++t) {
            n_no_coor += part_no[t];
            for (size_t r = 0; r < n_ref; ++r) merge_part(idx[r], part[t][r]);
        }
    }
    return serialise_bai(idx, n_no_coor);
}

}  // namespace bamout
