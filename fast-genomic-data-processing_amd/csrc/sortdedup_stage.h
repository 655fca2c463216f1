// sortdedup_stage.h -- the host-only pieces of mgx_sortdedup.hip's upload path, free of HIP so that
// tests/cpp/test_host_sanitize.cpp can drive them under the address/UB and thread sanitizers.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <thread>
#include <vector>

#include "../../include/mgx_sortdedup.h"

namespace mgx_stage {

// A gang of helper threads that lives for one upload: every staging piece (~1 ms of copying) is split over the gang without
// creating threads per piece (eight std::thread starts cost a quarter of a piece's copy time; cli/gang.h forks per call on purpose).
class Gang {
public:
    explicit Gang(int n) : n_(n < 1 ? 1 : n) {
        for (int t = 1; t < n_; ++t) th_.emplace_back([this, t] { loop(t); });
    }
    ~Gang() {
        stop_.store(true);
        gen_.fetch_add(1);
        for (auto& t : th_) t.join();
    }
    // body(first, last) over [0, n_items) in n contiguous shares; returns when all shares are done
    template <class F>
    void run(size_t n_items, size_t min_per_thread, F body) {
        if (n_ == 1 || n_items < 2 * min_per_thread) { body((size_t)0, n_items); return; }
        const size_t part = (n_items + (size_t)n_ - 1) / (size_t)n_;
        fn_ = [&, part, n_items](int t) { const size_t a = std::min(n_items, (size_t)t * part), b = std::min(n_items, a + part); if (a < b) body(a, b); };
        done_.store(0);
        gen_.fetch_add(1);
        fn_(0);
        while (done_.load() != n_ - 1) std::this_thread::yield();
    }
private:
    void loop(int t) {
        uint64_t seen = 0;
        for (;;) {
            while (gen_.load() == seen) std::this_thread::yield();
            seen = gen_.load();
            if (stop_.load()) return;
            fn_(t);
            done_.fetch_add(1);
        }
    }
    int n_;
    std::vector<std::thread> th_;
    std::function<void(int)> fn_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<int> done_{0};
    std::atomic<bool> stop_{false};
};

// Records src[0, m) as 24-byte wire records at `wire`, split over the gang in shares of at least 65 536 records.  A wire
// record is the low halves of the two 64-bit fields, then the record's second 16 bytes as they are: four 8-byte loads
// and three 8-byte stores, as cheap as the plain copy.  True when some coord or prime5 needs more than 32 bits.
inline bool pack24(Gang& gang, const mgx_rec_t* src, size_t m, void* wire) {
    static_assert(sizeof(mgx_rec_t) == 32 && offsetof(mgx_rec_t, prime5) == 8 && offsetof(mgx_rec_t, mate) == 16, "record layout");
    uint64_t* w = static_cast<uint64_t*>(wire);
    const uint64_t* s64 = reinterpret_cast<const uint64_t*>(src);
    std::atomic<uint64_t> high{0};
    gang.run(m, 65536, [&, w, s64](size_t a, size_t b) {
        uint64_t hi = 0;
        for (size_t i = a; i < b; ++i) {
            const uint64_t c0 = s64[4 * i], p0 = s64[4 * i + 1];
            hi |= c0 | p0;
            w[3 * i] = (c0 & 0xFFFFFFFFull) | (p0 << 32);
            w[3 * i + 1] = s64[4 * i + 2];
            w[3 * i + 2] = s64[4 * i + 3];
        }
        if (hi >> 32) high.fetch_or(1);
    });
    return high.load() != 0;
}

}  // namespace mgx_stage
