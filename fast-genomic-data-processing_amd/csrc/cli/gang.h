// gang.h -- fork-join over a few threads: the CLI's "spawn T threads over [n*t/T, n*(t+1)/T), join".
#pragma once

#include <cstddef>
#include <thread>
#include <vector>

namespace gang {

// Calls fn(t) for t in [0, T) on T threads and joins them.  The caller picks T: the sites' clamps differ on purpose, and
// where the threads first-touch pages, which thread gets which range matters.
template <class Fn>
void run_gang(size_t T, Fn&& fn) {
    std::vector<std::thread> gang;
    for (size_t t = 0; t < T; ++t) gang.emplace_back([&fn, t]() { fn(t); });
    for (auto& th : gang) th.join();
}

// The t-th of T contiguous parts of [0, n): [n*t/T, n*(t+1)/T).
struct Range { size_t begin, end; };
inline Range gang_range(size_t n, size_t t, size_t T) { return {n * t / T, n * (t + 1) / T}; }

}  // namespace gang
