// sw_i16_rule.h -- which Smith-Waterman pairs may take the packed 16-bit fill (k_sw_fill16, mgx_smithwaterman.hip).  Plain C++, no
// device code: the library includes it, and so does tests/cpp/sw_i16_rule_driver.cpp, which checks the rule on the CPU against a 64-bit
// restatement of the kernel's arithmetic (tests/test_sw_i16_rule_host.py).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace mgx_sw16 {

constexpr int64_t kMaxAlt = 4096;     // two alternates per lane group are staged in LDS as 32-bit words

// Every value k_sw_fill16 computes for a cell of the pair's own matrix, and every difference of two of them, must fit 16 bits.
//   H(i, j) >= the all-diagonal path from the boundary: blo + min(len) * min(match, mismatch, 0)
//   any H, E, F <= the best a path can collect: bhi + min(len) * max(match, mismatch, 0) when gaps cost (open, extend <= 0)
//   one more open / extend / match on top of either: `pad`
// LOW_INIT_VALUE only ever meets a real value as LOW + extend against H + open (first column of E, first row of F) and must lose
// strictly: low = L - |extend| - 1.  MATRIX_MIN_CUTOFF (-1e8) cannot bind inside 16 bits.
struct I16Rule {
    int64_t open, extend, dlo, dhi, pos, a_ext, pad;
    bool gaps_cost;
    I16Rule(int match, int mismatch, int open_, int extend_) : open(open_), extend(extend_), dlo(std::min(match, mismatch)), dhi(std::max(match, mismatch)) {
        pos = std::max<int64_t>({dhi, open, extend, 0});
        a_ext = std::llabs((long long)extend);
        pad = std::llabs((long long)open) + a_ext + std::max(std::llabs((long long)match), std::llabs((long long)mismatch));
        gaps_cost = open <= 0 && extend <= 0;
    }
    // lh <= every H, E, F of the matrix <= u0; lo / up: with one more term on either; low: the pair's LOW_INIT_VALUE; ll = low + extend at its lowest
    struct Bounds { int64_t lh, u0, lo, up, low, ll; };
    Bounds bounds(int64_t n, int64_t m) const {
        const int64_t mx = std::max(n, m), mn = std::min(n, m);
        const int64_t b_end = open + (mx - 1) * extend;
        const int64_t blo = std::min<int64_t>({0, open, b_end}), bhi = std::max<int64_t>({0, open, b_end});
        Bounds b;
        b.u0 = gaps_cost ? bhi + mn * std::max<int64_t>(dhi, 0) : bhi + (n + m) * pos;
        b.lh = blo + mn * std::min<int64_t>(dlo, 0);
        b.lo = b.lh - pad; b.up = b.u0 + pad;
        b.low = b.lo - a_ext - 1; b.ll = b.low - a_ext;
        return b;
    }
    bool admits(int64_t n, int64_t m, int32_t* low16) const {
        if (m > kMaxAlt) return false;
        const Bounds b = bounds(n, m);
        if (b.ll < -32768 || b.up > 32767 || b.up - b.ll > 32767) return false;
        *low16 = (int32_t)b.low;
        return true;
    }
};

}  // namespace mgx_sw16
