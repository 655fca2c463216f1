// sw_layout.h -- the jobs of a Smith-Waterman chunk and their places in the back-trace arena (mgx_smithwaterman.hip): classes, launch order, lane
// groups, region sizes, the chunk bound, the launches.  Integer arithmetic on the lengths alone, no HIP: the library includes it for host and device
// (a kernel may call a constexpr function), and tests/cpp/sw_layout_driver.cpp prints it for tests/test_sw_layout_host.py (CPU, ASan + UBSan).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "sw_i16_rule.h"

namespace mgx_sw_layout {
typedef uint8_t u8; typedef uint32_t u32; typedef uint64_t u64;

constexpr int kMaxRef = 2048;                    // 64 lanes x 32 rows
constexpr int kStripRpl = 32;                    // k_sw_fill_strip (MGX_SW_LONG_REF): rows per lane ...
constexpr int kStripRows = 64 * kStripRpl;       // ... and per strip
constexpr int kMaxLen = 32767;                   // the reference's lengths are int16_t (IntelSmithWaterman.cc:77)
constexpr u32 kPairedFrom = 8192;                // pairs in a chunk from which two lane groups share a wavefront

struct SwJob {
    u64 off1, off2;      // into the uploaded ref / alt bytes
    u64 bt_off;          // back-trace arena, bytes
    u64 sc_off;          // score arena (int32): last_row[ncol + 1] then last_col[nrow + 1]
    u64 el_off;          // element arena (int16): 2 * (len1 + len2 + 2)
    u32 len1, len2, rpl, strategy, out_index;
    u32 g;               // bits 0-7: lanes per pair (32 or 64) | kJobI16 | kJobHalf | kJobStrip
    u64 lr_off;          // 16-bit fill: the last lane's H values per swept position (back-trace arena, bytes)
                         // strip fill: the pair's boundary array, (H, F) of a strip's bottom row per column
    u64 lc_off;          // 16-bit fill: every lane's packed H values at the pair's last swept position
    int32_t low16;       // 16-bit fill: this pair's stand-in for LOW_INIT_VALUE
    u32 pad_;
};
constexpr u32 kJobI16 = 0x200u;     // k_sw_fill16: packed 16-bit scores, two pairs per lane group, back-trace nibbles
constexpr u32 kJobHalf = 0x400u;    // k_sw_fill16: this pair is the high half of its lane group
constexpr u32 kJobStrip = 0x800u;   // k_sw_fill_strip: the reference is cut into strips of kStripRows rows, written one after another
constexpr u32 kNoOutput = 0xFFFFFFFFu;   // out_index of a filler job (a 16-bit class is padded to whole wavefronts)
constexpr u32 max_jobs(u32 n_pairs) { return n_pairs + 256; }     // fillers: at most 3 per 16-bit class, 18 classes of either width

struct Shape { int g, rpl; };         // lanes per pair and reference positions per lane
// The lanes own the reference and sweep the alternate.  Up to 256 reference positions two pairs share a wavefront (32 lanes x 1..8) whenever
// the batch is large enough to fill the device that way; otherwise, and beyond, one pair per wavefront (64 lanes x 1..32) so that every SIMD
// still has several wavefronts to hide the dependent integer chain of a step behind.
inline Shape shape_for(int len1, bool paired) {
    if (paired) for (int r : {1, 2, 3, 4, 5, 6, 7, 8, 12, 16}) if (len1 <= 32 * r) return Shape{32, r};
    for (int r : {1, 2, 3, 4, 5, 6, 8, 16, 32}) if (len1 <= 64 * r) return Shape{64, r};
    return Shape{0, 0};
}
// the packed 16-bit fill (k_sw_fill16); admission: I16Rule (sw_i16_rule.h)
inline Shape shape16_for(int len1, bool paired) {
    static const int cls[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 20, 24, 32};
    if (paired) for (int r : cls) if (len1 <= 32 * r) return Shape{32, r};
    for (int r : cls) if (len1 <= 64 * r) return Shape{64, r};
    return Shape{0, 0};
}
// ---- region sizes.  Back-trace bytes of one lane and step: RPL of them, in a slot of whole 32-bit words from three positions per lane up
// (a 5-, 6- or 7-byte slot would be stored byte by byte); the 16-bit form keeps a nibble per row and pair, one word per four rows.
constexpr int bt_slot(int rpl) { return rpl <= 2 ? rpl : (rpl + 3) & ~3; }
constexpr int bt_slot16(int rpl) { return 4 * ((rpl + 3) / 4); }
constexpr u64 up16(u64 bytes) { return (bytes + 15) & ~15ull; }
constexpr u64 lanes_of(u64 len1, const Shape& sh) { return (len1 + sh.rpl - 1) / sh.rpl; }
constexpr u64 bt_bytes(u64 len1, u64 len2, const Shape& sh) { return up16((len2 + lanes_of(len1, sh)) * sh.g * bt_slot(sh.rpl)); }     // steps + 1 slots
constexpr u64 bt_bytes16(u64 steps_max, const Shape& sh) { return up16((steps_max + 1) * sh.g * bt_slot16(sh.rpl)); }
constexpr u64 lr_bytes16(u64 n_swp, const Shape& sh) { return up16((n_swp + 1) * sh.rpl * 4); }
constexpr u64 lc_bytes16(u64 n_lanes, const Shape& sh) { return up16(n_lanes * sh.rpl * 4); }
// the strip form: full strips at strip_bt_stride, then the last one with the lanes it has; and the boundary array
constexpr u64 strip_bt_stride(u64 ncol) { return (ncol + 64) * 64 * bt_slot(kStripRpl); }   // steps + 1 = ncol + 64
constexpr u64 n_strips_of(u64 len1) { return (len1 + kStripRows - 1) / kStripRows; }
constexpr u64 bt_bytes_strip(u64 len1, u64 len2) {
    const u64 full = n_strips_of(len1) - 1;
    return full * strip_bt_stride(len2) + bt_bytes(len1 - full * kStripRows, len2, Shape{64, kStripRpl});
}
constexpr u64 bnd_bytes_strip(u64 len2) { return up16((len2 + 1) * 8); }
// ---- chunks.  An upper bound of what a pair takes of the back-trace arena in any shape: the one-pair-per-wavefront 32-bit form (the paired
// form and the 16-bit form are smaller) plus the 16-bit kernel's edge rows; a reference of more than kMaxRef bases has one shape only, its
// strips and its boundary array, to the byte.  The bound only steers the cuts (the arena is reserved at the size build_jobs returns).
constexpr u64 chunk_bound(u64 l1, u64 l2) {
    const u64 rows = (l1 + 63) / 64, slot = rows <= 8 ? ((rows + 3) & ~3ull) : rows <= 16 ? 16 : 32;
    return l1 > (u64)kMaxRef ? bt_bytes_strip(l1, l2) + bnd_bytes_strip(l2)
                             : (l2 + 64 + 1) * 64 * slot + 8 * (l2 + 1) * ((l1 + 31) / 32 * 3 / 2 + 2) + 8 * (l1 + 64) + 64;
}
struct Lens { u64 l1, l2; };
inline Lens pair_lens(const u64* ref_off, const u64* alt_off, u64 p) { return Lens{ref_off[p + 1] - ref_off[p], alt_off[p + 1] - alt_off[p]}; }
// the end of the chunk that starts at pair lo: as many pairs as the limit holds by their bounds, one at the least
inline u64 chunk_end(const u64* ref_off, const u64* alt_off, u64 n_pairs, u64 lo, u64 limit) {
    u64 hi = lo, bt = 0;
    for (; hi < n_pairs; ++hi) {
        const Lens l = pair_lens(ref_off, alt_off, hi);
        if (hi > lo && bt + chunk_bound(l.l1, l.l2) > limit) break;
        bt += chunk_bound(l.l1, l.l2);
    }
    return hi;
}
// ---- the jobs of pairs [lo, hi), written to jobs[max_jobs(hi - lo)] in launch order.  Per pair in input order: class and admission.  Then
// launch order: the packed 16-bit classes first (32 lanes, then 64; most rows per lane first), the 32-bit classes after them, longest
// alternate first inside a class (the two pairs of a lane group and the groups of a wavefront finish together; a launch drains on its
// cheapest jobs).  Two counting sorts: a comparison sort of 10^5 jobs costs more than their alignments.  The score and element arenas are
// laid out in input order: pair q's score rows start at (bases before it) + 2 q.
struct Layout { u32 n_jobs; u64 bt_bytes, n_pairs_i16, n_pairs_strip, n_strips; };
inline Layout build_jobs(const u64* ref_off, const u64* alt_off, const u8* strategy, u64 lo, u64 hi, bool paired, bool use16,
                         const mgx_sw16::I16Rule& rule, SwJob* jobs) {
    const u32 n = (u32)(hi - lo);
    Layout L{};
    struct Pre { u32 len1, len2; int32_t low16; uint16_t cls; uint8_t rpl, g; };
    std::vector<Pre> pre(n);
    for (u32 q = 0; q < n; ++q) {
        const Lens l = pair_lens(ref_off, alt_off, lo + q);
        Pre& J = pre[q];
        J.len1 = (u32)l.l1; J.len2 = (u32)l.l2; J.low16 = 0;
        Shape sh{64, kStripRpl};
        if (J.len1 > (u32)kMaxRef) {
            // the strip class (the context has MGX_SW_LONG_REF): 64 lanes and 32-bit scores whatever MGX_SW_PAIRED and the 16-bit rule say.
            // It is launched LAST (the highest class key).  Launches of one stream run one after the other, so the place decides nothing about
            // the time; last leaves the jobs of the other classes where a context without the flag puts them, arena offsets included.
            J.cls = 255;
            L.n_pairs_strip++; L.n_strips += n_strips_of(J.len1);
        } else if (use16 && rule.admits(J.len1, J.len2, &J.low16)) {
            sh = shape16_for((int)J.len1, paired);
            J.cls = (uint16_t)((sh.g == 64 ? 64 : 0) + (32 - sh.rpl));                                  // < 128
            L.n_pairs_i16++;
        } else {
            sh = shape_for((int)J.len1, paired);
            J.cls = (uint16_t)(128 + (sh.g == 64 ? 64 : 0) + sh.rpl);                                   // < 256
        }
        J.rpl = (uint8_t)sh.rpl; J.g = (uint8_t)sh.g;
    }
    std::vector<u32> order(n), tmp(n), cnt(32770, 0);
    for (u32 q = 0; q < n; ++q) cnt[32767 - pre[q].len2 + 1]++;
    for (u32 k = 0; k < 32768; ++k) cnt[k + 1] += cnt[k];
    for (u32 q = 0; q < n; ++q) tmp[cnt[32767 - pre[q].len2]++] = q;
    u32 c2[257] = {0};
    for (u32 q = 0; q < n; ++q) c2[pre[q].cls + 1]++;
    for (int k = 0; k < 256; ++k) c2[k + 1] += c2[k];
    for (u32 x = 0; x < n; ++x) order[c2[pre[tmp[x]].cls]++] = tmp[x];
    auto make_job = [&](u32 q) {
        const Pre& R = pre[q];
        SwJob J{};
        J.off1 = ref_off[lo + q] - ref_off[lo]; J.off2 = alt_off[lo + q] - alt_off[lo];
        J.len1 = R.len1; J.len2 = R.len2; J.rpl = R.rpl; J.strategy = strategy[lo + q]; J.out_index = q; J.low16 = R.low16;
        J.sc_off = J.off1 + J.off2 + 2ull * q; J.el_off = 2 * J.sc_off;
        J.g = (u32)R.g | (R.cls < 128 ? kJobI16 : 0u) | (R.cls == 255 ? kJobStrip : 0u);
        return J;
    };
    u64 bt = 0;                          // (locals, not L's members: the stores to jobs[] may alias those)
    u32 n_jobs = 0;
    auto take = [&bt](u64 bytes) { const u64 at = bt; bt += bytes; return at; };     // the next region of the arena
    for (u32 x = 0; x < n;) {
        const Pre& R0 = pre[order[x]];
        const Shape sh{(int)R0.g, (int)R0.rpl};
        if (R0.cls >= 128) {             // a pair of its own: 32-bit scores, one strip or several
            SwJob J = make_job(order[x++]);
            J.bt_off = take((J.g & kJobStrip) ? bt_bytes_strip(J.len1, J.len2) : bt_bytes(J.len1, J.len2, sh));
            if (J.g & kJobStrip) J.lr_off = take(bnd_bytes_strip(J.len2));
            jobs[n_jobs++] = J;
            continue;
        }
        // one 16-bit class: lane groups of two pairs, whole wavefronts
        u32 y = x;
        while (y < n && pre[order[y]].cls == R0.cls) ++y;
        for (; x < y; x += 2) {
            SwJob A = make_job(order[x]), B{};
            if (x + 1 < y) B = make_job(order[x + 1]);
            else { B.out_index = kNoOutput; B.rpl = A.rpl; B.g = A.g; }
            B.g |= kJobHalf;
            const u64 n_swp = std::max(A.len2, B.len2), n_lanes = std::max(lanes_of(A.len1, sh), lanes_of(B.len1, sh));
            A.bt_off = B.bt_off = take(bt_bytes16(n_swp + n_lanes - 1, sh));
            // the halves share the last-row region when the same lane owns both last rows, the last-column region when both leave
            // the sweep at the same position; a filler (len1 == 0) shares both
            A.lr_off = B.lr_off = take(lr_bytes16(n_swp, sh));
            if (B.len1 > 0 && (A.len1 - 1) / sh.rpl != (B.len1 - 1) / sh.rpl) B.lr_off = take(lr_bytes16(n_swp, sh));
            A.lc_off = B.lc_off = take(lc_bytes16(n_lanes, sh));
            if (B.len1 > 0 && B.len2 != A.len2) B.lc_off = take(lc_bytes16(n_lanes, sh));
            jobs[n_jobs++] = A; jobs[n_jobs++] = B;
        }
        x = y;
        while (n_jobs % (2 * (64 / sh.g))) {           // filler groups up to the wavefront boundary
            SwJob F{}; F.out_index = kNoOutput; F.rpl = (u32)sh.rpl; F.g = (u32)sh.g | kJobI16 | (n_jobs % 2 ? kJobHalf : 0u);
            jobs[n_jobs++] = F;
        }
    }
    L.n_jobs = n_jobs; L.bt_bytes = bt;
    return L;
}
// ---- launches.  The fill launch that starts at job a: its end and the longest alternate in it (the LDS stage).  The 16-bit kernels take
// every class of one lane-group width in one launch (two when classes of more than 16 rows per lane are present: k_sw_fill16's BIG); a
// 32-bit launch is one class, i.e. equal rpl and an equal g word (flags included: the strip class is a launch of its own).
struct Launch { u32 end, max_len2; };
inline Launch next_launch(const SwJob* jobs, u32 n_jobs, u32 a) {
    const SwJob& A = jobs[a];
    auto same = [&A](const SwJob& B) {
        return (A.g & kJobI16) ? (B.g & kJobI16) && (B.g & 0xFFu) == (A.g & 0xFFu) && (B.rpl > 16) == (A.rpl > 16) : B.rpl == A.rpl && B.g == A.g;
    };
    Launch l{a, 0};
    for (; l.end < n_jobs && same(jobs[l.end]); ++l.end) l.max_len2 = std::max(l.max_len2, jobs[l.end].len2);
    return l;
}

}  // namespace mgx_sw_layout
