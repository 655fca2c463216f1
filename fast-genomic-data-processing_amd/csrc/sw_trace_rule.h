// sw_trace_rule.h -- what the Smith-Waterman fills write and what the back-trace makes of it (mgx_smithwaterman.hip), each rule once:
//   * the back-trace alphabet: the byte of the 32-bit fills, the nibble of the 16-bit fill, the map from nibble to byte
//   * addresses: the slot of (step, lane) that every fill stores through and BtView::cell inverts; a row's nibble inside a lane's words;
//     the packed last-row / last-column element of the 16-bit form; the three views the trace reads a pair through
//   * the 32-bit cell (PairWiseSW.h:31-66) and the matrix boundary (PairWiseSW.h:243-253)
//   * the best end cell among equal scores (PairWiseSW.h:256-285), as a fold over candidates in anti-diagonal order
//   * the walk (PairWiseSW.h:299-408): start cell, leading clip, state machine, merge, trailing overhang and offset per strategy
//   * the CIGAR text and its capacity (PairWiseSW.h:410-444, IntelSmithWaterman.cpp:8)
// No HIP, no heap, no environment: k_sw_trace_wave runs the fold and the walk wave-uniform with a provider that fetches 64 cells of a
// diagonal at a time; tests/cpp/sw_trace_driver.cpp fills a matrix with sw_cell, stores it through these addresses in every form and runs
// the same fold and walk serially and with 64 emulated lanes (tests/test_sw_trace_host.py, CPU, ASan + UBSan).
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/mgx_smithwaterman.h"      // MGX_SW_SOFTCLIP .. MGX_SW_IGNORE
#include "sw_layout.h"

#if defined(__HIPCC__)
#define MGX_SWT_FN __host__ __device__ inline
#else
#define MGX_SWT_FN inline
#endif

#pragma GCC visibility push(hidden)      // inline functions shared by two files of the library: none of them is part of its ABI
namespace mgx_sw_trace {
using namespace mgx_sw_layout;      // SwJob and its flags, bt_slot, bt_slot16, kStripRows, strip_bt_stride

// ---- the alphabet.  Back-trace byte of the 32-bit fills: bits 0-1 the operator H took, bit 2 / bit 3: E / F took the extension
constexpr int kOpMatch = 0, kOpInsert = 1, kOpDelete = 2, kInsertExt = 4, kDeleteExt = 8;
// Nibble of the 16-bit fill: the sign bits of its four packed differences
constexpr int kNibFWins = 1;        // F > max(diagonal, E): H took F
constexpr int kNibEWins = 2;        // E > diagonal: H took E unless F wins
constexpr int kNibFOpened = 4;      // F opened: no DELETE_EXT
constexpr int kNibEOpened = 8;      // E opened: no INSERT_EXT
MGX_SWT_FN int nibble_to_byte(int nib) {
    return ((nib & kNibFWins) ? kOpDelete : (nib & kNibEWins) ? kOpInsert : kOpMatch) | ((nib & kNibEOpened) ? 0 : kInsertExt) |
           ((nib & kNibFOpened) ? 0 : kDeleteExt);
}
constexpr int kMinCutoff = -100000000;           // MATRIX_MIN_CUTOFF, smithwaterman_common.h:73
constexpr int kLowInit = INT32_MIN / 2;          // LOW_INIT_VALUE, smithwaterman_common.h:74

// ---- addresses.  A lane group of g lanes stores, in step t = 1 .. steps, one slot of `slot` bytes per lane (bt_slot / bt_slot16 of its
// rows per lane): lane l is at column t - l.  Bytes from the start of the pair's region (of its strip: strips lie strip_bt_stride apart).
MGX_SWT_FN constexpr size_t bt_slot_at(int t, int lane, int g, int slot) { return ((size_t)t * g + lane) * slot; }
// Inside a slot.  32-bit form: row k of the lane is byte k.  16-bit form: a word per four rows, the low half the first pair's, the high
// half the second's; row k is nibble (k & 3) of its half, from the low bits up
MGX_SWT_FN constexpr int nib16_byte(int k, int half) { return (k >> 2) * 4 + half * 2 + ((k & 3) >> 1); }
MGX_SWT_FN constexpr int nib16_shift(int k) { return (k & 1) * 4; }
// The edges of the 16-bit form, as words of two packed H values (the half picks the pair): the lane that owns a pair's last row stores its
// rpl values per column j, every lane its rpl values at the pair's last column, so row i is word i - 1
MGX_SWT_FN constexpr size_t lr16_at(int j, int rpl, int k) { return (size_t)j * rpl + k; }
MGX_SWT_FN constexpr size_t lc16_at(int i) { return (size_t)i - 1; }
MGX_SWT_FN int half16(u32 word, int half) { return (int)(int16_t)(word >> (half ? 16 : 0)); }

// what the trace reads of a pair's back-trace, whichever kernel filled it: the byte of the 32-bit form
struct BtView {
    const u8* p; int rpl, g, slot; bool i16; int half;
    u64 strip_stride;          // bytes from one strip to the next; 0: the pair is one strip (every class but k_sw_fill_strip's)
    MGX_SWT_FN BtView(const SwJob& J, const u8* bt) : p(bt + J.bt_off), rpl((int)J.rpl), g((int)(J.g & 0xFFu)),
                                                      i16((J.g & kJobI16) != 0), half((J.g & kJobHalf) ? 1 : 0),
                                                      strip_stride((J.g & kJobStrip) ? strip_bt_stride(J.len2) : 0) {
        slot = i16 ? bt_slot16(rpl) : bt_slot(rpl);
    }
    MGX_SWT_FN int cell(int i, int j) const {
        int r = i - 1;
        size_t at = 0;
        if (strip_stride) { const int s = r / kStripRows; r -= s * kStripRows; at = (size_t)s * strip_stride; }
        const int l = r / rpl, k = r - l * rpl;                      // the lane that owns row i and its row in the lane
        const size_t base = at + bt_slot_at(j + l, l, g, slot);
        if (!i16) return p[base + k];
        return nibble_to_byte((p[base + nib16_byte(k, half)] >> nib16_shift(k)) & 15);
    }
};
// H(nrow, j), j = 1 .. ncol
struct LastRow {
    const int32_t* p32; const u32* p16; int rpl, k_last, half;
    MGX_SWT_FN LastRow(const SwJob& J, const u8* bt, const int32_t* sc) : p32(sc + J.sc_off), p16(reinterpret_cast<const u32*>(bt + J.lr_off)),
                                                                           rpl((int)J.rpl), k_last(((int)J.len1 - 1) % (int)J.rpl), half((J.g & kJobHalf) ? 1 : 0) {
        if (!(J.g & kJobI16)) p16 = nullptr;
    }
    MGX_SWT_FN int operator[](int j) const { return p16 ? half16(p16[lr16_at(j, rpl, k_last)], half) : p32[j]; }
};
// H(i, ncol), i = 1 .. nrow
struct LastCol {
    const int32_t* p32; const u32* p16; int half;
    MGX_SWT_FN LastCol(const SwJob& J, const u8* bt, const int32_t* sc) : p32(sc + J.sc_off + J.len2 + 1), p16(reinterpret_cast<const u32*>(bt + J.lc_off)),
                                                                           half((J.g & kJobHalf) ? 1 : 0) {
        if (!(J.g & kJobI16)) p16 = nullptr;
    }
    MGX_SWT_FN int operator[](int i) const { return p16 ? half16(p16[lc16_at(i)], half) : p32[i]; }
};

// ---- the 32-bit cell
struct SwParams { int match, mismatch, open, extend; };
MGX_SWT_FN int imax(int a, int b) { return a > b ? a : b; }
// H(x, 0) = H(0, x), x >= 1: the matrix boundary per overhang strategy (PairWiseSW.h:243-253)
MGX_SWT_FN int sw_edge(bool indel, const SwParams& P, int x) { return indel ? P.open + (x - 1) * P.extend : 0; }
// One 32-bit cell (PairWiseSW.h:31-66), row k of a lane: hl / gs are the row's H and its gap state along the sweep, diag / up_h / up_g
// come from the row above and leave as this row's for the row below; the back-trace byte goes into the lane's packed word.
MGX_SWT_FN void sw_cell(const SwParams& P, int sa, int c2, int k, int& hl, int& gs, int& diag, int& up_h, int& up_g, u32& packed) {
    const int open_s = hl + P.open, ext_s = gs + P.extend;               // along the sweep
    const int ee = imax(open_s, ext_s);
    const int open_c = up_h + P.open, ext_c = up_g + P.extend;           // along the lanes' own positions
    const int ff = imax(ext_c, open_c);
    // E is the horizontal gap (INSERT), F the vertical one (DELETE); ties prefer the extension
    int ext = 0;
    if (!(open_s > ext_s)) ext |= kInsertExt;
    if (!(open_c > ext_c)) ext |= kDeleteExt;
    int h = imax(diag + (sa == c2 ? P.match : P.mismatch), kMinCutoff);  // H prefers the diagonal, then E, then F
    int op = kOpMatch;
    if (ee > h) { op = kOpInsert; h = ee; }
    if (ff > h) { op = kOpDelete; h = ff; }
    diag = hl; hl = h; gs = ee; up_h = h; up_g = ff;
    packed |= (u32)(op | ext) << ((k & 3) * 8);
}

// ---- the best end cell (PairWiseSW.h:256-285).  The reference meets the cells of the last row and the last column in anti-diagonal
// order, on one anti-diagonal the row's cell (nrow, d - nrow) before the column's (d - ncol, ncol), and keeps a later cell of equal score
// by these rules; fed with the cells that hold the maximum, in that order, the fold ends on the reference's cell.  The last row counts
// for SOFTCLIP and IGNORE only (the caller offers no row candidate otherwise).
struct EndCell {
    int nrow, ncol, mi = 0, mj = 0;
    bool have = false;
    MGX_SWT_FN EndCell(int nrow_, int ncol_) : nrow(nrow_), ncol(ncol_) {}
    MGX_SWT_FN static int dist(int a, int b) { return a > b ? a - b : b - a; }
    MGX_SWT_FN void row(int j) { if (!have || dist(nrow, j) < dist(mi, mj)) { mi = nrow; mj = j; have = true; } }
    MGX_SWT_FN void col(int i) { if (!have || mj == ncol || dist(i, ncol) <= dist(mi, mj)) { mi = i; mj = ncol; have = true; } }
    // the candidates of anti-diagonals d0 .. d0 + 63: bit t of `rows` / `cols`: the row's / the column's cell of anti-diagonal d0 + t
    MGX_SWT_FN void replay(int d0, u64 rows, u64 cols) {
        for (u64 any = rows | cols; any; any &= any - 1) {
            const int t = __builtin_ctzll(any);
            if ((rows >> t) & 1) row(d0 + t - nrow);
            if ((cols >> t) & 1) col(d0 + t - ncol);
        }
    }
};

// ---- the walk (PairWiseSW.h:299-408), elements in run-length form: what the reference's final merge pass makes of its one-per-cell list.
//   cell(i, j)        the back-trace byte, asked one cell at a time inside a gap
//   diag.run(i, j)    in the match state: how many cells (i, j), (i - 1, j - 1), ... may be consumed as matches at once; 0: none, and then
//   diag.byte(i, j)   the byte of that same cell
//   store(k, op, len) element k of the list, in the order getCIGAR holds it (the text reverses it)
// Nothing here differs between the lanes of a wavefront: what lanes share is inside the provider.
struct Walked { int offset, n_elems; };
template <class Cell, class Diag, class Store>
MGX_SWT_FN Walked walk(int nrow, int ncol, int strategy, int mi, int mj, Cell cell, Diag& diag, Store store) {
    int i, j;
    if (strategy == MGX_SW_INDEL) { i = nrow; j = ncol; }
    else if (strategy == MGX_SW_LEADING_INDEL) { i = mi; j = ncol; }
    else { i = mi; j = mj; }
    int m = 0;                    // elements written so far
    int cur_op = -1, cur_len = 0; // the open element
    auto flush = [&]() {
        if (cur_op >= 0) { store(m, cur_op, cur_len); ++m; }
    };
    auto push = [&](int op, int len) {          // append, merging with the open element
        if (op == cur_op) cur_len += len;
        else { flush(); cur_op = op; cur_len = len; }
    };
    if (j < ncol) push(MGX_SW_SOFTCLIP, ncol - j);
    int state = 0;
    while (i > 0 && j > 0) {
        int btr;
        if (state == 0) {
            const int run = diag.run(i, j);
            if (run > 0) { i -= run; j -= run; push(kOpMatch, run); continue; }
            btr = diag.byte(i, j);
        } else {
            btr = cell(i, j);
        }
        if (state == kInsertExt) { --j; cur_len++; state = btr & kInsertExt; }
        else if (state == kDeleteExt) { --i; cur_len++; state = btr & kDeleteExt; }
        else {
            const int op = btr & 3;
            if (op == kOpMatch) { --i; --j; push(kOpMatch, 1); state = 0; }
            else if (op == kOpInsert) { --j; push(kOpInsert, 1); state = btr & kInsertExt; }
            else { --i; push(kOpDelete, 1); state = btr & kDeleteExt; }
        }
    }
    int offset;
    if (strategy == MGX_SW_SOFTCLIP) {
        if (j > 0) push(MGX_SW_SOFTCLIP, j);
        offset = i;
    } else if (strategy == MGX_SW_IGNORE) {
        if (j > 0) push(cur_op, j);             // "the last element once more, j long"
        offset = (int16_t)(i - j);
    } else {
        if (i > 0) push(kOpDelete, i);
        else if (j > 0) push(kOpInsert, j);
        offset = 0;
    }
    flush();
    return Walked{offset, m};
}

// The diagonal a wavefront caches: lane t holds cell (c_i - t, c_j - t), 0 (which reads as a match) beyond the matrix.  (i, j) is served
// from the cache when it lies on that diagonal at t = 0 .. 63; a provider refetches otherwise.  The run from position t is the number of
// matches from bit t of the lanes' ballot upwards, bounded by the matrix: the walk ends at i = 0 or j = 0.
constexpr int kDiagLanes = 64;
MGX_SWT_FN bool diag_cached(bool valid, int c_i, int c_j, int i, int j) { const int t = c_i - i; return valid && t >= 0 && t < kDiagLanes && c_j - j == t; }
MGX_SWT_FN int diag_run(u64 match_ballot, int t, int i, int j) {
    const u64 rest = ~(match_ballot >> t);
    const int run = rest ? (int)__builtin_ctzll(rest) : kDiagLanes;
    const int room = i < j ? i : j;
    return run < room ? run : room;
}

// host providers.  One cell at a time, no run consumed: the reference's own walk
template <class Cell>
struct SerialDiag {
    Cell cell;
    int run(int, int) { return 0; }
    int byte(int i, int j) { return cell(i, j); }
};
// the wavefront's provider with its 64 lanes and its ballot in loops; counts what the tests' seams are about
template <class Cell>
struct LanesDiag {
    Cell cell;
    int cached[kDiagLanes] = {}, c_i = 0, c_j = 0, t = 0;
    bool valid = false;
    int refetches = 0, longest_run = 0;
    int run(int i, int j) {
        if (!diag_cached(valid, c_i, c_j, i, j)) {
            c_i = i; c_j = j; valid = true; ++refetches;
            for (int lane = 0; lane < kDiagLanes; ++lane) cached[lane] = (i - lane >= 1 && j - lane >= 1) ? cell(i - lane, j - lane) : 0;
        }
        t = c_i - i;
        u64 ballot = 0;
        for (int lane = 0; lane < kDiagLanes; ++lane) if ((cached[lane] & 3) == kOpMatch) ballot |= 1ull << lane;
        const int n = diag_run(ballot, t, i, j);
        if (n > longest_run) longest_run = n;
        return n;
    }
    int byte(int, int) { return cached[t]; }
};

// ---- text (PairWiseSW.h:410-444).  What the reference's caller gives the text: 2 * max(lengths) bytes (IntelSmithWaterman.cpp:8), and
// here never more than the caller's row of `stride` bytes holds beside its NUL; kNoStride: there is no row
constexpr u64 kNoStride = 0;
inline int text_cap(u64 l1, u64 l2, u64 stride) {
    const u64 cap = 2 * (l1 > l2 ? l1 : l2);
    return (int)(stride != kNoStride && stride - 1 < cap ? stride - 1 : cap);
}
inline int itoa_len(int v) { const int neg = v < 0; if (neg) v = -v; int d = 0; while (v > 0) { v /= 10; ++d; } return d + neg; }
// last element first; an element whose text does not fit is skipped
// bam != nullptr: the elements that went into the text also as length << 4 | BAM operator (9 where the text says R), *n_bam of them;
// out == nullptr: no text, the elements alone
inline int render(const int16_t* el, int n_elems, char* out, int cap, u32* bam = nullptr, u32* n_bam = nullptr) {
    int cur = 0;
    for (int k = n_elems - 1; k >= 0; --k) {
        const int op = el[2 * k], len = el[2 * k + 1];
        const char c = op == kOpMatch ? 'M' : op == kOpInsert ? 'I' : op == kOpDelete ? 'D' : op == MGX_SW_SOFTCLIP ? 'S' : 'R';
        const int need = itoa_len(len) + 1;
        if (need > 1 && cur + need <= cap) {
            if (bam && len > 0) bam[(*n_bam)++] = (u32)len << 4 | (c == 'M' ? 0u : c == 'I' ? 1u : c == 'D' ? 2u : c == 'S' ? 4u : 9u);
            if (!out) { cur += need; continue; }
            int v = len;
            if (v < 0) { out[cur++] = '-'; v = -v; }
            const int d = itoa_len(v);
            for (int q = d - 1; q >= 0; --q) { out[cur + q] = (char)('0' + v % 10); v /= 10; }
            cur += d;
            out[cur++] = c;
        }
    }
    return cur;
}

}  // namespace mgx_sw_trace
#pragma GCC visibility pop
