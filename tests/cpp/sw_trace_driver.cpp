// sw_trace_driver.cpp -- csrc/sw_trace_rule.h on the CPU, for tests/test_sw_trace_host.py (built with -Wall -Wextra -Werror under ASan + UBSan).
//   sw_trace_driver FILE
// FILE: one pair per line, "match mismatch open extend strategy caps REF ALT"; caps: text capacities beside the default one, "3,6", or "-".
// Per pair the matrix is filled row by row with sw_cell and written, through the header's addresses, into every stored form the pair admits:
//   b32g64 b32g32     the 32-bit form at shape_for's class, one pair per wavefront / two (references up to kMaxRef bases)
//   strip             the strip form (longer references)
//   i16g64lo i16g64hi i16g32lo i16g32hi     the 16-bit form at shape16_for's class, as the low and as the high half (pairs I16Rule admits)
// in buffers of exactly sw_layout.h's sizes, poisoned with 0xFF first.  Per form the rule runs three ways -- `serial`: candidates offered cell by
// cell, one cell per step; `lanes`: the same end cell, the walk over 64 emulated lanes; `replay`: the end cell from 64-candidate masks, then
// the lanes' walk -- and prints
//   res PAIR FORM WAY score mi mj offset n_elems TEXT TEXT_AT_CAP,...        ("-" for an empty text or no caps)
//   cnt PAIR FORM refetches longest_run candidates                            (of the lanes' walk and the replay)
//   skip PAIR FORM                                                            (the pair does not admit the form)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "sw_trace_rule.h"

using namespace mgx_sw_trace;

namespace {

struct Matrix {                    // what a fill computes of one pair, in plain order
    int nrow, ncol;
    std::vector<u8> byte, nib;     // [(i - 1) * ncol + (j - 1)]
    std::vector<int32_t> last_row, last_col;      // [j], [i], entry 0 unused
    u8 at(const std::vector<u8>& v, int i, int j) const { return v[(size_t)(i - 1) * ncol + (j - 1)]; }
};

Matrix fill(const SwParams& P, int strategy, const std::string& ref, const std::string& alt) {
    Matrix M{(int)ref.size(), (int)alt.size(), {}, {}, {}, {}};
    const bool indel = strategy == MGX_SW_INDEL || strategy == MGX_SW_LEADING_INDEL;
    M.byte.resize((size_t)M.nrow * M.ncol); M.nib.resize(M.byte.size());
    M.last_row.assign(M.ncol + 1, 0); M.last_col.assign(M.nrow + 1, 0);
    std::vector<int> h_above(M.ncol + 1), f_above(M.ncol + 1, kLowInit), h_row(M.ncol + 1), f_row(M.ncol + 1);
    for (int j = 1; j <= M.ncol; ++j) h_above[j] = sw_edge(indel, P, j);
    h_above[0] = 0;
    for (int i = 1; i <= M.nrow; ++i) {
        int hl = sw_edge(indel, P, i), gs = kLowInit;
        h_row[0] = hl;
        for (int j = 1; j <= M.ncol; ++j) {
            int diag = h_above[j - 1], up_h = h_above[j], up_g = f_above[j];
            const int h0 = imax(diag + (ref[i - 1] == alt[j - 1] ? P.match : P.mismatch), kMinCutoff);
            u32 packed = 0;
            sw_cell(P, (u8)ref[i - 1], (u8)alt[j - 1], 0, hl, gs, diag, up_h, up_g, packed);
            h_row[j] = hl; f_row[j] = up_g;
            const int b = (int)(packed & 0xFF);
            // the 16-bit fill's four sign bits, from the same decisions
            const int nib = ((b & 3) == kOpDelete ? kNibFWins : 0) | (gs > h0 ? kNibEWins : 0) | ((b & kDeleteExt) ? 0 : kNibFOpened) |
                            ((b & kInsertExt) ? 0 : kNibEOpened);
            M.byte[(size_t)(i - 1) * M.ncol + (j - 1)] = (u8)b;
            M.nib[(size_t)(i - 1) * M.ncol + (j - 1)] = (u8)nib;
            if (i == M.nrow) M.last_row[j] = hl;
        }
        M.last_col[i] = hl;
        h_above.swap(h_row); f_above.swap(f_row);
    }
    return M;
}

struct Stored { SwJob J{}; std::unique_ptr<u8[]> bt; std::unique_ptr<int32_t[]> sc; };

// the 32-bit forms: slot bt_slot_at(j + lane, lane), byte k; strips lie strip_bt_stride apart
Stored store32(const Matrix& M, Shape sh, bool strip) {
    Stored S;
    SwJob& J = S.J;
    J.len1 = (u32)M.nrow; J.len2 = (u32)M.ncol; J.rpl = (u32)sh.rpl; J.g = (u32)sh.g | (strip ? kJobStrip : 0u);
    const u64 bytes = strip ? bt_bytes_strip(J.len1, J.len2) : bt_bytes(J.len1, J.len2, sh);
    S.bt.reset(new u8[bytes]);
    memset(S.bt.get(), 0xFF, bytes);
    S.sc.reset(new int32_t[(size_t)M.nrow + M.ncol + 2]);
    for (int j = 0; j <= M.ncol; ++j) S.sc[j] = j ? M.last_row[j] : INT32_MIN;
    for (int i = 0; i <= M.nrow; ++i) S.sc[M.ncol + 1 + i] = i ? M.last_col[i] : INT32_MIN;
    for (int i = 1; i <= M.nrow; ++i) {
        int r = i - 1;
        u64 at = 0;
        if (strip) { at = (u64)(r / kStripRows) * strip_bt_stride(J.len2); r %= kStripRows; }
        const int lane = r / sh.rpl, k = r % sh.rpl;
        for (int j = 1; j <= M.ncol; ++j) S.bt[at + bt_slot_at(j + lane, lane, sh.g, bt_slot(sh.rpl)) + k] = M.at(M.byte, i, j);
    }
    return S;
}

// the 16-bit form of a lane group that holds this pair alone, in either half: nibbles, then the last lane's rows, then every lane's last column
Stored store16(const Matrix& M, Shape sh, int half, int32_t low16) {
    Stored S;
    SwJob& J = S.J;
    J.len1 = (u32)M.nrow; J.len2 = (u32)M.ncol; J.rpl = (u32)sh.rpl; J.g = (u32)sh.g | kJobI16 | (half ? kJobHalf : 0u); J.low16 = low16;
    const u64 n_lanes = lanes_of(J.len1, sh), a = bt_bytes16(J.len2 + n_lanes - 1, sh), b = lr_bytes16(J.len2, sh), c = lc_bytes16(n_lanes, sh);
    J.lr_off = a; J.lc_off = a + b;
    S.bt.reset(new u8[a + b + c]);
    memset(S.bt.get(), 0xFF, a + b + c);
    auto put_half = [&](u64 off, size_t word, int v) {              // one half of a packed word, the other half stays poison
        const uint16_t h = (uint16_t)(int16_t)v;
        memcpy(S.bt.get() + off + 4 * word + 2 * half, &h, 2);
    };
    const int k_last = (M.nrow - 1) % sh.rpl;
    for (int j = 1; j <= M.ncol; ++j) put_half(J.lr_off, lr16_at(j, sh.rpl, k_last), M.last_row[j]);
    for (int i = 1; i <= M.nrow; ++i) {
        put_half(J.lc_off, lc16_at(i), M.last_col[i]);
        const int lane = (i - 1) / sh.rpl, k = (i - 1) % sh.rpl;
        for (int j = 1; j <= M.ncol; ++j) {
            u8& byte = S.bt[bt_slot_at(j + lane, lane, sh.g, bt_slot16(sh.rpl)) + nib16_byte(k, half)];
            byte = (u8)((byte & ~(15 << nib16_shift(k))) | (M.at(M.nib, i, j) << nib16_shift(k)));
        }
    }
    return S;
}

std::string text_of(const int16_t* el, int n, int cap) {
    std::unique_ptr<char[]> buf(new char[cap > 0 ? cap : 1]);       // cap bytes and not one more
    const int len = render(el, n, buf.get(), cap);
    return len ? std::string(buf.get(), (size_t)len) : "-";
}

void run_form(size_t pair, const char* form, const Stored& S, int strategy, const std::vector<int>& caps) {
    const SwJob& J = S.J;
    const int nrow = (int)J.len1, ncol = (int)J.len2;
    const LastRow last_row(J, S.bt.get(), S.sc.get());
    const LastCol last_col(J, S.bt.get(), S.sc.get());
    const BtView view(J, S.bt.get());
    const bool use_row = strategy == MGX_SW_SOFTCLIP || strategy == MGX_SW_IGNORE;
    int best = INT32_MIN;
    if (use_row) for (int j = 1; j <= ncol; ++j) best = imax(best, last_row[j]);
    for (int i = 1; i <= nrow; ++i) best = imax(best, last_col[i]);
    auto is_row = [&](int d) { const int j = d - nrow; return use_row && j >= 1 && j <= ncol && last_row[j] == best; };
    auto is_col = [&](int d) { const int i = d - ncol; return i >= 1 && i <= nrow && last_col[i] == best; };
    EndCell one(nrow, ncol), blocks(nrow, ncol);
    for (int d = 1; d <= nrow + ncol; ++d) {
        if (is_row(d)) one.row(d - nrow);
        if (is_col(d)) one.col(d - ncol);
    }
    int candidates = 0;
    for (int d0 = 1; d0 <= nrow + ncol; d0 += 64) {
        u64 rows = 0, cols = 0;
        for (int t = 0; t < 64 && d0 + t <= nrow + ncol; ++t) { rows |= (u64)is_row(d0 + t) << t; cols |= (u64)is_col(d0 + t) << t; }
        candidates += __builtin_popcountll(rows) + __builtin_popcountll(cols);
        blocks.replay(d0, rows, cols);
    }
    auto cell = [&](int i, int j) { return view.cell(i, j); };
    const size_t el_n = 2 * ((size_t)nrow + ncol + 2);            // the pair's share of the element arena
    auto report = [&](const char* way, const EndCell& end, auto& diag) {
        std::unique_ptr<int16_t[]> el(new int16_t[el_n]);
        const Walked w = walk(nrow, ncol, strategy, end.mi, end.mj, cell, diag,
                              [&](int k, int op, int len) { el[2 * (size_t)k] = (int16_t)op; el[2 * (size_t)k + 1] = (int16_t)len; });
        printf("res %zu %s %s %d %d %d %d %d %s ", pair, form, way, best, end.mi, end.mj, w.offset, w.n_elems,
               text_of(el.get(), w.n_elems, text_cap(J.len1, J.len2, kNoStride)).c_str());
        for (size_t c = 0; c < caps.size(); ++c) printf("%s%s", c ? "," : "", text_of(el.get(), w.n_elems, caps[c]).c_str());
        printf("%s\n", caps.empty() ? "-" : "");
    };
    SerialDiag<decltype(cell)> serial{cell};
    LanesDiag<decltype(cell)> lanes{cell}, lanes2{cell};
    report("serial", one, serial);
    report("lanes", one, lanes);
    report("replay", blocks, lanes2);
    printf("cnt %zu %s %d %d %d\n", pair, form, lanes.refetches, lanes.longest_run, candidates);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: sw_trace_driver FILE\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    for (size_t pair = 0; std::getline(f, line); ++pair) {
        std::istringstream in(line);
        SwParams P;
        int strategy;
        std::string caps_s, ref, alt;
        if (!(in >> P.match >> P.mismatch >> P.open >> P.extend >> strategy >> caps_s >> ref >> alt) || strategy < MGX_SW_SOFTCLIP ||
            strategy > MGX_SW_IGNORE || ref.size() > (size_t)kMaxLen || alt.size() > (size_t)kMaxLen) {
            fprintf(stderr, "bad input in line %zu\n", pair + 1);
            return 2;
        }
        std::vector<int> caps;
        if (caps_s != "-") { std::istringstream cs(caps_s); for (std::string c; std::getline(cs, c, ',');) caps.push_back(atoi(c.c_str())); }
        const Matrix M = fill(P, strategy, ref, alt);
        const bool is_long = M.nrow > kMaxRef;
        if (is_long) { run_form(pair, "strip", store32(M, Shape{64, kStripRpl}, true), strategy, caps); printf("skip %zu b32g64\nskip %zu b32g32\n", pair, pair); }
        else {
            printf("skip %zu strip\n", pair);
            run_form(pair, "b32g64", store32(M, shape_for(M.nrow, false), false), strategy, caps);
            run_form(pair, "b32g32", store32(M, shape_for(M.nrow, true), false), strategy, caps);
        }
        int32_t low16 = 0;
        const bool ok16 = !is_long && mgx_sw16::I16Rule(P.match, P.mismatch, P.open, P.extend).admits(M.nrow, M.ncol, &low16);
        for (int paired = 0; paired < 2; ++paired)
            for (int half = 0; half < 2; ++half) {
                char form[16];
                snprintf(form, sizeof form, "i16g%s%s", paired ? "32" : "64", half ? "hi" : "lo");
                if (ok16) run_form(pair, form, store16(M, shape16_for(M.nrow, paired != 0), half, low16), strategy, caps);
                else printf("skip %zu %s\n", pair, form);
            }
    }
    return 0;
}
