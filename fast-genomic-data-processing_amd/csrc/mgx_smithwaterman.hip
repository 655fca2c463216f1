// mgx_smithwaterman.hip -- Smith-Waterman with back-trace on gfx950 (C ABI: include/mgx_smithwaterman.h).
//
// What the reference does per pair with AVX anti-diagonals (intel/smithwaterman/PairWiseSW.h) is done
// here with one wavefront per pair and the machinery of the PairHMM kernel: lane l owns RPL
// consecutive rows of the matrix and walks the columns, one anti-diagonal of lanes per step; the
// bottom row of a lane (H and F of the current column) reaches the next lane through a lane shift.
// Integer DP, so results are the reference's exactly:
//   * cell recurrence and tie rules: PairWiseSW.h:31-66 (E/F prefer extension on ties; H prefers the
//     diagonal, then E, then F; back-trace byte = op | INSERT_EXT | DELETE_EXT)
//   * boundaries per overhang strategy: PairWiseSW.h:243-253
//   * best end cell among equal scores, replayed in anti-diagonal order: PairWiseSW.h:256-285
//   * back-trace state machine, leading / trailing overhang, merge: PairWiseSW.h:299-408
//   * CIGAR text and its capacity rule (host, next to the caller's buffer): PairWiseSW.h:410-444
// The cell, the end-cell ties, the walk and the text are stated once, in sw_trace_rule.h, which also runs on the CPU
// (tests/cpp/sw_trace_driver.cpp); this file keeps the sweeps, the launches and the host stages.
//
// Back-trace bytes are laid out by (step, lane, row-in-lane) so that one step of a wavefront stores
// 64 * RPL consecutive bytes (bt_slot_at); the trace converts (i, j) back to that index (BtView, sw_trace_rule.h).
//
// Three fill kernels:
//   k_sw_fill16   packed 16-bit scores, two pairs per lane group, the four decisions of a cell taken from the sign bits of four
//                 packed differences, back-trace nibbles, all row classes in one launch -- for every pair whose scores provably fit
//                 16 bits (I16Rule; the realignment workload of Mutect2 always does): 12.6 instructions per cell
//   k_sw_fill     32-bit scores, one pair per lane group, compare + select per decision, back-trace bytes, one launch per row class
//                 -- everything else (long references with long alternates, large scoring parameters)
//   k_sw_fill_strip  the 32-bit cell with a strip loop around the sweep, for references of 2049 .. 32 767 bases (MGX_SW_LONG_REF)
// All write what the trace kernel reads through BtView / LastRow / LastCol (sw_trace_rule.h: the addresses they store through and the
// views that invert them); a batch may mix them pair by pair.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <cstdio>
#include <memory>
#include <new>
#include <thread>
#include <vector>

#include "../../include/mgx_smithwaterman.h"
#include "mgx_hip_util.h"      // HIP_TRY
#include "mgx_realign_internal.h"
#include "sw_layout.h"
#include "sw_trace_rule.h"

using mgx::set_error;

namespace {

using namespace mgx_sw_layout;     // SwJob, shapes, region sizes, chunks, build_jobs, next_launch: sw_layout.h (CPU-tested)
using namespace mgx_sw_trace;      // alphabet, addresses, views, sw_edge / sw_cell, end cell, walk, text: sw_trace_rule.h (CPU-tested)

struct SwResult { int32_t score, max_i, max_j, offset, n_elems; };

// ---- what the fill kernels share beside sw_edge and sw_cell (sw_trace_rule.h).
// Two pieces that take a lane's register arrays are macros over the kernel's RPL: a function is optimised on its own before it is inlined,
// with the array as a pointer, and the pick became ONE indexed load, which moved hl to scratch memory (the store merely came out otherwise).
// H of the pair's last row, which is row k_last of the lane that owns it: a select per row, the registers are not indexable
#define MGX_SW_LAST_ROW_H(dst, hl, k_last) \
    do { int v_ = hl[0]; _Pragma("unroll") for (int k_ = 1; k_ < RPL; ++k_) if (k_ == k_last) v_ = hl[k_]; dst = v_; } while (0)
// the back-trace bytes of one lane and step into their slot (bt_slot_at): row k is byte k
#define MGX_SW_STORE_BT(dst_, packed) do { u8* dst = (dst_); \
    if constexpr (RPL == 1) dst[0] = (u8)packed[0]; \
    else if constexpr (RPL == 2) *reinterpret_cast<uint16_t*>(dst) = (uint16_t)packed[0]; \
    else { _Pragma("unroll") for (int q = 0; q < bt_slot(RPL) / 4; ++q) reinterpret_cast<u32*>(dst)[q] = packed[q]; } } while (0)

// G lanes per pair (two pairs share a wavefront when G = 32), RPL rows per lane.  Back-trace byte:
// bits 0-1 op, bit 2 INSERT_EXT, bit 3 DELETE_EXT (PairWiseSW.h:31-66).  (Storing the length of the
// diagonal match run in the spare bits, so that the trace crosses a run in one step, was measured:
// trace 0.58 -> 0.38 ms, fill 1.14 -> 1.42 ms per 20 000 pairs -- not kept.)
template <int G, int RPL>
__global__ __launch_bounds__(64) void k_sw_fill(const SwJob* __restrict__ jobs, u32 n_jobs, const u8* __restrict__ s1, const u8* __restrict__ s2,
                                                u8* __restrict__ bt, int32_t* __restrict__ sc, u32 lds_stride, SwParams P) {
    extern __shared__ u8 sh_all[];                    // the swept sequences: one global load per step would
    constexpr int GPW = 64 / G;                       // put ~200 serial HBM latencies on every wavefront's path
    const int grp = threadIdx.x / G, lane = threadIdx.x % G;
    const u32 job_idx = blockIdx.x * GPW + grp;
    const bool live = job_idx < n_jobs;
    SwJob J{};
    if (live) J = jobs[job_idx];
    const int nrow = (int)J.len1, ncol = (int)J.len2;
    const int n_own = nrow, n_swp = ncol;             // positions spread over the lanes | positions swept
    const bool indel = J.strategy == MGX_SW_INDEL || J.strategy == MGX_SW_LEADING_INDEL;
    const u8* own = s1 + J.off1;
    const u8* swp = s2 + J.off2;
    int32_t* last_row = sc + J.sc_off;               // H(nrow, j), j = 1 .. ncol
    int32_t* last_col = last_row + ncol + 1;         // H(i, ncol), i = 1 .. nrow
    int32_t* const edge_own = last_row;              // written step by step by the lane that owns the last position
    int32_t* const edge_swp = last_col;              // the registers after the last step
    u8* btp = bt + J.bt_off;
    u8* sh_b = sh_all + (size_t)grp * lds_stride;
    for (int x = lane; x < n_swp; x += G) sh_b[x] = swp[x];
    __syncthreads();
    const int r0 = lane * RPL;                       // this lane owns positions r0+1 .. r0+RPL (1-based)
    int sa[RPL], hl[RPL], gs[RPL];                   // gs: the gap state along the sweep (E when the lanes own rows, F when columns)
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
        const int i = r0 + k + 1;
        sa[k] = (live && i <= n_own) ? (int)own[i - 1] : 256;     // padding positions never match and feed nothing beyond them
        hl[k] = sw_edge(indel, P, i);                             // H(i, 0) / H(0, j)
        gs[k] = kLowInit;                                         // E(i, 0) / F(0, j)
    }
    int diag_in = sw_edge(r0 != 0 && indel, P, r0);               // H(r0, 0) / H(0, r0); H(0, 0) = 0
    const int n_lanes = live ? (n_own + RPL - 1) / RPL : 0;
    const int steps = live ? n_swp + n_lanes - 1 : 0;
    int steps_w = steps;                              // the wavefront walks to its longest pair
    if constexpr (GPW > 1) {
        const int other = __shfl_xor(steps, G, 64);
        steps_w = other > steps ? other : steps;
    }
    const int lane_last = live ? (n_own - 1) / RPL : -1, k_last = live ? (n_own - 1) % RPL : 0;
    int send_h = 0, send_g = kLowInit;
    for (int t = 1; t <= steps_w; ++t) {
        // what the lane before computed for this sweep position one step ago: H and the chained gap at its last position
        const int rh = __shfl_up(send_h, 1, G), rg = __shfl_up(send_g, 1, G);
        const int j = t - lane;                       // the sweep position of this lane at this step
        if (j >= 1 && j <= n_swp && lane < n_lanes) {
            int up_h, up_g, diag;
            if (lane == 0) {
                up_h = sw_edge(indel, P, j);                         // H(0, j) / H(i, 0)
                up_g = kLowInit;                                     // F(0, j) / E(i, 0)
                diag = sw_edge(j != 1 && indel, P, j - 1);           // the boundary one position back; H(0, 0) = 0
            } else { up_h = rh; up_g = rg; diag = diag_in; }
            diag_in = up_h;                                          // this step's neighbour value is the next step's diagonal
            const int c2 = (int)sh_b[j - 1];
            u32 packed[(RPL + 3) / 4] = {};
#pragma unroll
            for (int k = 0; k < RPL; ++k) sw_cell(P, sa[k], c2, k, hl[k], gs[k], diag, up_h, up_g, packed[k >> 2]);
            send_h = up_h; send_g = up_g;
            if (lane == lane_last) MGX_SW_LAST_ROW_H(edge_own[j], hl, k_last);
            MGX_SW_STORE_BT(btp + bt_slot_at(t, lane, G, bt_slot(RPL)), packed);
        }
    }
    // a lane's last active step is the last sweep position: its registers now hold H there (kept out of the loop --
    // a guarded store per cell and step doubled the instruction count of the sweep)
    if (lane < n_lanes) {
#pragma unroll
        for (int k = 0; k < RPL; ++k) if (r0 + k + 1 <= n_own) edge_swp[r0 + k + 1] = hl[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// References of more than kMaxRef bases (MGX_SW_LONG_REF): k_sw_fill<64, 32>'s cell body with a strip loop around the sweep, the
// pattern of pairhmm_fwd_strip.  One pair per wavefront; the reference is cut into strips of 64 lanes x 32 rows, the
// LAST strip takes the remainder, and the strips sweep the alternate (staged in LDS once) one after the other.
//   * Hand-off.  Three things cross a seam: H and F (the vertical gap) of the strip's bottom row per column, and the diagonal
//     H(r, j - 1), which is the H handed over one column earlier (diag_in, as between two lanes).  E belongs to a row.  The lane
//     that owns a strip's bottom row (lane 63: every strip but the last is full) stores (H, F) of column j into the pair's
//     boundary array bnd[j]; in the next strip lane 0 takes them where the one-strip kernel takes the matrix boundary.  In the
//     first strip the same registers hold that boundary's closed form, so the sweep does not tell the strips apart.
//   * One array per pair is enough.  Lane 0 is at column j in step j; lane 63 overwrites bnd[j] in step j + 63.  The boundary is
//     not loaded per step (a dependent global load on every step's path) but 64 columns at a time, one per lane, one block of 64
//     steps ahead: the block that starts at step t0 first loads columns t0 + 64 .. t0 + 127, which are overwritten from step
//     t0 + 127 on, and hands column t0 + x to lane 0 in step t0 + x with a v_readlane.  Loads and stores are one wavefront's, in
//     program order, and every value loaded sits in a register before its slot is stored to; a whole strip lies between a store
//     and the load that wants it, with a fence at the seam.  The sweep proper holds no load, so it never waits for its own
//     back-trace stores.  No workgroup waits for another.
//   * Back-trace: strip s is written in the (step, lane, row-in-lane) layout at s * strip_bt_stride(ncol) (BtView adds the term).
//   * H(i, ncol) is stored at the end of every strip, H(nrow, j) by the lane that owns row nrow in the last strip.
__global__ __launch_bounds__(64) void k_sw_fill_strip(const SwJob* __restrict__ jobs, u32 n_jobs, const u8* __restrict__ s1, const u8* __restrict__ s2,
                                                      u8* bt, int32_t* __restrict__ sc, SwParams P) {
    extern __shared__ u8 sh_strip[];
    constexpr int RPL = kStripRpl, SLOT = bt_slot(RPL);
    if (blockIdx.x >= n_jobs) return;
    const int lane = threadIdx.x;
    const SwJob J = jobs[blockIdx.x];
    const int nrow = (int)J.len1, ncol = (int)J.len2;
    const bool indel = J.strategy == MGX_SW_INDEL || J.strategy == MGX_SW_LEADING_INDEL;
    const u8* own = s1 + J.off1;
    const u8* swp = s2 + J.off2;
    int32_t* const last_row = sc + J.sc_off;          // H(nrow, j), j = 1 .. ncol
    int32_t* const last_col = last_row + ncol + 1;    // H(i, ncol), i = 1 .. nrow
    int2* const bnd = reinterpret_cast<int2*>(bt + J.lr_off);     // [ncol + 1], entry 0 unused
    for (int x = lane; x < ncol; x += 64) sh_strip[x] = swp[x];
    __syncthreads();
    const int n_strips = (nrow + kStripRows - 1) / kStripRows;
    for (int s = 0; s < n_strips; ++s) {
        const int base = s * kStripRows;              // rows base + 1 .. base + n_own
        const int n_own = min(nrow - base, kStripRows);
        const bool last = s == n_strips - 1;
        const int r0 = base + lane * RPL;
        int sa[RPL], hl[RPL], gs[RPL];
#pragma unroll
        for (int k = 0; k < RPL; ++k) {
            const int i = r0 + k + 1;
            const int b = (int)own[min(i, nrow) - 1];                 // every lane loads (a guarded load waits for its own round trip, 32 in a row)
            sa[k] = i <= nrow ? b : 256;                              // padding rows never match and feed nothing beyond them
            hl[k] = sw_edge(indel, P, i);                             // H(i, 0)
            gs[k] = kLowInit;                                         // E(i, 0)
        }
        int diag_in = sw_edge(r0 != 0 && indel, P, r0);               // H(r0, 0), H(0, 0) = 0; lane 0 of a later strip: the row above the seam
        const int n_lanes = (n_own + RPL - 1) / RPL, steps = ncol + n_lanes - 1;
        const int lane_last = (n_own - 1) / RPL, k_last = (n_own - 1) % RPL;
        u8* const btp = bt + J.bt_off + (u64)s * strip_bt_stride((u64)ncol);
        // the row above this strip, 64 columns per block of 64 steps: lane l holds column (block start) + l
        auto fetch = [&](int j, int& h, int& f) {
            h = 0; f = kLowInit;
            if (s == 0) { h = sw_edge(indel, P, j); }
            else if (j <= ncol) { const int2 v = bnd[j]; h = v.x; f = v.y; }
        };
        int cur_h = 0, cur_f = kLowInit, nxt_h, nxt_f;
        fetch(1 + lane, nxt_h, nxt_f);
        int send_h = 0, send_g = kLowInit;
        for (int t0 = 1; t0 <= steps; t0 += 64) {     // blocks of 64 steps: the sweep proper has no load to wait for
            cur_h = nxt_h; cur_f = nxt_f;
            fetch(t0 + 64 + lane, nxt_h, nxt_f);
            const int t1 = min(t0 + 63, steps);
            for (int t = t0; t <= t1; ++t) {
                const int rh = __shfl_up(send_h, 1, 64), rg = __shfl_up(send_g, 1, 64);
                const int bh = __builtin_amdgcn_readlane(cur_h, t - t0), bf = __builtin_amdgcn_readlane(cur_f, t - t0);
                const int j = t - lane;
                if (j >= 1 && j <= ncol && lane < n_lanes) {
                    int up_h = lane == 0 ? bh : rh, up_g = lane == 0 ? bf : rg;      // H(r0, j), F(r0, j)
                    int diag = diag_in;                                               // H(r0, j - 1)
                    diag_in = up_h;
                    const int c2 = (int)sh_strip[j - 1];
                    u32 packed[RPL / 4] = {};
#pragma unroll
                    for (int k = 0; k < RPL; ++k) sw_cell(P, sa[k], c2, k, hl[k], gs[k], diag, up_h, up_g, packed[k >> 2]);
                    send_h = up_h; send_g = up_g;
                    if (lane == lane_last) {
                        if (!last) bnd[j] = make_int2(up_h, up_g);        // lane 63, row base + kStripRows
                        else MGX_SW_LAST_ROW_H(last_row[j], hl, k_last);
                    }
                    MGX_SW_STORE_BT(btp + bt_slot_at(t, lane, 64, SLOT), packed);
                }
            }
        }
        if (lane < n_lanes) {
#pragma unroll
            for (int k = 0; k < RPL; ++k) if (r0 + k + 1 <= nrow) last_col[r0 + k + 1] = hl[k];
        }
        __threadfence();                              // this strip's boundary stores before the next strip's loads
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same fill with packed 16-bit scores (round 3).  The 32-bit sweep issues ~26 integer instructions per cell (compare + select for
// every tie rule and flag); here a lane group carries TWO pairs, one in each half of every register (v_pk_add / v_pk_max / v_pk_sub _i16),
// and the four decisions of a cell -- E opened, F opened, E beats the diagonal, F beats both -- are the SIGN BITS of four packed
// differences, merged with v_bfi into one nibble per pair: ~25 instructions per two cells.  Values are the reference's exactly as long
// as nothing wraps: the host admits a pair only when every real value and every difference of two of them fits 16 bits
// (I16Rule, sw_i16_rule.h: bounds from the lengths and the scoring parameters; LOW_INIT_VALUE becomes a per-pair value below every real one),
// everything else takes k_sw_fill.  Cells outside a pair's own matrix (the other half is longer, padding rows) may wrap: nothing real
// reads them.
//   * back-trace: one 32-bit word per lane, step and four rows: low half = the first pair's four nibbles (row 4q in bits 0-3),
//     high half = the second pair's; nibble = {8: E opened, 4: F opened, 2: E > diagonal, 1: F > max(diagonal, E)}
//   * H(nrow, j): the lane that owns a pair's last row stores its RPL packed H values per step (three or four store instructions;
//     picking the one row out of the registers would cost RPL selects per step); the trace kernel reads row (nrow - 1) % RPL of it
//   * H(i, ncol): every lane stores its RPL packed H values when it passes the pair's last column (the other pair may sweep on)
//   * every class of a batch runs in ONE launch (a wave-uniform switch over RPL; classes are padded to whole wavefronts with filler
//     jobs): 20 000 pairs are 5 000 wavefronts -- per-class launches of a few hundred wavefronts each would leave the device idle.
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 pk2(int lo, int hi) { s16x2 v; v.x = (short)lo; v.y = (short)hi; return v; }
__device__ __forceinline__ u32 bits(s16x2 v) { return __builtin_bit_cast(u32, v); }
__device__ __forceinline__ s16x2 s16(u32 v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ s16x2 pk_max(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }
// (a & mask) | (b & ~mask) in one instruction; written out, the compiler splits it into v_and + v_and_or (no 32-bit literals in VOP3 on gfx9)
__device__ __forceinline__ u32 bfi(u32 mask, u32 a, u32 b) { u32 r; asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(mask), "v"(a), "v"(b)); return r; }
// 1 in every half whose bases differ (as a compare it becomes two 16-bit compares, two selects and a v_perm)
__device__ __forceinline__ u32 pk_min_u16(u32 a, u32 b) { u32 r; asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ s16x2 pk_mad(u32 a, s16x2 b, s16x2 c) { u32 r; asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(bits(b)), "v"(bits(c))); return s16(r); }

template <int G, int RPL>
__device__ __forceinline__ void sw_fill16_body(const SwJob& JA, const SwJob& JB, const int lane, const u8* __restrict__ s1, const u8* __restrict__ s2,
                                               u8* __restrict__ bt, int32_t* __restrict__ sc, u32* sh, const SwParams P) {
    constexpr int GPW = 64 / G;
    constexpr int W = (RPL + 3) / 4;                  // back-trace words per lane and step
    const int nrowA = (int)JA.len1, ncolA = (int)JA.len2, nrowB = (int)JB.len1, ncolB = (int)JB.len2;
    const int n_swp = max(ncolA, ncolB);
    const bool indelA = JA.strategy == MGX_SW_INDEL || JA.strategy == MGX_SW_LEADING_INDEL;
    const bool indelB = JB.strategy == MGX_SW_INDEL || JB.strategy == MGX_SW_LEADING_INDEL;
    const u8* rowsA = s1 + JA.off1; const u8* rowsB = s1 + JB.off1;
    const u8* colsA = s2 + JA.off2; const u8* colsB = s2 + JB.off2;
    for (int x = lane; x < n_swp; x += G) sh[x] = (x < ncolA ? (u32)colsA[x] : 0u) | ((x < ncolB ? (u32)colsB[x] : 0u) << 16);
    __syncthreads();
    const int r0 = lane * RPL;
    const s16x2 vopen = pk2(P.open, P.open), vext = pk2(P.extend, P.extend), vmatch = pk2(P.match, P.match);
    const s16x2 vdelta = pk2(P.mismatch - P.match, P.mismatch - P.match);
    const s16x2 vlow = pk2(JA.low16, JB.low16);
    u32 sa[RPL];
    s16x2 hl[RPL], gs[RPL];
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
        const int i = r0 + k + 1;
        sa[k] = (i <= nrowA ? (u32)rowsA[i - 1] : 256u) | ((i <= nrowB ? (u32)rowsB[i - 1] : 256u) << 16);
        hl[k] = pk2(sw_edge(indelA, P, i), sw_edge(indelB, P, i));                                 // H(i, 0)
        gs[k] = vlow;                                                                             // E(i, 0)
    }
    s16x2 diag_in = r0 == 0 ? pk2(0, 0) : pk2(sw_edge(indelA, P, r0), sw_edge(indelB, P, r0));    // H(r0, 0)
    s16x2 bnd = pk2(indelA ? P.open : 0, indelB ? P.open : 0);                      // lane 0: H(0, j), starting at j = 1
    const s16x2 bstep = pk2(indelA ? P.extend : 0, indelB ? P.extend : 0);
    const int n_lanes = max((nrowA + RPL - 1) / RPL, (nrowB + RPL - 1) / RPL);
    const int steps = n_lanes > 0 ? n_swp + n_lanes - 1 : 0;
    int steps_w = steps;
    if constexpr (GPW > 1) {
        const int other = __shfl_xor(steps, G, 64);
        steps_w = other > steps ? other : steps;
    }
    const int lane_lastA = nrowA > 0 ? (nrowA - 1) / RPL : -1, lane_lastB = nrowB > 0 ? (nrowB - 1) / RPL : -1;
    u32* const lrA = reinterpret_cast<u32*>(bt + JA.lr_off);
    u32* const lrB = reinterpret_cast<u32*>(bt + JB.lr_off);
    const bool lr_apart = JA.lr_off != JB.lr_off;
    u32* const lcA = reinterpret_cast<u32*>(bt + JA.lc_off);
    u32* const lcB = reinterpret_cast<u32*>(bt + JB.lc_off);
    const bool lc_apart = JA.lc_off != JB.lc_off;
    u8* const btp = bt + JA.bt_off;
    s16x2 send_h = pk2(0, 0), send_g = vlow;
    for (int t = 1; t <= steps_w; ++t) {
        const u32 rh = (u32)__builtin_amdgcn_update_dpp(0, (int)bits(send_h), 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        const u32 rg = (u32)__builtin_amdgcn_update_dpp(0, (int)bits(send_g), 0x138, 0xf, 0xf, false);
        const int j = t - lane;
        if (j >= 1 && j <= n_swp && lane < n_lanes) {
            s16x2 up_h = lane == 0 ? bnd : s16(rh);                  // H(r0, j)
            s16x2 up_g = lane == 0 ? vlow : s16(rg);                 // F(r0, j)
            bnd += bstep;
            s16x2 diag = diag_in;                                    // H(r0, j - 1)
            diag_in = up_h;
            const u32 c2 = sh[j - 1];
            u32 word[W];
#pragma unroll
            for (int q = 0; q < W; ++q) word[q] = 0;
#pragma unroll
            for (int k = 0; k < RPL; ++k) {
                const s16x2 open_s = hl[k] + vopen, ext_s = gs[k] + vext;
                const s16x2 ee = pk_max(open_s, ext_s);
                const s16x2 open_c = up_h + vopen, ext_c = up_g + vext;
                const s16x2 ff = pk_max(ext_c, open_c);
                const u32 ne = pk_min_u16(sa[k] ^ c2, 0x00010001u);                                    // 1 where the bases differ
                const s16x2 h0 = diag + pk_mad(ne, vdelta, vmatch);
                const s16x2 m1 = pk_max(h0, ee);
                const s16x2 h = pk_max(m1, ff);
                // sign bit set: E opened (no INSERT_EXT) | F opened (no DELETE_EXT) | ee > h0 | ff > max(h0, ee)
                const u32 t1 = bits(ext_s - open_s), t2 = bits(ext_c - open_c), t3 = bits(h0 - ee), t4 = bits(m1 - ff);
                const u32 u12 = bfi(0x80008000u, t1, t2 >> 1), u34 = bfi(0x80008000u, t3, t4 >> 1);
                const u32 nib = bfi(0xC000C000u, u12, u34 >> 2);
                word[k >> 2] = bfi(0xF000F000u, nib, word[k >> 2] >> 4);
                diag = hl[k]; hl[k] = h; gs[k] = ee; up_h = h; up_g = ff;
            }
            if constexpr (RPL % 4 != 0) word[W - 1] >>= 4 * (4 - RPL % 4);
            send_h = up_h; send_g = up_g;
            u32* dst = reinterpret_cast<u32*>(btp + bt_slot_at(t, lane, G, bt_slot16(RPL)));
#pragma unroll
            for (int q = 0; q < W; ++q) dst[q] = word[q];
            // the lane's RPL packed H values (both halves) where LastRow / LastCol read them; a macro for the reason MGX_SW_LAST_ROW_H is one
#define MGX_SW16_STORE_ROWS(dst) do { u32* d_ = (dst); _Pragma("unroll") for (int k = 0; k < RPL; ++k) d_[k] = bits(hl[k]); } while (0)
            if (lane == lane_lastA) MGX_SW16_STORE_ROWS(lrA + lr16_at(j, RPL, 0));
            if (lr_apart && lane == lane_lastB) MGX_SW16_STORE_ROWS(lrB + lr16_at(j, RPL, 0));
            if (j == ncolA) MGX_SW16_STORE_ROWS(lcA + lc16_at(r0 + 1));
            if (lc_apart && j == ncolB) MGX_SW16_STORE_ROWS(lcB + lc16_at(r0 + 1));
#undef MGX_SW16_STORE_ROWS
        }
    }
}

// jobs: pairs 2g and 2g + 1 share lane group g; both of one class (rpl), a class ends on a wavefront boundary.  BIG: the classes of
// more than 16 rows per lane, a kernel of their own (178 registers; the common one keeps 100 and twice the wavefronts per SIMD)
template <int G, bool BIG>
__global__ __launch_bounds__(64) void k_sw_fill16(const SwJob* __restrict__ jobs, u32 n_jobs, const u8* __restrict__ s1, const u8* __restrict__ s2,
                                                  u8* __restrict__ bt, int32_t* __restrict__ sc, u32 lds_stride, SwParams P) {
    extern __shared__ u32 sh16_all[];
    constexpr int GPW = 64 / G;
    const int grp = threadIdx.x / G, lane = threadIdx.x % G;
    const u32 g = blockIdx.x * GPW + grp;
    SwJob JA{}, JB{};
    if (2 * g < n_jobs) { JA = jobs[2 * g]; JB = jobs[2 * g + 1]; }
    u32* sh = sh16_all + (size_t)grp * lds_stride;
    const int rpl = __builtin_amdgcn_readfirstlane((int)jobs[2 * (size_t)blockIdx.x * GPW].rpl);       // the wavefront's class
#define MGX_SW16_CASE(r) case r: sw_fill16_body<G, r>(JA, JB, lane, s1, s2, bt, sc, sh, P); break;
    if constexpr (BIG) {
        switch (rpl) {
            MGX_SW16_CASE(20) MGX_SW16_CASE(24) MGX_SW16_CASE(32)
            default: break;
        }
    } else {
        switch (rpl) {
            MGX_SW16_CASE(1) MGX_SW16_CASE(2) MGX_SW16_CASE(3) MGX_SW16_CASE(4) MGX_SW16_CASE(5) MGX_SW16_CASE(6) MGX_SW16_CASE(7) MGX_SW16_CASE(8)
            MGX_SW16_CASE(9) MGX_SW16_CASE(10) MGX_SW16_CASE(11) MGX_SW16_CASE(12) MGX_SW16_CASE(13) MGX_SW16_CASE(14) MGX_SW16_CASE(16)
            default: break;
        }
    }
#undef MGX_SW16_CASE
}

// The walk's diagonal provider on the device (sw_trace_rule.h: walk, LanesDiag is its CPU twin): the 64 lanes fetch the next 64 cells of the
// current DIAGONAL in one gather (lane t: cell (c_i - t, c_j - t)) and the walk consumes them from registers.  A run of diagonal matches
// is consumed in ONE step (round 3): the walk is wave-uniform -- one cell per iteration keeps 63 lanes idle for ~275 iterations per pair,
// and that issue time, not the memory, was most of the trace kernel.
struct WaveDiag {
    const BtView& view; const int lane;
    int cached = 0, c_i = 0, c_j = 0, tt = 0;
    bool valid = false;
    __device__ __forceinline__ int run(int i, int j) {
        if (!diag_cached(valid, c_i, c_j, i, j)) {
            c_i = i; c_j = j; valid = true;
            const int ii = i - lane, jj = j - lane;
            cached = (ii >= 1 && jj >= 1) ? view.cell(ii, jj) : 0;
        }
        tt = __builtin_amdgcn_readfirstlane(c_i - i);
        return diag_run(__ballot((cached & 3) == kOpMatch), tt, i, j);
    }
    __device__ __forceinline__ int byte(int, int) const { return __builtin_amdgcn_readlane(cached, tt); }
};

// One WAVEFRONT per pair: best end cell, back-trace, merged element list (in the order getCIGAR holds it).  A lane per
// pair walks ~275 dependent byte loads of ~2 us each with a third of a wavefront per SIMD to hide them
// behind; here an alignment of a few hundred matches with a handful of gaps costs a handful of memory round trips (WaveDiag).
// Inside a gap (extension states) cells are loaded one at a time as before.  The rules are sw_trace_rule.h's; the kernel keeps
// how the edges are loaded, the maximum, the provider and lane 0's element store, and the compact copy.
__global__ __launch_bounds__(64) void k_sw_trace_wave(const SwJob* __restrict__ jobs, u32 n, const u8* __restrict__ bt,
                                                      const int32_t* __restrict__ sc, int16_t* __restrict__ elems_all, SwResult* __restrict__ res,
                                                      int16_t* __restrict__ compact, int n_compact) {
    const u32 p = blockIdx.x;
    if (p >= n) return;
    const int lane = threadIdx.x;
    const SwJob J = jobs[p];
    if (J.out_index == kNoOutput) return;
    const int nrow = (int)J.len1, ncol = (int)J.len2, strategy = (int)J.strategy;
    const LastRow last_row(J, bt, sc);
    const LastCol last_col(J, bt, sc);
    const BtView view(J, bt);
    int16_t* el = elems_all + J.el_off;
    const bool use_row = strategy == MGX_SW_SOFTCLIP || strategy == MGX_SW_IGNORE;
    // ---- best end cell.  The maximum first, in parallel; then the cells that reach it go through EndCell::replay, 64 anti-diagonals a ballot
    int best = INT32_MIN;
    EndCell end(nrow, ncol);
    constexpr int kEdgeRegs = 8;
    if (nrow + ncol <= 64 * kEdgeRegs) {
        // the usual case (a read against its haplotype window): both edges fit the wavefront's registers -- all loads issued at
        // once, the maximum and the replay from registers (round 3; the two-pass form below paid one memory round trip per 64
        // anti-diagonals in the replay, behind the one for the maximum)
        int va[kEdgeRegs], vb[kEdgeRegs];
#pragma unroll
        for (int q = 0; q < kEdgeRegs; ++q) {
            const int d = 1 + 64 * q + lane, ja = d - nrow, ib = d - ncol;
            va[q] = (use_row && d <= nrow + ncol && ja >= 1) ? last_row[ja] : INT32_MIN;      // (no score is INT32_MIN: MATRIX_MIN_CUTOFF bounds them)
            vb[q] = (d <= nrow + ncol && ib >= 1) ? last_col[ib] : INT32_MIN;
            best = max(best, max(va[q], vb[q]));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off, 64));
#pragma unroll
        for (int q = 0; q < kEdgeRegs; ++q) {
            if (1 + 64 * q > nrow + ncol) break;
            end.replay(1 + 64 * q, __ballot(va[q] == best), __ballot(vb[q] == best));
        }
    } else {
        if (use_row) for (int j = 1 + lane; j <= ncol; j += 64) best = max(best, last_row[j]);
        for (int i = 1 + lane; i <= nrow; i += 64) best = max(best, last_col[i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off, 64));
        for (int d0 = 1; d0 <= nrow + ncol; d0 += 64) {
            const int d = d0 + lane;
            const int ja = d - nrow, ib = d - ncol;
            const bool eq_a = use_row && d <= nrow + ncol && ja >= 1 && last_row[ja] == best;
            const bool eq_b = d <= nrow + ncol && ib >= 1 && last_col[ib] == best;
            end.replay(d0, __ballot(eq_a), __ballot(eq_b));
        }
    }
    // ---- back-trace: the walk is wave-uniform, lane 0 writes the elements
    WaveDiag diag{view, lane};
    const Walked w = walk(nrow, ncol, strategy, end.mi, end.mj, [&](int i, int j) { return view.cell(i, j); }, diag,
                          [&](int k, int op, int len) { if (lane == 0) { el[2 * k] = (int16_t)op; el[2 * k + 1] = (int16_t)len; } });
    if (lane == 0) {
        SwResult r; r.score = best; r.max_i = end.mi; r.max_j = end.mj; r.offset = w.offset; r.n_elems = w.n_elems;
        res[J.out_index] = r;
    }
    __syncthreads();                             // lane 0's element stores before the block's lanes copy them
    int16_t* ce = compact + (size_t)J.out_index * 2 * n_compact;
    for (int q = lane; q < 2 * min(w.n_elems, n_compact); q += 64) ce[q] = el[q];
}

// alignments with more than kCompactElems elements: their element lists are packed densely for one download
struct GatherRef { u64 src, dst; u32 n; u32 pad_; };     // int16 offsets, n = number of int16 values
__global__ __launch_bounds__(256) void k_sw_gather(const GatherRef* __restrict__ refs, u32 n_refs, const int16_t* __restrict__ el,
                                                   int16_t* __restrict__ dense) {
    for (u32 r = blockIdx.x; r < n_refs; r += gridDim.x) {
        const GatherRef g = refs[r];
        for (u32 x = threadIdx.x; x < g.n; x += 256) dense[g.dst + x] = el[g.src + x];
    }
}

// knobs of one call, read from the environment once (tests and A/B runs set them between calls)
struct Knobs {
    int paired = -1;          // MGX_SW_PAIRED: force two lane groups per wavefront (1) or one (0)
    bool use16 = true;        // MGX_SW_I16=0: the 32-bit fill for every pair
    u64 arena = 0;            // MGX_SW_ARENA_LIMIT
    Knobs() {
        if (const char* e = getenv("MGX_SW_PAIRED")) paired = atoi(e) != 0;
        if (const char* e = getenv("MGX_SW_I16")) use16 = atoi(e) != 0;
        if (const char* e = getenv("MGX_SW_ARENA_LIMIT")) { const long long v = atoll(e); if (v > 0) arena = (u64)v; }
    }
};
constexpr int kCompactElems = 16;             // merged CIGAR elements copied back per pair without a second look

using mgx_hip::PinBuf;
using mgx_hip::DevArray;
// the context's device arrays grow by a quarter and 64 elements over what is asked
template <typename T> int grow(DevArray<T>& a, size_t n) { return a.reserve(n, n + n / 4 + 64); }

}  // namespace

struct mgx_sw {
    mgx_hip::Owner own;           // of the stream and the events; the first member: the stream goes last
    int device = 0;
    unsigned flags = 0;           // MGX_SW_*
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevArray<u8> d_s1, d_s2, d_bt;
    DevArray<SwJob> d_jobs;
    DevArray<int32_t> d_sc;
    DevArray<int16_t> d_el, d_cel, d_dense;
    DevArray<GatherRef> d_gather;
    DevArray<SwResult> d_res;
    mgx_sw_stats_t stats{};
    PinBuf pin;                   // pinned staging for the uploads (a pageable source is copied at a few GB/s)
    PinBuf pin_out;               // pinned landing area of the results (a pageable target goes through the runtime's own staging)
};

namespace {
// back-trace bytes per chunk of a batch (MGX_SW_ARENA_LIMIT overrides).  Measured on 200 000 pairs: with 8-12 GB
// chunks the call took 50-60 ms (a 20 ms stall follows every very large chunk), with 4 GB chunks 29 ms.
constexpr u64 kArenaLimit = 4ull << 30;

// pairs [lo, hi) of the input, already validated
struct Chunk {
    u64 lo, hi; u32 n;
    u64 base1, base2, n1, n2;     // the first byte and the byte count of the chunk's references / alternates in the caller's arrays
    size_t a1, a2;                // the byte counts rounded up to 256: pinned memory holds [references | alternates | jobs]
    Chunk(const mgx_sw_input_t* in, u64 lo_, u64 hi_) : lo(lo_), hi(hi_), n((u32)(hi_ - lo_)), base1(in->ref_off[lo_]), base2(in->alt_off[lo_]),
        n1(in->ref_off[hi_] - base1), n2(in->alt_off[hi_] - base2), a1((n1 + 255) & ~(size_t)255), a2((n2 + 255) & ~(size_t)255) {}
};
struct Outputs { int32_t* offset; char* cigar; u32 stride; int32_t* score; int cap_override; mgx_internal::SwElementSink* sink; };      // the caller's, indexed by input pair
Lens pair_lens(const mgx_sw_input_t* in, u64 p) { return mgx_sw_layout::pair_lens(in->ref_off, in->alt_off, p); }
using mgx_internal::SwDeviceSource;
struct Stager {                   // the helper threads of stage_sequences: upload_jobs joins them, and so does every way out before it
    std::thread t[2]; std::atomic<int> err{0}; bool apart = false;
    bool on_device = false;       // gather_sequences: the sequences are queued on the stream already
    void join() { for (auto& x : t) if (x.joinable()) x.join(); }
    ~Stager() { join(); }
};
// The sequences travel to pinned memory, on helper threads when there is a megabyte of them, while the caller lays out the jobs.
int stage_sequences(mgx_sw* c, const mgx_sw_input_t* in, const Chunk& k, Stager& st) {
    const size_t total = k.a1 + k.a2 + max_jobs(k.n) * sizeof(SwJob);
    int rc;
    if ((rc = c->pin.reserve(total, total + total / 4)) || (rc = grow(c->d_s1, k.n1 + 16)) || (rc = grow(c->d_s2, k.n2 + 16))) return rc;
    char* const pin = c->pin.p;
    st.apart = k.n1 + k.n2 >= (1u << 20);
    if (!st.apart) { memcpy(pin, in->ref + k.base1, k.n1); memcpy(pin + k.a1, in->alt + k.base2, k.n2); return 0; }
    // each helper also queues its array's upload as soon as it is staged: the copies cross the link while the jobs are laid out
    auto stage = [c, &st](u8* dst, char* via, const u8* src, size_t bytes) {
        memcpy(via, src, bytes);
        if (hipSetDevice(c->device) != hipSuccess || hipMemcpyAsync(dst, via, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) st.err = 1;
    };
    st.t[0] = std::thread(stage, c->d_s1.p, pin, in->ref + k.base1, (size_t)k.n1);
    st.t[1] = std::thread(stage, c->d_s2.p, pin + k.a1, in->alt + k.base2, (size_t)k.n2);
    return 0;
}
// The same stage for sequences that lie in device memory (mgx_internal::sw_align_from_device): the stream waits for their owner,
// and the owner's gather writes them where the upload would have; pinned memory keeps its layout, the jobs behind the (unused) sequences.
int gather_sequences(mgx_sw* c, const SwDeviceSource& src, const Chunk& k, Stager& st) {
    const size_t total = k.a1 + k.a2 + max_jobs(k.n) * sizeof(SwJob);
    int rc;
    if ((rc = c->pin.reserve(total, total + total / 4)) || (rc = grow(c->d_s1, k.n1 + 16)) || (rc = grow(c->d_s2, k.n2 + 16))) return rc;
    st.on_device = true;
    if (src.ready) HIP_TRY(hipStreamWaitEvent(c->stream, src.ready, 0));
    return src.gather(src.user, c->stream, k.lo, k.hi, c->d_s1.p, c->d_s2.p);
}
// the jobs in launch order and their places in the arenas (sw_layout.h), built in place behind the sequences in pinned memory
Layout lay_out(mgx_sw* c, const mgx_sw_params_t* params, const mgx_sw_input_t* in, const Chunk& k, const Knobs& knobs, SwJob* jobs) {
    const bool paired = knobs.paired >= 0 ? knobs.paired != 0 : k.n >= kPairedFrom;
    const mgx_sw16::I16Rule rule(params->match, params->mismatch, params->gap_open, params->gap_extend);
    const Layout L = build_jobs(in->ref_off, in->alt_off, in->strategy, k.lo, k.hi, paired, knobs.use16, rule, jobs);
    c->stats.n_pairs_i16 += L.n_pairs_i16; c->stats.n_pairs_strip += L.n_pairs_strip; c->stats.n_strips += L.n_strips;
    return L;
}

int upload_jobs(mgx_sw* c, const Chunk& k, Stager& st, const Layout& L, const SwJob* jobs) {
    hipStream_t s = c->stream;
    const u64 scn = k.n1 + k.n2 + 2ull * k.n, eln = 2 * scn;
    int rc;
    if ((rc = grow(c->d_bt, L.bt_bytes + 16)) || (rc = grow(c->d_jobs, L.n_jobs)) || (rc = grow(c->d_sc, scn)) || (rc = grow(c->d_el, eln)) ||
        (rc = grow(c->d_res, k.n)) || (rc = grow(c->d_cel, (size_t)k.n * 2 * kCompactElems))) return rc;
    st.join();                                    // the helpers have queued the sequences: the jobs follow them on the stream
    if (st.err.load()) { (void)hipGetLastError(); set_error("upload of the sequences failed"); return -EIO; }
    if (!st.apart && !st.on_device) {
        HIP_TRY(hipMemcpyAsync(c->d_s1.p, c->pin.p, k.n1, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->d_s2.p, c->pin.p + k.a1, k.n2, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(c->d_jobs.p, jobs, L.n_jobs * sizeof(SwJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    return 0;
}
// one launch per next_launch (sw_layout.h); `jobs` is the host copy, the kernels read the device's
void launch_fills(mgx_sw* c, const SwJob* jobs, u32 n_jobs, const SwParams& P) {
    hipStream_t s = c->stream;
#define MGX_SW_ARGS dj, m, c->d_s1.p, c->d_s2.p, c->d_bt.p, c->d_sc.p
#define MGX_SW16_LAUNCH(G_, BIG_) hipLaunchKernelGGL((k_sw_fill16<G_, BIG_>), dim3(m / (2 * gpw)), dim3(64), gpw * stride * sizeof(u32), s, MGX_SW_ARGS, stride, P)
#define MGX_SW_FILL(G_, R_) hipLaunchKernelGGL((k_sw_fill<G_, R_>), dim3((m + 64 / G_ - 1) / (64 / G_)), dim3(64), 64 / G_ * stride, s, MGX_SW_ARGS, stride, P)
#define MGX_SW_CASE(g, r) case r: MGX_SW_FILL(g, r); break;
    for (u32 a = 0; a < n_jobs; c->stats.n_launches++) {
        const Launch l = next_launch(jobs, n_jobs, a);
        const SwJob* dj = c->d_jobs.p + a;
        const u32 m = l.end - a, g = jobs[a].g & 0xFFu, gpw = 64 / g, stride = (l.max_len2 + 15) & ~15u;      // stride: the LDS stage of one lane group
        if (jobs[a].g & kJobI16) {                        // m / (2 * gpw) whole wavefronts: build_jobs pads every class with fillers
            const bool big = jobs[a].rpl > 16;
            if (g == 32) { if (big) MGX_SW16_LAUNCH(32, true); else MGX_SW16_LAUNCH(32, false); }
            else         { if (big) MGX_SW16_LAUNCH(64, true); else MGX_SW16_LAUNCH(64, false); }
        } else if (jobs[a].g & kJobStrip) {
            hipLaunchKernelGGL(k_sw_fill_strip, dim3(m), dim3(64), stride, s, MGX_SW_ARGS, P);
        } else if (g == 32) {
            switch (jobs[a].rpl) {
                MGX_SW_CASE(32, 1) MGX_SW_CASE(32, 2) MGX_SW_CASE(32, 3) MGX_SW_CASE(32, 4) MGX_SW_CASE(32, 5) MGX_SW_CASE(32, 6) MGX_SW_CASE(32, 7)
                MGX_SW_CASE(32, 8) MGX_SW_CASE(32, 12)
                default: MGX_SW_FILL(32, 16); break;
            }
        } else {
            switch (jobs[a].rpl) {
                MGX_SW_CASE(64, 1) MGX_SW_CASE(64, 2) MGX_SW_CASE(64, 3) MGX_SW_CASE(64, 4) MGX_SW_CASE(64, 5) MGX_SW_CASE(64, 6) MGX_SW_CASE(64, 8)
                MGX_SW_CASE(64, 16)
                default: MGX_SW_FILL(64, 32); break;
            }
        }
        a = l.end;
    }
#undef MGX_SW_CASE
#undef MGX_SW_FILL
#undef MGX_SW16_LAUNCH
#undef MGX_SW_ARGS
}

int launch_trace(mgx_sw* c, u32 n_jobs) {
    hipStream_t s = c->stream;
    HIP_TRY(hipEventRecord(c->ev[1], s));
    hipLaunchKernelGGL(k_sw_trace_wave, dim3(n_jobs), dim3(64), 0, s, c->d_jobs.p, n_jobs, c->d_bt.p, c->d_sc.p, c->d_el.p, c->d_res.p, c->d_cel.p, kCompactElems);
    HIP_TRY(hipEventRecord(c->ev[2], s));
    HIP_TRY(hipGetLastError());
    return 0;
}
// what came back: a fixed record per pair, and the element lists longer than kCompactElems, densely (pair q's starts at big_at[q])
struct Fetched { const SwResult* res; const int16_t* cel; std::vector<u64> big_at; std::unique_ptr<int16_t[]> big; };
int fetch_results(mgx_sw* c, const mgx_sw_input_t* in, const Chunk& k, u64 bt_bytes, Fetched& f) {
    hipStream_t s = c->stream;
    const size_t res_bytes = ((size_t)k.n * sizeof(SwResult) + 63) & ~(size_t)63, cel_bytes = (size_t)k.n * 2 * kCompactElems * sizeof(int16_t);
    int rc;
    if ((rc = c->pin_out.reserve(res_bytes + cel_bytes, (res_bytes + cel_bytes) * 5 / 4))) return rc;
    SwResult* const res = reinterpret_cast<SwResult*>(c->pin_out.p);
    int16_t* const cel = reinterpret_cast<int16_t*>(c->pin_out.p + res_bytes);
    HIP_TRY(hipMemcpyAsync(res, c->d_res.p, k.n * sizeof(SwResult), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cel, c->d_cel.p, cel_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // alignments with more elements than the fixed record holds: one gather launch, one more download
    std::vector<GatherRef> big_refs;
    f.big_at.assign(k.n, ~0ull);
    u64 eo2 = 0, dense_n = 0;
    for (u32 q = 0; q < k.n; ++q) {
        if (res[q].n_elems > kCompactElems) {
            f.big_at[q] = dense_n;
            big_refs.push_back(GatherRef{eo2, dense_n, (u32)(2 * res[q].n_elems), 0});
            dense_n += 2ull * res[q].n_elems;
        }
        const Lens l = pair_lens(in, k.lo + q);
        eo2 += 2 * (l.l1 + l.l2 + 2);
    }
    f.big.reset(new (std::nothrow) int16_t[dense_n + 1]);
    if (!f.big) return -ENOMEM;
    if (!big_refs.empty()) {
        if ((rc = grow(c->d_gather, big_refs.size())) || (rc = grow(c->d_dense, dense_n))) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_gather.p, big_refs.data(), big_refs.size() * sizeof(GatherRef), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_sw_gather, dim3((u32)std::min<size_t>(big_refs.size(), 65535)), dim3(256), 0, s, c->d_gather.p,
                           (u32)big_refs.size(), c->d_el.p, c->d_dense.p);
        HIP_TRY(hipMemcpyAsync(f.big.get(), c->d_dense.p, dense_n * sizeof(int16_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->stats.ms_fill += ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); c->stats.ms_trace += ms;
    c->stats.backtrace_bytes += bt_bytes;
    f.res = res; f.cel = cel;
    return 0;
}
// results and CIGAR text, a few threads when the batch is large (rendering long element lists is the library's biggest host cost)
void emit_text(mgx_sw* c, const mgx_sw_input_t* in, const Chunk& k, const Fetched& f, const Outputs& out) {
    if (out.sink) {             // room for every element of the chunk; chunks come in pair order
        for (u32 q = 0; q < k.n; ++q) out.sink->off[k.lo + q + 1] = out.sink->off[k.lo + q] + (u64)std::max(f.res[q].n_elems, 0);
        out.sink->el.resize(out.sink->off[k.lo + k.n]);
    }
    auto emit = [&](u32 q0, u32 q1, u64* cells_out) {
        u64 cells = 0;
        for (u32 q = q0; q < q1; ++q) {
            const u64 p = k.lo + q;
            const Lens l = pair_lens(in, p);
            const SwResult& r = f.res[q];
            out.offset[p] = r.offset;
            if (out.score) out.score[p] = r.score;
            if (out.cigar || out.sink) {
                char* dst = out.cigar ? out.cigar + (size_t)p * out.stride : nullptr;
                const int cap = out.cap_override >= 0 ? out.cap_override : text_cap(l.l1, l.l2, out.cigar ? (u64)out.stride : kNoStride);
                const int16_t* src = r.n_elems > kCompactElems ? f.big.get() + f.big_at[q] : f.cel + (size_t)q * 2 * kCompactElems;
                const int len = render(src, r.n_elems, dst, cap, out.sink ? out.sink->el.data() + out.sink->off[p] : nullptr, out.sink ? &out.sink->n[p] : nullptr);
                if (dst) dst[len] = 0;                    // cap <= stride - 1
            }
            cells += l.l1 * l.l2;
        }
        *cells_out = cells;
    };
    constexpr u32 kThreads = 4;
    u64 cells[kThreads] = {0};
    if (k.n < 16384) emit(0, k.n, &cells[0]);
    else {
        std::thread th[kThreads];
        for (u32 t = 0; t < kThreads; ++t) th[t] = std::thread(emit, (u32)((u64)k.n * t / kThreads), (u32)((u64)k.n * (t + 1) / kThreads), &cells[t]);
        for (auto& t : th) t.join();
    }
    for (u64 x : cells) c->stats.cells += x;
}

int run_chunk(mgx_sw* c, const mgx_sw_params_t* params, const mgx_sw_input_t* in, const Chunk& k, const Knobs& knobs, const Outputs& out,
              const SwDeviceSource* src) {
    static const bool prof = [] { const char* e = getenv("MGX_SW_PROF"); return e && atoi(e) != 0; }();      // host stage times on stderr
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tp[6] = {now()};
    const SwParams P{params->match, params->mismatch, params->gap_open, params->gap_extend};
    Stager st;
    Fetched f;
    if (int rc = src ? gather_sequences(c, *src, k, st) : stage_sequences(c, in, k, st)) return rc;
    SwJob* const jobs = reinterpret_cast<SwJob*>(c->pin.p + k.a1 + k.a2);
    const Layout L = lay_out(c, params, in, k, knobs, jobs);
    tp[1] = now();
    if (int rc = upload_jobs(c, k, st, L, jobs)) return rc;
    tp[2] = now();
    launch_fills(c, jobs, L.n_jobs, P);
    if (int rc = launch_trace(c, L.n_jobs)) return rc;
    tp[3] = now();
    if (int rc = fetch_results(c, in, k, L.bt_bytes, f)) return rc;
    tp[4] = now();
    emit_text(c, in, k, f, out);
    tp[5] = now();
    if (prof) fprintf(stderr, "[mgx_sw] %u pairs: jobs %.3f  stage+H2D %.3f  launches %.3f  kernels+D2H %.3f  text %.3f ms\n", k.n, tp[1] - tp[0], tp[2] - tp[1],
                      tp[3] - tp[2], tp[4] - tp[3], tp[5] - tp[4]);
    return 0;
}

}  // namespace

extern "C" {

int mgx_sw_create(int device, unsigned flags, mgx_sw_t** out) {
    if (!out) { set_error("out is NULL"); return -EINVAL; }
    *out = nullptr;
    if (const int rc = mgx_hip::pick_device(&device, nullptr)) return rc;
    std::unique_ptr<mgx_sw> c(new (std::nothrow) mgx_sw);
    if (!c) return -ENOMEM;
    c->device = device;
    c->flags = flags;
    c->own.stream(&c->stream);
    for (auto& e : c->ev) c->own.event(&e);
    if (!c->own.ok()) return c->own.error("a Smith-Waterman context");
    *out = c.release();
    return 0;
}

void mgx_sw_destroy(mgx_sw_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
}

static int align_impl(mgx_sw_t* c, const mgx_sw_params_t* params, const mgx_sw_input_t* in,
                      int32_t* out_offset, char* out_cigar, uint32_t cigar_stride, int32_t* out_score, int cap_override,
                      const SwDeviceSource* src = nullptr, mgx_internal::SwElementSink* sink = nullptr) {
    if (!c || !params || !in || !out_offset) { set_error("NULL argument"); return -EINVAL; }
    if (out_cigar && cigar_stride < 2) { set_error("cigar_stride must be at least 2"); return -EINVAL; }
    c->stats = mgx_sw_stats_t{};
    c->stats.n_pairs = in->n_pairs;
    if (sink) { sink->off.assign(in->n_pairs + 1, 0); sink->n.assign(in->n_pairs, 0); sink->el.clear(); }
    if (in->n_pairs == 0) return 0;
    if (!in->ref_off || !in->alt_off || (!src && (!in->ref || !in->alt)) || !in->strategy) { set_error("NULL array in input"); return -EINVAL; }
    if (in->n_pairs > 0x7FFFFFFFull) { set_error("more than 2^31-1 pairs in one batch"); return -E2BIG; }
    const int max_ref = (c->flags & MGX_SW_LONG_REF) ? kMaxLen : kMaxRef;
    for (u64 p = 0; p < in->n_pairs; ++p) {
        if (in->ref_off[p + 1] < in->ref_off[p] || in->alt_off[p + 1] < in->alt_off[p]) { set_error("pair %llu: offsets decrease", (unsigned long long)p); return -EINVAL; }
        const auto [l1, l2] = pair_lens(in, p);
        if (l1 == 0 || l2 == 0) { set_error("pair %llu: empty sequence", (unsigned long long)p); return -EINVAL; }
        if (l1 > (u64)max_ref) { set_error("pair %llu: reference of %llu bases (limit %d)", (unsigned long long)p, (unsigned long long)l1, max_ref); return -E2BIG; }
        if (l2 > (u64)kMaxLen) { set_error("pair %llu: alternate of %llu bases (limit 32767)", (unsigned long long)p, (unsigned long long)l2); return -E2BIG; }
        const int st = in->strategy[p];
        if (st < MGX_SW_SOFTCLIP || st > MGX_SW_IGNORE) { set_error("pair %llu: unknown overhang strategy %d", (unsigned long long)p, st); return -EINVAL; }
    }
    HIP_TRY(hipSetDevice(c->device));
    const Knobs knobs;
    const u64 limit = knobs.arena ? knobs.arena : kArenaLimit;
    const Outputs out{out_offset, out_cigar, cigar_stride, out_score, cap_override, sink};
    for (u64 lo = 0, hi; lo < in->n_pairs; lo = hi) {
        hi = chunk_end(in->ref_off, in->alt_off, in->n_pairs, lo, limit);      // by chunk_bound per pair (sw_layout.h)
        const int rc = run_chunk(c, params, in, Chunk(in, lo, hi), knobs, out, src);
        if (rc) return rc;
    }
    return 0;
}

int mgx_sw_align_batch(mgx_sw_t* c, const mgx_sw_params_t* params, const mgx_sw_input_t* in,
                       int32_t* out_offset, char* out_cigar, uint32_t cigar_stride, int32_t* out_score) {
    return align_impl(c, params, in, out_offset, out_cigar, cigar_stride, out_score, -1);
}

int mgx_sw_align(mgx_sw_t* c, const uint8_t* ref, int refLength, const uint8_t* alt, int altLength,
                 uint8_t* cigar, int cigarLength, int match, int mismatch, int open, int extend, uint8_t strategy) {
    if (!c || !ref || !alt || !cigar || refLength <= 0 || altLength <= 0 || cigarLength < 1) { set_error("bad argument"); return MGX_SW_ALIGN_ERROR(EINVAL); }
    const uint64_t o1[2] = {0, (uint64_t)refLength}, o2[2] = {0, (uint64_t)altLength};
    const mgx_sw_params_t P{match, mismatch, open, extend};
    const mgx_sw_input_t in{1, o1, ref, o2, alt, &strategy};
    int32_t off = 0;
    // the reference renders into a buffer of cigarLength bytes (the caller passes 2 * max(len)), zero-filled
    std::vector<char> tmp((size_t)cigarLength + 1, 0);
    const int rc = align_impl(c, &P, &in, &off, tmp.data(), (uint32_t)cigarLength + 1, nullptr, cigarLength);
    if (rc) return MGX_SW_ALIGN_ERROR(-rc);
    memcpy(cigar, tmp.data(), (size_t)cigarLength);
    return off;
}

int mgx_sw_stats(mgx_sw_t* c, mgx_sw_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = c->stats;
    return 0;
}

}  // extern "C"

namespace mgx_internal {
int sw_align_from_device(mgx_sw_t* c, const mgx_sw_params_t* params, const mgx_sw_input_t* in, const SwDeviceSource& src,
                         int32_t* out_offset, char* out_cigar, uint32_t cigar_stride, int32_t* out_score, SwElementSink* sink) {
    if (!src.gather) { set_error("NULL argument"); return -EINVAL; }
    return align_impl(c, params, in, out_offset, out_cigar, cigar_stride, out_score, -1, &src, sink);
}
SwView sw_view(mgx_sw_t* c) { return SwView{c->device, (c->flags & MGX_SW_LONG_REF) ? kMaxLen : kMaxRef, kMaxLen}; }
}  // namespace mgx_internal
