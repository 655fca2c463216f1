// mgx_bgzf.hip -- BGZF block compression on gfx950 (C ABI: include/mgx_bgzf.h), SURVEY.md 8f row F3.
//
// What the reference's writer threads do with zlib, one 64 KB block at a time (htslib bgzf_compress,
// deepmutect/htslib/bgzf.c:610-648, from sortmardup/main.cpp:371-421), is done here with one workgroup per
// BGZF block; a batch holds thousands of independent blocks, so the device is filled by blocks, not by the
// inside of one.  Per block, all in LDS (the 64 KB of input, a 4096-entry hash table, the code tables), in the order of
// k_bgzf_deflate's phases (the rules of the format themselves: deflate_rules.h):
//
//   3. literal costs: a sampled byte histogram prices a literal, so that a short match is only taken where it beats the
//      literals it replaces;
//   4. match / parse / tokens, a software pipeline over groups of kGrp windows of kWin positions.  ONE wavefront looks up the
//      hash of every position's 4 bytes, 64 positions per step, and THEN enters them in the table (atomic max: the nearest
//      earlier occurrence wins, so the result does not depend on scheduling); 14 wavefronts extend the candidate -- and the
//      distance-1 candidate, the run-length case of quality strings -- up to 258 bytes, apply the cost rule and one-step lazy
//      evaluation, and so decide the match AT every position; one wavefront finds which positions START a token (lane l walks
//      chunk l of the group, then re-walks from where the chunk before really ends until no start moves); every wavefront
//      turns the starts into packed tokens (dense, in position order, in global memory) and counts their symbols;
//   5. CRC-32: per-thread table-driven CRCs of 64-byte chunks, combined by multiplication with x^(8 * bytes after) modulo
//      the CRC polynomial;
//   6. two length-limited Huffman codes (rank by counting, the merges in rounds across the workgroup, the counts per length
//      repaired as zlib does in the rare case a code comes out longer than 15 bits);
//   7. the run-length coded header of RFC 1951 section 3.2.7 with its own code-length code;
//   8. the size from the symbol counts; a block that would not shrink is emitted stored;
//   9. the tokens are read back a window of 1024 at a time, a scan gives every token its bit offset, and the bits go into the
//      LDS buffer that held the input (OR into 32-bit words).
// A finished block (18-byte BGZF header, payload, CRC, ISIZE) lands in a 64 KB slot; a scan over the sizes and a
// copy kernel pack the slots back to back in pinned host memory.
// The compressor only: the record store that feeds it from HBM is mgx_store.hip, through mgx_bgzf_internal.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "../../include/mgx_bgzf.h"
#include "deflate_rules.h"
#include "mgx_bgzf_internal.h"

using mgx::set_error;
using namespace mgx_deflate;

namespace {

constexpr int kNT = 1024;                       // threads per workgroup (16 wavefronts: one block per CU, LDS-bound)
constexpr u32 kWin = 896;                       // positions per match window: 14 wavefronts decide matches, the 15th parses the previous group, the 16th looks up hash candidates
constexpr u32 kParse0 = kWin, kProd0 = kWin + 64; // first thread of the parsing (wavefront 14) and of the candidate-producing wavefront (15)
constexpr u32 kGrp = 4;                         // match windows per GROUP: 3584 positions = 56 chunks of 64 are matched, parsed and turned into tokens before the next
constexpr u32 kGrpPos = kGrp * kWin, kGrpChunks = kGrpPos / 64;
static_assert(kGrpPos % 64 == 0 && kGrpChunks <= 64, "a group is a whole number of 64-position chunks, one per lane of the parsing wavefront");
constexpr u32 kMaxIn = MGX_BGZF_MAX_BLOCK_IN;
constexpr u32 kSlot = 0x10000;                 // bytes of device scratch per finished block
constexpr u32 kSlotSkew = 2;                   // a block starts at slot + 2: its payload (18 bytes in) is 4-byte aligned
constexpr u32 kPad = 320;                      // zero bytes after the input in LDS (match extension reads ahead)
constexpr u32 kScratchPerWg = 65536u;          // u32 per workgroup: the block's packed tokens, densely, at most one per byte (the only per-block state that leaves the LDS)
static_assert(kMaxIn <= kScratchPerWg, "a token per input byte");

enum { V_OVER = 0, V_NUSED, V_K, V_CRCLAST, V_NTOK, V_NLIT, V_NDIST, V_NCLSYM, V_HDRBITS, V_CRC, V_CARRY, V_N };

struct __attribute__((aligned(16))) Lds {
    u32 buf[(0x10000 + 512) / 4];              // the block's bytes (at the source's alignment), later the output words
    u32 head[1 << kHashBits];                  // hash -> last position + 1
    u32 crc_tab[4][256];                       // slicing-by-4 tables
    u32 x2n[32];                               // x^(2^k) mod P
    u32 tpow[kNT];                             // x^(512 j) mod P
    u32 xr[65];                                // x^(8 r) mod P
    u32 f_ll[288], f_d[32], f_cl[20];          // symbol counts
    u16 c_ll[288], c_d[32], c_cl[20];          // codes, bit-reversed for LSB-first output
    u8 l_ll[288], l_d[32], l_cl[20];           // code lengths
    u16 sorted[288];
    u16 qid[2][288];                           // Huffman rounds: node ids of the active list (two buffers)
    u32 wl[288], wi[288];                      // weights: leaves (sorted), internal nodes (in creation order)
    u16 parent[576];
    u8 depth[576];
    u32 bl_count[16], next_code[16];
    u32 wsum[kNT / 64];
    u64 smask[6];                              // header: which of the (up to 316) code lengths start a run
    u16 cand[2][kGrpPos];                      // hash candidates (position + 1) of the current and the next group
    alignas(16) u32 gm[2][kGrpPos];            // the decided matches of the group being matched and of the one before, len << 16 | dist (0: literal)
    u32 cend[kGrpChunks];                      // parse: the index of the first token of chunk l of the group
    u64 mask[kGrpChunks];                      // parse: the positions of chunk l of the group that start a token
    u32 fw[288];                               // huff_build's working copy of the counts
    u8 bcost[256];                             // estimated cost of a literal byte in 1/16 bit, from the block's byte histogram
    u32 hdr[192];                              // the dynamic block header, as bits
    u16 clsym[320];                            // code-length symbols of the header: symbol | extra << 8
    u32 vars[V_N];
};
static_assert(sizeof(Lds) == 145936, "one workgroup per CU: what the dynamic LDS request is made of");

// Cycles per phase, summed over blocks (MGX_BGZF_PROF=1): a slot per lap, in the order the kernel takes them.  The P_A_ / P_B_
// slots lie inside P_PIPELINE, the P_LL_ slots (the literal/length code's huff_build) inside P_CODES.
enum Prof { P_LOAD = 0, P_PIPELINE, P_CRC, P_CODES, P_HEADER, P_EMIT, P_A_MATCH, P_A_PARSE, P_A_PRODUCE, P_B_TOKENS,
            P_LL_SETUP, P_LL_RANK, P_LL_MERGE, P_LL_DEPTHS, P_LL_ASSIGN, P_N };
constexpr int kProfSlots = 16;
static_assert(P_N <= kProfSlots, "a slot per lap");
struct PhaseClock {           // thread 0's clock: lap(slot) adds the cycles since the last lap
    unsigned long long* prof; long long t;
    __device__ __forceinline__ void start(unsigned long long* p) { prof = p; t = p ? clock64() : 0; }
    __device__ __forceinline__ void lap(int slot) {
        if (prof && threadIdx.x == 0) { const long long now = clock64(); atomicAdd(&prof[slot], (unsigned long long)(now - t)); t = now; }
    }
};

struct DeflateArgs {
    const u8* in;          // uncompressed bytes of the batch
    const u64* off;        // [n_blocks + 1]
    u32 n_blocks;
    u8* slots;             // [n_blocks][kSlot]
    u32* sizes;            // [n_blocks] bytes of the finished block
    u32* scratch;          // [gridDim.x][kScratchPerWg]: the block's tokens
    u32* n_stored;         // counter
    u32 lazy;
    u32 cost_base, cost_rle;    // estimated bits of a match's length + distance codes (distance 1: cost_rle); 0 = take every match
    unsigned long long* prof;   // optional [kProfSlots], indexed by Prof (MGX_BGZF_PROF=1)
};

struct AtomicOr { static __device__ __forceinline__ void or_word(u32* w, u32 v) { atomicOr(w, v); } };
typedef BitSink<AtomicOr> Sink;

__device__ __forceinline__ u32 load32(const u8* p) { u32 v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ u64 load64(const u8* p) { u64 v; __builtin_memcpy(&v, p, 8); return v; }

__device__ __forceinline__ u32 match_len(const u8* a, const u8* b, u32 maxlen) {
    u32 len = 0;
    while (len + 8 <= maxlen) {
        const u64 x = load64(a + len) ^ load64(b + len);
        if (x) return len + (u32)(__builtin_ctzll(x) >> 3);
        len += 8;
    }
    while (len + 4 <= maxlen) {
        const u32 x = load32(a + len) ^ load32(b + len);
        if (x) return len + (__builtin_ctz(x) >> 3);
        len += 4;
    }
    while (len < maxlen && a[len] == b[len]) ++len;
    return len;
}

// Wavefront-wide inclusive scans on the DPP network (row shifts, then the row broadcasts of gfx9): six VALU operations,
// no trip through the LDS crossbar as __shfl_up takes.  Lane 63 ends up with the reduction over the wavefront.
template <typename Op>
__device__ __forceinline__ u32 wave_scan_inclusive(u32 v, Op op) {
    v = op(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));     // row_shr:1
    v = op(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));     // row_shr:2
    v = op(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));     // row_shr:4
    v = op(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));     // row_shr:8
    v = op(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));     // row_bcast:15 into rows 1 and 3
    v = op(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));     // row_bcast:31 into rows 2 and 3
    return v;
}
struct OpAdd { __device__ __forceinline__ u32 operator()(u32 a, u32 b) const { return a + b; } };
struct OpXor { __device__ __forceinline__ u32 operator()(u32 a, u32 b) const { return a ^ b; } };
__device__ __forceinline__ u32 wave_last(u32 v) { return (u32)__builtin_amdgcn_readlane((int)v, 63); }
__device__ __forceinline__ u32 lane_below(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }   // wave_shr:1: lane i reads lane i - 1
__device__ __forceinline__ u32 lane_above(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, false); }   // wave_shl:1: lane i reads lane i + 1

// Workgroup-wide exclusive prefix sum (wave shuffles, then the wave totals through LDS).  *total = sum of all values.
__device__ __forceinline__ u32 block_scan(Lds& L, u32 v, u32* total) {
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 inc = wave_scan_inclusive(v, OpAdd());
    __syncthreads();                                   // earlier readers of L.wsum are done
    if (lane == 63) L.wsum[wave] = inc;
    __syncthreads();
    u32 before = 0, all = 0;
#pragma unroll
    for (u32 w = 0; w < kNT / 64; ++w) { const u32 t = L.wsum[w]; all += t; if (w < wave) before += t; }
    *total = all;
    return before + inc - v;
}

// ---- length-limited Huffman codes ----------------------------------------------------------------------------------------
__device__ __attribute__((noinline)) void limit_lengths_cold(Lds& L, const int n, const int limit, u8* len) { limit_lengths(L.bl_count, L.sorted, n, limit, len); }

// WAVE: one wavefront works alone -- the LDS executes a wavefront's instructions in order, so its lanes need no workgroup barrier
template <bool WAVE>
__device__ __forceinline__ void huff_sync() {
    if constexpr (WAVE) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    else __syncthreads();
}

// Huffman's merges in rounds, over the n leaves ranked in L.wl / L.sorted; leaves L.parent.  The active nodes form one sorted
// list Q.  t = Q[0] + Q[1] is the lightest node that can still be created, so every active node of weight <= t is merged
// before any new node is touched: the (even-sized) prefix of Q up to t pairs up neighbour with neighbour, exactly as the
// sequential algorithm would take them one pair at a time, and the new nodes -- their weights come out sorted -- are merged
// with the rest of Q into the next round's list (positions by binary search, old nodes first on equal weight).
// 12-16 rounds for the 250-280 symbols of a BAM block instead of as many dependent steps on one lane
// (126 k -> 36 k cycles per block; the same code lengths).
template <bool WAVE>
__device__ __forceinline__ void huff_merge_rounds(Lds& L, const int n, const int tid) {
    u32* qw[2] = {L.wl, L.wi};
    u16* qi[2] = {L.qid[0], L.qid[1]};
    if (tid < n) L.qid[0][tid] = (u16)tid;                       // leaves 0 .. n-1 in weight order (the rank step)
    if (tid == 0) L.vars[V_K] = (u32)n;
    huff_sync<WAVE>();
    u32 m = (u32)n, next_id = (u32)n;
    int cur = 0;
    while (m > 1) {
        const u32* w = qw[cur];
        const u32 t = w[0] + w[1];
        if ((u32)tid + 1 < m && w[tid] <= t && w[tid + 1] > t) L.vars[V_K] = (u32)tid + 1;     // at most one thread: Q is sorted
        huff_sync<WAVE>();
        const u32 k = L.vars[V_K] & ~1u, a = m - k, b = k >> 1;
        if ((u32)tid < b) {                                      // new node tid of this round
            const u32 nw = w[2 * tid] + w[2 * tid + 1];
            const u32 id = next_id + (u32)tid;
            L.parent[qi[cur][2 * tid]] = (u16)id; L.parent[qi[cur][2 * tid + 1]] = (u16)id;
            u32 lo = 0, hi = a;                                  // old nodes (Q[k ..)) of weight <= nw go first
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (w[k + mid] <= nw) lo = mid + 1; else hi = mid; }
            qw[cur ^ 1][(u32)tid + lo] = nw; qi[cur ^ 1][(u32)tid + lo] = (u16)id;
        } else if ((u32)tid >= k && (u32)tid < m) {              // old node that stays
            const u32 ow = w[tid];
            u32 lo = 0, hi = b;                                  // new nodes of weight < ow go first
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (w[2 * mid] + w[2 * mid + 1] < ow) lo = mid + 1; else hi = mid; }
            qw[cur ^ 1][((u32)tid - k) + lo] = ow; qi[cur ^ 1][((u32)tid - k) + lo] = qi[cur][tid];
        }
        m = a + b; next_id += b; cur ^= 1;
        huff_sync<WAVE>();
        if (tid == 0) L.vars[V_K] = m;                           // the next round's default: everything is <= t
        huff_sync<WAVE>();
    }
}

// The counts into L.fw (at least two symbols get a code: inflate accepts no incomplete literal/length or code-length code) and the
// used symbols ranked, rarest first and the lower symbol first on equal counts, into L.sorted / L.wl; leaves V_NUSED.
template <bool WAVE>
__device__ __forceinline__ void huff_rank(Lds& L, const u32* freq_in, const int N, u8* len, const int tid, PhaseClock& clk) {
    if (tid < N) L.fw[tid] = freq_in[tid];            // the caller's counts stay as they are (they price the block)
    u32* const freq = L.fw;
    huff_sync<WAVE>();
    const int used = WAVE ? (int)__popcll(__ballot(tid < N && freq[tid] != 0)) : __syncthreads_count(tid < N && freq[tid] != 0);
    if (tid == 0) {
        if (used == 0) { freq[0] = 1; freq[1] = 1; }
        else if (used == 1) freq[freq[0] ? 1 : 0] = 1;
    }
    clk.lap(P_LL_SETUP);
    huff_sync<WAVE>();
    if (tid < 16) L.bl_count[tid] = 0;
    if (tid == 0) { L.vars[V_NUSED] = 0; L.vars[V_OVER] = 0; }
    huff_sync<WAVE>();
    if (tid < N) {
        len[tid] = 0;
        const u32 f = freq[tid];
        if (f) {
            int r = 0;
            for (int j = 0; j < N; ++j) { const u32 g = freq[j]; r += (g != 0) & ((g < f) | ((g == f) & (j < tid))); }
            L.sorted[r] = (u16)tid;
            L.wl[r] = f;
            atomicAdd(&L.vars[V_NUSED], 1u);
        }
    }
    huff_sync<WAVE>();
    clk.lap(P_LL_RANK);
}

// Length-limited Huffman code of freq[0, N): lengths and (bit-reversed) canonical codes.  Called by the whole workgroup.
// Parallel but for the merge rounds: ranks by counting, leaf depths by walking up the parent links, code values by
// counting the earlier symbols of the same length.
// WAVE (N <= 64: the distance and the code-length alphabets): wavefront 0 does it alone and the others wait at the exit.
template <bool WAVE>
__device__ __forceinline__ void huff_build(Lds& L, const u32* freq_in, const int N, const int limit, u8* len, u16* code, unsigned long long* prof = nullptr) {
    const int tid = (int)threadIdx.x;
    PhaseClock clk;
    clk.start(prof);
    __syncthreads();
    if (WAVE && tid >= 64) { __syncthreads(); return; }
    huff_rank<WAVE>(L, freq_in, N, len, tid, clk);
    const int n = (int)L.vars[V_NUSED];
    huff_merge_rounds<WAVE>(L, n, tid);
    huff_sync<WAVE>();
    clk.lap(P_LL_MERGE);
    if (tid < n) {                               // depth of leaf tid: steps to the root (node 2n - 2)
        int d = 0;
        for (int id = tid; id != 2 * n - 2; id = L.parent[id]) ++d;
        if (d > limit) L.vars[V_OVER] = 1;
        len[L.sorted[tid]] = (u8)d;
        atomicAdd(&L.bl_count[d < 16 ? d : 15], 1u);
    }
    huff_sync<WAVE>();
    clk.lap(P_LL_DEPTHS);
    if (L.vars[V_OVER]) {
        if (tid == 0) limit_lengths_cold(L, n, limit, len);
        huff_sync<WAVE>();
    }
    if (tid == 0) canonical_next_code(L.bl_count, L.next_code);
    huff_sync<WAVE>();
    if (tid < N) {
        const u32 l = len[tid];
        u32 c = 0;
        if (l) {
            c = L.next_code[l];
            for (int j = 0; j < tid; ++j) c += (len[j] == l);
            c = reverse_code(c, l);
        }
        code[tid] = (u16)c;
    }
    __syncthreads();
    clk.lap(P_LL_ASSIGN);
}

// ---- the phases of one block, in the order k_bgzf_deflate runs them --------------------------------------------------------
struct Block {            // what the phases share (taken by reference and inlined: it lives in no memory)
    Lds& L;
    const DeflateArgs& a;
    u8* in;               // the block's bytes in L.buf, at the source's word alignment
    u32 n, tid;
    u32* tokd;            // the workgroup's token scratch
};

// 1. once per workgroup: the CRC tables, and the powers of x that shift a chunk's CRC to the end of the block
__device__ __forceinline__ void crc_tables_once(Lds& L, const u32 tid) {
    if (tid < 256) L.crc_tab[0][tid] = crc_table0(tid);
    __syncthreads();
    if (tid < 256) {
        u32 c = L.crc_tab[0][tid];
        for (int k = 1; k < 4; ++k) { c = crc_table_next(c, L.crc_tab[0]); L.crc_tab[k][tid] = c; }
    }
    if (tid == 0) {
        u32 p = kX1;
        L.x2n[0] = p;
        for (int k = 1; k < 32; ++k) { p = multmodp(p, p); L.x2n[k] = p; }
    }
    __syncthreads();
    L.tpow[tid] = x_pow_512(tid, L.x2n);
    if (tid <= 64) L.xr[tid] = x_pow_8(tid, L.x2n);
    __syncthreads();
}

// 2. load (whole words; the bytes around the block are another block's or padding) and clear the block's tables
__device__ __forceinline__ void load_block(const Block& B, const u64 o0) {
    Lds& L = B.L; const u32 tid = B.tid, n = B.n, mis = (u32)(o0 & 3u);
    const u32* src = reinterpret_cast<const u32*>(B.a.in + (o0 - mis));
    const u32 nw = (n + mis + 3) >> 2;
    for (u32 w = tid; w < nw; w += kNT) L.buf[w] = src[w];
    for (u32 i = tid; i < (1u << kHashBits); i += kNT) L.head[i] = 0;
    for (u32 i = tid; i < 288; i += kNT) L.f_ll[i] = 0;
    if (tid < 32) L.f_d[tid] = 0;
    if (tid < 20) L.f_cl[tid] = 0;
    __syncthreads();
    for (u32 i = tid; i < kPad; i += kNT) B.in[n + i] = 0;
}

// 3. byte histogram -> what a literal costs (a match is only worth taking if it beats the literals it replaces: in quality
//    strings of a few distinct values a literal costs 1-2 bits and a short match 15-25); every fourth byte is sample enough
__device__ __forceinline__ void literal_costs(const Block& B) {
    Lds& L = B.L; const u32 tid = B.tid, n = B.n;
    for (u32 i = tid * 4u + ((tid >> 8) & 3u); i < n; i += kNT * 4u) atomicAdd(&L.f_ll[B.in[i]], 1u);
    __syncthreads();
    if (tid < 256) {
        const u32 f = L.f_ll[tid];
        const float bits = f ? 16.0f * __log2f((float)((n + 3) >> 2) / (float)f) : 255.0f;
        L.bcost[tid] = (u8)min(255.0f, bits + 0.5f);
    }
    __syncthreads();
    if (tid < 256) L.f_ll[tid] = 0;
}

// 4a. the producer (wavefront 15): the hash candidates of one window, 64 positions per step.  The LDS executes a wavefront's
// instructions in order, so a step's lookups see every earlier step's entries and none of its own -- candidates are blind to
// the last < 64 bytes only, and the outcome is deterministic.
// (Not force-inlined, and its lane taken as tid & 63: inlined before its own loops are unrolled, or with the lane as tid - kProd0
// -- LDS addresses at negative offsets from a per-thread base --, the kernel's scratch grows from 144 to over 1000 bytes per lane.)
__device__ inline void produce_candidates(const Block& B, const u32 base, u16* cb) {
    static_assert(kProd0 % 64 == 0, "the producer is one whole wavefront");
    Lds& L = B.L; const u32 n = B.n, plane = B.tid & 63u;
    // three passes so that the LDS sees the 14 lookup / insert pairs back to back (its in-order execution is what
    // orders them), instead of a wait for every lookup's result before the next pair is issued
    constexpr int kSteps = (int)kWin / 64;
    u32 h[kSteps], c[kSteps];
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        const u32 p = base + (u32)k * 64u + plane;
        h[k] = p + 4 <= n ? hash4(load32(B.in + p)) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        const u32 p = base + (u32)k * 64u + plane;
        c[k] = 0;
        if (h[k] != 0xFFFFFFFFu) { c[k] = L.head[h[k]]; atomicMax(&L.head[h[k]], p + 1); }
    }
    // (two wavefronts walking the table, each owning the hash values of one parity, give the same candidates but were
    // measured slower: 545 k against 409 k cycles per block for the walk -- it is bound by LDS instructions, not lanes)
#pragma unroll
    for (int k = 0; k < kSteps; ++k) cb[k * 64 + (int)plane] = (u16)c[k];
}
__device__ __forceinline__ void produce_group(const Block& B, const u32 base0, u16* cb) {
    for (u32 g = 0; g < kGrp; ++g) if (base0 + g * kWin < B.n) produce_candidates(B, base0 + g * kWin, cb + g * kWin);
}

// 4b. the match decision of one window (wavefronts 0..13, a position per thread): cand -> gm, len << 16 | dist or 0
__device__ __forceinline__ void decide_window(const Block& B, const u32 base, const u16* cand, u32* gm) {
    Lds& L = B.L; const DeflateArgs& a = B.a; const u8* in = B.in; const u32 tid = B.tid, n = B.n;
    const u32 p = base + tid, lane = tid & 63u;
    u32 len = 0, dist = 0;
    // runs: byte p equals byte p - 1.  The wavefront's 64 flags in one ballot give every lane the length of the
    // distance-1 match at its position (its run of set flags) without a compare loop; only a run that reaches the
    // end of the wavefront's 64 positions is followed further
    const bool run_flag = p >= 1 && p < n && in[p - 1] == in[p];
    const u64 run_mask = __ballot(run_flag);
    // Hash candidates: inside a repeated stretch neighbouring positions point the same distance back, and then the
    // match at p + 1 is the match at p less its first byte.  Only the first lane of such a stretch (and lanes beyond
    // the end of their head's match) extend their candidate; the others take the head's length minus their offset.
    const u32 maxlen = p < n ? min(kMaxMatch, n - p) : 0u;
    u32 cdist = 0;
    if (p < n) { const u32 c = cand[tid]; if (c && p - (c - 1) <= kMaxDist) cdist = p - (c - 1); }
    const u32 prev_dist = lane_below(cdist);
    const bool head = cdist != 0 && (lane == 0 || cdist != prev_dist);
    u32 hlen = 0;
    if (head) hlen = match_len(in + p - cdist, in + p, maxlen);
    const u64 head_mask = __ballot(head);
    const u64 below = head_mask & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
    const u32 head_lane = below ? 63u - (u32)__builtin_clzll(below) : 0u;
    const u32 head_len = (u32)__shfl((int)hlen, (int)head_lane, 64);
    u32 clen = hlen;
    if (cdist != 0 && !head) {
        const u32 off = lane - head_lane;
        clen = head_len > off ? head_len - off : match_len(in + p - cdist, in + p, maxlen);     // past the head's match: on its own
    }
    if (p < n) {
        if (clen >= 4) { len = clen; dist = cdist; }
        if (run_flag && maxlen >= kMinMatch) {
            const u64 rest = ~(run_mask >> lane);
            u32 l = rest ? (u32)__builtin_ctzll(rest) : 64u;              // <= 64 - lane
            if (lane + l == 64u && l < maxlen) l += match_len(in + p - 1 + l, in + p + l, maxlen - l);
            l = min(l, maxlen);
            if (l >= kMinMatch && l >= len) { len = l; dist = 1; }
        }
        if (len && len <= 16 && a.cost_base) {
            const u32 w4 = load32(in + p);
            const u32 lit = short_match_literal_cost(len, L.bcost[w4 & 0xffu], L.bcost[(w4 >> 8) & 0xffu], L.bcost[(w4 >> 16) & 0xffu], L.bcost[w4 >> 24]);
            if (short_match_loses(dist, lit, a.cost_base, a.cost_rle)) len = 0;
        }
    }
    // one-step lazy evaluation: a longer match starting at the next byte (the neighbouring lane's) wins; the decision
    // is a function of the position alone, whatever the parse does around it
    const u32 len_next = lane_above(len);
    if (a.lazy && lane != 63u && len_next > len) len = 0;
    gm[tid] = len ? (len << 16 | dist) : 0u;
}

// 4c. parse (wavefront 14, lane l owns chunk l of the group).  The token AT a position is fixed by the match decision; which
// positions START a token is the chain carry -> carry + len -> ...  First every lane walks its chunk from the chunk's first
// position, in registers, 64 predicated steps: the chunk's token starts, and where its last token ends (chunk-relative).
__device__ __forceinline__ u32 walk_chunk_from_its_start(const u32* gmv, const u32 l, const u32 gcl, u64* mask) {
    u32 m2[32];                                      // the chunk's 64 token lengths (0 = literal), two per register
    if (l < kGrpChunks) {
        const uint4* v = reinterpret_cast<const uint4*>(gmv + l * 64u);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint4 x = v[q];
            m2[2 * q] = (x.x >> 16) | (x.y & 0xffff0000u);
            m2[2 * q + 1] = (x.z >> 16) | (x.w & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 32; ++q) m2[q] = 0;
    }
    u32 next = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i)
        if ((u32)i == next && (u32)i < gcl) { *mask |= 1ull << i; const u32 ln = (i & 1) ? m2[i >> 1] >> 16 : m2[i >> 1] & 0xffffu; next += ln ? ln : 1u; }
    return next;
}
// Then a lane learns where the previous chunk's last token really ends (lane 0: where the previous group's did) and only
// re-walks from there UNTIL THE NEW CHAIN MEETS THE OLD ONE -- two chains through the same jump table coincide from their
// first common position on, a few tokens in on BAM bytes --, reading the lengths from the LDS table; repeated until no
// chunk's start moves.  One wavefront: lane shifts and ballots, no barrier.  Leaves L.mask, L.cend, V_NTOK, V_CARRY.
__device__ __forceinline__ void parse_group(const Block& B, const u32 gbase, const u32* gmv) {
    Lds& L = B.L; const u32 n = B.n;
    const u32 l = B.tid - kParse0;
    const u32 glo = gbase + l * 64u;
    const u32 gcl = (l < kGrpChunks && glo < n) ? min(64u, n - glo) : 0u;
    u64 mask = 0;                                    // token starts of the chunk, from cur_start
    u32 my_end = glo;                                // where the chunk's last token ends (absolute; may pass the chunk)
    const u32 first_end = walk_chunk_from_its_start(gmv, l, gcl, &mask);
    if (gcl) my_end = glo + first_end;
    const u32 carry = L.vars[V_CARRY];
    u32 cur_start = glo;
    for (;;) {
        const u32 up = lane_below(my_end);
        const u32 prev = l == 0 ? carry : up;
        const u32 st = max(glo, prev);
        const bool changed = l < kGrpChunks && st != cur_start;
        if (changed) {
            cur_start = st;
            u32 nx = st - glo;                       // chunk-relative
            u64 add = 0;
            while (nx < gcl && !((mask >> nx) & 1ull)) {
                add |= 1ull << nx;
                const u32 ln = gmv[l * 64u + nx] >> 16;
                nx += ln ? ln : 1u;
            }
            if (nx < gcl) mask = add | (mask & ~((1ull << nx) - 1ull));      // met the old chain: its tail (and its end) stand
            else { mask = add; my_end = glo + nx; }                          // left the chunk first
        }
        if (!__ballot(changed)) break;
    }
    // tokens are stored densely, in position order: a chunk's tokens start at the count of all earlier ones
    const u32 cnt = l < kGrpChunks ? (u32)__builtin_popcountll(mask) : 0u;
    const u32 inc = wave_scan_inclusive(cnt, OpAdd());
    const u32 before = L.vars[V_NTOK];
    if (l < kGrpChunks) { L.mask[l] = mask; L.cend[l] = before + inc - cnt; }            // (group-local: the next group's parse comes after this group's tokens)
    const u32 all = wave_last(inc);
    const u32 last_end = (u32)__builtin_amdgcn_readlane((int)my_end, (int)kGrpChunks - 1);       // ends only grow along the chunks
    if (l == 0) { L.vars[V_NTOK] = before + all; L.vars[V_CARRY] = max(carry, last_end); }
}

// 4d. tokens (every wavefront; needs parse_group of the same group behind a barrier): the group's token starts become packed
// tokens in global memory, their symbols are counted in LDS
__device__ __forceinline__ void tokens_of_group(const Block& B, const u32 gbase, const u32* gmv) {
    Lds& L = B.L;
    for (u32 q = B.tid; q < kGrpPos; q += kNT) {
        const u32 p = gbase + q;
        if (p >= B.n) break;
        const u64 cmask = L.mask[q >> 6];             // (a group starts on a chunk boundary)
        if (!((cmask >> (q & 63u)) & 1ull)) continue;
        const u32 mm = gmv[q];
        const u32 len = mm >> 16;
        u32 t;
        if (len) {
            t = token_match(len, mm & 0xffffu);
            atomicAdd(&L.f_ll[tok_symbol(t)], 1u);
            atomicAdd(&L.f_d[tok_dist_symbol(t)], 1u);
        } else {
            t = B.in[p];
            atomicAdd(&L.f_ll[t], 1u);
        }
        B.tokd[L.cend[q >> 6] + (u32)__builtin_popcountll(cmask & ((1ull << (q & 63u)) - 1ull))] = t;
    }
}

// 4. Software pipeline over groups of kGrp windows (3584 positions = 56 chunks of 64), two workgroup barriers per group:
//   phase A   wavefronts 0..13 decide the matches of group g (into gm[g & 1]) while wavefront 14 PARSES group g - 1 and
//             wavefront 15 looks up the hash candidates of group g + 1 (into cand[(g + 1) & 1]);
//   phase B   every wavefront turns group g - 1's token starts into packed tokens (symbol counts in LDS, the tokens
//             themselves densely to global memory -- the only per-position state that leaves the LDS; round 2 kept a
//             256 KB match table per block in global scratch, written once and read twice: 16 x the algorithmic bytes).
// kGrp windows per barrier: a wavefront that meets long matches in one window catches up in the next ones.
__device__ __forceinline__ void match_parse_tokens(const Block& B) {
    Lds& L = B.L; const DeflateArgs& a = B.a; const u32 tid = B.tid, n = B.n;
    if (tid == 0) { L.vars[V_NTOK] = 0; L.vars[V_CARRY] = 0; }
    __syncthreads();
    if (tid >= kProd0) produce_group(B, 0, L.cand[0]);
    __syncthreads();
    u32 n_groups = 0;
    for (u32 grp = 0, base0 = 0; base0 < n; ++grp, base0 += kGrpPos) {
        n_groups = grp + 1;
        const long long ta0 = a.prof ? clock64() : 0;                                   // ---- phase A
        if (tid >= kProd0) produce_group(B, base0 + kGrpPos, L.cand[(grp + 1) & 1]);
        else if (tid >= kParse0) {
            if (grp) parse_group(B, base0 - kGrpPos, L.gm[(grp - 1) & 1]);
            if (a.prof && tid == kParse0) atomicAdd(&a.prof[P_A_PARSE], (unsigned long long)(clock64() - ta0));
        } else for (u32 g = 0; g < kGrp; ++g) {
            if (base0 + g * kWin >= n) break;
            decide_window(B, base0 + g * kWin, L.cand[grp & 1] + g * kWin, L.gm[grp & 1] + g * kWin);
        }
        if (a.prof && (tid == 0 || tid == kProd0)) atomicAdd(&a.prof[tid ? P_A_PRODUCE : P_A_MATCH], (unsigned long long)(clock64() - ta0));
        __syncthreads();
        const long long tb0 = a.prof ? clock64() : 0;                                   // ---- phase B
        if (grp) tokens_of_group(B, base0 - kGrpPos, L.gm[(grp - 1) & 1]);
        __syncthreads();
        if (a.prof && tid == 0) atomicAdd(&a.prof[P_B_TOKENS], (unsigned long long)(clock64() - tb0));
    }
    if (n_groups) {                                     // the last group's parse and tokens
        const u32 gb = (n_groups - 1) * kGrpPos;
        if (tid >= kParse0 && tid < kProd0) parse_group(B, gb, L.gm[(n_groups - 1) & 1]);
        __syncthreads();
        tokens_of_group(B, gb, L.gm[(n_groups - 1) & 1]);
        __syncthreads();
    }
}

// 5. CRC-32: thread t takes chunk t of 64 bytes and shifts its CRC to the end of the block; leaves V_CRC.  (The end-of-block
// symbol is counted here, ahead of the barrier that phase 6 needs anyway.)
__device__ __forceinline__ void block_crc(const Block& B) {
    Lds& L = B.L; const u32 tid = B.tid, n = B.n;
    const u32 lo = tid * kCrcChunk;
    const u32 cl = lo < n ? min(kCrcChunk, n - lo) : 0u;
    u32 c = crc_chunk_start(tid);
    u32 p = lo;
    for (; p + 4 <= lo + cl; p += 4) c = crc_word(c, load32(B.in + p), &L.crc_tab[0][0]);
    for (; p < lo + cl; ++p) c = crc_byte(c, B.in[p], &L.crc_tab[0][0]);
    const u32 nc = crc_chunks(n);
    const u32 shifted = crc_shifted_chunk(c, tid, nc, L.tpow);
    if (crc_is_last_chunk(tid, nc)) L.vars[V_CRCLAST] = c;
    const u32 part = wave_last(wave_scan_inclusive(shifted, OpXor()));
    if ((tid & 63u) == 0) L.wsum[tid >> 6] = part;
    if (tid == 0) L.f_ll[kEndOfBlock] = 1;
    __syncthreads();
    if (tid == 0) {
        u32 x = 0;
        for (int i = 0; i < kNT / 64; ++i) x ^= L.wsum[i];
        L.vars[V_CRC] = crc_finish(x, L.vars[V_CRCLAST], n, L.xr);
    }
}

// 7a. the header's code-length symbols (RFC 1951 3.2.7), in parallel: the nlit + ndist code lengths are cut into runs
// (ballots), every run knows how many code-length symbols it becomes (run_symbol_count), a scan places them.
// Leaves L.clsym, L.f_cl, V_NLIT, V_NDIST, V_NCLSYM and a cleared L.hdr.
__device__ __forceinline__ void header_symbols(const Block& B) {
    Lds& L = B.L; const u32 tid = B.tid;
    if (tid == 0) { L.vars[V_NLIT] = 257; L.vars[V_NDIST] = 1; }
    for (u32 i = tid; i < 192; i += kNT) L.hdr[i] = 0;
    __syncthreads();
    if (tid < (u32)kNumLL && L.l_ll[tid]) atomicMax(&L.vars[V_NLIT], tid + 1);
    if (tid < (u32)kNumD && L.l_d[tid]) atomicMax(&L.vars[V_NDIST], tid + 1);
    __syncthreads();
    const u32 nlit = L.vars[V_NLIT], total = nlit + L.vars[V_NDIST];
    auto length_at = [&](u32 i) -> u32 { return i < nlit ? L.l_ll[i] : L.l_d[i - nlit]; };
    const u32 v = tid < total ? length_at(tid) : 0xFFu;
    const bool start = tid < total && (tid == 0 || length_at(tid - 1) != v);
    const u64 bal = __ballot(start);
    if ((tid & 63u) == 0 && tid < 384) L.smask[tid >> 6] = bal;
    __syncthreads();
    u32 cnt = 0, run = 0;
    if (start) {                                            // the run ends where the next one starts
        u32 next = total;
        const u32 wv = tid >> 6, ln = tid & 63u;
        const u64 rest = ln == 63 ? 0ull : (L.smask[wv] >> (ln + 1));
        if (rest) next = tid + 1 + (u32)__builtin_ctzll(rest);
        else for (u32 w = wv + 1; w < 6; ++w) { const u64 mk = L.smask[w]; if (mk) { next = w * 64 + (u32)__builtin_ctzll(mk); break; } }
        if (next > total) next = total;
        run = next - tid;
        cnt = run_symbol_count(v, run);
    }
    u32 ns;
    u32 at = block_scan(L, cnt, &ns);
    if (start) run_symbols(v, run, [&](u32 sym, u32 extra) { L.clsym[at++] = (u16)(sym | extra << 8); atomicAdd(&L.f_cl[sym], 1u); });
    if (tid == 0) L.vars[V_NCLSYM] = ns;
}

// 7b. the header's bits into L.hdr: thread 0 writes the fixed part, then a scan gives every code-length symbol its bit
// offset behind it.  Leaves V_HDRBITS.
__device__ __forceinline__ void header_bits(const Block& B) {
    Lds& L = B.L; const u32 tid = B.tid;
    if (tid == 0) {
        Sink s;
        s.start(L.hdr, 0);
        put_dynamic_header_start(s, L.vars[V_NLIT], L.vars[V_NDIST], L.l_cl);
        L.vars[V_HDRBITS] = s.position();                   // so far; the code-length symbols follow
        s.finish();
    }
    __syncthreads();
    const u32 ns = L.vars[V_NCLSYM], fixed_bits = L.vars[V_HDRBITS];
    u32 sym = 0, extra = 0, nb = 0;
    if (tid < ns) {
        sym = L.clsym[tid] & 0xffu; extra = L.clsym[tid] >> 8;
        nb = L.l_cl[sym] + cl_extra_bits(sym);
    }
    u32 sym_bits;
    const u32 off = block_scan(L, nb, &sym_bits);
    if (tid < ns) {
        Sink s;
        s.start(L.hdr, fixed_bits + off);
        put_cl_symbol(s, sym, extra, L.c_cl, L.l_cl);
        s.finish();
    }
    __syncthreads();
    if (tid == 0) L.vars[V_HDRBITS] = fixed_bits + sym_bits;
    __syncthreads();
}

// 8. the bits of the tokens, from the symbol counts (the end-of-block symbol included)
__device__ __forceinline__ u32 token_bits_total(const Block& B) {
    Lds& L = B.L; const u32 tid = B.tid;
    u32 sym_bits = 0;
    if (tid < (u32)kNumLL) sym_bits = L.f_ll[tid] * (L.l_ll[tid] + (tid > kEndOfBlock ? length_extra_bits(tid) : 0u));
    else if (tid >= 512 && tid < 512u + kNumD) sym_bits = L.f_d[tid - 512] * (L.l_d[tid - 512] + dist_extra_bits(tid - 512));
    u32 total;
    (void)block_scan(L, sym_bits, &total);
    return total;
}

// 9a. a dynamic block: header and tokens as bits into L.buf (every reader of the input bytes is done), then out to `pay`.
// The tokens are read ONCE, a window of 1024 at a time: a window's bit offsets are the bits of the earlier windows (carried in
// a register) plus a workgroup scan of its own tokens' sizes; the next window's tokens (one window, tnext) are already in
// flight during the scan.  (Round 2 read the token list twice: once for the sizes, once for the bits.)
__device__ __forceinline__ void emit_dynamic(const Block& B, const u32 payload, const u32 hdr_bits, const u32 n_tok, u8* pay) {
    Lds& L = B.L; const u32 tid = B.tid; const u32* tokd = B.tokd;
    const u32 nw = (payload + 3) >> 2;
    for (u32 w = tid; w < nw; w += kNT) L.buf[w] = 0;
    __syncthreads();
    for (u32 w = tid; w < ((hdr_bits + 31) >> 5); w += kNT) atomicOr(&L.buf[w], L.hdr[w]);
    const u32 n_tw = (n_tok + kNT - 1) / kNT;
    u32 all_bits = 0;
    u32 tnext = tid < n_tok ? tokd[tid] : kTokNone;
    for (u32 w = 0; w < n_tw; ++w) {
        const u32 t = tnext;
        const u32 inext = (w + 1) * kNT + tid;
        tnext = inext < n_tok ? tokd[inext] : kTokNone;
        const u32 nb = token_bits(t, L.l_ll, L.l_d);
        u32 win_bits;
        const u32 off = block_scan(L, nb, &win_bits);
        if (nb) {
            Sink s;
            s.start(L.buf, hdr_bits + all_bits + off);
            put_token(s, t, L.c_ll, L.l_ll, L.c_d, L.l_d);
            s.finish();
        }
        all_bits += win_bits;
    }
    if (tid == 0) { Sink s; s.start(L.buf, hdr_bits + all_bits); s.put(L.c_ll[kEndOfBlock], L.l_ll[kEndOfBlock]); s.finish(); }
    __syncthreads();
    u32* payw = reinterpret_cast<u32*>(pay);
    for (u32 w = tid; w < (payload >> 2); w += kNT) payw[w] = L.buf[w];
    if (tid == 0) {
        const u8* ob = reinterpret_cast<const u8*>(L.buf);
        for (u32 i = payload & ~3u; i < payload; ++i) pay[i] = ob[i];
    }
}

// 9b. a stored block: five bytes and the input
__device__ __forceinline__ void emit_stored_block(const Block& B, u8* pay) {
    if (B.tid == 0) { write_stored_header(pay, B.n); atomicAdd(B.a.n_stored, 1u); }
    for (u32 i = B.tid; i < B.n; i += kNT) pay[kStoredHeader + i] = B.in[i];
}

__global__ __launch_bounds__(kNT) void k_bgzf_deflate(DeflateArgs a) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    Lds& L = *reinterpret_cast<Lds*>(smem);
    const u32 tid = threadIdx.x;
    crc_tables_once(L, tid);                                                            // 1
    for (u32 blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const u64 o0 = a.off[blk];
        const Block B{L, a, reinterpret_cast<u8*>(L.buf) + (u32)(o0 & 3u), (u32)(a.off[blk + 1] - o0), tid, a.scratch + (size_t)blockIdx.x * kScratchPerWg};
        const u32 n = B.n;
        PhaseClock clk;
        clk.start(a.prof);
        load_block(B, o0);                                                              // 2
        literal_costs(B);                                                               // 3
        clk.lap(P_LOAD);
        match_parse_tokens(B);                                                          // 4
        clk.lap(P_PIPELINE);
        block_crc(B);                                                                   // 5
        clk.lap(P_CRC);
        const u32 n_tok = L.vars[V_NTOK];
        huff_build<false>(L, L.f_ll, kNumLL, 15, L.l_ll, L.c_ll, a.prof);                // 6
        huff_build<true>(L, L.f_d, kNumD, 15, L.l_d, L.c_d);
        clk.lap(P_CODES);
        header_symbols(B);                                                              // 7
        huff_build<true>(L, L.f_cl, kNumCL, 7, L.l_cl, L.c_cl);
        header_bits(B);
        clk.lap(P_HEADER);
        const u32 token_total = token_bits_total(B);                                    // 8
        const u32 hdr_bits = L.vars[V_HDRBITS];
        u32 payload = (hdr_bits + token_total + 7) >> 3;
        const bool stored = emit_stored(payload, n);
        u8* const slot = a.slots + (size_t)blk * kSlot + kSlotSkew;
        u8* const pay = slot + kMemberHeader;
        __syncthreads();                                    // every reader of the input bytes is done
        if (!stored) emit_dynamic(B, payload, hdr_bits, n_tok, pay);                    // 9
        else { payload = n + kStoredHeader; emit_stored_block(B, pay); }
        if (tid == 0) a.sizes[blk] = write_member_frame(slot, payload, L.vars[V_CRC], n);  // 10
        __syncthreads();                                    // LDS is reused by the next block
        clk.lap(P_EMIT);
    }
}

// exclusive prefix sum of the block sizes (one workgroup; a batch has a few thousand blocks)
__global__ __launch_bounds__(256) void k_bgzf_offsets(const u32* sizes, u32 n, u64* out_off) {
    __shared__ u64 part[256];
    const u32 tid = threadIdx.x;
    const u32 per = (n + 255) / 256;
    const u32 lo = min(n, tid * per), hi = min(n, lo + per);
    u64 s = 0;
    for (u32 i = lo; i < hi; ++i) s += sizes[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { u64 run = 0; for (int i = 0; i < 256; ++i) { const u64 v = part[i]; part[i] = run; run += v; } out_off[n] = run; }
    __syncthreads();
    u64 run = part[tid];
    for (u32 i = lo; i < hi; ++i) { out_off[i] = run; run += sizes[i]; }
}

// slot -> its place in the packed output (pinned host memory: the stores cross PCIe).  A bounded grid of small workgroups
// walks the blocks: a workgroup per block would fill every CU's wavefront slots with stores waiting on the link and keep the
// next batch's 1024-thread deflate workgroups from being placed.
__global__ __launch_bounds__(256) void k_bgzf_pack(const u8* slots, const u32* sizes, const u64* out_off, u8* out, u32 n_blocks) {
    for (u32 blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const u8* src = slots + (size_t)blk * kSlot + kSlotSkew;
        u8* dst = out + out_off[blk];
        const u32 n = sizes[blk];
        // destination-aligned words, source read with whatever alignment it has
        const u32 lead = min(n, (u32)((4u - ((uintptr_t)dst & 3u)) & 3u));
        if (threadIdx.x < lead) dst[threadIdx.x] = src[threadIdx.x];
        const u32 nw = (n - lead) >> 2;
        u32* dw = reinterpret_cast<u32*>(dst + lead);
        const u8* sb = src + lead;
        for (u32 w = threadIdx.x; w < nw; w += 256) dw[w] = load32(sb + 4 * (size_t)w);
        const u32 done = lead + 4 * nw;
        if (threadIdx.x < n - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
    }
}

// ---- host: the checks that more than one entry point makes ------------------------------------------------------------------
// offsets[first .. first + count] cut pieces of at most kMaxIn bytes
int check_block_range(const u64* offsets, u64 first, u64 count) {
    for (u64 i = first; i < first + count; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > kMaxIn) {
            set_error("block %llu: [%llu, %llu) is not a piece of at most %u bytes", (unsigned long long)i, (unsigned long long)offsets[i], (unsigned long long)offsets[i + 1], kMaxIn);
            return -EINVAL;
        }
    }
    return 0;
}

// ---- host: the steps of a batch's submit --------------------------------------------------------------------------------------
int validate_batch(const mgx_bgzf_batch_t* b, u32 n_blocks) {
    if (n_blocks > b->max_blocks) { set_error("%u blocks in a batch made for %u", n_blocks, b->max_blocks); return -EINVAL; }
    if (b->h_off[0] != 0) { set_error("offsets[0] must be 0"); return -EINVAL; }
    if (const int rc = check_block_range(b->h_off, 0, n_blocks)) return rc;
    if (b->h_off[n_blocks] > b->in_cap) { set_error("%llu input bytes in a batch made for %llu", (unsigned long long)b->h_off[n_blocks], (unsigned long long)b->in_cap); return -EINVAL; }
    return 0;
}

int upload_batch(mgx_bgzf_t* c, mgx_bgzf_batch_t* b, bool input_resident) {
    if (!input_resident) {
        // the input goes up on its own stream: on the kernel stream it would wait for the deflate kernels of the batches
        // submitted before (d_in was last read by this batch's previous kernels, which its last wait() has seen finish)
        HIP_TRY(hipMemcpyAsync(b->d_in, b->h_in, b->n_in, hipMemcpyHostToDevice, c->up));
        HIP_TRY(hipEventRecord(b->ev_in, c->up));
        HIP_TRY(hipStreamWaitEvent(c->stream, b->ev_in, 0));
    }
    HIP_TRY(hipMemcpyAsync(b->d_off, b->h_off, ((size_t)b->n_blocks + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    return 0;
}

int launch_deflate(mgx_bgzf_t* c, mgx_bgzf_batch_t* b) {
    DeflateArgs a{};
    a.in = b->d_in; a.off = b->d_off; a.n_blocks = b->n_blocks; a.slots = b->d_slots; a.sizes = b->d_sizes;
    a.scratch = c->d_scratch; a.n_stored = c->d_n_stored; a.lazy = c->lazy; a.cost_base = c->cost_base; a.cost_rle = c->cost_rle; a.prof = c->d_prof;
    HIP_TRY(hipEventRecord(b->ev_k0, c->stream));
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(std::min(c->grid, b->n_blocks)), dim3(kNT), sizeof(Lds), c->stream, a);
    HIP_TRY(hipEventRecord(b->ev_k1, c->stream));
    return 0;
}

// The finished blocks are packed STRAIGHT INTO THE PINNED OUTPUT BUFFER by the pack kernel, on the copy stream behind this
// batch's deflate kernel only: no packed copy in HBM and no device-to-host copy behind it (round 2's was carried out by
// a blit kernel that took 4.3 ms beside the next batch's deflate kernel and slowed that one from 3.0 to 4.1 ms:
// 20 GB/s pinned to pinned; tools trace in profiles/r03_bgzf_pipeline_trace.txt), and the next batch's deflate kernel
// does not queue behind the packing.
int launch_pack(mgx_bgzf_t* c, mgx_bgzf_batch_t* b) {
    HIP_TRY(hipStreamWaitEvent(c->copy, b->ev_k1, 0));
    HIP_TRY(hipEventRecord(b->ev_p0, c->copy));
    hipLaunchKernelGGL(k_bgzf_offsets, dim3(1), dim3(256), 0, c->copy, b->d_sizes, b->n_blocks, b->d_out_off);
    hipLaunchKernelGGL(k_bgzf_pack, dim3(std::min<u32>(b->n_blocks, (u32)c->n_cu)), dim3(256), 0, c->copy, b->d_slots, b->d_sizes, b->d_out_off, b->h_out_dev, b->n_blocks);
    HIP_TRY(hipGetLastError());
    return 0;
}

int read_back_offsets(mgx_bgzf_t* c, mgx_bgzf_batch_t* b) {
    HIP_TRY(hipMemcpyAsync(b->h_out_off, b->d_out_off, ((size_t)b->n_blocks + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->copy));
    HIP_TRY(hipEventRecord(b->ev_out, c->copy));
    return 0;
}

}  // namespace

// ---- what the record store shares with the C ABI below (mgx_bgzf_internal.h) ----------------------------------------
int mgx_internal::bgzf_batch_create(mgx_bgzf_t* c, uint64_t in_capacity, uint32_t max_blocks, bool pinned_input, mgx_bgzf_batch_t** out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = nullptr;
    if (max_blocks == 0) { set_error("max_blocks is 0"); return -EINVAL; }
    in_capacity = std::min<u64>(in_capacity, (u64)max_blocks * kMaxIn);
    if (const int prc = mgx_bgzf_prepare(c)) return prc;
    HIP_TRY(hipSetDevice(c->device));
    mgx_bgzf_batch* b = new (std::nothrow) mgx_bgzf_batch;
    if (!b) { set_error("out of memory"); return -ENOMEM; }
    b->in_cap = in_capacity; b->max_blocks = max_blocks;
    b->out_cap = mgx_bgzf_bound(in_capacity, max_blocks);
    const size_t off_bytes = ((size_t)max_blocks + 1) * sizeof(u64);
    mgx_hip::Owner& m = b->own;
    if (pinned_input) m.pin(&b->h_in, in_capacity + 8);
    m.pin(&b->h_off, off_bytes); m.pin(&b->h_out, b->out_cap); m.pin(&b->h_out_off, off_bytes);
    m.device(&b->d_in, in_capacity + 8); m.device(&b->d_off, off_bytes); m.device(&b->d_slots, (size_t)max_blocks * kSlot);
    m.device(&b->d_sizes, (size_t)max_blocks * sizeof(u32)); m.device(&b->d_out_off, off_bytes);
    if (m.ok()) m.note(hipHostGetDevicePointer((void**)&b->h_out_dev, b->h_out, 0), "hipHostGetDevicePointer");
    m.event(&b->ev_k0); m.event(&b->ev_k1); m.event(&b->ev_p0); m.event(&b->ev_out); m.event(&b->ev_in, hipEventDisableTiming);
    if (!m.ok()) {
        set_error("%s failed for a batch of %llu bytes / %u blocks", m.failed, (unsigned long long)in_capacity, max_blocks);
        mgx_bgzf_batch_destroy(c, b);
        return -ENOMEM;
    }
    b->h_off[0] = 0;
    *out = b;
    return 0;
}

// input_resident: the batch's device input buffer was filled by a kernel on the context's stream (the record store)
int mgx_internal::bgzf_batch_submit(mgx_bgzf_t* c, mgx_bgzf_batch_t* b, uint32_t n_blocks, bool input_resident) {
    if (!c || !b) { set_error("NULL argument"); return -EINVAL; }
    if (const int rc = validate_batch(b, n_blocks)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    b->n_blocks = n_blocks; b->n_in = b->h_off[n_blocks]; b->submitted = true;
    if (n_blocks == 0) { b->h_out_off[0] = 0; return 0; }
    if (const int rc = upload_batch(c, b, input_resident)) return rc;
    if (const int rc = launch_deflate(c, b)) return rc;
    if (const int rc = launch_pack(c, b)) return rc;
    return read_back_offsets(c, b);
}

extern "C" {

uint64_t mgx_bgzf_bound(uint64_t n_bytes, uint64_t n_blocks) { return n_bytes + 31 * n_blocks; }

int mgx_bgzf_create(int device, unsigned flags, mgx_bgzf_t** out) {
    if (!out) { set_error("out is NULL"); return -EINVAL; }
    *out = nullptr;
    if (const int rc = mgx_hip::pick_device(&device, nullptr, true)) return rc;      // every negative ordinal: device 0
    std::unique_ptr<mgx_bgzf> c(new (std::nothrow) mgx_bgzf);
    if (!c) { set_error("out of memory"); return -ENOMEM; }
    c->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount;
    c->lazy = (flags & 1u) ? 0 : 1;
    if (const char* e = getenv("MGX_BGZF_LAZY")) c->lazy = atoi(e) != 0;
    if (const char* e = getenv("MGX_BGZF_COST_BASE")) c->cost_base = (u32)atoi(e);
    if (const char* e = getenv("MGX_BGZF_COST_RLE")) c->cost_rle = (u32)atoi(e);
    c->own.stream(&c->stream); c->own.stream(&c->copy); c->own.stream(&c->up);
    if (!c->own.ok()) return c->own.error("a BGZF context");
    // one workgroup per CU (157 KB of LDS, 1024 threads x 128 registers: a CU that runs one has no register left for anything
    // else, so the pack kernel of the batch before cannot run BESIDE a deflate kernel, only between two).  Leaving 8 or 16 CUs
    // free for it was measured: the deflate kernel then takes 9 rounds instead of 8 over a 2048-block batch (3.39 against
    // 3.04 ms) and pinned -> pinned falls from 28.0 to 24.1 GB/s.
    c->grid = (u32)c->n_cu;
    if (const char* e = getenv("MGX_BGZF_GRID")) { const int v = atoi(e); if (v > 0) c->grid = (u32)v; }
    // the compressor's own device state (scratch tables, counters, the kernel's LDS attribute -- which loads the code
    // object) is set up by the first batch or by mgx_bgzf_prepare: a record store needs none of it, and a tool that
    // creates the context while it parses its first input should not wait for it
    *out = c.release();
    return 0;
}

int mgx_bgzf_prepare(mgx_bgzf_t* c) {
    if (!c) { set_error("NULL argument"); return -EINVAL; }
    std::lock_guard<std::mutex> g(c->prep_mu);
    if (c->prepared) return 0;
    HIP_TRY(hipSetDevice(c->device));
    mgx_hip::Owner& m = c->own;
    const char* prof = getenv("MGX_BGZF_PROF");
    m.device(&c->d_scratch, (size_t)c->grid * kScratchPerWg * sizeof(u32));
    m.device(&c->d_n_stored, sizeof(u32));
    if (prof && atoi(prof)) m.device(&c->d_prof, kProfSlots * sizeof(unsigned long long));
    if (!m.ok()) { c->d_n_stored = nullptr; return m.error("the compressor's scratch"); }
    HIP_TRY(hipMemsetAsync(c->d_n_stored, 0, sizeof(u32), c->stream));
    if (c->d_prof) HIP_TRY(hipMemsetAsync(c->d_prof, 0, kProfSlots * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipFuncSetAttribute((const void*)k_bgzf_deflate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Lds)));
    c->prepared = true;
    return 0;
}

int mgx_bgzf_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
    if (!free_bytes || !total_bytes) { set_error("NULL argument"); return -EINVAL; }
    if (const int rc = mgx_hip::pick_device(&device, nullptr, true)) return rc;      // every negative ordinal: device 0
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    *free_bytes = f; *total_bytes = t;
    return 0;
}

void mgx_bgzf_destroy(mgx_bgzf_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->copy); (void)hipStreamSynchronize(c->up);
    if (c->d_prof) {
        unsigned long long p[kProfSlots];
        if (hipMemcpy(p, c->d_prof, sizeof p, hipMemcpyDeviceToHost) == hipSuccess && c->n_blocks) {
            for (int i = 0; i < P_N; ++i) p[i] /= c->n_blocks;
            fprintf(stderr, "mgx_bgzf cycles per block: load + literal costs %llu, match/parse/tokens pipeline %llu, crc %llu, literal/length + distance codes %llu, header %llu, size + emit %llu\n",
                    p[P_LOAD], p[P_PIPELINE], p[P_CRC], p[P_CODES], p[P_HEADER], p[P_EMIT]);
            fprintf(stderr, "   inside the pipeline: phase A as wavefront 0 sees it (match decisions) %llu, as wavefront 14 (parse alone) %llu, as wavefront 15 (hash candidates) %llu; phase B (tokens) %llu\n",
                    p[P_A_MATCH], p[P_A_PARSE], p[P_A_PRODUCE], p[P_B_TOKENS]);
            fprintf(stderr, "   literal/length code: setup %llu, rank %llu, merge rounds %llu, depths %llu, limit + code values %llu\n", p[P_LL_SETUP], p[P_LL_RANK], p[P_LL_MERGE], p[P_LL_DEPTHS], p[P_LL_ASSIGN]);
        }
    }
    delete c;
}

void mgx_bgzf_batch_destroy(mgx_bgzf_t* c, mgx_bgzf_batch_t* b) {
    if (!b) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->up); (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->copy); }
    delete b;                                          // its owner frees
}

int mgx_bgzf_batch_create(mgx_bgzf_t* c, uint64_t in_capacity, uint32_t max_blocks, mgx_bgzf_batch_t** out) {
    return mgx_internal::bgzf_batch_create(c, in_capacity, max_blocks, true, out);
}

uint8_t* mgx_bgzf_batch_input(mgx_bgzf_batch_t* b) { return b ? b->h_in : nullptr; }
uint64_t* mgx_bgzf_batch_offsets(mgx_bgzf_batch_t* b) { return b ? b->h_off : nullptr; }

int mgx_bgzf_batch_submit(mgx_bgzf_t* c, mgx_bgzf_batch_t* b, uint32_t n_blocks) { return mgx_internal::bgzf_batch_submit(c, b, n_blocks, false); }

int mgx_bgzf_batch_wait(mgx_bgzf_t* c, mgx_bgzf_batch_t* b, const uint8_t** out, const uint64_t** out_offsets) {
    if (!c || !b || !out || !out_offsets) { set_error("NULL argument"); return -EINVAL; }
    if (!b->submitted) { set_error("batch was not submitted"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    *out = b->h_out; *out_offsets = b->h_out_off;
    b->submitted = false;
    if (b->n_blocks == 0) return 0;
    HIP_TRY(hipEventSynchronize(b->ev_out));
    const u64 total = b->h_out_off[b->n_blocks];
    if (total > b->out_cap) { set_error("internal: %llu output bytes exceed the bound %llu", (unsigned long long)total, (unsigned long long)b->out_cap); return -EIO; }
    float ms = 0, ms_pack = 0;
    if (hipEventElapsedTime(&ms, b->ev_k0, b->ev_k1) == hipSuccess && hipEventElapsedTime(&ms_pack, b->ev_p0, b->ev_out) == hipSuccess)
    { c->ms_kernels = ms; c->ms_pack = ms_pack; }     // the deflate kernel | offsets + pack (its stores cross PCIe) + offsets read-back on the copy stream
    c->n_blocks += b->n_blocks; c->bytes_in += b->n_in; c->bytes_out += total;
    return 0;
}

int mgx_bgzf_compress(mgx_bgzf_t* c, const uint8_t* in, const uint64_t* offsets, uint64_t n_blocks, uint8_t* out,
                      uint64_t out_capacity, uint64_t* out_offsets) {
    if (!c || !offsets || !out_offsets || (n_blocks && (!in || !out))) { set_error("NULL argument"); return -EINVAL; }
    const u64 base = offsets[0];
    const u64 n_bytes = offsets[n_blocks] - base;
    if (out_capacity < mgx_bgzf_bound(n_bytes, n_blocks)) { set_error("output capacity %llu is below mgx_bgzf_bound = %llu", (unsigned long long)out_capacity, (unsigned long long)mgx_bgzf_bound(n_bytes, n_blocks)); return -EINVAL; }
    out_offsets[0] = 0;
    if (n_blocks == 0) return 0;
    constexpr u32 kPer = 1024;                  // blocks per internal batch (64 MB)
    const u32 per = (u32)std::min<u64>(kPer, n_blocks);
    mgx_bgzf_batch_t* bt[2] = {nullptr, nullptr};
    int rc = 0;
    for (int i = 0; i < 2 && !rc; ++i) rc = mgx_bgzf_batch_create(c, (u64)per * kMaxIn, per, &bt[i]);
    u64 done_out = 0;
    struct Flight { u64 first, count; };
    Flight fl[2] = {{0, 0}, {0, 0}};
    auto drain = [&](int k) -> int {
        if (!fl[k].count) return 0;
        const uint8_t* o; const uint64_t* oo;
        const int r = mgx_bgzf_batch_wait(c, bt[k], &o, &oo);
        if (r) return r;
        memcpy(out + done_out, o, oo[fl[k].count]);
        for (u64 i = 0; i < fl[k].count; ++i) out_offsets[fl[k].first + i + 1] = done_out + oo[i + 1];
        done_out += oo[fl[k].count];
        fl[k].count = 0;
        return 0;
    };
    int k = 0;
    for (u64 first = 0; first < n_blocks && !rc; first += per, k ^= 1) {
        rc = drain(k);
        if (rc) break;
        const u64 cnt = std::min<u64>(per, n_blocks - first);
        rc = check_block_range(offsets, first, cnt);        // before the copy below trusts the offsets
        if (rc) break;
        const u64 b0 = offsets[first], b1 = offsets[first + cnt];
        memcpy(bt[k]->h_in, in + b0, b1 - b0);
        for (u64 i = 0; i <= cnt; ++i) bt[k]->h_off[i] = offsets[first + i] - b0;
        rc = mgx_bgzf_batch_submit(c, bt[k], (u32)cnt);
        if (!rc) fl[k] = {first, cnt};
    }
    if (!rc) rc = drain(k);
    if (!rc) rc = drain(k ^ 1);
    for (int i = 0; i < 2; ++i) mgx_bgzf_batch_destroy(c, bt[i]);
    return rc;
}

int mgx_bgzf_stats(mgx_bgzf_t* c, mgx_bgzf_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    u32 ns = 0;
    if (c->d_n_stored) HIP_TRY(hipMemcpy(&ns, c->d_n_stored, sizeof ns, hipMemcpyDeviceToHost));
    out->n_blocks = c->n_blocks; out->bytes_in = c->bytes_in; out->bytes_out = c->bytes_out; out->n_stored = ns; out->ms_kernels = c->ms_kernels; out->ms_pack = c->ms_pack;
    return 0;
}

}  // extern "C"
