// mgx_sortdedup.hip -- device half of the sort / mark-duplicate path for MI355X (gfx950).
//
// Re-expresses sortmardup/main.cpp:235-388 (three per-partition std::sort/std::stable_sort calls,
// two run scans, two bitmaps) as an HBM-bound pipeline over packed 32-byte records:
//
//   build      records -> coordinate keys, compacted double-pair / single-pair entries
//              (pair.cpp:51-108 key rules) + indicator bits (main.cpp:181-192) + key maxima
//   radix      stable LSD radix sort, 8-bit digits, 4096-key tiles: per-tile histogram ->
//              column-wise scan -> ranked scatter through LDS (used for: doubles by mate 5' end,
//              doubles by sort_key, singles by sort_key, records by unified coordinate)
//   best-of-run  every run of equal keys keeps its best entry (score desc, tile/x/y asc, arrival
//              asc), the rest are duplicates (main.cpp:269-280, 319-340); singles additionally
//              test the indicator bitmap
//
// No collective and no host round trip inside the pipeline except one 640-byte read-back of the
// entry counts and key maxima (they size the sorts and pick the number of digit passes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <cerrno>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/mgx_sortdedup.h"
#include "mgx_hip_util.h"      // HIP_TRY
#include "sortdedup_stage.h"

using mgx::set_error;

namespace {

using u64 = unsigned long long;   // == uint64_t on this ABI; the type HIP atomics are declared for
using u32 = uint32_t;

constexpr int kScatterWaves = 4;                      // wavefronts per scatter workgroup
constexpr int kTileThreads = 256;
constexpr int kItems = 16;
constexpr int kTile = kTileThreads * kItems;          // 4096 keys per workgroup
constexpr int kChunkTiles = 128;                      // tiles per column-scan chunk
constexpr u32 kIgnorable = 0x4 | 0x100 | 0x800;
constexpr int kWalkCap = 64;                          // longest run a single lane walks

// Device-side scalars, one small read-back.  Every workgroup of the build kernel bumps the entry
// counters, so each one sits in its own 128-byte line (atomics on one line serialise at ~90/us and
// would otherwise also stall the plain reads of the maxima next to them).
struct Scalars {
    u64 max_coord, max_k1d, max_k2d, max_k1s, max_near;      // consecutive: the build kernel settles them as one array
    u32 n_long_d, n_long_s, n_long_n, n_dup;
    u32 bad_mate;                              // a record names a mate index outside the shard
    u32 pad0_[17];
    alignas(128) u32 n_double; u32 pad1_[31];  // "far" double pairs (two-word keys)
    alignas(128) u32 n_single; u32 pad2_[31];
    alignas(128) u32 n_near;   u32 pad3_[31];
    alignas(128) u32 n_multi_d; u32 n_multi_s, n_multi_n;                   // run heads with more than one entry
    u32 huge_runs; u32 pad4_[28];            // a position holds more near pairs than the in-run comparison accepts
};
static_assert(offsetof(Scalars, max_k1d) == offsetof(Scalars, max_coord) + 8 && offsetof(Scalars, max_k2d) == offsetof(Scalars, max_coord) + 16 &&
              offsetof(Scalars, max_k1s) == offsetof(Scalars, max_coord) + 24 && offsetof(Scalars, max_near) == offsetof(Scalars, max_coord) + 32,
              "k_build_emit settles the five maxima as the array max_coord[0 .. 5)");
// near pair: mate 5' end less than kNearSpan beyond record 1's (every proper pair; insert sizes are a
// few hundred bases).  14 delta bits + 2 orientation bits + a 32-bit position = 48 key bits: six
// 8-bit passes (a 16-bit delta would cost a seventh).
constexpr int kNearDeltaBits = 14;
constexpr u64 kNearSpan = 1ull << kNearDeltaBits;
// The identity occupies the upper 48 bits of the key word and only those are sorted; the 16 bits
// below ride along for free and carry 0xFFFF - (pair score), so the duplicate search knows the better
// pair of a run from the sorted keys alone and gathers records only for the losers' mate index (and
// on the rare score tie).
constexpr int kNearScoreBits = 16;
constexpr int kNearDeltaShift = kNearScoreBits;                       // delta
constexpr int kNearOrientShift = kNearScoreBits + kNearDeltaBits;     // orientation
constexpr int kNearShift = kNearOrientShift + 2;                      // record 1's 5' end
// Near pairs are SORTED on record 1's 5' end alone (the upper 32 bits: four passes instead of six).  All
// pairs that start at one position form a run; inside it the duplicate search groups by the remaining
// identity bits (orientation, insert) by comparing every entry with every other one -- runs are two or
// three entries, and a position with more than kHugeRun pairs (amplicon-like data) makes the whole
// pipeline fall back to the full six-pass sort, where equal identities are adjacent.
constexpr u32 kHugeRun = 4096;

__device__ __forceinline__ u64 lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// exclusive scan of one u32 per thread over a block of NW wavefronts (every thread of the block must
// call it); returns the exclusive prefix, *total (if asked for) gets the block sum.  sm must hold NW u32.
template <int NW>
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32* sm, u32* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        u32 t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    __syncthreads();
    if (lane == 63) sm[wave] = incl;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const u32 s = sm[w]; if (w < wave) base += s; tot += s; }
    if (total) *total = tot;
    return base + incl - v;
}

// maxima of N values per thread over a 256-thread block, folded into the N consecutive global words
// dst[0 .. N): one shuffle loop and one barrier for all N, then thread k settles value k.  The atomic is
// skipped when the (possibly stale) global value already covers the block's.  smem must hold 4 * N u64.
template <int N>
__device__ __forceinline__ void block_max_to(u64 (&v)[N], u64* smem, u64* dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = max(v[k], (u64)__shfl_xor(v[k], off, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) smem[wave * N + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const u64 m = max(max(smem[threadIdx.x], smem[N + threadIdx.x]), max(smem[2 * N + threadIdx.x], smem[3 * N + threadIdx.x]));
        if (m > __atomic_load_n(dst + threadIdx.x, __ATOMIC_RELAXED)) atomicMax(dst + threadIdx.x, m);
    }
}

// ---------------------------------------------------------------------------------------------
// the entry words as the kernels after the build read them
// ---------------------------------------------------------------------------------------------
// Sorted pair entries: k1 (sort_key, or the near key word) plus, for far doubles, the mate's 5' end and
// the record index.  PK: those two ride in one word, mate 5' end << 32 | record, and `recw` is unused.
// Unpacked record words of near pairs carry "the mate is the neighbour rec ^ 1" in the bits outside
// rec_mask (BuildOut::mate_flag).  Near pairs come as DOUBLE with k2 == nullptr: their key word is the
// whole identity.
template <bool DOUBLE, bool PK>
struct Entries {
    const u64* k2; const u32* recw; u32 rec_mask;
    static __device__ __forceinline__ u64 packed(u64 end2, u32 rec) { return (end2 << 32) | rec; }
    __device__ __forceinline__ u64 end2(u32 t) const { return PK ? (k2[t] >> 32) : k2[t]; }          // mate 5' end (far doubles)
    __device__ __forceinline__ u64 id2(u32 t) const { return (!DOUBLE || !k2) ? 0ull : end2(t); }    // second identity word
    __device__ __forceinline__ u32 rec(u32 t) const { return PK ? (u32)k2[t] : recw[t] & rec_mask; }
    __device__ __forceinline__ bool mate_is_neighbour(u32 t) const { return !PK && (recw[t] & ~rec_mask); }
    __device__ __forceinline__ u32 mate(const mgx_rec_t* recs, u32 t, u32 r) const { return mate_is_neighbour(t) ? (r ^ 1u) : recs[r].mate; }
};

// which orientations (FF FR RF RR = 0 1 2 3) put record END of a pair on the forward strand: FF and FR for
// record 1, FF and RF for record 2
template <int END>
__device__ __forceinline__ bool end_is_forward(u32 orient) { return orient == 0u || orient == (END == 2 ? 2u : 1u); }

// the near key word p1 << kNearShift | orient << kNearOrientShift | (p2 - p1) << kNearDeltaShift | inverted score
struct NearKey { u64 p1, p2; u32 orient; };
__device__ __forceinline__ NearKey decode_near(u64 key) {
    const u64 p1 = key >> kNearShift;
    return NearKey{p1, p1 + ((key >> kNearDeltaShift) & (kNearSpan - 1)), (u32)(key >> kNearOrientShift) & 3u};
}

// ---------------------------------------------------------------------------------------------
// build: classify records, emit pair entries and coordinate keys
// ---------------------------------------------------------------------------------------------
constexpr int kBuildBlock = 2048;

struct BuildOut {
    u64* ckey; u32* cval;                 // coordinate sort input
    u64* dk1; u64* dk2; u32* drec;        // double-pair entries (compacted, arrival order)
    u64* sk1; u32* srec;                  // single-pair entries
    u32* indicator; u64 indicator_bits;   // double_pair_indicator, 4L bits
    u64 L;
    int packed_coord;                     // ckey = coord << 32 | i (every coordinate < 2^32)
    int packed_pair;                      // dk2 = mate 5' end << 32 | record (every 5' end < 2^32)
    u64* nk; u32* nrec;                   // near double pairs: one key word p1 << 32 | orient << 30 | (p2 - p1) << 16 | inverted pair score
    int near_enabled;
    u32 mate_flag;                        // 0x80000000 when record indices leave bit 31 free: "the mate is the neighbour rec ^ 1"
    u32* half_hist;                       // [workgroups][256]: histogram of the coordinate's low byte (first digit of the record sort), or NULL
};

// Entries are compacted with one global atomic per workgroup and kind, so their order is not the
// arrival order; nothing downstream depends on it: runs are formed by key equality and total ties
// between entries are broken by the record index itself (k_mark_list), not by position.
//
// Single pass over the records: a workgroup reads its 2048 records once (all loads issued up
// front), classifies them, keeps the derived entry words in registers while the per-kind counts
// are settled (LDS atomics give block-local slots, ONE global atomic per kind gives the block's
// base -- a single counter word sustains only ~90 atomics/us, never one per wavefront), then
// stores the entries.  The mate's record is read through the cache: mates are adjacent in arrival
// order, so the line is already there.
__global__ __launch_bounds__(256) void k_build_emit(const mgx_rec_t* __restrict__ recs, u32 n, BuildOut o, Scalars* sc) {
    constexpr int ITEMS = kBuildBlock / 256;
    __shared__ u64 smax[4 * 5];
    __shared__ u32 s_cnt[3], s_base[3];
    __shared__ u32 s_hist[256];
    const u32 base = blockIdx.x * kBuildBlock;
    const u64 lt = lanemask_lt();
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    s_hist[threadIdx.x] = 0;
    __syncthreads();

    u64 coord[ITEMS], p5[ITEMS];
    u32 mate[ITEMS], flag[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 i = base + k * 256 + threadIdx.x;
        coord[k] = 0; p5[k] = 0; mate[k] = MGX_NO_MATE; flag[k] = kIgnorable;      // flag: SAM flag | score << 16
        if (i < n) { coord[k] = recs[i].coord; p5[k] = recs[i].prime5; mate[k] = recs[i].mate; flag[k] = (u32)recs[i].flag | (u32)recs[i].score << 16; }
    }
    u64 mp5[ITEMS]; u32 mflag[ITEMS];      // mflag: mate's flag | mate's score << 16
    bool bad = false;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 i = base + k * 256 + threadIdx.x;
        if (i < n && mate[k] != MGX_NO_MATE && mate[k] >= n) { bad = true; mate[k] = MGX_NO_MATE; flag[k] |= kIgnorable; }
        mp5[k] = 0; mflag[k] = 0;
        // only record 1 of a pair (mate > i, not ignorable) looks at its mate
        if (i < n && !(flag[k] & kIgnorable) && mate[k] != MGX_NO_MATE && mate[k] > i) { mp5[k] = recs[mate[k]].prime5; mflag[k] = (u32)recs[mate[k]].flag | (u32)recs[mate[k]].score << 16; }
    }
    if (bad) sc->bad_mate = 1;

    u64 ka[ITEMS], kb[ITEMS];       // entry words: near key | sort_key ; mate end (far doubles only)
    u32 slot[ITEMS];                // block-local slot within the entry's kind
    int cls[ITEMS];                 // 0 none, 1 far double, 2 single, 3 near double
    u64 m_coord = 0, m_k1d = 0, m_k2d = 0, m_k1s = 0, m_near = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 i = base + k * 256 + threadIdx.x;
        int c = 0;
        u64 wa = 0, wb = 0;
        if (i < n) {
            if (o.ckey) {      // (a shard's ordering half is a different record subset: k_order_keys writes the keys then)
                o.ckey[i] = o.packed_coord ? (coord[k] << 32) | i : coord[k];
                if (!o.packed_coord) o.cval[i] = i;
                m_coord = max(m_coord, coord[k]);
                // the record sort's first digit is the coordinate's low byte in either key form: its per-tile
                // histogram is gathered here, where the keys are made, instead of by a pass that re-reads them
                if (o.half_hist) atomicAdd(&s_hist[(u32)coord[k] & 255u], 1u);
            }
            if (!(flag[k] & kIgnorable)) c = mate[k] == MGX_NO_MATE ? 2 : (mate[k] > i ? 1 : 0);
            if (c == 1) {
                // DoublePair::DoublePair, pair.cpp:71-108
                u64 p1 = p5[k], p2 = mp5[k];
                bool f1 = !(flag[k] & 0x10), f2 = !(mflag[k] & 0x10);
                if (p1 > p2) { const u64 t = p1; p1 = p2; p2 = t; const bool tf = f1; f1 = f2; f2 = tf; }
                u32 orient = f1 ? (f2 ? 0u : 1u) : (f2 ? 2u : 3u);       // FF FR RF RR
                if (p1 == p2 && orient == 2u) orient = 1u;
                const u64 k1 = (p1 << 2) + orient;
                m_k1d = max(m_k1d, k1); m_k2d = max(m_k2d, p2);
                // near pair: the whole (sort_key, mate end) identity fits one word, injectively
                const bool near = o.near_enabled && p2 - p1 < kNearSpan;
                const u32 pair_score = ((flag[k] >> 16) + (mflag[k] >> 16)) & 0xFFFFu;              // pair.cpp:81: uint16 sum
                const u64 nkey = (p1 << kNearShift) | ((u64)orient << kNearOrientShift) | ((p2 - p1) << kNearDeltaShift) |
                                 (u64)(0xFFFFu - pair_score);
                c = near ? 3 : 1;
                wa = near ? nkey : k1;
                wb = p2;
                if (near) m_near = max(m_near, nkey);
            } else if (c == 2) {
                // SinglePair::SinglePair, pair.cpp:51-69
                wa = (p5[k] << 2) + ((flag[k] & 0x10) ? 3u : 0u);
                m_k1s = max(m_k1s, wa);
            }
        }
        ka[k] = wa; kb[k] = wb;
        cls[k] = c;
        const u64 bd = __ballot(c == 1), bs = __ballot(c == 2), bn = __ballot(c == 3);
        u32 based = 0, bases = 0, basen = 0;
        if ((threadIdx.x & 63) == 0) {
            if (bd) based = atomicAdd(&s_cnt[0], (u32)__popcll(bd));      // LDS
            if (bs) bases = atomicAdd(&s_cnt[1], (u32)__popcll(bs));
            if (bn) basen = atomicAdd(&s_cnt[2], (u32)__popcll(bn));
        }
        based = __shfl(based, 0, 64); bases = __shfl(bases, 0, 64); basen = __shfl(basen, 0, 64);
        slot[k] = c == 1 ? based + (u32)__popcll(bd & lt) : c == 2 ? bases + (u32)__popcll(bs & lt) : basen + (u32)__popcll(bn & lt);
    }
    __syncthreads();
    if (o.half_hist) o.half_hist[(size_t)blockIdx.x * 256 + threadIdx.x] = s_hist[threadIdx.x];
    if (threadIdx.x < 3) {
        const u32 cnt = s_cnt[threadIdx.x];
        u32* dst = threadIdx.x == 0 ? &sc->n_double : threadIdx.x == 1 ? &sc->n_single : &sc->n_near;
        s_base[threadIdx.x] = cnt ? atomicAdd(dst, cnt) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 i = base + k * 256 + threadIdx.x;
        if (cls[k] == 3) {
            const u32 at = s_base[2] + slot[k];
            o.nk[at] = ka[k]; o.nrec[at] = i | (mate[k] == (i ^ 1u) ? o.mate_flag : 0u);
        } else if (cls[k] == 1) {
            const u32 at = s_base[0] + slot[k];
            o.dk1[at] = ka[k];
            if (o.packed_pair) o.dk2[at] = Entries<true, true>::packed(kb[k], i); else { o.dk2[at] = kb[k]; o.drec[at] = i; }
        } else if (cls[k] == 2) {
            const u32 at = s_base[1] + slot[k];
            o.sk1[at] = ka[k]; o.srec[at] = i;
        }
    }
    // the five key maxima in one fused reduction (one barrier)
    u64 mx[5] = {m_coord, m_k1d, m_k2d, m_k1s, m_near};      // in the order of Scalars
    block_max_to(mx, smax, &sc->max_coord);
}

// Upload wire format: whenever a piece's coordinates and 5' ends all fit 32 bits (always, unless a 5' end wrapped
// below zero or L >= 2^32) the staging threads squeeze the 32-byte records to 24 bytes on their way into the pinned
// buffer -- a quarter fewer bytes over PCIe, the link being what an upload waits for -- and this kernel restores
// the 32-byte layout in HBM right behind the copy.
struct Wire24 { u32 coord, prime5, mate; uint16_t flag, score, tile, x, y, pad_; };
static_assert(sizeof(Wire24) == 24, "wire record is 24 bytes");
__global__ __launch_bounds__(256) void k_expand24(const Wire24* __restrict__ src, mgx_rec_t* __restrict__ dst, u32 n) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Wire24 w = src[i];
    mgx_rec_t r;
    r.coord = w.coord; r.prime5 = w.prime5; r.mate = w.mate; r.flag = w.flag; r.score = w.score;
    r.tile = w.tile; r.x = w.x; r.y = w.y; r.pad_ = 0;
    dst[i] = r;
}

// Sharded input (mgx_sortdedup_upload_shard): the records a shard ORDERS are not the records it MARKS, so the
// coordinate keys come from the routed (coordinate, global arrival index) arrays instead of the build kernel.
__global__ __launch_bounds__(256) void k_order_keys(const u64* __restrict__ coord, const u32* __restrict__ arrival, u32 n,
                                                    u64* __restrict__ ckey, u32* __restrict__ cval, int packed, Scalars* sc) {
    __shared__ u64 smax[4];
    u64 m = 0;
    for (u32 i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const u64 cd = coord[i];
        const u32 a = arrival[i];
        ckey[i] = packed ? (cd << 32) | a : cd;
        if (!packed) cval[i] = a;
        m = max(m, cd);
    }
    u64 mx[1] = {m};
    block_max_to(mx, smax, &sc->max_coord);
}

// Indicator marks routed from other shards (5' position << 1 | reverse half): ORed into the bitmap after the
// shard's own pairs have defined it and before its fragments are tested.  In the tiled layout a position at or
// beyond L - 64 cannot be hit by any of this shard's fragments (the layout is only chosen when all of its own
// 5' ends are below), so such a mark is dropped instead of aliasing into the other half.
__global__ __launch_bounds__(256) void k_or_marks(const u64* __restrict__ marks, u32 n, u32* __restrict__ indicator, u64 ind_bits,
                                                  u64 ind_off, u64 fwd_limit) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 mk = marks[i], pos = mk >> 1;
    if (pos >= fwd_limit) return;
    const u64 b = pos + ((mk & 1) ? ind_off : 0ull);
    if (b < ind_bits) atomicOr(&indicator[b >> 5], 1u << (b & 31));
}

// ---------------------------------------------------------------------------------------------
// radix sort pass: histogram -> column scan -> ranked scatter
// ---------------------------------------------------------------------------------------------
template <int TILE>
__global__ __launch_bounds__(256) void k_radix_hist(const u64* __restrict__ keys, u32 n, int shift, u32* __restrict__ hist) {
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u32 base = blockIdx.x * TILE;
#pragma unroll
    for (int k = 0; k < TILE / 256; ++k) {
        const u32 i = base + k * 256 + threadIdx.x;
        if (i < n) atomicAdd(&h[(u32)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];     // tile-major: coalesced
}

// first pass of the record sort: the build kernel's half-tile histograms (kBuildBlock records each) -> tile histograms
template <int TILE>
__global__ __launch_bounds__(256) void k_hist_merge(const u32* __restrict__ half, u32 n_half, u32* __restrict__ hist) {
    constexpr int RATIO = TILE / kBuildBlock;
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < RATIO; ++k) {
        const u32 hb = blockIdx.x * RATIO + k;
        if (hb < n_half) v += half[(size_t)hb * 256 + threadIdx.x];
    }
    hist[(size_t)blockIdx.x * 256 + threadIdx.x] = v;
}

// column sums per chunk of kChunkTiles tiles
__global__ __launch_bounds__(256) void k_radix_chunk_sums(const u32* __restrict__ hist, u32 n_tiles, u32* __restrict__ chunk_sums) {
    const u32 t0 = blockIdx.x * kChunkTiles, t1 = min(n_tiles, t0 + kChunkTiles);
    u32 s = 0;
    for (u32 t = t0; t < t1; ++t) s += hist[(size_t)t * 256 + threadIdx.x];
    chunk_sums[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

// one block: digit bases (exclusive over digits) + exclusive scan over chunks per digit column.
// A single workgroup alone on the device is pure latency, so both loops keep 16 independent loads in
// flight per thread (the in-place update would otherwise serialise on load -> store -> load).
__global__ __launch_bounds__(256) void k_radix_scan_chunks(u32* chunk_sums, u32 n_chunks) {
    __shared__ u32 sm[4];
    constexpr int B = 16;
    u32 tot = 0;
    for (u32 c0 = 0; c0 < n_chunks; c0 += B) {
        u32 x[B];
#pragma unroll
        for (int k = 0; k < B; ++k) x[k] = c0 + k < n_chunks ? chunk_sums[(size_t)(c0 + k) * 256 + threadIdx.x] : 0u;
#pragma unroll
        for (int k = 0; k < B; ++k) tot += x[k];
    }
    u32 all;
    u32 run = block_excl_scan<4>(tot, sm, &all);      // where this digit starts in the output
    for (u32 c0 = 0; c0 < n_chunks; c0 += B) {
        u32 x[B];
#pragma unroll
        for (int k = 0; k < B; ++k) x[k] = c0 + k < n_chunks ? chunk_sums[(size_t)(c0 + k) * 256 + threadIdx.x] : 0u;
#pragma unroll
        for (int k = 0; k < B; ++k) {
            if (c0 + k < n_chunks) chunk_sums[(size_t)(c0 + k) * 256 + threadIdx.x] = run;
            run += x[k];
        }
    }
}

// per chunk: running prefix down the tiles of the chunk, in place: hist[tile][d] -> global offset
__global__ __launch_bounds__(256) void k_radix_apply(u32* __restrict__ hist, u32 n_tiles, const u32* __restrict__ chunk_sums) {
    const u32 t0 = blockIdx.x * kChunkTiles, t1 = min(n_tiles, t0 + kChunkTiles);
    u32 run = chunk_sums[(size_t)blockIdx.x * 256 + threadIdx.x];
    constexpr int B = 16;
    for (u32 tb = t0; tb < t1; tb += B) {
        u32 x[B];
#pragma unroll
        for (int k = 0; k < B; ++k) x[k] = tb + k < t1 ? hist[(size_t)(tb + k) * 256 + threadIdx.x] : 0u;
#pragma unroll
        for (int k = 0; k < B; ++k) {
            if (tb + k < t1) hist[(size_t)(tb + k) * 256 + threadIdx.x] = run;
            run += x[k];
        }
    }
}

// One tile of WAVES x 1024 keys per workgroup of WAVES wavefronts; every wavefront ranks a contiguous slice.
// (8 wavefronts = 8192-key tiles double the run a digit leaves the tile with, but measured slower: DESIGN.md 4.2.)
// LOW32: last pass of the packed record sort -- only the low half of every key (the arrival index)
// is stored, to pout32, which makes the sorted keys themselves unnecessary.
template <bool HAS_P64, bool HAS_P32, int WAVES, bool LOW32 = false>
__global__ __launch_bounds__(WAVES * 64) void k_radix_scatter(const u64* __restrict__ kin, u64* __restrict__ kout,
                                                              const u64* __restrict__ pin64, u64* __restrict__ pout64,
                                                              const u32* __restrict__ pin32, u32* __restrict__ pout32,
                                                              u32 n, int shift, const u32* __restrict__ goff, u32 n_tiles) {
    constexpr int T = WAVES * 64;           // threads
    constexpr int ITEMS = kItems;           // keys per thread
    constexpr int kTile = T * ITEMS;        // keys per workgroup: 4096 with 4 wavefronts, 8192 with 8
    constexpr int SLICE = kTile / WAVES;    // keys per wavefront
    __shared__ u64 sbuf[kTile];             // exchange buffer (keys, then payloads): 32 KB / 64 KB
    __shared__ u32 wcnt[WAVES][256];        // per wavefront and digit: running count, later the slot base
    __shared__ u32 gdelta[256];             // global offset of the digit's run minus its tile-local start
    __shared__ u32 sm[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Workgroups are dealt to the 8 XCDs round-robin and every XCD has its own L2.  A digit's run of
    // ~16 keys starts at an arbitrary 8-byte offset, so most 128-byte lines are completed by the
    // NEXT tile: giving each XCD a contiguous range of tiles (walked in order) lets both halves of
    // such a line meet in one L2 instead of reaching HBM as two partial writes from two L2s.
    const u32 q = n_tiles >> 3, r = n_tiles & 7u, x = blockIdx.x & 7u;
    const u32 tile = x * q + min(x, r) + (blockIdx.x >> 3);
    const u32 tile0 = tile * kTile;
    const u32 tile_n = min((u32)kTile, n - tile0);
    for (int i = tid; i < WAVES * 256; i += T) (&wcnt[0][0])[i] = 0;
    const u32 my_goff = tid < 256 ? goff[(size_t)tile * 256 + tid] : 0u;
    __syncthreads();

    // phase 1: stable rank of every key inside its wavefront's slice
    u64 key[ITEMS];
    u64 pay[HAS_P64 ? ITEMS : 1];
    u32 lrank[ITEMS];
    constexpr bool KEEP_DIG = !(HAS_P64 && ITEMS > 8);   // register budget: recompute the digit in the widest form
    u32 dig[KEEP_DIG ? ITEMS : 1];
    const u64 lt = lanemask_lt();
    const bool hi_word = shift >= 32;       // digits are byte aligned (shift is a multiple of 8): never straddle
    const int sh = shift & 31;
    // all global loads of the tile are issued up front: the payload's HBM latency is then hidden
    // behind the ranking arithmetic instead of being exposed between two barriers later on.
    // Slots past the end of the input hold ~0: they are the last of the tile in input order and
    // carry the last digit, so ranking them like keys changes no valid key's slot.
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 li = wave * SLICE + k * 64 + lane;            // local index: slices are contiguous per wave
        key[k] = li < tile_n ? kin[tile0 + li] : ~0ull;
    }
    if constexpr (HAS_P64) {
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const u32 li = wave * SLICE + k * 64 + lane;
            pay[k] = li < tile_n ? pin64[tile0 + li] : 0ull;
        }
    }
    u32 pay32[HAS_P32 ? ITEMS : 1];      // loaded with the keys, not between two barriers
    if constexpr (HAS_P32) {
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const u32 li = wave * SLICE + k * 64 + lane;
            pay32[k] = li < tile_n ? pin32[tile0 + li] : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 d = ((hi_word ? (u32)(key[k] >> 32) : (u32)key[k]) >> sh) & 255u;
        if constexpr (KEEP_DIG) dig[k] = d;
        u64 peers = ~0ull;                                       // lanes holding the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const u32 r = __popcll(peers & lt);
        u32 old = 0;
        if (r == 0) old = atomicAdd(&wcnt[wave][d], (u32)__popcll(peers));
        old = __shfl(old, __ffsll((long long)peers) - 1, 64);
        lrank[k] = old + r;
    }
    __syncthreads();
    // phase 2: per digit, exclusive over the wavefronts, then exclusive over digits
    {
        u32 c[WAVES], tot = 0;
        if (tid < 256) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) { c[w] = wcnt[w][tid]; tot += c[w]; }
        }
        const u32 tb = block_excl_scan<WAVES>(tot, sm);          // threads >= 256 contribute 0 after all digits
        if (tid < 256) {
            u32 run = tb;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) { wcnt[w][tid] = run; run += c[w]; }
            gdelta[tid] = my_goff - tb;
        }
    }
    __syncthreads();
    // phase 3: keys to their tile-local sorted slot, then out in runs of consecutive addresses
    u32 lpos[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 li = wave * SLICE + k * 64 + lane;
        const u32 d = KEEP_DIG ? dig[KEEP_DIG ? k : 0] : ((hi_word ? (u32)(key[k] >> 32) : (u32)key[k]) >> sh) & 255u;
        lpos[k] = wcnt[wave][d] + lrank[k];
        if (li < tile_n) sbuf[lpos[k]] = key[k];
    }
    __syncthreads();
    u32 gpos[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const u32 i = k * T + tid;
        gpos[k] = 0;
        if (i < tile_n) {
            const u64 kk = sbuf[i];
            const u32 d = ((hi_word ? (u32)(kk >> 32) : (u32)kk) >> sh) & 255u;
            gpos[k] = gdelta[d] + i;
            if constexpr (LOW32) pout32[gpos[k]] = (u32)kk;
            else kout[gpos[k]] = kk;
        }
    }
    if constexpr (HAS_P64) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const u32 li = wave * SLICE + k * 64 + lane;
            if (li < tile_n) sbuf[lpos[k]] = pay[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const u32 i = k * T + tid;
            if (i < tile_n) pout64[gpos[k]] = sbuf[i];
        }
    }
    if constexpr (HAS_P32) {
        __syncthreads();
        u32* sbuf32 = reinterpret_cast<u32*>(sbuf);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const u32 li = wave * SLICE + k * 64 + lane;
            if (li < tile_n) sbuf32[lpos[k]] = pay32[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const u32 i = k * T + tid;
            if (i < tile_n) pout32[gpos[k]] = sbuf32[i];
        }
    }
}

// packed coordinate keys (coord << 32 | arrival index): the order is the low half of the sorted keys
__global__ __launch_bounds__(256) void k_unpack_order(const u64* __restrict__ keys, u32 n, u32* __restrict__ order) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) order[i] = (u32)keys[i];
}

// double_pair_indicator (main.cpp:181-192), set from SORTED pair entries so that consecutive lanes
// touch consecutive words: END = 2 after the sort by mate 5' end (sets the record-2 bits), END = 1
// after the sort by sort_key (sets the record-1 bits).  Random-order atomics into the 4L-bit map
// cost a 64-byte read-modify-write each; in sorted order they stay in L2.
template <int END, bool PK>
__global__ __launch_bounds__(256) void k_set_indicator(const u64* __restrict__ k1, const u64* __restrict__ k2, u32 n,
                                                       u32* __restrict__ indicator, u64 indicator_bits, u64 L) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Entries<true, PK> e{k2, nullptr, 0xFFFFFFFFu};
    const u64 a1 = k1[i];
    const u64 b = (END == 2 ? e.end2(i) : a1 >> 2) + (end_is_forward<END>((u32)(a1 & 3)) ? 0ull : L);
    if (b < indicator_bits) atomicOr(&indicator[b >> 5], 1u << (b & 31));
}

// Tiled form of the same bitmap, used whenever every 5' end lies below L - 64 (always, except for
// positions wrapped below zero or clipped past the last contig): the reverse-strand half then
// starts at Lp = L rounded up to a whole tile instead of L -- no forward bit can reach it, so the
// answers are unchanged -- and each workgroup OWNS kIndTile positions of both halves: it finds its
// slice of the sorted entries by binary search, sets bits in LDS and writes whole words with plain
// coalesced stores.  No global atomics and no memset of the 4L-bit map.
constexpr u32 kIndTile = 65536;              // positions per workgroup (2 x 8 KB of LDS)

__device__ __forceinline__ void tile_clear(u32* fw, u32* rv) {
    for (u32 w = threadIdx.x; w < kIndTile / 32; w += 256) { fw[w] = 0; rv[w] = 0; }
}
// the workgroup's LDS tile -> its words of both halves of the bitmap (after a barrier)
template <bool DEFINE>
__device__ __forceinline__ void tile_flush(const u32* fw, const u32* rv, u32* __restrict__ indicator, u64 Lp) {
    u32* gf = indicator + (size_t)blockIdx.x * (kIndTile / 32);
    u32* gr = indicator + (size_t)(Lp >> 5) + (size_t)blockIdx.x * (kIndTile / 32);
    for (u32 w = threadIdx.x; w < kIndTile / 32; w += 256) {
        if (DEFINE) { gf[w] = fw[w]; gr[w] = rv[w]; }                         // first pass: defines every word
        else { if (fw[w]) gf[w] |= fw[w]; if (rv[w]) gr[w] |= rv[w]; }        // later passes: this tile owns them
    }
}

template <int END, bool PK, bool DEFINE>
__global__ __launch_bounds__(256) void k_indicator_tiles(const u64* __restrict__ k1, const u64* __restrict__ k2, u32 n,
                                                         u32* __restrict__ indicator, u64 Lp) {
    __shared__ u32 fw[kIndTile / 32], rv[kIndTile / 32];
    __shared__ u32 s_lo, s_hi;
    const Entries<true, PK> e{k2, nullptr, 0xFFFFFFFFu};
    auto POS = [&](u32 t) -> u64 { return END == 2 ? e.end2(t) : (k1[t] >> 2); };
    tile_clear(fw, rv);
    const u64 pos_lo = (u64)blockIdx.x * kIndTile, pos_hi = pos_lo + kIndTile;
    if (threadIdx.x < 2) {
        const u64 target = threadIdx.x == 0 ? pos_lo : pos_hi;
        u32 a = 0, b = n;                                   // first entry with POS >= target
        while (a < b) { const u32 m = a + (b - a) / 2; if (POS(m) < target) a = m + 1; else b = m; }
        if (threadIdx.x == 0) s_lo = a; else s_hi = a;
    }
    __syncthreads();
    const u32 lo = s_lo, hi = s_hi;
    for (u32 i = lo + threadIdx.x; i < hi; i += 256) {
        const u32 p = (u32)(POS(i) - pos_lo);
        atomicOr(end_is_forward<END>((u32)(k1[i] & 3)) ? &fw[p >> 5] : &rv[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    tile_flush<DEFINE>(fw, rv, indicator, Lp);
}

// Near pairs (one key word p1 << 32 | orient << 30 | delta << 16 | inverted score, sorted on its upper 48 bits): both ends of every pair in ONE
// pass.  A pair's record-1 end lies in the tile of p1, its record-2 end at p1 + delta < p1 + kNearSpan in
// that tile or the next, so tile t scans the entries with p1 in [t*65536 - (kNearSpan - 1), (t+1)*65536).
// Always the first pass over the bitmap: defines every word.
// sub_start[x] = first sorted entry whose record-1 end is at or beyond x * kNearSpan (written by k_find_runs):
// the tile's slice of the entries without two 27-step binary searches per workgroup.
__global__ __launch_bounds__(256) void k_indicator_tiles_near(const u64* __restrict__ nk, u32 n, u32* __restrict__ indicator, u64 Lp,
                                                              const u32* __restrict__ sub_start, u32 n_sub) {
    __shared__ u32 fw[kIndTile / 32], rv[kIndTile / 32];
    __shared__ u32 s_lo, s_hi;
    tile_clear(fw, rv);
    const u64 pos_lo = (u64)blockIdx.x * kIndTile, pos_hi = pos_lo + kIndTile;
    constexpr u32 kSubPerTile = kIndTile / (u32)kNearSpan;
    if (threadIdx.x == 0) {
        // entries with p1 >= pos_lo - kNearSpan (a superset of the pairs whose second end can reach this tile) ...
        s_lo = blockIdx.x == 0 ? 0u : sub_start[blockIdx.x * kSubPerTile - 1];
        // ... up to the first entry at or beyond pos_hi
        s_hi = sub_start[min((blockIdx.x + 1) * kSubPerTile, n_sub)];
    }
    __syncthreads();
    const u32 lo = s_lo, hi = min(s_hi, n);
    for (u32 i = lo + threadIdx.x; i < hi; i += 256) {
        const NearKey k = decode_near(nk[i]);
        if (k.p1 >= pos_lo) {
            const u32 p = (u32)(k.p1 - pos_lo);
            atomicOr(end_is_forward<1>(k.orient) ? &fw[p >> 5] : &rv[p >> 5], 1u << (p & 31));
        }
        if (k.p2 >= pos_lo && k.p2 < pos_hi) {
            const u32 p = (u32)(k.p2 - pos_lo);
            atomicOr(end_is_forward<2>(k.orient) ? &fw[p >> 5] : &rv[p >> 5], 1u << (p & 31));
        }
    }
    __syncthreads();
    tile_flush<true>(fw, rv, indicator, Lp);
}

// atomic fallback for near pairs (reference bitmap layout)
__global__ __launch_bounds__(256) void k_set_indicator_near(const u64* __restrict__ nk, u32 n, u32* __restrict__ indicator,
                                                            u64 indicator_bits, u64 L) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const NearKey k = decode_near(nk[i]);
    const u64 b1 = k.p1 + (end_is_forward<1>(k.orient) ? 0ull : L), b2 = k.p2 + (end_is_forward<2>(k.orient) ? 0ull : L);
    if (b1 < indicator_bits) atomicOr(&indicator[b1 >> 5], 1u << (b1 & 31));
    if (b2 < indicator_bits) atomicOr(&indicator[b2 >> 5], 1u << (b2 & 31));
}

// ---------------------------------------------------------------------------------------------
// best-of-run and duplicate marking
// ---------------------------------------------------------------------------------------------
// both records of a losing pair: one 2-byte store when the mate is the neighbour (flag in the record word)
__device__ __forceinline__ void mark_pair(uint8_t* dup, const mgx_rec_t* recs, u32 r, bool neighbour) {
    if (neighbour) reinterpret_cast<uint16_t*>(dup)[r >> 1] = 0x0101;
    else { dup[r] = 1; dup[recs[r].mate] = 1; }
}

// quality of a pair entry: smaller is better -- score descending, then tile, x, y ascending
// (main.cpp:253-264 / 303-314); the record index (= arrival order) breaks total ties
__device__ __forceinline__ u64 place_word(const mgx_rec_t& a) {          // what decides between equal scores
    return ((u64)a.tile << 32) | ((u64)a.x << 16) | (u64)a.y;
}
__device__ __forceinline__ u64 quality_word(uint16_t score, const mgx_rec_t& a) {
    return ((u64)(0xFFFFu - (u32)score) << 48) | place_word(a);
}
__device__ __forceinline__ u64 quality_double(const mgx_rec_t* recs, u32 rec) {
    const mgx_rec_t a = recs[rec];
    const mgx_rec_t b = recs[a.mate];
    return quality_word((uint16_t)(a.score + b.score), a);                // pair.cpp:81: uint16 sum
}
__device__ __forceinline__ u64 quality_single(const mgx_rec_t* recs, u32 rec) {
    const mgx_rec_t a = recs[rec];
    return quality_word(a.score, a);
}

// main.cpp:325-331: the kept single read of a run is a duplicate iff a double pair has an end on its
// position and strand.  rev_off: where the reverse-strand half of the bitmap starts.
__device__ __forceinline__ bool single_hits_pair_end(const u32* __restrict__ indicator, u64 ind_bits, u64 rev_off, u64 key) {
    const u64 target = (key >> 2) + (((key & 3) == 3) ? rev_off : 0ull);
    return target < ind_bits && ((indicator[target >> 5] >> (target & 31)) & 1u);
}

// Near pairs sorted on record 1's 5' end only: the run [first, end) holds every pair that starts there.
// Entry t loses to any other entry of the run with the same identity (the key bits above the score)
// and a better score -- tile, x, y, then arrival order on a score tie.  Records are gathered only on
// such a tie.
template <class E>
__device__ __forceinline__ bool near_entry_loses(const u64* __restrict__ k1, const E& entries, const mgx_rec_t* __restrict__ recs,
                                                 u32 first, u32 end, u32 t) {
    const u64 kt = k1[t];
    const u64 idt = kt >> kNearScoreBits;
    const u32 st = (u32)(kt & 0xFFFFu);
    bool have_t = false;
    u32 rt = 0; u64 qt = 0;
    for (u32 u = first; u < end; ++u) {
        if (u == t) continue;
        const u64 ku = k1[u];
        if ((ku >> kNearScoreBits) != idt) continue;
        const u32 su = (u32)(ku & 0xFFFFu);
        if (su < st) return true;
        if (su == st) {
            if (!have_t) { rt = entries.rec(t); qt = place_word(recs[rt]); have_t = true; }
            const u32 ru = entries.rec(u);
            const u64 qu = place_word(recs[ru]);
            if (qu < qt || (qu == qt && ru < rt)) return true;
        }
    }
    return false;
}

// A whole workgroup finds where the run that starts at `first` ends: the first t in (first, n) with
// !same_run(t), or n.  Every thread of the block must call it with the same first and n; the value
// that ends the loop is read from LDS between two barriers, so all threads leave it in the same round.
template <class F>
__device__ __forceinline__ u32 block_run_end(u32 first, u32 n, F same_run) {
    __shared__ u32 s_end;
    for (u32 c = first; c < n; c += 256) {
        const u32 t = c + threadIdx.x;
        if (threadIdx.x == 0) s_end = n;
        __syncthreads();
        if (t < n && !same_run(t)) atomicMin(&s_end, t);
        __syncthreads();
        const u32 e = s_end;
        __syncthreads();
        if (e < n) return e;
    }
    return n;
}

// Duplicate search over the sorted entries, in two steps so that the random-access part runs dense:
//   k_find_runs : one lane per entry finds the run heads.  A run of ONE entry (nine in ten) needs no
//                 quality comparison at all: nothing to mark for pairs; for singles only the
//                 indicator test of main.cpp:325-331.  Heads of longer runs are appended to a list
//                 (LDS slots + one global atomic per 4096-entry workgroup; list order is irrelevant).
//   k_mark_list : one lane per listed head walks its run (runs are short), gathers the records'
//                 quality words and marks everything but the best.  Runs longer than kWalkCap go to
//                 a second list that k_mark_long handles with a whole workgroup each.
constexpr int kFindItems = 16;

template <bool DOUBLE, bool PK, int KS>
__global__ __launch_bounds__(256) void k_find_runs(const u64* __restrict__ k1, const u64* __restrict__ k2,
                                                   const u32* __restrict__ rec, u32 n,
                                                   const u32* __restrict__ indicator, u64 indicator_bits, u64 rev_off,
                                                   uint8_t* __restrict__ dup, u32* __restrict__ multi_list, u32* n_multi,
                                                   u32* __restrict__ sub_start, u32 n_sub) {
    __shared__ u32 s_base;
    __shared__ u32 s_scan[4];
    const Entries<DOUBLE, PK> e{k2, rec, 0xFFFFFFFFu};      // only singles read a record index here: no flag bits
    const u32 base = blockIdx.x * (256 * kFindItems);
    u32 is_multi = 0;
#pragma unroll
    for (int k = 0; k < kFindItems; ++k) {
        const u32 i = base + k * 256 + threadIdx.x;
        bool multi = false;
        // neighbours come from the adjacent lanes; only the two edge lanes of a wavefront load theirs
        const int lane = threadIdx.x & 63;
        const u64 a1 = i < n ? k1[i] >> KS : 0ull, a2 = i < n ? e.id2(i) : 0ull;     // KS: key bits below the identity
        u64 p1 = __shfl_up(a1, 1, 64), p2 = DOUBLE ? __shfl_up(a2, 1, 64) : 0ull;
        u64 n1 = __shfl_down(a1, 1, 64), n2 = DOUBLE ? __shfl_down(a2, 1, 64) : 0ull;
        if (lane == 0 && i > 0 && i < n) { p1 = k1[i - 1] >> KS; p2 = e.id2(i - 1); }
        if (lane == 63 && i + 1 < n) { n1 = k1[i + 1] >> KS; n2 = e.id2(i + 1); }
        if constexpr (KS >= kNearScoreBits) {
            // near pairs: where the sorted entries cross a kNearSpan boundary of the genome (for the bitmap pass)
            if (sub_start && i < n) {
                const u32 cur = (u32)((a1 >> (kNearShift - KS)) >> kNearDeltaBits);
                const int prev = i == 0 ? -1 : (int)((p1 >> (kNearShift - KS)) >> kNearDeltaBits);
                for (int x = prev + 1; x <= (int)cur && x <= (int)n_sub; ++x) sub_start[x] = i;
                if (i == n - 1) for (u32 x = cur + 1; x <= n_sub; ++x) sub_start[x] = n;
            }
        }
        if (i < n) {
            const bool head = i == 0 || p1 != a1 || (DOUBLE && p2 != a2);
            if (head) {
                multi = i + 1 < n && n1 == a1 && (!DOUBLE || n2 == a2);
                if (!DOUBLE && !multi && single_hits_pair_end(indicator, indicator_bits, rev_off, a1)) dup[e.rec(i)] = 1;
            }
        }
        is_multi |= (multi ? 1u : 0u) << k;
    }
    // one block scan over the per-thread counts (instead of a ballot + LDS atomic per item), one global
    // atomic per workgroup; the list's order is irrelevant
    u32 total;
    u32 at = block_excl_scan<4>((u32)__popc(is_multi), s_scan, &total);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(n_multi, total) : 0u;
    __syncthreads();
    at += s_base;
#pragma unroll
    for (int k = 0; k < kFindItems; ++k)
        if ((is_multi >> k) & 1u) multi_list[at++] = base + k * 256 + threadIdx.x;
}

template <bool DOUBLE, bool PK, int KS>
__global__ __launch_bounds__(256) void k_mark_list(const u64* __restrict__ k1, const u64* __restrict__ k2,
                                                   const u32* __restrict__ rec, u32 n, const mgx_rec_t* __restrict__ recs, u32 n_records,
                                                   const u32* __restrict__ indicator, u64 indicator_bits, u64 rev_off,
                                                   uint8_t* __restrict__ dup, const u32* __restrict__ multi_list, const u32* n_multi,
                                                   u32* __restrict__ long_list, u32* n_long, u32 rec_mask) {
    const Entries<DOUBLE, PK> e{k2, rec, rec_mask};
    const u32 total = *n_multi;
    for (u32 li = blockIdx.x * 256 + threadIdx.x; li < total; li += gridDim.x * 256) {
        const u32 i = multi_list[li];
        if constexpr (KS > kNearScoreBits) {
            // near pairs sorted on record 1's 5' end only: every entry of the run against every other one
            const u64 run_id = k1[i] >> KS;
            u32 j = i + 1;
            for (; j < n && j - i < kWalkCap; ++j) if ((k1[j] >> KS) != run_id) break;
            if (j < n && j - i >= kWalkCap && (k1[j] >> KS) == run_id) {
                long_list[atomicAdd(n_long, 1u)] = i;                                 // long run: defer
                continue;
            }
            for (u32 t = i; t < j; ++t)
                if (near_entry_loses(k1, e, recs, i, j, t)) mark_pair(dup, recs, e.rec(t), e.mate_is_neighbour(t));
            continue;
        } else if constexpr (KS > 0) {
            // near pairs: the low KS bits of the key word are 0xFFFF - pair score, so the best entry of
            // the run is known from the sorted keys; records are gathered only when several entries
            // share the best score (tile, x, y, then arrival order decide) and for the losers' mates
            const u64 id = k1[i] >> KS;
            u32 best = i, bs = (u32)(k1[i] & ((1u << KS) - 1));
            bool tie = false;
            u32 j = i + 1;
            for (; j < n && j - i < kWalkCap; ++j) {
                const u64 kj = k1[j];
                if ((kj >> KS) != id) break;
                const u32 sj = (u32)(kj & ((1u << KS) - 1));
                if (sj < bs) { bs = sj; best = j; tie = false; }
                else if (sj == bs) tie = true;
            }
            if (j < n && j - i >= kWalkCap && (k1[j] >> KS) == id) {
                long_list[atomicAdd(n_long, 1u)] = i;                                 // long run: defer
                continue;
            }
            if (tie) {
                u64 bq = ~0ull; u32 br = 0xFFFFFFFFu;
                for (u32 t = i; t < j; ++t) {
                    if ((u32)(k1[t] & ((1u << KS) - 1)) != bs) continue;
                    const u32 rt = e.rec(t);
                    const u64 q = place_word(recs[rt]);
                    if (q < bq || (q == bq && rt < br)) { bq = q; br = rt; best = t; }
                }
            }
            for (u32 t = i; t < j; ++t) {
                if (t == best) continue;
                mark_pair(dup, recs, e.rec(t), e.mate_is_neighbour(t));
            }
            continue;
        }
        const u64 a1 = k1[i], a2 = e.id2(i);
        // the first two entries belong to the run by construction: their record gathers (the slow,
        // random part) are issued together instead of one after the other
        const u32 r0 = e.rec(i), r1 = e.rec(i + 1);
        const mgx_rec_t ra = recs[r0], rb = recs[r1];
        u64 q0, q1;
        if (DOUBLE) {
            // mates sit next to each other in arrival order (mgx_sortdedup_pack emits record 1, record 2):
            // the neighbour in the same 64-byte pair is fetched together with the record instead of
            // after it; only a mate that lives elsewhere costs a second, dependent gather
            const u32 na = r0 ^ 1u, nb = r1 ^ 1u;
            uint16_t ma = na < n_records ? recs[na].score : (uint16_t)0, mb = nb < n_records ? recs[nb].score : (uint16_t)0;
            if (ra.mate != na) ma = recs[ra.mate].score;
            if (rb.mate != nb) mb = recs[rb.mate].score;
            q0 = quality_word((uint16_t)(ra.score + ma), ra);                 // pair.cpp:81: uint16 sum
            q1 = quality_word((uint16_t)(rb.score + mb), rb);
        } else {
            q0 = quality_word(ra.score, ra); q1 = quality_word(rb.score, rb);
        }
        u32 best = i, best_rec = r0;
        u64 bq = q0;
        if (q1 < bq || (q1 == bq && r1 < best_rec)) { bq = q1; best = i + 1; best_rec = r1; }
        u32 j = i + 2;
        for (; j < n && j - i < kWalkCap; ++j) {
            if (k1[j] != a1 || (DOUBLE && e.id2(j) != a2)) break;
            const u32 rj = e.rec(j);
            const u64 q = DOUBLE ? quality_double(recs, rj) : quality_single(recs, rj);
            if (q < bq || (q == bq && rj < best_rec)) { bq = q; best = j; best_rec = rj; }
        }
        if (j < n && j - i >= kWalkCap && k1[j] == a1 && (!DOUBLE || e.id2(j) == a2)) {
            long_list[atomicAdd(n_long, 1u)] = i;                                     // long run: defer
            continue;
        }
        if (!DOUBLE && single_hits_pair_end(indicator, indicator_bits, rev_off, a1)) dup[e.rec(best)] = 1;
        for (u32 t = i; t < j; ++t) {
            if (t == best) continue;
            const u32 r = e.rec(t);
            dup[r] = 1;
            if (DOUBLE) dup[e.mate(recs, t, r)] = 1;
        }
    }
}

template <bool DOUBLE, bool PK, int KS>
__global__ __launch_bounds__(256) void k_mark_long(const u64* __restrict__ k1, const u64* __restrict__ k2,
                                                   const u32* __restrict__ rec, u32 n, const mgx_rec_t* __restrict__ recs,
                                                   const u32* __restrict__ indicator, u64 indicator_bits, u64 rev_off,
                                                   uint8_t* __restrict__ dup, const u32* __restrict__ long_list, const u32* n_long, u32 rec_mask) {
    __shared__ u64 sq[256];
    __shared__ u32 sp[256];
    __shared__ u32 sr[256];
    const Entries<DOUBLE, PK> e{k2, rec, rec_mask};
    for (u32 li = blockIdx.x; li < *n_long; li += gridDim.x) {
        const u32 i = long_list[li];
        const u64 a1 = k1[i] >> KS, a2 = e.id2(i);          // KS: key bits below the identity
        const u32 end = block_run_end(i, n, [&](u32 t) { return (k1[t] >> KS) == a1 && (!DOUBLE || e.id2(t) == a2); });
        // the run's best entry: per thread, then over the block
        u64 bq = ~0ull; u32 bp = 0xFFFFFFFFu, bpr = 0xFFFFFFFFu;
        for (u32 t = i + threadIdx.x; t < end; t += 256) {
            const u32 r = e.rec(t);
            const u64 q = DOUBLE ? quality_double(recs, r) : quality_single(recs, r);
            if (q < bq || (q == bq && r < bpr)) { bq = q; bp = t; bpr = r; }
        }
        sq[threadIdx.x] = bq; sp[threadIdx.x] = bp; sr[threadIdx.x] = bpr;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                const u64 q = sq[threadIdx.x + s]; const u32 p = sp[threadIdx.x + s], r = sr[threadIdx.x + s];
                if (q < sq[threadIdx.x] || (q == sq[threadIdx.x] && r < sr[threadIdx.x])) { sq[threadIdx.x] = q; sp[threadIdx.x] = p; sr[threadIdx.x] = r; }
            }
            __syncthreads();
        }
        const u32 best = sp[0];
        __syncthreads();
        if (!DOUBLE && threadIdx.x == 0 && single_hits_pair_end(indicator, indicator_bits, rev_off, a1)) dup[e.rec(best)] = 1;
        for (u32 t = i + threadIdx.x; t < end; t += 256) {
            if (t == best) continue;
            const u32 r = e.rec(t);
            dup[r] = 1;
            if (DOUBLE) dup[e.mate(recs, t, r)] = 1;
        }
        __syncthreads();
    }
}

// long runs of the position-sorted near pairs: one workgroup per run, every entry against every other
// (bounded by kHugeRun; beyond that the flag sends the whole pipeline to the six-pass sort)
template <int RS>
__global__ __launch_bounds__(256) void k_mark_long_sub(const u64* __restrict__ k1, const u32* __restrict__ rec, u32 n,
                                                       const mgx_rec_t* __restrict__ recs, uint8_t* __restrict__ dup,
                                                       const u32* __restrict__ long_list, const u32* n_long, u32* huge_runs, u32 rec_mask) {
    const Entries<true, false> e{nullptr, rec, rec_mask};
    for (u32 li = blockIdx.x; li < *n_long; li += gridDim.x) {
        const u32 i = long_list[li];
        const u64 run_id = k1[i] >> RS;
        const u32 end = block_run_end(i, n, [&](u32 t) { return (k1[t] >> RS) == run_id; });
        if (end - i > kHugeRun) {
            if (threadIdx.x == 0) atomicOr(huge_runs, 1u);
            continue;
        }
        for (u32 t = i + threadIdx.x; t < end; t += 256)
            if (near_entry_loses(k1, e, recs, i, end, t)) mark_pair(dup, recs, e.rec(t), e.mate_is_neighbour(t));
    }
}

__global__ __launch_bounds__(256) void k_count_dup(const uint8_t* dup, u32 n, Scalars* sc) {
    // 16 flag bytes per load (the array comes from hipMalloc: 256-byte aligned); bytes are 0 or 1
    u32 c = 0;
    const u32 n16 = n / 16;
    const uint4* d4 = reinterpret_cast<const uint4*>(dup);
    for (u32 i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) {
        const uint4 v = d4[i];
        c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    for (u32 i = n16 * 16 + blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) c += dup[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sc->n_dup, c);
}

inline int bits_of(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b ? b : 1; }

}  // namespace

struct mgx_sortdedup {
    template <typename T> using DevArray = mgx_hip::DevArray<T>;      // each grown to the exact count
    mgx_hip::Owner own;                    // of the streams, the events and d_sc; the first member: the streams go last
    mgx_hip::Owner work;                   // of the work buffers below, released and refilled as a whole (ensure_capacity)
    int device = 0;
    unsigned flags = 0;
    hipStream_t compute = nullptr, copy = nullptr;
    int n_cu = 256;
    uint64_t L = 0;
    u32 n = 0;                             // records the duplicate search works on (the marking half of a shard)
    u32 n_order = 0;                       // records the coordinate sort orders (== n unless the input is a shard)
    bool sharded = false;
    DevArray<u64> ocoord; DevArray<u32> oarr;          // a shard's ordering half as uploaded
    DevArray<u64> marks; u32 n_marks = 0;  // indicator marks routed from other shards
    size_t cap = 0;                        // record capacity of the work buffers below
    DevArray<mgx_rec_t> recs;              // the uploaded records (a streamed upload grows it by hand: ensure_recs keeps the contents)
    mgx_hip::Mirror stage[2];              // staging buffers of the exact chunk size; device side: compact 24-byte records before expansion
    uint64_t up_L = 0, up_high = 0;        // streamed upload in progress: reference length, highest record index seen + 1
    bool uploading = false;
    u64 *d_ckey[2] = {nullptr, nullptr}; u32* d_cval[2] = {nullptr, nullptr};
    u64 *d_k1[2] = {nullptr, nullptr}, *d_k2[2] = {nullptr, nullptr}; u32* d_prec[2] = {nullptr, nullptr};
    u64* d_sk1[2] = {nullptr, nullptr}; u32* d_srec[2] = {nullptr, nullptr};
    u64* d_nk[2] = {nullptr, nullptr}; u32* d_nrec[2] = {nullptr, nullptr};     // near double pairs
    // three independent sorts run concurrently (main: far pairs + singles, side[0]: near pairs,
    // side[1]: records), each with its own histogram / scan / long-run scratch
    struct Scratch { u32 *hist = nullptr, *chunk = nullptr, *longl = nullptr, *multi = nullptr; } scr[3];
    hipStream_t side[2] = {nullptr, nullptr};
    hipEvent_t ev_ind = nullptr, ev_side[2] = {nullptr, nullptr};
    DevArray<u32> indicator; uint64_t indicator_bits = 0;      // the bitmap, in 32-bit words
    DevArray<u32> sub_start;                                   // first near entry per kNearSpan positions (bitmap pass)
    uint8_t* d_dup = nullptr;
    u32* d_half_hist = nullptr;            // [ceil(n / kBuildBlock)][256], written by the build kernel
    Scalars* d_sc = nullptr;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    std::vector<hipEvent_t> ev_scatter;    // pairs (start, stop) per scatter launch
    size_t ev_used = 0;
    size_t ev_rec_begin = 0, ev_rec_end = 0;   // event range of the record sort's scatter launches
    uint64_t rec_scatter_bytes = 0, scatter_bytes = 0;
    int order_buf = 0;                     // which d_cval holds the final order
    bool packed_coord = false;             // L < 2^32: coordinate sort on packed (coord, index) words
    bool packed_pair = false;              // every 5' end < 2^32: (mate end, record) ride in one word
    bool ran = false;
    bool near_by_position = true;          // near pairs sorted on record 1's 5' end only (MGX_SORTDEDUP_NEAR_EXACT=1: six-pass sort)
    bool finished = false;                 // the results of the last run have been checked for the fallback
    Scalars sc{};
    mgx_sortdedup_stats_t stats{};
};

namespace {

constexpr size_t kPinnedChunk = 64u << 20;

int ensure_capacity(mgx_sortdedup* c, size_t n) {
    if (n <= c->cap) return 0;
    mgx_hip::Owner& w = c->work;
    w.reset();
    c->cap = 0;
    const size_t half = n / 2 + 1;
    const size_t n_tiles = (n + kTile - 1) / kTile + 1;
    auto dev = [&w](auto** p, size_t count) { w.device(p, std::max<size_t>(count, 1) * sizeof(**p)); };
    for (int i = 0; i < 2; ++i) {
        dev(&c->d_ckey[i], n); dev(&c->d_cval[i], n);
        dev(&c->d_k1[i], half); dev(&c->d_k2[i], half); dev(&c->d_prec[i], half);
        dev(&c->d_sk1[i], n); dev(&c->d_srec[i], n);
        dev(&c->d_nk[i], half); dev(&c->d_nrec[i], half);
    }
    for (auto& q : c->scr) {
        dev(&q.hist, n_tiles * 256);                          // tile histograms, then offsets
        dev(&q.chunk, ((n_tiles + kChunkTiles - 1) / kChunkTiles + 1) * 256);
        dev(&q.longl, n / kWalkCap + 16);
        dev(&q.multi, n / 2 + 16);          // heads of runs with >= 2 entries
    }
    dev(&c->d_dup, n);
    dev(&c->d_half_hist, (n / kBuildBlock + 2) * 256);
    if (!w.ok()) { w.release(); return -ENOMEM; }
    c->cap = n;
    return 0;
}

// one stable LSD radix sort of (key, [p64], p32) over `bits` low bits of the key
// buffers are ping-pong pairs; *cur is the index of the input buffer and is updated
int radix_sort(mgx_sortdedup* c, hipStream_t s, const mgx_sortdedup::Scratch& q, u64* key[2], u64* p64[2], u32* p32[2], u32 n,
               int first_shift, int bits, int* cur, u32* low32_out = nullptr, bool* low32_done = nullptr, const u32* first_half_hist = nullptr) {
    constexpr int WAVES = kScatterWaves;
    constexpr int TILE = WAVES * 64 * kItems;
    if (low32_done) *low32_done = false;
    if (n == 0) return 0;
    const u32 n_tiles = (n + TILE - 1) / TILE;
    const u32 n_chunks = (n_tiles + kChunkTiles - 1) / kChunkTiles;
    for (int shift = first_shift; shift < first_shift + bits; shift += 8) {
        const int in = *cur, out = in ^ 1;
        if (first_half_hist && shift == first_shift)
            hipLaunchKernelGGL(k_hist_merge<TILE>, dim3(n_tiles), dim3(256), 0, s, first_half_hist, (n + kBuildBlock - 1) / kBuildBlock, q.hist);
        else {
            hipLaunchKernelGGL(k_radix_hist<TILE>, dim3(n_tiles), dim3(256), 0, s, key[in], n, shift, q.hist);
            c->stats.n_key_hist_launches++;
        }
        hipLaunchKernelGGL(k_radix_chunk_sums, dim3(n_chunks), dim3(256), 0, s, q.hist, n_tiles, q.chunk);
        hipLaunchKernelGGL(k_radix_scan_chunks, dim3(1), dim3(256), 0, s, q.chunk, n_chunks);
        hipLaunchKernelGGL(k_radix_apply, dim3(n_chunks), dim3(256), 0, s, q.hist, n_tiles, q.chunk);
        const bool timing = c->ev_used + 2 <= c->ev_scatter.size();
        if (timing) HIP_TRY(hipEventRecord(c->ev_scatter[c->ev_used], s));
        // q.hist now holds the tile offsets
#define MGX_SCATTER(P64, P32, LOW, K_IN, K_OUT, P64_IN, P64_OUT, P32_IN, P32_OUT)                                                      \
        hipLaunchKernelGGL((k_radix_scatter<P64, P32, WAVES, LOW>), dim3(n_tiles), dim3(WAVES * 64), 0, s, K_IN, K_OUT, P64_IN, P64_OUT, \
                           P32_IN, P32_OUT, n, shift, q.hist, n_tiles)
        if (p64 && !p32)
            MGX_SCATTER(true, false, false, key[in], key[out], p64[in], p64[out], (const u32*)nullptr, (u32*)nullptr);
        else if (p64)
            MGX_SCATTER(true, true, false, key[in], key[out], p64[in], p64[out], p32[in], p32[out]);
        else if (p32)
            MGX_SCATTER(false, true, false, key[in], key[out], (const u64*)nullptr, (u64*)nullptr, p32[in], p32[out]);
        else if (low32_out && shift + 8 >= first_shift + bits) {
            MGX_SCATTER(false, false, true, key[in], key[out], (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, low32_out);
            if (low32_done) *low32_done = true;
        } else
            MGX_SCATTER(false, false, false, key[in], key[out], (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr);
#undef MGX_SCATTER
        if (timing) { HIP_TRY(hipEventRecord(c->ev_scatter[c->ev_used + 1], s)); c->ev_used += 2; }
        c->scatter_bytes += (uint64_t)n * 2 * (8 + (p32 ? 4 : 0) + (p64 ? 8 : 0));
        if (low32_done && *low32_done) c->scatter_bytes -= (uint64_t)n * 4;
        c->stats.n_radix_passes++;
        *cur = out;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

inline u64 tile_aligned(u64 L) { return (L + kIndTile - 1) / kIndTile * kIndTile; }   // where the tiled bitmap's reverse-strand half starts

// Layout of the indicator bitmap for one run: tiled (plain stores, reverse half at a tile-aligned offset) whenever every
// 5' end is safely below L; otherwise the reference's exact layout with global atomics.
struct BitmapPlan {
    bool tiled;
    u64 Lp, ind_off, ind_bits;   // tile_aligned(L); offset of the reverse-strand half; bits of both halves
    u32 n_ind_tiles, n_sub;      // bitmap tiles, entries of the near pass's sub-tile table
};

// duplicate search over one sorted entry array: run heads -> dense list -> marks (+ long runs)
template <bool DOUBLE, bool PK, int KS = 0>
void launch_find(mgx_sortdedup* c, hipStream_t s, const u64* k1, const u64* k2, const u32* rec, u32 n_entries,
                 const mgx_sortdedup::Scratch& q, u32* n_multi, const BitmapPlan& bp, u32* sub_start = nullptr, u32 n_sub = 0) {
    if (!n_entries) return;
    const u32 per = 256 * kFindItems;
    hipLaunchKernelGGL((k_find_runs<DOUBLE, PK, KS>), dim3((n_entries + per - 1) / per), dim3(256), 0, s, k1, k2, rec, n_entries,
                       c->indicator.p, bp.ind_bits, bp.ind_off, c->d_dup, q.multi, n_multi, sub_start, n_sub);
}

template <bool DOUBLE, bool PK, int KS = 0>
void launch_mark(mgx_sortdedup* c, hipStream_t s, const u64* k1, const u64* k2, const u32* rec, u32 n_entries,
                 const mgx_sortdedup::Scratch& q, u32* n_multi, u32* n_long, const BitmapPlan& bp, bool find_done = false,
                 u32 rec_mask = 0xFFFFFFFFu) {
    if (!n_entries) return;
    if (!find_done) launch_find<DOUBLE, PK, KS>(c, s, k1, k2, rec, n_entries, q, n_multi, bp);
    hipLaunchKernelGGL((k_mark_list<DOUBLE, PK, KS>), dim3(c->n_cu * 16), dim3(256), 0, s, k1, k2, rec, n_entries, c->recs.p, c->n,
                       c->indicator.p, bp.ind_bits, bp.ind_off, c->d_dup, q.multi, n_multi, q.longl, n_long, rec_mask);
    if constexpr (KS > kNearScoreBits)
        hipLaunchKernelGGL((k_mark_long_sub<KS>), dim3(c->n_cu * 2), dim3(256), 0, s, k1, rec, n_entries, c->recs.p, c->d_dup, q.longl, n_long,
                           &c->d_sc->huge_runs, rec_mask);
    else
        hipLaunchKernelGGL((k_mark_long<DOUBLE, PK, KS>), dim3(c->n_cu * 2), dim3(256), 0, s, k1, k2, rec, n_entries, c->recs.p,
                           c->indicator.p, bp.ind_bits, bp.ind_off, c->d_dup, q.longl, n_long, rec_mask);
}

// a run-time choice as a template argument: f(std::true_type{}) or f(std::false_type{})
template <class F>
void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// record-END bits of the far pairs into the bitmap: the atomic form, or the tiled one over its tiles with the reverse
// half at Lp.  define: this is the first pass over the tiled bitmap (only the record-2 pass ever is).
template <int END>
void launch_indicator(mgx_sortdedup* c, hipStream_t s, const u64* k1, const u64* k2, u32 nd, const BitmapPlan& bp, bool define = false) {
    with_bool(c->packed_pair, [&](auto pk) {
        constexpr bool PK = decltype(pk)::value;
        if (!bp.tiled) {
            hipLaunchKernelGGL((k_set_indicator<END, PK>), dim3((nd + 255) / 256), dim3(256), 0, s, k1, k2, nd, c->indicator.p, c->indicator_bits, c->L);
        } else if constexpr (END == 2) {
            with_bool(define, [&](auto def) {
                hipLaunchKernelGGL((k_indicator_tiles<2, PK, decltype(def)::value>), dim3(bp.n_ind_tiles), dim3(256), 0, s, k1, k2, nd, c->indicator.p, bp.Lp);
            });
        } else {
            assert(!define);
            hipLaunchKernelGGL((k_indicator_tiles<END, PK, false>), dim3(bp.n_ind_tiles), dim3(256), 0, s, k1, k2, nd, c->indicator.p, bp.Lp);
        }
    });
}

}  // namespace

extern "C" {

int mgx_sortdedup_create(int device, unsigned flags, mgx_sortdedup_t** out) {
    if (!out) { set_error("out is NULL"); return -EINVAL; }
    *out = nullptr;
    static std::atomic<unsigned> next{0};      // MGX_DEVICE_AUTO: contexts are dealt round-robin over the visible GPUs
    if (const int rc = mgx_hip::pick_device(&device, &next)) return rc;
    std::unique_ptr<mgx_sortdedup> c(new (std::nothrow) mgx_sortdedup);
    if (!c) return -ENOMEM;
    c->device = device; c->flags = flags;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount;
    // MGX_STREAM_HIGH_PRIORITY (bit 16): the pipeline's short HBM-bound kernels go ahead of a co-resident PairHMM context's
    const bool high = (flags & (1u << 16)) != 0;
    mgx_hip::Owner& m = c->own;
    m.stream(&c->compute, c->n_cu, (flags >> 8) & 0xFFu, high);
    m.stream(&c->copy, 0, 0, high);
    for (int i = 0; i < 2; ++i) { m.stream(&c->side[i], 0, 0, high); m.event(&c->ev_side[i], hipEventDisableTiming); }
    m.event(&c->ev_ind, hipEventDisableTiming);
    m.device(&c->d_sc, sizeof(Scalars));
    m.event(&c->ev_start); m.event(&c->ev_stop);
    c->ev_scatter.resize(64);
    for (auto& e : c->ev_scatter) m.event(&e);
    for (int i = 0; i < 2; ++i) m.event(&c->pin_ev[i]);   // staging buffers: on first upload
    if (!m.ok()) return m.error("a sort context");
    *out = c.release();
    return 0;
}

void mgx_sortdedup_destroy(mgx_sortdedup_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

}  // extern "C"

namespace {

// device room for `n` records; the first `keep` records already uploaded survive a growth
int ensure_recs(mgx_sortdedup_t* c, size_t n, size_t keep) {
    if (n <= c->recs.cap) return 0;
    const size_t cap = std::max<size_t>(n, keep ? c->recs.cap + c->recs.cap / 2 : 0);
    mgx_hip::DevArray<mgx_rec_t> fresh;
    if (fresh.reserve(cap)) { set_error("out of device memory for %zu records", cap); return -ENOMEM; }
    if (keep && c->recs.p) {
        HIP_TRY(hipMemcpyAsync(fresh.p, c->recs.p, keep * sizeof(mgx_rec_t), hipMemcpyDeviceToDevice, c->copy));
        HIP_TRY(hipStreamSynchronize(c->copy));
    }
    c->recs.swap(fresh);      // the old array goes with `fresh`
    return 0;
}

// bitmap, sub-tile table, work buffers and the per-input decisions shared by all upload forms
int prepare_input(mgx_sortdedup_t* c, uint64_t L, size_t capacity) {
    int rc = ensure_capacity(c, capacity);
    if (rc) { set_error("out of device memory for %zu records", capacity); return rc; }
    // double_pair_indicator: 4L bits like the reference (main.cpp:115), or the two tile-aligned halves
    const uint64_t Lp = tile_aligned(L);
    const uint64_t bits = std::max<uint64_t>(4 * L + 64, 2 * Lp + 2 * (uint64_t)kIndTile);
    if ((rc = c->indicator.reserve((size_t)((bits + 31) / 32)))) return rc;
    if ((rc = c->sub_start.reserve((size_t)(Lp / kNearSpan) + 2))) return rc;
    c->indicator_bits = 4 * L; c->L = L; c->ran = false;
    c->near_by_position = true;             // decided again for every input (see finish_run)
    c->packed_coord = L < 0xFFFFFFFFull;     // coord <= L (bam_record.cpp:18-24)
    c->packed_pair = L < 0xF0000000ull;      // 5' ends <= L + clip; verified against the device maximum
    return 0;
}

int ensure_staging(mgx_sortdedup_t* c, size_t chunk) {
    if (chunk <= c->stage[1].cap) return 0;      // [1] is filled last: both are there or neither
    HIP_TRY(hipStreamSynchronize(c->copy));
    for (auto& st : c->stage) st.release();
    for (auto& st : c->stage) if (const int rc = st.reserve(chunk, chunk)) { c->stage[0].release(); return rc; }
    return 0;
}

// Host memory -> HBM through the two pinned staging buffers on the copy stream (asynchronous; the caller syncs), in pieces
// of as many whole items as a buffer holds; the buffers take turns and one is refilled only after what was last enqueued
// from it has left it (pin_ev).  records: a piece travels in the 24-byte wire form and is expanded on the device whenever
// its values allow it, raw otherwise (MGX_SORTDEDUP_WIRE=32 keeps every piece raw).
int staged_upload(mgx_sortdedup_t* c, void* dst_, const void* src_, size_t n_items, size_t item_bytes, bool records = false) {
    // one core moves ~12 GB/s into the staging buffer, less than a quarter of what the link takes: every piece is
    // split over a gang of threads (MGX_UPLOAD_THREADS, default 4).  Measured on the GPU box, 200 M records, 24-byte
    // wire form (profiles/r02_upload_threads.txt): 4 threads 89.6 ms, 8: 95.9, 12: 97.4, 16: 113.4 -- beyond four the
    // threads only compete for memory bandwidth; raw 32-byte records with 8 threads: 114.9 ms.
    static const int n_thr = [] { const char* e = getenv("MGX_UPLOAD_THREADS"); return std::min(16, std::max(1, e ? atoi(e) : 4)); }();
    static const bool compact_ok = [] { const char* e = getenv("MGX_SORTDEDUP_WIRE"); return !(e && atoi(e) == 32); }();
    const bool wire = records && compact_ok;
    if (!n_items) return 0;
    const size_t total = n_items * item_bytes;
    int rc = ensure_staging(c, std::min(kPinnedChunk, std::max<size_t>((total + 1) / 2, 1u << 20)));
    if (rc) return rc;
    const size_t piece = c->stage[0].cap / item_bytes;
    mgx_stage::Gang gang(total >= (32u << 20) ? n_thr : 1);
    int buf = 0;
    for (size_t off = 0; off < n_items; off += piece, buf ^= 1) {
        const size_t m = std::min(piece, n_items - off), len = m * item_bytes;
        const char* src = static_cast<const char*>(src_) + off * item_bytes;
        char *dst = static_cast<char*>(dst_) + off * item_bytes, *stage = reinterpret_cast<char*>(c->stage[buf].pin);
        HIP_TRY(hipEventSynchronize(c->pin_ev[buf]));
        if (wire && !mgx_stage::pack24(gang, reinterpret_cast<const mgx_rec_t*>(src), m, stage)) {
            HIP_TRY(hipMemcpyAsync(c->stage[buf].dev, stage, m * sizeof(Wire24), hipMemcpyHostToDevice, c->copy));
            hipLaunchKernelGGL(k_expand24, dim3((u32)((m + 255) / 256)), dim3(256), 0, c->copy, (const Wire24*)c->stage[buf].dev, (mgx_rec_t*)dst, (u32)m);
        } else {
            gang.run(len, 4u << 20, [=](size_t a, size_t b) { memcpy(stage + a, src + a, b - a); });
            HIP_TRY(hipMemcpyAsync(dst, stage, len, hipMemcpyHostToDevice, c->copy));
        }
        HIP_TRY(hipEventRecord(c->pin_ev[buf], c->copy));
    }
    return 0;
}

// ---- the stages of mgx_sortdedup_run, in the order it calls them; DESIGN.md 4.2 has the overview ----
// The only host round trip of a run: entry counts and key maxima size the sorts.  A maximum >= 2^32 (a coordinate beyond
// L, a 5' end wrapped below zero) does not fit the packed words: one rebuild, in the wide form of whatever did not fit.
int build_entries(mgx_sortdedup_t* c) {
    hipStream_t s = c->compute;
    const u32 n = c->n, n_order = c->n_order;
    for (int attempt = 0; attempt < 2; ++attempt) {
        c->stats.n_builds = (uint32_t)attempt + 1;
        HIP_TRY(hipMemsetAsync(c->d_sc, 0, sizeof(Scalars), s));
        if (n) {
            HIP_TRY(hipMemsetAsync(c->d_dup, 0, n, s));
            BuildOut o{};
            o.ckey = c->sharded ? nullptr : c->d_ckey[0]; o.cval = c->d_cval[0];      // a shard's order keys come from k_order_keys
            o.dk1 = c->d_k1[0]; o.dk2 = c->d_k2[0]; o.drec = c->d_prec[0]; o.sk1 = c->d_sk1[0]; o.srec = c->d_srec[0]; o.nk = c->d_nk[0]; o.nrec = c->d_nrec[0];
            o.indicator = c->indicator.p; o.indicator_bits = c->indicator_bits; o.L = c->L;
            o.packed_coord = c->packed_coord ? 1 : 0; o.packed_pair = c->packed_pair ? 1 : 0;
            o.near_enabled = c->packed_pair ? 1 : 0;                                  // the one-word near key holds a 32-bit position
            o.mate_flag = n < 0x80000000u ? 0x80000000u : 0u; o.half_hist = c->sharded ? nullptr : c->d_half_hist;
            hipLaunchKernelGGL(k_build_emit, dim3((n + kBuildBlock - 1) / kBuildBlock), dim3(256), 0, s, c->recs.p, n, o, c->d_sc);
            HIP_TRY(hipGetLastError());
        }
        if (c->sharded && n_order)
            hipLaunchKernelGGL(k_order_keys, dim3(std::min<u32>((n_order + 255) / 256, (u32)c->n_cu * 16)), dim3(256), 0, s, c->ocoord.p, c->oarr.p,
                               n_order, c->d_ckey[0], c->d_cval[0], c->packed_coord ? 1 : 0, c->d_sc);
        // the round trip, inside the timed pipeline: the copy queues behind the kernels on their stream, one wait
        HIP_TRY(hipMemcpyAsync(&c->sc, c->d_sc, sizeof(Scalars), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const bool packed_coord = c->packed_coord && c->sc.max_coord < (1ull << 32), packed_pair = c->packed_pair && c->sc.max_k2d < (1ull << 32);
        if (packed_coord == c->packed_coord && packed_pair == c->packed_pair) break;
        c->packed_coord = packed_coord; c->packed_pair = packed_pair;
    }
    if (c->sc.bad_mate) { set_error("a record's mate index is outside the uploaded shard"); return -EINVAL; }
    c->stats.n_double = (uint64_t)c->sc.n_double + c->sc.n_near; c->stats.n_single = c->sc.n_single;     // sc.n_double: far pairs only
    c->stats.key_bits_coord = bits_of(c->sc.max_coord);
    c->stats.key_bits_pair1 = bits_of(std::max<uint64_t>(c->sc.max_k1d, c->sc.max_k1s));
    c->stats.key_bits_pair2 = bits_of(c->sc.max_k2d);
    return 0;
}

// The bitmap's layout for this run.  The atomic layout ORs into its words, so it is cleared here, on the main stream
// ahead of every pass; the tiled one has no memset: the first pass over it stores every word (`define`).
int plan_bitmap(mgx_sortdedup_t* c, BitmapPlan* bp) {
    const uint64_t maxpos = std::max<uint64_t>(c->sc.max_k2d, std::max<uint64_t>(c->sc.max_k1d >> 2, c->sc.max_k1s >> 2));
    const bool tiled = c->L > 64 && maxpos < c->L - 64;
    const u64 Lp = tile_aligned(c->L);
    *bp = BitmapPlan{tiled, Lp, tiled ? Lp : c->L, tiled ? 2 * Lp : c->indicator_bits, (u32)(Lp / kIndTile), (u32)(Lp / kNearSpan)};
    c->stats.bitmap_tiled = tiled ? 1 : 0;
    if (!tiled && c->n) HIP_TRY(hipMemsetAsync(c->indicator.p, 0, (size_t)((c->indicator_bits + 64 + 31) / 32) * 4, c->compute));
    return 0;
}

// Near double pairs (see kNearShift): one sort of (key word, record) makes equal pairs adjacent, all the run search needs.
// Records ev_ind once their ends are in the bitmap and ev_side[0] after the marks.  *defined: it stored every bitmap word.
int near_pass(mgx_sortdedup_t* c, const BitmapPlan& bp, bool multi, bool* defined) {
    hipStream_t sN = (multi && bp.tiled) ? c->side[0] : c->compute;      // atomic bitmap: behind plan_bitmap's memset
    const u32 n = c->n, nn = c->sc.n_near;
    const int near_shift = c->near_by_position ? kNearShift : kNearScoreBits;
    auto with_ks = [c](auto&& f) {
        with_bool(c->near_by_position, [&](auto by_pos) { f(std::integral_constant<int, decltype(by_pos)::value ? kNearShift : kNearScoreBits>{}); });
    };
    int cur = 0;
    int rc = radix_sort(c, sN, c->scr[1], c->d_nk, nullptr, c->d_nrec, nn, near_shift, std::max(bits_of(c->sc.max_near) - near_shift, 1), &cur);
    if (rc) return rc;
    const u64* key = c->d_nk[cur]; const u32* rec = c->d_nrec[cur];
    const bool near_tiles = bp.tiled && n && c->packed_pair;
    u32* sub = near_tiles ? c->sub_start.p : nullptr;
    // run heads first: the same pass over the sorted keys notes where they cross the bitmap's sub-tile boundaries
    if (near_tiles && !nn) HIP_TRY(hipMemsetAsync(sub, 0, ((size_t)bp.n_sub + 1) * 4, sN));
    with_ks([&](auto ks) { launch_find<true, false, decltype(ks)::value>(c, sN, key, nullptr, rec, nn, c->scr[1], &c->d_sc->n_multi_n, bp, sub, bp.n_sub); });
    if (near_tiles)
        hipLaunchKernelGGL(k_indicator_tiles_near, dim3(bp.n_ind_tiles), dim3(256), 0, sN, key, nn, c->indicator.p, bp.Lp, sub, bp.n_sub);
    else if (!bp.tiled && nn)
        hipLaunchKernelGGL(k_set_indicator_near, dim3((nn + 255) / 256), dim3(256), 0, sN, key, nn, c->indicator.p, c->indicator_bits, c->L);
    *defined = near_tiles;
    HIP_TRY(hipEventRecord(c->ev_ind, sN));
    const u32 rec_mask = n < 0x80000000u ? 0x7FFFFFFFu : 0xFFFFFFFFu;      // bit 31 of an entry's record word: "the mate is rec ^ 1"
    u32 *n_multi = &c->d_sc->n_multi_n, *n_long = &c->d_sc->n_long_n;
    with_ks([&](auto ks) { launch_mark<true, false, decltype(ks)::value>(c, sN, key, nullptr, rec, nn, c->scr[1], n_multi, n_long, bp, true, rec_mask); });
    HIP_TRY(hipEventRecord(c->ev_side[0], sN));
    return 0;
}

// Records by unified coordinate (stable: equal coordinates keep arrival order) on side stream 1: order_buf, ev_side[1],
// and the event range and bytes of "the record-sort scatter kernel" for the statistics.
int record_sort(mgx_sortdedup_t* c, bool multi) {
    hipStream_t sR = multi ? c->side[1] : c->compute;
    const u32 n_order = c->n_order;
    const u32* half_hist = c->sharded ? nullptr : c->d_half_hist;      // the build kernel's histogram of the first digit
    const bool pc = c->packed_coord;          // key = coord << 32 | arrival index: sorted on the high half only, 8 bytes per record per pass
    int cur = 0;
    bool unpacked = false;                    // did the last pass store the order directly?
    c->ev_rec_begin = c->ev_used;
    const uint64_t bytes_before = c->scatter_bytes;
    const int rc = radix_sort(c, sR, c->scr[2], c->d_ckey, nullptr, pc ? nullptr : c->d_cval, n_order, pc ? 32 : 0, bits_of(c->sc.max_coord), &cur,
                              pc ? c->d_cval[0] : nullptr, pc ? &unpacked : nullptr, half_hist);
    if (rc) return rc;
    if (pc && n_order && !unpacked) hipLaunchKernelGGL(k_unpack_order, dim3((n_order + 255) / 256), dim3(256), 0, sR, c->d_ckey[cur], n_order, c->d_cval[0]);
    c->order_buf = pc ? 0 : cur;
    c->ev_rec_end = c->ev_used;
    c->rec_scatter_bytes = c->scatter_bytes - bytes_before;
    if (unpacked && c->ev_rec_end >= c->ev_rec_begin + 2) {
        // the statistics cover the full-width launches only; the last one is a different instantiation (half the store bytes)
        c->ev_rec_end -= 2;
        c->rec_scatter_bytes -= (uint64_t)n_order * 12;
    }
    HIP_TRY(hipEventRecord(c->ev_side[1], sR));
    return 0;
}

// Far double pairs (discordant, cross-contig, or all when keys are wider than 32 bits), main stream: LSD by the mate end,
// then by sort_key.  Packed: sort_key and (mate end << 32 | record) take turns as key and payload, 16 B per entry per pass.
int far_pass(mgx_sortdedup_t* c, const BitmapPlan& bp, bool defined) {
    hipStream_t s = c->compute;
    const u32 n = c->n, nd = c->sc.n_double;
    const bool pk = c->packed_pair;
    u32** prec = pk ? nullptr : c->d_prec;
    int cur = 0, rc;
    if ((rc = radix_sort(c, s, c->scr[0], c->d_k2, c->d_k1, prec, nd, pk ? 32 : 0, bits_of(c->sc.max_k2d), &cur))) return rc;
    HIP_TRY(hipStreamWaitEvent(s, c->ev_ind, 0));      // the near pass writes the bitmap's words first
    // tiled: record 2's pass defines the words the near pass has not, and for that runs even without far pairs
    if (bp.tiled ? (n && (nd || !defined)) : nd != 0) launch_indicator<2>(c, s, c->d_k1[cur], c->d_k2[cur], nd, bp, !defined);
    if (n && c->n_marks)      // ends of pairs that live in other shards
        hipLaunchKernelGGL(k_or_marks, dim3((c->n_marks + 255) / 256), dim3(256), 0, s, c->marks.p, c->n_marks, c->indicator.p, bp.ind_bits, bp.ind_off,
                           bp.tiled ? c->L - 64 : ~0ull);
    if ((rc = radix_sort(c, s, c->scr[0], c->d_k1, c->d_k2, prec, nd, 0, bits_of(c->sc.max_k1d), &cur))) return rc;
    if (!nd) return 0;
    launch_indicator<1>(c, s, c->d_k1[cur], c->d_k2[cur], nd, bp);
    with_bool(pk, [&](auto packed) {
        constexpr bool PK = decltype(packed)::value;
        launch_mark<true, PK>(c, s, c->d_k1[cur], c->d_k2[cur], PK ? nullptr : c->d_prec[cur], nd, c->scr[0], &c->d_sc->n_multi_d, &c->d_sc->n_long_d, bp);
    });
    return 0;
}

// Single reads, on the main stream after far_pass: they test the bitmap every pair end is in by now.
int single_pass(mgx_sortdedup_t* c, const BitmapPlan& bp) {
    const u32 ns = c->sc.n_single;
    int cur = 0;
    const int rc = radix_sort(c, c->compute, c->scr[0], c->d_sk1, nullptr, c->d_srec, ns, 0, bits_of(c->sc.max_k1s), &cur);
    if (!rc) launch_mark<false, false>(c, c->compute, c->d_sk1[cur], nullptr, c->d_srec[cur], ns, c->scr[0], &c->d_sc->n_multi_s, &c->d_sc->n_long_s, bp);
    return rc;
}

// Waits for the pipeline, fetches the scalars and applies the one fallback that can only be decided afterwards: a position with
// more near pairs than the in-run comparison accepts sends the input through the pipeline again with the six-pass near sort.
int finish_run(mgx_sortdedup_t* c) {
    while (!c->finished) {
        HIP_TRY(hipStreamSynchronize(c->compute));
        HIP_TRY(hipMemcpy(&c->sc, c->d_sc, sizeof(Scalars), hipMemcpyDeviceToHost));
        c->finished = !(c->sc.huge_runs && c->near_by_position);
        if (c->finished) break;
        c->near_by_position = false;
        const int rc = mgx_sortdedup_run(c);      // leaves finished == false: the scalars are read once more
        if (rc) return rc;
        c->stats.n_pipeline_runs = 2;
    }
    return 0;
}

// total time (and, if asked for, number) of the scatter launches timed by the event pairs [begin, end) of ev_scatter
int sum_event_pairs(const mgx_sortdedup_t* c, size_t begin, size_t end, float* ms_sum, uint32_t* count = nullptr) {
    *ms_sum = 0;
    for (size_t k = begin; k + 1 < end; k += 2) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_scatter[k], c->ev_scatter[k + 1]));
        *ms_sum += ms;
    }
    if (count) *count = (uint32_t)((end - begin) / 2);
    return 0;
}

}  // namespace

extern "C" {

int mgx_sortdedup_upload_begin(mgx_sortdedup_t* c, uint64_t L, uint64_t n_expected) {
    if (!c) { set_error("ctx is NULL"); return -EINVAL; }
    if (n_expected >= 0xFFFFFFF0ull) { set_error("more than 2^32 records in one shard"); return -E2BIG; }
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_recs(c, (size_t)n_expected, 0);
    if (rc) return rc;
    c->up_L = L; c->up_high = 0; c->uploading = true; c->ran = false;
    return 0;
}

int mgx_sortdedup_upload_chunk(mgx_sortdedup_t* c, uint64_t first_record, uint64_t n_records, const mgx_rec_t* recs) {
    if (!c) { set_error("ctx is NULL"); return -EINVAL; }
    if (!c->uploading) { set_error("mgx_sortdedup_upload_begin has not been called"); return -EINVAL; }
    if (n_records && !recs) { set_error("recs is NULL"); return -EINVAL; }
    if (first_record + n_records >= 0xFFFFFFF0ull) { set_error("more than 2^32 records in one shard"); return -E2BIG; }
    if (first_record > c->up_high) {           // a gap would leave records of the device array undefined
        set_error("chunk starts at record %llu but only %llu records have been uploaded", (unsigned long long)first_record, (unsigned long long)c->up_high);
        return -EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_recs(c, (size_t)(first_record + n_records), (size_t)c->up_high);
    if (rc) return rc;
    if ((rc = staged_upload(c, c->recs.p + first_record, recs, (size_t)n_records, sizeof(mgx_rec_t), true))) return rc;
    c->up_high = std::max(c->up_high, first_record + n_records);
    return 0;
}

int mgx_sortdedup_upload_end(mgx_sortdedup_t* c, uint64_t n_records) {
    if (!c) { set_error("ctx is NULL"); return -EINVAL; }
    if (!c->uploading) { set_error("mgx_sortdedup_upload_begin has not been called"); return -EINVAL; }
    if (n_records != c->up_high) { set_error("%llu records announced, chunks covered %llu", (unsigned long long)n_records, (unsigned long long)c->up_high); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    c->uploading = false;
    int rc = prepare_input(c, c->up_L, (size_t)n_records);
    if (rc) return rc;
    c->n = c->n_order = (u32)n_records; c->sharded = false; c->n_marks = 0;
    HIP_TRY(hipStreamSynchronize(c->copy));
    return 0;
}

int mgx_sortdedup_upload(mgx_sortdedup_t* c, uint64_t L, uint64_t n_records, const mgx_rec_t* recs) {
    int rc = mgx_sortdedup_upload_begin(c, L, n_records);
    if (!rc) rc = mgx_sortdedup_upload_chunk(c, 0, n_records, recs);
    if (!rc) rc = mgx_sortdedup_upload_end(c, n_records);
    return rc;
}

int mgx_sortdedup_upload_shard(mgx_sortdedup_t* c, uint64_t L, const mgx_sortdedup_shard_t* sh) {
    if (!c || !sh) { set_error("NULL argument"); return -EINVAL; }
    if (sh->n_order >= 0xFFFFFFF0ull || sh->n_mark >= 0xFFFFFFF0ull || sh->n_marks >= 0xFFFFFFF0ull) { set_error("more than 2^32 entries in one shard"); return -E2BIG; }
    if ((sh->n_order && (!sh->order_coord || !sh->order_arrival)) || (sh->n_mark && (!sh->mark_recs || !sh->mark_arrival)) ||
        (sh->n_marks && !sh->marks)) { set_error("a shard array is NULL (was the shard materialised by mgx_sortdedup_route?)"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    c->uploading = false;
    int rc = ensure_recs(c, (size_t)sh->n_mark, 0);
    if (!rc) rc = prepare_input(c, L, (size_t)std::max(sh->n_order, sh->n_mark));
    if (!rc) rc = c->ocoord.reserve((size_t)sh->n_order);
    if (!rc) rc = c->oarr.reserve((size_t)sh->n_order);
    if (!rc) rc = c->marks.reserve((size_t)sh->n_marks);
    if (rc) return rc;
    c->n = (u32)sh->n_mark; c->n_order = (u32)sh->n_order; c->n_marks = (u32)sh->n_marks; c->sharded = true;
    if ((rc = staged_upload(c, c->recs.p, sh->mark_recs, (size_t)sh->n_mark, sizeof(mgx_rec_t), true))) return rc;
    if ((rc = staged_upload(c, c->ocoord.p, sh->order_coord, (size_t)sh->n_order * 8, 1))) return rc;      // plain bytes
    if ((rc = staged_upload(c, c->oarr.p, sh->order_arrival, (size_t)sh->n_order * 4, 1))) return rc;
    if ((rc = staged_upload(c, c->marks.p, sh->marks, (size_t)sh->n_marks * 8, 1))) return rc;
    HIP_TRY(hipStreamSynchronize(c->copy));
    return 0;
}

// The three sorts are independent: near pairs on side stream 0, records on side stream 1, far pairs and singles on the
// main stream, so their short histogram / scan launches overlap the other sorts' bandwidth-bound scatters: 18.0 ms against
// 19.4 ms on a single stream (MGX_SORTDEDUP_STREAMS=1) at 200 M records, in-process A/B (tools/dev_sort_ab.py).
int mgx_sortdedup_run(mgx_sortdedup_t* c) {
    if (!c) { set_error("ctx is NULL"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    // both switches are read on every run: tests and the benchmark flip them between runs of one process
    if (const char* e = getenv("MGX_SORTDEDUP_NEAR_EXACT")) { if (atoi(e) != 0) c->near_by_position = false; }
    const char* env_streams = getenv("MGX_SORTDEDUP_STREAMS");
    const bool multi = !(env_streams && atoi(env_streams) == 1);
    c->stats = mgx_sortdedup_stats_t{};
    c->stats.n_records = c->n_order; c->stats.n_pipeline_runs = 1;
    c->ev_used = 0; c->scatter_bytes = 0;
    HIP_TRY(hipEventRecord(c->ev_start, c->compute));
    BitmapPlan bp;
    bool defined = false;                     // has a pass already written every word of the tiled bitmap?
    int rc = build_entries(c);
    if (!rc) rc = plan_bitmap(c, &bp);
    if (!rc) rc = near_pass(c, bp, multi, &defined);
    if (!rc) rc = record_sort(c, multi);
    if (!rc) rc = far_pass(c, bp, defined);
    if (!rc) rc = single_pass(c, bp);
    if (rc) return rc;
    // the join: the duplicate count needs the marks of all three chains
    HIP_TRY(hipStreamWaitEvent(c->compute, c->ev_side[0], 0));
    HIP_TRY(hipStreamWaitEvent(c->compute, c->ev_side[1], 0));
    if (c->n) hipLaunchKernelGGL(k_count_dup, dim3(c->n_cu * 4), dim3(256), 0, c->compute, c->d_dup, c->n, c->d_sc);
    HIP_TRY(hipEventRecord(c->ev_stop, c->compute));
    HIP_TRY(hipGetLastError());
    c->ran = true; c->finished = false;
    return 0;
}

int mgx_sortdedup_results(mgx_sortdedup_t* c, uint32_t* out_order, uint8_t* out_dup) {
    if (!c) { set_error("ctx is NULL"); return -EINVAL; }
    if (!c->ran) { set_error("mgx_sortdedup_run has not been called"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = finish_run(c); if (rc) return rc; }
    if (c->n && out_dup) HIP_TRY(hipMemcpyAsync(out_dup, c->d_dup, (size_t)c->n, hipMemcpyDeviceToHost, c->compute));
    if (c->n_order && out_order) HIP_TRY(hipMemcpyAsync(out_order, c->d_cval[c->order_buf], (size_t)c->n_order * 4, hipMemcpyDeviceToHost, c->compute));
    HIP_TRY(hipStreamSynchronize(c->compute));
    return 0;
}

int mgx_sortdedup_stats(mgx_sortdedup_t* c, mgx_sortdedup_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    if (!c->ran) { set_error("mgx_sortdedup_run has not been called"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    int rc = finish_run(c);
    if (rc) return rc;
    mgx_sortdedup_stats_t st = c->stats;
    st.n_dup_records = c->sc.n_dup;
    st.n_near = c->sc.n_near;
    st.n_multi_far = c->sc.n_multi_d; st.n_multi_single = c->sc.n_multi_s; st.n_multi_near = c->sc.n_multi_n;
    st.n_long_far = c->sc.n_long_d; st.n_long_single = c->sc.n_long_s; st.n_long_near = c->sc.n_long_n;
    st.packed_coord = c->packed_coord ? 1 : 0; st.packed_pair = c->packed_pair ? 1 : 0;
    st.near_by_position = c->near_by_position ? 1 : 0;
    HIP_TRY(hipEventElapsedTime(&st.ms_total, c->ev_start, c->ev_stop));
    if ((rc = sum_event_pairs(c, 0, c->ev_used, &st.ms_radix_scatter))) return rc;
    if ((rc = sum_event_pairs(c, c->ev_rec_begin, c->ev_rec_end, &st.ms_scatter_records, &st.n_scatter_records))) return rc;
    st.radix_scatter_bytes = c->scatter_bytes;
    st.scatter_records_bytes = c->rec_scatter_bytes;
    // LSD-8 traffic model, SURVEY.md section 8d
    const uint64_t N = c->n_order, P = (uint64_t)st.n_double + st.n_single;
    const uint64_t pc = (st.key_bits_coord + 7) / 8, pp = (st.key_bits_pair1 + st.key_bits_pair2 + 7) / 8;
    st.alg_bytes = N * (8 + pc * 2 * 12) + P * (16 + pp * 2 * 20) + P * 29 + N;
    *out = st;
    return 0;
}

int mgx_sortdedup_sort_mark(mgx_sortdedup_t* c, uint64_t L, uint64_t n_records, const mgx_rec_t* recs,
                            uint32_t* out_order, uint8_t* out_dup) {
    int rc = mgx_sortdedup_upload(c, L, n_records, recs);
    if (!rc) rc = mgx_sortdedup_run(c);
    if (!rc) rc = mgx_sortdedup_results(c, out_order, out_dup);
    return rc;
}

}  // extern "C"
