// mgx_bam.hip -- BAM input on gfx950 (C ABI: include/mgx_bam.h), DESIGN.md 4.8: where the records of inflated BAM bytes
// start, and the sort / duplicate keys of every record, from bytes that are already in device memory.
//
// Index.  Record i + 1 starts where record i ends, so the chain is serial by nature.  It is cut into tiles of
// MGX_BAM_TILE bytes, and exactness never rests on a guess:
//   k_bam_tiles (speculate)  one wavefront per tile stages the tile and a halo in LDS, GUESSES the first record start in
//                            it (64 offsets per step against the validity rule and what a BAM file can hold, the lowest
//                            hit of a ballot), walks the chain from there to the tile's end out of LDS and leaves the
//                            starts in the tile's slots, with its count, exit offset and status.  The tile that holds
//                            `first` starts there: that entry is exact.
//   k_bam_stitch             one workgroup follows the chain of tiles from `first`: a tile is on the chain when its entry
//                            equals the exit of the tile before it (tiles that a long record spans are empty).  The first
//                            tile that disagrees is marked for a re-walk from its TRUE entry; the pass goes on
//                            optimistically (later tiles' guesses taken for true) and marks what disagrees with that, so
//                            one round repairs every independent miss.  It also sums the counts of the tiles on the chain.
//   k_bam_tiles (re-walk)    the marked tiles again, from the entries the stitch gave them.
//   ... at most kRounds stitch passes; every pass moves the verified frontier past at least one tile, and
//   k_bam_finish             walks serially from the frontier if the last pass still found a disagreement.
//   k_bam_compact            the slots of the tiles on the chain, densely, as rec_off[].
// A pass that marks nothing has verified every entry from `first` by induction: the chain is the host walk's.  No kernel
// waits for another workgroup; every phase is one launch, enqueued without a host round trip (a phase that has nothing
// to do returns at once).
//
// Keys.  k_bam_keys: eight lanes per record read the qualities in 8-byte pieces and compare the name with the previous
// record's, then reduce across the group; the group's first lane takes the rest of the key from key_from of
// bam_record_core.h, as the host and SAM text input do.
//
// Corrupt input is a returned error (the host walk's message), never a fault: every read lies below n, every LDS index
// below the staged range, every slot index below the tile's slot count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "../../include/mgx_bam.h"
#include "bam_record_core.h"
#include "mgx_bgzf_ctx.h"
#include "mgx_hip_util.h"

using mgx::set_error;

namespace {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
using namespace mgx_bam;

constexpr u32 kHalo = 320;                 // >= kMaxNameEnd: a record that starts inside a tile has all a validity check reads in LDS
constexpr u32 kDefaultTile = 16384;     // measured: DESIGN.md 4.8 (index 1.8 ms per 512 MiB; 4096: 4.0, 1024: 14.2, 32768: 1.9)
constexpr u32 kMinTile = 256, kMaxTile = 32768;
constexpr u32 kRounds = 4;                 // stitch passes before the serial finish
constexpr u32 kStitch = mgx_hip::kScanBlock;       // threads (and tiles per step) of the stitch
constexpr u64 kNone = ~0ull;
constexpr u32 kStEnd = 1;                  // the walk met a record that does not count: the chain ends at `exit`
constexpr u32 kStErr = 0x100;              // ... an invalid record at `exit`: | Rule
static_assert(kHalo >= kMaxNameEnd && kHalo % 16 == 0, "halo");

struct BamResult {
    u64 n_records, next, err_off, frontier_cur;
    u32 err_rule;                          // != 0: the counted record at err_off broke this rule
    u32 n_marked, consistent, frontier_tile, frontier_base, n_rewalked, n_rounds, n_redo;
};

struct BamArgs {
    const u8* data; u64 n, first, max_records;
    u32 tile, slots, n_tiles; int32_t n_ref;
    u64* guess; u64* exit; u64* entry;     // per tile: the entry it was walked from, where its walk ended, the entry to re-walk from
    u32* cnt; u32* st; u32* eff; u32* tbase; u32* list; u32* slot;
    BamResult* res;
    u64* rec_off; mgx_bam_key_t* keys;
};

// The chain from `entry` to the end of tile [base, end), read through origin + (offset - base).  Wave-uniform.
__device__ void walk_tile(const u8* origin, u64 base, u64 end, u64 n, u64 entry, u32* slot, u32 n_slots, bool writer, u32* cnt_out, u64* exit_out, u32* st_out) {
    u64 o = entry;
    u32 cnt = 0, st = 0;
    while (o < end) {
        if (o >= n || n - o < 4) { st = kStEnd; break; }
        const u8* p = origin + (o - base);
        const int64_t bs = rd32s(p);
        if (bs > 0 && (u64)bs > n - o - 4) { st = kStEnd; break; }
        const u32 rule = bs < 32 ? (u32)kBlockSize : check_record(p);
        if (rule != kValid) { st = kStErr | rule; break; }
        if (writer && cnt < n_slots) slot[cnt] = (u32)(o - base);
        ++cnt;
        o += 4 + (u64)bs;
    }
    *cnt_out = cnt; *exit_out = o; *st_out = st;
}

// whether what follows a guessed record looks like a record, as far as it lies inside the data
__device__ bool follower_ok(const u8* data, u64 n, u64 at, int32_t n_ref) {
    if (n - at < 4) return true;
    const int32_t bs = rd32s(data + at);
    if (bs < 32 || bs > (int32_t)MGX_BAM_MAX_RECORD) return false;
    if (n - at < kFixed) return true;
    const Fixed f = read_fixed(data + at);
    return check_fixed(f) == kValid && plausible(f, n_ref);
}

// rewalk == 0: every tile, from a guess.  rewalk == 1: the tiles the stitch marked, from the entries it gave.
__global__ __launch_bounds__(64) void k_bam_tiles(BamArgs a, int rewalk) {
    extern __shared__ uint4 lds4[];
    u8* L = (u8*)lds4;
    const u32 lane = threadIdx.x;
    const u32 T = a.tile, staged = T + kHalo;
    u32 n_work = a.n_tiles;
    if (rewalk) {
        if (a.res->consistent) return;
        n_work = a.res->n_marked;
    }
    for (u32 w = blockIdx.x; w < n_work; w += gridDim.x) {
        const u32 t = rewalk ? a.list[w] : w;
        const u64 base = (u64)t * T, end = base + T;
        if (!rewalk && end <= a.first) {                       // before the chain starts
            if (lane == 0) { a.guess[t] = kNone; a.exit[t] = base; a.cnt[t] = 0; a.st[t] = 0; }
            continue;
        }
        __syncthreads();                                       // the LDS served the tile before
        for (u32 i = lane * 16; i < staged; i += 64 * 16) {
            lds4[i / 16] = mgx_hip::load16_below(a.data, base + i, a.n);      // the last bytes of the data: zeros behind them
        }
        __syncthreads();
        u64 entry = kNone;
        if (rewalk) entry = a.entry[t];
        else if (a.first >= base) entry = a.first;             // base <= first < end: exact
        else {
            for (u32 s = 0; s < T && entry == kNone; s += 64) {
                const u64 c = base + s + lane;
                bool hit = false;
                if (c + kFixed <= a.n) {
                    const u8* p = L + (s + lane);
                    const Fixed f = read_fixed(p);
                    if (check_fixed(f) == kValid && plausible(f, a.n_ref) && (u64)f.bs <= a.n - c - 4 && p[kFixed + f.l_read_name - 1] == 0)
                        hit = follower_ok(a.data, a.n, c + 4 + (u64)f.bs, a.n_ref);
                }
                const unsigned long long m = __ballot(hit);
                if (m) entry = base + s + (u32)(__ffsll((long long)m) - 1);
            }
        }
        u32 cnt = 0, st = 0;
        u64 ex = base;
        if (entry != kNone) walk_tile(L, base, end, a.n, entry, a.slot + (u64)t * a.slots, a.slots, lane == 0, &cnt, &ex, &st);
        if (lane == 0) { a.guess[t] = entry; a.exit[t] = ex; a.cnt[t] = cnt; a.st[t] = st; }
    }
}

struct StitchState {
    u64 cur, term_off, f_cur;
    u32 done, sure, total, n_marked, term_st, f_tile, f_base;
};

__device__ void set_result(BamResult* r, u32 total, bool done, u32 term_st, u64 term_off, u64 cur) {
    r->consistent = 1;
    r->n_records = total;
    r->next = done ? term_off : cur;
    if (done && (term_st & kStErr)) { r->err_rule = term_st & 0xffu; r->err_off = term_off; }
}

__global__ __launch_bounds__(kStitch) void k_bam_stitch(BamArgs a) {
    __shared__ u64 g[kStitch], e[kStitch];
    __shared__ u32 c[kStitch], s[kStitch], eff[kStitch], scan[kStitch];
    __shared__ StitchState S;
    const u32 tid = threadIdx.x;
    if (a.res->consistent) return;
    if (tid == 0) { S.cur = a.first; S.term_off = 0; S.f_cur = 0; S.done = 0; S.sure = 1; S.total = 0; S.n_marked = 0; S.term_st = 0; S.f_tile = 0; S.f_base = 0; }
    __syncthreads();
    for (u32 t0 = 0; t0 < a.n_tiles; t0 += kStitch) {
        const u32 t = t0 + tid;
        const bool valid = t < a.n_tiles;
        g[tid] = valid ? a.guess[t] : kNone; e[tid] = valid ? a.exit[t] : 0;
        c[tid] = valid ? a.cnt[t] : 0; s[tid] = valid ? a.st[t] : 0;
        __syncthreads();
        const u64 cur = S.cur;
        const u32 was_done = S.done;
        bool ok = true;
        if (valid) {
            const u64 pe = tid ? e[tid - 1] : cur;
            const u32 ps = tid ? s[tid - 1] : 0;
            ok = ps == 0 && s[tid] == 0 && g[tid] != kNone && g[tid] == pe;
        }
        const bool fast = __syncthreads_and(ok) && !was_done && cur != kNone;
        if (fast) {                                            // every tile of the step continues the one before it
            eff[tid] = c[tid];
        } else if (tid == 0) {
            u64 at = cur;
            u32 run = 0;
            const u32 lim = min(kStitch, a.n_tiles - t0);
            for (u32 i = 0; i < kStitch; ++i) {
                eff[i] = 0;
                if (i >= lim || S.done) continue;
                const u64 te = (u64)(t0 + i + 1) * a.tile;
                if (at == kNone) { if (g[i] == kNone) continue; at = g[i]; }     // optimistic: the next guess taken for true
                if (at >= te) continue;                        // a record spans the tile: no start in it
                if (g[i] == at) {
                    eff[i] = c[i]; run += c[i]; at = e[i];
                    if (s[i]) { S.done = 1; S.term_st = s[i]; S.term_off = e[i]; }
                } else {
                    a.entry[t0 + i] = at; a.list[S.n_marked++] = t0 + i;
                    if (S.sure) { S.sure = 0; S.f_tile = t0 + i; S.f_cur = at; S.f_base = S.total + run; }
                    at = kNone;
                }
            }
            S.cur = at;
        }
        __syncthreads();
        if (fast && tid == 0) S.cur = e[min(kStitch, a.n_tiles - t0) - 1];
        const u32 before = mgx_hip::block_scan_exclusive(eff[tid], scan);
        if (valid) { a.eff[t] = eff[tid]; a.tbase[t] = S.total + before; }
        __syncthreads();
        if (tid == 0) S.total += scan[kStitch - 1];
        __syncthreads();
    }
    if (tid == 0) {
        BamResult* r = a.res;
        r->n_marked = S.n_marked;
        if (S.n_marked == 0) set_result(r, S.total, S.done != 0, S.term_st, S.term_off, S.cur);
        else { r->n_rewalked += S.n_marked; r->n_rounds += 1; r->frontier_tile = S.f_tile; r->frontier_cur = S.f_cur; r->frontier_base = S.f_base; }
    }
}

// The bound on the rounds was reached: one thread walks from the verified frontier to the end.
__global__ __launch_bounds__(64) void k_bam_finish(BamArgs a) {
    if (threadIdx.x != 0 || a.res->consistent) return;
    BamResult* r = a.res;
    u64 cur = r->frontier_cur;
    u32 total = r->frontier_base, walked = 0;
    bool done = false;
    u32 term_st = 0; u64 term_off = 0;
    for (u32 t = r->frontier_tile; t < a.n_tiles; ++t) {
        const u64 base = (u64)t * a.tile, end = base + a.tile;
        u32 cnt = 0, st = 0;
        if (!done && cur < end) {
            u64 ex;
            walk_tile(a.data + base, base, end, a.n, cur, a.slot + (u64)t * a.slots, a.slots, true, &cnt, &ex, &st);
            cur = ex; ++walked;
            if (st) { done = true; term_st = st; term_off = ex; }
        }
        a.eff[t] = cnt; a.tbase[t] = total;
        total += cnt;
    }
    r->n_rewalked += walked; r->n_rounds += 1; r->n_marked = 0;
    set_result(r, total, done, term_st, term_off, cur);
}

__global__ __launch_bounds__(64) void k_bam_compact(BamArgs a) {
    const u32 lane = threadIdx.x;
    for (u32 t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const u32 n = min(a.eff[t], a.slots);
        const u64 at = a.tbase[t], base = (u64)t * a.tile;
        for (u32 k = lane; k < n; k += 64)
            if (at + k < a.max_records) a.rec_off[at + k] = base + a.slot[(u64)t * a.slots + k];
    }
}

constexpr u32 kGroup = 8;                  // lanes per record

__global__ __launch_bounds__(256) void k_bam_keys(BamArgs a) {
    const u64 n = min(a.res->n_records, a.max_records);
    const u32 gl = threadIdx.x % kGroup;
    const u64 n_groups = (u64)gridDim.x * (256 / kGroup);
    for (u64 i = (u64)blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup; i < n; i += n_groups) {
        const u8* p = a.data + a.rec_off[i];                   // a valid record wholly inside n: the index verified it
        const Fixed f = read_fixed(p);
        const u8* name = p + kFixed;
        const u8* cig = name + f.l_read_name;
        const u8* qual = cig + 4ull * f.n_cigar + ((u64)f.l_seq + 1) / 2;
        const u32 l_seq = (u32)f.l_seq;
        u32 score = 0;
        for (u32 j = gl * 8; j < l_seq; j += kGroup * 8) {
            if (j + 8 <= l_seq) {
                u64 v;
                __builtin_memcpy(&v, qual + j, 8);
                for (int k = 0; k < 8; ++k) { const u32 q = (u32)(v >> (8 * k)) & 0xffu; score += q >= 15 ? q : 0u; }
            } else score += score_bytes(qual, j, l_seq);
        }
        u32 eq = 0;
        if (i > 0) {
            const u8* prev = a.data + a.rec_off[i - 1];
            eq = prev[12] == f.l_read_name;
            if (eq) for (u32 j = gl; j + 1 < f.l_read_name; j += kGroup) eq &= (u32)(name[j] == prev[kFixed + j]);
        }
        for (int o = kGroup / 2; o >= 1; o >>= 1) {
            score += (u32)__shfl_xor((int)score, o, 64);
            eq &= (u32)__shfl_xor((int)eq, o, 64);
        }
        if (gl == 0) {
            mgx_bam_key_t k;
            key_from(f, name, cig, (u16)score, (u8)eq, &k);
            a.keys[i] = k;
            if (k.redo) atomicAdd(&a.res->n_redo, 1u);
        }
    }
}

}  // namespace

struct mgx_bam_batch {
    mgx_bgzf_inflate* inflate = nullptr;
    u64 cap = 0, max_records = 0; int32_t n_ref = 0;
    u32 tile = kDefaultTile, slots = 0, max_tiles = 0;
    mgx_hip::Owner own;                                        // of every buffer and event below
    u8* h_in = nullptr; u8* d_in = nullptr;                    // a buffer of its own, when not attached
    BamArgs a{};                                               // the device arrays
    BamResult* h_res = nullptr; u64* h_rec_off = nullptr; mgx_bam_key_t* h_keys = nullptr;     // pinned
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev_res = nullptr, ev_done = nullptr;
    u64 n = 0; u32 n_tiles = 0;
    bool submitted = false;
};

extern "C" {

void mgx_bam_batch_destroy(mgx_bgzf_t* c, mgx_bam_batch_t* b) {
    if (!b) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->copy); }
    delete b;                                                  // its owner frees
}

int mgx_bam_batch_create(mgx_bgzf_t* c, mgx_bgzf_inflate_t* inflate, uint64_t byte_capacity, uint64_t max_records, int32_t n_ref, mgx_bam_batch_t** out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = nullptr;
    if (max_records >= 0xFFFFFFFFull) { set_error("more than 2^32-1 records in a BAM batch"); return -E2BIG; }
    if (n_ref < 0) { set_error("n_ref is %d", n_ref); return -EINVAL; }
    u32 tile = kDefaultTile;
    if (const char* e = getenv("MGX_BAM_TILE")) {
        const long long v = atoll(e);
        if (v < kMinTile || v > kMaxTile || (v & (v - 1))) { set_error("MGX_BAM_TILE=%s is not a power of two from %u to %u", e, kMinTile, kMaxTile); return -EINVAL; }
        tile = (u32)v;
    }
    if (inflate) byte_capacity = std::min<u64>(byte_capacity, inflate->out_cap);
    if (byte_capacity / tile >= 0xFFFFFFF0ull) { set_error("a BAM batch of %llu bytes", (unsigned long long)byte_capacity); return -E2BIG; }
    HIP_TRY(hipSetDevice(c->device));
    mgx_bam_batch* b = new (std::nothrow) mgx_bam_batch;
    if (!b) { set_error("out of memory"); return -ENOMEM; }
    b->inflate = inflate; b->cap = byte_capacity; b->max_records = max_records; b->n_ref = n_ref;
    b->tile = tile; b->slots = tile / kMinRecord + 1; b->max_tiles = (u32)((byte_capacity + tile - 1) / tile);
    const size_t nt = std::max<u32>(b->max_tiles, 1), nr = std::max<u64>(max_records, 1);
    mgx_hip::Owner& m = b->own;
    if (!inflate) { m.pin(&b->h_in, byte_capacity + 16); m.device(&b->d_in, byte_capacity + 16); }
    m.device(&b->a.guess, nt * 8); m.device(&b->a.exit, nt * 8); m.device(&b->a.entry, nt * 8);
    m.device(&b->a.cnt, nt * 4); m.device(&b->a.st, nt * 4); m.device(&b->a.eff, nt * 4); m.device(&b->a.tbase, nt * 4); m.device(&b->a.list, nt * 4);
    m.device(&b->a.slot, nt * b->slots * 4); m.device(&b->a.res, sizeof(BamResult));
    m.device(&b->a.rec_off, nr * 8); m.device(&b->a.keys, nr * sizeof(mgx_bam_key_t));
    m.pin(&b->h_res, sizeof(BamResult)); m.pin(&b->h_rec_off, nr * 8); m.pin(&b->h_keys, nr * sizeof(mgx_bam_key_t));
    m.event(&b->ev0); m.event(&b->ev1); m.event(&b->ev2); m.event(&b->ev_res, hipEventDisableTiming); m.event(&b->ev_done, hipEventDisableTiming);
    if (!m.ok()) {
        set_error("allocation failed for a BAM batch of %llu bytes, %llu records", (unsigned long long)byte_capacity, (unsigned long long)max_records);
        mgx_bam_batch_destroy(c, b);
        return -ENOMEM;
    }
    *out = b;
    return 0;
}

uint8_t* mgx_bam_batch_input(mgx_bam_batch_t* b) { return b ? b->h_in : nullptr; }

int mgx_bam_batch_submit(mgx_bgzf_t* c, mgx_bam_batch_t* b, uint64_t n_bytes, uint64_t first) {
    if (!c || !b) { set_error("NULL argument"); return -EINVAL; }
    if (b->submitted) { set_error("BAM batch submitted twice without a wait"); return -EINVAL; }
    if (n_bytes > b->cap) { set_error("%llu bytes in a BAM batch made for %llu", (unsigned long long)n_bytes, (unsigned long long)b->cap); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    BamArgs a = b->a;
    a.n = n_bytes; a.first = first; a.max_records = b->max_records; a.tile = b->tile; a.slots = b->slots; a.n_ref = b->n_ref;
    a.n_tiles = (u32)((n_bytes + b->tile - 1) / b->tile);
    if (b->inflate) a.data = b->inflate->d_out;
    else { a.data = b->d_in; if (n_bytes) HIP_TRY(hipMemcpyAsync(b->d_in, b->h_in, n_bytes, hipMemcpyHostToDevice, s)); }
    b->n = n_bytes; b->n_tiles = a.n_tiles;
    HIP_TRY(hipMemsetAsync(a.res, 0, sizeof(BamResult), s));
    HIP_TRY(hipEventRecord(b->ev0, s));
    const u32 wide = (u32)c->n_cu * 16;
    const size_t lds = b->tile + kHalo;
    if (a.n_tiles) hipLaunchKernelGGL(k_bam_tiles, dim3(std::min(a.n_tiles, wide)), dim3(64), lds, s, a, 0);
    for (u32 r = 0; r < kRounds; ++r) {
        if (r && a.n_tiles) hipLaunchKernelGGL(k_bam_tiles, dim3(std::min(a.n_tiles, 1024u)), dim3(64), lds, s, a, 1);
        hipLaunchKernelGGL(k_bam_stitch, dim3(1), dim3(kStitch), 0, s, a);
    }
    hipLaunchKernelGGL(k_bam_finish, dim3(1), dim3(64), 0, s, a);
    if (a.n_tiles) hipLaunchKernelGGL(k_bam_compact, dim3(std::min(a.n_tiles, wide)), dim3(64), 0, s, a);
    HIP_TRY(hipEventRecord(b->ev1, s));
    hipLaunchKernelGGL(k_bam_keys, dim3(wide), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev2, s));
    HIP_TRY(hipMemcpyAsync(b->h_res, a.res, sizeof(BamResult), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(b->ev_res, s));
    b->submitted = true;
    return 0;
}

int mgx_bam_batch_wait(mgx_bgzf_t* c, mgx_bam_batch_t* b, const uint64_t** rec_off, const mgx_bam_key_t** keys, uint64_t* n_records, uint64_t* next) {
    if (!c || !b || !rec_off || !keys || !n_records || !next) { set_error("NULL argument"); return -EINVAL; }
    if (!b->submitted) { set_error("BAM batch was not submitted"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    b->submitted = false;
    *rec_off = b->h_rec_off; *keys = b->h_keys; *n_records = 0; *next = 0;
    HIP_TRY(hipEventSynchronize(b->ev_res));
    const BamResult r = *b->h_res;
    {
        std::lock_guard<std::mutex> g(c->bam_mu);
        c->bam_tiles = b->n_tiles; c->bam_rewalked = r.n_rewalked; c->bam_redo = r.n_redo; c->bam_rounds = r.n_rounds;
        float ms = 0;
        c->bam_ms_index = hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess ? ms : 0;
        c->bam_ms_keys = hipEventElapsedTime(&ms, b->ev1, b->ev2) == hipSuccess ? ms : 0;
    }
    if (!r.consistent) { set_error("the BAM index did not complete"); return -EIO; }
    *next = r.next;
    if (r.n_records > b->max_records) {
        set_error("%llu records in a BAM batch made for %llu", (unsigned long long)r.n_records, (unsigned long long)b->max_records);
        return -E2BIG;
    }
    *n_records = r.n_records;
    if (r.n_records) {                                         // behind the kernels, which have ended: the sizes are known only now
        HIP_TRY(hipMemcpyAsync(b->h_rec_off, b->a.rec_off, r.n_records * 8, hipMemcpyDeviceToHost, c->copy));
        HIP_TRY(hipMemcpyAsync(b->h_keys, b->a.keys, r.n_records * sizeof(mgx_bam_key_t), hipMemcpyDeviceToHost, c->copy));
        HIP_TRY(hipEventRecord(b->ev_done, c->copy));
        HIP_TRY(hipEventSynchronize(b->ev_done));
    }
    if (r.err_rule) {
        set_error("BAM record at offset %llu: %s", (unsigned long long)r.err_off, rule_text(r.err_rule));
        return -EBADMSG;
    }
    return 0;
}

int mgx_bam_scan(mgx_bgzf_t* c, const uint8_t* data, uint64_t n, uint64_t first, int32_t n_ref, uint64_t max_records, uint64_t* rec_off,
                 mgx_bam_key_t* keys, uint64_t* n_records, uint64_t* next) {
    if (!c || !n_records || !next || (n && !data) || (max_records && (!rec_off || !keys))) { set_error("NULL argument"); return -EINVAL; }
    mgx_bam_batch_t* b = nullptr;
    int rc = mgx_bam_batch_create(c, nullptr, n, max_records, n_ref, &b);
    if (rc) return rc;
    if (n) memcpy(b->h_in, data, n);
    rc = mgx_bam_batch_submit(c, b, n, first);
    if (!rc) {
        const uint64_t* ro; const mgx_bam_key_t* k;
        rc = mgx_bam_batch_wait(c, b, &ro, &k, n_records, next);
        if ((rc == 0 || rc == -EBADMSG) && *n_records) { memcpy(rec_off, ro, *n_records * 8); memcpy(keys, k, *n_records * sizeof(mgx_bam_key_t)); }
    }
    return mgx_hip::keep_error(rc, [&] { mgx_bam_batch_destroy(c, b); });
}

int mgx_bam_stats(mgx_bgzf_t* c, mgx_bam_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    std::lock_guard<std::mutex> g(c->bam_mu);
    out->n_tiles = c->bam_tiles; out->n_tiles_rewalked = c->bam_rewalked; out->n_redo = c->bam_redo; out->n_rounds = c->bam_rounds;
    out->ms_index = c->bam_ms_index; out->ms_keys = c->bam_ms_keys;
    return 0;
}

}  // extern "C"
