// mgx_sam.hip -- SAM text input on gfx950 (C ABI: include/mgx_sam.h), DESIGN.md 4.9: the alignment lines of SAM text as
// BAM records with their sort / duplicate keys, by the rule set of sam_line_core.h, which the host implementation
// (sam_host.cpp) compiles too and which defines the result.
//
// The phases of a submit, each a launch (the scans three: mgx_scan.h), enqueued without a host round trip; no kernel waits for
// another workgroup:
//   k_sam_lines (count)   one wavefront per tile of MGX_SAM_TILE bytes, 16 bytes per lane and step (1 KiB per wavefront
//                         load).  A lane sees the two bytes before and the byte after its 16 through its neighbours'
//                         registers (__shfl), the edge lanes through one more load: enough to tell where a non-empty
//                         line starts and where one ends (empty lines and a trailing CR are resolved here).  A line
//                         belongs to the tile where it starts, its end to the tile where it ends; both are counted.
//   scan                  exclusive, over the tiles' two counts in one 64-bit word.
//   k_sam_lines (write)   the same predicates again: line_off[] and line_end[], densely.
//   k_sam_line (size)     a group of 16 lanes per line stages the line in LDS with 16-byte loads and runs scan_line on
//                         it out of LDS: the BAM size, or 0 for a declined line (also: longer than the staging buffer).
//   scan                  exclusive, over the sizes: rec_off[] and the total.
//   k_sam_line (encode)   the same staging; all lanes of the group run encode_line on the same bytes, so they stay
//                         together: lane 0 stores the short serial pieces (fixed part, CIGAR, tag headers), all 16
//                         store the long runs (name, bases, qualities, Z / H values) in pieces of 8 bytes.
//   k_sam_keys            record_key() of bam_record_core.h on the record just written, one lane per line; same_qname
//                         is taken from the text, and a declined line's key says so.
//
// Malformed text is a declined line, never a fault: every global read lies below n, every LDS index inside the staged
// line (scan_line and encode_line index the line by offsets below its length), every store below the record's offset
// plus its size (Writer checks each one against the size the scan gave).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "../../include/mgx_sam.h"
#include "bam_record_core.h"
#include "mgx_bgzf_ctx.h"
#include "mgx_scan.h"
#include "sam_host.h"
#include "sam_line_core.h"

using mgx::set_error;

namespace {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
using namespace mgx_sam;
using namespace mgx_hip;

constexpr u32 kDefaultTile = 16384, kMinTile = 256, kMaxTile = 32768;      // not measured against each other
constexpr u32 kGroup = 16;                 // lanes per line (eight were not measured against it)
constexpr u32 kBlock = 256, kGroups = kBlock / kGroup;
constexpr u32 kStage16 = (kMaxLine + 15 + 15) / 16 + 1;                     // 16-byte pieces of a staged line at any alignment

struct SamResult { u64 n_lines, n_ends, n_out; u32 n_declined, pad; };

struct SamArgs {
    const u8* text; u64 n, max_records, out_cap;
    u32 tile, n_tiles;
    const u32* table;
    u64* tile_cnt; u64* tile_base;         // per tile: starts | ends << 32; its exclusive scan (n_tiles + 1 entries)
    u64* part;                             // the scans' per-workgroup sums
    u64* line_off; u64* line_end; u32* line_len; u32* size; u64* rec_off;
    u8* out; mgx_bam_key_t* keys; SamResult* res;
};

// 24 bytes of text around a lane's 16: the dword before, the 16, the dword after
struct Window {
    u32 w[6]; u64 base;                    // base: the text offset of w[0]'s first byte (may be "negative": never indexed there)
    __device__ u8 operator()(u64 i) const { const u32 k = (u32)(i - base); return (u8)(w[k >> 2] >> (8 * (k & 3))); }
};

// pass 0: the counts of every tile.  pass 1: the dense arrays, from the scanned counts.
__global__ __launch_bounds__(64) void k_sam_lines(SamArgs a, int pass) {
    const u32 lane = threadIdx.x;
    for (u32 t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const u64 base = (u64)t * a.tile;
        const u64 lim = min(base + a.tile, a.n + 1);           // positions [base, lim) are this tile's; position n can end a line
        u32 n_start = 0, n_end = 0;                            // pass 0: this lane's; pass 1: the tile's so far
        u64 at_start = 0, at_end = 0;
        if (pass) { const u64 b = a.tile_base[t]; at_start = b & 0xFFFFFFFFu; at_end = b >> 32; }
        for (u32 s = 0; s < a.tile; s += 64 * 16) {
            const u64 g = base + s + (u64)lane * 16;
            const uint4 v = load16_below(a.text, g, a.n);
            u32 before = (u32)__shfl_up((int)v.w, 1, 64), after = (u32)__shfl_down((int)v.x, 1, 64);
            if (lane == 0) before = (g >= 4 && g <= a.n) ? *(const u32*)(a.text + g - 4) : 0u;    // g is a multiple of 16: bytes [g - 4, g) lie below n
            if (lane == 63) after = g + 16 < a.n ? (u32)a.text[g + 16] : 0u;
            Window win;
            win.w[0] = before; win.w[1] = v.x; win.w[2] = v.y; win.w[3] = v.z; win.w[4] = v.w; win.w[5] = after; win.base = g - 4;
            u32 m_start = 0, m_end = 0;
#pragma unroll
            for (u32 j = 0; j < 16; ++j) {
                const u64 p = g + j;
                if (p < lim) {
                    if (line_starts(win, p, a.n)) m_start |= 1u << j;
                    if (line_ends(win, p, a.n)) m_end |= 1u << j;
                }
            }
            if (!pass) { n_start += __popc(m_start); n_end += __popc(m_end); continue; }
            // the lanes' counts -> each lane's place in the step (inclusive scan over the wavefront, both counts in one word)
            const u32 mine = __popc(m_start) | __popc(m_end) << 16;
            u32 incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const u32 o = (u32)__shfl_up((int)incl, d, 64); if (lane >= (u32)d) incl += o; }
            const u32 total = (u32)__shfl((int)incl, 63, 64);
            u64 ks = at_start + n_start + ((incl - mine) & 0xFFFFu), ke = at_end + n_end + ((incl - mine) >> 16);
#pragma unroll
            for (u32 j = 0; j < 16; ++j) {
                if (m_start >> j & 1) { if (ks < a.max_records) a.line_off[ks] = g + j; ++ks; }
                if (m_end >> j & 1) { if (ke < a.max_records) a.line_end[ke] = g + j - (win(g + j - 1) == '\r' ? 1 : 0); ++ke; }
            }
            n_start += total & 0xFFFFu; n_end += total >> 16;
        }
        if (!pass) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { n_start += (u32)__shfl_xor((int)n_start, o, 64); n_end += (u32)__shfl_xor((int)n_end, o, 64); }
            if (lane == 0) a.tile_cnt[t] = (u64)n_start | (u64)n_end << 32;
        }
    }
}

// the tile scan's total is the number of lines
__global__ void k_sam_counts(SamArgs a) {
    if (threadIdx.x || blockIdx.x) return;
    const u64 t = a.tile_base[a.n_tiles];
    a.res->n_lines = t & 0xFFFFFFFFu; a.res->n_ends = t >> 32;
}

__global__ void k_sam_total(SamArgs a) {
    if (threadIdx.x || blockIdx.x) return;
    a.res->n_out = a.rec_off[min(a.res->n_lines, a.max_records)];
}

// Line i of the group into its LDS region with 16-byte loads; the line's first byte lands at the returned offset
// (the line keeps its alignment modulo 16).  len <= kMaxLine.
__device__ u32 stage_line(const SamArgs& a, u64 off, u32 len, uint4* S, u32 gl) {
    const u64 a0 = off & ~15ull;
    const u32 o = (u32)(off - a0);
    for (u32 c = gl * 16; c < o + len; c += kGroup * 16) {
        const u64 g = a0 + c;
        const uint4 v = load16_below(a.text, g, a.n);
        S[c / 16] = v;                                         // c / 16 < kStage16: c < 15 + kMaxLine
    }
    return o;
}

// encode == 0: size and validate.  encode == 1: write the accepted lines at their offsets.
__global__ __launch_bounds__(kBlock) void k_sam_line(SamArgs a, int encode) {
    __shared__ uint4 stage[kGroups][kStage16];
    if (a.res->n_lines != a.res->n_ends) return;               // cannot happen; the host reports it.  Uniform.
    const u64 n = min(a.res->n_lines, a.max_records);
    if (encode && a.rec_off[n] > a.out_cap) return;            // cannot happen either (size_bound)
    const u32 grp = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
    const Table table = table_view(a.table);
    const u64 per_pass = (u64)gridDim.x * kGroups;
    for (u64 i0 = (u64)blockIdx.x * kGroups; i0 < n; i0 += per_pass) {       // uniform over the workgroup
        const u64 i = i0 + grp;
        const bool have = i < n;
        u64 off = 0; u32 len = 0;
        bool fits = false;
        if (have) {
            off = a.line_off[i];
            const u64 end = a.line_end[i];
            fits = off < end && end <= a.n && end - off <= kMaxLine;      // the first two always hold
            len = fits ? (u32)(end - off) : 0;
        }
        u32 o = 0;
        if (fits && (!encode || a.size[i])) o = stage_line(a, off, len, stage[grp], gl);
        __syncthreads();
        if (have) {
            const u8* s = (const u8*)stage[grp] + o;
            if (!encode) {
                if (gl == 0) {
                    Line L;
                    L.size = 0;
                    if (fits) scan_line(s, len, table, kMaxLine, &L);
                    a.size[i] = L.size;
                    a.line_len[i] = (u32)min(a.line_end[i] - off, (u64)0xFFFFFFFFu);
                    if (L.size == 0) atomicAdd(&a.res->n_declined, 1u);
                }
            } else if (fits && a.size[i]) {
                Line L;
                if (scan_line(s, len, table, kMaxLine, &L) && L.size == a.size[i] && a.rec_off[i] + L.size <= a.out_cap) {
                    Writer w = {a.out + a.rec_off[i], 0, L.size, gl, kGroup};
                    encode_line(s, len, L, w);
                }
            }
        }
        __syncthreads();                                       // the LDS serves the next lines
    }
}

__global__ __launch_bounds__(kBlock) void k_sam_keys(SamArgs a) {
    if (a.res->n_lines != a.res->n_ends) return;
    const u64 n = min(a.res->n_lines, a.max_records);
    if (a.rec_off[n] > a.out_cap) return;
    for (u64 i = (u64)blockIdx.x * kBlock + threadIdx.x; i < n; i += (u64)gridDim.x * kBlock) {
        mgx_bam_key_t k;
        k.d5 = 0; k.tid = 0; k.pos = 0; k.end = 0; k.flag = 0; k.score = 0; k.tile = 0; k.x = 0; k.y = 0; k.same_qname = 0; k.redo = kRedoDeclined;
        const u8* rec = a.out + a.rec_off[i];
        // the record k_sam_line wrote: record_key reads what the record's own lengths say, so they are checked against its size
        if (a.size[i] >= mgx_bam::kMinRecord && (u32)mgx_bam::rd32(rec) + 4 == a.size[i] && mgx_bam::check_record(rec) == mgx_bam::kValid)
            mgx_bam::record_key(rec, nullptr, &k);
        // same_qname from the text: every read lies inside a line, below n
        u8 same = 0;
        if (i > 0 && a.line_off[i - 1] < a.line_end[i - 1] && a.line_end[i - 1] <= a.line_off[i] && a.line_off[i] < a.line_end[i] && a.line_end[i] <= a.n)
            same = same_qname(a.text + a.line_off[i], (u32)(a.line_end[i] - a.line_off[i]), a.text + a.line_off[i - 1], (u32)(a.line_end[i - 1] - a.line_off[i - 1])) ? 1 : 0;
        k.same_qname = same;
        a.keys[i] = k;
    }
}

}  // namespace

struct mgx_sam_batch {
    u64 cap = 0, max_records = 0, out_cap = 0;
    u32 tile = kDefaultTile, max_tiles = 0;
    hipStream_t stream = nullptr;
    mgx_hip::Owner own;                                        // of every buffer and event below
    u8* h_in = nullptr; u8* d_in = nullptr; u32* d_table = nullptr;
    SamArgs a{};
    SamResult* h_res = nullptr; u64* h_line_off = nullptr; u32* h_line_len = nullptr; u64* h_rec_off = nullptr; mgx_bam_key_t* h_keys = nullptr;
    u8* h_out = nullptr;                                       // pinned, allocated by the first wait that asks for the bytes
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr, ev_res = nullptr;
    u64 n = 0; u32 n_tiles = 0;
    bool submitted = false;
};

extern "C" {

void mgx_sam_batch_destroy(mgx_bgzf_t* c, mgx_sam_batch_t* b) {
    if (!b) return;
    if (c) (void)hipSetDevice(c->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    b->own.release();
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int mgx_sam_batch_create(mgx_bgzf_t* c, const mgx_sam_table_t* table, uint64_t text_capacity, uint64_t max_records, mgx_sam_batch_t** out) {
    if (!c || !table || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = nullptr;
    if (text_capacity >= 0xFFFFFF00ull) { set_error("a SAM batch of %llu bytes (at most 2^32 - 256)", (unsigned long long)text_capacity); return -E2BIG; }
    if (max_records >= 0xFFFFFFFFull) { set_error("more than 2^32-1 lines in a SAM batch"); return -E2BIG; }
    u32 tile = kDefaultTile;
    if (const char* e = getenv("MGX_SAM_TILE")) {
        const long long v = atoll(e);
        if (v < kMinTile || v > kMaxTile || (v & (v - 1))) { set_error("MGX_SAM_TILE=%s is not a power of two from %u to %u", e, kMinTile, kMaxTile); return -EINVAL; }
        tile = (u32)v;
    }
    HIP_TRY(hipSetDevice(c->device));
    mgx_sam_batch* b = new (std::nothrow) mgx_sam_batch;
    if (!b) { set_error("out of memory"); return -ENOMEM; }
    b->cap = text_capacity; b->max_records = max_records; b->tile = tile;
    b->out_cap = MGX_SAM_OUT_BOUND(max_records, text_capacity);
    b->max_tiles = (u32)(text_capacity / tile + 1);            // position n is one: see k_sam_lines
    const size_t nt = b->max_tiles, nr = std::max<u64>(max_records, 1);
    const size_t n_part = std::max(nt, nr) / kScanChunk + 2;
    mgx_hip::Owner& m = b->own;
    m.note(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking), "hipStreamCreate");
    m.pin(&b->h_in, text_capacity + 16); m.device(&b->d_in, text_capacity + 16);
    m.device(&b->d_table, table->blob.size() * 4);
    m.device(&b->a.tile_cnt, nt * 8); m.device(&b->a.tile_base, (nt + 1) * 8); m.device(&b->a.part, n_part * 8);
    m.device(&b->a.line_off, nr * 8); m.device(&b->a.line_end, nr * 8); m.device(&b->a.line_len, nr * 4); m.device(&b->a.size, nr * 4); m.device(&b->a.rec_off, (nr + 1) * 8);
    m.device(&b->a.out, b->out_cap + 16); m.device(&b->a.keys, nr * sizeof(mgx_bam_key_t)); m.device(&b->a.res, sizeof(SamResult));
    m.pin(&b->h_res, sizeof(SamResult)); m.pin(&b->h_line_off, nr * 8); m.pin(&b->h_line_len, nr * 4); m.pin(&b->h_rec_off, (nr + 1) * 8); m.pin(&b->h_keys, nr * sizeof(mgx_bam_key_t));
    m.event(&b->ev0); m.event(&b->ev1); m.event(&b->ev2); m.event(&b->ev3); m.event(&b->ev_res, hipEventDisableTiming);
    if (m.ok()) m.note(hipMemcpy(b->d_table, table->blob.data(), table->blob.size() * 4, hipMemcpyHostToDevice), "hipMemcpy");
    if (!m.ok()) {
        set_error("allocation failed for a SAM batch of %llu bytes, %llu lines", (unsigned long long)text_capacity, (unsigned long long)max_records);
        mgx_sam_batch_destroy(c, b);
        return -ENOMEM;
    }
    b->a.text = b->d_in; b->a.table = b->d_table;
    *out = b;
    return 0;
}

uint8_t* mgx_sam_batch_input(mgx_sam_batch_t* b) { return b ? b->h_in : nullptr; }
uint64_t mgx_sam_batch_device_records(mgx_sam_batch_t* b) { return b ? (uint64_t)(uintptr_t)b->a.out : 0; }

int mgx_sam_batch_submit(mgx_bgzf_t* c, mgx_sam_batch_t* b, uint64_t n_bytes) {
    if (!c || !b) { set_error("NULL argument"); return -EINVAL; }
    if (b->submitted) { set_error("SAM batch submitted twice without a wait"); return -EINVAL; }
    if (n_bytes > b->cap) { set_error("%llu bytes in a SAM batch made for %llu", (unsigned long long)n_bytes, (unsigned long long)b->cap); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = b->stream;
    SamArgs a = b->a;
    a.n = n_bytes; a.max_records = b->max_records; a.out_cap = b->out_cap; a.tile = b->tile;
    a.n_tiles = (u32)(n_bytes / b->tile + 1);
    b->n = n_bytes; b->n_tiles = a.n_tiles;
    if (n_bytes) HIP_TRY(hipMemcpyAsync(b->d_in, b->h_in, n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(a.res, 0, sizeof(SamResult), s));
    HIP_TRY(hipEventRecord(b->ev0, s));
    const u32 wide = (u32)c->n_cu * 8;
    hipLaunchKernelGGL(k_sam_lines, dim3(std::min(a.n_tiles, wide * 4)), dim3(64), 0, s, a, 0);
    scan_exclusive(s, ScanArray<u64>{a.tile_cnt}, nullptr, a.n_tiles, a.part, a.tile_base);
    hipLaunchKernelGGL(k_sam_counts, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_sam_lines, dim3(std::min(a.n_tiles, wide * 4)), dim3(64), 0, s, a, 1);
    HIP_TRY(hipEventRecord(b->ev1, s));
    hipLaunchKernelGGL(k_sam_line, dim3(wide), dim3(kBlock), 0, s, a, 0);
    scan_exclusive(s, ScanArray<u32>{a.size}, &a.res->n_lines, b->max_records, a.part, a.rec_off);
    hipLaunchKernelGGL(k_sam_total, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_sam_line, dim3(wide), dim3(kBlock), 0, s, a, 1);
    HIP_TRY(hipEventRecord(b->ev2, s));
    hipLaunchKernelGGL(k_sam_keys, dim3(wide), dim3(kBlock), 0, s, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev3, s));
    HIP_TRY(hipMemcpyAsync(b->h_res, a.res, sizeof(SamResult), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(b->ev_res, s));
    b->submitted = true;
    return 0;
}

int mgx_sam_batch_wait(mgx_bgzf_t* c, mgx_sam_batch_t* b, const uint64_t** line_off, const uint32_t** line_len, const uint64_t** rec_off,
                       const mgx_bam_key_t** keys, uint64_t* n_lines, uint64_t* n_bytes_out, const uint8_t** bam) {
    if (!c || !b || !line_off || !line_len || !rec_off || !keys || !n_lines || !n_bytes_out) { set_error("NULL argument"); return -EINVAL; }
    if (!b->submitted) { set_error("SAM batch was not submitted"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    b->submitted = false;
    *line_off = b->h_line_off; *line_len = b->h_line_len; *rec_off = b->h_rec_off; *keys = b->h_keys; *n_lines = 0; *n_bytes_out = 0;
    if (bam) *bam = nullptr;
    HIP_TRY(hipEventSynchronize(b->ev_res));
    const SamResult r = *b->h_res;
    {
        std::lock_guard<std::mutex> g(c->sam_mu);
        c->sam_lines = r.n_lines; c->sam_declined = r.n_declined; c->sam_bytes_in = b->n; c->sam_bytes_out = r.n_out; c->sam_tiles = b->n_tiles;
        float ms = 0;
        c->sam_ms_lines = hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess ? ms : 0;
        c->sam_ms_encode = hipEventElapsedTime(&ms, b->ev1, b->ev2) == hipSuccess ? ms : 0;
        c->sam_ms_keys = hipEventElapsedTime(&ms, b->ev2, b->ev3) == hipSuccess ? ms : 0;
    }
    if (r.n_lines != r.n_ends) { set_error("the line finder counted %llu starts and %llu ends", (unsigned long long)r.n_lines, (unsigned long long)r.n_ends); return -EIO; }
    if (r.n_lines > b->max_records) {
        set_error("%llu lines in a SAM batch made for %llu", (unsigned long long)r.n_lines, (unsigned long long)b->max_records);
        return -E2BIG;
    }
    if (r.n_out > b->out_cap) { set_error("%llu bytes of BAM in a SAM batch made for %llu", (unsigned long long)r.n_out, (unsigned long long)b->out_cap); return -E2BIG; }
    hipStream_t s = b->stream;
    const u64 n = r.n_lines;
    if (bam && r.n_out && !b->h_out) {
        if (!b->own.pin(&b->h_out, b->out_cap)) {
            b->own.err = hipSuccess; b->h_out = nullptr;       // a later wait may try again
            set_error("pinned allocation of %llu bytes for a SAM batch's records failed", (unsigned long long)b->out_cap);
            return -ENOMEM;
        }
    }
    if (n) {
        HIP_TRY(hipMemcpyAsync(b->h_line_off, b->a.line_off, n * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(b->h_line_len, b->a.line_len, n * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(b->h_keys, b->a.keys, n * sizeof(mgx_bam_key_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(b->h_rec_off, b->a.rec_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (bam && r.n_out) HIP_TRY(hipMemcpyAsync(b->h_out, b->a.out, r.n_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bam) *bam = b->h_out;
    *n_lines = n; *n_bytes_out = r.n_out;
    return 0;
}

int mgx_sam_encode(mgx_bgzf_t* c, const mgx_sam_table_t* table, const uint8_t* text, uint64_t n, uint64_t max_lines, uint64_t out_capacity,
                   uint64_t* line_off, uint32_t* line_len, uint64_t* rec_off, mgx_bam_key_t* keys, uint8_t* out, uint64_t* n_lines, uint64_t* n_out,
                   uint64_t* n_declined) {
    if (!c || !table || !line_off || !line_len || !rec_off || !n_lines || !n_out || !n_declined || (n && !text)) { set_error("NULL argument"); return -EINVAL; }
    *n_lines = 0; *n_out = 0; *n_declined = 0;
    mgx_sam_batch_t* b = nullptr;
    int rc = mgx_sam_batch_create(c, table, n, max_lines, &b);
    if (rc) return rc;
    if (n) memcpy(b->h_in, text, n);
    rc = mgx_sam_batch_submit(c, b, n);
    if (!rc) {
        const uint64_t* lo; const uint32_t* ll; const uint64_t* ro; const mgx_bam_key_t* k; const uint8_t* bytes = nullptr;
        rc = mgx_sam_batch_wait(c, b, &lo, &ll, &ro, &k, n_lines, n_out, out ? &bytes : nullptr);
        if (!rc && out && *n_out > out_capacity) { set_error("%llu bytes of BAM, room for %llu", (unsigned long long)*n_out, (unsigned long long)out_capacity); rc = -E2BIG; }
        if (!rc) {
            memcpy(line_off, lo, *n_lines * 8); memcpy(line_len, ll, *n_lines * 4); memcpy(rec_off, ro, (*n_lines + 1) * 8);
            if (keys) memcpy(keys, k, *n_lines * sizeof(mgx_bam_key_t));
            if (out && *n_out) memcpy(out, bytes, *n_out);
            *n_declined = b->h_res->n_declined;
        }
    }
    return mgx_hip::keep_error(rc, [&] { mgx_sam_batch_destroy(c, b); });
}

int mgx_sam_stats(mgx_bgzf_t* c, mgx_sam_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    std::lock_guard<std::mutex> g(c->sam_mu);
    out->n_lines = c->sam_lines; out->n_declined = c->sam_declined; out->bytes_in = c->sam_bytes_in; out->bytes_out = c->sam_bytes_out;
    out->n_tiles = c->sam_tiles; out->ms_lines = c->sam_ms_lines; out->ms_encode = c->sam_ms_encode; out->ms_keys = c->sam_ms_keys;
    return 0;
}

}  // extern "C"
