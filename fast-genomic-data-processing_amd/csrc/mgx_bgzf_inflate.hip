// mgx_bgzf_inflate.hip -- BGZF block inflate on gfx950 (C ABI: include/mgx_bgzf.h), DESIGN.md 4.7.
//
// The read side of htslib's bgzf_read_block / inflate_block (bgzf.c:716-780, 1100-1180).  A batch holds thousands of
// independent BGZF blocks; their compressed offsets and their output offsets (prefix sums of the ISIZEs, which the host
// block scanner reads from the trailers) are known before anything is decoded, so one wavefront takes one block and
// writes its bytes straight to their final place in the batch's output buffer.  Per block:
//   1. header, BSIZE and ISIZE checks, then the DEFLATE stream decoded symbol by symbol by the whole wavefront in step
//      (wave-uniform: the code is bgzf_inflate_core.h, the same text the host tests run under AddressSanitizer), Huffman
//      tables in LDS.  Literals and matches go into an LDS window of up to 512 tokens / 4 KB of output;
//   2. a full window is expanded by all 64 lanes: a scan over the token lengths places every token, each output byte finds
//      its token by binary search and becomes either its value (a literal, or a match byte whose source lies before the
//      window: read back from the output) or a link to an earlier byte of the window (a match with distance < length
//      repeats its period: source = start - dist + (k mod dist)).  Links are resolved by pointer jumping -- a link's
//      target is replaced by its target's content until every byte is a value -- in O(log chain) rounds, and the window
//      is written out with plain vector stores;
//   3. stored blocks are copied by all lanes from the input;
//   4. CRC-32 of the output: every lane its 1/64, shifted by multiplication with x^(8 * bytes after) modulo the CRC
//      polynomial (the combination k_bgzf_deflate uses), XOR-reduced over the wavefront, compared with the trailer.
// Every block writes a status word (bgzf_inflate_core.h Status): corrupt input is a returned error, never a fault --
// every read, table index, distance and write is checked against the block's own ranges before it happens.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mgx_bgzf.h"
#include "bgzf_inflate_core.h"
#include "mgx_bgzf_ctx.h"

using mgx::set_error;

namespace {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
using namespace mgx_inflate;

constexpr u32 kTok = 512;                 // tokens per window
constexpr u32 kWin = 4096;                // a window is expanded once its output reaches this many bytes
constexpr u32 kCells = kWin + 258;        // ... so it holds at most this many
constexpr u32 kWavesPerCu = 8;            // workgroups of one wavefront per CU in the grid (LDS: ~17 KB each)
constexpr u32 kCrcPoly = 0xEDB88320u;
constexpr u16 kLink = 0x8000;             // a cell that still points at an earlier cell of the window

struct InfLds {
    Tables t;                             // Huffman tables of the current DEFLATE block
    u32 tok[kTok];                        // literal: bit 31 | byte; match: length << 16 | distance
    u16 tstart[kTok + 1];                 // window-relative output offset of each token
    u16 cell[kCells];                     // the window's bytes: a value (< 256) or kLink | earlier cell
    u32 crc_tab[256];
    u32 x2n[32];                          // x^(2^k) mod P
};

struct InflateArgs {
    const u8* in; const u64* in_off; const u64* out_off; u8* out; u32* status; u32 n_blocks;
};

__device__ __forceinline__ u32 multmodp(u32 a, u32 b) {
    // product of two polynomials modulo the CRC polynomial, bit 31 = x^0 (reflected)
    u32 p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// The sink of the wave-uniform decode loop: every lane calls it with the same arguments, so flush() may use the whole
// wavefront.  out = the block's output (its length was checked against ISIZE by the decode loop before every call).
struct WaveSink {
    InfLds& L; u8* out; u32 lane; u32 w0; u32 nt; u32 wbytes;

    __device__ void flush() {
        if (nt == 0) return;
        __syncthreads();
        // token offsets: lane l sums its run of tokens, a wavefront scan places the runs
        const u32 per = (nt + 63u) / 64u;
        const u32 t0 = min(nt, lane * per), t1 = min(nt, t0 + per);
        u32 s = 0;
        for (u32 i = t0; i < t1; ++i) { const u32 tk = L.tok[i]; s += (tk >> 31) ? 1u : (tk >> 16); }
        u32 inc = s;
        for (u32 o = 1; o < 64; o <<= 1) { const u32 v = (u32)__shfl_up((int)inc, o, 64); if (lane >= o) inc += v; }
        u32 run = inc - s;
        for (u32 i = t0; i < t1; ++i) { L.tstart[i] = (u16)run; const u32 tk = L.tok[i]; run += (tk >> 31) ? 1u : (tk >> 16); }
        __syncthreads();
        // every byte: a value, or a link to an earlier byte of the window
        for (u32 q = lane; q < wbytes; q += 64) {
            u32 lo = 0, hi = nt - 1;                       // the last token starting at or before q
            while (lo < hi) { const u32 mid = (lo + hi + 1) >> 1; if (L.tstart[mid] <= q) lo = mid; else hi = mid - 1; }
            const u32 tk = L.tok[lo];
            u16 c;
            if (tk >> 31) c = (u16)(tk & 0xffu);
            else {
                const u32 len = tk >> 16, d = tk & 0xffffu, k = q - L.tstart[lo];
                const int src = (int)L.tstart[lo] - (int)d + (int)(d < len ? k % d : k);
                c = src < 0 ? (u16)out[(int)w0 + src] : (u16)(kLink | (u32)src);      // w0 + src >= 0: distance <= position
            }
            L.cell[q] = c;
        }
        __syncthreads();
        // pointer jumping: a link takes its target's content (a value, or the target's own, earlier link)
        for (;;) {
            bool pending = false;
            for (u32 q = lane; q < wbytes; q += 64) {
                const u16 c = L.cell[q];
                if (c & kLink) { const u16 c2 = L.cell[c & (kLink - 1)]; L.cell[q] = c2; pending |= (c2 & kLink) != 0; }
            }
            __syncthreads();
            if (!__any(pending)) break;
        }
        for (u32 q = lane; q < wbytes; q += 64) out[w0 + q] = (u8)L.cell[q];
        __syncthreads();                                   // the next window reads these bytes back
        w0 += wbytes; nt = 0; wbytes = 0;
    }
    __device__ void push(u32 tk, u32 n) {
        L.tok[nt] = tk;
        ++nt; wbytes += n;
        if (nt == kTok || wbytes >= kWin) flush();
    }
    __device__ void lit(u32 b, u32) { push(0x80000000u | b, 1); }
    __device__ void match(u32 len, u32 dist, u32) { push(len << 16 | dist, len); }
    __device__ void stored(const u8* src, u32 len, u32 pos) {
        flush();
        for (u32 i = lane; i < len; i += 64) out[pos + i] = src[i];
        __syncthreads();
        w0 = pos + len;
    }
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(InflateArgs a) {
    __shared__ InfLds L;
    const u32 lane = threadIdx.x;
    for (u32 i = lane; i < 256; i += 64) {
        u32 c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        L.crc_tab[i] = c;
    }
    if (lane == 0) {
        u32 p = 0x40000000u;                               // x^1
        L.x2n[0] = p;
        for (int k = 1; k < 32; ++k) { p = multmodp(p, p); L.x2n[k] = p; }
    }
    __syncthreads();
    for (u32 blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const u64 i0 = a.in_off[blk], i1 = a.in_off[blk + 1];
        const u64 o0 = a.out_off[blk];
        const u32 out_len = (u32)(a.out_off[blk + 1] - o0);    // <= 64 KB: checked by the host at submit
        const u8* in = a.in + i0;
        u8* out = a.out + o0;
        u32 payload = 0, crc_want = 0, got = 0;
        u32 st = member_bounds(in, i1 - i0, out_len, &payload, &crc_want);
        if (st == kOk) {
            WaveSink sink{L, out, lane, 0, 0, 0};
            st = inflate_raw(in + kHeaderBytes, payload, out_len, L.t, sink, &got);
            sink.flush();
            if (st == kOk && got != out_len) st = kIsizeMismatch;
        }
        if (st == kOk) {
            const u32 per = (out_len + 63u) / 64u;
            const u32 lo = min(out_len, lane * per), hi = min(out_len, lo + per);
            u32 c = lane == 0 ? 0xFFFFFFFFu : 0u;
            for (u32 p = lo; p < hi; ++p) c = L.crc_tab[(c ^ out[p]) & 0xffu] ^ (c >> 8);
            for (u32 after = out_len - hi, k = 3; after; after >>= 1, ++k) if (after & 1u) c = multmodp(L.x2n[k], c);
            for (int o = 32; o >= 1; o >>= 1) c ^= (u32)__shfl_xor((int)c, o, 64);
            if ((c ^ 0xFFFFFFFFu) != crc_want) st = kCrcMismatch;
        }
        if (lane == 0) a.status[blk] = st;
        __syncthreads();                                   // the LDS serves the next block
    }
}

}  // namespace

extern "C" {

void mgx_bgzf_inflate_batch_destroy(mgx_bgzf_t* c, mgx_bgzf_inflate_t* b) {
    if (!b) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->up); (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->copy); }
    delete b;                                              // its owner frees
}

int mgx_bgzf_inflate_batch_create(mgx_bgzf_t* c, uint64_t in_capacity, uint64_t out_capacity, uint32_t max_blocks, mgx_bgzf_inflate_t** out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = nullptr;
    if (max_blocks == 0) { set_error("max_blocks is 0"); return -EINVAL; }
    in_capacity = std::min<u64>(in_capacity, (u64)max_blocks * kMaxBlock);
    out_capacity = std::min<u64>(out_capacity, (u64)max_blocks * kMaxIsize);
    HIP_TRY(hipSetDevice(c->device));
    mgx_bgzf_inflate* b = new (std::nothrow) mgx_bgzf_inflate;
    if (!b) { set_error("out of memory"); return -ENOMEM; }
    b->in_cap = in_capacity; b->out_cap = out_capacity; b->max_blocks = max_blocks;
    const size_t off_bytes = 2 * ((size_t)max_blocks + 1) * sizeof(u64);
    mgx_hip::Owner& m = b->own;
    m.pin(&b->h_in, in_capacity + 8); m.pin(&b->h_off, off_bytes); m.pin(&b->h_out, out_capacity + 8); m.pin(&b->h_status, (size_t)max_blocks * sizeof(u32));
    m.device(&b->d_in, in_capacity + 8); m.device(&b->d_off, off_bytes); m.device(&b->d_out, out_capacity + 8); m.device(&b->d_status, (size_t)max_blocks * sizeof(u32));
    m.event(&b->ev_in, hipEventDisableTiming); m.event(&b->ev_k0); m.event(&b->ev_k1); m.event(&b->ev_done, hipEventDisableTiming);
    if (!m.ok()) {
        set_error("%s failed for an inflate batch of %llu / %llu bytes, %u blocks", m.failed, (unsigned long long)in_capacity, (unsigned long long)out_capacity, max_blocks);
        mgx_bgzf_inflate_batch_destroy(c, b);
        return -ENOMEM;
    }
    b->h_off[0] = 0; b->h_off[max_blocks + 1] = 0;
    *out = b;
    return 0;
}

uint8_t* mgx_bgzf_inflate_batch_input(mgx_bgzf_inflate_t* b) { return b ? b->h_in : nullptr; }

int mgx_bgzf_inflate_batch_offsets(mgx_bgzf_inflate_t* b, uint64_t** in_offsets, uint64_t** out_offsets) {
    if (!b || !in_offsets || !out_offsets) { set_error("NULL argument"); return -EINVAL; }
    *in_offsets = b->h_off; *out_offsets = b->h_off + b->max_blocks + 1;
    return 0;
}

int mgx_bgzf_inflate_batch_submit(mgx_bgzf_t* c, mgx_bgzf_inflate_t* b, uint32_t n_blocks) {
    if (!c || !b) { set_error("NULL argument"); return -EINVAL; }
    if (b->submitted) { set_error("inflate batch submitted twice without a wait"); return -EINVAL; }
    if (n_blocks > b->max_blocks) { set_error("%u blocks in an inflate batch made for %u", n_blocks, b->max_blocks); return -EINVAL; }
    const u64* io = b->h_off; const u64* oo = b->h_off + b->max_blocks + 1;
    if (io[0] != 0 || oo[0] != 0) { set_error("in_offsets[0] and out_offsets[0] must be 0"); return -EINVAL; }
    for (u32 i = 0; i < n_blocks; ++i) {
        if (io[i + 1] < io[i] || io[i + 1] - io[i] > kMaxBlock) {
            set_error("block %u: compressed range [%llu, %llu) is not a BGZF block of at most 64 KB", i, (unsigned long long)io[i], (unsigned long long)io[i + 1]);
            return -EINVAL;
        }
        if (oo[i + 1] < oo[i] || oo[i + 1] - oo[i] > kMaxIsize) {
            set_error("block %u: output range [%llu, %llu) is more than 64 KB", i, (unsigned long long)oo[i], (unsigned long long)oo[i + 1]);
            return -EINVAL;
        }
    }
    const u64 n_in = io[n_blocks], n_out = oo[n_blocks];
    if (n_in > b->in_cap || n_out > b->out_cap) {
        set_error("%llu compressed / %llu output bytes in an inflate batch made for %llu / %llu", (unsigned long long)n_in, (unsigned long long)n_out,
                  (unsigned long long)b->in_cap, (unsigned long long)b->out_cap);
        return -EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    b->n_blocks = n_blocks; b->n_in = n_in; b->n_out = n_out; b->submitted = true;
    if (n_blocks == 0) return 0;
    hipStream_t s = c->stream;
    // the compressed bytes go up on the upload stream (under the kernels of the batch before), the offsets behind them
    HIP_TRY(hipMemcpyAsync(b->d_in, b->h_in, n_in, hipMemcpyHostToDevice, c->up));
    HIP_TRY(hipMemcpyAsync(b->d_off, b->h_off, ((size_t)n_blocks + 1) * sizeof(u64), hipMemcpyHostToDevice, c->up));
    HIP_TRY(hipMemcpyAsync(b->d_off + b->max_blocks + 1, oo, ((size_t)n_blocks + 1) * sizeof(u64), hipMemcpyHostToDevice, c->up));
    HIP_TRY(hipEventRecord(b->ev_in, c->up));
    HIP_TRY(hipStreamWaitEvent(s, b->ev_in, 0));
    InflateArgs a{b->d_in, b->d_off, b->d_off + b->max_blocks + 1, b->d_out, b->d_status, n_blocks};
    HIP_TRY(hipEventRecord(b->ev_k0, s));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(std::min<u32>(n_blocks, (u32)c->n_cu * kWavesPerCu)), dim3(64), 0, s, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev_k1, s));
    // the bytes come back on the copy stream, behind this batch's kernel only
    HIP_TRY(hipStreamWaitEvent(c->copy, b->ev_k1, 0));
    HIP_TRY(hipMemcpyAsync(b->h_status, b->d_status, (size_t)n_blocks * sizeof(u32), hipMemcpyDeviceToHost, c->copy));
    if (n_out) HIP_TRY(hipMemcpyAsync(b->h_out, b->d_out, n_out, hipMemcpyDeviceToHost, c->copy));
    HIP_TRY(hipEventRecord(b->ev_done, c->copy));
    return 0;
}

int mgx_bgzf_inflate_batch_wait(mgx_bgzf_t* c, mgx_bgzf_inflate_t* b, const uint8_t** out, const uint32_t** status) {
    if (!c || !b || !out) { set_error("NULL argument"); return -EINVAL; }
    if (!b->submitted) { set_error("inflate batch was not submitted"); return -EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    *out = b->h_out;
    if (status) *status = b->h_status;
    b->submitted = false;
    if (b->n_blocks == 0) return 0;
    HIP_TRY(hipEventSynchronize(b->ev_done));
    float ms = 0;
    {
        std::lock_guard<std::mutex> g(c->inf_mu);
        if (hipEventElapsedTime(&ms, b->ev_k0, b->ev_k1) == hipSuccess) c->inf_ms_kernel = ms;
        c->inf_blocks += b->n_blocks; c->inf_bytes_in += b->n_in; c->inf_bytes_out += b->n_out;
    }
    for (u32 i = 0; i < b->n_blocks; ++i) {
        if (b->h_status[i] != kOk) {
            u32 n_bad = 0;
            for (u32 j = i; j < b->n_blocks; ++j) n_bad += b->h_status[j] != kOk;
            set_error("BGZF block %u of the batch (compressed offset %llu): %s (%u bad block%s in the batch)", i, (unsigned long long)b->h_off[i],
                      status_text(b->h_status[i]), n_bad, n_bad == 1 ? "" : "s");
            return -EBADMSG;
        }
    }
    return 0;
}

int mgx_bgzf_decompress(mgx_bgzf_t* c, const uint8_t* in, uint64_t n_in, uint8_t* out, uint64_t out_capacity, uint64_t* n_out) {
    if (!c || !n_out || (n_in && !in)) { set_error("NULL argument"); return -EINVAL; }
    *n_out = 0;
    const u64 max_blocks = n_in / (kHeaderBytes + kTrailerBytes) + 1;
    std::vector<u64> off(max_blocks + 1);
    std::vector<u32> isize(max_blocks);
    u64 nb = 0; int stop = 0;
    if (const int rc = mgx_bgzf_scan_blocks(in, n_in, max_blocks, off.data(), isize.data(), nullptr, &nb, &stop)) return rc;
    if (stop != MGX_BGZF_SCAN_END) {
        set_error("the input is not whole BGZF blocks: %s at offset %llu", stop == MGX_BGZF_SCAN_PARTIAL ? "a truncated block" : "not a BGZF block",
                  (unsigned long long)off[nb]);
        return -EBADMSG;
    }
    u64 total = 0;
    for (u64 i = 0; i < nb; ++i) total += isize[i];
    if (total > out_capacity) { set_error("%llu bytes inflated, output capacity %llu", (unsigned long long)total, (unsigned long long)out_capacity); return -EINVAL; }
    if (total && !out) { set_error("NULL argument"); return -EINVAL; }
    if (nb == 0) return 0;
    constexpr u32 kPer = 1024;                     // blocks per internal batch (at most 64 MB each way)
    const u32 per = (u32)std::min<u64>(kPer, nb);
    mgx_bgzf_inflate_t* bt[2] = {nullptr, nullptr};
    int rc = 0;
    for (int i = 0; i < 2 && !rc; ++i) rc = mgx_bgzf_inflate_batch_create(c, std::min<u64>(n_in, (u64)per * kMaxBlock), std::min<u64>(total, (u64)per * kMaxIsize) + 1, per, &bt[i]);
    struct Flight { u64 first, count, out_at; };
    Flight fl[2] = {{0, 0, 0}, {0, 0, 0}};
    auto drain = [&](int k) -> int {
        if (!fl[k].count) return 0;
        const uint8_t* o; const uint32_t* st;
        const int r = mgx_bgzf_inflate_batch_wait(c, bt[k], &o, &st);
        if (r) {
            for (u64 i = 0; i < fl[k].count; ++i)
                if (st[i]) { set_error("BGZF block %llu (offset %llu): %s", (unsigned long long)(fl[k].first + i), (unsigned long long)off[fl[k].first + i], status_text(st[i])); break; }
            return r;
        }
        if (bt[k]->n_out) memcpy(out + fl[k].out_at, o, bt[k]->n_out);
        fl[k].count = 0;
        return 0;
    };
    int k = 0;
    u64 out_at = 0;
    for (u64 first = 0; first < nb && !rc; first += per, k ^= 1) {
        rc = drain(k);
        if (rc) break;
        const u64 cnt = std::min<u64>(per, nb - first);
        u64 *io, *oo;
        mgx_bgzf_inflate_batch_offsets(bt[k], &io, &oo);
        const u64 b0 = off[first];
        memcpy(bt[k]->h_in, in + b0, off[first + cnt] - b0);
        for (u64 i = 0; i <= cnt; ++i) io[i] = off[first + i] - b0;
        oo[0] = 0;
        for (u64 i = 0; i < cnt; ++i) oo[i + 1] = oo[i] + isize[first + i];
        rc = mgx_bgzf_inflate_batch_submit(c, bt[k], (u32)cnt);
        if (!rc) { fl[k] = {first, cnt, out_at}; out_at += oo[cnt]; }
    }
    if (!rc) rc = drain(k);
    if (!rc) rc = drain(k ^ 1);
    for (int i = 0; i < 2; ++i) mgx_bgzf_inflate_batch_destroy(c, bt[i]);
    if (!rc) *n_out = total;
    return rc;
}

int mgx_bgzf_inflate_stats(mgx_bgzf_t* c, mgx_bgzf_inflate_stats_t* out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    std::lock_guard<std::mutex> g(c->inf_mu);
    out->n_blocks = c->inf_blocks; out->bytes_in = c->inf_bytes_in; out->bytes_out = c->inf_bytes_out; out->ms_kernel = c->inf_ms_kernel;
    return 0;
}

}  // extern "C"
