// mgx_store.hip -- the record store (C ABI: the mgx_bgzf_store_* calls of include/mgx_bgzf.h), DESIGN.md 4.6: BAM
// records resident in HBM from ingest to output.  put copies whole records into large pieces of device memory from any
// thread (pinned staging and copy streams of its own) and returns their address; emit scans the records' places in the
// uncompressed stream (mgx_scan.h), gathers one window of the stream at a time into a compressor batch's device input
// (k_store_gather) and hands the finished BGZF blocks to a sink, three batches in flight.  Of the compressor (mgx_bgzf.hip)
// it needs a batch without pinned input and a submit that copies nothing up: mgx_bgzf_internal.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mgx_bgzf.h"
#include "mgx_bgzf_internal.h"
#include "mgx_scan.h"

using mgx::set_error;

namespace {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kMaxIn = MGX_BGZF_MAX_BLOCK_IN;

// what record order[q] takes in the uncompressed stream: its block_size field and its bytes
struct StreamLength {
    const u32* order; const u32* len;
    __device__ u64 operator()(u64 q) const { return 4u + len[order[q]]; }
};

// One wavefront per record q in [q0, q1): block_size + bytes to their place in the window [win0, win0 + win_bytes) of the
// stream; a duplicate gets FLAG |= 0x400 (byte 15 of the record, bit 2) on the way.
__global__ __launch_bounds__(256) void k_store_gather(const u64* addr, const u32* len, const u32* order, const u8* dup, const u64* uoff,
                                                      u64 q0, u64 q1, u64 win0, u64 win_bytes, u8* dst) {
    const u64 q = q0 + (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= q1) return;
    const u32 lane = threadIdx.x & 63u;
    const u32 r = order[q];
    const u32 n = len[r];
    const u8* src = reinterpret_cast<const u8*>(addr[r]);
    const u64 at = uoff[q];
    const bool is_dup = dup[r] != 0;
    for (u32 i = lane; i < n + 4u; i += 64u) {
        const u64 o = at + i;
        if (o < win0 || o >= win0 + win_bytes) continue;
        u8 v;
        if (i < 4) v = (u8)(n >> (8 * i));
        else { v = src[i - 4]; if (is_dup && i == 4u + 15u) v |= 0x04; }
        dst[o - win0] = v;
    }
}

struct EmitScratch {                       // the temporaries of one emit: freed behind the stream's work, then the batches
    mgx_bgzf* c; hipStream_t s; mgx_hip::Owner own; mgx_bgzf_batch_t* bt[3] = {nullptr, nullptr, nullptr};
    ~EmitScratch() { (void)hipStreamSynchronize(s); own.release(); for (auto* b : bt) if (b) mgx_bgzf_batch_destroy(c, b); }
};

}  // namespace

struct mgx_bgzf_store {
    mgx_bgzf* ctx = nullptr;
    std::mutex mu;
    std::vector<u8*> chunks;
    u64 cur_off = 0, cur_cap = 0, total = 0;
    // put() stages through pinned buffers of its own (a copy from pageable memory is slow and serialises the callers)
    // and copies on streams of its own, never on the null stream (which would wait for every blocking stream of the process)
    static constexpr int kStage = 24;
    static constexpr size_t kStageBytes = 4u << 20;
    hipStream_t copy[kStage] = {};
    u8* stage[kStage] = {};                    // pinned, allocated by the first put that takes the slot (in parallel, off create's path)
    std::mutex stage_mu; std::condition_variable stage_cv;
    std::vector<int> stage_free;
};

extern "C" {

int mgx_bgzf_store_create(mgx_bgzf_t* c, mgx_bgzf_store_t** out) {
    if (!c || !out) { set_error("NULL argument"); return -EINVAL; }
    *out = nullptr;
    mgx_bgzf_store* st = new (std::nothrow) mgx_bgzf_store;
    if (!st) { set_error("out of memory"); return -ENOMEM; }
    st->ctx = c;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        set_error("record store: %s", hipGetErrorString(e));
        mgx_bgzf_store_destroy(st);
        return -EIO;
    }
    // a slot's stream and pinned buffer are made by the first put that takes the slot: in parallel on the callers'
    // threads instead of 24 stream creations and 96 MB of page pinning in front of the first put
    for (int i = 0; i < mgx_bgzf_store::kStage; ++i) st->stage_free.push_back(mgx_bgzf_store::kStage - 1 - i);
    *out = st;
    return 0;
}

// Allocates HBM for about `bytes` more record bytes now (1 GB pieces), so that the puts of the first slices do not wait
// for hipMalloc one after the other.
int mgx_bgzf_store_reserve(mgx_bgzf_store_t* st, uint64_t bytes) {
    if (!st) { set_error("NULL argument"); return -EINVAL; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    std::lock_guard<std::mutex> g(st->mu);
    if (!st->chunks.empty() || bytes == 0) return 0;
    const u64 cap = std::min<u64>(std::max<u64>((bytes + 15) & ~15ull, 64ull << 20), 256ull << 20);      // a first piece that is quick to map
    u8* p = nullptr;
    if (hipMalloc((void**)&p, cap) != hipSuccess) { set_error("hipMalloc of %llu bytes for the record store failed", (unsigned long long)cap); return -ENOMEM; }
    st->chunks.push_back(p); st->cur_off = 0; st->cur_cap = cap;
    return 0;
}

void mgx_bgzf_store_destroy(mgx_bgzf_store_t* st) {
    if (!st) return;
    (void)hipSetDevice(st->ctx->device);
    for (u8* p : st->chunks) (void)hipFree(p);
    for (auto& sc : st->copy) if (sc) (void)hipStreamDestroy(sc);
    for (auto& p : st->stage) if (p) (void)hipHostFree(p);
    delete st;
}

// n bytes of the store's HBM (1 GB pieces; a put never straddles two), 16-byte aligned
static int store_alloc(mgx_bgzf_store* st, u64 n, u8** dst) {
    std::lock_guard<std::mutex> g(st->mu);
    const u64 need = (n + 15) & ~15ull;
    if (st->cur_off + need > st->cur_cap) {
        const u64 cap = std::max<u64>(need, 1ull << 30);
        u8* p = nullptr;
        if (hipMalloc((void**)&p, cap) != hipSuccess) { set_error("hipMalloc of %llu bytes for the record store failed (%llu bytes stored)", (unsigned long long)cap, (unsigned long long)st->total); return -ENOMEM; }
        st->chunks.push_back(p); st->cur_off = 0; st->cur_cap = cap;
    }
    *dst = st->chunks.back() + st->cur_off;
    st->cur_off += need; st->total += n;
    return 0;
}

static int store_take_slot(mgx_bgzf_store* st) {
    std::unique_lock<std::mutex> lk(st->stage_mu);
    st->stage_cv.wait(lk, [&] { return !st->stage_free.empty(); });
    const int k = st->stage_free.back(); st->stage_free.pop_back();
    return k;
}

static void store_give_slot(mgx_bgzf_store* st, int k) {
    { std::lock_guard<std::mutex> g(st->stage_mu); st->stage_free.push_back(k); }
    st->stage_cv.notify_one();
}

int mgx_bgzf_store_put_device(mgx_bgzf_store_t* st, uint64_t device_ptr, uint64_t n, uint64_t* addr) {
    if (!st || !addr || (n && !device_ptr)) { set_error("NULL argument"); return -EINVAL; }
    if (n == 0) { *addr = 0; return 0; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    u8* dst;
    if (const int rc = store_alloc(st, n, &dst)) return rc;
    const int k = store_take_slot(st);             // for the slot's stream: nothing is staged
    hipError_t e = hipSuccess;
    if (!st->copy[k]) e = hipStreamCreateWithFlags(&st->copy[k], hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, (const void*)(uintptr_t)device_ptr, n, hipMemcpyDeviceToDevice, st->copy[k]);
    if (e == hipSuccess) e = hipStreamSynchronize(st->copy[k]);
    store_give_slot(st, k);
    if (e != hipSuccess) { set_error("copy of %llu device bytes to the record store: %s", (unsigned long long)n, hipGetErrorString(e)); return -EIO; }
    *addr = (uint64_t)(uintptr_t)dst;
    return 0;
}

int mgx_bgzf_store_put(mgx_bgzf_store_t* st, const uint8_t* bytes, uint64_t n, uint64_t* addr) {
    if (!st || !addr || (n && !bytes)) { set_error("NULL argument"); return -EINVAL; }
    if (n == 0) { *addr = 0; return 0; }           // nothing to store (a slice of blank lines); no chunk is touched
    HIP_TRY(hipSetDevice(st->ctx->device));
    u8* dst;
    if (const int rc = store_alloc(st, n, &dst)) return rc;
    for (u64 done = 0; done < n;) {
        const int k = store_take_slot(st);
        const u64 piece = std::min<u64>(mgx_bgzf_store::kStageBytes, n - done);
        hipError_t e = hipSuccess;
        if (!st->copy[k]) e = hipStreamCreateWithFlags(&st->copy[k], hipStreamNonBlocking);                                     // this slot's first use
        if (e == hipSuccess && !st->stage[k]) e = hipHostMalloc((void**)&st->stage[k], mgx_bgzf_store::kStageBytes, hipHostMallocDefault);
        if (e == hipSuccess) {
            memcpy(st->stage[k], bytes + done, piece);
            e = hipMemcpyAsync(dst + done, st->stage[k], piece, hipMemcpyHostToDevice, st->copy[k]);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st->copy[k]);
        store_give_slot(st, k);
        if (e != hipSuccess) { set_error("copy of %llu bytes to the record store: %s", (unsigned long long)piece, hipGetErrorString(e)); return -EIO; }
        done += piece;
    }
    *addr = (uint64_t)(uintptr_t)dst;
    return 0;
}

int mgx_bgzf_store_emit(mgx_bgzf_store_t* st, uint64_t n, const uint32_t* order, const uint8_t* dup, const uint64_t* addr, const uint32_t* len,
                        mgx_bgzf_sink_t sink, void* user, uint64_t* uoff_out) {
    if (!st || !sink || !uoff_out || (n && (!order || !dup || !addr || !len))) { set_error("NULL argument"); return -EINVAL; }
    mgx_bgzf* c = st->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const bool trace = getenv("MGX_BGZF_TRACE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto now = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
    uoff_out[0] = 0;
    if (n == 0) return 0;
    if (n > 0xFFFFFFF0ull) { set_error("more than 2^32 records"); return -E2BIG; }
    hipStream_t s = c->stream;
    u32 *d_order = nullptr, *d_len = nullptr; u8* d_dup = nullptr; u64 *d_addr = nullptr, *d_uoff = nullptr, *d_part = nullptr;
    int rc = 0;
    EmitScratch tmp{c, s};                                        // every return below frees through it
    mgx_bgzf_batch_t** bt = tmp.bt;
    tmp.own.device(&d_order, n * sizeof(u32)); tmp.own.device(&d_len, n * sizeof(u32)); tmp.own.device(&d_dup, n); tmp.own.device(&d_addr, n * sizeof(u64));
    tmp.own.device(&d_uoff, (n + 1) * sizeof(u64)); tmp.own.device(&d_part, (n / mgx_hip::kScanChunk + 2) * sizeof(u64));
    HIP_TRY(tmp.own.err);
    HIP_TRY(hipMemcpyAsync(d_order, order, n * sizeof(u32), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_len, len, n * sizeof(u32), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_dup, dup, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_addr, addr, n * sizeof(u64), hipMemcpyHostToDevice, s));
    mgx_hip::scan_exclusive(s, StreamLength{d_order, d_len}, nullptr, n, d_part, d_uoff);      // the total lands in uoff[n]
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(uoff_out, d_uoff, (n + 1) * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const u64 total = uoff_out[n];
    double t_wait = 0, t_sink = 0;
    if (trace) fprintf(stderr, "  store_emit: arrays on the device, offsets scanned and back: %.3f s\n", now());
    constexpr u32 kPer = 1024;                                    // blocks per batch (67 MB of the stream)
    const u64 win = (u64)kPer * kMaxIn;
    const u64 n_win = (total + win - 1) / win;
    for (int i = 0; i < 3 && !rc && (u64)i < n_win; ++i) rc = mgx_internal::bgzf_batch_create(c, win, kPer, false, &bt[i]);
    if (rc) return rc;
    if (trace) fprintf(stderr, "  store_emit: batches allocated: %.3f s\n", now());
    auto collect = [&](u64 k) -> int {
        const uint8_t* o; const uint64_t* oo;
        mgx_bgzf_batch_t* b = bt[k % 3];
        const double t0 = now();
        const int r = mgx_bgzf_batch_wait(c, b, &o, &oo);
        if (r) return r;
        const double t1 = now();
        const int sr = sink(user, o, oo[b->n_blocks], b->n_blocks, oo);
        t_wait += t1 - t0; t_sink += now() - t1;
        if (sr) { set_error("the sink returned %d", sr); return -EIO; }
        return 0;
    };
    u64 q_lo = 0;
    for (u64 k = 0; k < n_win && !rc; ++k) {
        if (k >= 3) rc = collect(k - 3);
        if (rc) break;
        mgx_bgzf_batch_t* b = bt[k % 3];
        const u64 w0 = k * win, wb = std::min(win, total - w0);
        // records that touch [w0, w0 + wb): from the one holding byte w0 to the last one starting before the window's end
        while (q_lo + 1 <= n && uoff_out[q_lo + 1] <= w0) ++q_lo;
        const u64 q_hi = (u64)(std::lower_bound(uoff_out + q_lo, uoff_out + n, w0 + wb) - uoff_out);
        const u32 nb = (u32)((wb + kMaxIn - 1) / kMaxIn);
        for (u32 i = 0; i <= nb; ++i) b->h_off[i] = std::min<u64>((u64)i * kMaxIn, wb);
        if (q_hi > q_lo)
            hipLaunchKernelGGL(k_store_gather, dim3((u32)((q_hi - q_lo + 3) / 4)), dim3(256), 0, s, d_addr, d_len, d_order, d_dup, d_uoff, q_lo, q_hi, w0, wb, b->d_in);
        rc = mgx_internal::bgzf_batch_submit(c, b, nb, true);
    }
    for (u64 k = n_win >= 3 ? n_win - 3 : 0; k < n_win && !rc; ++k) rc = collect(k);
    if (trace) fprintf(stderr, "  store_emit: %llu windows done: %.3f s (waiting for the device %.3f s, in the sink %.3f s)\n", (unsigned long long)n_win, now(), t_wait, t_sink);
    return rc;
}

}  // extern "C"
