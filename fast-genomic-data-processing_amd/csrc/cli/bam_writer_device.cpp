// bam_writer_device.cpp -- the BAM writer's device half (see bam_writer.h): everything that calls the compressor of libmgx.so
// (include/mgx_bgzf.h).  The -z pinned slice compressor, the header compressed on the device, write_bam_store.
#include "bam_writer_parts.h"

#include "../../../include/mgx_bgzf.h"

#include <unistd.h>

#include <condition_variable>
#include <mutex>
#include <thread>

namespace bamout {

std::atomic<int> g_store_arrays_ready{0};

namespace {

constexpr uint32_t kDeviceBatchBlocks = 512;   // BGZF blocks per device batch (32 MB of BAM bytes), two batches per writer thread

// the header in BGZF blocks of its own, on the device (the zlib form is in bam_writer.cpp)
bool compress_header(mgx_bgzf_t* ctx, const std::vector<uint8_t>& head, std::vector<uint8_t>* file, std::string* err) {
    std::vector<uint64_t> off;
    for (size_t o = 0; o < head.size(); o += kBlockIn) off.push_back(o);
    off.push_back(head.size());
    std::vector<uint64_t> out_off(off.size());
    file->resize(mgx_bgzf_bound(head.size(), off.size() - 1));
    if (mgx_bgzf_compress(ctx, head.data(), off.data(), off.size() - 1, file->data(), file->size(), out_off.data())) { *err = mgx_last_error(); return false; }
    file->resize(out_off.back());
    return true;
}

// compress_slice_batched's backend in production: two pinned batches of a context of this thread's own
struct DeviceBatches {
    mgx_bgzf_t* ctx = nullptr;
    mgx_bgzf_batch_t* batch[2] = {nullptr, nullptr};
    uint64_t cap = 0; uint32_t max_blocks = 0;
    std::string err;
    bool fail() { err = mgx_last_error(); return false; }
    bool create(int device, uint64_t capacity, uint32_t blocks) {
        cap = capacity; max_blocks = blocks;
        if (mgx_bgzf_create(device, 0, &ctx)) return fail();
        for (int i = 0; i < 2; ++i)
            if (mgx_bgzf_batch_create(ctx, cap, max_blocks, &batch[i])) return fail();
        return true;
    }
    ~DeviceBatches() {
        for (int i = 0; i < 2; ++i) if (batch[i]) mgx_bgzf_batch_destroy(ctx, batch[i]);
        if (ctx) mgx_bgzf_destroy(ctx);
    }
    uint8_t* input(int k) { return mgx_bgzf_batch_input(batch[k]); }
    uint64_t* offsets(int k) { return mgx_bgzf_batch_offsets(batch[k]); }
    bool submit(int k, uint32_t n_blocks) { return mgx_bgzf_batch_submit(ctx, batch[k], n_blocks) == 0 || fail(); }
    bool wait(int k, const uint8_t** out, const uint64_t** out_off) { return mgx_bgzf_batch_wait(ctx, batch[k], out, out_off) == 0 || fail(); }
};

struct PinnedSlices : SliceCompressor {
    DeviceBatches dv;
    const bool ready;
    explicit PinnedSlices(int device) : ready(dv.create(device, (uint64_t)kDeviceBatchBlocks * kBlockIn, kDeviceBatchBlocks)) {}
    void run(const RecordRefs& recs, size_t lo, size_t hi, Slice* s) override {
        if (ready) compress_slice_batched(recs, lo, hi, &dv, s); else s->ok = false;
        if (!s->ok) err = "device compressor: " + dv.err;
    }
};

// One of MGX_CLI_WRITERS helpers of a BlockSink: copies its share of a batch out of the pinned buffer and writes it in the background
struct Helper {
    std::thread th; std::mutex mu; std::condition_variable cv;
    const uint8_t* src = nullptr; uint64_t n = 0, at = 0; int state = 0;      // 0 idle, 1 job posted, 2 copied (writing), -1 quit
    std::vector<uint8_t> buf; bool ok = true;
    void work(int fd) {
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return state == 1 || state == -1; });
            if (state == -1) return;
            if (buf.size() < n) buf.resize(n);
            memcpy(buf.data(), src, n);
            state = 2;
            cv.notify_all();
            lk.unlock();
            const bool w = pwrite_all(fd, buf.data(), n, at);
            lk.lock();
            if (!w) ok = false;
            state = 0;
            cv.notify_all();
        }
    }
};

// Where mgx_bgzf_store_emit's blocks go: into the file at `at`, the compressed position of every block kept for the index.
// take() must be done with a batch's bytes when it returns.  Round 3: it simply writes them -- one pwrite of the whole batch
// from the pinned buffer, on the thread store_emit calls it on.  The device does not wait for that (store_emit keeps three
// windows in flight, and a window takes the device 1.5 ms against 7 ms in the file), and ONE writer is what the file takes
// fastest: buffered pwrite()s of one file go through its inode lock one at a time, and threads queueing for it move less than
// a single one (tools/dev_tmpfs_write.py on the GPU box, 16 GB into tmpfs: 1 thread 6.3 GB/s; 4 threads on one file 3.7;
// 8 threads 3.5; a file each 18.7 / 33.5 -- a BAM is one file).  Rounds 1-2 had four helpers copy a quarter of the batch each
// and write it in the background: 3.5 GB/s at 200 M records.  MGX_CLI_WRITERS=n (n > 0) brings the helpers back.
struct BlockSink {
    int fd; uint64_t at; std::vector<uint64_t> block_at; std::vector<Helper> h;
    BlockSink(int fd_, uint64_t at_) : fd(fd_), at(at_) {
        const char* e = getenv("MGX_CLI_WRITERS");
        h = std::vector<Helper>((size_t)std::max(0, std::min(e ? atoi(e) : 0, 32)));
        for (Helper& x : h) x.th = std::thread([&x, fd_]() { x.work(fd_); });
    }
    static int take(void* user, const uint8_t* blocks, uint64_t n_bytes, uint32_t n_blocks, const uint64_t* block_off) {
        BlockSink* k = (BlockSink*)user;
        for (uint32_t i = 0; i < n_blocks; ++i) k->block_at.push_back(k->at + block_off[i]);
        const int nh = (int)k->h.size();
        bool ok = true;
        if (nh == 0) ok = pwrite_all(k->fd, blocks, n_bytes, k->at);
        for (int t = 0; t < nh; ++t) {
            Helper& x = k->h[t];
            const uint64_t lo = n_bytes * t / nh, hi = n_bytes * (t + 1) / nh;
            std::unique_lock<std::mutex> lk(x.mu);
            x.cv.wait(lk, [&] { return x.state == 0; });          // its previous quarter is on disk
            x.src = blocks + lo; x.n = hi - lo; x.at = k->at + lo; x.state = 1;
            x.cv.notify_all();
        }
        for (int t = 0; t < nh; ++t) {
            Helper& x = k->h[t];
            std::unique_lock<std::mutex> lk(x.mu);
            x.cv.wait(lk, [&] { return x.state != 1; });          // copied: the batch's buffer may be reused
            ok = ok && x.ok;
        }
        if (!ok) return 1;
        k->at += n_bytes;
        return 0;
    }
    bool join() {                                // false: a helper could not write
        bool ok = true;
        for (Helper& x : h) {
            { std::unique_lock<std::mutex> lk(x.mu); x.cv.wait(lk, [&] { return x.state == 0; }); x.state = -1; x.cv.notify_all(); }
            x.th.join();
            ok = ok && x.ok;
        }
        return ok;
    }
};

}  // namespace

bool compress_header_on(int device, const std::vector<uint8_t>& head, std::vector<uint8_t>* file, std::string* err) {
    mgx_bgzf_t* ctx = nullptr;
    if (mgx_bgzf_create(device, 0, &ctx)) { *err = mgx_last_error(); return false; }
    const bool ok = compress_header(ctx, head, file, err);
    mgx_bgzf_destroy(ctx);
    return ok;
}

std::unique_ptr<SliceCompressor> make_pinned_compressor(int device) { return std::unique_ptr<SliceCompressor>(new PinnedSlices(device)); }

// The records live in HBM (mgx_bgzf_store): recs[k].blob is a DEVICE address.  The device gathers them in output order,
// marks the duplicates, cuts the stream every 65 280 bytes and compresses it; this thread writes the blocks as they come
// back and keeps the compressed position of every block for the index.
bool write_bam_store(const std::string& path, const samtext::Header& hdr, const RecordRefs& recs, void* bgzf_ctx, void* store,
                     int threads, std::string* err) {
    const StageClock clock{"write_bam_store", 22};
    std::vector<uint8_t> file;
    if (!compress_header((mgx_bgzf_t*)bgzf_ctx, header_bytes(hdr), &file, err)) return false;
    const int fd = open_output(path, err);
    if (fd < 0) return false;
    const bool head_ok = pwrite_all(fd, file.data(), file.size(), 0);
    const size_t n = recs.size();
    // (arrays of 200 M entries: left uninitialised, so that their pages are first touched by the gang below and not zeroed by one thread)
    std::unique_ptr<uint32_t[]> order(new uint32_t[n + 1]), len(new uint32_t[n + 1]);
    std::unique_ptr<uint8_t[]> dup(new uint8_t[n + 1]);
    std::unique_ptr<uint64_t[]> addr(new uint64_t[n + 1]), uoff(new uint64_t[n + 1]);
    const size_t T = (size_t)std::max(1, std::min(threads, 16));
    gang::run_gang(T, [&](size_t t) {
        const auto r = gang::gang_range(n, t, T);
        for (size_t q = r.begin; q < r.end; ++q) {
            order[q] = (uint32_t)q; len[q] = recs[q].len; dup[q] = recs[q].set_dup; addr[q] = (uint64_t)(uintptr_t)recs[q].blob;
        }
    });
    g_store_arrays_ready.store(1);
    clock.stamp("arrays ready");
    BlockSink sink(fd, file.size());
    const int emit_rc = mgx_bgzf_store_emit((mgx_bgzf_store_t*)store, n, order.get(), dup.get(), addr.get(), len.get(), BlockSink::take, &sink, uoff.get());
    const bool helpers_ok = sink.join();
    if (emit_rc || !helpers_ok) {
        *err = helpers_ok ? std::string("device: ") + mgx_last_error() : "short write to " + path;
        close(fd);
        return false;
    }
    clock.stamp("stream written");
    sink.block_at.push_back(sink.at);                // the position after the last block: virtual offsets at the very end
    if (!finish_file(fd, head_ok, sink.at, path, err)) return false;
    // not the BlockCutter's rule: the device cuts this stream at fixed 0xff00 offsets, whatever record is there
    auto voff = [&](size_t k, uint64_t* vb, uint64_t* ve) {
        *vb = (sink.block_at[uoff[k] / kBlockIn] << 16) | (uoff[k] % kBlockIn);
        *ve = (sink.block_at[uoff[k + 1] / kBlockIn] << 16) | (uoff[k + 1] % kBlockIn);
    };
    const bool iok = write_bai(path, bai_bytes(hdr.ref_name.size(), recs, voff, threads), err);      // this voff holds no state: any thread, any order
    clock.stamp("index written");
    return iok;
}

}  // namespace bamout
