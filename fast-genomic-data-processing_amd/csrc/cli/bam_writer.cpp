// bam_writer.cpp -- see bam_writer.h.  Formats follow SAMv1 sections 4.1 (BGZF), 4.2 (BAM), 5.2 (BAI).  The host half: zlib blocks,
// the file's assembly, the slice pool, write_bam.  It calls nothing of libmgx.so (that half is bam_writer_device.cpp).
#include "bam_writer_parts.h"

#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <cerrno>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

namespace bamout {

std::vector<uint8_t> header_bytes(const samtext::Header& hdr) {
    std::vector<uint8_t> head;
    head.insert(head.end(), {'B', 'A', 'M', 1});
    put<int32_t>(head, (int32_t)hdr.text.size());
    head.insert(head.end(), hdr.text.begin(), hdr.text.end());
    put<int32_t>(head, (int32_t)hdr.ref_name.size());
    for (size_t i = 0; i < hdr.ref_name.size(); ++i) {
        put<int32_t>(head, (int32_t)hdr.ref_name[i].size() + 1);
        head.insert(head.end(), hdr.ref_name[i].begin(), hdr.ref_name[i].end());
        head.push_back(0);
        put<int32_t>(head, (int32_t)hdr.ref_len[i]);
    }
    return head;
}

int open_output(const std::string& path, std::string* err) {
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) *err = "cannot open " + path;
    return fd;
}

bool pwrite_all(int fd, const uint8_t* p, size_t len, uint64_t at) {
    while (len) {
        const ssize_t w = pwrite(fd, p, len, (off_t)at);
        if (w <= 0) { if (w < 0 && errno == EINTR) continue; return false; }
        p += w; len -= (size_t)w; at += (uint64_t)w;
    }
    return true;
}

bool finish_file(int fd, bool ok, uint64_t at, const std::string& path, std::string* err) {
    static const uint8_t kEofBlock[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    ok = ok && pwrite_all(fd, kEofBlock, 28, at);
    ok = (close(fd) == 0) && ok;
    if (!ok) *err = "short write to " + path;
    return ok;
}

bool write_bai(const std::string& path, const std::vector<uint8_t>& bai, std::string* err) {
    const int fd = open_output(path + ".bai", err);
    if (fd < 0) return false;
    bool ok = pwrite_all(fd, bai.data(), bai.size(), 0);
    ok = (close(fd) == 0) && ok;
    if (!ok) *err = "short write to " + path + ".bai";
    return ok;
}

namespace {

constexpr size_t kBgzfHeader = 18, kBgzfFooter = 8;

// A deflate state that is set up once per writer thread and reset per block (deflateInit2 allocates and clears
// ~256 KB every time; a slice holds thousands of blocks).
struct Deflater {
    z_stream zs; bool ok = false; int level;
    explicit Deflater(int lvl) : level(lvl) {
        memset(&zs, 0, sizeof zs);
        ok = deflateInit2(&zs, lvl, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK;
    }
    ~Deflater() { if (ok) deflateEnd(&zs); }
    Deflater(const Deflater&) = delete;
    Deflater& operator=(const Deflater&) = delete;
};

// one BGZF block for in[0, n); appended to out.  level 0..9
bool bgzf_block(const uint8_t* in, size_t n, Deflater* df, std::vector<uint8_t>* out) {
    uint8_t buf[65536];
    if (!df->ok) return false;
    std::unique_ptr<Deflater> stored;           // level 0, only when the block does not fit compressed (incompressible data)
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (attempt == 1) { stored.reset(new Deflater(0)); if (!stored->ok) return false; }
        z_stream& zs = attempt == 0 ? df->zs : stored->zs;
        if (attempt == 0 && deflateReset(&zs) != Z_OK) return false;
        zs.next_in = const_cast<uint8_t*>(in); zs.avail_in = (uInt)n;
        zs.next_out = buf + kBgzfHeader; zs.avail_out = (uInt)(sizeof buf - kBgzfHeader - kBgzfFooter);
        const int rc = deflate(&zs, Z_FINISH);
        const size_t clen = zs.total_out;
        if (rc != Z_STREAM_END) continue;      // did not fit: retry stored (always fits for n <= 0xff00)
        const size_t total = kBgzfHeader + clen + kBgzfFooter;
        static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        memcpy(buf, head, 16);
        const uint16_t bsize = (uint16_t)(total - 1);
        memcpy(buf + 16, &bsize, 2);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n), isize = (uint32_t)n;
        memcpy(buf + kBgzfHeader + clen, &crc, 4);
        memcpy(buf + kBgzfHeader + clen + 4, &isize, 4);
        out->insert(out->end(), buf, buf + total);
        return true;
    }
    return false;
}

// the header in BGZF blocks of its own, with zlib (the device form is in bam_writer_device.cpp)
bool compress_header(int level, const std::vector<uint8_t>& head, std::vector<uint8_t>* file, std::string* err) {
    Deflater df(level);
    for (size_t off = 0; off < head.size(); off += kBlockIn)
        if (!bgzf_block(head.data() + off, std::min<size_t>(kBlockIn, head.size() - off), &df, file)) { *err = "deflate failed"; return false; }
    return true;
}

struct ZlibSlices : SliceCompressor {            // a slice through zlib: a block is deflated when the cutter closes it
    Deflater df;
    explicit ZlibSlices(int level) : df(level) { err = "deflate failed"; }
    void run(const RecordRefs& recs, size_t lo, size_t hi, Slice* s) override {
        std::vector<uint8_t> block;              // the open block (and, for a moment, a record that goes on behind it)
        std::vector<uint64_t> block_at;
        BlockCutter cut;
        block.reserve(kBlockIn + 1024);
        s->vbeg.resize(hi - lo); s->vend.resize(hi - lo);
        auto close = [&](uint64_t n) {
            block_at.push_back(s->bytes.size());
            if (!bgzf_block(block.data(), n, &df, &s->bytes)) s->ok = false;
            block.erase(block.begin(), block.begin() + (std::ptrdiff_t)n);
        };
        for (size_t k = lo; k < hi; ++k) {
            const uint64_t need = 4 + (uint64_t)recs[k].len;
            cut.before(need, close);
            s->vbeg[k - lo] = cut.voff();
            block.resize(block.size() + need);
            put_record(block.data() + block.size() - need, recs[k]);
            cut.after(need, close);
            s->vend[k - lo] = cut.voff();
        }
        cut.close_open(close);
        block_at.push_back(s->bytes.size());
        to_compressed_offsets(s, block_at);
    }
};

// The slices [lo[s], lo[s + 1]) compressed on T threads, each with a compressor of its own, and written to fd behind one another
// from base[0] on while later ones are still being compressed: as soon as slice s is done its place in the file is known (base[s],
// filled in here up to base[n_slices], the end), the writer thread puts it there and drops its bytes; the pool compresses ahead.
// false: a slice could not be compressed, *err says why.  *all_written: every byte went into the file.
using MakeCompressor = std::function<std::unique_ptr<SliceCompressor>()>;
bool compress_and_write_slices(int fd, const RecordRefs& recs, const std::vector<size_t>& lo, int T, const MakeCompressor& make, const StageClock& clock,
                               std::vector<Slice>& slices, std::vector<uint64_t>& base, bool* all_written, std::string* err) {
    const size_t n_slices = slices.size();
    std::atomic<bool> write_ok{true};
    size_t next = 0;                            // slices are claimed in order
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> done(n_slices, 0);
    std::string first_err;
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t)
        pool.emplace_back([&]() {
            const std::unique_ptr<SliceCompressor> z = make();
            for (;;) {
                size_t s;
                { std::lock_guard<std::mutex> g(mu); if (next >= n_slices) return; s = next++; }
                z->run(recs, lo[s], lo[s + 1], &slices[s]);
                { std::lock_guard<std::mutex> g(mu); if (!slices[s].ok && first_err.empty()) first_err = z->err; done[s] = 1; }
                cv.notify_all();
            }
        });
    std::vector<size_t> wq;                     // slices whose place is known, not yet written
    size_t wq_next = 0; bool wq_closed = false;
    std::mutex wmu; std::condition_variable wcv;
    // ONE writer: buffered pwrite()s of one file take its inode lock in turn, and threads that queue for it write slower than
    // a single one does (tools/dev_tmpfs_write.py on the GPU box: 1 thread 6.3 GB/s, 4 threads 3.7, 8 threads 3.5)
    std::thread writer([&]() {
        for (;;) {
            size_t s;
            {
                std::unique_lock<std::mutex> lk(wmu);
                wcv.wait(lk, [&] { return wq_next < wq.size() || wq_closed; });
                if (wq_next >= wq.size()) return;
                s = wq[wq_next++];
            }
            if (slices[s].ok && !pwrite_all(fd, slices[s].bytes.data(), slices[s].bytes.size(), base[s])) write_ok = false;
            std::vector<uint8_t>().swap(slices[s].bytes);
        }
    });
    for (size_t s = 0; s < n_slices; ++s) {
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done[s] != 0; }); }
        base[s + 1] = base[s] + slices[s].bytes.size();
        if (s == 0) clock.stamp("first slice compressed");
        { std::lock_guard<std::mutex> g(wmu); wq.push_back(s); }
        wcv.notify_one();
    }
    { std::lock_guard<std::mutex> g(wmu); wq_closed = true; }
    wcv.notify_all();
    clock.stamp("last slice compressed");
    for (auto& th : pool) th.join();
    clock.stamp("compressors released");
    writer.join();
    clock.stamp("file written");
    *all_written = write_ok.load();
    for (const Slice& s : slices) if (!s.ok) { *err = first_err; return false; }
    return true;
}

inline uint64_t rebase(uint64_t v, uint64_t base) { return (((v >> 16) + base) << 16) | (v & 0xffff); }

}  // namespace

bool write_bam(const std::string& path, const samtext::Header& hdr, const RecordRefs& recs,
               int threads, int level, int device, std::string* err) {
    const StageClock clock{"write_bam", 28};
    if (device >= 0 && !(compress_header_on && make_pinned_compressor)) { *err = "this program was linked without the device compressor"; return false; }
    std::vector<uint8_t> file;
    if (!(device >= 0 ? compress_header_on(device, header_bytes(hdr), &file, err) : compress_header(level, header_bytes(hdr), &file, err))) return false;
    clock.stamp("header compressed");

    // ---- records: contiguous slices compressed independently (sortmardup/main.cpp:371-421)
    const size_t n = recs.size();
    // device compressor: the writer threads only gather records into pinned memory, a few of them saturate it
    const int T = device >= 0 ? std::max(1, std::min(threads, 8)) : std::max(1, threads);
    const size_t n_slices = n ? std::min<size_t>((size_t)T * (device >= 0 ? 16 : 4), (n + 4095) / 4096) : 0;
    std::vector<Slice> slices(n_slices);
    std::vector<size_t> lo(n_slices + 1, 0);
    for (size_t s = 0; s <= n_slices; ++s) lo[s] = n_slices ? n * s / n_slices : 0;
    const int fd = open_output(path, err);
    if (fd < 0) return false;
    const bool head_ok = pwrite_all(fd, file.data(), file.size(), 0);
    std::vector<uint64_t> base(n_slices + 1, file.size());
    MakeCompressor make = [&]() { return std::unique_ptr<SliceCompressor>(new ZlibSlices(level)); };
    if (device >= 0) make = [&]() { auto z = make_pinned_compressor(device); clock.stamp("a writer's batches are ready"); return z; };
    bool body_ok = false;
    if (!compress_and_write_slices(fd, recs, lo, T, make, clock, slices, base, &body_ok, err)) { close(fd); return false; }
    if (!finish_file(fd, head_ok && body_ok, base[n_slices], path, err)) return false;

    // ---- BAI (merge of the per-slice offsets, the job of the reference's merge_index)
    size_t cur_slice = 0;
    auto voff = [&](size_t k, uint64_t* vb, uint64_t* ve) {
        while (k >= lo[cur_slice + 1]) ++cur_slice;          // k only grows
        *vb = rebase(slices[cur_slice].vbeg[k - lo[cur_slice]], base[cur_slice]);
        *ve = rebase(slices[cur_slice].vend[k - lo[cur_slice]], base[cur_slice]);
    };
    const bool iok = write_bai(path, bai_bytes(hdr.ref_name.size(), recs, voff), err);
    clock.stamp("index written");
    return iok;
}

}  // namespace bamout
