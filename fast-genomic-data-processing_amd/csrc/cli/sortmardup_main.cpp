// sortmardup_main.cpp -- `sortmardup`: coordinate sort + mark duplicates, SAM text in, BAM + BAI out.
//
// Same command line and outputs as the reference tool (sortmardup/main.cpp:47-78):
//     sortmardup [-I input.sam] [-t threads] [-b] -O output.bam
// text SAM from a file or stdin; output.bam is replaced if it exists; output.bam.bai is written
// next to it; stage timings go to stdout (time_stamp(), main.cpp:597-607).
// Input formats: plain SAM text; BGZF-compressed SAM (inflated on the device in batches, the text parsed in place from
// the pinned buffers: gz_source.cpp); plain gzip, one member or several (zlib on the reader thread: serial).
// The gzip magic in the first two bytes decides; BAM input is refused unless -b says that the input is BAM.
// -b (extension): the input is BGZF BAM, from a file or stdin.  The same inflate batches; the header is parsed on the host,
// and where the records start and their sort / duplicate keys are found on the device behind each batch's inflate
// (mgx_bam.h); the parsers only re-derive what the device rules declined, pair the records
// (mgx_bam_pack_keys) and hand the record bytes on unchanged.  Anything else given with -b is refused.  MGX_CLI_BAM=host
// walks and keys the records on the host instead (A/B, debugging).
//
// Ingest is a pipeline over bounded slices of the text, the shape of the reference's reader thread feeding its
// shuffle threads through a bounded queue of line blocks (main.cpp:505-562, 129-192):
//   reader (main thread)   cuts ~8 MB slices at a template boundary (a queryname group never straddles two slices,
//                          so mates are found inside their slice) and queues them; of a regular file it only reads
//                          the few KB around every cut; a stream and inflated text come in pieces that are cut in
//                          place; the queue is bounded                                          (slice_cut.cpp)
//   parsers (-t threads)   read their slice (regular file), parse it into BAM-ready records, run             (ingest.cpp)
//                          mgx_sortdedup_pack on it (host keys, arrival order, slice-local mate indices), hand the
//                          BAM bytes to the device record store (-z device) and build the writer's per-record view
//   commit (in slice order, by whichever parser finishes the next slice)
//                          turns mate indices into global arrival indices and hands the packed records to
//                          mgx_sortdedup_upload_chunk: staging and the PCIe copy run while later slices are
//                          still being parsed
// then mgx_sortdedup_run (MI355X: radix sorts + duplicate search) and the output: the records are gathered in sorted
// order, duplicate-flagged and BGZF-compressed on the device (-z device, mgx_bgzf_store_emit), or gathered by writer
// threads for the device compressor (-z pinned) or for zlib (-z zlib, the reference's way); BAI from the records'
// virtual offsets.
// There is no CPU fallback: without a HIP device the tool exits with an error.
// main() below is the list of the stages: options, input, header, device bring-up (ingest.cpp), ingest, sort, output
// (bam_writer.cpp); the fork-join gangs are gang.h.
#include <fcntl.h>
#include <getopt.h>
#include <malloc.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "bam_writer.h"
#include "gang.h"
#include "gz_source.h"
#include "ingest.h"
#include "mgx_pairhmm.h"       // mgx_last_error
#include "sam_text.h"
#include "slice_cut.h"

namespace {

using clk = std::chrono::steady_clock;
clk::time_point g_t0, g_last;
void time_stamp(const char* hint) {
    const auto now = clk::now();
    printf("%s: %.3f s (total %.3f s)\n", hint, std::chrono::duration<double>(now - g_last).count(),
           std::chrono::duration<double>(now - g_t0).count());
    fflush(stdout);
    g_last = now;
}

struct Options {
    const char* in_path = nullptr; const char* out_path = nullptr;
    int threads = (int)std::thread::hardware_concurrency();
    int device = 0, level = 6;
    OutMode out_mode = kOutDevice;
    size_t slice_bytes = 8u << 20;     // 8 MB: 20 M records parse in 1.2 s (32 MB slices: 2.1 s -- fewer, longer tasks per thread)
    bool bam = false;                  // -b: the input is BGZF BAM
};

// False (after the usage line) when the command line is not one the tool takes.
bool parse_options(int argc, char** argv, Options* o) {
    auto usage = [&]() { fprintf(stderr, "usage: %s [-I input.sam] [-t num] [-b] -O output.bam\n", argv[0]); return false; };
    int c;
    while ((c = getopt(argc, argv, "I:O:t:d:l:s:z:b")) >= 0) {
        switch (c) {
            case 'I': o->in_path = optarg; break;
            case 'O': o->out_path = optarg; break;
            case 't': o->threads = atoi(optarg); break;
            case 'd': o->device = atoi(optarg); break;       // extension: HIP device ordinal
            case 'l': o->level = atoi(optarg); break;        // extension: deflate level (with -z zlib)
            case 'z':                                        // extension: where the output is made
                // device (default): BAM bytes resident in HBM from ingest on, gathered + compressed on the device
                // pinned: BAM bytes in host memory, gathered by the writer threads into pinned batches, compressed on the device
                // zlib:   BAM bytes in host memory, zlib at -l level on the writer threads (the reference's way)
                o->out_mode = !strcmp(optarg, "zlib") ? kOutZlib : !strcmp(optarg, "pinned") ? kOutPinned : kOutDevice;
                break;
            case 's': o->slice_bytes = (size_t)atoll(optarg); break;   // extension: bytes of SAM text per slice
            case 'b': o->bam = true; break;                  // extension: the input is BGZF BAM
            default: return usage();
        }
    }
    if (!o->out_path) return usage();
    if (o->threads < 1) o->threads = 1;
    if (o->slice_bytes < 1024) o->slice_bytes = 1024;
    return true;
}

// The input: a regular file of plain text is read by the parser threads themselves (their own slice, in place from a populated
// mapping or by pread into their own buffer): the reader only looks at a few KB around every cut to place it on a
// queryname-group boundary.  (Mapping the file and letting every page fault on its own cost 1.8 M page faults per 7 GB and
// made the ingest time vary by 50 % from run to run.)  Everything else -- a stream, compressed input -- is read through
// `f` by a piece source.
struct Input {
    const char* path = nullptr; FILE* f = nullptr;
    uint64_t file_bytes = 0;                                 // of a regular file
    bool gz = false;                                         // the gzip magic in the first two bytes: gzip / BGZF
    std::string first_bytes;                                 // what that check read from a stream
    int fd = -1;                                             // a regular file of plain text; base: its mapping, or NULL
    const char* base = nullptr;

    bool open(const char* in_path) {
        path = in_path;
        f = path ? fopen(path, "rb") : stdin;
        if (!f) return false;
        { struct stat sb; if (path && stat(path, &sb) == 0) file_bytes = (uint64_t)sb.st_size; }
#ifdef F_SETPIPE_SZ
        (void)fcntl(fileno(f), F_SETPIPE_SZ, 1 << 20);      // a pipe on stdin: 1 MB instead of 64 KB per hand-over (ignored for files)
#endif
        setvbuf(f, nullptr, _IONBF, 0);                      // the piece sources ask for megabytes at a time: no second buffer
        const int fd0 = (path && file_bytes) ? fileno(f) : -1;
        unsigned char m[2] = {0, 0};
        size_t got = 0;
        if (fd0 >= 0) got = pread(fd0, m, 2, 0) == 2 ? 2 : 0;
        else for (int c0; got < 2 && (c0 = fgetc(f)) != EOF;) m[got++] = (unsigned char)c0;
        gz = got == 2 && m[0] == 0x1f && m[1] == 0x8b;
        if (fd0 < 0) first_bytes.assign(reinterpret_cast<char*>(m), got);
        fd = gz ? -1 : fd0;
        // Round 3: the parsers read their slice IN PLACE from a mapping of the file, after one madvise(MADV_POPULATE_READ) per slice has
        // the kernel fill in its page-table entries (2048 of them in one call, no fault per page), instead of copying the slice out of
        // the page cache with pread: 200 M records ingest 5.7 -> 4.5-5.1 s on one box.  MGX_CLI_MMAP_IN=0, a kernel without
        // MADV_POPULATE_READ or a file that cannot be mapped keep the pread path.
#ifdef MADV_POPULATE_READ
        const char* e = getenv("MGX_CLI_MMAP_IN");
        if (fd >= 0 && (!e || atoi(e) != 0)) {
            void* mp = mmap(nullptr, (size_t)file_bytes, PROT_READ, MAP_SHARED, fd, 0);
            if (mp != MAP_FAILED) {
                // is the advice known to this kernel? (EINVAL on kernels before 5.14)
                if (madvise(mp, std::min<size_t>((size_t)file_bytes, 4096), MADV_POPULATE_READ) == 0) base = static_cast<const char*>(mp);
                else (void)munmap(mp, (size_t)file_bytes);
            }
        }
#endif
        return true;
    }
    const char* name() const { return path ? path : "stdin"; }
    void close() { if (path) fclose(f); }
    // The header of a regular file: its head, more of it until a line that does not start with '@' is in sight.  *body: where
    // the first alignment line starts.  False on a read error.
    bool read_file_header(samtext::Header* hdr, uint64_t* body) const {
        std::vector<char> head;
        for (size_t want = 1u << 20;; want *= 4) {
            head.resize((size_t)std::min<uint64_t>(want, file_bytes));
            if (!pread_all(fd, head.data(), head.size(), 0)) return false;
            size_t off = 0; bool body_seen = false;
            while (off < head.size()) {
                if (head[off] != '@') { body_seen = true; break; }
                const char* nl = (const char*)memchr(head.data() + off, '\n', head.size() - off);
                if (!nl) break;
                off = (size_t)(nl - head.data()) + 1;
            }
            if (body_seen || head.size() == file_bytes) break;
        }
        *body = samtext::parse_header(head.data(), head.size(), hdr);
        return true;
    }
};

// The committed slices' writer records, flattened into arrival order (the array's pages are first touched by the copying gang).
bamout::NoInitVector<Kept> flatten(std::vector<std::unique_ptr<Chunk>>& kept_chunks, size_t n, int threads) {
    bamout::NoInitVector<Kept> by_arrival(n);
    std::atomic<size_t> next_chunk{0};
    gang::run_gang((size_t)std::max(1, std::min(threads, 16)), [&](size_t) {
        for (size_t i; (i = next_chunk.fetch_add(1)) < kept_chunks.size();) {
            Chunk& ch = *kept_chunks[i];
            if (!ch.kept.empty()) memcpy(&by_arrival[ch.arrival_base], ch.kept.data(), ch.kept.size() * sizeof(Kept));
            std::vector<Kept>().swap(ch.kept);
        }
    });
    return by_arrival;
}

// mgx_sortdedup_run on the n uploaded records; the output order and the duplicate marks, by arrival index.  False: mgx_last_error().
bool sort_and_fetch(mgx_sortdedup_t* sd, size_t n, int threads, bamout::NoInitVector<uint32_t>* order, bamout::NoInitVector<uint8_t>* dup) {
    if (mgx_sortdedup_upload_end(sd, n)) return false;
    order->resize(n); dup->resize(n);
    // the results land in fresh memory: its pages are touched by all threads first (a device-to-host copy into untouched
    // pageable memory faults them in one by one on the runtime's copy path: up to 0.5 s for the 1 GB of 200 M records)
    const size_t T = (size_t)std::max(1, std::min(threads, 16));
    gang::run_gang(T, [&](size_t t) {
        auto touch = [&](uint8_t* p, size_t bytes) { for (size_t o = bytes * t / T & ~(size_t)4095, e = bytes * (t + 1) / T; o < e; o += 4096) p[o] = 0; };
        touch(reinterpret_cast<uint8_t*>(order->data()), n * sizeof(uint32_t));
        touch(dup->data(), n);
    });
    return !(mgx_sortdedup_run(sd) || mgx_sortdedup_results(sd, order->data(), dup->data()));
}

// mark + compress + write: the records in output order, to out_path and out_path.bai
bool write_output(const Options& opt, const GpuBringUp& gpu, const samtext::Header& hdr, bamout::NoInitVector<Kept>& by_arrival,
                  bamout::NoInitVector<uint32_t>& order, bamout::NoInitVector<uint8_t>& dup, std::string* err) {
    const size_t n = order.size();
    bamout::RecordRefs out(n);
    // a gather with random reads from by_arrival: spread over the threads
    const size_t T = (size_t)std::max(1, std::min(opt.threads, 16));
    gang::run_gang(T, [&](size_t t) {
        const auto part = gang::gang_range(n, t, T);
        for (size_t q = part.begin; q < part.end; ++q) {
            const uint32_t arrival = order[q];
            const Kept& k = by_arrival[arrival];
            out[q] = bamout::RecordRef{k.blob, k.len, k.tid, k.beg, k.end, dup[arrival] != 0, k.mapped};
        }
    });
    // what the output stage no longer needs goes back to the kernel on a thread of its own while the stream is written (at 200 M
    // records: 7 GB of per-record bookkeeping that would otherwise be torn down after the last byte is on disk)
    // (madvise, not free: unmapping takes the address space's lock for writing for as long as it frees pages, and the output
    // stage's threads are first-touching their own arrays right now; dropping the pages only needs it for reading)
    std::atomic<bool> writer_returned{false};
    std::thread reaper([&]() {
        while (gpu.store && !bamout::g_store_arrays_ready.load() && !writer_returned.load()) std::this_thread::sleep_for(std::chrono::milliseconds(2));
        auto drop = [](void* p, size_t bytes) {
            const uintptr_t a = ((uintptr_t)p + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)p + bytes) & ~(uintptr_t)4095;
            if (e > a) (void)madvise((void*)a, e - a, MADV_DONTNEED);
        };
        drop(by_arrival.data(), by_arrival.size() * sizeof(Kept));
        drop(order.data(), order.size() * sizeof(uint32_t));
        drop(dup.data(), dup.size());
    });
    const bool wrote = gpu.store ? bamout::write_bam_store(opt.out_path, hdr, out, gpu.zctx, gpu.store, opt.threads, err)
                                 : bamout::write_bam(opt.out_path, hdr, out, opt.threads, opt.level, gpu.out_mode == kOutPinned ? opt.device : -1, err);
    writer_returned.store(true);
    reaper.join();
    return wrote;
}

}  // namespace

int main(int argc, char** argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);   // the three sorts overlap on three streams: keep them on distinct hardware queues
    // The parser threads allocate and free a slice's arrays (megabytes each) thousands of times: keep them inside the malloc
    // arenas instead of one mmap / munmap -- and its page faults on fresh zero pages -- per array.
    mallopt(M_MMAP_THRESHOLD, 32 << 20);
    mallopt(M_TRIM_THRESHOLD, 1 << 30);
    mallopt(M_TOP_PAD, 64 << 20);
    Options opt;
    if (!parse_options(argc, argv, &opt)) return 2;
    g_t0 = g_last = clk::now();
    time_stamp("program start");
    unlink(opt.out_path);                                    // main.cpp:66-68

    Input in;
    if (!in.open(opt.in_path)) { fprintf(stderr, "cannot read %s\n", in.name()); return 1; }

    // ---- header: of a regular file from its head; of a piece source, the '@' lines of its first pieces
    samtext::Header hdr;
    uint64_t body_pos = 0;                                   // regular file: where the alignment lines start
    std::unique_ptr<slicecut::PieceSource> src;              // everything else
    GzSource* gzs = nullptr;
    slicecut::PieceHead head; std::string carry;             // text of the pieces read so far that is not in a slice yet
    if (opt.bam) {
        if (!in.gz) { fprintf(stderr, "%s is not BAM: -b reads BGZF-compressed BAM, and this is not compressed\n", in.name()); return 1; }
        const char* e = getenv("MGX_CLI_INFLATE"); const char* eb = getenv("MGX_CLI_BAM");
        src.reset(gzs = new GzSource(in.f, in.first_bytes, in.name(), opt.device, opt.threads, e && !strcmp(e, "host"),
                                     eb && !strcmp(eb, "host") ? GzSource::kBamHost : GzSource::kBamDevice));
        if (!gzs->read_bam_header(&hdr)) { fprintf(stderr, "%s\n", gzs->err().c_str()); return 1; }
    } else if (in.fd >= 0) {
        if (!in.read_file_header(&hdr, &body_pos)) { fprintf(stderr, "cannot read %s\n", in.path); return 1; }
    } else {
        const char* e = getenv("MGX_CLI_INFLATE");
        if (in.gz) src.reset(gzs = new GzSource(in.f, in.first_bytes, in.name(), opt.device, opt.threads, e && !strcmp(e, "host")));
        else src.reset(new slicecut::StreamSource(in.f, in.first_bytes));
        if (!slicecut::scan_piece_header(*src, &head)) { fprintf(stderr, "%s\n", src->err().c_str()); return 1; }
        const size_t body = samtext::parse_header(head.text.data(), head.text.size(), &hdr);
        carry.assign(head.text, body, std::string::npos);
    }
    uint64_t L = 0;
    for (uint64_t x : hdr.ref_len) L += x;
    // bytes of SAM text, for the sizes of the device buffers: of compressed input, the file's size times the ratio of what is inflated so far
    // (the sizes are stated in SAM text, of which BAM bytes are about 0.6)
    const uint64_t text_bytes = gzs ? (uint64_t)((double)in.file_bytes * gzs->ratio() * (opt.bam ? 5.0 / 3.0 : 1.0)) : in.file_bytes;

    // MGX_CLI_SAM=device: every parser thread's batch holds a slice of text, twice that for its records and their arrays
    const uint64_t sam_hbm = !opt.bam && sam_on_device() ? (uint64_t)opt.threads * opt.slice_bytes * 5 : 0;
    GpuBringUp gpu(opt.device, opt.out_mode, text_bytes, (gzs ? gzs->hbm_bytes_to_come() : 0) + sam_hbm, L);

    // ---- ingest: the reader (this thread) cuts slices, the parsers take them from the queue
    Ingest ingest(hdr, gpu, opt.threads, in.base, in.fd, src.get());
    const slicecut::Push push = [&](slicecut::Slice sl) { return ingest.push(std::move(sl)); };
    if (opt.bam) {
        if (!gzs->cut_bam(opt.slice_bytes, push, [&] { return ingest.failed(); })) ingest.fail(gzs->err());
    } else if (in.fd >= 0) {
        const int fd = in.fd;
        if (!slicecut::cut_file_ranges([fd](char* dst, size_t n, uint64_t at) { return pread_all(fd, dst, n, at); }, body_pos, in.file_bytes,
                                       opt.slice_bytes, push))
            ingest.fail("read error on the input file");
    } else if (!slicecut::cut_pieces(*src, std::move(head), std::move(carry), opt.slice_bytes, push, [&] { return ingest.failed(); })) ingest.fail(src->err());
    ingest.finish();
    if (gzs && getenv("MGX_CLI_TRACE"))
        fprintf(stderr, "  inflate: %.3f GB compressed -> %.3f GB of text, %.3f s waiting for the device\n", gzs->in_bytes() / 1e9, gzs->out_bytes() / 1e9, gzs->seconds_waiting());
    src.reset();                                             // the inflate batches' pinned and device memory
    gpu.join();
    if (!gpu.ready()) { fprintf(stderr, "GPU: %s\n", gpu.error().c_str()); return 1; }
    in.close();
    if (ingest.failed()) { fprintf(stderr, "%s\n", ingest.error().c_str()); return 1; }
    const size_t n = (size_t)ingest.n_total;
    bamout::NoInitVector<Kept> by_arrival = flatten(ingest.kept_chunks, n, opt.threads);
    printf("%zu alignment records, %zu reference sequences, %llu slices\n", n, hdr.ref_name.size(), (unsigned long long)ingest.n_slices());
    time_stamp("read + parse + pair + upload done");
    if (getenv("MGX_CLI_TRACE")) fprintf(stderr, "  ingest: %.3f s inside the in-order commit (one thread at a time), %.3f s of it in mgx_sortdedup_upload_chunk\n", ingest.commit_seconds, ingest.upload_seconds);

    // ---- sort + duplicate search
    bamout::NoInitVector<uint32_t> order; bamout::NoInitVector<uint8_t> dup;
    if (!sort_and_fetch(gpu.sd, n, opt.threads, &order, &dup)) { fprintf(stderr, "GPU: %s\n", mgx_last_error()); return 1; }
    mgx_sortdedup_stats_t st{};
    mgx_sortdedup_stats(gpu.sd, &st);
    printf("double pairs %llu, single pairs %llu, records marked duplicate %llu, device pipeline %.3f ms\n",
           (unsigned long long)st.n_double, (unsigned long long)st.n_single, (unsigned long long)st.n_dup_records, st.ms_total);
    mgx_sortdedup_destroy(gpu.sd);
    time_stamp("sort + duplicate search done");

    // ---- mark + compress + write
    std::string err;
    if (!write_output(opt, gpu, hdr, by_arrival, order, dup, &err)) { fprintf(stderr, "write: %s\n", err.c_str()); return 1; }
    time_stamp("output done");
    // Both files are closed.  What is left is tearing down ~N small records' bookkeeping, the arenas and the HIP runtime --
    // a few tenths of a second at 20 M records that change nothing on disk: leave it to the kernel.
    fflush(stdout); fflush(stderr);
    _exit(0);
}
