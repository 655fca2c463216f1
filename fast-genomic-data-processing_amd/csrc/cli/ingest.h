// ingest.h -- the device bring-up and the parse / pack / commit half of the ingest of the sortmardup-compatible CLI
// (the pipeline's overview: sortmardup_main.cpp; the reader's half: slice_cut.h).
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/mgx_bgzf.h"
#include "../../../include/mgx_sam.h"
#include "mgx_sortdedup.h"
#include "sam_text.h"
#include "slice_cut.h"

bool sam_on_device();                                          // MGX_CLI_SAM=device: SAM text is encoded on the device
bool pread_all(int fd, char* dst, size_t n, uint64_t at);      // all n bytes at `at`; false on a read error or a short file

enum OutMode { kOutDevice, kOutPinned, kOutZlib };      // -z: where the output is made

// what the writer needs per record, in ARRIVAL order
struct Kept { const uint8_t* blob; uint32_t len; int32_t tid, beg, end; bool mapped; };

struct Chunk {                       // one parsed + packed slice
    std::vector<uint16_t> flag; std::vector<int32_t> tid; std::vector<int64_t> pos; std::vector<int32_t> end;
    std::vector<uint32_t> cigar; std::vector<uint64_t> cigar_off{0};
    std::vector<uint16_t> score;                                        // BAMRecord::score per record, from the parser
    std::vector<char> qname; std::vector<uint64_t> qname_off{0};
    std::vector<uint8_t> blob; std::vector<uint64_t> blob_off{0};      // BAM bytes per record (kept until the output is written)
    std::vector<mgx_rec_t> recs; std::vector<uint32_t> input_index;   // arrival order inside the slice
    std::vector<uint64_t> rec_addr; std::vector<uint32_t> rec_len;     // device-encoded SAM with -z device: every record's own address in HBM
    uint64_t dev_base = 0;               // -z device: where the slice's BAM bytes are in HBM (blob is dropped then)
    uint64_t arrival_base = 0;           // set at commit: the slice's first arrival index
    std::vector<Kept> kept;              // what the writer needs per record, slice-local arrival order (filled by the parser thread)
    std::string err;
};

// The device contexts come up on a thread of their own (the HIP runtime takes a few tenths of a second to start)
// while the first slices are already being parsed; a parser waits for them only when it has bytes for the device.
// The thread is joined by join() or by the destructor, whichever way main() is left.
class GpuBringUp {
public:
    // text_bytes: bytes of SAM text expected (0: unknown); inflate_hbm: device memory the input side will still take;
    // L: sum of the reference lengths
    GpuBringUp(int device, OutMode out_mode, uint64_t text_bytes, uint64_t inflate_hbm, uint64_t L);
    ~GpuBringUp() { join(); }
    void join() { if (thread_.joinable()) thread_.join(); }
    bool ready();                                    // waits for the store and the sort context; false: error() says why
    int state_now();                                 // 0 starting, 1 ready, -1 failed
    const std::string& error() const { return error_; }
    // valid once ready() has returned true (out_mode: after join(); -z device falls back to -z pinned when the records
    // cannot fit into the device's free memory)
    mgx_bgzf_t* zctx = nullptr; mgx_bgzf_store_t* store = nullptr; mgx_sortdedup_t* sd = nullptr;
    OutMode out_mode;

private:
    void run(int device, uint64_t text_bytes, uint64_t inflate_hbm, uint64_t L);
    std::mutex mu_; std::condition_variable cv_; int state_ = 0;      // mu_ guards state_ and error_
    std::string error_;
    std::thread thread_;
};

// The slice queue, the parser pool and the in-order commit.  The reader calls push() for every slice and finish() at the end.
class Ingest {
public:
    // in_base / in_fd: the mapping (or NULL) and the descriptor of a regular input file, for slices that are ranges of it;
    // src: the piece source to stop when the pipeline fails (or NULL)
    Ingest(const samtext::Header& hdr, GpuBringUp& gpu, int threads, const char* in_base, int in_fd, slicecut::PieceSource* src);
    ~Ingest() { finish(); }
    bool push(slicecut::Slice sl);                   // numbers the slice, waits for room in the queue; false once failed
    void fail(const std::string& msg);               // the first message is kept
    void finish();                                   // no more slices: waits for the parsers, drops what was never parsed
    bool failed() const { return failed_.load(); }
    const std::string& error() const { return first_error_; }
    uint64_t n_slices() const { return seq_; }
    // the result, once finish() has returned
    std::vector<std::unique_ptr<Chunk>> kept_chunks;         // committed slices: their writer records, and (not -z device) the BAM bytes
    uint64_t n_total = 0;
    double commit_seconds = 0, upload_seconds = 0;           // serial part of the ingest (MGX_CLI_TRACE)

private:
    struct SamBatch { mgx_sam_batch_t* b = nullptr; uint64_t cap = 0, max_rec = 0; };      // one per parser thread
    void worker();
    bool parse(const slicecut::Slice& sl, std::vector<char>* text_buf, SamBatch* sb, Chunk* ch);
    void parse_slice_device(const char* data, size_t size, SamBatch* sb, Chunk* c);
    bool finish_chunk(std::unique_ptr<Chunk> ch, uint64_t seq);
    void commit_ready(std::vector<std::vector<mgx_rec_t>>* trash);      // called with commit_mu_ held

    const samtext::Header& hdr_; GpuBringUp& gpu_; const char* in_base_; int in_fd_; slicecut::PieceSource* src_;
    uint64_t seq_ = 0;                                       // reader thread only
    std::mutex mu_; std::condition_variable cv_work_, cv_room_;      // mu_ guards queue_, done_reading_, first_error_
    std::deque<slicecut::Slice> queue_; size_t queue_cap_; bool done_reading_ = false;
    std::atomic<bool> failed_{false}; std::string first_error_;
    std::mutex commit_mu_;                                   // guards ready_, next_commit_ and the public result
    std::map<uint64_t, std::unique_ptr<Chunk>> ready_; uint64_t next_commit_ = 0;
    std::vector<std::thread> pool_;
    mgx_sam_table_t* sam_table_ = nullptr;                   // MGX_CLI_SAM=device: non-NULL
    std::atomic<uint64_t> sam_lines_device_{0}, sam_lines_host_{0};
    std::atomic<uint64_t> sam_ns_[5] = {};                   // thread time per step of parse_slice_device, for MGX_CLI_TRACE
};
