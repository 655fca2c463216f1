// gz_source.h -- compressed SAM input for the sortmardup-compatible CLI: a piece source (slice_cut.h) of inflated text.
#pragma once

#include <zlib.h>

#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/mgx_bgzf.h"
#include "slice_cut.h"

// gzip / BGZF input -> inflated text, in order (htslib reads compressed SAM the same way: bgzf.c:1100-1180).
//   BGZF: the block scanner finds whole blocks in what was read (straight into a batch's pinned input), a batch is inflated
//         on the device (mgx_bgzf_inflate_*) and its text comes back into the batch's pinned output, which the
//         parsers read in place.  kSlots batches, up to kDepth of them in flight; a batch is reused once the text cut from it
//         has been parsed.  MGX_CLI_INFLATE=host inflates the same batches with zlib on a gang of `threads` host threads
//         that the reader starts per batch, beside the parsers (A/B).  MGX_CLI_INFLATE_BATCH: compressed bytes per batch.
//   gzip: from the first member that is not BGZF on (bgzf.c:1143-1148), zlib on this thread: correct, but serial.
// Text that starts with the BAM magic is refused (`name` says whose it is): err().
class GzSource : public slicecut::PieceSource {
public:
    static constexpr int kSlots = 4, kDepth = 2;

    GzSource(FILE* f, std::string head, std::string name, int device, int threads, bool host);
    ~GzSource() override;
    const std::string& err() const override { return err_; }
    // Stops the source: a next() waiting for a batch to come free returns false (the pipeline failed: the slices that
    // hold the batches may never be parsed).
    void abort() override;
    // The next piece of text; false at the end of the input or on an error (err() says which).
    bool next(slicecut::TextChunk* out) override;
    // device memory the inflate batches will still take, beyond what they hold now (for the -z device memory check, which
    // sees the batches allocated so far as used), and the inflation ratio so far
    uint64_t hbm_bytes_to_come() const;
    double ratio() const { return in_bytes_ ? (double)out_bytes_ / (double)in_bytes_ : 1.0; }
    uint64_t in_bytes() const { return in_bytes_; }
    uint64_t out_bytes() const { return out_bytes_; }
    double seconds_waiting() const { return wait_s_; }

private:
    struct Slot {
        mgx_bgzf_inflate_t* b = nullptr;
        uint8_t* in = nullptr; uint64_t* io = nullptr; uint64_t* oo = nullptr;
        std::vector<uint8_t> host_in; std::vector<char> host_out;
        uint64_t n_out = 0, at = 0;
        bool busy = false;
    };
    bool next_piece(slicecut::TextChunk* out);
    int free_slot();
    void release(int k);
    bool setup(Slot& s);
    bool fill_and_submit(int k);
    bool host_inflate(Slot& s, uint32_t nb);
    bool next_gzip(slicecut::TextChunk* out);

    FILE* f_;
    std::vector<uint8_t> pending_, gz_rest_, zin_;
    std::vector<uint32_t> isize_;
    std::vector<std::unique_ptr<uint64_t[]>> host_off_;
    std::string name_;
    int device_, threads_;
    bool host_;
    mgx_bgzf_t* ctx_ = nullptr;
    Slot slots_[kSlots];
    std::deque<int> flight_;
    uint64_t in_cap_ = 64ull << 20, out_cap_ = 0;
    uint32_t max_blocks_ = 0;
    std::mutex mu_; std::condition_variable cv_;       // mu_ guards aborted_ and the slots' busy flags
    bool aborted_ = false;
    bool file_eof_ = false, bgzf_done_ = false, gzip_tail_ = false, gzip_ = false, eof_block_ = false, first_ = true;
    z_stream zs_{}; bool zinit_ = false, in_member_ = false;
    uint64_t in_bytes_ = 0, out_bytes_ = 0;
    double wait_s_ = 0;
    std::string err_;
};
