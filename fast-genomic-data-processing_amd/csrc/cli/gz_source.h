// gz_source.h -- compressed input for the sortmardup-compatible CLI: a piece source (slice_cut.h) of inflated SAM text, and
// with -b the source of BAM records, found and keyed on the device behind the inflate.
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

#include "../../../include/mgx_bam.h"
#include "../../../include/mgx_bgzf.h"
#include "sam_text.h"
#include "slice_cut.h"

// gzip / BGZF input -> inflated text, in order (htslib reads compressed SAM the same way: bgzf.c:1100-1180).
//   BGZF: the block scanner finds whole blocks in what was read (straight into a batch's pinned input), a batch is inflated
//         on the device (mgx_bgzf_inflate_*) and its text comes back into the batch's pinned output, which the
//         parsers read in place.  kSlots batches, up to kDepth of them in flight; a batch is reused once the text cut from it
//         has been parsed.  MGX_CLI_INFLATE=host inflates the same batches with zlib on a gang of `threads` host threads
//         that the reader starts per batch, beside the parsers (A/B).  MGX_CLI_INFLATE_BATCH: compressed bytes per batch.
//   gzip: from the first member that is not BGZF on (bgzf.c:1143-1148), zlib on this thread: correct, but serial.
// Text that starts with the BAM magic is refused (`name` says whose it is): err().
//   BAM (-b): the same batches; read_bam_header() parses the header on the host from the first batches' bytes, cut_bam()
//         submits the record index + keys (mgx_bam_batch_*) behind each batch's inflate, with `first` taken from where the
//         batch before ended, and cuts slices of whole records where a read-name group ends (the same_qname bits): in place
//         in the batch's pinned output, which they hold the way text slices do.  What straddles two batches -- the record cut
//         by a batch's end, the name group around it -- is copied into an owned slice, which its parser keys on the host.
//         MGX_CLI_BAM=host: the host walk and host keys on the reader thread instead (A/B, debugging).
class GzSource : public slicecut::PieceSource {
public:
    static constexpr int kSlots = 4, kDepth = 2;
    enum BamMode { kNotBam, kBamDevice, kBamHost };

    GzSource(FILE* f, std::string head, std::string name, int device, int threads, bool host, BamMode bam = kNotBam);
    ~GzSource() override;
    const std::string& err() const override { return err_; }
    // Stops the source: a next() waiting for a batch to come free returns false (the pipeline failed: the slices that
    // hold the batches may never be parsed).
    void abort() override;
    // The next piece of text; false at the end of the input or on an error (err() says which).
    bool next(slicecut::TextChunk* out) override;
    // -b: the BAM header (the text verbatim, the references from the binary list); false: err()
    bool read_bam_header(samtext::Header* hdr);
    // -b, after read_bam_header(): every record in slices of about slice_bytes; false when the source failed (err())
    bool cut_bam(size_t slice_bytes, const slicecut::Push& push, const slicecut::Stopped& stopped);
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
        const char* out_ptr = nullptr;                                   // the inflated bytes of the batch last waited for
        uint64_t n_out = 0, at = 0;
        bool busy = false;
        mgx_bam_batch_t* bb = nullptr;                                   // -b: the index + keys behind this batch's inflate
        std::vector<uint64_t> h_off; std::vector<mgx_bam_key_t> h_keys;  // ... or made on the host
    };
    struct BamIndex { const uint64_t* off = nullptr; const mgx_bam_key_t* keys = nullptr; uint64_t n = 0, next = 0; };
    bool next_piece(slicecut::TextChunk* out);
    bool top_up();                                         // batches read and submitted until kDepth are in flight
    int next_batch();                                      // the next inflated batch's slot; -1: the blocks are used up or err_, -2: aborted
    bool bgzf_ended_well();                                // after next_batch() == -1 without err_
    bool index_batch(Slot& s, uint64_t first, BamIndex* ix);
    bool index_on_host(Slot& s, uint64_t first, BamIndex* ix);
    bool seam_record(const uint8_t* data, uint64_t n_out, uint64_t* first, bool* whole);
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
    BamMode bam_ = kNotBam;
    int32_t n_ref_ = 0;
    int bam_slot_ = -1; uint64_t bam_first_ = 0;           // the batch in which the records start, and where
    uint64_t batch_base_ = 0;                              // offset of the current batch in the uncompressed stream
    std::vector<uint8_t> carry_; uint64_t carry_whole_ = 0, carry_at_ = 0;   // bytes not in a slice yet: whole records, then a cut one
    uint64_t max_records_ = 0;
    uint64_t n_host_batches_ = 0;                          // batches with more records than that: indexed on the host
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
