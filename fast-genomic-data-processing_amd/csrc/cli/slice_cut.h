// slice_cut.h -- the reader's half of the ingest: where the SAM text is cut into slices.
//
// A slice is at most `slice_bytes` of text, ends where a queryname group ends (mates are found inside their slice), and
// the window doubles while one group fills it.  Two cutters implement that rule: over ranges of a regular file, of which
// only a few KB around every tentative cut are read, and over pieces of text that a source hands out in order (inflated
// BGZF / gzip: gz_source.h; a plain stream: StreamSource), cut in place.  No device call and no SAM parsing here: this
// translation unit needs libc and libstdc++ only, and tests/cpp/slice_cut_driver.cpp runs it under the sanitizers.
#pragma once

#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>

namespace slicecut {

struct Slice {                       // owned text, a range of the input file, or text inside a piece's buffer
    uint64_t seq = 0; std::string text; uint64_t file_off = 0; size_t file_len = 0; bool from_file = false;
    const char* ext = nullptr; size_t ext_len = 0; std::shared_ptr<void> hold;      // a piece's text: parsed in place
    // BAM input (gz_source.h): whole alignment records instead of lines.  Owned bytes in `text` (keyed by the parser), or
    // n_rec records inside a batch's buffer, record i at bam_data + rec_off[i] with the device-made key keys[i]
    // (mgx_bam_key_t); bam_at: where the slice's bytes start in the uncompressed stream (for messages).
    bool bam = false; const uint8_t* bam_data = nullptr; const uint64_t* rec_off = nullptr; const void* keys = nullptr; size_t n_rec = 0;
    uint64_t bam_at = 0;
};

// A piece of text; `hold` keeps its buffer alive (the slices cut from it are parsed in place, and the buffer goes back to
// the source, or is freed, when the last of them is done).
struct TextChunk { const char* data = nullptr; size_t size = 0; std::shared_ptr<void> hold; };

// Text in pieces, in order.
struct PieceSource {
    virtual ~PieceSource() = default;
    virtual bool next(TextChunk* out) = 0;           // false at the end of the input or on an error (err() says which)
    virtual const std::string& err() const = 0;
    virtual void abort() = 0;                        // the pipeline failed: a next() that waits for a buffer returns false
};

// Bytes of text per piece where a source chooses the size itself (a plain stream, gzip members inflated by zlib).
constexpr size_t kPieceBytes = 16u << 20;

// A plain stream (stdin, a FIFO): pieces of `piece_bytes` read into buffers of their own, after `head` (what the format
// check consumed).  A read that returns nothing ends the input; it has no error of its own to report.
class StreamSource : public PieceSource {
public:
    StreamSource(FILE* f, std::string head, size_t piece_bytes = kPieceBytes) : f_(f), head_(std::move(head)), piece_(piece_bytes) {}
    bool next(TextChunk* out) override;
    const std::string& err() const override { static const std::string none; return none; }
    void abort() override {}
private:
    FILE* f_; std::string head_; size_t piece_; bool eof_ = false;
};

const char* line_qname_end(const char* line, const char* end);
// Offset at which the LAST queryname group of [data, data + size) starts (size ends on a line boundary).
size_t last_group_start(const char* data, size_t size);

// The '@' lines at the head of a piece source (kept apart; the body is cut from the pieces in place), and the piece in
// which the body starts.
struct PieceHead { std::string text; TextChunk first; size_t first_off = 0; bool have = false; };
bool scan_piece_header(PieceSource& src, PieceHead* head);          // false: the source failed (src.err())

// A cutter hands every slice to `push`, which numbers it (seq) and returns false to stop the cutting.
using Push = std::function<bool(Slice)>;
// True once the pipeline has failed: the piece cutter asks before it takes the next piece.
using Stopped = std::function<bool()>;
// Bytes [at, at + n) of the file into dst; false on a read error.
using ReadAt = std::function<bool(char* dst, size_t n, uint64_t at)>;

// Slices of [pos, size) of a regular file as (file_off, file_len).  False on a read error.
bool cut_file_ranges(const ReadAt& read, uint64_t pos, uint64_t size, size_t slice_bytes, const Push& push);

// Slices of the body of a piece source, after scan_piece_header(): `carry` is body text that is not in a piece (what
// the header parser left of head.text).  A slice inside one piece is cut in place and shares the piece's `hold`; only a
// group that straddles two pieces is copied, into an owned slice.  What is carried is bounded: once it holds half a
// window and another group starts in it, it goes out as a slice.  False when the source failed (src.err()).
bool cut_pieces(PieceSource& src, PieceHead head, std::string carry, size_t slice_bytes, const Push& push, const Stopped& stopped);

}  // namespace slicecut
