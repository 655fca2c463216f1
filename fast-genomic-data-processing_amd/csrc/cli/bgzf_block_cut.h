// bgzf_block_cut.h -- where a slice of BAM records is cut into BGZF blocks (SAMv1 4.1: at most 0xff00 bytes a block here, htslib's
// BGZF_BLOCK_SIZE).  The one statement of the rule: both slice compressors of bam_writer drive it, which is why -z zlib and -z pinned
// hold the same blocks.  No zlib, no device: tests/test_bam_writer_host.py runs it against a restatement.
#pragma once

#include <cstdint>

namespace bamout {

constexpr uint64_t kBlockIn = 0xff00;          // uncompressed bytes per BGZF block

// Sees the records one at a time as need = 4 + len bytes.  close(n) tells the caller that the first n bytes it holds open are a
// finished block.  A position is (ordinal of the block within the slice) << 16 | offset in the block.
struct BlockCutter {
    uint64_t ordinal = 0;                      // blocks closed so far
    uint64_t open = 0;                         // bytes of the open block
    uint64_t voff() const { return (ordinal << 16) | open; }
    template <class Close> void close_open(Close&& close) { if (open) { close(open); ++ordinal; open = 0; } }
    // before the record's bytes are appended: a record that does not fit starts a block.  voff() is then the record's start
    template <class Close> void before(uint64_t need, Close&& close) { if (open > 0 && open + need > kBlockIn) close_open(close); }
    // after they are: a record larger than one block spans several, cut greedily; a full block closes.  voff() is the record's end
    template <class Close> void after(uint64_t need, Close&& close) {
        open += need;
        while (open > kBlockIn) { close(kBlockIn); ++ordinal; open -= kBlockIn; }
        if (open == kBlockIn) close_open(close);
    }
};

}  // namespace bamout
