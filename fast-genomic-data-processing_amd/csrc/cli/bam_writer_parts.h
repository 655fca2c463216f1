// bam_writer_parts.h -- what the two halves of the BAM writer share: bam_writer.cpp (host only: links with zlib and pthread alone)
// and bam_writer_device.cpp (everything that calls libmgx.so).  Nothing here needs zlib or the device.
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bai_index.h"
#include "bgzf_block_cut.h"

namespace bamout {

struct StageClock {                  // MGX_CLI_TRACE: seconds since the function began, printed at each stage's end
    const char* who; int width;
    const bool on = getenv("MGX_CLI_TRACE") != nullptr;
    const std::chrono::steady_clock::time_point begin = std::chrono::steady_clock::now();
    void stamp(const char* what) const {
        if (on) fprintf(stderr, "  %s %-*s %.3f s\n", who, width, what, std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count());
    }
};

// BAM header (magic, text, reference table) as the bytes of the first BGZF blocks
std::vector<uint8_t> header_bytes(const samtext::Header& hdr);
int open_output(const std::string& path, std::string* err);                      // -1: *err is set
bool pwrite_all(int fd, const uint8_t* p, size_t len, uint64_t at);
// the EOF block at `at`, close; `ok`: every write so far went through.  false: *err is the "short write" message
bool finish_file(int fd, bool ok, uint64_t at, const std::string& path, std::string* err);
bool write_bai(const std::string& path, const std::vector<uint8_t>& bai, std::string* err);

struct Slice {                       // output of one writer thread
    std::vector<uint8_t> bytes;      // compressed
    std::vector<uint64_t> vbeg, vend;   // per record: (compressed offset within slice) << 16 | offset in block
    bool ok = true;
};

// "block_size, record" at dst, 0x400 set in the flag where the record is marked
inline void put_record(uint8_t* dst, const RecordRef& r) {
    const uint32_t bs = r.len;
    memcpy(dst, &bs, 4);
    memcpy(dst + 4, r.blob, r.len);
    if (r.set_dup) { uint16_t f; memcpy(&f, dst + 4 + kFlagOffset, 2); f |= 0x400; memcpy(dst + 4 + kFlagOffset, &f, 2); }
}

// The cutter's positions (block ordinal << 16 | offset) become the slice's; block_at[k] is the compressed offset of block k of the
// slice, one entry more than there are blocks holds the slice's length.
inline void to_compressed_offsets(Slice* s, const std::vector<uint64_t>& block_at) {
    for (size_t i = 0; i < s->vbeg.size(); ++i) {
        s->vbeg[i] = (block_at[s->vbeg[i] >> 16] << 16) | (s->vbeg[i] & 0xffff);
        s->vend[i] = (block_at[s->vend[i] >> 16] << 16) | (s->vend[i] & 0xffff);
    }
}

// One per thread of the slice pool; run() fills *s, and where s->ok comes back false, err says why.
struct SliceCompressor {
    std::string err;
    virtual ~SliceCompressor() = default;
    virtual void run(const RecordRefs& recs, size_t lo, size_t hi, Slice* s) = 0;
};

// The device's part in write_bam(device >= 0), defined in bam_writer_device.cpp.  Weak: a program linked without that file (and
// without libmgx.so) still writes with zlib, and write_bam refuses a device there.
__attribute__((weak)) bool compress_header_on(int device, const std::vector<uint8_t>& head, std::vector<uint8_t>* file, std::string* err);
__attribute__((weak)) std::unique_ptr<SliceCompressor> make_pinned_compressor(int device);

// A slice through a batch compressor (mgx_bgzf.h's batches in production): the records are gathered straight into a batch's
// input buffer, block boundaries are only offsets into it, and two batches alternate (one being filled while the other is being
// compressed).  Backend: input(k) / offsets(k) of batch k = 0, 1; submit(k, n_blocks); wait(k, &bytes, &offsets) with
// offsets[n_blocks] = the bytes' length; cap (bytes of a batch's input), max_blocks; err, set where submit or wait return false.
template <class Backend>
void compress_slice_batched(const RecordRefs& recs, size_t lo, size_t hi, Backend* be, Slice* s) {
    s->vbeg.resize(hi - lo); s->vend.resize(hi - lo);
    std::vector<uint64_t> block_at;
    BlockCutter cut;
    int cur = 0;                               // batch being filled
    uint32_t in_flight[2] = {0, 0};            // blocks submitted and not yet collected
    uint8_t* in = be->input(cur);
    uint64_t* off = be->offsets(cur);
    uint32_t nb = 0;                           // closed blocks of the current batch; the open block is [off[nb], off[nb] + cut.open)
    off[0] = 0;
    auto collect = [&](int k) {
        if (!in_flight[k]) return;
        const uint8_t* o; const uint64_t* oo;
        if (!be->wait(k, &o, &oo)) { s->ok = false; in_flight[k] = 0; return; }
        const uint64_t base = s->bytes.size();
        for (uint32_t i = 0; i < in_flight[k]; ++i) block_at.push_back(base + oo[i]);
        s->bytes.insert(s->bytes.end(), o, o + oo[in_flight[k]]);
        in_flight[k] = 0;
    };
    auto submit = [&]() {                      // sends the closed blocks of the current batch, moves on to the other one
        if (nb == 0) return;
        collect(cur ^ 1);                      // keeps the slice's blocks in order: the older batch first
        if (be->submit(cur, nb)) in_flight[cur] = nb; else s->ok = false;
        // the open block's bytes move to the head of the other batch
        uint8_t* in2 = be->input(cur ^ 1);
        if (cut.open) memcpy(in2, in + off[nb], cut.open);
        cur ^= 1;
        in = in2; off = be->offsets(cur);
        off[0] = 0; nb = 0;
    };
    auto close = [&](uint64_t n) { off[nb + 1] = off[nb] + n; ++nb; };
    for (size_t k = lo; k < hi && s->ok; ++k) {
        const uint64_t need = 4 + (uint64_t)recs[k].len;
        cut.before(need, close);
        // room for the record and for the blocks it may close
        if (off[nb] + cut.open + need > be->cap || nb + need / kBlockIn + 2 > be->max_blocks) {
            if (cut.open > 0 && off[nb] + cut.open + need > be->cap && nb == 0) cut.close_open(close);   // a batch of one short block rather than none
            submit();
            if (cut.open + need > be->cap) { s->ok = false; be->err = "a record larger than the compressor's batch"; break; }
        }
        s->vbeg[k - lo] = cut.voff();
        put_record(in + off[nb] + cut.open, recs[k]);
        cut.after(need, close);
        s->vend[k - lo] = cut.voff();
    }
    cut.close_open(close);
    submit();
    collect(cur);          // (the batch just left is cur ^ 1 after submit's swap; both are collected, older first)
    collect(cur ^ 1);
    block_at.push_back(s->bytes.size());
    if (s->ok) to_compressed_offsets(s, block_at);
}

}  // namespace bamout
