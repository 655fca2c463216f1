// bam_writer_driver.cpp -- the host half of the CLI's BAM writer without a device and without libmgx.so, for
// tests/test_bam_writer_host.py (built with -Werror under AddressSanitizer + UBSan, linked with zlib and pthread alone).
//   cut   IN OUT                  the block cutter over IN's records: blocks, then every record's (start, end) as ordinal << 16 | offset
//   batch IN OUT CAP_BLOCKS MAX   compress_slice_batched on a host stand-in for the device batches
//   index IN OUT THREADS          bai_bytes (MGX_CLI_BAI_PARTS read as in the tool)
//   write IN OUT.bam THREADS DEV  write_bam at zlib level 6 (DEV -1; 0 must be refused in this link)
// IN: u32 l_text, text, u32 n_ref, {u32 l_name, name, u64 length}, u32 n, {u32 len, i32 tid, beg, end, u8 set_dup, mapped, u64 vbeg, vend, bytes}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "bam_writer_parts.h"

using namespace bamout;

namespace {

struct Input {
    std::vector<uint8_t> raw;
    samtext::Header hdr;
    RecordRefs recs;
    std::vector<uint64_t> vbeg, vend;
};

template <class T> T take(const std::vector<uint8_t>& raw, size_t* p) {
    T v;
    if (*p + sizeof v > raw.size()) { printf("input cut short\n"); exit(2); }
    memcpy(&v, raw.data() + *p, sizeof v); *p += sizeof v;
    return v;
}

void load(const char* path, Input* in) {
    std::ifstream f(path, std::ios::binary);
    in->raw.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    size_t p = 0;
    const uint32_t l_text = take<uint32_t>(in->raw, &p);
    in->hdr.text.assign((const char*)in->raw.data() + p, l_text); p += l_text;
    const uint32_t n_ref = take<uint32_t>(in->raw, &p);
    for (uint32_t i = 0; i < n_ref; ++i) {
        const uint32_t l = take<uint32_t>(in->raw, &p);
        in->hdr.ref_name.emplace_back((const char*)in->raw.data() + p, l); p += l;
        in->hdr.ref_len.push_back(take<uint64_t>(in->raw, &p));
    }
    const uint32_t n = take<uint32_t>(in->raw, &p);
    for (uint32_t i = 0; i < n; ++i) {
        RecordRef r;
        r.len = take<uint32_t>(in->raw, &p);
        r.tid = take<int32_t>(in->raw, &p); r.beg = take<int32_t>(in->raw, &p); r.end = take<int32_t>(in->raw, &p);
        r.set_dup = take<uint8_t>(in->raw, &p) != 0; r.mapped = take<uint8_t>(in->raw, &p) != 0;
        in->vbeg.push_back(take<uint64_t>(in->raw, &p)); in->vend.push_back(take<uint64_t>(in->raw, &p));
        if (p + r.len > in->raw.size()) { printf("input cut short\n"); exit(2); }
        r.blob = in->raw.data() + p; p += r.len;
        in->recs.push_back(r);
    }
}

struct Out {
    std::vector<uint8_t> b;
    template <class T> void add(T v) { put<T>(b, v); }
    void bytes(const uint8_t* p, size_t n) { add<uint64_t>(n); b.insert(b.end(), p, p + n); }
    void save(const char* path) const { std::ofstream f(path, std::ios::binary); f.write((const char*)b.data(), (std::streamsize)b.size()); }
};

// The device batches' stand-in: a block is "compressed" to its length as 2 bytes and a copy of its bytes.  Like the device it reads a
// batch's input after submit() returned -- as late as wait() here, so that a host that wrote into a batch in flight is found out.
struct HostBatches {
    uint64_t cap; uint32_t max_blocks;
    std::string err;
    std::vector<uint8_t> in[2], out[2];
    std::vector<uint64_t> off[2], out_off[2];
    uint32_t flying[2] = {0, 0}, submits = 0, carried = 0;     // carried: submits whose open block went on at the head of the other batch
    std::vector<uint8_t> behind;               // what lay behind the closed blocks of the batch submitted last (at most a block of it)
    std::string events;                        // "s0w0s1...": submit / wait and the batch, in the order they were called
    HostBatches(uint64_t cap_, uint32_t max_) : cap(cap_), max_blocks(max_) {
        for (int k = 0; k < 2; ++k) { in[k].resize(cap); off[k].resize(max_blocks + 1); }
    }
    uint8_t* input(int k) { return in[k].data(); }
    uint64_t* offsets(int k) { return off[k].data(); }
    bool submit(int k, uint32_t n_blocks) {
        if (flying[k] || n_blocks == 0 || n_blocks > max_blocks) { err = "stand-in: bad submit"; return false; }
        // the open block was carried over if this batch begins with the bytes that lay behind the last one's closed blocks
        if (submits && behind.size() >= 8 && off[k][1] >= 8 && memcmp(behind.data(), in[k].data(), 8) == 0) ++carried;
        const uint64_t end = off[k][n_blocks];
        behind.assign(in[k].begin() + (std::ptrdiff_t)std::min(cap, end), in[k].begin() + (std::ptrdiff_t)std::min(cap, end + kBlockIn));
        flying[k] = n_blocks; ++submits; events += k ? "s1" : "s0";
        return true;
    }
    bool wait(int k, const uint8_t** o, const uint64_t** oo) {
        if (!flying[k]) { err = "stand-in: wait for a batch that is not in flight"; return false; }
        out[k].clear(); out_off[k].assign(1, 0);
        for (uint32_t i = 0; i < flying[k]; ++i) {
            const uint64_t b = off[k][i], e = off[k][i + 1];
            if (e < b || e - b > kBlockIn || e > cap) { err = "stand-in: bad block offsets"; return false; }
            put<uint16_t>(out[k], (uint16_t)(e - b));
            out[k].insert(out[k].end(), in[k].begin() + (std::ptrdiff_t)b, in[k].begin() + (std::ptrdiff_t)e);
            out_off[k].push_back(out[k].size());
        }
        flying[k] = 0; events += k ? "w1" : "w0";
        *o = out[k].data(); *oo = out_off[k].data();
        return true;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) { printf("usage: see the head of bam_writer_driver.cpp\n"); return 2; }
    const std::string mode = argv[1];
    Input in;
    load(argv[2], &in);
    const size_t n = in.recs.size();
    Out out;
    if (mode == "cut") {
        std::vector<uint8_t> stream;
        for (const RecordRef& r : in.recs) { stream.resize(stream.size() + 4 + r.len); put_record(stream.data() + stream.size() - 4 - r.len, r); }
        BlockCutter cut;
        size_t at = 0;
        std::vector<uint64_t> sizes, v;
        auto close = [&](uint64_t k) { sizes.push_back(k); at += k; };
        for (const RecordRef& r : in.recs) {
            cut.before(4 + (uint64_t)r.len, close); v.push_back(cut.voff());
            cut.after(4 + (uint64_t)r.len, close); v.push_back(cut.voff());
        }
        cut.close_open(close);
        if (at != stream.size()) { printf("the blocks hold %zu bytes of %zu\n", at, stream.size()); return 1; }
        out.add<uint32_t>((uint32_t)sizes.size());
        at = 0;
        for (uint64_t k : sizes) { out.bytes(stream.data() + at, k); at += k; }
        for (uint64_t x : v) out.add<uint64_t>(x);
    } else if (mode == "batch" && argc == 6) {
        HostBatches be((uint64_t)atoi(argv[4]) * kBlockIn, (uint32_t)atoi(argv[5]));
        Slice s;
        compress_slice_batched(in.recs, 0, n, &be, &s);
        out.add<uint8_t>(s.ok); out.add<uint32_t>(be.submits); out.add<uint32_t>(be.carried);
        out.bytes((const uint8_t*)be.events.data(), be.events.size());
        out.bytes((const uint8_t*)be.err.data(), be.err.size());
        out.bytes(s.bytes.data(), s.bytes.size());
        if (s.ok) for (size_t k = 0; k < n; ++k) { out.add<uint64_t>(s.vbeg[k]); out.add<uint64_t>(s.vend[k]); }
    } else if (mode == "index" && argc == 5) {
        auto voff = [&](size_t k, uint64_t* vb, uint64_t* ve) { *vb = in.vbeg[k]; *ve = in.vend[k]; };
        out.b = bai_bytes(in.hdr.ref_name.size(), in.recs, voff, atoi(argv[4]));
    } else if (mode == "write" && argc == 6) {
        std::string err;
        const bool ok = write_bam(argv[3], in.hdr, in.recs, atoi(argv[4]), 6, atoi(argv[5]), &err);
        printf("write_bam %s: %s\n", ok ? "ok" : "failed", err.c_str());
        return 0;
    } else {
        printf("unknown mode\n");
        return 2;
    }
    out.save(argv[3]);
    printf("done\n");
    return 0;
}
