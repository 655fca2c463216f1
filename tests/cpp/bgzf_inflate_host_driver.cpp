// Host driver for tests/test_bgzf_inflate_host.py: the inflater's shared core (bgzf_inflate_core.h) and the block scanner
// (bgzf_scan.cpp) as plain C++, built with -fsanitize=address,undefined.
//
//   driver inflate FILE   FILE holds cases: u32 block_len, block bytes, u32 want_len (0xFFFFFFFF: none), want bytes.
//                         Every block is decoded into a buffer of exactly its ISIZE (heap, so that ASan sees one byte past
//                         it); a clean decode must give the want bytes (a mutated block carries its original's).
//                         Prints "cases N ok K err E wrong W" and one "status S count" line per error status seen.
//   driver scan FILE      prints "stop S n N" and the offset, ISIZE and CRC of every block found
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/mgx_bgzf.h"
#include "../../fast-genomic-data-processing_amd/csrc/bgzf_inflate_core.h"

using namespace mgx_inflate;

namespace {

struct HostSink {
    uint8_t* out; uint32_t cap;
    void lit(uint32_t b, uint32_t pos) { out[pos] = (uint8_t)b; }
    void match(uint32_t len, uint32_t dist, uint32_t pos) { for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos + i - dist]; }
    void stored(const uint8_t* src, uint32_t len, uint32_t pos) { if (len) memcpy(out + pos, src, len); }
};

uint32_t crc32_of(const uint8_t* p, size_t n) {
    static uint32_t tab[256];
    static bool made = false;
    if (!made) {
        for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1; tab[i] = c; }
        made = true;
    }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// One whole member, the way the kernel checks it.  out: isize bytes.
uint32_t inflate_member(const uint8_t* block, uint32_t n, std::vector<uint8_t>* out) {
    if (n < kHeaderBytes + kTrailerBytes) return kBadBlockSize;
    const uint32_t isize = rd32(block + n - 4);
    if (isize > kMaxIsize) return kBadIsize;
    uint32_t payload = 0, crc = 0;
    uint32_t st = member_bounds(block, n, isize, &payload, &crc);
    if (st != kOk) return st;
    uint8_t* buf = new uint8_t[isize ? isize : 1];
    HostSink sink{buf, isize};
    static Tables t;
    uint32_t got = 0;
    st = inflate_raw(block + kHeaderBytes, payload, isize, t, sink, &got);
    if (st == kOk && got != isize) st = kIsizeMismatch;
    if (st == kOk && crc32_of(buf, isize) != crc) st = kCrcMismatch;
    if (st == kOk) out->assign(buf, buf + isize);
    delete[] buf;
    return st;
}

bool read_all(const char* path, std::vector<uint8_t>* d) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t b[1 << 16];
    size_t g;
    while ((g = fread(b, 1, sizeof b, f)) > 0) d->insert(d->end(), b, b + g);
    fclose(f);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s inflate|scan FILE\n", argv[0]); return 2; }
    std::vector<uint8_t> d;
    if (!read_all(argv[2], &d)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    if (!strcmp(argv[1], "scan")) {
        const uint64_t maxb = d.size() / 26 + 2;
        std::vector<uint64_t> off(maxb + 1);
        std::vector<uint32_t> isz(maxb), crc(maxb);
        uint64_t nb = 0; int stop = -1;
        const int rc = mgx_bgzf_scan_blocks(d.data(), d.size(), maxb, off.data(), isz.data(), crc.data(), &nb, &stop);
        printf("rc %d stop %d n %llu end %llu\n", rc, stop, (unsigned long long)nb, (unsigned long long)off[nb]);
        for (uint64_t i = 0; i < nb; ++i) printf("%llu %u %u\n", (unsigned long long)off[i], isz[i], crc[i]);
        return 0;
    }
    size_t at = 0;
    uint64_t cases = 0, ok = 0, err = 0, wrong = 0;
    std::map<uint32_t, uint64_t> by_status;
    auto u32 = [&](uint32_t* v) { if (at + 4 > d.size()) return false; *v = rd32(d.data() + at); at += 4; return true; };
    while (at < d.size()) {
        uint32_t bl = 0, wl = 0;
        if (!u32(&bl) || at + bl > d.size()) { fprintf(stderr, "bad case file\n"); return 2; }
        // the block in a heap buffer of its own exact size: a read past it is an ASan report
        std::vector<uint8_t> block(d.begin() + (long)at, d.begin() + (long)(at + bl));
        at += bl;
        if (!u32(&wl)) { fprintf(stderr, "bad case file\n"); return 2; }
        const bool has_want = wl != 0xFFFFFFFFu;
        const uint32_t want_len = has_want ? wl : 0;
        if (at + want_len > d.size()) { fprintf(stderr, "bad case file\n"); return 2; }
        const uint8_t* want = d.data() + at;
        at += want_len;
        std::vector<uint8_t> out;
        const uint32_t st = bl ? inflate_member(block.data(), bl, &out) : (uint32_t)kBadBlockSize;
        ++cases;
        if (st == kOk) {
            ++ok;
            // a clean decode must reproduce the want bytes (for a mutated block: the original's)
            const bool same = out.size() == want_len && (want_len == 0 || !memcmp(out.data(), want, want_len));
            if (has_want && !same) { ++wrong; if (wrong <= 5) printf("wrong output for case %llu\n", (unsigned long long)(cases - 1)); }
        } else {
            ++err;
            by_status[st]++;
        }
    }
    printf("cases %llu ok %llu err %llu wrong %llu\n", (unsigned long long)cases, (unsigned long long)ok, (unsigned long long)err, (unsigned long long)wrong);
    for (auto& kv : by_status) printf("status %u %llu %s\n", kv.first, (unsigned long long)kv.second, status_text(kv.first));
    return 0;
}
