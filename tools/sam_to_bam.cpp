// sam_to_bam.cpp -- SAM text -> the uncompressed bytes of a BAM file (header + records), the records in the order of the
// text: the input of tools/dev_bam_cli.py, which compresses them into BGZF blocks on the device.  Uses the CLI's own
// SAM parser (csrc/cli/sam_text.cpp), so the records are byte for byte what `sortmardup` makes of the same text.
//     g++ -O2 -std=c++17 -pthread -I fast-genomic-data-processing_amd/csrc/cli tools/sam_to_bam.cpp fast-genomic-data-processing_amd/csrc/cli/sam_text.cpp -o sam_to_bam
//     sam_to_bam in.sam out.bam.raw [threads]
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "sam_text.h"

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s in.sam out.bam.raw [threads]\n", argv[0]); return 2; }
    const int T = argc > 3 ? std::max(1, atoi(argv[3])) : 8;
    const int fd = open(argv[1], O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) { perror(argv[1]); return 1; }
    const size_t size = (size_t)sb.st_size;
    const char* data = (const char*)mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0);
    if (data == MAP_FAILED) { perror("mmap"); return 1; }
    samtext::Header hdr;
    const size_t body = samtext::parse_header(data, size, &hdr);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 1; }
    auto put32 = [&](int32_t v) { fwrite(&v, 4, 1, out); };
    fwrite("BAM\1", 1, 4, out);
    put32((int32_t)hdr.text.size()); fwrite(hdr.text.data(), 1, hdr.text.size(), out);
    put32((int32_t)hdr.ref_name.size());
    for (size_t i = 0; i < hdr.ref_name.size(); ++i) {
        put32((int32_t)hdr.ref_name[i].size() + 1); fwrite(hdr.ref_name[i].c_str(), 1, hdr.ref_name[i].size() + 1, out); put32((int32_t)hdr.ref_len[i]);
    }
    // ranges of whole lines, one per thread at a time; the pieces are written in order
    std::vector<size_t> cut(T + 1, size);
    cut[0] = body;
    for (int t = 1; t < T; ++t) {
        size_t p = body + (size - body) / T * t;
        const char* nl = (const char*)memchr(data + p, '\n', size - p);
        cut[t] = nl ? (size_t)(nl - data) + 1 : size;
    }
    std::vector<std::vector<uint8_t>> piece(T);
    std::vector<std::string> errs(T);
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back([&, t]() {
        std::vector<uint32_t> cigar; std::vector<char> qname; std::vector<uint8_t> blob;
        std::vector<uint8_t>& o = piece[t];
        o.reserve((cut[t + 1] - cut[t]) * 7 / 10);
        for (size_t off = cut[t]; off < cut[t + 1];) {
            const char* nl = (const char*)memchr(data + off, '\n', cut[t + 1] - off);
            size_t len = nl ? (size_t)(nl - (data + off)) : cut[t + 1] - off;
            const size_t next = off + len + 1;
            if (len && data[off + len - 1] == '\r') --len;
            if (len) {
                samtext::Parsed pr;
                cigar.clear(); qname.clear(); blob.clear();
                if (!samtext::parse_record_into(data + off, len, hdr, &pr, &cigar, nullptr, &qname, &blob, &errs[t])) return;
                const int32_t bs = (int32_t)blob.size();
                const uint8_t* b = (const uint8_t*)&bs;
                o.insert(o.end(), b, b + 4); o.insert(o.end(), blob.begin(), blob.end());
            }
            off = next;
        }
    });
    for (auto& th : pool) th.join();
    for (int t = 0; t < T; ++t) {
        if (!errs[t].empty()) { fprintf(stderr, "SAM parse error: %s\n", errs[t].c_str()); return 1; }
        if (!piece[t].empty() && fwrite(piece[t].data(), 1, piece[t].size(), out) != piece[t].size()) { perror("write"); return 1; }
    }
    return fclose(out) ? 1 : 0;
}
