// bam_host_driver.cpp -- the host side of BAM input (csrc/bam_host.cpp, mgx_bam_pack_keys of csrc/sortdedup_pack.cpp) as a
// stand-alone program, built by tests/test_bam_sanitize_host.py under AddressSanitizer + UBSan.
//   dump FILE        header, record offsets, keys and packed records of one inflated BAM file, as text
//   cases FILE       FILE = [u32 length][bytes] ...: every case through header, walk, keys and pack; prints how many
//                    gave a result and how many an error
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "mgx_bam.h"

extern "C" const char* mgx_last_error(void);

namespace {

struct Parsed {
    int rc = 0;                         // of the step that stopped the case: 0 all steps ran
    mgx_bam_header_t hdr{};
    std::vector<uint64_t> name_off, target_len, rec_off;
    std::vector<uint32_t> name_len, ref_len, input_index;
    std::vector<mgx_bam_key_t> keys;
    std::vector<mgx_rec_t> recs;
    uint64_t n_records = 0, next = 0, L = 0;
};

Parsed run_case(const uint8_t* d, uint64_t n) {
    Parsed p;
    // exactly n readable bytes: a copy, so that the sanitizer sees every read past the end
    std::vector<uint8_t> copy(d, d + n);
    d = copy.data();
    p.rc = mgx_bam_parse_header(d, n, &p.hdr, 0, nullptr, nullptr, nullptr);
    if (p.rc) return p;
    const uint32_t nr = p.hdr.n_ref;
    p.name_off.resize(nr); p.name_len.resize(nr); p.ref_len.resize(nr);
    p.rc = mgx_bam_parse_header(d, n, &p.hdr, nr, p.name_off.data(), p.name_len.data(), p.ref_len.data());
    if (p.rc) return p;
    for (uint32_t r : p.ref_len) p.target_len.push_back(r);
    p.rc = mgx_bam_walk_host(d, n, p.hdr.first, 0, nullptr, &p.n_records, &p.next);
    if (p.rc) return p;
    p.rec_off.resize(p.n_records);
    uint64_t again = 0, next2 = 0;
    p.rc = mgx_bam_walk_host(d, n, p.hdr.first, p.n_records, p.rec_off.data(), &again, &next2);
    if (p.rc) return p;
    if (again != p.n_records || next2 != p.next) { p.rc = -1000; return p; }
    p.keys.resize(p.n_records);
    p.rc = mgx_bam_keys_host(d, p.rec_off.data(), p.n_records, p.keys.data());
    if (p.rc) return p;
    p.recs.resize(p.n_records); p.input_index.resize(p.n_records);
    p.rc = mgx_bam_pack_keys(p.n_records, p.keys.data(), nr, p.target_len.data(), p.recs.data(), p.input_index.data(), &p.L);
    return p;
}

std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s dump|cases FILE\n", argv[0]); return 2; }
    const std::vector<uint8_t> file = slurp(argv[2]);
    if (!strcmp(argv[1], "dump")) {
        const Parsed p = run_case(file.data(), file.size());
        if (p.rc) { printf("rc %d %s\n", p.rc, mgx_last_error()); return 0; }
        printf("rc 0 first %llu text_len %llu n_ref %u n_records %llu next %llu L %llu\n", (unsigned long long)p.hdr.first, (unsigned long long)p.hdr.text_len,
               p.hdr.n_ref, (unsigned long long)p.n_records, (unsigned long long)p.next, (unsigned long long)p.L);
        for (uint32_t r = 0; r < p.hdr.n_ref; ++r) printf("ref %.*s %u\n", (int)p.name_len[r], (const char*)file.data() + p.name_off[r], p.ref_len[r]);
        for (uint64_t i = 0; i < p.n_records; ++i) {
            const mgx_bam_key_t& k = p.keys[i];
            const mgx_rec_t& r = p.recs[i];
            printf("rec %llu %lld %d %d %d %u %u %u %u %u %u %u | %llu %llu %u %u %u %u %u %u %u\n", (unsigned long long)p.rec_off[i], (long long)k.d5, k.tid, k.pos,
                   k.end, k.flag, k.score, k.tile, k.x, k.y, k.same_qname, k.redo, (unsigned long long)r.coord, (unsigned long long)r.prime5, r.mate, r.flag,
                   r.score, r.tile, r.x, r.y, p.input_index[i]);
        }
        return 0;
    }
    if (!strcmp(argv[1], "cases")) {
        uint64_t at = 0, n_cases = 0, n_ok = 0, n_err = 0, n_partial = 0, n_records = 0;
        while (at + 4 <= file.size()) {
            uint32_t len;
            memcpy(&len, &file[at], 4);
            at += 4;
            if (len > file.size() - at) { fprintf(stderr, "bad case file\n"); return 2; }
            const Parsed p = run_case(file.data() + at, len);
            at += len;
            ++n_cases;
            if (p.rc == 0) { ++n_ok; n_records += p.n_records; }
            else if (p.rc == MGX_BAM_PARTIAL) ++n_partial;
            else if (p.rc < 0 && p.rc > -1000 && mgx_last_error()[0]) ++n_err;
            else { fprintf(stderr, "case %llu: rc %d without a message\n", (unsigned long long)n_cases, p.rc); return 1; }
        }
        printf("cases %llu ok %llu err %llu partial %llu records %llu\n", (unsigned long long)n_cases, (unsigned long long)n_ok, (unsigned long long)n_err,
               (unsigned long long)n_partial, (unsigned long long)n_records);
        return 0;
    }
    return 2;
}
