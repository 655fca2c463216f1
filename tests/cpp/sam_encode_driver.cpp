// tests/cpp/sam_encode_driver.cpp -- test driver (not product code) for SAM text input on the host (include/mgx_sam.h).
//
// As a shared library (SAM_DRIVER_MAIN undefined; built with cli/sam_text.cpp only) it gives tests/test_sam_encode_host.py
// the definition of the result: samtext::parse_record_into on every line of a text, framed here with memchr.
//
// As a program (-DSAM_DRIVER_MAIN; built with sam_host.cpp, mgx_common.cpp, cli/sam_text.cpp under AddressSanitizer + UBSan)
// it runs the host functions over the cases of a file -- and, with "trunc", over every prefix of every case -- and holds
// mgx_sam_encode_host and the accepted lines of mgx_sam_encode_rules to that definition.
//
// Case file: u32 n_ref, n_ref x (u32 len, bytes), then until the end (u32 len, bytes) per case.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sam_text.h"

namespace {

struct RefLines {
    std::vector<uint64_t> rec_off;         // n_lines + 1
    std::vector<uint8_t> ok, bytes;
    std::vector<std::string> err;
};

void reference(const char* text, uint64_t n, const samtext::Header& h, RefLines* r) {
    std::vector<uint32_t> cigar; std::vector<char> qname; std::vector<uint8_t> blob;
    r->rec_off.assign(1, 0); r->ok.clear(); r->bytes.clear(); r->err.clear();
    uint64_t p = 0;
    while (p < n) {
        const char* nl = (const char*)memchr(text + p, '\n', (size_t)(n - p));
        size_t len = nl ? (size_t)(nl - (text + p)) : (size_t)(n - p);
        const char* line = text + p;
        p += len + 1;
        if (len && line[len - 1] == '\r') --len;
        if (len == 0) continue;
        samtext::Parsed ps;
        std::string e;
        cigar.clear(); qname.clear(); blob.clear();
        const bool ok = samtext::parse_record_into(line, len, h, &ps, &cigar, nullptr, &qname, &blob, &e);
        if (ok) {
            const uint32_t bs = (uint32_t)blob.size();
            const uint8_t* b = (const uint8_t*)&bs;
            r->bytes.insert(r->bytes.end(), b, b + 4);
            r->bytes.insert(r->bytes.end(), blob.begin(), blob.end());
        }
        r->ok.push_back(ok ? 1 : 0); r->err.push_back(e);
        r->rec_off.push_back(r->bytes.size());
    }
}

samtext::Header header_of(uint32_t n_ref, const uint8_t* names, const uint32_t* name_off) {
    samtext::Header h;
    for (uint32_t i = 0; i < n_ref; ++i) { h.ref_name.emplace_back((const char*)names + name_off[i], name_off[i + 1] - name_off[i]); h.ref_len.push_back(0); }
    return h;
}

}  // namespace

// -> 0; rec_off has max_lines + 1 entries, ok max_lines; -1: more lines or bytes than there is room for
extern "C" int sam_reference_lines(const char* text, uint64_t n, uint32_t n_ref, const uint8_t* names, const uint32_t* name_off, uint64_t max_lines,
                                   uint64_t out_cap, uint64_t* rec_off, uint8_t* ok, uint8_t* out, uint64_t* n_lines) {
    RefLines r;
    reference(text, n, header_of(n_ref, names, name_off), &r);
    if (r.ok.size() > max_lines || r.bytes.size() > out_cap) return -1;
    *n_lines = r.ok.size();
    memcpy(rec_off, r.rec_off.data(), r.rec_off.size() * 8);
    if (!r.ok.empty()) memcpy(ok, r.ok.data(), r.ok.size());
    if (!r.bytes.empty()) memcpy(out, r.bytes.data(), r.bytes.size());
    return 0;
}

#ifdef SAM_DRIVER_MAIN
#include <cerrno>

#include "mgx_sam.h"

extern "C" const char* mgx_last_error(void);

namespace {

struct Totals { uint64_t cases = 0, lines = 0, declined = 0, rejected = 0, mismatches = 0; };

bool read_u32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

void run_case(const mgx_sam_table_t* table, const samtext::Header& h, const std::vector<uint8_t>& text_in, uint64_t n, Totals* t) {
    // a heap copy of exactly n bytes: a read past the text is a sanitizer report
    std::vector<uint8_t> text(text_in.begin(), text_in.begin() + n);
    const uint8_t* tp = text.data();
    RefLines ref;
    reference((const char*)tp, n, h, &ref);
    const uint64_t max_lines = n / 2 + 1, cap = MGX_SAM_OUT_BOUND(max_lines, n);
    std::vector<uint64_t> line_off(max_lines), rec_off(max_lines + 1);
    std::vector<uint32_t> line_len(max_lines);
    std::vector<mgx_bam_key_t> keys(max_lines);
    std::vector<uint8_t> out(cap + 1);
    uint64_t n_lines = 0, n_out = 0, n_dec = 0, bad = 0;
    ++t->cases;
    if (mgx_sam_lines_host(tp, n, max_lines, line_off.data(), line_len.data(), &n_lines) || n_lines != ref.ok.size()) { ++t->mismatches; return; }
    for (uint32_t max_line : {0u, 1u << 20}) {
        int rc = mgx_sam_encode_rules(table, tp, n, max_line, max_lines, cap, line_off.data(), line_len.data(), rec_off.data(), keys.data(), out.data(),
                                      &n_lines, &n_out, &n_dec);
        if (rc || n_lines != ref.ok.size()) { ++t->mismatches; return; }
        for (uint64_t i = 0; i < n_lines; ++i) {
            const uint64_t sz = rec_off[i + 1] - rec_off[i], want = ref.rec_off[i + 1] - ref.rec_off[i];
            if (sz == 0) { if (!(keys[i].redo & MGX_SAM_REDO_DECLINED)) ++t->mismatches; continue; }
            if (!ref.ok[i] || sz != want || memcmp(out.data() + rec_off[i], ref.bytes.data() + ref.rec_off[i], sz) != 0 || sz > MGX_SAM_OUT_BOUND(1, line_len[i]))
                ++t->mismatches;
        }
        if (max_line == 0) { t->lines += n_lines; t->declined += n_dec; }
    }
    const int rc = mgx_sam_encode_host(table, tp, n, max_lines, cap, line_off.data(), line_len.data(), rec_off.data(), keys.data(), out.data(), &n_lines,
                                       &n_out, &n_dec, &bad);
    uint64_t first_bad = ref.ok.size();
    for (uint64_t i = 0; i < ref.ok.size(); ++i) if (!ref.ok[i]) { first_bad = i; break; }
    if (first_bad < ref.ok.size()) {
        ++t->rejected;
        if (rc != -EBADMSG || bad != first_bad || !strstr(mgx_last_error(), ref.err[first_bad].c_str())) ++t->mismatches;
    } else if (rc || n_out != ref.bytes.size() || (n_out && memcmp(out.data(), ref.bytes.data(), n_out) != 0)) ++t->mismatches;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[1], "cases") && strcmp(argv[1], "trunc"))) { fprintf(stderr, "usage: %s cases|trunc FILE\n", argv[0]); return 2; }
    const bool trunc = strcmp(argv[1], "trunc") == 0;
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    uint32_t n_ref = 0;
    if (!read_u32(f, &n_ref)) return 2;
    std::vector<uint8_t> names; std::vector<uint32_t> name_off(1, 0);
    for (uint32_t i = 0; i < n_ref; ++i) {
        uint32_t len;
        if (!read_u32(f, &len)) return 2;
        names.resize(names.size() + len);
        if (len && fread(names.data() + names.size() - len, 1, len, f) != len) return 2;
        name_off.push_back((uint32_t)names.size());
    }
    names.push_back(0);
    mgx_sam_table_t* table = nullptr;
    if (mgx_sam_table_create(n_ref, names.data(), name_off.data(), &table)) { fprintf(stderr, "%s\n", mgx_last_error()); return 2; }
    const samtext::Header h = header_of(n_ref, names.data(), name_off.data());
    Totals t;
    uint32_t len;
    while (read_u32(f, &len)) {
        std::vector<uint8_t> text(len);
        if (len && fread(text.data(), 1, len, f) != len) return 2;
        if (trunc) for (uint64_t n = 0; n <= len; ++n) run_case(table, h, text, n, &t);
        else run_case(table, h, text, len, &t);
    }
    fclose(f);
    mgx_sam_table_destroy(table);
    printf("cases %llu lines %llu declined %llu rejected %llu mismatches %llu\n", (unsigned long long)t.cases, (unsigned long long)t.lines,
           (unsigned long long)t.declined, (unsigned long long)t.rejected, (unsigned long long)t.mismatches);
    return t.mismatches ? 1 : 0;
}
#endif
