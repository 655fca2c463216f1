// sam_host.cpp -- SAM text input on the host (include/mgx_sam.h): the reference-name table, the line
// framing, the rule set of sam_line_core.h run serially (what the device must equal), and the same completed by the
// command-line tool's full parser (cli/sam_text.cpp, compiled into the library) for the lines the rules decline.
// No device call.
#include "sam_host.h"

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/mgx_sam.h"
#include "bam_record_core.h"
#include "cli/sam_text.h"
#include "mgx_common.h"
#include "sam_line_core.h"

using mgx::set_error;
using namespace mgx_sam;

extern "C" int mgx_sam_table_create(uint32_t n_ref, const uint8_t* names, const uint32_t* name_off, mgx_sam_table_t** out) {
    if (!out || (n_ref && (!name_off || (name_off[n_ref] && !names)))) { set_error("NULL argument"); return -EINVAL; }
    *out = nullptr;
    if (n_ref >= 0x40000000u) { set_error("%u references", n_ref); return -E2BIG; }
    for (uint32_t i = 0; i < n_ref; ++i)
        if (name_off[i + 1] < name_off[i]) { set_error("name_off decreases at reference %u", i); return -EINVAL; }
    mgx_sam_table* t = new (std::nothrow) mgx_sam_table;
    if (!t) { set_error("out of memory"); return -ENOMEM; }
    uint32_t n_slots = 2;
    while (n_slots < 2 * n_ref) n_slots <<= 1;
    const uint32_t n_bytes = n_ref ? name_off[n_ref] - name_off[0] : 0;
    t->blob.assign(4 + (size_t)n_ref + 1 + n_slots + (n_bytes + 3) / 4, 0);
    uint32_t* w = t->blob.data();
    w[0] = n_ref; w[1] = n_slots; w[2] = n_bytes;
    uint32_t* off = w + 4; uint32_t* slot = off + n_ref + 1;
    for (uint32_t i = 0; i <= n_ref; ++i) off[i] = n_ref ? name_off[i] - name_off[0] : 0;
    for (uint32_t i = 0; i < n_slots; ++i) slot[i] = kEmptySlot;
    if (n_bytes) memcpy(slot + n_slots, names + name_off[0], n_bytes);
    const Table v = table_view(w);
    for (uint32_t i = 0; i < n_ref; ++i) {             // in index order: of equal names the first keeps the slot
        const uint8_t* s = v.names + off[i]; const uint32_t len = off[i + 1] - off[i];
        uint32_t h = name_hash(s, len) & (n_slots - 1);
        while (slot[h] != kEmptySlot && !name_is(v, slot[h], s, len)) h = (h + 1) & (n_slots - 1);
        if (slot[h] == kEmptySlot) slot[h] = i;
        t->header.ref_name.emplace_back((const char*)s, len);
        t->header.ref_len.push_back(0);
    }
    *out = t;
    return 0;
}

extern "C" void mgx_sam_table_destroy(mgx_sam_table_t* t) { delete t; }

extern "C" int mgx_sam_lines_host(const uint8_t* text, uint64_t n, uint64_t max_lines, uint64_t* line_off, uint32_t* line_len, uint64_t* n_lines) {
    if (!n_lines || (n && !text) || ((line_off == nullptr) != (line_len == nullptr))) { set_error("NULL argument"); return -EINVAL; }
    uint64_t cnt = 0, p = 0;
    *n_lines = 0;
    while (p < n) {
        const uint8_t* nl = (const uint8_t*)memchr(text + p, '\n', n - p);
        uint64_t len = nl ? (uint64_t)(nl - (text + p)) : n - p;
        const uint64_t at = p;
        p += len + 1;
        if (len && text[at + len - 1] == '\r') --len;
        if (len == 0) continue;
        if (len > 0xFFFFFFFFull) { set_error("a line of %llu bytes", (unsigned long long)len); return -E2BIG; }
        if (line_off) {
            if (cnt >= max_lines) { set_error("more than %llu lines", (unsigned long long)max_lines); return -E2BIG; }
            line_off[cnt] = at; line_len[cnt] = (uint32_t)len;
        }
        ++cnt;
    }
    *n_lines = cnt;
    return 0;
}

namespace {

struct EncodeArgs {
    const mgx_sam_table_t* table; const uint8_t* text; uint64_t n; uint32_t max_line; uint64_t max_lines, out_capacity;
    uint64_t* line_off; uint32_t* line_len; uint64_t* rec_off; mgx_bam_key_t* keys; uint8_t* out;
    uint64_t* n_lines; uint64_t* n_out; uint64_t* n_declined; uint64_t* bad_line;
};

int encode(const EncodeArgs& a, bool complete) {
    if (!a.table || !a.line_off || !a.line_len || !a.rec_off || !a.n_lines || !a.n_out || !a.n_declined || (a.n && !a.text)) { set_error("NULL argument"); return -EINVAL; }
    *a.n_out = 0; *a.n_declined = 0;
    if (const int rc = mgx_sam_lines_host(a.text, a.n, a.max_lines, a.line_off, a.line_len, a.n_lines)) return rc;
    const Table t = table_view(a.table->blob.data());
    const uint32_t max_line = a.max_line ? a.max_line : kMaxLine;
    uint64_t at = 0, declined = 0;
    std::vector<uint32_t> cigar; std::vector<char> qname; std::vector<uint8_t> blob;
    std::string err;
    for (uint64_t i = 0; i < *a.n_lines; ++i) {
        const uint8_t* s = a.text + a.line_off[i];
        const uint32_t len = a.line_len[i];
        Line L;
        a.rec_off[i] = at;
        uint64_t size = 0;
        bool redo = false;
        if (scan_line(s, len, t, max_line, &L)) {
            size = L.size;
            if (a.out) {
                if (at + size > a.out_capacity) { set_error("more than %llu bytes of BAM", (unsigned long long)a.out_capacity); return -E2BIG; }
                Writer w = {a.out + at, 0, L.size, 0, 1};
                if (encode_line(s, len, L, w) != L.size) { set_error("line %llu: the encoder wrote %u bytes, sized %u", (unsigned long long)i, w.pos, L.size); return -EIO; }
            }
        } else if (complete) {
            samtext::Parsed ps;
            cigar.clear(); qname.clear(); blob.clear();
            if (!samtext::parse_record_into((const char*)s, len, a.table->header, &ps, &cigar, nullptr, &qname, &blob, &err)) {
                if (a.bad_line) *a.bad_line = i;
                set_error("%s at: %.*s", err.c_str(), (int)(len < 80 ? len : 80), (const char*)s);
                return -EBADMSG;
            }
            size = 4 + blob.size();
            if (a.out) {
                if (at + size > a.out_capacity) { set_error("more than %llu bytes of BAM", (unsigned long long)a.out_capacity); return -E2BIG; }
                const uint32_t bs = (uint32_t)blob.size();
                memcpy(a.out + at, &bs, 4);
                memcpy(a.out + at + 4, blob.data(), blob.size());
            }
            ++declined;
        } else { redo = true; ++declined; }
        if (a.keys && a.out) {
            mgx_bam_key_t k;
            memset(&k, 0, sizeof k);
            if (!redo) mgx_bam::record_key(a.out + at, nullptr, &k); else k.redo = kRedoDeclined;
            k.same_qname = i && same_qname(s, len, a.text + a.line_off[i - 1], a.line_len[i - 1]) ? 1 : 0;
            a.keys[i] = k;
        }
        at += size;
    }
    a.rec_off[*a.n_lines] = at;
    *a.n_out = at; *a.n_declined = declined;
    return 0;
}

}  // namespace

extern "C" int mgx_sam_encode_rules(const mgx_sam_table_t* table, const uint8_t* text, uint64_t n, uint32_t max_line, uint64_t max_lines,
                                    uint64_t out_capacity, uint64_t* line_off, uint32_t* line_len, uint64_t* rec_off, mgx_bam_key_t* keys,
                                    uint8_t* out, uint64_t* n_lines, uint64_t* n_out, uint64_t* n_declined) {
    return encode({table, text, n, max_line, max_lines, out_capacity, line_off, line_len, rec_off, keys, out, n_lines, n_out, n_declined, nullptr}, false);
}

extern "C" int mgx_sam_encode_host(const mgx_sam_table_t* table, const uint8_t* text, uint64_t n, uint64_t max_lines, uint64_t out_capacity,
                                   uint64_t* line_off, uint32_t* line_len, uint64_t* rec_off, mgx_bam_key_t* keys, uint8_t* out,
                                   uint64_t* n_lines, uint64_t* n_out, uint64_t* n_declined, uint64_t* bad_line) {
    return encode({table, text, n, 0, max_lines, out_capacity, line_off, line_len, rec_off, keys, out, n_lines, n_out, n_declined, bad_line}, true);
}
