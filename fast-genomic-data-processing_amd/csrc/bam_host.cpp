// bam_host.cpp -- BAM input on the host (include/mgx_bam.h): the header, the serial chain walk that
// defines what the device index must equal, and the keys, with the two cases the shared rules (bam_record_core.h)
// decline: tokens that need strtol, and the long-CIGAR placeholder.  No device call.
#include <cerrno>
#include <cstdint>
#include <cstring>

#include "../../include/mgx_bam.h"
#include "bam_record_core.h"
#include "mgx_common.h"
#include "sortdedup_pack.h"

using mgx::set_error;
using namespace mgx_bam;

extern "C" int mgx_bam_parse_header(const uint8_t* data, uint64_t n, mgx_bam_header_t* hdr, uint32_t max_ref, uint64_t* name_off,
                                    uint32_t* name_len, uint32_t* ref_len) {
    if (!hdr || (n && !data) || (max_ref && (!name_off || !name_len || !ref_len))) { set_error("NULL argument"); return -EINVAL; }
    static const uint8_t magic[4] = {'B', 'A', 'M', 1};
    for (uint64_t i = 0; i < 4 && i < n; ++i)
        if (data[i] != magic[i]) { set_error("not BAM: the inflated bytes do not start with the BAM magic"); return -EILSEQ; }
    if (n < 8) return MGX_BAM_PARTIAL;
    const int32_t l_text = rd32s(data + 4);
    if (l_text < 0) { set_error("BAM header: l_text is %d", l_text); return -EILSEQ; }
    uint64_t p = 8 + (uint64_t)l_text;
    if (p + 4 > n) return MGX_BAM_PARTIAL;
    const int32_t n_ref = rd32s(data + p);
    if (n_ref < 0) { set_error("BAM header: n_ref is %d", n_ref); return -EILSEQ; }
    p += 4;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (p + 4 > n) return MGX_BAM_PARTIAL;
        const int32_t l_name = rd32s(data + p);
        if (l_name < 1) { set_error("BAM header: reference %d has l_name %d", r, l_name); return -EILSEQ; }
        if (p + 4 + (uint64_t)l_name + 4 > n) return MGX_BAM_PARTIAL;
        if (data[p + 4 + (uint64_t)l_name - 1] != 0) { set_error("BAM header: the name of reference %d does not end with NUL", r); return -EILSEQ; }
        const int32_t l_ref = rd32s(data + p + 4 + (uint64_t)l_name);
        if (l_ref < 0) { set_error("BAM header: reference %d has length %d", r, l_ref); return -EILSEQ; }
        if ((uint32_t)r < max_ref) { name_off[r] = p + 4; name_len[r] = (uint32_t)l_name - 1; ref_len[r] = (uint32_t)l_ref; }
        p += 4 + (uint64_t)l_name + 4;
    }
    uint64_t tl = (uint64_t)l_text;
    while (tl > 0 && data[8 + tl - 1] == 0) --tl;
    hdr->first = p; hdr->text_off = 8; hdr->text_len = tl; hdr->n_ref = (uint32_t)n_ref; hdr->pad_ = 0;
    return 0;
}

extern "C" int mgx_bam_walk_host(const uint8_t* data, uint64_t n, uint64_t first, uint64_t max_records, uint64_t* rec_off,
                                 uint64_t* n_records, uint64_t* next) {
    if (!n_records || !next || (n && !data)) { set_error("NULL argument"); return -EINVAL; }
    uint64_t o = first, cnt = 0;
    *n_records = 0; *next = first;
    while (o < n && n - o >= 4) {
        const int64_t bs = rd32s(data + o);
        if (bs > 0 && (uint64_t)bs > n - o - 4) break;             // does not count: it ends beyond n
        // a counted record: its block_size is below 32 (then only that is looked at) or all of it lies inside n
        const uint32_t rule = bs < 32 ? (uint32_t)kBlockSize : check_record(data + o);
        if (rule != kValid) {
            *n_records = cnt; *next = o;
            set_error("BAM record at offset %llu: %s", (unsigned long long)o, rule_text(rule));
            return -EBADMSG;
        }
        if (rec_off) {
            if (cnt >= max_records) { set_error("more than %llu BAM records", (unsigned long long)max_records); return -E2BIG; }
            rec_off[cnt] = o;
        }
        ++cnt;
        o += 4 + (uint64_t)bs;
    }
    *n_records = cnt; *next = o;
    return 0;
}

namespace {

// Whether the optional fields aux[0, n) hold a CG tag of type B,I.  Malformed fields end the search.
bool has_cg_tag(const uint8_t* aux, uint64_t n) {
    uint64_t p = 0;
    while (n - p >= 3) {
        const uint8_t t0 = aux[p], t1 = aux[p + 1], ty = aux[p + 2];
        p += 3;
        uint64_t sz;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': {
                uint64_t e = p;
                while (e < n && aux[e] != 0) ++e;
                if (e >= n) return false;
                sz = e + 1 - p;
                break;
            }
            case 'B': {
                if (n - p < 5) return false;
                const uint8_t sub = aux[p];
                if (t0 == 'C' && t1 == 'G' && sub == 'I') return true;
                const uint64_t cnt = rd32(aux + p + 1);
                const uint64_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                if (w == 0) return false;
                sz = 5 + cnt * w;
                break;
            }
            default: return false;
        }
        if (sz > n - p) return false;
        p += sz;
    }
    return false;
}

// what the shared rules declined, for the valid record at p
int redo_key(const uint8_t* p, uint64_t off, mgx_bam_key_t* k) {
    const Fixed f = read_fixed(p);
    if (k->redo & kRedoToken) {
        uint16_t t[3];
        mgx::qname_tile_x_y((const char*)p + kFixed, f.l_read_name - 1, t);
        k->tile = t[0]; k->x = t[1]; k->y = t[2];
    }
    if (k->redo & kRedoLongCigar) {
        const uint64_t fixed = 32ull + f.l_read_name + 4ull * f.n_cigar + ((uint64_t)f.l_seq + 1) / 2 + (uint64_t)f.l_seq;
        if (has_cg_tag(p + 4 + fixed, (uint64_t)f.bs - fixed)) {
            set_error("BAM record at offset %llu: its CIGAR is in a CG tag (more than 65535 operations), which is not read", (unsigned long long)off);
            return -ENOTSUP;
        }
    }
    k->redo = 0;
    return 0;
}

}  // namespace

extern "C" int mgx_bam_keys_redo(const uint8_t* data, const uint64_t* rec_off, uint64_t n_records, mgx_bam_key_t* keys) {
    if (n_records && (!data || !rec_off || !keys)) { set_error("NULL argument"); return -EINVAL; }
    for (uint64_t i = 0; i < n_records; ++i)
        if (keys[i].redo) if (const int rc = redo_key(data + rec_off[i], rec_off[i], &keys[i])) return rc;
    return 0;
}

extern "C" int mgx_bam_keys_rules(const uint8_t* data, const uint64_t* rec_off, uint64_t n_records, mgx_bam_key_t* keys) {
    if (n_records && (!data || !rec_off || !keys)) { set_error("NULL argument"); return -EINVAL; }
    for (uint64_t i = 0; i < n_records; ++i) record_key(data + rec_off[i], i ? data + rec_off[i - 1] : nullptr, &keys[i]);
    return 0;
}

extern "C" int mgx_bam_keys_host(const uint8_t* data, const uint64_t* rec_off, uint64_t n_records, mgx_bam_key_t* keys) {
    if (n_records && (!data || !rec_off || !keys)) { set_error("NULL argument"); return -EINVAL; }
    for (uint64_t i = 0; i < n_records; ++i) {
        record_key(data + rec_off[i], i ? data + rec_off[i - 1] : nullptr, &keys[i]);
        if (keys[i].redo) if (const int rc = redo_key(data + rec_off[i], rec_off[i], &keys[i])) return rc;
    }
    return 0;
}
