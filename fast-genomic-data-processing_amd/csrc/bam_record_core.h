// bam_record_core.h -- the rules of a BAM alignment record (SAMv1 4.2) that BAM input needs, one text for
// the host implementation (bam_host.cpp, which the CPU tests run under AddressSanitizer + UBSan) and for the device
// kernels (mgx_bam.hip, mgx_sam.hip): when a record is valid, and what sorting and duplicate marking need from it (mgx_bam_key_t).
//
// Plain C++, no library call.  Records sit at any byte offset: every multi-byte field is assembled from bytes.
// The key rules restate base_quality_score / unclipped_five_prime / tile_x_y / token_to_u16 of sortdedup_pack.cpp, which
// stays their specification; what those do through strtol (a token that is not 1-18 plain digits) is declined here with
// a `redo` bit and left to the host.
#ifndef MGX_BAM_RECORD_CORE_H
#define MGX_BAM_RECORD_CORE_H

#include <stdint.h>

#include "../../include/mgx_bam.h"

#ifndef MGX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MGX_HD __host__ __device__
#else
#define MGX_HD
#endif
#endif

namespace mgx_bam {

enum Rule : uint32_t {
    kValid = 0,
    kBlockSize,       // block_size outside [32, MGX_BAM_MAX_RECORD]
    kNameLength,      // l_read_name is 0
    kSeqLength,       // l_seq is negative
    kParts,           // fixed part + name + CIGAR + bases + qualities exceed block_size
    kNameNul,         // the read name does not end with NUL
    kNumRules
};

inline const char* rule_text(uint32_t r) {
    static const char* const names[kNumRules] = {
        "valid", "block_size is not between 32 and 2^28", "l_read_name is 0", "l_seq is negative",
        "name, CIGAR, bases and qualities are longer than block_size", "the read name does not end with NUL"};
    return r < kNumRules ? names[r] : "unknown rule";
}

constexpr uint32_t kFixed = 36;            // block_size and the 32 fixed bytes: what a validity check reads before the name
constexpr uint32_t kMinRecord = 37;        // ... plus a name of one NUL: the shortest chain link (4 + block_size)
constexpr uint32_t kMaxNameEnd = kFixed + 255;   // the name's NUL lies below this offset

MGX_HD inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
MGX_HD inline uint32_t rd32(const uint8_t* p) { return rd16(p) | rd16(p + 2) << 16; }
MGX_HD inline int32_t rd32s(const uint8_t* p) { return (int32_t)rd32(p); }

// The fixed part of the record at p (kFixed readable bytes).
struct Fixed {
    int32_t bs, tid, pos, l_seq, next_tid, next_pos;
    uint32_t l_read_name, n_cigar, flag;
};

MGX_HD inline Fixed read_fixed(const uint8_t* p) {
    Fixed f;
    f.bs = rd32s(p); f.tid = rd32s(p + 4); f.pos = rd32s(p + 8);
    f.l_read_name = p[12]; f.n_cigar = rd16(p + 16); f.flag = rd16(p + 18);
    f.l_seq = rd32s(p + 20); f.next_tid = rd32s(p + 24); f.next_pos = rd32s(p + 28);
    return f;
}

// the rules that need the fixed part only
MGX_HD inline uint32_t check_fixed(const Fixed& f) {
    if (f.bs < 32 || f.bs > (int32_t)MGX_BAM_MAX_RECORD) return kBlockSize;
    if (f.l_read_name < 1) return kNameLength;
    if (f.l_seq < 0) return kSeqLength;
    const uint64_t parts = 32ull + f.l_read_name + 4ull * f.n_cigar + ((uint64_t)f.l_seq + 1) / 2 + (uint64_t)f.l_seq;
    if (parts > (uint64_t)f.bs) return kParts;
    return kValid;
}

// All rules, for a record whose 4 + block_size bytes are readable at p (what the walk establishes before it asks), or,
// with block_size out of range, whose kFixed bytes are.
MGX_HD inline uint32_t check_record(const uint8_t* p) {
    const Fixed f = read_fixed(p);
    const uint32_t r = check_fixed(f);
    if (r != kValid) return r;
    return p[kFixed + f.l_read_name - 1] == 0 ? kValid : kNameNul;
}

// What the index kernel asks of a guessed record start beyond validity: reference ids and positions a BAM file can hold.
MGX_HD inline bool plausible(const Fixed& f, int32_t n_ref) {
    return f.tid >= -1 && f.tid < n_ref && f.next_tid >= -1 && f.next_tid < n_ref && f.pos >= -1 && f.next_pos >= -1;
}

// ---- keys ------------------------------------------------------------------------------------------------------------
constexpr uint8_t kRedoToken = 1;          // a tile / x / y token is not 1-18 plain digits
constexpr uint8_t kRedoLongCigar = 2;      // the CIGAR has the shape of htslib's long-CIGAR placeholder: <l_seq>S <n>N

MGX_HD inline bool consumes_reference(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
MGX_HD inline bool is_clip(uint32_t op) { return op == 4 || op == 5; }

// score of q[lo, hi): callers add the pieces of a record in a uint16_t, which wraps like the reference's accumulator
MGX_HD inline uint16_t score_bytes(const uint8_t* q, uint32_t lo, uint32_t hi) {
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += q[i] >= 15 ? q[i] : 0u;
    return (uint16_t)s;
}

// d5 = unclipped_five_prime(coord, ...) - coord, the reference length, and the placeholder shape
MGX_HD inline void cigar_keys(const uint8_t* cig, uint32_t n_cigar, bool forward, int32_t l_seq, int64_t* d5, int64_t* ref_len, uint8_t* redo) {
    uint64_t ref = 0;
    for (uint32_t i = 0; i < n_cigar; ++i) { const uint32_t c = rd32(cig + 4 * i); if (consumes_reference(c & 15u)) ref += c >> 4; }
    *ref_len = (int64_t)ref;
    uint64_t d = 0;
    if (n_cigar != 0) {
        if (forward) {
            for (uint32_t i = 0; i < n_cigar; ++i) { const uint32_t c = rd32(cig + 4 * i); if (!is_clip(c & 15u)) break; d -= c >> 4; }
        } else {
            uint32_t i = n_cigar;
            while (i > 0) { const uint32_t c = rd32(cig + 4 * (i - 1)); if (!is_clip(c & 15u)) break; d += c >> 4; --i; }
            d += ref;                      // clips consume no reference: the operations left are all that do
            d -= 1;
        }
    }
    *d5 = (int64_t)d;
    if (n_cigar == 2) {
        const uint32_t c0 = rd32(cig), c1 = rd32(cig + 4);
        if ((c0 & 15u) == 4 && (c0 >> 4) == (uint32_t)l_seq && (c1 & 15u) == 3) *redo |= kRedoLongCigar;
    }
}

// token_to_u16 without its strtol branch: false when that branch would run
MGX_HD inline bool token_digits(const uint8_t* s, uint32_t len, uint16_t* out) {
    if (len == 0 || len > 18) return false;
    uint64_t v = 0;
    for (uint32_t i = 0; i < len; ++i) { const uint32_t d = (uint32_t)s[i] - '0'; if (d > 9) return false; v = v * 10 + d; }
    *out = (uint16_t)v;
    return true;
}

// tile_x_y: the ':'-separated tokens of the name (empty ones do not count); 7 tokens -> 5th to 7th, 6 -> 4th to 6th
MGX_HD inline void name_keys(const uint8_t* q, uint32_t len, uint16_t out[3], uint8_t* redo) {
    uint32_t tb[8], tl[8];
    uint32_t n = 0, i = 0;
    while (i < len) {
        while (i < len && q[i] == ':') ++i;
        if (i >= len) break;
        const uint32_t b = i;
        while (i < len && q[i] != ':') ++i;
        if (n < 8) { tb[n] = b; tl[n] = i - b; }
        ++n;
    }
    out[0] = out[1] = out[2] = 0;
    const int first = n == 7 ? 4 : (n == 6 ? 3 : -1);
    if (first < 0) return;
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = token_digits(q + tb[first + k], tl[first + k], &out[k]) && ok;
    if (!ok) { out[0] = out[1] = out[2] = 0; *redo |= kRedoToken; }
}

// whether the names (without NUL) of the valid records at a and b are equal
MGX_HD inline bool same_name(const uint8_t* a, const uint8_t* b) {
    const uint32_t la = a[12];
    if (la != b[12]) return false;
    for (uint32_t i = 0; i + 1 < la; ++i) if (a[kFixed + i] != b[kFixed + i]) return false;
    return true;
}

// The key of a valid record from its fixed part, name and CIGAR, with the two fields whose computation differs between
// the callers handed in: the device kernel sums the qualities and compares the names eight lanes to a record.  (Hidden:
// out of the library's symbol list where a compiler leaves it out of line.)
__attribute__((visibility("hidden"))) MGX_HD inline void key_from(const Fixed& f, const uint8_t* name, const uint8_t* cig, uint16_t score, uint8_t same_qname, mgx_bam_key_t* k) {
    uint8_t redo = 0;
    int64_t d5, ref;
    cigar_keys(cig, f.n_cigar, (f.flag & 0x10u) == 0, f.l_seq, &d5, &ref, &redo);
    uint16_t t[3];
    name_keys(name, f.l_read_name - 1, t, &redo);
    k->d5 = d5; k->tid = f.tid; k->pos = f.pos;
    k->end = (int32_t)((int64_t)f.pos + (ref > 0 ? ref : 1));
    k->flag = (uint16_t)f.flag; k->score = score;
    k->tile = t[0]; k->x = t[1]; k->y = t[2];
    k->same_qname = same_qname; k->redo = redo;
}

// The whole key of the valid record at p; prev = the record before it in the call, or nullptr.
MGX_HD inline void record_key(const uint8_t* p, const uint8_t* prev, mgx_bam_key_t* k) {
    const Fixed f = read_fixed(p);
    const uint8_t* name = p + kFixed;
    const uint8_t* cig = name + f.l_read_name;
    const uint8_t* qual = cig + 4ull * f.n_cigar + ((uint64_t)f.l_seq + 1) / 2;
    key_from(f, name, cig, score_bytes(qual, 0, (uint32_t)f.l_seq), prev && same_name(p, prev) ? 1 : 0, k);
}

}  // namespace mgx_bam
#endif
