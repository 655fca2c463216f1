// sam_line_core.h -- the rules that turn one SAM alignment line into one BAM record (block_size + the record of SAMv1
// 4.2), one text for the host implementation (sam_host.cpp, which the CPU tests run under AddressSanitizer + UBSan) and
// for the device kernels (mgx_sam.hip), DESIGN.md 4.9.  Plain C++, no library call.
//
// The definition of the result is samtext::parse_record_into (cli/sam_text.cpp): what these rules encode is byte-equal
// to it.  The rules may DECLINE a line (size 0): the host parser then encodes it, or words the error, as it always did.
// What is declined:
//   - a line longer than max_line bytes (the device stages a line in LDS: kMaxLine; the host functions take the limit
//     as an argument so that the rules can be run on longer lines too);
//   - fewer than 11 fields; QNAME empty or longer than 254 bytes;
//   - FLAG, POS, MAPQ, PNEXT, TLEN not an optional sign followed by 1-18 digits;
//   - FLAG outside [0, 65535], MAPQ outside [0, 255] (the host rejects them); POS or PNEXT outside [-2^31 + 1, 2^31 - 1],
//     TLEN outside [-2^31, 2^31 - 1] (the host truncates them);
//   - RNAME / RNEXT not in the header ('*', and '=' for RNEXT, are handled here);
//   - a CIGAR the host calls bad (an unknown letter, an operation without a length, digits at the end), an operation
//     length of 2^28 or more, more than 65535 operations -- and, added to the list this feature was specified with, an operation length written
//     with more than 9 digits: the host accumulates the digits in 64 bits and lets them wrap, which is not restated;
//   - SEQ and QUAL of different lengths (QUAL '*' excepted);
//   - an optional field shorter than 5 bytes or without its two colons, or of a type other than A i Z H B;
//   - an `i` value that is not sign + 1-18 digits or lies outside [-2^31, 2^32) (the host truncates it);
//   - type f (strtof is not restated); type B with subtype f, an unknown subtype, no subtype, or an item that is not
//     sign + 1-18 digits.
// Everything else is encoded.  Empty optional fields are skipped; empty items of a B array are skipped; B items are
// cast to their width as the host's strtol / strtoul path casts them (two's complement, the low bytes).
//
// Size bound: 4 + block_size <= 36 + 2 * len.  36 bytes are block_size and the fixed part, which the five numeric
// fields, RNAME and RNEXT feed without further output.  Of the rest every output byte is paid by input bytes:
//   QNAME        n + 1 bytes (the NUL) for n bytes and the tab behind it;
//   CIGAR        4 bytes per operation, which is at least one digit and one letter: factor 2;
//   SEQ + QUAL   (l + 1) / 2 + l bytes for 2 l bytes (or, QUAL '*', for l + 1 bytes: 1.5 l + 0.5 <= 2 l for l >= 1);
//   A / i        4 / at most 7 bytes for a tab and at least 5 / 6 bytes;   Z / H   v + 4 bytes for a tab and v + 5 bytes;
//   B            8 + w k bytes (w <= 4) for a tab, 6 bytes and k items of at least a comma and a digit: 8 + 4 k <= 2 (7 + 2 k).
// CIGAR and B:i / B:I are the cases that come close to the factor.
#ifndef MGX_SAM_LINE_CORE_H
#define MGX_SAM_LINE_CORE_H

#include <stdint.h>

#ifndef MGX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MGX_HD __host__ __device__
#else
#define MGX_HD
#endif
#endif

namespace mgx_sam {

constexpr uint32_t kMaxLine = 2048;        // the longest line the device stages (MGX_SAM_MAX_LINE)
constexpr uint32_t kFixed = 36;            // block_size + the 32 fixed bytes
constexpr uint8_t kRedoDeclined = 4;       // mgx_bam_key_t::redo bit 2: the line was declined, the host parser encodes it
constexpr uint32_t kEmptySlot = 0xFFFFFFFFu;

MGX_HD inline uint64_t size_bound(uint64_t len) { return kFixed + 2 * len; }

// UCSC binning (SAMv1 5.3) as the writer has always computed it: bamout::reg2bin is this function
MGX_HD inline int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// ---- reference names: an open-addressed table in one block of 32-bit words, the same bytes on host and device ------
//   word 0 n_ref, 1 n_slots (a power of two, > n_ref), 2 bytes of names, 3 unused; name_off[n_ref + 1]; slot[n_slots]
//   (a reference index or kEmptySlot); the names back to back.  Of equal names only the lowest index has a slot.
struct Table {
    const uint32_t* name_off; const uint32_t* slot; const uint8_t* names;
    uint32_t n_ref, n_slots;
};

MGX_HD inline Table table_view(const uint32_t* blob) {
    Table t;
    t.n_ref = blob[0]; t.n_slots = blob[1];
    t.name_off = blob + 4; t.slot = t.name_off + t.n_ref + 1; t.names = (const uint8_t*)(t.slot + t.n_slots);
    return t;
}

MGX_HD inline uint32_t name_hash(const uint8_t* s, uint32_t len) {
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < len; ++i) h = (h ^ s[i]) * 16777619u;
    return h;
}

MGX_HD inline bool name_is(const Table& t, uint32_t r, const uint8_t* s, uint32_t len) {
    const uint32_t b = t.name_off[r];
    if (t.name_off[r + 1] - b != len) return false;
    for (uint32_t i = 0; i < len; ++i) if (t.names[b + i] != s[i]) return false;
    return true;
}

// the lowest index of the reference called s[0, len), or -1 (Header::find)
MGX_HD inline int32_t find_ref(const Table& t, const uint8_t* s, uint32_t len) {
    uint32_t h = name_hash(s, len) & (t.n_slots - 1);
    for (uint32_t probe = 0; probe < t.n_slots; ++probe) {
        const uint32_t r = t.slot[h];
        if (r == kEmptySlot) return -1;
        if (r < t.n_ref && name_is(t, r, s, len)) return (int32_t)r;
        h = (h + 1) & (t.n_slots - 1);
    }
    return -1;
}

// ---- text ------------------------------------------------------------------------------------------------------------
// an optional sign followed by 1-18 digits
MGX_HD inline bool parse_int(const uint8_t* s, uint32_t n, int64_t* v) {
    if (n == 0) return false;
    const bool neg = s[0] == '-';
    uint32_t i = (s[0] == '-' || s[0] == '+') ? 1 : 0;
    if (i == n || n - i > 18) return false;
    int64_t x = 0;
    for (; i < n; ++i) {
        const uint32_t d = (uint32_t)s[i] - '0';
        if (d > 9) return false;
        x = x * 10 + (int64_t)d;
    }
    *v = neg ? -x : x;
    return true;
}

MGX_HD inline uint32_t find_byte(const uint8_t* s, uint32_t from, uint32_t to, uint8_t c) {
    while (from < to && s[from] != c) ++from;
    return from;
}

MGX_HD inline int cigar_op(uint8_t ch) {
    switch (ch) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; case 'B': return 9;
        default: return -1;
    }
}

// the 4-bit code of a base: "=ACMGRSVTWYHKDBN", either case, anything else 15.  The 26 letters' codes are the nibbles
// of two constants (a..p, q..z), so that the kernel needs no table in memory.
MGX_HD inline uint32_t base_code(uint8_t c) {
    if (c == '=') return 0;
    const uint32_t k = (uint32_t)(c | 0x20) - 'a';
    if (k >= 26) return 15;
    return (uint32_t)((k < 16 ? 0xFFF3FCFFB4FFD2E1ull >> (4 * k) : 0xFAF97F865Full >> (4 * (k - 16))) & 15u);
}

// What the size-and-validate pass learns of an accepted line; offsets are into the line.
struct Line {
    uint32_t f[11], n[11];                 // the mandatory fields
    uint32_t aux;                          // where the optional fields start (len + 1: there are none)
    int32_t tid, pos, mtid, mpos, tlen, end;
    uint32_t flag, mapq, n_cigar, l_seq;
    bool no_qual;
    uint32_t size;                         // 4 + block_size; 0: declined
};

// The output of a line.  A group of n_lanes lanes runs the SAME calls on the same line: the short serial pieces are
// stored by lane 0, the long runs by all lanes in pieces of 8 bytes.  out == nullptr only counts.  No store lies at or
// beyond cap, whatever the line holds.
struct Writer {
    uint8_t* out; uint32_t pos, cap, lane, n_lanes;

    MGX_HD void put8(uint32_t v) { if (out && lane == 0 && pos < cap) out[pos] = (uint8_t)v; pos += 1; }
    MGX_HD void put16(uint32_t v) { put8(v & 0xff); put8(v >> 8 & 0xff); }
    MGX_HD void put32(uint32_t v) {
        if (out && lane == 0 && pos + 4 <= cap) { const uint32_t w = v; __builtin_memcpy(out + pos, &w, 4); }
        pos += 4;
    }
    // kind 0: copy; 1: qualities (byte - 33); 2: a constant byte v; all n bytes
    MGX_HD void run(const uint8_t* src, uint32_t n, int kind, uint8_t v) {
        if (out) {
            for (uint32_t i = lane * 8; i < n; i += n_lanes * 8) {
                const uint32_t k = n - i < 8 ? n - i : 8;
                uint8_t t[8];
                for (uint32_t j = 0; j < 8; ++j) t[j] = j < k ? (kind == 2 ? v : kind == 1 ? (uint8_t)(src[i + j] - 33) : src[i + j]) : 0;
                if (k == 8 && pos + i + 8 <= cap) __builtin_memcpy(out + pos + i, t, 8);
                else for (uint32_t j = 0; j < k; ++j) if (pos + i + j < cap) out[pos + i + j] = t[j];
            }
        }
        pos += n;
    }
    // l bases -> (l + 1) / 2 bytes
    MGX_HD void bases(const uint8_t* src, uint32_t l) {
        const uint32_t nb = (l + 1) / 2;
        if (out) {
            for (uint32_t i = lane * 8; i < nb; i += n_lanes * 8) {
                const uint32_t k = nb - i < 8 ? nb - i : 8;
                uint8_t t[8];
                for (uint32_t j = 0; j < 8; ++j) {
                    const uint32_t b = 2 * (i + j);
                    t[j] = j < k ? (uint8_t)(base_code(src[b]) << 4 | (b + 1 < l ? base_code(src[b + 1]) : 0u)) : 0;
                }
                if (k == 8 && pos + i + 8 <= cap) __builtin_memcpy(out + pos + i, t, 8);
                else for (uint32_t j = 0; j < k; ++j) if (pos + i + j < cap) out[pos + i + j] = t[j];
            }
        }
        pos += nb;
    }
};

// the smallest BAM integer type holding v (put_int_tag), v in [-2^31, 2^32)
MGX_HD inline void put_int_tag(Writer& w, int64_t v) {
    if (v < 0) {
        if (v >= -128) { w.put8('c'); w.put8((uint32_t)v & 0xff); }
        else if (v >= -32768) { w.put8('s'); w.put16((uint32_t)v & 0xffff); }
        else { w.put8('i'); w.put32((uint32_t)v); }
    } else {
        if (v <= 255) { w.put8('C'); w.put8((uint32_t)v); }
        else if (v <= 65535) { w.put8('S'); w.put16((uint32_t)v); }
        else { w.put8('I'); w.put32((uint32_t)v); }
    }
}

// One non-empty optional field f[0, n).  false: declined (what was written then does not count).
MGX_HD inline bool aux_field(const uint8_t* f, uint32_t n, Writer& w) {
    if (n < 5 || f[2] != ':' || f[4] != ':') return false;
    const uint8_t type = f[3];
    const uint8_t* v = f + 5;
    const uint32_t vn = n - 5;
    if (type != 'A' && type != 'i' && type != 'Z' && type != 'H' && type != 'B') return false;
    w.put8(f[0]); w.put8(f[1]);
    if (type == 'A') { w.put8('A'); w.put8(vn ? v[0] : 0); return true; }
    if (type == 'i') {
        int64_t x;
        if (!parse_int(v, vn, &x) || x < -2147483648ll || x > 4294967295ll) return false;
        put_int_tag(w, x);
        return true;
    }
    if (type == 'Z' || type == 'H') { w.put8(type); w.run(v, vn, 0, 0); w.put8(0); return true; }
    if (vn < 1) return false;
    const uint8_t sub = v[0];
    const uint32_t width = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I') ? 4 : 0;
    if (width == 0) return false;
    uint32_t count = 0;
    for (uint32_t i = 1; i < vn;) {
        if (v[i] == ',') { ++i; continue; }
        const uint32_t j = find_byte(v, i, vn, ',');
        int64_t x;
        if (!parse_int(v + i, j - i, &x)) return false;
        ++count; i = j;
    }
    w.put8('B'); w.put8(sub); w.put32(count);
    if (!w.out) { w.pos += count * width; return true; }
    for (uint32_t i = 1; i < vn;) {
        if (v[i] == ',') { ++i; continue; }
        const uint32_t j = find_byte(v, i, vn, ',');
        int64_t x = 0;
        parse_int(v + i, j - i, &x);
        if (width == 1) w.put8((uint32_t)x & 0xff); else if (width == 2) w.put16((uint32_t)x & 0xffff); else w.put32((uint32_t)x);
        i = j;
    }
    return true;
}

// all optional fields of s[0, len) from offset p on
MGX_HD inline bool aux_fields(const uint8_t* s, uint32_t len, uint32_t p, Writer& w) {
    while (p <= len) {
        const uint32_t e = find_byte(s, p, len, '\t');
        if (e > p && !aux_field(s + p, e - p, w)) return false;
        p = e + 1;
    }
    return true;
}

// Size and validate: the line s[0, len) (no newline, no trailing CR, len > 0).  L->size is 4 + block_size, or 0.
MGX_HD inline bool scan_line(const uint8_t* s, uint32_t len, const Table& t, uint32_t max_line, Line* L) {
    L->size = 0;
    if (len > max_line) return false;
    uint32_t p = 0;
    for (int k = 0; k < 11; ++k) {
        if (p > len) return false;
        const uint32_t e = find_byte(s, p, len, '\t');
        L->f[k] = p; L->n[k] = e - p;
        p = e + 1;
    }
    L->aux = p;
    const uint32_t* f = L->f; const uint32_t* n = L->n;
    int64_t v;
    if (n[0] == 0 || n[0] > 254) return false;
    if (!parse_int(s + f[1], n[1], &v) || v < 0 || v > 65535) return false;
    L->flag = (uint32_t)v;
    const bool no_ref = n[2] == 1 && s[f[2]] == '*';
    L->tid = no_ref ? -1 : find_ref(t, s + f[2], n[2]);
    if (L->tid < 0 && !no_ref) return false;
    if (!parse_int(s + f[3], n[3], &v) || v < -2147483647ll || v > 2147483647ll) return false;
    L->pos = (int32_t)v - 1;
    if (!parse_int(s + f[4], n[4], &v) || v < 0 || v > 255) return false;
    L->mapq = (uint32_t)v;
    uint32_t n_cig = 0;
    int64_t ref_len = 0;
    if (!(n[5] == 1 && s[f[5]] == '*')) {
        uint32_t num = 0, digits = 0;
        for (uint32_t i = 0; i < n[5]; ++i) {
            const uint8_t ch = s[f[5] + i];
            if (ch >= '0' && ch <= '9') { if (++digits > 9) return false; num = num * 10 + (uint32_t)(ch - '0'); continue; }
            const int op = cigar_op(ch);
            if (op < 0 || digits == 0 || num >= (1u << 28)) return false;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += (int64_t)num;
            ++n_cig; num = 0; digits = 0;
        }
        if (digits) return false;
        if (n_cig > 65535) return false;
    }
    L->n_cigar = n_cig;
    L->end = (int32_t)((int64_t)L->pos + (ref_len > 0 ? ref_len : 1));
    if (n[6] == 1 && s[f[6]] == '=') L->mtid = L->tid;
    else if (n[6] == 1 && s[f[6]] == '*') L->mtid = -1;
    else { L->mtid = find_ref(t, s + f[6], n[6]); if (L->mtid < 0) return false; }
    if (!parse_int(s + f[7], n[7], &v) || v < -2147483647ll || v > 2147483647ll) return false;
    L->mpos = (int32_t)v - 1;
    if (!parse_int(s + f[8], n[8], &v) || v < -2147483648ll || v > 2147483647ll) return false;
    L->tlen = (int32_t)v;
    const bool no_seq = n[9] == 1 && s[f[9]] == '*';
    L->l_seq = no_seq ? 0u : n[9];
    L->no_qual = n[10] == 1 && s[f[10]] == '*';
    if (!L->no_qual && n[10] != L->l_seq) return false;
    Writer count = {nullptr, 0, 0, 0, 1};
    if (!aux_fields(s, len, L->aux, count)) return false;
    L->size = kFixed + n[0] + 1 + 4 * n_cig + (L->l_seq + 1) / 2 + L->l_seq + count.pos;
    return true;
}

// Encode: the accepted line as scan_line left it in L, through w (w.cap = L.size).  Returns the bytes written.
MGX_HD inline uint32_t encode_line(const uint8_t* s, uint32_t len, const Line& L, Writer& w) {
    w.put32(L.size - 4);
    w.put32((uint32_t)L.tid); w.put32((uint32_t)L.pos);
    w.put8(L.n[0] + 1); w.put8(L.mapq); w.put16((uint32_t)reg2bin(L.pos, L.end) & 0xffff);
    w.put16(L.n_cigar); w.put16(L.flag); w.put32(L.l_seq);
    w.put32((uint32_t)L.mtid); w.put32((uint32_t)L.mpos); w.put32((uint32_t)L.tlen);
    w.run(s + L.f[0], L.n[0], 0, 0); w.put8(0);
    if (L.n_cigar) {
        uint32_t num = 0;
        for (uint32_t i = 0; i < L.n[5]; ++i) {
            const uint8_t ch = s[L.f[5] + i];
            if (ch >= '0' && ch <= '9') { num = num * 10 + (uint32_t)(ch - '0'); continue; }
            w.put32(num << 4 | (uint32_t)cigar_op(ch));
            num = 0;
        }
    }
    w.bases(s + L.f[9], L.l_seq);
    if (L.no_qual) w.run(nullptr, L.l_seq, 2, 0xFF); else w.run(s + L.f[10], L.l_seq, 1, 0);
    aux_fields(s, len, L.aux, w);
    return w.pos;
}

// ---- line framing (parse_slice of cli/ingest.cpp): lines end at '\n', one trailing '\r' is dropped, empty lines are
// skipped, the last line may lack its newline.  Both predicates look at single bytes around a position, so a tile of
// text can evaluate them for its own positions.  at(i) is the byte at i for 0 <= i < n.
// whether a non-empty line starts at p (0 <= p < n)
template <typename At>
MGX_HD inline bool line_starts(const At& at, uint64_t p, uint64_t n) {
    if (p >= n || (p > 0 && at(p - 1) != '\n')) return false;
    const uint8_t c = at(p);
    if (c == '\n') return false;
    return !(c == '\r' && (p + 1 == n || at(p + 1) == '\n'));
}
// whether a non-empty line ends in front of q (1 <= q <= n: a newline at q, or the end of the text)
template <typename At>
MGX_HD inline bool line_ends(const At& at, uint64_t q, uint64_t n) {
    if (q == 0 || q > n) return false;
    if (q == n ? at(n - 1) == '\n' : at(q) != '\n') return false;
    const uint8_t c = at(q - 1);
    if (c == '\n') return false;
    return !(c == '\r' && (q == 1 || at(q - 2) == '\n'));
}

// the QNAME of a line for same_qname: the bytes before the first tab
MGX_HD inline uint32_t qname_len(const uint8_t* s, uint32_t len) { return find_byte(s, 0, len, '\t'); }
MGX_HD inline bool same_qname(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
    const uint32_t qa = qname_len(a, la);
    if (qa != qname_len(b, lb)) return false;
    for (uint32_t i = 0; i < qa; ++i) if (a[i] != b[i]) return false;
    return true;
}

}  // namespace mgx_sam
#endif
