// bgzf_inflate_core.h -- the validity logic of the BGZF inflater, one text for the device kernel
// (mgx_bgzf_inflate.hip) and for plain host C++ (the block scanner, bgzf_scan.cpp, and the CPU tests that run it under
// AddressSanitizer + UBSan).
//
// What is here: the BGZF member header (htslib bgzf.c:874-880), Huffman code construction with zlib's rejection rules
// (inftrees.c: over-subscribed sets, incomplete sets except a single code of length 1 in the literal/length or distance
// code, a missing end-of-block code), and the DEFLATE decode loop of RFC 1951 with every read, table index, distance
// and output length checked against the block's own ranges.  What the decoded symbols become is left to a Sink:
//     sink.lit(byte, pos)        one literal at output position pos
//     sink.match(len, dist, pos) len bytes copied from pos - dist (3 <= len <= 258, 1 <= dist <= pos)
//     sink.stored(src, len, pos) len bytes of a stored block, src inside the input range
// The loop is wave-uniform on the device: every lane of the wavefront runs it with the same values, so a sink may use
// wavefront-collective operations inside these calls.
#ifndef MGX_BGZF_INFLATE_CORE_H
#define MGX_BGZF_INFLATE_CORE_H

#include <stdint.h>

#ifndef MGX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MGX_HD __host__ __device__
#else
#define MGX_HD
#endif
#endif

namespace mgx_inflate {

enum Status : uint32_t {
    kOk = 0,
    kBadHeader,        // not a gzip member with the BGZF extra field
    kBadBlockSize,     // BSIZE + 1 is not the block's compressed range, or too small to hold header and trailer
    kTruncated,        // the DEFLATE stream runs past the end of the payload
    kBadBlockType,     // BTYPE 11
    kStoredLength,     // LEN != ~NLEN
    kBadCodeLengths,   // too many length / distance symbols, a repeat with nothing to repeat or past the end
    kOverSubscribed,   // a code-length set with more codes than fit
    kIncomplete,       // an incomplete code-length set (allowed only for one code of length 1 in a literal/length or distance code)
    kMissingEob,       // no code for end-of-block
    kBadSymbol,        // a bit pattern no code has, or literal/length 286-287, distance 30-31
    kDistTooFar,       // a distance back past the start of the block
    kOutputOverflow,   // more output than ISIZE (at most 65 536 bytes)
    kIsizeMismatch,    // the stream ended with fewer bytes than ISIZE, or ISIZE is not the output range given
    kCrcMismatch,      // CRC-32 of the output differs from the trailer's
    kBadIsize,         // ISIZE above 65 536
    kNumStatus
};

inline const char* status_text(uint32_t s) {
    static const char* const names[kNumStatus] = {
        "ok", "not a BGZF member header", "block size field does not match the block", "DEFLATE stream truncated",
        "invalid block type", "stored block length does not match its complement", "invalid code lengths",
        "over-subscribed code", "incomplete code", "no end-of-block code", "invalid code", "distance too far back",
        "output longer than ISIZE", "output length differs from ISIZE", "CRC-32 mismatch", "ISIZE above 64 KB"};
    return s < kNumStatus ? names[s] : "unknown status";
}

constexpr uint32_t kHeaderBytes = 18, kTrailerBytes = 8;
constexpr uint32_t kMaxBlock = 65536;   // BSIZE is 16 bits: a member is at most 65 536 bytes
constexpr uint32_t kMaxIsize = 65536;   // and inflates to at most 64 KB

MGX_HD inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
MGX_HD inline uint32_t rd32(const uint8_t* p) { return rd16(p) | rd16(p + 2) << 16; }

// A BGZF member header at p (avail bytes readable): kOk and the member's total size, kTruncated when fewer than 18 bytes
// are there, kBadHeader otherwise.  The layout is htslib's check (bgzf.c:874-880): the FEXTRA flag, XLEN 6, one 'BC'
// subfield of length 2.
MGX_HD inline uint32_t parse_header(const uint8_t* p, uint64_t avail, uint32_t* block_size) {
    if (avail < 4) return kTruncated;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return kBadHeader;
    if (avail < kHeaderBytes) return kTruncated;
    if (rd16(p + 10) != 6 || p[12] != 'B' || p[13] != 'C' || rd16(p + 14) != 2) return kBadHeader;
    *block_size = rd16(p + 16) + 1;
    if (*block_size < kHeaderBytes + kTrailerBytes) return kBadBlockSize;
    return kOk;
}

// ---- bits, LSB first, never past n bytes ---------------------------------------------------------------------------
struct BitReader {
    const uint8_t* p; uint32_t n, pos; uint64_t buf; uint32_t cnt; bool over;
    MGX_HD void init(const uint8_t* src, uint32_t len) { p = src; n = len; pos = 0; buf = 0; cnt = 0; over = false; }
    MGX_HD void refill() { while (cnt <= 56 && pos < n) { buf |= (uint64_t)p[pos++] << cnt; cnt += 8; } }
    MGX_HD uint32_t peek(uint32_t k) { if (cnt < k) refill(); return (uint32_t)(buf & ((1ull << k) - 1)); }   // zero bits past the end
    MGX_HD void drop(uint32_t k) { buf >>= k; cnt -= k; }
    MGX_HD uint32_t bits(uint32_t k) {    // k <= 32
        if (cnt < k) refill();
        if (cnt < k) { over = true; return 0; }
        const uint32_t v = (uint32_t)(buf & ((1ull << k) - 1));
        drop(k);
        return v;
    }
};

// ---- canonical Huffman codes ---------------------------------------------------------------------------------------
constexpr int kFastLL = 10, kFastD = 8;   // first-level lookup: codes up to this many bits in one table read
struct Huff { uint16_t count[16]; uint16_t symbol[288]; };   // puff.c's form: codes per length, symbols in code order
struct Tables {
    uint16_t fast_ll[1 << kFastLL];      // entry: length << 9 | symbol, 0 = a code longer than kFastLL bits (or none)
    uint16_t fast_d[1 << kFastD];
    Huff ll, d;
    uint8_t lens[320];                   // 286 + 30 code lengths; the 19 of the code-length code first
};
enum CodeKind { kCodes, kLens, kDists };

// Builds the code of lens[0, n).  kOk, kOverSubscribed, or kIncomplete (zlib inftrees.c: an incomplete set passes only
// for a literal/length or distance code whose longest code is 1 bit; an empty distance code passes and fails on use).
MGX_HD inline uint32_t build(const uint8_t* lens, int n, CodeKind kind, Huff* h, uint16_t* fast, int fast_bits) {
    for (int l = 0; l < 16; ++l) h->count[l] = 0;
    for (int s = 0; s < n; ++s) h->count[lens[s]]++;
    for (int i = 0; i < (1 << fast_bits); ++i) fast[i] = 0;
    if (h->count[0] == n) return kind == kDists ? kOk : kIncomplete;
    int left = 1, max = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - h->count[l];
        if (left < 0) return kOverSubscribed;
        if (h->count[l]) max = l;
    }
    if (left > 0 && (kind == kCodes || max != 1)) return kIncomplete;
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h->count[l]);
    for (int s = 0; s < n; ++s) if (lens[s]) h->symbol[offs[lens[s]]++] = (uint16_t)s;
    // first-level table: every code of at most fast_bits bits fills the entries that start with it (bit-reversed)
    uint32_t code = 0; int idx = 0;
    for (int l = 1; l <= fast_bits; ++l) {
        for (int k = 0; k < h->count[l]; ++k, ++idx, ++code) {
            uint32_t r = 0;
            for (int b = 0; b < l; ++b) r |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t j = r; j < (1u << fast_bits); j += 1u << l) fast[j] = (uint16_t)(l << 9 | h->symbol[idx]);
        }
        code <<= 1;
    }
    return kOk;
}

// One symbol, or -1: no code has the pattern (or the input ended inside it -- *trunc says which).
MGX_HD inline int decode(BitReader& br, const Huff& h, const uint16_t* fast, int fast_bits, bool* trunc) {
    const uint32_t e = fast[br.peek(15) & ((1u << fast_bits) - 1)];
    if (e) {
        const uint32_t l = e >> 9;
        if (l > br.cnt) { *trunc = true; return -1; }
        br.drop(l);
        return (int)(e & 511u);
    }
    int code = 0, first = 0, index = 0;      // puff.c decode(), from the first bit (short codes are all in the table)
    for (int len = 1; len < 16; ++len) {
        if ((uint32_t)len > br.cnt) { *trunc = true; return -1; }
        code |= (int)((br.buf >> (len - 1)) & 1u);
        const int count = h.count[len];
        if (code - count < first) { br.drop((uint32_t)len); return h.symbol[index + (code - first)]; }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -1;
}

MGX_HD inline uint32_t fixed_tables(Tables& t) {
    for (int s = 0; s < 288; ++s) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    uint32_t st = build(t.lens, 288, kLens, &t.ll, t.fast_ll, kFastLL);
    for (int s = 0; s < 32; ++s) t.lens[s] = 5;
    if (st == kOk) st = build(t.lens, 32, kDists, &t.d, t.fast_d, kFastD);
    return st;
}

MGX_HD inline uint32_t dynamic_tables(BitReader& br, Tables& t) {
    const uint32_t nlen = br.bits(5) + 257, ndist = br.bits(5) + 1, ncode = br.bits(4) + 4;
    if (br.over) return kTruncated;
    if (nlen > 286 || ndist > 30) return kBadCodeLengths;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) cl[order[i]] = (uint8_t)br.bits(3);
    if (br.over) return kTruncated;
    // the code-length code goes through the distance tables (7 bits at most: always the first-level table)
    uint32_t st = build(cl, 19, kCodes, &t.d, t.fast_d, kFastD);
    if (st != kOk) return st;
    uint32_t i = 0;
    while (i < nlen + ndist) {
        bool trunc = false;
        const int sym = decode(br, t.d, t.fast_d, kFastD, &trunc);
        if (sym < 0) return trunc ? kTruncated : kBadCodeLengths;
        if (sym < 16) { t.lens[i++] = (uint8_t)sym; continue; }
        uint32_t rep; uint8_t v = 0;
        if (sym == 16) { if (i == 0) return kBadCodeLengths; v = t.lens[i - 1]; rep = 3 + br.bits(2); }
        else if (sym == 17) rep = 3 + br.bits(3);
        else rep = 11 + br.bits(7);
        if (br.over) return kTruncated;
        if (i + rep > nlen + ndist) return kBadCodeLengths;
        while (rep--) t.lens[i++] = v;
    }
    if (t.lens[256] == 0) return kMissingEob;
    st = build(t.lens, (int)nlen, kLens, &t.ll, t.fast_ll, kFastLL);
    if (st != kOk) return st;
    return build(t.lens + nlen, (int)ndist, kDists, &t.d, t.fast_d, kFastD);
}

// Raw DEFLATE of in[0, n_in) into at most out_cap bytes.  *n_out = bytes produced (also on error: how far it got).
template <class Sink>
MGX_HD uint32_t inflate_raw(const uint8_t* in, uint32_t n_in, uint32_t out_cap, Tables& t, Sink& sink, uint32_t* n_out) {
    BitReader br;
    br.init(in, n_in);
    uint32_t out = 0, st = kOk;
    for (;;) {
        const uint32_t last = br.bits(1), type = br.bits(2);
        if (br.over) { st = kTruncated; break; }
        if (type == 0) {
            br.drop(br.cnt & 7u);                            // to the byte boundary
            const uint32_t len = br.bits(16), nlen = br.bits(16);
            if (br.over) { st = kTruncated; break; }
            if (len != (~nlen & 0xffffu)) { st = kStoredLength; break; }
            const uint32_t at = br.pos - br.cnt / 8;          // the bytes still in the bit buffer come first
            if (len > n_in - at) { st = kTruncated; break; }
            if (len > out_cap - out) { st = kOutputOverflow; break; }
            sink.stored(in + at, len, out);
            out += len;
            br.pos = at + len; br.buf = 0; br.cnt = 0;
        } else if (type == 3) {
            st = kBadBlockType; break;
        } else {
            st = type == 1 ? fixed_tables(t) : dynamic_tables(br, t);
            if (st != kOk) break;
            for (;;) {
                bool trunc = false;
                int sym = decode(br, t.ll, t.fast_ll, kFastLL, &trunc);
                if (sym < 0) { st = trunc ? kTruncated : kBadSymbol; break; }
                if (sym < 256) {
                    if (out >= out_cap) { st = kOutputOverflow; break; }
                    sink.lit((uint32_t)sym, out);
                    ++out;
                    continue;
                }
                if (sym == 256) break;
                sym -= 257;
                if (sym >= 29) { st = kBadSymbol; break; }
                uint32_t len;
                if (sym < 8) len = 3u + (uint32_t)sym;
                else if (sym == 28) len = 258;
                else { const uint32_t e = ((uint32_t)sym >> 2) - 1; len = ((4u + ((uint32_t)sym & 3u)) << e) + 3u + br.bits(e); }
                const int ds = decode(br, t.d, t.fast_d, kFastD, &trunc);
                if (ds < 0) { st = trunc ? kTruncated : kBadSymbol; break; }
                if (ds >= 30) { st = kBadSymbol; break; }
                uint32_t dist;
                if (ds < 4) dist = 1u + (uint32_t)ds;
                else { const uint32_t e = ((uint32_t)ds >> 1) - 1; dist = ((2u + ((uint32_t)ds & 1u)) << e) + 1u + br.bits(e); }
                if (br.over) { st = kTruncated; break; }
                if (dist > out) { st = kDistTooFar; break; }
                if (len > out_cap - out) { st = kOutputOverflow; break; }
                sink.match(len, dist, out);
                out += len;
            }
            if (st != kOk) break;
        }
        if (last) break;
    }
    *n_out = out;
    return st;
}

// The checks around the DEFLATE stream of one member block[0, n): header, BSIZE == n, ISIZE <= 64 KB and == out_len.
// *payload / *payload_len: the DEFLATE stream; *crc: the trailer's CRC-32.
MGX_HD inline uint32_t member_bounds(const uint8_t* block, uint64_t n, uint32_t out_len, uint32_t* payload_len, uint32_t* crc) {
    uint32_t bsize = 0;
    uint32_t st = parse_header(block, n, &bsize);
    if (st == kTruncated) return kBadBlockSize;
    if (st != kOk) return st;
    if (bsize != n) return kBadBlockSize;
    const uint32_t isize = rd32(block + n - 4);
    if (isize > kMaxIsize) return kBadIsize;
    if (isize != out_len) return kIsizeMismatch;
    *crc = rd32(block + n - 8);
    *payload_len = (uint32_t)n - kHeaderBytes - kTrailerBytes;
    return kOk;
}

}  // namespace mgx_inflate

#endif
