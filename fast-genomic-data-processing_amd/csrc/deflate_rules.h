// deflate_rules.h -- the rules of DEFLATE (RFC 1951), gzip's CRC-32 and the BGZF member frame that k_bgzf_deflate (mgx_bgzf.hip)
// follows, each written once.  No HIP: the kernel calls them per lane, tests/cpp/deflate_rules_driver.cpp calls them serially
// (tests/test_deflate_rules_host.py: CPU, ASan + UBSan, against the RFC's tables, package-merge and zlib).
// Everything is inline and no struct is chosen by address (see the scratch note in best_allele_rule.h), so nothing here costs the
// kernel a register.  The inflater keeps its own tables (bgzf_inflate_core.h).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MGX_DF_FN __host__ __device__ __forceinline__
#else
#define MGX_DF_FN inline
#endif

namespace mgx_deflate {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr int kNumLL = 286, kNumD = 30, kNumCL = 19;
constexpr u32 kEndOfBlock = 256, kMinMatch = 3, kMaxMatch = 258, kMaxDist = 32768;
constexpr int kHashBits = 12;

MGX_DF_FN u32 floor_log2(u32 x) { return 31u - (u32)__builtin_clz(x); }            // x != 0

// ---- symbols (RFC 1951 3.2.5).  The number of extra bits is a function of the symbol; the encoders below take it from there.
MGX_DF_FN u32 length_extra_bits(u32 ls) { return (ls >= 265 && ls < 285) ? (ls - 261) >> 2 : 0u; }
MGX_DF_FN u32 dist_extra_bits(u32 ds) { return ds >= 4 ? (ds >> 1) - 1 : 0u; }
MGX_DF_FN u32 length_symbol(u32 length) {                                          // 3..258 -> 257..285
    const u32 l = length - 3;
    if (l < 8) return 257 + l;
    if (l == 255) return 285;
    const u32 msb = floor_log2(l);
    return 257 + 4 * (msb - 1) + ((l >> (msb - 2)) & 3);
}
MGX_DF_FN u32 dist_symbol(u32 dist) {                                              // 1..32768 -> 0..29
    const u32 x = dist - 1;
    if (x < 4) return x;
    const u32 msb = floor_log2(x);
    return 2 * msb + ((x >> (msb - 1)) & 1);
}
struct Code { u32 sym, eb, ev; };                                                  // symbol, number of extra bits, extra value
// (a symbol's base is a multiple of 2^eb above 3 -- or 1 for a distance --, so the extra value is the low eb bits)
MGX_DF_FN Code length_code(u32 length) { const u32 s = length_symbol(length), eb = length_extra_bits(s); return Code{s, eb, (length - 3) & ((1u << eb) - 1)}; }
MGX_DF_FN Code dist_code(u32 dist) { const u32 s = dist_symbol(dist), eb = dist_extra_bits(s); return Code{s, eb, (dist - 1) & ((1u << eb) - 1)}; }

// ---- a token in 32 bits: bits 0..8 literal/length symbol (kTokNone: no token), 9..13 the length's extra value, 14..18 the
// distance symbol, 19..31 the distance's extra value.  A literal is its byte.
constexpr u32 kTokNone = 0x1FFu;
MGX_DF_FN u32 token_pack(u32 ls, u32 lev, u32 ds, u32 dev) { return ls | lev << 9 | ds << 14 | dev << 19; }
MGX_DF_FN u32 token_match(u32 length, u32 dist) { const Code l = length_code(length), d = dist_code(dist); return token_pack(l.sym, l.ev, d.sym, d.ev); }
MGX_DF_FN u32 tok_symbol(u32 t) { return t & 0x1FFu; }
MGX_DF_FN u32 tok_length_extra(u32 t) { return (t >> 9) & 31u; }
MGX_DF_FN u32 tok_dist_symbol(u32 t) { return (t >> 14) & 31u; }
MGX_DF_FN u32 tok_dist_extra(u32 t) { return t >> 19; }
MGX_DF_FN bool tok_is_match(u32 t) { return tok_symbol(t) > kEndOfBlock; }         // (not for kTokNone)
MGX_DF_FN u32 token_bits(u32 t, const u8* l_ll, const u8* l_d) {
    const u32 ls = tok_symbol(t);
    if (ls == kTokNone) return 0;
    u32 nb = l_ll[ls];
    if (ls > kEndOfBlock) { const u32 ds = tok_dist_symbol(t); nb += length_extra_bits(ls) + l_d[ds] + dist_extra_bits(ds); }
    return nb;
}

// ---- match search
MGX_DF_FN u32 hash4(u32 four_bytes) { return (four_bytes * 2654435761u) >> (32 - kHashBits); }
// What the literals cost that a match of at most 16 bytes replaces, in 1/16 bit, from the prices of its first four bytes (three
// for a 3-byte match), and the rule itself: the match is dropped unless its estimated bits -- cost_rle at distance 1, else
// cost_base, plus the distance's extra bits -- are fewer.
MGX_DF_FN u32 short_match_literal_cost(u32 len, u32 c0, u32 c1, u32 c2, u32 c3) { const u32 lit = c0 + c1 + c2; return len == 3 ? lit : (lit + c3) * len >> 2; }
MGX_DF_FN bool short_match_loses(u32 dist, u32 literal_cost, u32 cost_base, u32 cost_rle) {
    return 16u * ((dist == 1 ? cost_rle : cost_base) + dist_extra_bits(dist_symbol(dist))) >= literal_cost;
}

// ---- the counts per length of an over-deep code, and canonical code values
// A code deeper than `limit` (rare: the counts must grow like Fibonacci numbers) is repaired on the counts per length, as in
// zlib's gen_bitlen.  Lifting the deeper leaves to the limit over-subscribes the code by `over` units of 2^-limit; a step
// takes one unit back: the deepest leaf short of the limit goes one level down and a leaf from the limit becomes its
// brother.  The code stays complete and as deep as the limit; the lengths go to the symbols by rank, longest to rarest.
// sorted[0, n): the used symbols, rarest first; len[symbol]: depths in, lengths out; bl_count[16]: scratch in, counts out.
MGX_DF_FN void limit_lengths(u32* bl_count, const u16* sorted, const int n, const int limit, u8* len) {
    for (int b = 0; b < 16; ++b) bl_count[b] = 0;
    for (int r = 0; r < n; ++r) { const int d = len[sorted[r]]; ++bl_count[d < limit ? d : limit]; }
    u32 over = 0;
    for (int b = 1; b <= limit; ++b) over += bl_count[b] << (limit - b);
    for (over -= 1u << limit; over; --over) {
        int b = limit - 1;
        while (b > 1 && bl_count[b] == 0) --b;
        --bl_count[b]; bl_count[b + 1] += 2; --bl_count[limit];
    }
    int r = 0;
    for (int b = limit; b >= 1; --b) for (u32 k = bl_count[b]; k; --k) len[sorted[r++]] = (u8)b;
}
// the first code of every length (RFC 1951 3.2.2, step 2); bl_count[0] is cleared
MGX_DF_FN void canonical_next_code(u32* bl_count, u32* next_code) {
    u32 c = 0;
    next_code[0] = 0;
    bl_count[0] = 0;
    for (int bits = 1; bits <= 15; ++bits) { c = (c + bl_count[bits - 1]) << 1; next_code[bits] = c; }
}
MGX_DF_FN u32 reverse_code(u32 c, u32 len) {                                       // a code is sent from its most significant bit; len >= 1
#if defined(__clang__)
    return __builtin_bitreverse32(c) >> (32 - len);
#else
    u32 r = 0;
    for (u32 i = 0; i < len; ++i) r |= ((c >> i) & 1u) << (len - 1 - i);
    return r;
#endif
}

// ---- the header's code-length symbols (RFC 1951 3.2.7) of a run of `run` equal code lengths of value v: zeros as 18
// (11-138, here 138 at a time), 17 (3-10) or single zeros; another value once, then 16 (repeat 3-6, here 6 at a time) or singles
MGX_DF_FN u32 cl_extra_bits(u32 sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }
MGX_DF_FN u32 run_symbol_count(u32 v, u32 run) {
    if (v == 0) { const u32 rem = run % 138; return run / 138 + (rem >= 3 ? 1u : rem); }
    const u32 rem = (run - 1) % 6;
    return 1 + (run - 1) / 6 + (rem >= 3 ? 1u : rem);
}
template <typename Emit>
MGX_DF_FN void run_symbols(u32 v, u32 run, Emit emit) {                            // emit(symbol, extra value)
    if (v == 0) {
        u32 r = run;
        for (; r >= 138; r -= 138) emit(18, 127);
        if (r >= 11) emit(18, r - 11); else if (r >= 3) emit(17, r - 3); else for (; r; --r) emit(0, 0);
    } else {
        emit(v, 0);
        u32 r = run - 1;
        for (; r >= 6; r -= 6) emit(16, 3);
        if (r >= 3) emit(16, r - 3); else for (; r; --r) emit(v, 0);
    }
}
MGX_DF_FN u32 cl_order(u32 i) {                                                    // the order in which the header lists the code-length code
    const u8 order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// ---- LSB-first bit writer into 32-bit words that other writers share: Store::or_word is a plain OR on the host and an atomic
// OR in the kernel
struct PlainOr { static MGX_DF_FN void or_word(u32* w, u32 v) { *w |= v; } };
template <typename Store>
struct BitSink {
    u32* words; u32 word; u64 acc; u32 nbits;
    MGX_DF_FN void start(u32* w, u32 bitpos) { words = w; word = bitpos >> 5; acc = 0; nbits = bitpos & 31; }
    MGX_DF_FN void put(u32 v, u32 nb) {
        acc |= (u64)v << nbits;
        nbits += nb;
        if (nbits >= 32) { Store::or_word(&words[word++], (u32)acc); acc >>= 32; nbits -= 32; }
    }
    MGX_DF_FN u32 position() const { return word * 32 + nbits; }
    MGX_DF_FN void finish() { if (nbits) Store::or_word(&words[word], (u32)acc); }
};
// BFINAL = 1, BTYPE = 10 (dynamic), HLIT, HDIST, HCLEN and the code-length code's lengths (trailing zeros of the order trimmed)
template <typename Sink>
MGX_DF_FN void put_dynamic_header_start(Sink& s, u32 nlit, u32 ndist, const u8* l_cl) {
    u32 ncl = 19;
    while (ncl > 4 && l_cl[cl_order(ncl - 1)] == 0) --ncl;
    s.put(1u | 2u << 1, 3);
    s.put(nlit - 257, 5); s.put(ndist - 1, 5); s.put(ncl - 4, 4);
    for (u32 i = 0; i < ncl; ++i) s.put(l_cl[cl_order(i)], 3);
}
template <typename Sink>
MGX_DF_FN void put_cl_symbol(Sink& s, u32 sym, u32 extra, const u16* c_cl, const u8* l_cl) {
    s.put(c_cl[sym], l_cl[sym]);
    if (sym >= 16) s.put(extra, cl_extra_bits(sym));
}
template <typename Sink>
MGX_DF_FN void put_token(Sink& s, u32 t, const u16* c_ll, const u8* l_ll, const u16* c_d, const u8* l_d) {
    const u32 ls = tok_symbol(t);
    s.put(c_ll[ls], l_ll[ls]);
    if (ls > kEndOfBlock) {
        const u32 ds = tok_dist_symbol(t), leb = length_extra_bits(ls), deb = dist_extra_bits(ds);
        if (leb) s.put(tok_length_extra(t), leb);
        s.put(c_d[ds], l_d[ds]);
        if (deb) s.put(tok_dist_extra(t), deb);
    }
}

// ---- stored or dynamic, and the bytes around the payload
// a dynamic payload that is no shorter than the stored form (5 bytes + the input), or an empty block, is emitted stored
MGX_DF_FN bool emit_stored(u32 dynamic_payload, u32 n) { return dynamic_payload >= n + 5 || n == 0; }
constexpr u32 kStoredHeader = 5, kMemberHeader = 18, kMemberFooter = 8;
MGX_DF_FN void write_stored_header(u8* pay, u32 n) {                               // BFINAL = 1, BTYPE = 00, LEN, NLEN
    pay[0] = 1; pay[1] = (u8)(n & 0xff); pay[2] = (u8)(n >> 8); pay[3] = (u8)(~n & 0xff); pay[4] = (u8)((~n >> 8) & 0xff);
}
// the 18-byte BGZF header (gzip with the BC extra field: BSIZE = member size - 1) and the footer (CRC-32, ISIZE) around a payload
// of `payload` bytes at member + 18; returns the member's size
MGX_DF_FN u32 write_member_frame(u8* member, u32 payload, u32 crc, u32 n) {
    const u32 total = kMemberHeader + payload + kMemberFooter;
    const u8 head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) member[i] = head[i];
    member[16] = (u8)((total - 1) & 0xff); member[17] = (u8)((total - 1) >> 8);
    u8* f = member + kMemberHeader + payload;
    for (int i = 0; i < 4; ++i) { f[i] = (u8)(crc >> (8 * i)); f[4 + i] = (u8)(n >> (8 * i)); }
    return total;
}

// ---- CRC-32 (reflected: bit 31 = x^0) of a block cut into chunks of 64 bytes whose CRCs are combined by multiplication modulo
// the CRC polynomial
constexpr u32 kCrcPoly = 0xEDB88320u, kCrcChunk = 64;
constexpr u32 kX0 = 0x80000000u, kX1 = 0x40000000u;                                // the polynomials 1 and x
MGX_DF_FN u32 multmodp(u32 a, u32 b) {
    u32 p = 0;
#if defined(__HIPCC__)
#pragma unroll 4
#endif
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// slicing-by-4 tables: tab[0][i] from the polynomial, tab[k][i] from tab[k - 1][i] and tab[0]
MGX_DF_FN u32 crc_table0(u32 i) { u32 c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1; return c; }
MGX_DF_FN u32 crc_table_next(u32 prev, const u32* tab0) { return (prev >> 8) ^ tab0[prev & 0xffu]; }
MGX_DF_FN u32 crc_word(u32 c, u32 four_bytes, const u32* tab) {                    // tab: the four tables back to back
    const u32 x = c ^ four_bytes;
    return tab[768 + (x & 0xffu)] ^ tab[512 + ((x >> 8) & 0xffu)] ^ tab[256 + ((x >> 16) & 0xffu)] ^ tab[x >> 24];
}
MGX_DF_FN u32 crc_byte(u32 c, u32 byte, const u32* tab) { return tab[(c ^ byte) & 0xffu] ^ (c >> 8); }
// x2n[k] = x^(2^k), k < 32: x2n[0] = kX1, x2n[k] = multmodp(x2n[k - 1], x2n[k - 1]).  From them x^(512 j), j < 1024 (what shifts a
// chunk's CRC over j later chunks) and x^(8 r), r <= 64 (over the last, shorter chunk)
MGX_DF_FN u32 x_pow_512(u32 j, const u32* x2n) { u32 p = kX0; for (int k = 0; k < 10; ++k) if ((j >> k) & 1u) p = multmodp(x2n[9 + k], p); return p; }
MGX_DF_FN u32 x_pow_8(u32 r, const u32* x2n) { u32 p = kX0; const u32 e = 8u * r; for (int k = 0; k < 10; ++k) if ((e >> k) & 1u) p = multmodp(x2n[k], p); return p; }
MGX_DF_FN u32 crc_chunks(u32 n) { return (n + kCrcChunk - 1) / kCrcChunk; }
MGX_DF_FN u32 crc_last_chunk_bytes(u32 n) { const u32 nc = crc_chunks(n); return nc ? n - kCrcChunk * (nc - 1u) : 0u; }
MGX_DF_FN u32 crc_chunk_start(u32 chunk) { return chunk == 0 ? 0xFFFFFFFFu : 0u; }  // the register a chunk's CRC starts from
// Chunks 0 .. nc-2 are followed by r + 64 (nc - 2 - t) bytes (r = size of the last chunk): one multiplication by the table's power
// per chunk, the common factor x^(8 r) once over their XOR; the last chunk's register as it is (an empty block: chunk 0's).
MGX_DF_FN u32 crc_shifted_chunk(u32 chunk_crc, u32 chunk, u32 nc, const u32* tpow) { return chunk + 2u <= nc ? multmodp(tpow[nc - 2u - chunk], chunk_crc) : 0u; }
MGX_DF_FN bool crc_is_last_chunk(u32 chunk, u32 nc) { return chunk + 1u == (nc ? nc : 1u); }
MGX_DF_FN u32 crc_finish(u32 xor_of_shifted, u32 last_chunk_crc, u32 n, const u32* xr) {
    return multmodp(xr[crc_last_chunk_bytes(n)], xor_of_shifted) ^ last_chunk_crc ^ 0xFFFFFFFFu;
}
// the CRC-32 of n bytes from chunk_crc[max(1, crc_chunks(n))], each chunk's register started from crc_chunk_start
MGX_DF_FN u32 crc_combine(const u32* chunk_crc, u32 n, const u32* tpow, const u32* xr) {
    const u32 nc = crc_chunks(n);
    u32 x = 0;
    for (u32 t = 0; t + 2u <= nc; ++t) x ^= crc_shifted_chunk(chunk_crc[t], t, nc, tpow);
    return crc_finish(x, chunk_crc[nc ? nc - 1 : 0], n, xr);
}

}  // namespace mgx_deflate
