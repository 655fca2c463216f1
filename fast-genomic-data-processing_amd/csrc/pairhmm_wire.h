// pairhmm_wire.h -- the bit-packed wire form of a PairHMM batch: what crosses PCIe when a context or a queue is
// created with MGX_PAIRHMM_WIRE, and what the device kernel pairhmm_expand_wire (mgx_pairhmm.hip) turns back into
// the byte arrays the PairHMM kernels read.  Pure host code: libc and libstdc++ only, no HIP, so that a stand-alone
// program can run it under the sanitizers (tests/cpp/pairhmm_wire_driver.cpp).
//
// A batch on the wire is the packer's batch (pairhmm_pack.h: local indices, every referenced read and haplotype
// once, first-use order) with the six byte arrays replaced by
//   bases4, hap4     4-bit codes, two positions per byte: position p in byte p / 2, low nibble for even p.  The
//                    code is the kernels' numbering (base_code): A 0, C 1, T 2, G 3, N 4, any other byte 0;
//                    expansion writes "ACTGN"[code].
//   qual, ins, del   the values byte & 127 as a little-endian bit stream over the concatenated reads: position p
//                    occupies bits [p w, p w + w), bit b being bit b % 8 of byte b / 8, so eight positions are
//                    exactly w bytes.  w is chosen per array and per batch: 6 when every masked value of the
//                    array is at most 63, otherwise 7.
//   gcp              w = 0 when every masked byte of the batch is one value, kept in gcp_const (the reference's
//                    gap-continuation penalty is one constant, PairHMMLikelihoodCalculationEngine.cpp:284-292);
//                    otherwise packed like the others.
// The last partial group of eight (the last odd nibble) is zero-filled, and an expander never reads past
// ceil(n / 8) * w (ceil(n / 2)) bytes of a packed array.
//
// Why nothing changes: the expanded arrays are canonical, not the caller's bytes -- qualities are masked with 127
// and bases folded to the five letters.  The kernels apply the same mask and the same fold to every byte they load
// (pairhmm_kernels.hip.inc:301-302: `a.ins[o] & 127`, `a.del[o] & 127`, `a.gcp[o] & 127`, `a.qual[o] & 127`, and
// :266, :409, :421 for the plain form's test and the strip boundaries; :85-93 base_code and :99-107 base_code4 for
// read and haplotype bases), and mask and fold are idempotent: (b & 127) & 127 == b & 127, and
// base_code("ACTGN"[base_code(b)]) == base_code(b).  So every value the recurrence is built from is the same
// bit pattern as without the wire form, and with them every likelihood and every used_f64 flag.
//
// Sizes (A(x) = x rounded up to 256, rb / hb = read / haplotype bases of the batch, n test cases, nr / nh sequences):
//   packed array lengths   bases4 ceil(rb / 2), hap4 ceil(hb / 2), qual / ins / del / gcp ceil(rb / 8) * w
//   mgx_pairhmm_pack_batch_wire's buffer (tight: nothing is padded, so a heap block of `need` bytes ends where hap4 ends)
//       need = 8 (nr + 1) + 8 (nh + 1) + 8 n + ceil(rb / 2) + ceil(rb / 8) (w_qual + w_ins + w_del + w_gcp) + ceil(hb / 2)
//   what a batch uploads (the slab prefix [jobs | bases4 | qual | ins | del | gcp | hap4], every part aligned)
//       A(32 n) + A(ceil(rb / 2)) + A(ceil(rb / 8) w_qual) + A(.. w_ins) + A(.. w_del) + A(.. w_gcp) + A(ceil(hb / 2))
//     against A(32 n) + 5 A(rb) + A(hb) of the plain form: for independent 128 x 256 test cases with qualities up to
//     63 and a constant gcp, 64 + 3 * 96 + 128 + 32 = 512 bytes per test case instead of 928, plus the padding of the
//     seven parts (less than 7 * 256 bytes per batch; none when n is a multiple of 8).
#pragma once

#include <cstdint>
#include <cstring>

#include "pairhmm_pack.h"

namespace mgx {
namespace wire {

constexpr uint64_t kLetters = 0x0000004E47544341ull;      // "ACTGN" and three zero bytes: letter of code c is byte c & 7

inline uint8_t code_of(uint8_t b) { return b == 'C' ? 1 : b == 'T' ? 2 : b == 'G' ? 3 : b == 'N' ? 4 : 0; }
inline uint8_t letter_of(unsigned code) { return (uint8_t)(kLetters >> (8 * (code & 7u))); }

inline uint64_t nibble_bytes(uint64_t n) { return (n + 1) / 2; }
inline uint64_t stream_bytes(uint64_t n, unsigned w) { return (n + 7) / 8 * w; }

// two bases -> one byte of codes, indexed by the two bytes as a little-endian 16-bit word (64 KiB, of which real
// data touches the 25 entries of "ACGTN" x "ACGTN")
inline const uint8_t* pair_table() {
    static const struct Table {
        uint8_t t[65536];
        Table() { for (unsigned hi = 0; hi < 256; ++hi) for (unsigned lo = 0; lo < 256; ++lo) t[hi << 8 | lo] = (uint8_t)(code_of((uint8_t)lo) | code_of((uint8_t)hi) << 4); }
    } table;
    return table.t;
}

// Appends base codes to a nibble stream; the stream runs on across the sequences it is fed.
struct NibblePacker {
    uint8_t* dst;
    uint64_t n = 0;              // positions written so far
    explicit NibblePacker(uint8_t* d) : dst(d) {}
    void append(const uint8_t* s, uint64_t len) {
        if (len == 0) return;
        uint64_t i = 0;
        if (n & 1) { dst[n >> 1] |= (uint8_t)(code_of(s[0]) << 4); i = 1; }      // completes the byte the last sequence left half full
        const uint8_t* t = pair_table();
        uint8_t* o = dst + ((n + 1) >> 1);
        n += len;
        for (; i + 8 <= len; i += 8, o += 4) {          // 8 bytes in, 4 bytes out
            uint16_t p0, p1, p2, p3;
            memcpy(&p0, s + i, 2); memcpy(&p1, s + i + 2, 2); memcpy(&p2, s + i + 4, 2); memcpy(&p3, s + i + 6, 2);
            o[0] = t[p0]; o[1] = t[p1]; o[2] = t[p2]; o[3] = t[p3];
        }
        for (; i + 2 <= len; i += 2) *o++ = (uint8_t)(code_of(s[i]) | code_of(s[i + 1]) << 4);
        if (i < len) *o = code_of(s[i]);                // high nibble zero: the zero fill, or completed by the next sequence
    }
};

// eight masked bytes (one per byte of x) -> 8 W bits
template <int W>
constexpr uint64_t squeeze8(uint64_t x) {
    static_assert(W == 6 || W == 7, "field width");
    if (W == 7) {
        x &= 0x7F7F7F7F7F7F7F7Full;
        x = (x & 0x007F007F007F007Full) | ((x & 0x7F007F007F007F00ull) >> 1);
        x = (x & 0x00003FFF00003FFFull) | ((x & 0x3FFF00003FFF0000ull) >> 2);
        x = (x & 0x000000000FFFFFFFull) | ((x & 0x0FFFFFFF00000000ull) >> 4);
    } else {
        x &= 0x3F3F3F3F3F3F3F3Full;
        x = (x & 0x003F003F003F003Full) | ((x & 0x3F003F003F003F00ull) >> 2);
        x = (x & 0x00000FFF00000FFFull) | ((x & 0x0FFF00000FFF0000ull) >> 4);
        x = (x & 0x0000000000FFFFFFull) | ((x & 0x00FFFFFF00000000ull) >> 8);
    }
    return x;
}
// ... and back: 8 W bits -> eight bytes
template <int W>
constexpr uint64_t spread8(uint64_t x) {
    static_assert(W == 6 || W == 7, "field width");
    if (W == 7) {
        x = (x & 0x000000000FFFFFFFull) | ((x << 4) & 0x0FFFFFFF00000000ull);
        x = (x & 0x00003FFF00003FFFull) | ((x << 2) & 0x3FFF00003FFF0000ull);
        x = (x & 0x007F007F007F007Full) | ((x << 1) & 0x7F007F007F007F00ull);
    } else {
        x = (x & 0x0000000000FFFFFFull) | ((x << 8) & 0x00FFFFFF00000000ull);
        x = (x & 0x00000FFF00000FFFull) | ((x << 4) & 0x0FFF00000FFF0000ull);
        x = (x & 0x003F003F003F003Full) | ((x << 2) & 0x3F003F003F003F00ull);
    }
    return x;
}

// Appends values byte & 127 to a W-bit little-endian bit stream that runs on across the sequences it is fed.
// Fewer than 8 bits are ever pending, so eight new fields (at most 56 bits) fit the 64-bit accumulator whatever the
// phase: the fast path takes 8 bytes in and puts W bytes out per step at every bit phase.
template <int W>
struct BitPacker {
    uint8_t* dst;                // next byte to write
    uint64_t acc = 0;            // pending bits, low first
    unsigned pending = 0;        // how many: < 8
    explicit BitPacker(uint8_t* d) : dst(d) {}
    void append(const uint8_t* s, uint64_t len) {
        uint64_t i = 0;
        for (; i + 8 <= len; i += 8) {
            uint64_t x;
            memcpy(&x, s + i, 8);
            acc |= squeeze8<W>(x) << pending;
            memcpy(dst, &acc, W);                       // W whole bytes are complete (little-endian host)
            dst += W;
            acc >>= 8 * W;
        }
        for (; i < len; ++i) {
            acc |= (uint64_t)(s[i] & ((1u << W) - 1u) & 127u) << pending;
            pending += W;
            if (pending >= 8) { *dst++ = (uint8_t)acc; acc >>= 8; pending -= 8; }
        }
    }
    // the pending bits and the zero fill of the last group: `n` positions have been appended in all
    void finish(uint64_t n) {
        uint8_t* const end = dst - (n * W) / 8 + stream_bytes(n, W);
        while (dst < end) { *dst++ = (uint8_t)acc; acc >>= 8; }
        pending = 0;
    }
};

// Widths of one batch.
struct Widths { uint8_t qual = 6, ins = 6, del = 6, gcp = 0, gcp_const = 0; };

// OR of the masked bytes of [s, s + len) into *all, OR of their differences from `first` into *diff
inline void scan_or(const uint8_t* s, uint64_t len, uint8_t* all) {
    uint8_t a = 0;
    for (uint64_t i = 0; i < len; ++i) a |= s[i];
    *all |= a;
}
inline void scan_or_diff(const uint8_t* s, uint64_t len, uint8_t first, uint8_t* all, uint8_t* diff) {
    uint8_t a = 0, d = 0;
    for (uint64_t i = 0; i < len; ++i) { a |= s[i]; d |= (uint8_t)(s[i] ^ first); }
    *all |= a; *diff |= d;
}
// an OR has bit 6 set exactly when one of the values has: every masked value <= 63 <=> (OR & 64) == 0
inline uint8_t width_of(uint8_t all) { return (all & 64) ? 7 : 6; }

// The sequences of a batch as runs of neighbours in the source arrays, as pack_copy walks them: fn(src, len) per
// run of reads (read = true) or haplotypes, in the batch's order.  plan == nullptr: the arrays of `in` as they are.
template <typename Fn>
inline void for_each_run(const mgx_pairhmm_input_t* in, const PackPlan* plan, bool read, Fn fn) {
    const uint64_t* off = read ? in->read_off : in->hap_off;
    if (!plan) {
        const uint64_t n = read ? in->n_reads : in->n_haps;
        if (n) fn((uint64_t)0, off[n]);                 // a plain batch copies [0, off[n]) and keeps the caller's offsets
        return;
    }
    const std::vector<uint64_t>& l = read ? plan->lread : plan->lhap;
    for (size_t a = 0; a < l.size();) {
        size_t b = a + 1;
        while (b < l.size() && l[b] == l[b - 1] + 1) ++b;
        fn(off[l[a]], off[l[b - 1] + 1] - off[l[a]]);
        a = b;
    }
}

// The pre-pass: one read of the four quality arrays of the batch's reads.
inline Widths scan_widths(const mgx_pairhmm_input_t* in, const PackPlan* plan) {
    uint8_t q = 0, i = 0, d = 0, g = 0, gdiff = 0, first = 0;
    bool any = false;
    for_each_run(in, plan, true, [&](uint64_t src, uint64_t len) {
        if (!len) return;
        if (!any) { first = in->gcp[src]; any = true; }
        scan_or(in->qual + src, len, &q); scan_or(in->ins + src, len, &i); scan_or(in->del + src, len, &d);
        scan_or_diff(in->gcp + src, len, first, &g, &gdiff);
    });
    Widths w;
    w.qual = width_of(q); w.ins = width_of(i); w.del = width_of(d);
    if ((gdiff & 127) == 0) { w.gcp = 0; w.gcp_const = (uint8_t)(first & 127); }       // constant after the mask
    else w.gcp = width_of(g);
    return w;
}

// one quality array of the batch -> its bit stream (w = 6 or 7) at dst, stream_bytes(n, w) bytes
inline void pack_stream(const mgx_pairhmm_input_t* in, const PackPlan* plan, const uint8_t* src, unsigned w, uint8_t* dst) {
    uint64_t n = 0;
    if (w == 7) {
        BitPacker<7> p(dst);
        for_each_run(in, plan, true, [&](uint64_t s, uint64_t len) { p.append(src + s, len); n += len; });
        p.finish(n);
    } else {
        BitPacker<6> p(dst);
        for_each_run(in, plan, true, [&](uint64_t s, uint64_t len) { p.append(src + s, len); n += len; });
        p.finish(n);
    }
}
// read bases or haplotype bases -> nibble codes at dst, nibble_bytes(n) bytes
inline void pack_nibbles(const mgx_pairhmm_input_t* in, const PackPlan* plan, bool read, uint8_t* dst) {
    NibblePacker p(dst);
    const uint8_t* src = read ? in->bases : in->hap_bases;
    for_each_run(in, plan, read, [&](uint64_t s, uint64_t len) { p.append(src + s, len); });
}

// The six arrays of a batch into their wire form, straight from the caller's arrays: pack_copy's job, bit-packing.
// Every destination holds exactly its packed length (sizes above); gcp is not touched when w.gcp == 0.
inline void pack_arrays(const mgx_pairhmm_input_t* in, const PackPlan* plan, const Widths& w, uint8_t* bases4, uint8_t* qual,
                        uint8_t* ins, uint8_t* del, uint8_t* gcp, uint8_t* hap4) {
    pack_nibbles(in, plan, true, bases4);
    pack_stream(in, plan, in->qual, w.qual, qual);
    pack_stream(in, plan, in->ins, w.ins, ins);
    pack_stream(in, plan, in->del, w.del, del);
    if (w.gcp) pack_stream(in, plan, in->gcp, w.gcp, gcp);
    pack_nibbles(in, plan, false, hap4);
}

// ---- the reference expander: position by position, written for the eye; the device kernel is tested against it
inline void expand_nibbles(const uint8_t* src, uint64_t n, uint8_t* dst) {
    for (uint64_t p = 0; p < n; ++p) dst[p] = letter_of((unsigned)(src[p >> 1] >> (4 * (p & 1))) & 15u);
}
inline void expand_stream(const uint8_t* src, uint64_t n, unsigned w, uint8_t* dst) {
    for (uint64_t p = 0; p < n; ++p) {
        unsigned v = 0;
        for (unsigned k = 0; k < w; ++k) {
            const uint64_t b = p * w + k;
            v |= (unsigned)((src[b >> 3] >> (b & 7)) & 1u) << k;
        }
        dst[p] = (uint8_t)v;
    }
}
inline void expand(const mgx_pairhmm_wire_t* wv, uint8_t* bases, uint8_t* qual, uint8_t* ins, uint8_t* del, uint8_t* gcp, uint8_t* hap) {
    const uint64_t rb = wv->n_reads ? wv->read_off[wv->n_reads] : 0, hb = wv->n_haps ? wv->hap_off[wv->n_haps] : 0;
    expand_nibbles(wv->bases4, rb, bases);
    expand_stream(wv->qual, rb, wv->w_qual, qual);
    expand_stream(wv->ins, rb, wv->w_ins, ins);
    expand_stream(wv->del, rb, wv->w_del, del);
    if (wv->w_gcp) expand_stream(wv->gcp, rb, wv->w_gcp, gcp);
    else if (rb) memset(gcp, wv->gcp_const, rb);
    expand_nibbles(wv->hap4, hb, hap);
}

// Where the arrays of a planned batch lie in mgx_pairhmm_pack_batch_wire's buffer, and its size (the closed form above).
struct BufferLayout { size_t roff, hoff, pr, ph, bases4, qual, ins, del, gcp, hap4, need; };
inline BufferLayout buffer_layout(uint64_t nr, uint64_t nh, uint64_t n, uint64_t rb, uint64_t hb, const Widths& w) {
    BufferLayout L;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += bytes; return at; };
    L.roff = take((nr + 1) * 8); L.hoff = take((nh + 1) * 8);
    L.pr = take(n * 4); L.ph = take(n * 4);
    L.bases4 = take(nibble_bytes(rb));
    L.qual = take(stream_bytes(rb, w.qual)); L.ins = take(stream_bytes(rb, w.ins)); L.del = take(stream_bytes(rb, w.del));
    L.gcp = take(stream_bytes(rb, w.gcp));
    L.hap4 = take(nibble_bytes(hb));
    L.need = off;
    return L;
}

// Test cases of `plan` as a wire batch in buf (L.need bytes); *out points into buf.
inline void pack_batch(const mgx_pairhmm_input_t* in, const PackPlan& plan, const Widths& w, const BufferLayout& L, uint8_t* buf,
                       mgx_pairhmm_wire_t* out) {
    const uint64_t n = plan.hi - plan.lo, nr = plan.lread.size(), nh = plan.lhap.size();
    memcpy(buf + L.roff, plan.roff.data(), (nr + 1) * 8); memcpy(buf + L.hoff, plan.hoff.data(), (nh + 1) * 8);
    if (n) { memcpy(buf + L.pr, plan.pair_read.data(), n * 4); memcpy(buf + L.ph, plan.pair_hap.data(), n * 4); }
    pack_arrays(in, &plan, w, buf + L.bases4, buf + L.qual, buf + L.ins, buf + L.del, buf + L.gcp, buf + L.hap4);
    mgx_pairhmm_wire_t o{};
    o.n_reads = nr; o.n_haps = nh; o.n_pairs = n;
    o.read_off = (const uint64_t*)(buf + L.roff); o.hap_off = (const uint64_t*)(buf + L.hoff);
    o.pair_read = (const uint32_t*)(buf + L.pr); o.pair_hap = (const uint32_t*)(buf + L.ph);
    o.w_qual = w.qual; o.w_ins = w.ins; o.w_del = w.del; o.w_gcp = w.gcp; o.gcp_const = w.gcp_const;
    o.bases4 = buf + L.bases4; o.qual = buf + L.qual; o.ins = buf + L.ins; o.del = buf + L.del; o.gcp = buf + L.gcp; o.hap4 = buf + L.hap4;
    *out = o;
}

}  // namespace wire
}  // namespace mgx
