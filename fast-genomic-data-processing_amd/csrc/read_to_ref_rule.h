// read_to_ref_rule.h -- AlignmentUtils::createReadAlignedToRef behind its aligner call (read/AlignmentUtils.cpp:505-543) on run-length
// elements in BAM encoding (len << 4 | op): consolidateCigar, getConsolidatedPaddedCigar(1000), calcFirstBaseMatchingReferenceInCigar,
// trimCigarByBases, applyCigarToCigar, cleanUpCigar, leftAlignIndel(refIndex = readStartOnHaplotype, readIndex = 0, doNotThrow = true), the
// leading-deletion shift and the hard clips.  No HIP, no heap, no per-call arrays: k_read_to_ref (mgx_realign.hip) runs it wave-uniform,
// tests/cpp/read_to_ref_driver.cpp runs it serially and with the kernel's lane grouping (tests/test_read_to_ref_host.py, CPU, ASan + UBSan).
//
// One streaming merge with two cursors replaces the reference's base-by-base lists:
//   aligner cursor     the aligner's elements without the zero lengths (consolidateCigar; joining equal neighbours changes nothing
//                      in a merge whose output is consolidated anyway)
//   haplotype cursor   the haplotype's elements and then 1000M, trimmed at `offset` as trimCigar(byReference = false) does it: a
//                      read-consuming element keeps what lies at or behind the offset, a D stays iff it starts at or behind it
//   transformer        M = X are one class, I S one class (AlignmentUtils.h:257-268); per pair (AlignmentUtils.cpp:13-70)
//                        (M,M) M both   (M,I) I both   (M,D) D second    (D,M) D both   (D,D) D second   (D,I) nothing, both
//                        (I,*) I first; any other pair has no transformer: the reference throws.  Stops when either side is exhausted.
//   emitter            joins equal neighbours (consolidateCigar), drops the leading D (cleanUpCigar) and keeps in scalars what the
//                      left-alignment needs.  A consolidated list of M, I, D with exactly one I/D not at index 0 is aM b<op> [cM],
//                      so those are: the count of I/D, the first three lengths and element 1's operator.
//   left-alignment     leftAlignSingleIndel (:295-359) on a, b, c: shift s = 1, 2, ... moves one base from a to c (an appended 1M when
//                      nothing follows); a shift is accepted when createIndelString gives the same bytes as for s = 0; b misses in a
//                      row end the loop, and so does s = a, where an accepted shift is cleaned up (0M gone, a leading D gone with it).
//                      The alternative string is never built: byte j of it is read where createIndelString would have copied it from,
//                      and two strings of equal length differ at most in [refIndex(s), refIndex(0) + inserted) -- `whole` compares all.
// Statuses as in include/mgx_realign.h.  UNDEFINED is reported, and nothing is read, where createIndelString (:401-421) would allocate a
// negative length or copy read bases from outside the read, and for an aligner list that is one element of length 0, which
// consolidateCigar keeps and applyCigarToCigar never gets past.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MGX_RTR_FN __host__ __device__ inline
#else
#define MGX_RTR_FN inline
#endif

namespace mgx_to_ref_rule {

constexpr uint8_t kOk = 0, kDropped = 1, kUnchanged = 2, kThrows = 3, kUndefined = 4, kNoRoom = 5;
constexpr uint32_t kOpM = 0, kOpI = 1, kOpD = 2, kOpS = 4, kOpH = 5, kOpEq = 7, kOpX = 8;
constexpr uint32_t kPad = 1000;                       // getConsolidatedPaddedCigar(1000)
constexpr int kClassM = 0, kClassI = 1, kClassD = 2, kNoClass = 3;

MGX_RTR_FN int op_class(uint32_t op) {
    return (op == kOpM || op == kOpEq || op == kOpX) ? kClassM : (op == kOpI || op == kOpS) ? kClassI : op == kOpD ? kClassD : kNoClass;
}

struct Input {
    const uint32_t* sw; uint32_t n_sw; int32_t offset;            // the aligner's elements and its alignment offset on the haplotype;
                                                                  // sw == nullptr: <read_len>M, SWNativeAlignerWrapper's verbatim shortcut
    const uint32_t* hap; uint32_t n_hap; int32_t hap_start;       // Haplotype::getCigar() as it is, getAlignmentStartHapwrtRef
    const uint8_t* ref; uint32_t ref_len;                         // the reference haplotype's bases
    const uint8_t* read; uint32_t read_len;
    int32_t reference_start;
    uint32_t hard_lead, hard_trail;                               // the original read's H lengths, 0 = none
};
struct Result { int32_t start; uint32_t n; uint8_t status; };

MGX_RTR_FN uint32_t sw_count(const Input& in) { return in.sw ? in.n_sw : 1u; }
MGX_RTR_FN uint32_t sw_element(const Input& in, uint32_t i) { return in.sw ? in.sw[i] : (in.read_len << 4 | kOpM); }
// the haplotype's elements followed by the padding
MGX_RTR_FN uint32_t hap_element(const Input& in, uint32_t i) { return i < in.n_hap ? in.hap[i] : (kPad << 4 | kOpM); }

// createIndelString (:370-424) for the list (a - s)M b<op> ...: where its bytes come from, instead of the bytes
struct Alt { int64_t p, q, ins, p2, len; int state; };     // state 0: a string, 1: nullptr, 2: undefined
MGX_RTR_FN Alt indel_string(const Input& in, int64_t r0, bool del, int64_t a, int64_t b, int64_t s) {
    const int64_t total = a - s, ref_len = in.ref_len;
    int64_t bp = b;
    if (total + b > ref_len) bp -= total + b - ref_len;
    const int64_t len = ref_len + (del ? -bp : bp);
    if (len < 0) return Alt{0, 0, 0, 0, 0, 2};
    const int64_t p = r0 + total;
    if (p > len || p > ref_len) return Alt{0, 0, 0, 0, 0, 1};
    int64_t cur = p, p2 = p;
    if (del) p2 += bp;
    else {
        if (bp < 0 || total + bp > (int64_t)in.read_len) return Alt{0, 0, 0, 0, 0, 2};
        cur += bp;
    }
    if (ref_len - p2 > len - cur) return Alt{0, 0, 0, 0, 0, 1};
    if (ref_len - p2 < 0) return Alt{0, 0, 0, 0, 0, 2};
    return Alt{p, total, cur - p, p2, len, 0};
}
MGX_RTR_FN uint8_t alt_byte(const Input& in, const Alt& x, int64_t j) {
    return j < x.p ? in.ref[j] : j < x.p + x.ins ? in.read[x.q + (j - x.p)] : in.ref[x.p2 + (j - x.p - x.ins)];
}

// Any::operator()(lo, hi, pred): is pred(j) true for some j in [lo, hi)?  The only work that lanes may share.
struct SerialAny {
    template <class P> MGX_RTR_FN bool operator()(int64_t lo, int64_t hi, P pred) const {
        for (int64_t j = lo; j < hi; ++j) if (pred(j)) return true;
        return false;
    }
};

// store(k, element): element k of the output row; called for every k in order, later again for the at most three patched ones.
// The caller's functor bounds k by its row (NO_ROOM is decided here, from the count alone).
template <class Store, class Any>
MGX_RTR_FN Result read_to_ref(const Input& in, uint32_t room, Store store, Any any, bool whole = false) {
    if (in.offset == -1) return Result{0, 0, kUnchanged};
    if (sw_count(in) == 1 && (sw_element(in, 0) >> 4) == 0) return Result{0, 0, kUndefined};

    // calcFirstBaseMatchingReferenceInCigar and trimCigarByBases' checks, over the whole padded list
    int64_t pos = 0, ref_at = 0, r0 = -1;
    for (uint32_t i = 0; i <= in.n_hap; ++i) {
        const uint32_t e = hap_element(in, i);
        const int64_t len = e >> 4;
        const int cls = op_class(e & 15);
        if (len == 0) continue;
        if (cls == kClassM) {
            if (r0 < 0 && pos + len > in.offset) r0 = ref_at + (in.offset > pos ? in.offset - pos : 0);
            pos += len; ref_at += len;
        } else if (cls == kClassI) pos += len;
        else if (cls == kClassD) ref_at += len;
        else return Result{0, 0, kThrows};
    }
    if (in.offset < 0 || in.offset > pos - 1) return Result{0, 0, kThrows};

    // applyCigarToCigar, consolidateCigar, cleanUpCigar
    const uint32_t base = in.hard_lead ? 1u : 0u;
    uint32_t i12 = 0, i23 = 0, op12 = 0, op23 = 0;
    int64_t rem12 = 0, rem23 = 0, hpos = 0;
    uint32_t pend_op = 0, k = 0, n_indel = 0, op1 = 0;
    int64_t pend = 0, a = 0, b = 0, c = 0, read_clean = 0;
    auto flush = [&]() {
        if (pend == 0 || (k == 0 && pend_op == kOpD)) { pend = 0; return; }
        if (k == 0) a = pend;
        if (k == 1) { b = pend; op1 = pend_op; }
        if (k == 2) c = pend;
        n_indel += pend_op != kOpM;
        if (pend_op != kOpD) read_clean += pend;
        store(base + k, (uint32_t)pend << 4 | pend_op);
        ++k; pend = 0;
    };
    auto emit = [&](uint32_t op, int64_t len) {
        if (pend && op != pend_op) flush();
        pend_op = op; pend += len;
    };
    for (;;) {
        while (rem12 == 0 && i12 < sw_count(in)) { const uint32_t e = sw_element(in, i12++); rem12 = e >> 4; op12 = e & 15; }
        while (rem23 == 0 && i23 <= in.n_hap) {
            const uint32_t e = hap_element(in, i23++);
            const int64_t len = e >> 4;
            op23 = e & 15;
            if (op23 == kOpD) rem23 = hpos >= in.offset ? len : 0;
            else { const int64_t from = hpos > in.offset ? hpos : in.offset; rem23 = hpos + len > from ? hpos + len - from : 0; hpos += len; }
        }
        if (rem12 == 0 || rem23 == 0) break;
        const int c12 = op_class(op12), c23 = op_class(op23);
        if (c12 == kNoClass) return Result{0, 0, kThrows};
        const int64_t both = rem12 < rem23 ? rem12 : rem23;
        if (c12 == kClassI) { emit(kOpI, rem12); rem12 = 0; }
        else if (c23 == kClassD) { emit(kOpD, rem23); rem23 = 0; }
        else {
            if (c12 == kClassM) emit(c23 == kClassM ? kOpM : kOpI, both);
            else if (c23 == kClassM) emit(kOpD, both);
            rem12 -= both; rem23 -= both;
        }
    }
    flush();

    // leftAlignIndel
    int64_t lead = 0;
    if (n_indel == 1 && op1 != kOpM) {
        const bool del = op1 == kOpD;
        const Alt x0 = indel_string(in, r0, del, a, b, 0);
        if (x0.state == 2) return Result{0, 0, kUndefined};
        int64_t best = 0;
        if (x0.state == 0)
            for (int64_t s = 1, miss = 0; miss < b; ++s) {
                const Alt xs = indel_string(in, r0, del, a, b, s);
                if (xs.state == 2) return Result{0, 0, kUndefined};
                bool equal = xs.state == 0 ? xs.len == x0.len : x0.len == 0;
                if (equal && xs.state == 0) {
                    const int64_t hi = x0.p + x0.ins < x0.len ? x0.p + x0.ins : x0.len;
                    equal = !any(whole ? 0 : xs.p, whole ? x0.len : hi, [&](int64_t j) { return alt_byte(in, x0, j) != alt_byte(in, xs, j); });
                }
                if (equal) { best = s; miss = 0; } else ++miss;
                if (s == a) break;
            }
        if (best == a) {                       // moved to the read's start: cleanUpCigar
            if (del) { lead = b; store(base, (uint32_t)(c + a) << 4 | kOpM); k = 1; }
            else { store(base, (uint32_t)b << 4 | kOpI); store(base + 1, (uint32_t)(c + a) << 4 | kOpM); k = 2; }
        } else if (best) {
            store(base, (uint32_t)(a - best) << 4 | kOpM);
            store(base + 2, (uint32_t)(c + best) << 4 | kOpM);
            k = 3;
        }
    }
    if (read_clean != (int64_t)in.read_len) return Result{0, 0, kThrows};
    if (in.hard_lead) store(0, in.hard_lead << 4 | kOpH);
    if (in.hard_trail) store(base + k, in.hard_trail << 4 | kOpH);
    const uint32_t n = base + k + (in.hard_trail ? 1u : 0u);
    const int32_t start = (int32_t)((int64_t)in.reference_start + in.hap_start + r0 + lead);
    return Result{start, n, n > room ? kNoRoom : kOk};
}

}  // namespace mgx_to_ref_rule
