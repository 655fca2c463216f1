// activity_rule.h -- Mutect2Engine::isActive per locus (M2/Mutect2Engine.cpp:58-150), stated once for the kernels of mgx_activity.hip and
// for the CPU tests (tests/cpp/activity_rule_driver.cpp, tests/test_activity_host.py, ASan + UBSan).  No HIP, no heap, no environment.
//
// Rule 1, the read's element at a locus: one byte, 0 = in the pileup and not alt, 1..127 = the alt quality (an alt quality is never 0).
//   The reference builds a PositionToCigarMap per read (samtools/SAMRecord.cpp:557-584): one entry per CIGAR element up to the last one
//   that consumes reference, keyed by the reference position (relative to the read's start) at which the element was reached.  PeUtils
//   (utils/PeUtils.cpp:44-60) takes the last entry whose key is <= pos - start.  Entries of elements that consume no reference (I S H P)
//   share their key with their successor and are never taken; so the element at a locus is the reference-consuming element whose span
//   holds it, `currentStart` is where that span begins and `offset` is the read offset of the element's first base plus the distance into
//   it.  For a skip (N) the map's offset is the read offset before the element MINUS its length, which may lie in front of the read; the
//   C ABI refuses N.  `locate` finds the element by a serial walk; `ref_len` / `read_len` / `first_end_above` are the pieces of the
//   kernel's search (64 elements, one per lane: an inclusive scan of the reference lengths, then a binary search for the first end above
//   the position, which is reference-consuming because the others repeat their predecessor's end).
//   The cases in the order of altQuals (:91-111), e = the element, `last` = the locus is the element's last base:
//     1. e is D                                  -> indelQual(len e)                                (isDeletion, :125-126)
//     2. last and e + 1 is D                     -> indelQual(len (e + 1))                          (isBeforeDeletionStart: the next on-genome element IS e + 1)
//     3. last and e + 1 is I                     -> indelQual(len (e + 1))                          (isBeforeInsertion: getBetween(1)[0] IS e + 1)
//     4. q > min_q and (last, e + 1 is S, q[offset + 1] > min_q  or  first base, e - 1 is S, q[offset - 1] > min_q) -> indelQual(1)
//     5. base != ref byte and q > min_q          -> q, or min(q, pcr_error_qual / 2) under a mapped mate of a proper pair:
//                                                   mate_start <= pos < mate_start + read length
//   indelQual(n) = min(30 + 10 (n - 1), 127).
// Rule 2, the locus (:58-88, :133-150): nRef = tumour size - nAlt (every read whose window holds the locus counts, deletions included);
//   fTildeRatio = exp(digamma(nRef + 1) - digamma(nAlt + 1)); betaEntropy = (-log10Fact(n + 1) + log10Fact(nAlt) + log10Fact(nRef)) log(10);
//   per alt quality z = (1 - eps) / (1 - eps + eps fTildeRatio), term = z (logOneMinusEps - logEps) + fastBernoulliEntropy(z)
//   (MathUtils.cpp:24-27), summed in the input order of the reads; log-odds = betaEntropy + sum.  Not active: no alt element; log-odds <
//   initial_log_odds; with has_normal && !genotype_germline_sites, normalAltCount > normalSize * 0.3 && normalQualSum > 100.
// The tables (digamma, log10 factorial, per quality eps / logEps / logOneMinusEps) are built on the host: mgx_tables.cpp.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MGX_ACT_FN __host__ __device__ inline
#else
#define MGX_ACT_FN inline
#endif

namespace mgx_activity_rule {

constexpr uint32_t kOpM = 0, kOpI = 1, kOpD = 2, kOpN = 3, kOpS = 4, kOpH = 5, kOpP = 6, kOpEq = 7, kOpX = 8;
constexpr uint16_t kFlagProperPair = 0x2, kFlagMateUnmapped = 0x8;
constexpr double kLn10 = 2.302585092994046;      // std::log(10), MathUtils::log10ToLog

MGX_ACT_FN bool consumes_ref(uint32_t op) { return op == kOpM || op == kOpD || op == kOpN || op == kOpEq || op == kOpX; }      // bam_cigar_type & 2
MGX_ACT_FN bool consumes_read(uint32_t op) { return op == kOpM || op == kOpI || op == kOpS || op == kOpEq || op == kOpX; }     // bam_cigar_type & 1
MGX_ACT_FN uint32_t ref_len(uint32_t el) { return consumes_ref(el & 15) ? el >> 4 : 0u; }
MGX_ACT_FN uint32_t read_len(uint32_t el) { return consumes_read(el & 15) ? el >> 4 : 0u; }
MGX_ACT_FN uint8_t indel_qual(uint32_t n) { const uint64_t q = 30 + 10 * (uint64_t)(n - 1); return (uint8_t)(q < 127 ? q : 127); }

struct Read {
    const uint32_t* cigar; uint32_t n_cigar;
    const uint8_t* bases; const uint8_t* quals; uint32_t n_bases;
    int32_t start, mate_start;
    uint16_t flags;
};
struct ElementParams { int32_t pcr_error_qual, min_base_quality; };
// where a locus lies in a read: element e, which starts `ref_at` reference bases behind the read's start and whose first base is read
// base `read_at` (for D: the next read base)
struct Where { uint32_t e, ref_at, read_at; };

// rel = pos - read start, inside the read's reference span
MGX_ACT_FN Where locate(const uint32_t* cigar, uint32_t n_cigar, uint32_t rel) {
    Where w{0, 0, 0};
    for (; w.e < n_cigar; ++w.e) {
        const uint32_t r = ref_len(cigar[w.e]);
        if (r && rel < w.ref_at + r) break;
        w.ref_at += r; w.read_at += read_len(cigar[w.e]);
    }
    return w;
}

// the first of 64 lanes whose inclusive end lies above rel, 64 if none: end_of(j) is lane j's value, non-decreasing in j
template <class EndOf> MGX_ACT_FN uint32_t first_end_above(EndOf end_of, uint32_t rel) {
    uint32_t lo = 0;                                  // the answer lies in [lo, lo + 64]
    for (uint32_t step = 32; step; step >>= 1)
        if (!(end_of(lo + step - 1) > rel)) lo += step;
    return end_of(lo) > rel ? lo : 64u;
}

MGX_ACT_FN uint8_t element_byte(const Read& rd, const Where& w, int32_t pos, uint8_t ref_byte, const ElementParams& p) {
    const uint32_t rel = (uint32_t)(pos - rd.start);
    const uint32_t el = rd.cigar[w.e], op = el & 15, len = el >> 4;
    const bool last = rel == w.ref_at + len - 1, first = rel == w.ref_at;
    const uint32_t next = w.e + 1 < rd.n_cigar ? rd.cigar[w.e + 1] : 0xFu;            // 0xF: no operator
    if (op == kOpD) return indel_qual(len);
    if (last && ((next & 15) == kOpD || (next & 15) == kOpI)) return indel_qual(next >> 4);
    const uint32_t at = w.read_at + (rel - w.ref_at);
    const int32_t q = rd.quals[at];
    if (q > p.min_base_quality) {
        if (last && (next & 15) == kOpS && rd.quals[at + 1] > p.min_base_quality) return indel_qual(1);
        if (first && w.e > 0 && (rd.cigar[w.e - 1] & 15) == kOpS && rd.quals[at - 1] > p.min_base_quality) return indel_qual(1);
        if (rd.bases[at] != ref_byte) {
            const bool mate = (rd.flags & kFlagProperPair) && !(rd.flags & kFlagMateUnmapped) && rd.mate_start != -1;
            const bool overlaps = mate && rd.mate_start <= pos && (int64_t)pos < (int64_t)rd.mate_start + (int64_t)rd.n_bases;
            const int32_t cap = p.pcr_error_qual / 2;
            return (uint8_t)(overlaps && cap < q ? cap : q);
        }
    }
    return 0;
}

// ---- rule 2 ------------------------------------------------------------------------------------------------------------------------
struct Tables {
    const double* digamma;           // [max_depth + 3]
    const double* log10_factorial;   // [max_depth + 3]
    const double* eps;               // [128] pow(10, q / -10.0)
    const double* log_eps;           // [128] q * PHRED_TO_LOG_ERROR_PROB_FACTOR
    const double* log_one_minus_eps; // [128] log1mexp(log_eps)
};
struct LocusParams { int32_t has_normal, genotype_germline_sites; double initial_log_odds; };
struct Counts { uint32_t tumour, alt, normal, normal_alt, normal_qual_sum; };
struct Locus { double log_odds; uint32_t depth; uint8_t active; };

MGX_ACT_FN void count(Counts& c, uint32_t sample, uint8_t byte) {
    const uint32_t tumour = sample == 0, normal = 1u - tumour, alt = byte != 0;
    c.tumour += tumour; c.alt += tumour & alt;
    c.normal += normal; c.normal_alt += normal & alt; c.normal_qual_sum += normal * byte;
}
MGX_ACT_FN double f_tilde_ratio(const Tables& t, uint32_t n_ref, uint32_t n_alt) { return exp(t.digamma[n_ref + 1] - t.digamma[n_alt + 1]); }
MGX_ACT_FN double beta_entropy(const Tables& t, uint32_t n_ref, uint32_t n_alt) {
    return (-t.log10_factorial[n_ref + n_alt + 1] + t.log10_factorial[n_alt] + t.log10_factorial[n_ref]) * kLn10;
}
MGX_ACT_FN double bernoulli_entropy(double p) {
    const double product = p * (1 - p);
    return product * (11 + 33 * product) / (2 + 20 * product);
}
MGX_ACT_FN double alt_term(const Tables& t, uint8_t q, double f_tilde) {
    const double eps = t.eps[q];
    const double z = (1 - eps) / (1 - eps + eps * f_tilde);
    return z * (t.log_one_minus_eps[q] - t.log_eps[q]) + bernoulli_entropy(z);
}
MGX_ACT_FN uint8_t decide(const Counts& c, double log_odds, const LocusParams& p) {
    if (c.alt == 0 || log_odds < p.initial_log_odds) return 0;
    if (p.has_normal && !p.genotype_germline_sites && c.normal_alt > c.normal * 0.3 && c.normal_qual_sum > 100) return 0;
    return 1;
}

// A locus in two walks over the reads whose window holds it, in input order: count(c, sample, byte) for each; then, where has_sum(c,
// max_depth), sum += alt_term(t, byte, f_tilde_ratio(..)) over the tumour's alt bytes; then locus_of.  max_depth bounds the table
// indices: a deeper locus gives its depth alone.
MGX_ACT_FN bool has_sum(const Counts& c, uint32_t max_depth) { return c.alt != 0 && c.tumour + c.normal <= max_depth; }
MGX_ACT_FN Locus locus_of(const Tables& t, const LocusParams& p, const Counts& c, uint32_t max_depth, double sum) {
    Locus out{NAN, c.tumour + c.normal, 0};
    if (!has_sum(c, max_depth)) return out;
    out.log_odds = beta_entropy(t, c.tumour - c.alt, c.alt) + sum;
    out.active = decide(c, out.log_odds, p);
    return out;
}

}  // namespace mgx_activity_rule
