/*
 * mgx_realign.h -- C ABI of the fused "realign reads to their best haplotype" stage (libmgx.so).
 *
 * What Mutect2Engine runs right after computeReadLikelihoods (M2/Mutect2Engine.cpp:223-231,
 * realignReadsToTheirBestHaplotype), between one upload and the downloads of its results.  Reference
 * interface replaced (paths relative to deepmutect/Mutect2Cpp-master/src/):
 *
 *   mgx_pairhmm_best_alleles  <- AlleleLikelihoods::bestAllelesBreakingTies, i.e. searchBestAllele(sample, r,
 *                                canBeReference = true, priorities) per read
 *                                (utils/genotyper/AlleleLikelihoods.h:92-146), on rows the caller holds
 *   mgx_realign_regions       <- computeReadLikelihoods (mgx_pairhmm_regions), then per read that
 *                                filterPoorlyModeledEvidence keeps: searchBestAllele, and
 *                                AlignmentUtils::createReadAlignedToRef's aligner call
 *                                (read/AlignmentUtils.cpp:498): SWNativeAlignerWrapper::align(haplotype, read,
 *                                parameters, strategy) with its verbatim shortcut
 *                                (smithwaterman/SWNativeAlignerWrapper.cpp:10-31, Mutect2Utils.cpp:69-82)
 *   mgx_read_to_ref           <- createReadAlignedToRef behind its aligner call (read/AlignmentUtils.cpp:505-543) on
 *                                alignments the caller holds: the read's start on the reference and its
 *                                read -> reference CIGAR
 *   mgx_realign_regions_to_ref <- mgx_realign_regions and, per kept read, mgx_read_to_ref on its own results
 *
 * The best-haplotype rule, on v[a] = log10[a] * log(10) (the rounded product, MathUtils.cpp:16-18) with the
 * threshold T = 0.2 * log(10): b0 is the first index that attains max v; the tie-break is entered iff some
 * a != b0 has v[b0] - v[a] < T; its candidates are the a != b0 with !(v[b0] - v[a] > T); c is the first
 * candidate that attains the maximum priority over the candidates; the result is c if priority[c] >
 * priority[b0], otherwise b0.  Values are finite or -inf; a row that is all -inf gives 0.  Only
 * bestAlleleIndex is reproduced (the reference's second-best bookkeeping feeds a commented-out tag).
 * Priorities are the caller's (HAPLOTYPE_ALIGNMENT_TIEBREAKING_PRIORITY,
 * haplotypecaller/AssemblyBasedCallerUtils.cpp:180-187, depends on the haplotype's CIGAR).
 *
 * The read -> reference rule (csrc/read_to_ref_rule.h states it once, for the kernel and for the CPU tests): consolidateCigar of the
 * aligner's CIGAR, getConsolidatedPaddedCigar(1000) of the haplotype's, calcFirstBaseMatchingReferenceInCigar, trimCigarByBases,
 * applyCigarToCigar (M = X one class, I S one class: the aligner's soft clips come out as insertions), cleanUpCigar,
 * leftAlignIndel(refIndex = readStartOnHaplotype, readIndex = 0, doNotThrow = true) against the reference haplotype's bases, the
 * leading-deletion shift of the start, the original read's hard clips around the result and the final read-length check.  What the
 * reference does per read beyond that, the SAMRecord clone with setPosition and setCigar, stays host code in the caller.
 * All functions return 0 or a negative errno-style code with mgx_last_error() set.  No CPU fallback.
 */
#ifndef MGX_REALIGN_H
#define MGX_REALIGN_H

#include <stdint.h>

#include "mgx_pairhmm.h"
#include "mgx_smithwaterman.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_REALIGN_NOT_ALIGNED INT32_MIN   /* out_offset of a read the filter dropped */

typedef struct mgx_realign_stats {
    uint64_t n_reads, n_kept, n_verbatim, n_sw_pairs;   /* of the last mgx_realign_regions call on the context */
    float ms_best, ms_verbatim, ms_gather;    /* HIP events, valid when both contexts time (MGX_PAIRHMM_TIMING) */
} mgx_realign_stats_t;

/* bestAllelesBreakingTies on rows the caller already holds: row r is values[row_off[r] .. + row_nh[r]) in log10,
 * priority[row_off[r] + h] or priority == NULL (no tie-breaking).  Rows must end below 2^32 values (-E2BIG). */
int mgx_pairhmm_best_alleles(mgx_pairhmm_t* ctx, uint64_t n_rows, const uint64_t* row_off, const uint32_t* row_nh,
                             const double* values_log10, const double* priority, int32_t* out_best);

/* mgx_pairhmm_regions, then per kept read: best haplotype, verbatim shortcut, Smith-Waterman of the read (alt)
 * against that haplotype (ref).
 *   out_log10, out_keep   mgx_pairhmm_regions' outputs, bit for bit (out_keep and its entries may be NULL, as there)
 *   out_best[g][r]        the rule above on the device's own normalised values, for every read
 *   out_offset, out_cigar, out_score (may be NULL)
 *                         for a read with keep == 1 what mgx_sw_align_batch returns for (haplotype best, read bases,
 *                         strategy, sw_params), text capacity min(2 * max(lengths), cigar_stride - 1) included;
 *                         read r's text starts at out_cigar[g] + r * cigar_stride.  For SOFTCLIP and IGNORE a read that
 *                         occurs verbatim in its best haplotype (bytes compared, no base folding) is not aligned:
 *                         "<len>M", offset = its last occurrence, score = len * match.
 *                         For keep == 0: MGX_REALIGN_NOT_ALIGNED, an empty string, score 0.
 * -EINVAL if the two contexts sit on different devices.  -E2BIG, before anything is launched, if a haplotype of a
 * region that has reads (any of them may come out best) or a read exceeds the Smith-Waterman context's lengths.
 * Empty regions are allowed. */
int mgx_realign_regions(mgx_pairhmm_t* ctx, mgx_sw_t* sw, uint32_t n_regions, const mgx_pairhmm_input_t* regions,
                        const uint8_t* const* mapq, const mgx_read_model_t* model,
                        const double* const* hap_priority,      /* [g][n_haps]; NULL or NULL entries = none */
                        const mgx_sw_params_t* sw_params,       /* NULL = {10,-15,-30,-5} */
                        uint8_t strategy,                       /* MGX_SW_SOFTCLIP in the reference */
                        double* const* out_log10, uint8_t* const* out_keep,
                        int32_t* const* out_best, int32_t* const* out_offset,
                        char* const* out_cigar, uint32_t cigar_stride, int32_t* const* out_score /* may be NULL */);
int mgx_realign_stats(mgx_pairhmm_t* ctx, mgx_realign_stats_t* out);

/* ---- read -> reference --------------------------------------------------------------------------------------------------------- */
#define MGX_TO_REF_OK        0  /* realigned: out_start, out_cigar, out_n_cigar valid */
#define MGX_TO_REF_DROPPED   1  /* keep == 0 (fused call only) */
#define MGX_TO_REF_UNCHANGED 2  /* aligner offset == -1: the reference returns the original read */
#define MGX_TO_REF_THROWS    3  /* the reference throws here (operator pair without transformer, a validateArg, ran off the
                                   haplotype CIGAR, final read-length check): its caller drops the region */
#define MGX_TO_REF_UNDEFINED 4  /* the reference would index outside its arrays */
#define MGX_TO_REF_NO_ROOM   5  /* more than cigar_stride elements; out_n_cigar = the count needed */
#define MGX_TO_REF_N_STATUS  6

/* CIGAR elements are BAM-encoded: length << 4 | operator (MIDNSHP=X = 0..8). */
typedef struct mgx_to_ref_input {
    uint64_t n_reads;
    const uint64_t* read_off;       /* [n_reads + 1] into read_bases */
    const uint8_t* read_bases;
    const int32_t* sw_offset;       /* [n_reads] the aligner's alignment offset on the haplotype */
    const uint64_t* sw_cigar_off;   /* [n_reads + 1] into sw_cigar */
    const uint32_t* sw_cigar;       /* the aligner's read -> haplotype CIGARs */
    const uint32_t* read_hap;       /* [n_reads] the read's haplotype, an index into the three arrays below */
    uint64_t n_haps;
    const uint64_t* hap_cigar_off;  /* [n_haps + 1] into hap_cigar */
    const uint32_t* hap_cigar;      /* Haplotype::getCigar() as it is, unpadded and unconsolidated */
    const int32_t* hap_start;       /* [n_haps] getAlignmentStartHapwrtRef */
    const uint32_t* read_ref;       /* [n_reads] the reference haplotype of the read's region, an index into ref_off */
    uint64_t n_refs;
    const uint64_t* ref_off;        /* [n_refs + 1] into ref_bases */
    const uint8_t* ref_bases;
    const int32_t* reference_start; /* [n_reads] */
    const uint32_t* hard_clips;     /* [2 * n_reads] leading and trailing H length of the original read, 0 = none; may be NULL */
} mgx_to_ref_input_t;

/* the to-reference part of one region of mgx_realign_regions_to_ref; haplotypes are the region's own, in its order */
typedef struct mgx_to_ref_region {
    const uint64_t* hap_cigar_off;  /* [n_haps + 1] into hap_cigar */
    const uint32_t* hap_cigar;
    const int32_t* hap_start;       /* [n_haps] */
    uint32_t ref_hap;               /* which of the region's haplotypes is the reference haplotype */
    int32_t reference_start;
    const uint32_t* hard_clips;     /* [2 * n_reads]; may be NULL */
} mgx_to_ref_region_t;

typedef struct mgx_realign_to_ref_stats {
    uint64_t n_status[MGX_TO_REF_N_STATUS];   /* reads per status of the last to-reference call on the context */
    float ms_to_ref;                          /* the kernel, HIP events, valid when the context times (MGX_PAIRHMM_TIMING) */
} mgx_realign_to_ref_stats_t;

/* Per read r: out_status[r]; for MGX_TO_REF_OK out_start[r] (reference_start + hap_start + readStartOnHaplotype + the leading
 * deletions the left-alignment removed), out_n_cigar[r] elements at out_cigar + r * cigar_stride, hard clips included.  For
 * MGX_TO_REF_NO_ROOM out_n_cigar[r] is the count the row would need.  Otherwise out_start[r] = 0, out_n_cigar[r] = 0; a row that
 * is not OK holds nothing of meaning.  Per-read outcomes are statuses, never an error code.
 * -EINVAL / -E2BIG before anything is launched: NULL arrays, decreasing offsets, an index out of range, an operator code above 8,
 * a read or reference haplotype of 2^28 bases or more, 2^32 elements or more. */
int mgx_read_to_ref(mgx_pairhmm_t* ctx, const mgx_to_ref_input_t* in, int32_t* out_start, uint32_t* out_cigar, uint32_t cigar_stride,
                    uint32_t* out_n_cigar, uint8_t* out_status);

/* mgx_realign_regions, every output as that call gives it, and per read of region g the outputs of mgx_read_to_ref on that call's
 * own best haplotype, offset and aligner CIGAR (for a verbatim read "<len>M" at its match): out_start[g][r], out_n_ref_cigar[g][r]
 * elements at out_ref_cigar[g] + r * ref_cigar_stride, out_status[g][r]; MGX_TO_REF_DROPPED where keep == 0.  The aligner's CIGAR
 * is taken as its text holds it (an element the text has no room for is absent here too). */
int mgx_realign_regions_to_ref(mgx_pairhmm_t* ctx, mgx_sw_t* sw, uint32_t n_regions, const mgx_pairhmm_input_t* regions,
                               const uint8_t* const* mapq, const mgx_read_model_t* model, const double* const* hap_priority,
                               const mgx_sw_params_t* sw_params, uint8_t strategy,
                               double* const* out_log10, uint8_t* const* out_keep, int32_t* const* out_best, int32_t* const* out_offset,
                               char* const* out_cigar, uint32_t cigar_stride, int32_t* const* out_score /* may be NULL */,
                               const mgx_to_ref_region_t* to_ref /* [n_regions] */,
                               int32_t* const* out_start, uint32_t* const* out_ref_cigar, uint32_t ref_cigar_stride,
                               uint32_t* const* out_n_ref_cigar, uint8_t* const* out_status);
int mgx_realign_to_ref_stats(mgx_pairhmm_t* ctx, mgx_realign_to_ref_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MGX_REALIGN_H */
