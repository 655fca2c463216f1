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
 * consolidateCigar, applyCigarToCigar, leftAlignIndel and the SAMRecord clone stay host code in the caller.
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

#ifdef __cplusplus
}
#endif
#endif /* MGX_REALIGN_H */
