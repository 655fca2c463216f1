/*
 * mgx_activity.h -- C ABI of the active-site detection per locus (libmgx.so).
 *
 * What the reference runs once for every locus of the genome before any region exists (M2/main.cpp:254-300): the pileup of
 * the locus, the alt qualities of its reads and the log-odds that decide whether the locus is active.  Reference interface
 * replaced (paths relative to deepmutect/Mutect2Cpp-master/src/):
 *
 *   mgx_activity_interval  <- Mutect2Engine::isActive per locus (Mutect2Engine.cpp:58-88) with altQuals (:91-111),
 *                             indelQual, isNextToUsefulSoftClip, getCurrentOrFollowingIndelLength (:114-127) and
 *                             logLikelihoodRatio (:133-150, repeatFactor 1); per (read, locus) PeUtils
 *                             (utils/PeUtils.cpp:10-183) over the PositionToCigarMap of samtools/SAMRecord.cpp:557-584;
 *                             the tables behind MathUtils::digamma / log10Factorial (MathUtils.cpp:12-27),
 *                             QualityUtils::qualToErrorProb (QualityUtils.cpp:31-45) and NaturalLogUtils::qualToLogErrorProb /
 *                             qualToLogProb (NaturalLogUtils.cpp:13-32)
 *
 * The rule is stated once in csrc/activity_rule.h.  What stays with the caller: the read filters, the down-sampler and the
 * adaptor boundary that give each read its pileup window (read/ReadCache.cpp:324-338), and everything behind the per-locus
 * value (ActivityProfile / BandPassActivityProfile smoothing, the cutting of regions).
 * All functions return 0 or a negative errno-style code with mgx_last_error() set.  No CPU fallback.
 */
#ifndef MGX_ACTIVITY_H
#define MGX_ACTIVITY_H

#include <stdint.h>

#include "mgx_pairhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgx_activity mgx_activity_t;

#define MGX_ACTIVITY_DEFAULT_MAX_DEPTH 65535u
#define MGX_ACTIVITY_TUMOUR 0
#define MGX_ACTIVITY_NORMAL 1

/* One contig interval [interval_start, interval_start + n_loci) and the reads whose pileup windows may touch it, as
 * structure-of-arrays.  Positions are 0-based.  CIGAR elements are BAM-encoded: length << 4 | operator (MIDNSHP=X = 0..8). */
typedef struct mgx_activity_input {
    int32_t interval_start;
    uint32_t n_loci;
    const uint8_t* ref_bases;      /* [n_loci] refCache->getBase(pos); bytes are compared as they are */
    uint64_t n_reads;
    const int32_t* read_start;     /* [n_reads] SAMRecord::getStart */
    const uint64_t* cigar_off;     /* [n_reads + 1] into cigar */
    const uint32_t* cigar;
    const uint64_t* base_off;      /* [n_reads + 1] into bases and quals */
    const uint8_t* bases;
    const uint8_t* quals;          /* 0..127 */
    const uint16_t* flags;         /* [n_reads] the BAM FLAG; only 0x2 (proper pair) and 0x8 (mate unmapped) are read */
    const int32_t* mate_start;     /* [n_reads] core.mpos; -1 counts as an unmapped mate (SAMRecord::mateIsUnmapped) */
    const uint8_t* sample;         /* [n_reads] MGX_ACTIVITY_TUMOUR or MGX_ACTIVITY_NORMAL */
    const int32_t* act_start;      /* [n_reads] pileRead::activateStart, non-decreasing over the reads */
    const int32_t* act_stop;       /* [n_reads] pileRead::activateStop, inclusive; act_stop < act_start = an empty window */
} mgx_activity_input_t;

typedef struct mgx_activity_params {
    int32_t has_normal;                 /* Mutect2Engine::hasNormal() */
    int32_t genotype_germline_sites;    /* MTAC.genotypeGermlineSites */
    int32_t min_callable_depth;         /* a locus counts in n_callable when its depth is above this */
    int32_t pcr_error_qual;             /* 40; 2..254 */
    int32_t min_base_quality;           /* MINIMUM_BASE_QUALITY, 6; 0..127 */
    uint32_t flags;                     /* MGX_PAIRHMM_TIMING: HIP events around the two kernels */
    double initial_log_odds;            /* M2ArgumentCollection.h:40-45 */
} mgx_activity_params_t;

typedef struct mgx_activity_stats {
    uint64_t n_loci, n_elements, n_active, n_callable;   /* of the last mgx_activity_interval call on the context */
    uint32_t n_launches;                                  /* kernels that call launched: 0 after an argument error */
    float ms_elements, ms_locus;                          /* HIP events, valid when the call asked for MGX_PAIRHMM_TIMING */
} mgx_activity_stats_t;

/* max_depth: the deepest locus (tumour + normal reads) the count tables reach; 0 = MGX_ACTIVITY_DEFAULT_MAX_DEPTH.
 * -ENODEV without a HIP device. */
int mgx_activity_create(int device, uint32_t max_depth, mgx_activity_t** out);
void mgx_activity_destroy(mgx_activity_t* ctx);
/* has_normal 0, genotype_germline_sites 0, min_callable_depth 10, initial_log_odds 4.605170185988092, pcr_error_qual 40,
 * min_base_quality 6, flags 0 */
void mgx_activity_params_defaults(mgx_activity_params_t* p);

/* Per locus l of the interval:
 *   out_active[l]    1 or 0: the ActivityProfileState value of Mutect2Engine.cpp:70/74/84/87
 *   out_log_odds[l]  tumorLogOdds where the reference computes it, NaN where the tumour pileup has no alt element
 *   out_depth[l]     tumour size + normal size (AlignmentContext::getReadNum, :61)
 * A read is in the pileup of every locus of its window, deletions included.  out_log_odds[l] depends on the reads that
 * cover l and their order alone, not on the interval they are passed with.
 * -EINVAL / -E2BIG before anything is launched: NULL arrays, decreasing offsets, act_start not sorted, a window that is not
 * empty and leaves the read's reference span, an operator code above 8 or N (the reference reads outside the read there), a
 * zero-length element, a CIGAR whose read length is not the read's number of bases, a quality above 127 (the reference
 * pushes it through a signed char; that is not reproduced), a sample other than 0 / 1, 2^32 pileup elements or more, an
 * interval or a read that ends beyond 2^31.
 * -E2BIG after the run, with no output written, if a locus is deeper than the context's max_depth. */
int mgx_activity_interval(mgx_activity_t* ctx, const mgx_activity_input_t* in, const mgx_activity_params_t* p,
                          uint8_t* out_active, double* out_log_odds /* may be NULL */, uint32_t* out_depth /* may be NULL */);
int mgx_activity_stats(mgx_activity_t* ctx, mgx_activity_stats_t* out);
/* The element bytes of the last mgx_activity_interval call that ran, for inspection: per read, in input order, one byte per
 * position of its window (0 = in the pileup, not alt; 1..127 = the alt quality; 0 outside the interval).  n must be that
 * call's n_elements. */
int mgx_activity_last_elements(mgx_activity_t* ctx, uint8_t* out, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* MGX_ACTIVITY_H */
