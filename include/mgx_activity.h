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
 * adaptor boundary that give each read its pileup window (read/ReadCache.cpp:324-338).  The step behind the per-locus value
 * (ActivityProfile / BandPassActivityProfile smoothing, the cutting of regions) is mgx_activity_profile_regions below.
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

/* ---- active regions from per-locus values: BandPassActivityProfile + ActivityProfile::popReadyAssemblyRegions as
 * M2/main.cpp:267-328 drives them over ONE contiguous locus sequence (the rule: csrc/activity_profile_rule.h).  The profile is
 * empty before the first locus and force-converted behind the last, so two halves of an interval do not compose to the whole:
 * one call per contiguous stretch.  What stays with the caller: the `getStart() >= start && < end` filter of main.cpp:276,
 * fillNextAssemblyRegionWithReads, and gaps in the locus sequence. */
#define MGX_ACTIVITY_BAND_TILE 256       /* states per workgroup of the band-pass kernel */
#define MGX_ACTIVITY_MAX_FILTER 256      /* the largest filter size F a call takes */

typedef struct mgx_activity_region_params {
    int32_t max_prob_propagation;        /* MTAC.maxProbPropagationDistance, 50; must be >= the filter size */
    int32_t padding;                     /* assemblyRegionPadding, 100 */
    int32_t min_region_size;             /* minAssemblyRegionSize, 50 */
    int32_t max_region_size;             /* maxAssemblyRegionSize, 300 */
    int32_t max_filter_size;             /* BandPassActivityProfile::MAX_FILTER_SIZE, 50 */
    int32_t adaptive_filter_size;        /* 1 */
    uint32_t flags;                      /* MGX_PAIRHMM_TIMING: HIP events around the band-pass kernel and around the rest */
    uint32_t n_band_weights;             /* 2F + 1 when band_weights is given */
    double active_prob_threshold;        /* 0.002 */
    double sigma;                        /* BandPassActivityProfile::DEFAULT_SIGMA, 17.0 */
    const double* band_weights;          /* NULL: makeKernel(F, sigma) as the reference builds it, in double on the host */
} mgx_activity_region_params_t;

typedef struct mgx_activity_region { int32_t start, end, ext_start, ext_end; } mgx_activity_region_t;      /* 0-based, ends inclusive */

/* The region calls keep their counts in a struct and a call of their own, so that mgx_activity_stats_t keeps its layout. */
typedef struct mgx_activity_region_stats {
    uint64_t n_states, n_runs, n_regions;   /* of the last region call on the context */
    uint32_t n_launches;                    /* kernels that call launched: 0 after an argument error */
    float ms_band, ms_cut;                  /* HIP events, valid when the call asked for MGX_PAIRHMM_TIMING */
} mgx_activity_region_stats_t;

/* the values of main.cpp:197,447, band_weights NULL */
void mgx_activity_region_params_defaults(mgx_activity_region_params_t* rp);
/* Host only: the 2F + 1 weights a call with these parameters uses, and F.  -ENOSPC (filter_size written) when cap is too small. */
int mgx_activity_band_weights(const mgx_activity_region_params_t* rp, double* out, uint32_t cap, int32_t* filter_size);
/* prob[l]: the ActivityProfileState value of locus interval_start + l, in [0, 1].  out_regions: the active regions in order of
 * start; out_profile (may be NULL): the smoothed value of every state, n_states of them (states may lie beyond the last locus,
 * up to F behind the last locus with prob > 0, never beyond the contig).  Held equal to the reference's compiled ActivityProfile.cpp (regions equal, state
 * values bit-equal; tests/golden/activity_regions.npz), the early return of popReadyAssemblyRegions behind an inactive piece
 * included.  The device flushes subnormal products prob * weight.
 * -EINVAL before anything is launched: max_prob_propagation below the filter size, a probability that is NaN or outside
 * [0, 1], min_region_size < 1, max_region_size < min_region_size, padding < 0, contig_length not beyond the last locus, a
 * threshold or weight that is not finite, sigma <= 0, a filter size above MGX_ACTIVITY_MAX_FILTER, an even n_band_weights.
 * -E2BIG before anything is launched: the interval or the contig ends beyond 2^31.
 * -ENOSPC after the run with no output written: more regions than cap (n_regions holds the count needed) or more states
 * than profile_cap (n_states holds it). */
int mgx_activity_profile_regions(mgx_activity_t* ctx, int32_t interval_start, uint32_t n_loci, const double* prob, int64_t contig_length,
                                 const mgx_activity_region_params_t* rp, mgx_activity_region_t* out_regions, uint64_t cap,
                                 uint64_t* n_regions, double* out_profile /* may be NULL */, uint64_t profile_cap, uint64_t* n_states);
/* Reads to regions in one call: the two kernels of mgx_activity_interval, then the region kernels on the 0 / 1 bytes where the
 * second left them on the device, on one stream.  The regions (and profile) are those of mgx_activity_profile_regions fed with
 * out_active.  out_active, out_log_odds, out_depth may each be NULL; the per-locus arrays are downloaded only when one of them
 * is asked for, and mgx_activity_stats' n_active / n_callable are counted only then.  Every argument error of either call
 * before anything is launched; -E2BIG (a locus deeper than max_depth) before any region kernel, nothing written. */
int mgx_activity_interval_regions(mgx_activity_t* ctx, const mgx_activity_input_t* in, const mgx_activity_params_t* p, int64_t contig_length,
                                  const mgx_activity_region_params_t* rp, mgx_activity_region_t* out_regions, uint64_t cap,
                                  uint64_t* n_regions, double* out_profile /* may be NULL */, uint64_t profile_cap, uint64_t* n_states,
                                  uint8_t* out_active /* may be NULL */, double* out_log_odds /* may be NULL */, uint32_t* out_depth /* may be NULL */);
int mgx_activity_region_stats(mgx_activity_t* ctx, mgx_activity_region_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MGX_ACTIVITY_H */
