/*
 * oracle/pairhmm_oracle.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Scalar CPU restatement of the reference PairHMM likelihood path.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library, and only
 * as the checker.  The shipped path (fast-genomic-data-processing_amd/csrc) never links it.
 *
 * Parity pin: validated against the reference's own AVX-512/AVX kernels compiled in place
 * from /root/reference (oracle/_ref, see oracle/Makefile) and against the golden vectors in
 * tests/golden/ generated from that build (tests/golden/make_golden.py).
 *
 * Reference files restated (paths relative to deepmutect/Mutect2Cpp-master/src/):
 *   intel/pairhmm/Context.h:65-122,134-209      tables: ph2pr, jacobianLogTable, matchToMatchProb
 *   haplotypecaller/ReadForPairHMM.cpp:18-82    per-read byte masking (&127) and 7 prob vectors
 *   intel/pairhmm/pairhmm_common.h:68-87        base -> code table (unknown byte -> 'A')
 *   intel/pairhmm/avx-pairhmm-template.h:30-62,97-102,110-192,204-345  the M/X/Y recurrence
 *   intel/pairhmm/IntelPairHmm.cc:332-351       float first, < 1e-28f -> double, log10 - const
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <xmmintrin.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define MAX_QUAL 254
#define JAC_TOL 8.0
#define JAC_STEP 0.0001
#define JAC_INV_STEP (1.0 / JAC_STEP)
#define JAC_SIZE 80001 /* (int)(8.0 / 0.0001) + 1, Context.h:33 */
#define MM_SIZE (((MAX_QUAL + 1) * (MAX_QUAL + 2)) >> 1)

static float  f_ph2pr[128], f_jac[JAC_SIZE], f_mm[MM_SIZE];
static double d_ph2pr[128], d_jac[JAC_SIZE], d_mm[MM_SIZE];
static float  f_init, f_log10_init;
static double d_init, d_log10_init;
static uint8_t conv[256];
static int inited = 0;

/* Context.h:91-94 */
static int fround_f(float d) { return (d > 0.0f) ? (int)(d + 0.5f) : (int)(d - 0.5f); }
static int fround_d(double d) { return (d > 0.0) ? (int)(d + 0.5) : (int)(d - 0.5); }

/* Context.h:96-122 */
static float approx_sum_f(float small, float big) {
    if (small > big) { float t = big; big = small; small = t; }
    if (isinf(small) || isinf(big)) return big;
    float diff = big - small;
    if (diff >= (float)JAC_TOL) return big;
    int ind = fround_f((float)(diff * ((float)JAC_INV_STEP)));
    return big + f_jac[ind];
}
static double approx_sum_d(double small, double big) {
    if (small > big) { double t = big; big = small; small = t; }
    if (isinf(small) || isinf(big)) return big;
    double diff = big - small;
    if (diff >= JAC_TOL) return big;
    int ind = fround_d(diff * JAC_INV_STEP);
    return big + d_jac[ind];
}

void ph_oracle_init(void) {
    if (inited) return;
    /* Context.h:65-72 */
    for (int k = 0; k < JAC_SIZE; k++) {
        double v = log10(1.0 + pow(10.0, -((double)k) * JAC_STEP));
        f_jac[k] = (float)v;
        d_jac[k] = v;
    }
    /* Context.h:75-89 (note the truncated constant INV_LN10) */
    const double INV_LN10 = 0.434294;
    for (int i = 0, offset = 0; i <= MAX_QUAL; offset += ++i)
        for (int j = 0; j <= i; j++) {
            double sf = approx_sum_f((float)-0.1 * (float)i, (float)-0.1 * (float)j);
            double sd = approx_sum_d(-0.1 * (double)i, -0.1 * (double)j);
            double mf = log1p(-fmin(1.0, pow(10, sf))) * INV_LN10;
            double md = log1p(-fmin(1.0, pow(10, sd))) * INV_LN10;
            f_mm[offset + j] = (float)pow(10, mf);
            d_mm[offset + j] = pow(10, md);
        }
    /* Context.h:134-147, 175-188 */
    for (int x = 0; x < 128; x++) {
        d_ph2pr[x] = pow(10.0, -((double)x) / 10.0);
        f_ph2pr[x] = powf(10.f, -((float)x) / 10.f);
    }
    d_init = ldexp(1.0, 1020);
    d_log10_init = log10(d_init);
    f_init = ldexpf(1.f, 120);
    f_log10_init = log10f(f_init);
    /* pairhmm_common.h:75-81; table is zero-initialised so any other byte maps to 0 ('A') */
    memset(conv, 0, sizeof conv);
    conv['A'] = 0; conv['C'] = 1; conv['T'] = 2; conv['G'] = 3; conv['N'] = 4;
    inited = 1;
}

/* Context.h:156-167, 197-209; quals are already &127 so the MAX_QUAL branch is dead */
static float mm_prob_f(int ins, int del) {
    int mn = del, mx = ins;
    if (ins <= del) { mn = ins; mx = del; }
    return f_mm[((mx * (mx + 1)) >> 1) + mn];
}
static double mm_prob_d(int ins, int del) {
    int mn = del, mx = ins;
    if (ins <= del) { mn = ins; mx = del; }
    return d_mm[((mx * (mx + 1)) >> 1) + mn];
}

/* Tables for the product to be compared against in tests (never used by the product itself). */
const float*  ph_oracle_table_mm_f32(void) { ph_oracle_init(); return f_mm; }
const double* ph_oracle_table_mm_f64(void) { ph_oracle_init(); return d_mm; }
const float*  ph_oracle_table_ph2pr_f32(void) { ph_oracle_init(); return f_ph2pr; }
const double* ph_oracle_table_ph2pr_f64(void) { ph_oracle_init(); return d_ph2pr; }

#define MATCH(rc, hc) ((rc) == (hc) || (rc) == 4 || (hc) == 4)

/* avx-pairhmm-template.h:204-345 restated cell by cell (same operation order per cell,
 * last-row sums taken in column order, sumM and sumX kept apart and added once). */
#define DEFINE_PROB(NAME, T, PH2PR, MMPROB, INIT)                                             \
T NAME(int R, const uint8_t* bases, const uint8_t* qual, const uint8_t* ins,                  \
       const uint8_t* del, const uint8_t* gcp, int H, const uint8_t* hap) {                   \
    T* buf = (T*)malloc(sizeof(T) * 6 * (size_t)(H + 1));                                     \
    T *Mp = buf, *Xp = Mp + (H + 1), *Yp = Xp + (H + 1);                                      \
    T *Mc = Yp + (H + 1), *Xc = Mc + (H + 1), *Yc = Xc + (H + 1);                             \
    T init_Y = INIT / (T)H;                                                                   \
    for (int c = 0; c <= H; c++) { Mp[c] = 0; Xp[c] = 0; Yp[c] = init_Y; }                    \
    T sumM = 0, sumX = 0;                                                                     \
    for (int r = 1; r <= R; r++) {                                                            \
        int _i = ins[r - 1] & 127, _d = del[r - 1] & 127, _c = gcp[r - 1] & 127;              \
        int _q = qual[r - 1] & 127;                                                           \
        T pMM = MMPROB(_i, _d), pXX = PH2PR[_c], pYY = PH2PR[_c];                             \
        T pMX = PH2PR[_i], pMY = PH2PR[_d], pGAPM = (T)1.0 - PH2PR[_c];                       \
        T distm = PH2PR[_q];                                                                  \
        T one_m = (T)1.0 - distm;                                                             \
        T d3 = distm / (T)3.0;                                                                \
        int rc = conv[bases[r - 1]];                                                          \
        Mc[0] = 0; Xc[0] = 0; Yc[0] = 0;                                                      \
        for (int c = 1; c <= H; c++) {                                                        \
            int hc = conv[hap[c - 1]];                                                        \
            T e = MATCH(rc, hc) ? one_m : d3;                                                 \
            T t1 = Mp[c - 1] * pMM;                                                           \
            T t2 = Xp[c - 1] * pGAPM;                                                         \
            T t3 = Yp[c - 1] * pGAPM;                                                         \
            Mc[c] = ((t1 + t2) + t3) * e;                                                     \
            T u1 = Mp[c] * pMX;                                                               \
            T u2 = Xp[c] * pXX;                                                               \
            Xc[c] = u1 + u2;                                                                  \
            T v1 = Mc[c - 1] * pMY;                                                           \
            T v2 = Yc[c - 1] * pYY;                                                           \
            Yc[c] = v1 + v2;                                                                  \
        }                                                                                     \
        if (r == R)                                                                           \
            for (int c = 1; c <= H; c++) { sumM = sumM + Mc[c]; sumX = sumX + Xc[c]; }        \
        T* t;                                                                                 \
        t = Mp; Mp = Mc; Mc = t; t = Xp; Xp = Xc; Xc = t; t = Yp; Yp = Yc; Yc = t;            \
    }                                                                                         \
    T res = sumM + sumX;                                                                      \
    free(buf);                                                                                \
    return res;                                                                               \
}

DEFINE_PROB(ph_oracle_prob_f32, float, f_ph2pr, mm_prob_f, f_init)
DEFINE_PROB(ph_oracle_prob_f64, double, d_ph2pr, mm_prob_d, d_init)

/* IntelPairHmm.cc:332-351.  used_double (may be NULL) reports which branch was taken. */
double ph_oracle_log10(int R, const uint8_t* bases, const uint8_t* qual, const uint8_t* ins,
                       const uint8_t* del, const uint8_t* gcp, int H, const uint8_t* hap,
                       int* used_double) {
    ph_oracle_init();
    unsigned old = _MM_GET_FLUSH_ZERO_MODE();
    _MM_SET_FLUSH_ZERO_MODE(_MM_FLUSH_ZERO_ON); /* IntelPairHmm.cc:230 */
    double out;
    float rf = ph_oracle_prob_f32(R, bases, qual, ins, del, gcp, H, hap);
    if (rf < 1e-28f) {
        double rd = ph_oracle_prob_f64(R, bases, qual, ins, del, gcp, H, hap);
        out = log10(rd) - d_log10_init;
        if (used_double) *used_double = 1;
    } else {
        out = (double)(log10f(rf) - f_log10_init);
        if (used_double) *used_double = 0;
    }
    _MM_SET_FLUSH_ZERO_MODE(old);
    return out;
}

/* Batch form over the same packed layout the C-ABI takes (include/mgx_pairhmm.h).
 * threads <= 0 -> all cores.  Returns the number of threads used. */
int ph_oracle_batch(int64_t n_pairs, const uint64_t* read_off, const uint8_t* bases,
                    const uint8_t* qual, const uint8_t* ins, const uint8_t* del,
                    const uint8_t* gcp, const uint64_t* hap_off, const uint8_t* hap_bases,
                    const uint32_t* pair_read, const uint32_t* pair_hap, double* out_log10,
                    uint8_t* used_double, int threads) {
    ph_oracle_init();
    int used = 1;
#ifdef _OPENMP
    if (threads <= 0) threads = omp_get_max_threads();
    used = threads;
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
#endif
    for (int64_t i = 0; i < n_pairs; i++) {
        uint64_t ro = read_off[pair_read[i]], ho = hap_off[pair_hap[i]];
        int R = (int)(read_off[pair_read[i] + 1] - ro);
        int H = (int)(hap_off[pair_hap[i] + 1] - ho);
        int ud = 0;
        out_log10[i] = ph_oracle_log10(R, bases + ro, qual + ro, ins + ro, del + ro, gcp + ro, H,
                                       hap_bases + ho, &ud);
        if (used_double) used_double[i] = (uint8_t)ud;
    }
    return used;
}

/* ------------------------------------------------------------------------------------------------
 * Row F2 of SURVEY.md section 8f: the per-read quality model in front of the PairHMM and the
 * normalisation / filter behind it.  Parity: n_repetitions and equal_range below are pinned to the reference's own
 * findNumberOfRepetitions (both overloads) and Utils::equalRange, compiled from utils/variant/GATKVariantContextUtils.cpp and
 * utils/Utils.cpp where they lie (oracle/_ref/ref_read_model; answers in tests/golden/read_model.npz, compared through
 * ph_oracle_n_repetitions on 100 000 triples).  MathUtils::fastRound does not build here (boost) and stays restated.
 * Still restated, because haplotypecaller/PairHMMLikelihoodCalculationEngine.cpp needs the whole SAMRecord model:
 * findTandemRepeatUnits :175-254 and the lines around it -- by three independent restatements that must agree byte for byte
 * (this file, oracle/ref_harness/ref_read_model_harness.cpp around the linked search, tests/read_model_cases.py) -- and
 * utils/genotyper/AlleleLikelihoods.h:153-166, 372-419 (A15), which is still boost-bound (this file and the Python).
 * ---------------------------------------------------------------------------------------------- */

/* utils/Utils.cpp:9-17 */
static int equal_range(const uint8_t* l, int lo, const uint8_t* r, int ro, int n) {
    for (int i = 0; i < n; i++) if (l[lo + i] != r[ro + i]) return 0;
    return 1;
}
/* utils/variant/GATKVariantContextUtils.cpp:59-100 */
static int n_repetitions(const uint8_t* unit_full, int unit_off, int unit_len, const uint8_t* test_full,
                         int test_off, int test_len, int leading) {
    if (test_len == 0) return 0;
    int diff = test_len - unit_len, n = 0;
    if (leading) {
        for (int s = 0; s <= diff; s += unit_len) {
            if (equal_range(test_full, s + test_off, unit_full, unit_off, unit_len)) n++; else return n;
        }
    } else {
        for (int s = diff; s >= 0; s -= unit_len) {
            if (equal_range(test_full, s + test_off, unit_full, unit_off, unit_len)) n++; else return n;
        }
    }
    return n;
}
/* PairHMMLikelihoodCalculationEngine.cpp:175-254 */
static int tandem_repeat_units(const uint8_t* b, int length, int offset) {
    int maxBW = 0, bw_off = offset, bw_len = 1;
    for (int str = 1; str <= 8; str++) {
        if (offset + 1 - str < 0) break;
        maxBW = n_repetitions(b, offset - str + 1, str, b, 0, offset + 1, 0);
        if (maxBW > 1) { bw_off = offset - str + 1; bw_len = str; break; }
    }
    int maxRL = maxBW;
    if (offset < length - 1) {
        int maxFW = 0, fw_off = offset + 1, fw_len = 1;
        for (int str = 1; str <= 8; str++) {
            if (offset + str + 1 > length) break;
            maxFW = n_repetitions(b, offset + 1, str, b, offset + 1, length - offset - 1, 1);
            if (maxFW > 1) { fw_off = offset + 1; fw_len = str; break; }
        }
        if (fw_len == bw_len && memcmp(b + fw_off, b + bw_off, fw_len) == 0) {
            maxRL = maxFW + maxBW;
        } else {
            maxBW = n_repetitions(b, fw_off, fw_len, b, 0, offset + 1, 0);
            maxRL = maxFW + maxBW;
        }
    }
    if (maxRL > 20) maxRL = 20;
    return maxRL;
}

/* modifyReadQualities (:123-147): applyPCRErrorModel (:149-157), capMinimumReadQualities (:256-267),
 * buildGapContinuationPenalties (:284-292).  Arrays are modified in place; gcp is written. */
void ph_oracle_read_model(int64_t n_reads, const uint64_t* read_off, const uint8_t* bases, uint8_t* qual,
                          uint8_t* ins, uint8_t* del, uint8_t* gcp, const uint8_t* mapq, int rate_factor,
                          int bq_threshold, int constant_gcp) {
    uint8_t cache[21];
    for (int i = 0; i <= 20; i++) {      /* :45-61 */
        double d = 40.0 - exp((double)i / ((double)rate_factor * M_PI));
        int r = (d > 0.0 ? (int)(d + 0.5) : (int)(d - 0.5)) + 1;
        cache[i] = (uint8_t)(char)(r > 10 ? r : 10);
    }
    for (int64_t r = 0; r < n_reads; r++) {
        const uint64_t o = read_off[r];
        const int len = (int)(read_off[r + 1] - o);
        if (rate_factor > 0)
            for (int i = 1; i < len; i++) {
                int rl = tandem_repeat_units(bases + o, len, i - 1);
                if (cache[rl] < ins[o + i - 1]) ins[o + i - 1] = cache[rl];
                if (cache[rl] < del[o + i - 1]) del[o + i - 1] = cache[rl];
            }
        for (int i = 0; i < len; i++) {
            int q = qual[o + i];
            if (mapq[r] < q) q = mapq[r];
            qual[o + i] = (uint8_t)(q < bq_threshold ? 6 : q);
            if (ins[o + i] < 6) ins[o + i] = 6;
            if (del[o + i] < 6) del[o + i] = 6;
            if (constant_gcp >= 0) gcp[o + i] = (uint8_t)constant_gcp;
        }
    }
}

/* AlleleLikelihoods.h:153-166, 372-391 (normalizeLikelihoods) and :404-419 with
 * PairHMMLikelihoodCalculationEngine.cpp:294-299 (filterPoorlyModeledEvidence).
 * io is [read][haplotype]; keep[r] = 0 for reads the filter removes. */
void ph_oracle_normalize_filter(int64_t n_reads, int64_t n_haps, const uint64_t* read_off, double* io,
                                double log10_rate, double max_error_per_base, uint8_t* keep) {
    for (int64_t r = 0; r < n_reads; r++) {
        double best = -INFINITY;
        for (int64_t h = 0; h < n_haps; h++) if (io[r * n_haps + h] > best) best = io[r * n_haps + h];
        if (!isinf(log10_rate) && n_haps > 1) {
            double cap = best + log10_rate;
            for (int64_t h = 0; h < n_haps; h++) if (io[r * n_haps + h] < cap) io[r * n_haps + h] = cap;
        }
        double len = (double)(read_off[r + 1] - read_off[r]);
        double max_err = fmin(2.0, ceil(len * max_error_per_base));
        keep[r] = !(best < max_err * -4.0);
    }
}

int ph_oracle_tandem_repeat(const uint8_t* bases, int length, int offset) { return tandem_repeat_units(bases, length, offset); }
int ph_oracle_n_repetitions(const uint8_t* unit, int unit_len, const uint8_t* test, int test_len, int leading) { return n_repetitions(unit, 0, unit_len, test, 0, test_len, leading); }
