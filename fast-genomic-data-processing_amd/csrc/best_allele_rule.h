// best_allele_rule.h -- AlleleLikelihoods::searchBestAllele(sample, read, canBeReference = true, priorities) as two associative folds
// (utils/genotyper/AlleleLikelihoods.h:92-146; only bestAlleleIndex is consumed downstream, so the order-dependent second-best bookkeeping
// is not kept).  No HIP: pairhmm_best_allele_rows (pairhmm_kernels.hip.inc) folds these per lane and then across lanes with shuffles,
// tests/cpp/best_allele_driver.cpp folds them serially, in strided lanes and in random split trees (tests/test_best_allele_host.py, CPU,
// ASan + UBSan).
//   values     v[a] = log10[a] * std::log(10), the rounded product (switchToNaturalLog, AlleleLikelihoods.h:462-476, MathUtils.cpp:16-18)
//   threshold  T = 0.2 * std::log(10) (PairHMMLikelihoodCalculationEngine.cpp:23)
//   first fold   b0 = the first index that attains max v                                          "max value, then lowest index"
//   second fold  over a != b0:  entered |= v[b0] - v[a] < T;  a is a candidate iff !(v[b0] - v[a] > T);
//                c = the first candidate that attains the maximum priority over the candidates    "max priority, then lowest index"
//   result       c if entered and priority[c] > priority[b0], else b0
// Inputs are finite or -inf.  A row that is all -inf: every difference is a NaN, nothing is entered, the result is 0.
// Build with -ffp-contract=off (the product is rounded before the subtraction, as in the reference).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MGX_BA_FN __host__ __device__ inline
#else
#define MGX_BA_FN inline
#endif

namespace mgx_best_allele {

constexpr double kLn10 = 0x1.26bb1bbb55516p+1;        // std::log(10)
constexpr double kThreshold = 0.2 * kLn10;            // NATURAL_LOG_INFORMATIVE_THRESHOLD
constexpr uint32_t kNone = 0xFFFFFFFFu;               // the index of a fold over nothing
constexpr double kMinusInf = -__builtin_inf();

// ---- first fold: the likelihood-best allele
struct Top { double v; uint32_t at; };
MGX_BA_FN Top top_identity() { return Top{kMinusInf, kNone}; }
MGX_BA_FN Top top_of(double log10, uint32_t a) { return Top{log10 * kLn10, a}; }
// (field by field: a choice between two whole structs goes through their addresses, which put the kernel's copies into scratch memory)
MGX_BA_FN Top merge(Top x, Top y) {
    const bool take = y.v > x.v || (y.v == x.v && y.at < x.at);
    return Top{take ? y.v : x.v, take ? y.at : x.at};
}

// ---- second fold: is the tie-break entered, and its best candidate
struct Cand { double pri; uint32_t at, entered; };
MGX_BA_FN Cand cand_identity() { return Cand{kMinusInf, kNone, 0u}; }
// allele a with natural-log value v_a = top_of(log10[a], a).v and priority pri_a, against the first fold's result
MGX_BA_FN Cand cand_of(Top best, double v_a, double pri_a, uint32_t a) {
    const double d = best.v - v_a;
    const bool other = a != best.at, in = other && !(d > kThreshold);
    return Cand{in ? pri_a : kMinusInf, in ? a : kNone, (other && d < kThreshold) ? 1u : 0u};
}
MGX_BA_FN Cand merge(Cand x, Cand y) {
    const bool take = x.at == kNone || (y.at != kNone && (y.pri > x.pri || (y.pri == x.pri && y.at < x.at)));
    return Cand{take ? y.pri : x.pri, take ? y.at : x.at, x.entered | y.entered};
}

// pri_best = priority[best.at]; a row without alleles gives 0
MGX_BA_FN uint32_t result(Top best, double pri_best, Cand c) {
    if (best.at == kNone) return 0u;
    return (c.entered && c.at != kNone && c.pri > pri_best) ? c.at : best.at;
}

}  // namespace mgx_best_allele
