// mgx_tables.cpp -- host-side construction of the PairHMM probability tables (product code).
//
// The device kernels look transition/emission probabilities up in two tables per precision.
// To return the reference's numbers the tables have to be the reference's tables, including
// its deliberate quirks, so they are built here the way Context<NUMBER> builds them
// (deepmutect/Mutect2Cpp-master/src/intel/pairhmm/Context.h):
//   * ph2pr[q] = 10^(-q/10), q in [0,127]; fp32 uses powf on float operands   (:139, :180)
//   * matchToMatchProb[(max*(max+1)/2) + min] through the Jacobian-logarithm approximation
//     with a 1e-4 step table of 80 001 entries, hard rounding, and the TRUNCATED constant
//     INV_LN10 = 0.434294                                                     (:65-122)
// Quality bytes are masked to 7 bits before lookup (ReadForPairHMM.cpp:34-36), so only the
// first 128*129/2 = 8256 triangular entries are reachable; the whole 255-quality triangle is
// still built so that index arithmetic is identical.
#include "mgx_tables.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

namespace mgx {
namespace {

constexpr int kMaxQual = 254;
constexpr double kJacTol = 8.0;
constexpr double kJacStep = 0.0001;
constexpr double kJacInvStep = 1.0 / kJacStep;
constexpr int kJacSize = 80001;

template <typename T>
struct Builder {
    std::vector<T> jac;

    static int fast_round(T d) { return (d > T(0)) ? int(d + T(0.5)) : int(d - T(0.5)); }

    T approx_log10_sum(T small, T big) const {
        if (small > big) std::swap(small, big);
        if (std::isinf(small) || std::isinf(big)) return big;
        T diff = big - small;
        if (diff >= T(kJacTol)) return big;
        int ind = fast_round(T(diff * T(kJacInvStep)));
        return big + jac[ind];
    }

    void build(Tables<T>& t) {
        jac.resize(kJacSize);
        for (int k = 0; k < kJacSize; ++k)
            jac[k] = T(std::log10(1.0 + std::pow(10.0, -double(k) * kJacStep)));
        const double inv_ln10 = 0.434294;  // sic: the reference truncates 1/ln(10)
        t.mm.resize(kMmSize);
        for (int i = 0, offset = 0; i <= kMaxQual; offset += ++i)
            for (int j = 0; j <= i; ++j) {
                double log10_sum = approx_log10_sum(T(-0.1) * T(i), T(-0.1) * T(j));
                double m2m_log10 = std::log1p(-std::min(1.0, std::pow(10, log10_sum))) * inv_ln10;
                t.mm[offset + j] = T(std::pow(10, m2m_log10));
            }
    }
};

}  // namespace

template <>
const Tables<float>& tables<float>() {
    static Tables<float> t;
    static std::once_flag once;
    std::call_once(once, [] {
        Builder<float>().build(t);
        t.ph2pr.resize(kPh2prSize);
        for (int x = 0; x < kPh2prSize; ++x) t.ph2pr[x] = powf(10.f, -float(x) / 10.f);
        t.ph2pr_div3.resize(kPh2prSize); t.gap_ratio.resize(kPh2prSize);
        for (int x = 0; x < kPh2prSize; ++x) {
            t.ph2pr_div3[x] = t.ph2pr[x] / 3.0f;                                   // VEC_DIV(distm, 3), avx-pairhmm-template.h:150
            const float g = 1.0f - t.ph2pr[x];
            t.gap_ratio[x] = g != 0.0f ? t.ph2pr[x] / g : 0.0f;
        }
        t.initial = ldexpf(1.f, 120);
        t.log10_initial = log10f(t.initial);
    });
    return t;
}

template <>
const Tables<double>& tables<double>() {
    static Tables<double> t;
    static std::once_flag once;
    std::call_once(once, [] {
        Builder<double>().build(t);
        t.ph2pr.resize(kPh2prSize);
        for (int x = 0; x < kPh2prSize; ++x) t.ph2pr[x] = std::pow(10.0, -double(x) / 10.0);
        t.ph2pr_div3.resize(kPh2prSize); t.gap_ratio.resize(kPh2prSize);
        for (int x = 0; x < kPh2prSize; ++x) {
            t.ph2pr_div3[x] = t.ph2pr[x] / 3.0;
            const double g = 1.0 - t.ph2pr[x];
            t.gap_ratio[x] = g != 0.0 ? t.ph2pr[x] / g : 0.0;
        }
        t.initial = std::ldexp(1.0, 1020);
        t.log10_initial = std::log10(t.initial);
    });
    return t;
}

// digamma at the integers as the reference's cache evaluates it: from 49 on the asymptotic series ln x - 1/(2x) - 1/(12 x^2) -/+ ..., and
// psi(n) = psi(n + 1) - 1/n below it.  The series' next term is +1/(120 x^4); the reference subtracts it (sic, as Apache Commons Math's
// Gamma.digamma does), which puts every value 2/(120 x^4) <= 2.9e-9 below the function.  Under a common offset the difference
// digamma(nRef + 1) - digamma(nAlt + 1) of the rule keeps it only where one count is below 49 and the other is not, but there it moves the
// log-odds by more than the 1e-9 they are held to, so the sign is the reference's.  log10(n!) = lgamma(n + 1) log10(e).
void build_activity_tables(unsigned n_counts, ActivityTables* out) {
    constexpr unsigned kSeriesFrom = 49;
    auto series = [](double x) {
        const double inv = 1.0 / (x * x);
        return std::log(x) - 0.5 / x - inv * (1.0 / 12 + inv * (1.0 / 120 - inv / 252));
    };
    const unsigned n_dig = std::max(n_counts, kSeriesFrom + 1);
    std::vector<double> dig(n_dig);
    for (unsigned n = kSeriesFrom; n < n_dig; ++n) dig[n] = series(double(n));
    for (unsigned n = kSeriesFrom; n-- > 0;) dig[n] = dig[n + 1] - 1.0 / double(n);          // n = 0: -inf
    out->digamma.assign(dig.begin(), dig.begin() + n_counts);
    out->log10_factorial.resize(n_counts);
    for (unsigned n = 0; n < n_counts; ++n) out->log10_factorial[n] = std::lgamma(double(n) + 1.0) * 0.4342944819032518;
    constexpr double kPhredToLogErrorProb = -0.23025850929940458;      // -ln(10) / 10
    constexpr double kLogHalf = -0.6931471805599453;
    for (int q = 0; q < 128; ++q) {
        out->eps[q] = std::pow(10.0, double(q) / -10.0);
        const double a = double(q) * kPhredToLogErrorProb;
        out->log_eps[q] = a;
        // log(1 - exp(a)) for a <= 0, the branch by which side of log(1/2) a lies
        out->log_one_minus_eps[q] = a == 0 ? -HUGE_VAL : a < kLogHalf ? std::log1p(-std::exp(a)) : std::log(-std::expm1(a));
    }
}

}  // namespace mgx
