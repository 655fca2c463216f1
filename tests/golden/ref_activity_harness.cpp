// ref_activity_harness.cpp -- the reference's own PeUtils (utils/PeUtils.cpp) over the PositionToCigarMap its SAMRecord constructor builds
// (samtools/SAMRecord.cpp:495-584), and its own digamma / log10Factorial caches and quality table, on cases read from a text file.
// Mutect2Engine.cpp, MathUtils.cpp and NaturalLogUtils.cpp do not build outside the reference's tree (boost/multi_array.hpp), so
// Mutect2Engine.cpp:58-150 (isActive, altQuals, indelQual, isNextToUsefulSoftClip, getCurrentOrFollowingIndelLength, logLikelihoodRatio),
// MathUtils.cpp:16-27 and NaturalLogUtils.cpp:13-25 are restated below against the reference's PeUtils, SAMRecord and cache symbols: the
// element bytes and the tables come from compiled reference code, the locus formula from this restatement.  bam1_t records are filled in
// by hand through the macros of the reference's htslib/sam.h; the two htslib functions the constructor calls are defined here.
// Built by tests/golden/make_golden_activity.py against the reference's sources where they lie; nothing of it is linked into the product.
//
//   ref_activity cases <file>    input as tests/activity_cases.py::to_text writes it; per case "E <hex bytes>", "L <n>", n lines
//                                "active depth log_odds" (hex float or nan), "end"
//   ref_activity tables <n>      n lines "digamma(k) log10Factorial(k)" (k = 0: nan 0), then 128 lines "eps logEps logOneMinusEps"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "Mutect2Utils.h"
#include "PeUtils.h"
#include "QualityUtils.h"
#include "ReadUtils.h"
#include "cache/DigammaCache.h"
#include "cache/Log10FactorialCache.h"
#include "samtools/SAMRecord.h"

void Mutect2Utils::validateArg(bool condition, const std::string& msg) {
    if (!condition) throw std::invalid_argument(msg);
}
bool ReadUtils::consumesReadBases(uint32_t cigarElement) { return bam_cigar_type(bam_cigar_op(cigarElement)) & 1; }
bool ReadUtils::consumesReferenceBases(uint32_t cigarElement) { return bam_cigar_type(bam_cigar_op(cigarElement)) & 2; }
extern "C" {
hts_pos_t bam_cigar2rlen(int n_cigar, const uint32_t* cigar) {
    hts_pos_t l = 0;
    for (int k = 0; k < n_cigar; ++k) if (bam_cigar_type(bam_cigar_op(cigar[k])) & 2) l += bam_cigar_oplen(cigar[k]);
    return l;
}
const char* sam_hdr_tid2name(const sam_hdr_t*, int tid) { return tid >= 0 ? "chr1" : nullptr; }
}

namespace {
DigammaCache DIGAMMA;
Log10FactorialCache LOG_10_FACTORIAL;
const double PHRED_TO_LOG_ERROR_PROB_FACTOR = -0.23025850929940458, LOG1MEXP_THRESHOLD = -0.6931471805599453;
const int MINIMUM_BASE_QUALITY = 6;      // the reference has it as a constant: the cases of the fixture use no other

// log(1 - e^a) for a <= 0, the branch as NaturalLogUtils.cpp:22-26 takes it; MathUtils.cpp:24-27
double log1mexp(double a) {
    if (a >= 0) return a > 0 ? std::nan("") : -std::numeric_limits<double>::infinity();
    return a < LOG1MEXP_THRESHOLD ? std::log1p(-std::exp(a)) : std::log(-std::expm1(a));
}
double fastBernoulliEntropy(double p) { const double pq = p * (1 - p); return pq * (11 + 33 * pq) / (2 + 20 * pq); }

SAMRecord* make_record(int32_t pos, int32_t mpos, uint16_t flag, const std::vector<uint32_t>& cigar, const std::string& bases, const std::vector<uint8_t>& qual) {
    bam1_t* b = (bam1_t*)calloc(1, sizeof(bam1_t));
    const size_t l_qname = 4, l_qseq = bases.size(), l_data = l_qname + cigar.size() * 4 + ((l_qseq + 1) >> 1) + l_qseq;
    uint8_t* d = (uint8_t*)calloc(l_data ? l_data : 1, 1);
    memcpy(d, "r", 1);
    if (!cigar.empty()) memcpy(d + l_qname, cigar.data(), cigar.size() * 4);
    uint8_t* seq = d + l_qname + cigar.size() * 4;
    for (size_t i = 0; i < l_qseq; ++i) {
        const uint8_t code = bases[i] == 'A' ? 1 : bases[i] == 'C' ? 2 : bases[i] == 'G' ? 4 : bases[i] == 'T' ? 8 : 15;
        seq[i >> 1] |= (uint8_t)(code << ((~i & 1) << 2));
    }
    if (l_qseq) memcpy(seq + ((l_qseq + 1) >> 1), qual.data(), l_qseq);
    b->data = d; b->l_data = (int)l_data; b->m_data = (uint32_t)l_data;
    b->core.pos = pos; b->core.tid = 0; b->core.mtid = 0; b->core.mpos = mpos; b->core.flag = flag;
    b->core.l_qname = (uint16_t)l_qname; b->core.l_extranul = 2; b->core.n_cigar = (uint32_t)cigar.size(); b->core.l_qseq = (int32_t)l_qseq;
    return new SAMRecord(b, nullptr, true);          // never destroyed: the harness ends with the process
}

// What altQuals (Mutect2Engine.cpp:91-111, with :114-127) appends for one read at one position, 0 where it appends nothing.  Every
// question about the read is put to the reference's PeUtils and SAMRecord.
uint8_t indel_quality(int length) { return (uint8_t)std::min(30 + 10 * (length - 1), 127); }
uint8_t alt_quality(SAMRecord* rec, int pos, char ref_base, int pcr_error_qual, int min_q) {
    PeUtils at(rec, pos);
    const int indel = at.isDeletion() ? at.getCurrentCigarElement()->getLength() : at.getLengthOfImmediatelyFollowingIndel();
    if (indel > 0) return indel_quality(indel);
    const int here = at.getOffset();
    const bool clip_before = at.isAfterSoftClip() && at.getBaseQuality(here - 1) > min_q, clip_behind = at.isBeforeSoftClip() && at.getBaseQuality(here + 1) > min_q;
    if (at.getQual() > min_q && (clip_behind || clip_before)) return indel_quality(1);
    if (at.getBase() == ref_base || !(at.getQual() > min_q)) return 0;
    const bool has_mate = rec->isProperlyPaired() && !rec->mateIsUnmapped();
    const int mate_start = has_mate ? rec->getMateStart() : INT32_MAX;
    const bool under_mate = mate_start <= pos && pos < mate_start + rec->getLength();
    return (uint8_t)(under_mate ? std::min((int)at.getQual(), pcr_error_qual / 2) : (int)at.getQual());
}
// logLikelihoodRatio (:133-150) with repeatFactor 1, on the reference's digamma / log10Factorial caches and its error-probability table
double log_odds_of(int n_ref, const std::vector<uint8_t>& alt) {
    const int n_alt = (int)alt.size();
    const double f_tilde = std::exp(DIGAMMA.get(n_ref + 1) - DIGAMMA.get(n_alt + 1));
    const double beta_entropy = (-LOG_10_FACTORIAL.get(n_ref + n_alt + 1) + LOG_10_FACTORIAL.get(n_alt) + LOG_10_FACTORIAL.get(n_ref)) * std::log(10);
    double sum = 0;
    for (uint8_t q : alt) {
        const double eps = QualityUtils::qualToErrorProb(q), log_eps = (double)q * PHRED_TO_LOG_ERROR_PROB_FACTOR;
        const double z = (1 - eps) / (1 - eps + eps * f_tilde);
        sum += z * (log1mexp(log_eps) - log_eps) + fastBernoulliEntropy(z);
    }
    return beta_entropy + sum;
}
void print_double(double v) { if (std::isnan(v)) printf("nan"); else printf("%a", v); }
struct Row { SAMRecord* rec; int act_start, act_stop, sample; };
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    QualityUtils::initial();
    if (!strcmp(argv[1], "tables")) {
        const int n = atoi(argv[2]);
        for (int k = 0; k < n; ++k) { print_double(k ? DIGAMMA.get(k) : std::nan("")); printf(" "); print_double(LOG_10_FACTORIAL.get(k)); printf("\n"); }
        for (int q = 0; q < 128; ++q) {
            print_double(QualityUtils::qualToErrorProb((uint8_t)q)); printf(" "); print_double(q * PHRED_TO_LOG_ERROR_PROB_FACTOR); printf(" ");
            print_double(log1mexp(q * PHRED_TO_LOG_ERROR_PROB_FACTOR)); printf("\n");
        }
        return 0;
    }
    std::ifstream f(argv[2]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string word, ref;
        int interval_start, n_loci, has_normal, ggs, min_callable, pcr, min_q; size_t n_reads; double initial;
        ss >> word >> interval_start >> n_loci >> ref >> n_reads >> has_normal >> ggs >> min_callable >> pcr >> min_q >> initial;
        if (!ss || word != "case" || min_q != MINIMUM_BASE_QUALITY) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        std::vector<Row> rows(n_reads);
        for (auto& r : rows) {
            if (!std::getline(f, line)) return 2;
            std::istringstream rs(line);
            int start, mate_start, flags; size_t n_cigar; std::string bases, quals;
            rs >> start >> mate_start >> flags >> r.sample >> r.act_start >> r.act_stop >> n_cigar;
            std::vector<uint32_t> cg(n_cigar);
            for (auto& e : cg) rs >> e;
            rs >> bases >> quals;
            if (!rs) { fprintf(stderr, "bad read: %s\n", line.c_str()); return 2; }
            if (bases == "-") { bases.clear(); quals.clear(); }
            std::vector<uint8_t> q(bases.size());
            for (size_t i = 0; i < q.size(); ++i) q[i] = (uint8_t)strtoul(quals.substr(2 * i, 2).c_str(), nullptr, 16);
            r.rec = make_record(start, mate_start, (uint16_t)flags, cg, bases, q);
        }
        // the pileups: per locus, in read order, (sample, what altQuals appends or 0)
        std::vector<std::vector<std::pair<int, uint8_t>>> piles(n_loci);
        printf("E ");
        for (auto& r : rows)
            for (int pos = r.act_start; pos <= r.act_stop; ++pos) {
                uint8_t b = 0;
                if (pos >= interval_start && pos < interval_start + n_loci) {
                    b = alt_quality(r.rec, pos, (char)ref[pos - interval_start], pcr, min_q);
                    piles[pos - interval_start].emplace_back(r.sample, b);
                }
                printf("%02x", b);
            }
        printf("\nL %d\n", n_loci);
        for (int l = 0; l < n_loci; ++l) {                                                 // isActive, :58-88
            std::vector<uint8_t> tumour_alt;
            int n_tumour = 0, n_normal = 0, n_normal_alt = 0;
            double normal_sum = 0;
            for (auto& e : piles[l]) {
                if (e.first == 0) { n_tumour++; if (e.second) tumour_alt.push_back(e.second); }
                else { n_normal++; if (e.second) { n_normal_alt++; normal_sum += e.second; } }
            }
            const double log_odds = tumour_alt.empty() ? std::nan("") : log_odds_of(n_tumour - (int)tumour_alt.size(), tumour_alt);
            const bool vetoed = has_normal && !ggs && n_normal_alt > n_normal * 0.3 && normal_sum > 100;
            const int active = !tumour_alt.empty() && !(log_odds < initial) && !vetoed;
            printf("%d %d ", active, n_tumour + n_normal); print_double(log_odds); printf("\n");
        }
        printf("end\n");
    }
    return 0;
}
