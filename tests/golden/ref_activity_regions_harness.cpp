// ref_activity_regions_harness.cpp -- the reference's own ActivityProfile.cpp and ActivityProfileState.cpp, compiled where they lie, driven as
// M2/main.cpp:267-328 drives them over the cases tests/activity_region_cases.py writes.  The pop cadence, the cut and the accumulation
// into the state list are compiled reference code.  BandPassActivityProfile.cpp reaches boost/multi_array.hpp through MathUtils.h and
// SimpleInterval.cpp / AssemblyRegion.cpp include boost/utility.hpp, which this build does not have, so restated here are: the 20 lines of
// the band-pass subclass (processState, makeKernel, determineFilterSize, getMaxProbPropagationDistance, with MathUtils.cpp:29-52), the
// SimpleInterval members the two compiled files call (SimpleInterval.cpp:18-31,76-78), AssemblyRegion's constructor and destructor
// (AssemblyRegion.cpp:13-23,52 with IntervalUtils.cpp:9-23; it records what it is given) and SAMSequenceRecord's constructor, through
// which the header gets its sequence length.  Built by tests/golden/make_golden_activity_regions.py; nothing of it is linked into the
// product.
//   ref_activity_regions <file>     per case "R n", n lines "start end ext_start ext_end", "V values", "K weights", "end" (hex floats)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "ActivityProfile.h"
#include "ActivityProfileState.h"
#include "AssemblyRegion.h"
#include "SimpleInterval.h"
#include "samtools/SAMFileHeader.h"

// ---- what the compiled files need from outside
SimpleInterval::SimpleInterval(int contig, int start, int end) : start(start), end(end), contig(contig) {
    if (contig == -1 || start < 0 || start > end) throw std::invalid_argument("SimpleInterval::validatePositions failed.");
}
SimpleInterval::SimpleInterval(SimpleInterval const& o) : start(o.start), end(o.end), contig(o.contig) {}
SimpleInterval::SimpleInterval() : start(0), end(0), contig(-1) {}
void SimpleInterval::clearContig() { this->contig = -1; }
SAMSequenceRecord::SAMSequenceRecord(std::string& name, int sequenceLength) : mSequenceIndex(0), mSequenceLength(sequenceLength), mSequenceName(name) {}

AssemblyRegion::AssemblyRegion(SimpleInterval const& activeRegionLoc, std::vector<std::shared_ptr<ActivityProfileState>> supportingStates, const bool isActive,
                               const int extension, SAMFileHeader* header)
    : header(header), supportingStates(std::move(supportingStates)), activeRegionLoc(std::make_shared<SimpleInterval>(activeRegionLoc)), extension(extension),
      isActive(isActive) {
    const int contigLength = header->getSequenceDictionary().getSequences()[activeRegionLoc.getContigInt()].getSequenceLength();
    const int boundedStart = std::max(0, activeRegionLoc.getStart() - extension), boundedStop = std::min(contigLength - 1, activeRegionLoc.getEnd() + extension);
    if (!(boundedStart >= contigLength || boundedStop < 0)) extendedLoc = std::make_shared<SimpleInterval>(activeRegionLoc.getContigInt(), boundedStart, boundedStop);
    spanIncludingReads = extendedLoc;
}
AssemblyRegion::~AssemblyRegion() = default;

namespace {
// BandPassActivityProfile.cpp, restated against the compiled base class
class BandPass : public ActivityProfile {
public:
    std::vector<double> kernel;
    int filterSize;
    std::vector<std::shared_ptr<ActivityProfileState>> out;
    std::map<int, double> left;          // position -> the value its state had when last seen in the list, i.e. when it was popped

    BandPass(int maxProbPropagationDistance, double activeProbThreshold, const std::vector<double>& weights, SAMFileHeader* header)
        : ActivityProfile(maxProbPropagationDistance, activeProbThreshold, header), kernel(weights), filterSize((int)(weights.size() - 1) / 2) {}

    static double normalDistribution(double mean, double sd, double x) { return exp(-(x - mean) * (x - mean) / (2.0 * sd * sd)) / (sd * sqrt(2.0 * M_PI)); }
    static std::vector<double> makeKernel(int filterSize, double sigma) {
        const int bandSize = (filterSize << 1) + 1;
        std::vector<double> k;
        for (int i = 0; i < bandSize; i++) k.push_back(normalDistribution(filterSize, sigma, i));
        double sum = 0.0;
        for (auto& e : k) sum += e;
        for (auto& e : k) e = e / sum;
        return k;
    }
    static int determineFilterSize(const std::vector<double>& k, double minProbToKeepInFilter) {
        const int middle = (int)(k.size() - 1) >> 1;
        int filterEnd = middle;
        while (filterEnd > 0) {
            if (k[filterEnd - 1] < minProbToKeepInFilter) break;
            filterEnd--;
        }
        return middle - filterEnd;
    }
    std::vector<std::shared_ptr<ActivityProfileState>>* processState(const std::shared_ptr<ActivityProfileState>& justAddedState) override {
        const double activeProb = justAddedState->isActiveProb();
        if (activeProb > 0.0) {
            for (int i = -filterSize; i <= filterSize; i++) {
                optional<SimpleInterval> loc = getLocForOffset(justAddedState->getLoc(), i);
                if (loc.has_value()) out.emplace_back(std::make_shared<ActivityProfileState>(loc.value(), activeProb * kernel[i + filterSize]));
            }
        } else {
            out.emplace_back(justAddedState);
        }
        return &out;
    }
    int getMaxProbPropagationDistance() override { return maxProbPropagationDistance + filterSize; }
    void look() { for (auto& s : stateList) left[s->getLoc().getStart()] = s->isActiveProb(); }
};

std::vector<double> numbers(const std::string& line, char tag) {
    std::istringstream ss(line);
    std::string word;
    ss >> word;
    if (word.size() != 1 || word[0] != tag) { fprintf(stderr, "expected %c: %.40s\n", tag, line.c_str()); exit(2); }
    std::vector<double> v;
    while (ss >> word) v.push_back(strtod(word.c_str(), nullptr));
    return v;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string word, thr;
        int first, n_loci, contig, prop, padding, mn, mx, n_w;
        ss >> word >> first >> n_loci >> contig >> prop >> thr >> padding >> mn >> mx >> n_w;
        if (!ss || word != "case") { fprintf(stderr, "bad line: %.60s\n", line.c_str()); return 2; }
        std::getline(in, line);
        std::vector<double> w = numbers(line, 'W');
        std::getline(in, line);
        const std::vector<double> p = numbers(line, 'P');
        if ((int)w.size() != n_w || (int)p.size() != n_loci) return 2;
        if (w.empty()) w = BandPass::makeKernel(BandPass::determineFilterSize(BandPass::makeKernel(50, 17.0), 1e-5), 17.0);          // main.cpp:197
        // a header whose one sequence has the case's length: zeroed storage (its constructor is not built), the dictionary's vector filled
        SAMFileHeader* header = (SAMFileHeader*)calloc(1, sizeof(SAMFileHeader));
        std::string name = "chr1";
        header->getSequenceDictionary().getSequences().push_back(SAMSequenceRecord(name, contig));
        BandPass profile(prop, strtod(thr.c_str(), nullptr), w, header);
        std::vector<std::shared_ptr<AssemblyRegion>> regions;
        for (int l = 0; l < n_loci; ++l) {                                              // main.cpp:267-291
            const int pos = first + l;
            if (!profile.isEmpty()) {
                const bool forceConversion = pos != profile.getEnd() + 1;
                profile.look();
                for (auto& r : *profile.popReadyAssemblyRegions(padding, mn, mx, forceConversion)) regions.push_back(r);
            }
            profile.add(std::make_shared<ActivityProfileState>(0, pos, p[l]));
        }
        while (!profile.isEmpty()) {                                                    // main.cpp:320-328
            profile.look();
            for (auto& r : *profile.popReadyAssemblyRegions(padding, mn, mx, true)) regions.push_back(r);
        }
        printf("R %zu\n", regions.size());
        for (auto& r : regions) printf("%d %d %d %d\n", r->getStart(), r->getEnd(), r->getExtendedSpan()->getStart(), r->getExtendedSpan()->getEnd());
        printf("V");
        for (auto& kv : profile.left) printf(" %a", kv.second);
        printf("\nK");
        for (double x : w) printf(" %a", x);
        printf("\nend\n");
    }
    return 0;
}
