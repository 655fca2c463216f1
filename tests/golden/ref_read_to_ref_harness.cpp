// ref_read_to_ref_harness.cpp -- calls the reference's own AlignmentUtils functions in the order of createReadAlignedToRef lines
// 505-543 (read/AlignmentUtils.cpp) on cases read from a text file.  The function itself needs SAMRecord and Haplotype objects and
// with them half of the reference's tree; its body between the aligner call and the return is this sequence of calls.  Built by
// tests/golden/make_golden_read_to_ref.py against the reference's sources where they lie; nothing of it is linked into the product.
//
// input, one case per line:   offset hap_start reference_start n_sw e.. n_hap e.. ref read        (elements len << 4 | BAM op, "-" = empty)
// output, one line per case:  status start n e..        status 0 = a result, 2 = the original read is returned, 3 = the reference throws
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "AlignmentUtils.h"
#include "CigarUtils.h"
#include "Mutect2Utils.h"
#include "SWParameters.h"

void Mutect2Utils::validateArg(bool condition, const std::string& msg) {
    if (!condition) throw std::invalid_argument(msg);
}
const SWParameters CigarUtils::ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS(10, -15, -30, -5);

namespace {
struct Open : AlignmentUtils {
    using AlignmentUtils::applyCigarToCigar;
    using AlignmentUtils::calcFirstBaseMatchingReferenceInCigar;
};

// the reference's enum is M I D N S H P X EQ; BAM's codes are M I D N S H P = X
const int kBamOfEnum[9] = {0, 1, 2, 3, 4, 5, 6, 8, 7};

std::shared_ptr<Cigar> cigar_of(const std::vector<uint32_t>& el) {
    std::vector<CigarElement> v;
    for (uint32_t e : el) v.emplace_back(CigarElement((int)(e >> 4), CigarOperatorUtils::binaryToEnum((int)(e & 15))));
    return std::make_shared<Cigar>(v);
}
std::shared_ptr<uint8_t[]> bytes_of(const std::string& s) {
    std::shared_ptr<uint8_t[]> p(new uint8_t[s.size() + 1]);
    memcpy(p.get(), s.data(), s.size());
    return p;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        int offset, hap_start, reference_start;
        size_t n;
        ss >> offset >> hap_start >> reference_start >> n;
        std::vector<uint32_t> sw(n);
        for (auto& e : sw) ss >> e;
        ss >> n;
        std::vector<uint32_t> hap(n);
        for (auto& e : hap) ss >> e;
        std::string ref, read;
        ss >> ref >> read;
        if (ref == "-") ref.clear();
        if (read == "-") read.clear();
        if (!ss) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        if (offset == -1) { printf("2 0 0\n"); continue; }                                       // :500-503
        try {
            auto swCigar = AlignmentUtils::consolidateCigar(cigar_of(sw));                       // :505
            auto extendedHaplotypeCigar = cigar_of(hap);                                         // Haplotype::getConsolidatedPaddedCigar(1000)
            extendedHaplotypeCigar->add(CigarElement(1000, CigarOperator::M));
            extendedHaplotypeCigar = AlignmentUtils::consolidateCigar(extendedHaplotypeCigar);
            int readStartOnHaplotype = Open::calcFirstBaseMatchingReferenceInCigar(extendedHaplotypeCigar, offset);       // :516
            int readStartOnReference = reference_start + hap_start + readStartOnHaplotype;
            auto haplotypeToRef = AlignmentUtils::trimCigarByBases(extendedHaplotypeCigar, offset, extendedHaplotypeCigar->getReadLength() - 1);
            auto raw = Open::applyCigarToCigar(swCigar, haplotypeToRef);
            auto clean = AlignmentUtils::cleanUpCigar(raw);
            auto fin = AlignmentUtils::leftAlignIndel(clean, bytes_of(ref), (int)ref.size(), bytes_of(read), (int)read.size(),
                                                      readStartOnHaplotype, 0, true);            // :524
            int leadingDeletions = clean->getReferenceLength() - fin->getReferenceLength();
            if (fin->getReadLength() != (int)read.size()) throw std::exception();                // :543
            printf("0 %d %d", readStartOnReference + leadingDeletions, fin->numCigarElements());
            for (auto& ce : fin->getCigarElements()) printf(" %u", (unsigned)ce.getLength() << 4 | (unsigned)kBamOfEnum[(int)ce.getOperator()]);
            printf("\n");
        } catch (...) {
            printf("3 0 0\n");
        }
    }
    return 0;
}
