// read_to_ref_driver.cpp -- csrc/read_to_ref_rule.h on the CPU (tests/test_read_to_ref_host.py; -Werror, ASan + UBSan).
// Every case runs three ways: serially with the window comparison, with the kernel's grouping of that comparison (64 strided lanes
// joined by an OR), and serially comparing the whole alternative strings.  All buffers are heap blocks of exactly the stated sizes,
// so that a read or a store outside them is an error here.
//
// input, one case per line:   hard_lead hard_trail stride offset hap_start reference_start n_sw e.. n_hap e.. ref read   ("-" = empty)
// output, three lines per case (serial, lanes, whole):   status start n e..      (elements only for status 0)
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "read_to_ref_rule.h"

namespace R = mgx_to_ref_rule;

// the kernel's grouping: lane l takes lo + l, lo + l + 64, ...; the lanes' answers are joined as a ballot joins them
struct LanesAny {
    template <class P> bool operator()(int64_t lo, int64_t hi, P pred) const {
        bool lanes[64];
        for (int l = 0; l < 64; ++l) {
            lanes[l] = false;
            for (int64_t j = lo + l; j < hi; j += 64) if (pred(j)) { lanes[l] = true; break; }
        }
        bool any = false;
        for (bool b : lanes) any |= b;
        return any;
    }
};

struct RowStore {
    std::vector<uint32_t>* row;
    void operator()(uint32_t k, uint32_t e) const { if (k < row->size()) (*row)[k] = e; }
};

template <class Any> void run(const R::Input& in, uint32_t stride, Any any, bool whole) {
    std::vector<uint32_t> row(stride, 0xFFFFFFFFu);
    const R::Result r = R::read_to_ref(in, stride, RowStore{&row}, any, whole);
    const bool placed = r.status == R::kOk || r.status == R::kNoRoom;
    printf("%u %d %u", (unsigned)r.status, placed ? r.start : 0, placed ? r.n : 0u);
    if (r.status == R::kOk) for (uint32_t k = 0; k < r.n; ++k) printf(" %u", row[k]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        R::Input in{};
        uint32_t stride;
        size_t n;
        ss >> in.hard_lead >> in.hard_trail >> stride >> in.offset >> in.hap_start >> in.reference_start >> n;
        std::vector<uint32_t> sw(n);
        for (auto& e : sw) ss >> e;
        ss >> n;
        std::vector<uint32_t> hap(n);
        for (auto& e : hap) ss >> e;
        std::string ref_s, read_s;
        ss >> ref_s >> read_s;
        if (!ss) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        if (ref_s == "-") ref_s.clear();
        if (read_s == "-") read_s.clear();
        const std::vector<uint8_t> ref(ref_s.begin(), ref_s.end()), read(read_s.begin(), read_s.end());
        in.sw = sw.data(); in.n_sw = (uint32_t)sw.size(); in.hap = hap.data(); in.n_hap = (uint32_t)hap.size();
        in.ref = ref.data(); in.ref_len = (uint32_t)ref.size(); in.read = read.data(); in.read_len = (uint32_t)read.size();
        run(in, stride, R::SerialAny{}, false);
        run(in, stride, LanesAny{}, false);
        run(in, stride, R::SerialAny{}, true);
    }
    return 0;
}
