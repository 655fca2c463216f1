// pairhmm_cell_driver.cpp -- runs the host emulation of the PairHMM cells (tools/cell_emulator.cpp over csrc/pairhmm_cell.h) on a small
// batch read from a file, for tests/test_pairhmm_cell_host.py, which builds this with -Werror under AddressSanitizer + UBSan and compares
// what it prints with what the optimised shared library returns.
// Input (whitespace-separated decimals): n, then per test case R H, R bytes each of bases, qual, ins, del, gcp, and H haplotype bytes.
// Output: "res <form> <test case> <fp32 bits, hex>" for forms 1..4 and "way <test case> <path code>" of form 4.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void cell_emulate_batch(int form, int n, const uint32_t* pair_read, const uint32_t* pair_hap, const uint64_t* read_off,
                        const uint64_t* hap_off, const uint8_t* bases, const uint8_t* qual, const uint8_t* ins,
                        const uint8_t* del, const uint8_t* gcp, const uint8_t* hap, float* out_res);
void cell_emulate_paths(int n, uint8_t* out);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s batch.txt\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0) { std::fprintf(stderr, "bad count\n"); return 2; }
    std::vector<uint64_t> read_off(1, 0), hap_off(1, 0);
    std::vector<uint8_t> seq[5], hap;      // bases, qual, ins, del, gcp
    auto take = [&](std::vector<uint8_t>& dst, int count) {
        for (int i = 0; i < count; ++i) {
            int v = 0;
            if (std::fscanf(f, "%d", &v) != 1 || v < 0 || v > 255) return false;
            dst.push_back((uint8_t)v);
        }
        return true;
    };
    for (int k = 0; k < n; ++k) {
        int R = 0, H = 0;
        bool ok = std::fscanf(f, "%d %d", &R, &H) == 2 && R >= 0 && H >= 0;
        for (int a = 0; ok && a < 5; ++a) ok = take(seq[a], R);
        ok = ok && take(hap, H);
        if (!ok) { std::fprintf(stderr, "bad test case %d\n", k); return 2; }
        read_off.push_back(seq[0].size());
        hap_off.push_back(hap.size());
    }
    std::fclose(f);
    // a vector without elements may hand out a null pointer: one spare byte keeps every array addressable
    for (auto& v : seq) v.push_back(0);
    hap.push_back(0);
    std::vector<uint32_t> idx((size_t)n);
    for (int k = 0; k < n; ++k) idx[(size_t)k] = (uint32_t)k;
    std::vector<float> res((size_t)n);
    std::vector<uint8_t> way((size_t)n);
    for (int form = 1; form <= 4; ++form) {
        cell_emulate_batch(form, n, idx.data(), idx.data(), read_off.data(), hap_off.data(), seq[0].data(), seq[1].data(), seq[2].data(),
                           seq[3].data(), seq[4].data(), hap.data(), res.data());
        for (int k = 0; k < n; ++k) {
            uint32_t bits;
            std::memcpy(&bits, &res[(size_t)k], 4);
            std::printf("res %d %d %08x\n", form, k, bits);
        }
    }
    cell_emulate_paths(n, way.data());
    for (int k = 0; k < n; ++k) std::printf("way %d %d\n", k, (int)way[(size_t)k]);
    return 0;
}
