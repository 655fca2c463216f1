// pairhmm_etab_driver.cpp -- csrc/pairhmm_etab.h on its own, for AddressSanitizer + UBSan (tests/test_pairhmm_etab_host.py).
// For every RPL 1..16, CODES 4 and 5 and both layouts it prints the layout -- size, the read list of a column, the offset of every
// (row, code, lane) -- and then does what the kernels do with it on a heap block of exactly the wave's bytes: builds the table with
// the stores of the kernel's build loop (16-, 8- or 4-byte, at the read list's addresses), reads every column back with the read
// list's loads and compares with the value that belongs there.  One byte past the block, or a misaligned 16-byte access, aborts.
// It also prints which layout every instantiated class (G, RPL, CODES) takes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "pairhmm_etab.h"

using namespace mgx_hmm_etab;

static float value_of(int row, int code, int lane) { return (float)(1 + row + 100 * code + 1000 * lane); }

// the kernel's table build and column loads; returns the number of mismatches
static int simulate(int rpl, int codes, bool quads) {
    const int bytes = bytes_per_wave(rpl, codes);
    // new[] of float4-sized units: 16-byte aligned like the kernels' dynamic LDS, and exactly `bytes` long
    struct alignas(16) Unit { uint8_t b[16]; };
    std::unique_ptr<Unit[]> block(new Unit[(size_t)bytes / 16]);
    uint8_t* etab = block[0].b;
    std::memset(etab, 0xFF, (size_t)bytes);
    for (int lane = 0; lane < kLanes; ++lane)
        for (int k = 0; k < n_reads(rpl, quads); ++k) {
            const Read rd = read_of(rpl, codes, quads, k);
            for (int code = 0; code < codes; ++code) {
                uint8_t* q = etab + rd.offset + lane * rd.bytes + code * rd.code_stride;
                float v[4];
                for (int t = 0; t < 4; ++t) v[t] = value_of(rd.row0 + t, code, lane);
                if (rd.bytes == kQuadBytes) {
                    if (reinterpret_cast<uintptr_t>(q) % 16) return -1;
                    std::memcpy(q, v, 16);
                } else if (rd.row0 + 1 < rpl) {
                    std::memcpy(q, v, 8);
                } else {
                    std::memcpy(q, v, 4);
                }
            }
        }
    int bad = 0;
    for (int lane = 0; lane < kLanes; ++lane)
        for (int code = 0; code < codes; ++code) {
            int seen[64] = {0};
            for (int k = 0; k < n_reads(rpl, quads); ++k) {
                const Read rd = read_of(rpl, codes, quads, k);
                const uint8_t* q = etab + rd.offset + lane * rd.bytes + code * rd.code_stride;
                float v[4] = {0, 0, 0, 0};
                if (rd.bytes == kQuadBytes && reinterpret_cast<uintptr_t>(q) % 16) return -1;
                std::memcpy(v, q, (size_t)rd.bytes);
                for (int t = 0; t < rd.bytes / 4; ++t) {
                    const int row = rd.row0 + t;
                    if (row >= rpl) continue;
                    seen[row]++;
                    float direct;
                    std::memcpy(&direct, etab + etab_offset(rpl, codes, quads, row, code, lane), 4);
                    bad += v[t] != value_of(row, code, lane) || direct != v[t];
                }
            }
            for (int row = 0; row < rpl; ++row) bad += seen[row] != 1;
        }
    return bad;
}

int main() {
    for (int rpl = 1; rpl <= 16; ++rpl)
        for (int codes = 4; codes <= 5; ++codes)
            for (int quads = 0; quads <= 1; ++quads) {
                const bool q = quads != 0;
                printf("layout %d %d %d %d %d %d\n", rpl, codes, quads, bytes_per_wave(rpl, codes), n_reads(rpl, q), n_quads(rpl, q));
                for (int k = 0; k < n_reads(rpl, q); ++k) {
                    const Read rd = read_of(rpl, codes, q, k);
                    printf("read %d %d %d %d %d %d %d %d\n", rpl, codes, quads, k, rd.offset, rd.bytes, rd.code_stride, rd.row0);
                }
                for (int row = 0; row < 2 * row_pairs(rpl); ++row)
                    for (int code = 0; code < codes; ++code) {
                        printf("off %d %d %d %d %d", rpl, codes, quads, row, code);
                        for (int lane = 0; lane < kLanes; ++lane) printf(" %d", etab_offset(rpl, codes, q, row, code, lane));
                        printf("\n");
                    }
                printf("sim %d %d %d %d\n", rpl, codes, quads, simulate(rpl, codes, q));
            }
    const int widths[4] = {4, 8, 16, 64};
    for (int G : widths)
        for (int rpl = 1; rpl <= 16; ++rpl)
            for (int codes = 4; codes <= 5; ++codes) printf("class %d %d %d %d\n", G, rpl, codes, quad_layout(G, rpl, codes) ? 1 : 0);
    return 0;
}
