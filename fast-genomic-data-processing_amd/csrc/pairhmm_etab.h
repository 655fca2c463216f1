// pairhmm_etab.h -- where the fp32 PairHMM kernels (pairhmm_kernels.hip.inc) keep a wavefront's emission table in LDS.
// Plain C++17, constexpr, no HIP: the kernels build and read the table through it, and tests/cpp/pairhmm_etab_driver.cpp
// walks it on the CPU (tests/test_pairhmm_etab_host.py: injective, inside the wave's bytes, aligned, conflict-free).
//
// A lane keeps RPL rows; the table holds, per row and haplotype code, the row's emission for that code, and a lane
// fetches all its rows of ONE code per column.  The rows are cut into RP2 = ceil(RPL / 2) row pairs:
//   * quad layout: RPL / 4 QUAD tables first, each [code][lane][4 rows] -- 16 bytes per lane, 1024 bytes per code, one
//     ds_read_b128 per quad -- and the remaining 1..3 rows in one or two trailing PAIR tables [code][lane][2 rows] --
//     8 bytes per lane, 512 bytes per code, one ds_read_b64 (ds_read_b32 for a single row) each.  Only FULL quads: the
//     compiler narrows the read of a quad of three rows to ds_read_b96, which takes the LDS pipe 8 cycles, against 2 + 2
//     for the ds_read_b64 and ds_read_b32 of two pair tables (reads of different widths are not fused);
//   * pair layout (what every class had before the quads): RP2 pair tables.
// Both take RP2 * CODES * 512 bytes per wavefront, which is what pairhmm_plan.h's lds_bytes() books.
// Why quads: two 8-byte reads whose tables lie a multiple of 512 bytes apart are fused by the compiler into one
// ds_read2st64_b64, which moves 128 bytes per clock of the CU's LDS pipe (8 cycles per wavefront instruction);
// ds_read_b128 moves 256 (4 cycles), so the same 16 bytes per lane cost half the LDS time.  A lone ds_read_b64 also
// runs at 256 bytes per clock.
// Banks (64 of 4 bytes; a ds_read_b128 is served in four groups of 16 lanes, a ds_read_b64 in two of 32): the code
// strides are multiples of 256 bytes, so the bank does not depend on the code a lane asks for, and within a group
// lane * 16 (or lane * 8) bytes fall on distinct banks: conflict-free whatever codes the lanes hold.
#pragma once

namespace mgx_hmm_etab {

constexpr int kLanes = 64;
constexpr int kPairBytes = 8, kQuadBytes = 16;                       // per lane and code
constexpr int kPairCodeStride = kLanes * kPairBytes;                 // 512
constexpr int kQuadCodeStride = kLanes * kQuadBytes;                 // 1024

constexpr int row_pairs(int rpl) { return (rpl + 1) / 2; }
constexpr int bytes_per_wave(int rpl, int codes) { return row_pairs(rpl) * codes * kPairCodeStride; }

// Which classes take the quad layout: those whose rows are all in quads, RPL = 4, 8, 12, 16, whatever G and CODES.  A
// mixed table needs a second lane address and a second "code * stride" per column -- one more VALU instruction per
// column and one more register -- and the kernels are bound by vector issue before they are bound by LDS: measured on
// an MI355X, the mixed classes lost (reads of 100 bases, 7 rows per lane: +1.5 %; reads of 151 bases, 10 rows per lane,
// five codes: +1.0 %; profiles/pairhmm_etab_b128_ab.txt), and with 7 rows per lane the kernels held to 128 registers
// gain 4 to 12 bytes of scratch.  They keep the pair layout.  (G and CODES are parameters so that a class can be
// taken out on its own.)
constexpr bool quad_layout(int G, int rpl, int codes) {
    (void)G; (void)codes;
    return rpl % 4 == 0;
}

constexpr int n_quads(int rpl, bool quads) { return quads ? rpl / 4 : 0; }
constexpr int n_reads(int rpl, bool quads) { return row_pairs(rpl) - n_quads(rpl, quads); }      // LDS reads per column

// Read k of a column: `bytes` per lane at `offset` + code * `code_stride` + lane * `bytes` from the wave's table,
// delivering the rows [row0, row0 + bytes / 4) (those below RPL: the last pair of an odd RPL holds one row).
struct Read {
    int offset, bytes, code_stride, row0;
};
constexpr Read read_of(int rpl, int codes, bool quads, int k) {
    const int nq = n_quads(rpl, quads);
    if (k < nq) return Read{k * codes * kQuadCodeStride, kQuadBytes, kQuadCodeStride, 4 * k};
    return Read{nq * codes * kQuadCodeStride + (k - nq) * codes * kPairCodeStride, kPairBytes, kPairCodeStride, 4 * nq + 2 * (k - nq)};
}
// the read that delivers `row`
constexpr int read_index(int rpl, bool quads, int row) {
    const int nq = n_quads(rpl, quads);
    return row < 4 * nq ? row / 4 : nq + (row - 4 * nq) / 2;
}
// byte offset of e(row of `lane`, code) in the wave's table
constexpr int etab_offset(int rpl, int codes, bool quads, int row, int code, int lane) {
    const Read r = read_of(rpl, codes, quads, read_index(rpl, quads, row));
    return r.offset + code * r.code_stride + lane * r.bytes + (row - r.row0) * 4;
}

template <int RPL, int CODES, bool QUADS>
struct Layout {
    static constexpr int kQuads = n_quads(RPL, QUADS), kReads = n_reads(RPL, QUADS), kBytes = bytes_per_wave(RPL, CODES);
    static constexpr bool kQuadLayout = QUADS;
    static_assert(kBytes % kQuadBytes == 0, "every wavefront's table starts 16-byte aligned");
    static_assert(kQuads == 0 || read_of(RPL, CODES, QUADS, kQuads - 1).offset % kQuadBytes == 0, "quad tables are 16-byte aligned");
    static_assert(read_of(RPL, CODES, QUADS, kReads - 1).offset + CODES * read_of(RPL, CODES, QUADS, kReads - 1).code_stride == kBytes,
                  "the tables fill the wavefront's bytes exactly");
    static_assert(kPairCodeStride % 256 == 0 && kQuadCodeStride % 256 == 0, "the bank of an entry does not depend on its code");
};

}  // namespace mgx_hmm_etab
