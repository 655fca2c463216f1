// pairhmm_kernels.hip.inc -- the CDNA4 (gfx950) PairHMM forward-recurrence kernels.
// Included by mgx_pairhmm.hip only.
//
// What is computed (deepmutect/Mutect2Cpp-master/src/intel/pairhmm/avx-pairhmm-template.h:
// 110-192, 204-345; SURVEY.md section 8a row A12): for read rows r = 1..R and haplotype
// columns c = 1..H
//     M[r][c] = ((M[r-1][c-1]*pMM_r + X[r-1][c-1]*pGAPM_r) + Y[r-1][c-1]*pGAPM_r) * e(r,c)
//     X[r][c] =   M[r-1][c]*pMX_r   + X[r-1][c]*pXX_r
//     Y[r][c] =   M[r][c-1]*pMY_r   + Y[r][c-1]*pYY_r
//     e(r,c)  = (read_r == hap_c or either is 'N') ? 1 - distm_r : distm_r / 3
// with row 0 = (0, 0, INITIAL/H), column 0 = (0, 0, 0), result = sum_c M[R][c] + sum_c X[R][c].
//
// How it is mapped onto a wavefront (this is NOT the reference's 8/16-row stripe scheme):
//   * A pair is owned by a GROUP of G lanes (G = 16: four pairs per wavefront, G = 64: one; G = 8 and G = 4
//     for reads of at most 64 / 32 bases: eight / sixteen pairs per wavefront, interleaved in the DPP rows).
//     Lane j of the group keeps RPL consecutive read rows in registers ("rows per lane"), so the
//     group covers up to G*RPL rows and a whole read is one pass -- no stripe hand-off.
//   * Time runs along anti-diagonals of LANES: at step d lane j processes haplotype column
//     d - j for all of its RPL rows, top to bottom.  Inside a lane every dependency is a
//     register of the previous column (or of the row just computed); between lanes only the
//     bottom row's (M, X, Y) moves, one lane to the right, with a DPP shift
//     (row_shr:1 for G = 16, wave_shr:1 for G = 64): 3 cross-lane moves per RPL cells (2 in the five-operation sweep,
//     where the bottom row evaluates what the next lane's top row needs of it: column5 below).
//   * Fill/drain costs nl-1 steps per pair (nl = lanes in use <= G) instead of 63: with G = 16
//     a 128x256 pair keeps 94 % of its lane-steps busy (80 % with two 64-row stripes).
//   * Rows are packed against the LAST used lane so that read row R is always that lane's
//     bottom row; the spare rows at the top of lane 0 are "row-0 clones" (all coefficients 0,
//     pYY = 1, Y = INITIAL/H) which reproduce the boundary row exactly.
//   * The haplotype is staged once per pair into LDS as base codes; each lane reads its own
//     column's code with one ds_read_u8 per step, prefetched one step ahead.
//   * The last-row sums are accumulated on the bottom row of every lane, in column order,
//     sumM and sumX apart, and read from lane nl-1 at the end (as the reference does).  (Five-operation sweep: read
//     row R makes the additions of sumM in its own, otherwise unread, y.)
//   * fp32 results < 1e-28f are appended to a re-run list; the same template instantiated for
//     double processes that list (IntelPairHmm.cc:338-350).
//   * The cell is not computed in the reference's 8-operation order but in an algebraically equal
//     one: 6 operations in fp32 (X scaled by pGAPM of the row below, Y carried divided by its own
//     row's pMY), 7 in fp64, and 5 in the first fp32 launch of the classes of up to 16 lanes (every row rescaled once more;
//     what that form cannot take goes to the N-haplotype list below).  pairhmm_cell.h states every form, its per-row
//     coefficients and the rules around them once, with the algebra; this file and the host emulation
//     (tools/cell_emulator.cpp) both compute with its functions, so the two round alike.

#include <type_traits>

#include "best_allele_rule.h"
#include "pairhmm_cell.h"      // the cell: model values, forms, coefficients, deferral rules, result and thresholds
#include "pairhmm_etab.h"      // the emission table's layout in LDS
#include "pairhmm_plan.h"      // Job, SeqRef, RegionRef, kMaxCodes, kMultiBins: what the host writes and these kernels read

namespace {

using namespace mgx_hmm_plan;
namespace etab = mgx_hmm_etab;
namespace cell = mgx_hmm_cell;
using cell::base_code;
using cell::kCodeN;
using Ar = cell::Bare;         // the arithmetic the cell functions take: the bare operations, flushed by the compile flags

struct KernelArgs {
    const Job* jobs;            // jobs of the batch
    const uint32_t* job_list;   // optional indirection (re-run list), indices into jobs
    const uint32_t* n_dyn;      // optional device-side job count (re-run list length)
    uint32_t n_static;          // job count when n_dyn == nullptr ...
    uint32_t job_first;         // ... and the first job of the launch (a bin is a contiguous job range)
    const uint8_t* bases;
    const uint8_t* qual;
    const uint8_t* ins;
    const uint8_t* del;
    const uint8_t* gcp;
    const uint8_t* hap_bases;
    const void* ph2pr;          // T[128]
    const void* mm;             // T[32640]
    const void* ph2pr_div3;     // T[128]: ph2pr[q] / 3 (the mismatch emission, avx-pairhmm-template.h:150)
    const void* gap_ratio;      // T[128]: ph2pr[q] / (1 - ph2pr[q]) (pXX / pGAPM of the scaled form; 0 at q = 0)
    double* out_log10;          // [n_pairs]
    uint8_t* used_f64;          // [n_pairs]
    uint32_t* rerun_list;       // fp32: jobs (indices into jobs) whose result underflowed -> re-run in fp64;
    uint32_t* rerun_count;      // fp64: jobs whose result is in reach of the flush-to-zero threshold -> exact re-run
    uint32_t* nhap_list;        // fp32 with the four-code table: jobs whose haplotype holds an N -> the five-code fp32
    uint32_t* nhap_count;       // launch of the same class (no result is written for them here)
    uint32_t* form_count;       // fp32 with the five-operation cell: how many jobs of those lists hold no N but were deferred for the cell form
    uint32_t lds_stride;        // bytes of LDS per group (>= max H of the bin + 2)
    void* strip_scratch;        // strip-mined class only: [workgroups][2][3][strip_stride] boundary rows (M, X, Y per column)
    uint32_t strip_stride;
    float log10_initial_f;
    double log10_initial_d;
};

constexpr int kCodePad = 7;

// base_code() of four bytes at once.  (b >> 1) & 7 is distinct for A C T G N (0 1 2 3 7), so two
// byte-permute lookups give the candidate code and the ASCII value it stands for; a byte that is not
// exactly that ASCII value (lower case, IUPAC, control bytes ...) gets code 0 like the reference's
// zero-initialised table.
__device__ __forceinline__ uint32_t base_code4(uint32_t w) {
    const uint32_t sel = (w >> 1) & 0x07070707u;
    const uint32_t code = __builtin_amdgcn_perm(0x04000000u, 0x03020100u, sel);      // idx 0..7 -> 0 1 2 3 0 0 0 4
    const uint32_t want = __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, sel);      // idx 0..7 -> A C T G . . . N
    const uint32_t diff = want ^ w;
    const uint32_t nz = (((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) & 0x80808080u;  // bit 7 set where the byte differs
    const uint32_t ok = ((nz ^ 0x80808080u) >> 7) * 0xFFu;                            // 0xFF where it matches
    return code & ok;
}

// Groups narrower than a DPP row (G = 8, 4) are INTERLEAVED in the row: group g of a row owns the lanes
// lr = g, g + S, g + 2S, ... (S = 16 / G), so the hand-off to the group's next lane is row_shr:S and the
// S lanes that have no source in the row -- exactly lane 0 of each group -- keep `old`, as for G = 16.
template <int G> constexpr int lane_stride() { return G < 16 ? 16 / G : 1; }

// One-lane shift towards higher lanes inside the group; the group's lane 0 keeps `old`.
template <int G>
__device__ __forceinline__ int dpp_shr1(int old, int v) {
    if constexpr (G == 64)
        return __builtin_amdgcn_update_dpp(old, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    else
        return __builtin_amdgcn_update_dpp(old, v, 0x110 + lane_stride<G>() /* row_shr:S */, 0xf, 0xf, false);
}
template <int G>
__device__ __forceinline__ float shr1(float old, float v) {
    return __builtin_bit_cast(float, dpp_shr1<G>(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v)));
}
template <int G>
__device__ __forceinline__ double shr1(double old, double v) {
    long long o = __builtin_bit_cast(long long, old), x = __builtin_bit_cast(long long, v);
    unsigned lo = (unsigned)dpp_shr1<G>((int)(unsigned)o, (int)(unsigned)x);
    unsigned hi = (unsigned)dpp_shr1<G>((int)(unsigned)(o >> 32), (int)(unsigned)(x >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}

// value held by the next lane of the group (the group's last lane gets its own value back)
template <int G, typename T>
__device__ __forceinline__ T shr1_down(T v) {
    const int lane = (int)(threadIdx.x & 63);
    constexpr int S = lane_stride<G>();
    const int j = G < 16 ? (lane & 15) / S : lane % G;
    const int src = (j == G - 1) ? lane : lane + S;
    return __shfl(v, src, 64);
}

// LDS emission table (fp32 kernels): holds e(row s of a lane, haplotype code) for every row, code and lane, so the per-cell
// compare+select becomes one conflict-free LDS read per four rows in the classes of 4, 8, 12 and 16 rows per lane
// (ds_read_b128 from a quad table [code][lane][4 rows], address "code*1024 + lane*16" plus an immediate offset) and per
// two rows in the others (ds_read_b64 from a pair table [code][lane][2 rows], "code*512 + lane*8").  pairhmm_etab.h is
// the layout: which class has which tables, their offsets, and why 16 bytes at a time (two 8-byte reads a multiple of
// 512 bytes apart become one ds_read2st64_b64, which takes the LDS pipe twice as long as a ds_read_b128).  Both layouts
// take ceil(RPL / 2) * CODES * 512 bytes per wavefront, which is what the host books (pairhmm_plan.h, lds_bytes).  (With
// the five-operation cell the entries are E = e * pMM of the row below, rounded once here; same layout, same size.)
// CODES (a template parameter of the body) is the number of code columns.  5: A C T G N  (PAD reads as N: harmless).
// 4: no column for N -- 8 KB instead of 10 KB per wavefront of eight rows per lane, so that the register budget and not
// LDS decides how many wavefronts a CU holds (16 instead of 14).  The first fp32 launch of every class but the
// strip-mined one has four columns; a test case whose haplotype holds an N gets no result from it and is appended to
// the class's N-haplotype list, which the five-column fp32 instantiation of the same class then works through (per
// test case, never per wavefront: a value does not depend on the batch it is in, nor on which launch computed it --
// both read the same table entries for A C T G).  fp64 has no table; its CODES stays 5.
template <int RPL, int CODES> constexpr int etab_bytes_per_wave() { return etab::bytes_per_wave(RPL, CODES); }

// The recurrence for the jobs of ONE class (G, RPL); `block` / `n_blocks` are the workgroup's index and count among
// the workgroups working on this class (the whole grid for a single-class launch).
// STRIP (reads longer than G * RPL rows, the strip-mined class): the read is cut into strips of G * RPL rows -- the
// first one takes the remainder, so that only it has row-0 clones -- which sweep the haplotype one after the other;
// a strip's bottom row (M, X, Y per column) goes to a boundary array in global memory and is what lane 0 of the next
// strip sees above its top row (the reference's shiftOutM/X/Y between its stripes, avx-pairhmm-template.h:253-300).
// EXACT (fp64, the last tier): the reference's operation order with every multiply and add rounded -- and flushed --
// on its own.  Flush-to-zero is on in the reference (IntelPairHmm.cc:230) and here, and a result within a few
// hundred orders of magnitude of 2^-1022 depends on WHICH intermediate products were flushed: the fused
// multiply-adds and the scaled form of the fast tiers flush at other points than the reference does.
// FIVE (fp32, four-code table, groups of up to 16 lanes -- reads of at most 192 bases): the five-operation cell is the
// only form of the sweep (pairhmm_cell.h); a test case it cannot take joins the N-haplotype list.
template <typename T, int G, int RPL, bool STRIP = false, bool EXACT = false, int CODES = kMaxCodes, bool FIVE = false>
__device__ __forceinline__ void pairhmm_body(const KernelArgs& a, uint8_t* smem, const uint32_t block, const uint32_t n_blocks) {
    constexpr int GPW = 64 / G;                   // groups per wavefront
    constexpr bool kETab = (sizeof(T) == 4);      // fp32: emission table in LDS; fp64: compare+select
    constexpr int kNumCodes = CODES;
    static_assert(CODES == 4 || CODES == kMaxCodes, "four or five code columns");
    static_assert(kETab || CODES == kMaxCodes, "fp64 has no table: the N code is compared");
    static_assert(!FIVE || (kETab && CODES == 4 && G <= kFiveOpMaxG && !STRIP && !EXACT), "the five-operation cell: first fp32 launch of the classes of up to 16 lanes");
    constexpr bool kSix = (sizeof(T) == 4) && !EXACT;   // fp32: the 6-operation cell; fp64: the scaled 7-operation cell (see sweep)
    using ETab = etab::Layout<RPL, CODES, kETab && etab::quad_layout(G, RPL, CODES)>;
    constexpr int S = lane_stride<G>();           // lane stride of a group inside its DPP row
    const int gpb = (int)blockDim.x / G;          // groups per block
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    // lane inside the group, and the group's index in the block (consecutive jobs -> consecutive groups)
    const int j = G < 16 ? (lane & 15) / S : lane % G;
    const int grp = wave * GPW + (G < 16 ? (lane >> 4) * S + (lane & 15) % S : lane / G);
    // LDS: [waves][etab] then [groups][hap codes]
    const int n_waves = (int)blockDim.x >> 6;
    uint8_t* etab_base = smem + (kETab ? (size_t)wave * etab_bytes_per_wave<RPL, CODES>() : 0);
    uint8_t* hapbuf = smem + (kETab ? (size_t)n_waves * etab_bytes_per_wave<RPL, CODES>() : 0) +
                      (size_t)grp * a.lds_stride;
    const T* __restrict__ ph2pr = (const T*)a.ph2pr;
    const T* __restrict__ mm = (const T*)a.mm;
    const T* __restrict__ ph2pr_div3 = (const T*)a.ph2pr_div3;
    const T* __restrict__ gap_ratio = (const T*)a.gap_ratio;
    const uint32_t n_jobs = a.n_dyn ? *a.n_dyn : a.n_static;

    for (uint32_t base = block * (uint32_t)gpb; base < n_jobs; base += n_blocks * (uint32_t)gpb) {
        const uint32_t slot = base + (uint32_t)grp;
        const bool live = slot < n_jobs;
        uint32_t job_idx = 0;
        Job job;
        job.read_off = 0; job.hap_off = 0; job.R = 0; job.H = 0; job.pair = 0; job.pad_ = 0;
        if (live) {
            job_idx = a.job_list ? a.job_list[slot] : a.job_first + slot;
            job = a.jobs[job_idx];
        }
        const int R = (int)job.R, H = (int)job.H;
        constexpr int kStripRows = G * RPL;
        const int n_strips = STRIP ? (R > kStripRows ? (R + kStripRows - 1) / kStripRows : 1) : 1;
        const int first_rows = R - (n_strips - 1) * kStripRows;     // rows of the first strip (all of them without STRIP)

        // ---- stage the haplotype into LDS as codes.  Layout of a group's buffer:
        //      [0, G) PAD | [G, G+H) codes | [G+H, stride) PAD, so lane j reads index d - j + G
        //      at step d with no clamping (stride >= max H of the bin + 2G + 8).
        __syncthreads();                          // previous iteration's readers are done
        bool hap_n = false;                       // (four-code table) this lane staged an N of the haplotype
        {
            const uint8_t* hp = a.hap_bases + job.hap_off;
            const int n_words = (int)a.lds_stride >> 2;            // stride is a multiple of 16
            uint32_t* hb32 = reinterpret_cast<uint32_t*>(hapbuf);
            for (int w = j; w < n_words; w += G) {
                const int c0 = 4 * w - G;                           // haplotype index of the word's first byte
                uint32_t packed;
                if (live && c0 >= 0 && c0 + 4 <= H) {
                    uint32_t raw;
                    __builtin_memcpy(&raw, hp + c0, 4);             // unaligned dword load
                    packed = base_code4(raw);
                } else {
                    packed = 0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int c = c0 + t;
                        const int code = (live && c >= 0 && c < H) ? base_code(hp[c]) : (kNumCodes > 4 ? kCodeN : 0);
                        packed |= (uint32_t)code << (8 * t);
                    }
                }
                if constexpr (kETab && kNumCodes == 4) {
                    const uint32_t x = packed ^ (0x01010101u * (uint32_t)kCodeN);      // a zero byte where the code is N
                    hap_n |= ((x - 0x01010101u) & ~x & 0x80808080u) != 0;
                    packed &= 0x03030303u;
                }
                hb32[w] = packed;
            }
        }
        bool group_hap_n = false;
        uint64_t gmask = ~0ull;                                    // the lanes of this lane's group
        if constexpr (G == 16) gmask = 0xFFFFull << (lane & 48);
        else if constexpr (G < 16) gmask = (uint64_t)((G == 8 ? 0x5555u : 0x1111u) << ((lane & 15) % S)) << (lane & 48);
        if constexpr (kETab && kNumCodes == 4) group_hap_n = (__ballot((int)hap_n) & gmask) != 0;

        T sumM = 0, sumX = 0;
        bool zero_gap = false;                            // some row has pGAPM == 0 (gcp byte 0)
        bool zero_mm = false;                             // (FIVE) some row has pMM == 0
        bool defer = group_hap_n;                         // the test case is left to the class's second launch
        T res_scale = 1;                                  // (FIVE) A' of this lane's bottom row: the last lane's turns sum x into sum X
        T dn_a = 0, dn_B = 0, dn_q = 0;                   // (FIVE) a, B', q' of the next lane's top row: what this lane's bottom row hands down with
        T paths0 = 0;                                     // (FIVE) group lane 0: the paths value its top row gets from the boundary row
        if constexpr (STRIP) {                            // every strip of a pair must take the same algebraic form
            for (int rr = lane; rr < R; rr += 64) zero_gap |= cell::row_needs_plain(a.gcp[job.read_off + (uint64_t)rr] & 127);
        }
        int nl = 0;
        T* const bnd = STRIP ? reinterpret_cast<T*>(a.strip_scratch) + (size_t)block * 6u * a.strip_stride : nullptr;
      for (int strip = 0; strip < n_strips; ++strip) {
        const int rows_here = (STRIP && strip > 0) ? kStripRows : first_rows;
        const int row_base = (STRIP && strip > 0) ? first_rows + (strip - 1) * kStripRows : 0;
        const bool last_strip = strip == n_strips - 1;
        nl = (rows_here + RPL - 1) / RPL;                 // lanes in use
        const int top_clones = nl * RPL - rows_here;      // spare rows at the top of lane 0 (first strip only)
        volatile T* const bcur = STRIP ? bnd + (size_t)(strip & 1) * 3u * a.strip_stride : nullptr;           // written by this strip
        const volatile T* const bprev = STRIP ? bnd + (size_t)((strip & 1) ^ 1) * 3u * a.strip_stride : nullptr;   // written by the previous one
        if (STRIP && strip > 0) __syncthreads();          // the previous strip's table readers are done, its boundary row is written

        // ---- per-row constants (ReadForPairHMM.cpp:62-80, avx-pairhmm-template.h:129-171)
        // k0..k4 hold, per row,   plain form:  pMM, pGAPM, pMX, pXX(=pYY), pMY
        //                         scaled form: pMM, A,     B,   C,         D      (see sweep)
        T k0[RPL], k1[RPL], k2[RPL], k3[RPL], k4[RPL], eM[RPL], eX[RPL];
        int rb[RPL];
        T pm[RPL], px[RPL], py[RPL];
        bool clone[RPL];
        T ratio[RPL];                                     // pXX / pGAPM per row (scaled form)
        const T init_y = cell::initial_y<Ar, T>(H);
#pragma unroll
        for (int s = 0; s < RPL; ++s) {
            const int rho = j * RPL + s - top_clones;     // 0-based read row, < 0: clone of row 0
            k0[s] = 0; k1[s] = 0; k2[s] = 0; k3[s] = 0; k4[s] = 0; eM[s] = 0; eX[s] = 0;
            rb[s] = 0; pm[s] = 0; px[s] = 0; py[s] = 0; clone[s] = false; ratio[s] = 0;
            if (live && j < nl) {
                if (rho < 0) {
                    clone[s] = true;
                    k3[s] = 1;                            // pYY = 1 keeps Y = INITIAL/H
                    py[s] = init_y;
                } else {
                    const uint64_t o = job.read_off + (uint64_t)(row_base + rho);
                    // (the 7-bit masks, pMM's index and the mismatch emission are pairhmm_cell.h's q7, pMM_of and mismatch_of written
                    // out: integer expressions moved into a function come back canonicalised otherwise, and with them the whole
                    // register allocation -- DESIGN.md 3.2)
                    const int qi = a.ins[o] & 127, qd = a.del[o] & 127, qc = a.gcp[o] & 127;
                    const int qq = a.qual[o] & 127;
                    const int mn = qi <= qd ? qi : qd, mx = qi <= qd ? qd : qi;
                    k0[s] = mm[((mx * (mx + 1)) >> 1) + mn];
                    k3[s] = cell::pXX_of(ph2pr, qc);
                    k1[s] = cell::pGAPM_of<Ar>(ph2pr, qc);
                    k2[s] = cell::pMX_of(ph2pr, qi);
                    k4[s] = cell::pMY_of(ph2pr, qd);
                    zero_gap |= cell::row_needs_plain(qc);
                    if constexpr (FIVE) zero_mm |= cell::row_has_zero_pMM(k0[s]);
                    eM[s] = cell::match_of<Ar>(ph2pr, qq);
                    const int code = base_code(a.bases[o]);
                    eX[s] = (code == kCodeN) ? eM[s] : ph2pr_div3[qq];
                    ratio[s] = cell::ratio_of(gap_ratio, qc);
                    rb[s] = code;
                }
            }
        }
        // FIVE, the static rule: the cell divides by every row's pMM and pGAPM, so a test case with a zero among them is left
        // to the second launch -- per test case, like a haplotype with an N
        if constexpr (FIVE) {
            defer |= (__ballot((int)(zero_gap | zero_mm)) & gmask) != 0;
            // The coefficients of the five-operation cell, per row: k1 = a = A' of the row above, k2 = B', k3 = q', k4 = pYY, and
            // the emissions times s = pMM of the row below.  Rows below / above the lane's own come from the neighbour lanes.
            using Edge = cell::Edge<T>;
            const bool last_lane = j == nl - 1;
            const T g_next_lane = shr1_down<G>(k1[0]), mm_next_lane = shr1_down<G>(k0[0]);
            T rcp[RPL], Ap[RPL], gr[RPL];
#pragma unroll
            for (int s = 0; s < RPL; ++s) {
                const T gb = (s + 1 < RPL) ? k1[s + 1] : (last_lane ? Edge::g_below() : g_next_lane);
                const T sb = (s + 1 < RPL) ? k0[s + 1] : (last_lane ? Edge::s_below() : mm_next_lane);
                rcp[s] = cell::five_rcp<Ar>(k0[s]);
                Ap[s] = clone[s] ? Edge::A_above() : cell::five_Ap<Ar>(gb, k2[s], rcp[s]);
                gr[s] = cell::scaled_B<Ar>(gb, ratio[s]);
                eM[s] = cell::five_E<Ar>(eM[s], sb); eX[s] = cell::five_E<Ar>(eX[s], sb);
            }
            const T my_up = shr1<G>(Edge::pMY_above(), clone[RPL - 1] ? Edge::pMY_above() : k4[RPL - 1]);
            const T a_up = shr1<G>(Edge::A_above(), Ap[RPL - 1]);
            T qv[RPL], av[RPL], bv[RPL];
#pragma unroll
            for (int s = 0; s < RPL; ++s) {
                const int rho = j * RPL + s - top_clones;
                const T my_above = s ? (clone[s - 1] ? Edge::pMY_above() : k4[s - 1]) : my_up;
                av[s] = s ? Ap[s - 1] : a_up;
                qv[s] = rho == 0 ? k1[s] : cell::five_q<Ar>(k1[s], my_above, rcp[s]);     // read row 0: g (y of the boundary row is unscaled)
                bv[s] = cell::five_Bp<Ar>(gr[s], av[s], Ap[s]);
            }
#pragma unroll
            for (int s = 0; s < RPL; ++s) {
                k4[s] = k3[s];                                            // pYY
                k1[s] = av[s]; k2[s] = bv[s]; k3[s] = qv[s];
                if (clone[s]) { k1[s] = 0; k2[s] = 0; k3[s] = 0; k4[s] = 1; }
            }
            res_scale = Ap[RPL - 1];
            // The hand-off (pairhmm_cell.h): a lane's bottom row evaluates the next lane's top-row paths value and x itself, so it
            // keeps that row's a, B' and q' and the top row's own three are used once more, for the boundary value of group lane 0.
            // The last used lane hands on with zeros, to a lane that is not in use (or to none).  Its bottom row is read row R,
            // which sums its m in its yb.
            const T a_dn = shr1_down<G>(k1[0]), B_dn = shr1_down<G>(k2[0]), q_dn = shr1_down<G>(k3[0]);
            dn_a = last_lane ? (T)0 : a_dn; dn_B = last_lane ? (T)0 : B_dn; dn_q = last_lane ? (T)0 : q_dn;
            paths0 = cell::five_boundary_paths<Ar>(init_y, k1[0], k3[0]);
            if (last_lane) k4[RPL - 1] = Edge::pYY_sum_row();
        }
        if constexpr (kETab) {
            // one store per read of the column loop (pairhmm_etab.h) and code
            auto entry = [&](int s, int code) { return (code == rb[s] || code == kCodeN) ? eM[s] : eX[s]; };
#pragma unroll
            for (int k = 0; k < ETab::kReads; ++k) {
                const etab::Read rd = etab::read_of(RPL, CODES, ETab::kQuadLayout, k);
                const int s = rd.row0;
#pragma unroll
                for (int code = 0; code < kNumCodes; ++code) {
                    uint8_t* q = etab_base + rd.offset + lane * rd.bytes + code * rd.code_stride;
                    if (rd.bytes == etab::kQuadBytes)
                        *reinterpret_cast<float4*>(q) = make_float4(entry(s, code), entry(s + 1, code), entry(s + 2, code), entry(s + 3, code));
                    else if (s + 1 < RPL)
                        *reinterpret_cast<float2*>(q) = make_float2(entry(s, code), entry(s + 1, code));
                    else
                        *reinterpret_cast<float*>(q) = entry(s, code);      // the last, single row of an odd RPL
                }
            }
        }
        __syncthreads();                          // hapbuf / etab visible

        // ---- anti-diagonal sweep
        // (a group that leaves its test case to the five-code launch takes no steps of its own: like a group without a job
        // it follows its neighbours, and a wavefront made of such groups only skips the sweep)
        const bool swept = live && !defer;
        const int nsteps_g = swept ? (H + nl - 1) : 0;
        int nmax = nsteps_g, nmin = swept ? nsteps_g : 0x7fffffff;
        if constexpr (GPW > 1) {
            // every lane of a group holds the group's value: combine across the groups interleaved in a row
            // (xor below S), then across rows / groups (xor from max(G, 16) up)
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                if (off >= S && off < (G < 16 ? 16 : G)) continue;
                const int o1 = __shfl_xor(nmax, off, 64), o2 = __shfl_xor(nmin, off, 64);
                nmax = o1 > nmax ? o1 : nmax;
                nmin = o2 < nmin ? o2 : nmin;
            }
        }
        nmax = __builtin_amdgcn_readfirstlane(nmax);
        nmin = __builtin_amdgcn_readfirstlane(nmin);
        if (nmin > nmax) nmin = nmax;

        const uint8_t* hp_lane = hapbuf + (G - j);  // hp_lane[d] = code of this lane's column at step d
        // this lane's entry of code 0 at offset 0 of a quad table and of a pair table
        const uint8_t* et_quad = etab_base + lane * etab::kQuadBytes;
        const uint8_t* et_pair = etab_base + lane * etab::kPairBytes;

        auto load_e = [&](int h, T (&dst)[RPL]) {
            if constexpr (kETab) {
                // the column's read list: one ds_read_b128 per quad table, one ds_read_b64 (b32: a single row) per pair table
#pragma unroll
                for (int k = 0; k < ETab::kReads; ++k) {
                    const etab::Read rd = etab::read_of(RPL, CODES, ETab::kQuadLayout, k);
                    const int s = rd.row0;
                    if (rd.bytes == etab::kQuadBytes) {
                        const float4 v = *reinterpret_cast<const float4*>(et_quad + h * rd.code_stride + rd.offset);
                        dst[s] = v.x; dst[s + 1] = v.y; dst[s + 2] = v.z; dst[s + 3] = v.w;
                    } else {
                        const float2 v = *reinterpret_cast<const float2*>(et_pair + h * rd.code_stride + rd.offset);
                        dst[s] = v.x;
                        if (s + 1 < RPL) dst[s + 1] = v.y;
                    }
                }
            } else {
                const bool hN = (h == kCodeN);
#pragma unroll
                for (int s = 0; s < RPL; ++s) dst[s] = ((h == rb[s]) | hN) ? eM[s] : eX[s];
            }
        };

        // The sweep in one of the algebraic forms of pairhmm_cell.h (the algebra is in its header comment): plain, or the
        // precision's fast form, selected per wavefront; with FIVE the five-operation cell.
        const bool use_plain = EXACT || __any((int)zero_gap) != 0;
        constexpr int kPlain = 0, kScaled = 1, kSixOp = 2, kFiveOp = 3;

        auto sweep = [&](auto form_tag) {
            constexpr int FORM = decltype(form_tag)::value;
            constexpr bool SC = FORM == kScaled;
            constexpr bool SIX = FORM == kSixOp;
            constexpr bool FIV = FORM == kFiveOp;
            T y_above = init_y;                     // what the group's lane 0 sees above its top row
            if constexpr (SC || SIX) {
                // g of the row below each row: next row in this lane, or the next lane's top row
                T g_own[RPL], g_below[RPL];
#pragma unroll
                for (int s = 0; s < RPL; ++s) g_own[s] = k1[s];
                T g_next_lane = shr1_down<G>(g_own[0]);          // lane j+1's top-row g
#pragma unroll
                for (int s = 0; s < RPL; ++s) g_below[s] = (s + 1 < RPL) ? g_own[s + 1] : g_next_lane;
                if (j == nl - 1) {                               // read row R: unscaled; a strip's last row: the next strip's first row
                    g_below[RPL - 1] = cell::Edge<T>::g_below();
                    if constexpr (STRIP) { if (!last_strip) g_below[RPL - 1] = cell::pGAPM_of<Ar>(ph2pr, a.gcp[job.read_off + (uint64_t)(row_base + rows_here)] & 127); }
                }
                // six: pMY of the row above each row -- this lane's row s - 1, or lane j - 1's bottom row; above the group's
                // lane 0 lies the boundary row (pMY_0 := 1, so y_0 = INITIAL/H) or the previous strip's last read row.
                // A row-0 clone passes pMY' = 1 on.
                T my_above[RPL];
                if constexpr (SIX) {
                    T my_own[RPL];
#pragma unroll
                    for (int s = 0; s < RPL; ++s) my_own[s] = clone[s] ? cell::Edge<T>::pMY_above() : k4[s];
                    T my_top = cell::Edge<T>::pMY_above();
                    if constexpr (STRIP) {
                        if (strip > 0) my_top = cell::pMY_of(ph2pr, a.del[job.read_off + (uint64_t)(row_base - 1)] & 127);
                    }
                    my_above[0] = shr1<G>(my_top, my_own[RPL - 1]);
#pragma unroll
                    for (int s = 1; s < RPL; ++s) my_above[s] = my_own[s - 1];
                }
#pragma unroll
                for (int s = 0; s < RPL; ++s) {
                    if (clone[s]) {
                        py[s] = SIX ? init_y : cell::scaled_Y0<Ar>(g_below[s], init_y);   // Y^ / y of a row-0 clone, constant (D = 1)
                    } else {
                        const T gb = g_below[s];
                        const T pMX = k2[s], pXX = k3[s], pMY = k4[s];
                        k1[s] = cell::scaled_A<Ar>(gb, pMX);
                        k2[s] = cell::scaled_B<Ar>(gb, ratio[s]);
                        if constexpr (SIX) k3[s] = cell::six_q<Ar>(g_own[s], my_above[s]);
                        else k3[s] = cell::scaled_C<Ar>(gb, pMY);
                        k4[s] = pXX;                             // D = pYY
                    }
                    if (clone[s]) { k1[s] = 0; k2[s] = 0; k3[s] = 0; k4[s] = 1; }
                }
                y_above = SIX ? init_y : cell::scaled_Y0<Ar>(g_own[0], init_y);
            }
            const T old_y = (j == 0) ? y_above : (T)0;
            T uaM = 0, uaX = 0, uaY = old_y, ubM = 0, ubX = 0, ubY = old_y;   // two shifted-in sets
            if constexpr (STRIP) {
                // later strips: above lane 0's top row lies the previous strip's bottom row -- zeros in the DP's
                // column 0 (the diagonal input of the first column), boundary[0] above the first column
                if (strip > 0) {
                    uaY = 0; ubY = 0;
                    if (j == 0 && H > 0) { ubM = bprev[0]; ubX = bprev[a.strip_stride]; ubY = bprev[2u * a.strip_stride]; }
                }
            }

            // one column (every form but the five-operation one: column5 below): o2* = values shifted in two
            // steps ago (M,X,Y), o1* = last step (M,X); the new shifted-in set overwrites o2's registers.  The DPP `old` operand is the register's
            // own previous content, so the group's lane 0 keeps (0, 0, y_above) for ever.
            auto column = [&](const T (&ec)[RPL], T& o2M, T& o2X, T& o2Y, const T o1M, const T o1X, bool count, const int dcol) {
                // Every multiply-add below is an explicit fma (the file is built with
                // -ffp-contract=off): the two inlined copies of this lambda in the main loop and the
                // copy in the tail loop must round identically, or a pair's result would depend on
                // how many of its columns ran in which loop, i.e. on its wavefront neighbours.
                T Mn[RPL], Xn[RPL], Yn[RPL];
                if constexpr (SIX) {
                    // in place, bottom row first: a row's new M and y overwrite the old ones once the row below has
                    // read them, so no value has to be moved out of the way; X follows top down from the new M
#pragma unroll
                    for (int s = RPL - 1; s >= 0; --s) {
                        const T t = s ? cell::six_M_paths<Ar>(pm[s - 1], px[s - 1], py[s - 1], k0[s], k3[s])
                                      : cell::six_M_paths<Ar>(o2M, o2X, o2Y, k0[0], k3[0]);
                        py[s] = cell::six_y<Ar>(pm[s], py[s], k4[s]);
                        pm[s] = cell::emit<Ar>(t, ec[s]);
                    }
                    px[0] = cell::scaled_X<Ar>(o1M, o1X, k1[0], k2[0]);
#pragma unroll
                    for (int s = 1; s < RPL; ++s) px[s] = cell::scaled_X<Ar>(pm[s - 1], px[s - 1], k1[s], k2[s]);
#pragma unroll
                    for (int s = 0; s < RPL; ++s) { Mn[s] = pm[s]; Xn[s] = px[s]; Yn[s] = py[s]; }
                } else if constexpr (SC) {
                    Mn[0] = cell::scaled_M<Ar>(o2M, o2X, o2Y, k0[0], ec[0]);
                    Xn[0] = cell::scaled_X<Ar>(o1M, o1X, k1[0], k2[0]);
                    Yn[0] = cell::scaled_Y<Ar>(pm[0], py[0], k3[0], k4[0]);
#pragma unroll
                    for (int s = 1; s < RPL; ++s) {
                        Mn[s] = cell::scaled_M<Ar>(pm[s - 1], px[s - 1], py[s - 1], k0[s], ec[s]);
                        Xn[s] = cell::scaled_X<Ar>(Mn[s - 1], Xn[s - 1], k1[s], k2[s]);
                        Yn[s] = cell::scaled_Y<Ar>(pm[s], py[s], k3[s], k4[s]);
                    }
                } else if constexpr (EXACT) {
                    // avx-pairhmm-template.h:183-192, unfused (the file is built with -ffp-contract=off)
                    Mn[0] = cell::exact_M<Ar>(o2M, o2X, o2Y, k0[0], k1[0], ec[0]);
                    Xn[0] = cell::exact_X<Ar>(o1M, o1X, k2[0], k3[0]);
                    Yn[0] = cell::exact_Y<Ar>(pm[0], py[0], k4[0], k3[0]);
#pragma unroll
                    for (int s = 1; s < RPL; ++s) {
                        Mn[s] = cell::exact_M<Ar>(pm[s - 1], px[s - 1], py[s - 1], k0[s], k1[s], ec[s]);
                        Xn[s] = cell::exact_X<Ar>(Mn[s - 1], Xn[s - 1], k2[s], k3[s]);
                        Yn[s] = cell::exact_Y<Ar>(pm[s], py[s], k4[s], k3[s]);
                    }
                } else {
                    Mn[0] = cell::plain_M<Ar>(o2M, o2X, o2Y, k0[0], k1[0], ec[0]);
                    Xn[0] = cell::plain_X<Ar>(o1M, o1X, k2[0], k3[0]);
                    Yn[0] = cell::plain_Y<Ar>(pm[0], py[0], k4[0], k3[0]);
#pragma unroll
                    for (int s = 1; s < RPL; ++s) {
                        Mn[s] = cell::plain_M<Ar>(pm[s - 1], px[s - 1], py[s - 1], k0[s], k1[s], ec[s]);
                        Xn[s] = cell::plain_X<Ar>(Mn[s - 1], Xn[s - 1], k2[s], k3[s]);
                        Yn[s] = cell::plain_Y<Ar>(pm[s], py[s], k4[s], k3[s]);
                    }
                }
#pragma unroll
                for (int s = 0; s < RPL; ++s) { pm[s] = Mn[s]; px[s] = Xn[s]; py[s] = Yn[s]; }
                if (count && (!STRIP || last_strip)) { sumM += Mn[RPL - 1]; sumX += Xn[RPL - 1]; }
                o2M = shr1<G>(o2M, Mn[RPL - 1]);
                o2X = shr1<G>(o2X, Xn[RPL - 1]);
                o2Y = shr1<G>(o2Y, Yn[RPL - 1]);
                if constexpr (STRIP) {
                    // the set just shifted in is used as "row above, this column" at the next step and as "row above,
                    // previous column" the step after: for lane 0 of a later strip that is boundary[dcol + 1]
                    if (strip > 0 && j == 0) {
                        const int c1 = dcol + 1;
                        const bool in = c1 < H;
                        o2M = in ? bprev[c1] : (T)0; o2X = in ? bprev[a.strip_stride + c1] : (T)0; o2Y = in ? bprev[2u * a.strip_stride + c1] : (T)0;
                    }
                    if (!last_strip && j == nl - 1) {
                        const int c = dcol - j;
                        if (c >= 0 && c < H) { bcur[c] = Mn[RPL - 1]; bcur[a.strip_stride + c] = Xn[RPL - 1]; bcur[2u * a.strip_stride + c] = Yn[RPL - 1]; }
                    }
                }
            };

            // The five-operation column.  Two values cross to the next lane (pairhmm_cell.h): the paths value of its top row, which it
            // needs two steps later (`tin`: two registers alternate, as ua* / ub* do; group lane 0 keeps the boundary value for
            // ever), and its top row's x, which it needs at the next step (`x_dn`, shifted into px[0] there: after the m phase,
            // which still reads the old px[0] for row 1, and before the x chain; group lane 0's px[0] stays 0).  Read row R -- the
            // last used lane's bottom row -- sums its m in its yb (sum_m_of_row below), so only sum x is added here.
            T ta = (j == 0) ? paths0 : (T)0, tb = ta, x_dn = 0;
            auto column5 = [&](const T (&ec)[RPL], T& tin, bool count) {
#pragma unroll
                for (int s = RPL - 1; s >= 0; --s) {
                    const T t = s ? cell::five_m_paths<Ar>(pm[s - 1], px[s - 1], py[s - 1], k1[s], k3[s]) : tin;
                    py[s] = cell::six_y<Ar>(pm[s], py[s], k4[s]);
                    pm[s] = cell::emit<Ar>(t, ec[s]);
                }
                px[0] = shr1<G>(px[0], x_dn);
#pragma unroll
                for (int s = 1; s < RPL; ++s) px[s] = cell::five_x<Ar>(pm[s - 1], px[s - 1], k2[s]);
                if (count) sumX += px[RPL - 1];
                tin = shr1<G>(tin, cell::five_paths_down<Ar>(pm[RPL - 1], px[RPL - 1], py[RPL - 1], dn_a, dn_q));
                x_dn = cell::five_x_down<Ar>(pm[RPL - 1], px[RPL - 1], dn_B);
            };
            // after a group's last step: read row R's yb holds every m but the last column's
            auto sum_m_of_row = [&]() { sumM = cell::five_sum_m<Ar>(py[RPL - 1], pm[RPL - 1]); };

            T e[RPL];
            int d = 0;
            int h1 = hp_lane[1];
            load_e((int)hp_lane[0], e);
            // main loop: two columns per iteration (register sets a/b alternate), no guards: every
            // step below nmin is inside every live group's range.
            for (; d + 2 <= nmin; d += 2) {
                T e1[RPL];
                load_e(h1, e1);
                const int h2 = hp_lane[d + 2], h3 = hp_lane[d + 3];
                if constexpr (FIV) column5(e, ta, true); else column(e, uaM, uaX, uaY, ubM, ubX, true, d);
                load_e(h2, e);
                if constexpr (FIV) column5(e1, tb, true); else column(e1, ubM, ubX, ubY, uaM, uaX, true, d + 1);
                h1 = h3;
            }
            // (a group's last step is the main loop's last one or a step of the tail, as its wavefront neighbours' H have it)
            if constexpr (FIV) { if (d == nsteps_g) sum_m_of_row(); }
            // tail: at most a few guarded columns (groups of one wavefront differ slightly in H)
            for (; d < nmax; ++d) {
                const int hn = hp_lane[d + 1];
                T t;
                if constexpr (FIV) {
                    column5(e, ta, d < nsteps_g);
                    t = ta; ta = tb; tb = t;
                } else {
                    column(e, uaM, uaX, uaY, ubM, ubX, d < nsteps_g, d);
                    t = uaM; uaM = ubM; ubM = t;
                    t = uaX; uaX = ubX; ubX = t;
                    t = uaY; uaY = ubY; ubY = t;
                }
                if constexpr (FIV) { if (d == nsteps_g - 1) sum_m_of_row(); }      // the columns after it run on pad codes
                load_e(hn, e);
            }
        };
        if constexpr (FIVE) sweep(std::integral_constant<int, kFiveOp>{});
        else if constexpr (EXACT) sweep(std::integral_constant<int, kPlain>{});
        else if (use_plain) sweep(std::integral_constant<int, kPlain>{});
        else if constexpr (kSix) sweep(std::integral_constant<int, kSixOp>{});
        else sweep(std::integral_constant<int, kScaled>{});
      }   // strips

        // ---- result (IntelPairHmm.cc:338-350)
        if (live && j == nl - 1) {
            const T res = FIVE ? cell::five_result<Ar>(sumM, res_scale, sumX) : cell::result<Ar>(sumM, sumX);
            if constexpr (sizeof(T) == 4) {
                // (FIVE) the dynamic rule: a result that is not finite -- an overflow in any cell -- is left to the second launch
                if (defer || (FIVE && cell::five_overflowed(res))) {
                    const uint32_t k = atomicAdd(a.nhap_count, 1u);
                    a.nhap_list[k] = job_idx;
                    if constexpr (FIVE) { if (!group_hap_n) atomicAdd(a.form_count, 1u); }
                } else if (res < cell::kFloatFirstBelow) {
                    const uint32_t k = atomicAdd(a.rerun_count, 1u);
                    a.rerun_list[k] = job_idx;
                } else {
                    a.out_log10[job.pair] = (double)(log10f(res) - a.log10_initial_f);
                }
            } else {
                // below kExactBelow the flushed products may carry a visible share of the result (each flushed
                // term is < 2^-1022 and the model passes on at most its own mass: with fewer than 1e21 operations
                // per test case the share is < 1e-6 above the threshold); a zero counts as below
                if (!EXACT && a.rerun_count && res < cell::kExactBelow) {
                    const uint32_t k = atomicAdd(a.rerun_count, 1u);
                    a.rerun_list[k] = job_idx;
                } else {
                    a.out_log10[job.pair] = log10(res) - a.log10_initial_d;
                    a.used_f64[job.pair] = 1;
                }
            }
        }
    }
}

// fp32 classes of up to 8 rows per lane fit the register budget of 4 wavefronts per SIMD (128 VGPRs) natively -- 8 rows
// per lane at exactly 128 -- except 7 rows per lane (129 registers), which the bound brings to 128 at the cost of one or
// two values parked in scratch outside the sweep.  The bound is applied to that class ONLY: on the 8-row classes it
// changes the allocator's choices and parks 16-18 values (236 MB of scratch writes per 1 M test cases; same duration).
// (Holding 11 rows per lane -- 171 registers -- to the 168 of 3 wavefronts spills 19: not done.)  10 rows per lane (the
// 151-base reads) need 169 with the 6-operation cell: held to the 168 of 3 wavefronts.
template <typename T, int G, int RPL, int CODES = kMaxCodes, bool FIVE = false>
#ifndef MGX_HMM_MINWAVES_8
#define MGX_HMM_MINWAVES_8 4
#endif
__global__ __launch_bounds__(256, (sizeof(T) == 4 && RPL == 7) ? MGX_HMM_MINWAVES_8 : (sizeof(T) == 4 && RPL == 10) ? 3 : 1) void pairhmm_fwd(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    pairhmm_body<T, G, RPL, false, false, CODES, FIVE>(a, smem, blockIdx.x, gridDim.x);
}

// the strip-mined class: reads of more than 1024 bases, one test case per wavefront, 64 lanes x 16 rows per strip
constexpr int kStripG = 64, kStripRPL = 16;
template <typename T>
__global__ __launch_bounds__(64) void pairhmm_fwd_strip(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    pairhmm_body<T, kStripG, kStripRPL, true>(a, smem, blockIdx.x, gridDim.x);
}
// the exact tier: reads of any length (one strip up to 1024 bases), one test case per wavefront
__global__ __launch_bounds__(64) void pairhmm_fwd_exact(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    pairhmm_body<double, kStripG, kStripRPL, true, true>(a, smem, blockIdx.x, gridDim.x);
}

// Several classes in ONE launch (fp32, one wavefront per workgroup): a batch of mixed read lengths otherwise needs
// a launch per class, and every launch ends with a drain during which most of the device idles (ragged 1 M test
// cases: nine launches, ~9 % of the kernel time).  Workgroups are dealt to the classes in the order the host lists
// them -- most rows per lane first, inside a class longest haplotype first -- so the single drain is made of the
// cheapest jobs.  GSET 0: the 16-lane classes with 1..8 rows per lane; GSET 1: the 8- and 4-lane classes (their
// 8 / 16 haplotypes per wavefront need more LDS, which would cost the 16-lane classes occupancy in a common launch).
struct MultiArgs {
    KernelArgs a;                              // job_first, n_static and lds_stride are filled in per class
    uint32_t n_bins;
    uint32_t block_first[kMultiBins + 1];      // first workgroup of every class
    uint32_t job_first[kMultiBins], job_count[kMultiBins], lds_stride[kMultiBins];
    uint8_t G[kMultiBins], RPL[kMultiBins];
    uint8_t bin[kMultiBins];                   // the class's index in the batch: its N-haplotype counter
};

template <int GSET>
__device__ __forceinline__ void pairhmm_multi_body(const MultiArgs& m, uint8_t* smem) {
    uint32_t k = 0;
    while (k + 1 < m.n_bins && blockIdx.x >= m.block_first[k + 1]) ++k;       // wave-uniform
    KernelArgs a = m.a;
    a.job_first = m.job_first[k]; a.n_static = m.job_count[k]; a.lds_stride = m.lds_stride[k];
    a.nhap_list += m.job_first[k]; a.nhap_count += m.bin[k];          // every class keeps its own N-haplotype list
    const uint32_t blk = blockIdx.x - m.block_first[k], nblk = m.block_first[k + 1] - m.block_first[k];
    const int code = (int)m.G[k] * 16 + (int)m.RPL[k];
#define MGX_MCASE(g, r) case (g) * 16 + (r): pairhmm_body<float, g, r, false, false, 4, true>(a, smem, blk, nblk); break;
    if constexpr (GSET == 0) {
        switch (code) {
            MGX_MCASE(16, 1) MGX_MCASE(16, 2) MGX_MCASE(16, 3) MGX_MCASE(16, 4) MGX_MCASE(16, 5) MGX_MCASE(16, 6) MGX_MCASE(16, 7) MGX_MCASE(16, 8)
            default: break;
        }
    } else {
        switch (code) {
            MGX_MCASE(8, 1) MGX_MCASE(8, 2) MGX_MCASE(8, 3) MGX_MCASE(8, 4) MGX_MCASE(8, 5) MGX_MCASE(8, 6) MGX_MCASE(8, 7) MGX_MCASE(8, 8)
            MGX_MCASE(4, 1) MGX_MCASE(4, 2) MGX_MCASE(4, 3) MGX_MCASE(4, 4) MGX_MCASE(4, 5) MGX_MCASE(4, 6) MGX_MCASE(4, 7) MGX_MCASE(4, 8)
            default: break;
        }
    }
#undef MGX_MCASE
}

template <int GSET>
__global__ __launch_bounds__(256) void pairhmm_fwd_multi(MultiArgs m) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    pairhmm_multi_body<GSET>(m, smem);
}

// Cross-product batches (every read against every haplotype of a region, the shape
// VectorLoglessPairHMM builds): job descriptors are generated on the device from two small tables
// instead of being written one by one on the host.
__global__ __launch_bounds__(256) void pairhmm_make_jobs_multi(const SeqRef* __restrict__ reads, const uint32_t* __restrict__ read_region,
                                                               const uint32_t* __restrict__ job_prefix, uint32_t n_reads,
                                                               const RegionRef* __restrict__ regions, const SeqRef* __restrict__ haps,
                                                               uint32_t n_jobs, Job* __restrict__ jobs) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_jobs) return;
    uint32_t lo = 0, hi = n_reads;                 // last read with job_prefix[r] <= q
    while (hi - lo > 1) { const uint32_t m = lo + (hi - lo) / 2; if (job_prefix[m] <= q) lo = m; else hi = m; }
    const SeqRef r = reads[lo];
    const RegionRef g = regions[read_region[lo]];
    const SeqRef h = haps[g.hap_begin + (q - job_prefix[lo])];
    Job j;
    j.read_off = r.off; j.hap_off = h.off; j.R = r.len; j.H = h.len;
    j.pair = g.out_base + (r.id - g.read_base) * g.n_haps + h.id; j.pad_ = 0;
    jobs[q] = j;
}

// ---------------------------------------------------------------------------------------------
// Row F2 (SURVEY.md 8f): the per-read quality model in front of the recurrence and the
// normalisation / filter behind it, so that a whole computeReadLikelihoods() call
// (PairHMMLikelihoodCalculationEngine.cpp:77-97) needs one upload and one download.
// ---------------------------------------------------------------------------------------------
struct ReadModel {
    uint8_t pcr_cache[21];     // pcrIndelErrorModelCache, PairHMMLikelihoodCalculationEngine.cpp:45-61
    int rate_factor;           // 0: leave ins/del alone
    int bq_threshold;          // baseQualityScoreThreshold (18)
    int constant_gcp;          // < 0: keep the caller's gcp
};

// GATKVariantContextUtils::findNumberOfRepetitions (GATKVariantContextUtils.cpp:59-100) on one string
__device__ __forceinline__ int n_repetitions(const uint8_t* s, int unit_off, int unit_len, int test_off, int test_len, bool leading) {
    if (test_len == 0) return 0;
    const int diff = test_len - unit_len;
    int n = 0;
    if (leading) {
        for (int st = 0; st <= diff; st += unit_len) {
            bool eq = true;
            for (int i = 0; i < unit_len; ++i) eq &= s[st + test_off + i] == s[unit_off + i];
            if (!eq) return n;
            ++n;
        }
    } else {
        for (int st = diff; st >= 0; st -= unit_len) {
            bool eq = true;
            for (int i = 0; i < unit_len; ++i) eq &= s[st + test_off + i] == s[unit_off + i];
            if (!eq) return n;
            ++n;
        }
    }
    return n;
}
// PairHMMLikelihoodCalculationEngine::findTandemRepeatUnits (:175-254)
__device__ int tandem_repeat_units(const uint8_t* b, int length, int offset) {
    int maxBW = 0, bw_off = offset, bw_len = 1;
    for (int str = 1; str <= 8; ++str) {
        if (offset + 1 - str < 0) break;
        maxBW = n_repetitions(b, offset - str + 1, str, 0, offset + 1, false);
        if (maxBW > 1) { bw_off = offset - str + 1; bw_len = str; break; }
    }
    int maxRL = maxBW;
    if (offset < length - 1) {
        int maxFW = 0, fw_len = 1;
        const int fw_off = offset + 1;
        for (int str = 1; str <= 8; ++str) {
            if (offset + str + 1 > length) break;
            maxFW = n_repetitions(b, offset + 1, str, offset + 1, length - offset - 1, true);
            if (maxFW > 1) { fw_len = str; break; }
        }
        bool same = fw_len == bw_len;
        if (same) for (int i = 0; i < fw_len; ++i) same &= b[fw_off + i] == b[bw_off + i];
        if (!same) maxBW = n_repetitions(b, fw_off, fw_len, 0, offset + 1, false);
        maxRL = maxFW + maxBW;
    }
    return maxRL > 20 ? 20 : maxRL;
}

// one workgroup per read: applyPCRErrorModel (:149-157), capMinimumReadQualities (:256-267),
// buildGapContinuationPenalties (:284-292), in place on the uploaded arrays
__global__ __launch_bounds__(128) void pairhmm_read_model(const SeqRef* __restrict__ reads, const uint8_t* __restrict__ bases,
                                                          uint8_t* qual, uint8_t* ins, uint8_t* del, uint8_t* gcp,
                                                          const uint8_t* __restrict__ mapq, ReadModel m) {
    __shared__ uint8_t sb[1024 + 16];
    const SeqRef r = reads[blockIdx.x];
    const int len = (int)r.len;
    // reads of up to 1024 bases are searched in LDS; longer ones (the strip-mined class) straight in global memory
    const bool in_lds = len <= 1024;
    if (in_lds) for (int i = threadIdx.x; i < len; i += blockDim.x) sb[i] = bases[r.off + i];
    __syncthreads();
    const uint8_t* sbp = in_lds ? sb : bases + r.off;
    const int mq = mapq[r.id];
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
        int qi = ins[r.off + i], qd = del[r.off + i];
        if (m.rate_factor > 0 && i < len - 1) {
            const int c = m.pcr_cache[tandem_repeat_units(sbp, len, i)];
            qi = c < qi ? c : qi; qd = c < qd ? c : qd;
        }
        int q = qual[r.off + i];
        q = mq < q ? mq : q;
        qual[r.off + i] = (uint8_t)(q < m.bq_threshold ? 6 : q);
        ins[r.off + i] = (uint8_t)(qi < 6 ? 6 : qi);
        del[r.off + i] = (uint8_t)(qd < 6 ? 6 : qd);
        if (m.constant_gcp >= 0) gcp[r.off + i] = (uint8_t)m.constant_gcp;
    }
}

// one wavefront per read over its n_haps results: normalizeLikelihoods (AlleleLikelihoods.h:153-166,
// 372-391) and the filterPoorlyModeledEvidence decision (:404-419, log10MinTrueLikelihood
// PairHMMLikelihoodCalculationEngine.cpp:294-299).  Every read has its own row (start, width) in the output: the
// reads of a batch may belong to different regions.
__global__ __launch_bounds__(256) void pairhmm_normalize_filter_rows(double* __restrict__ out, const uint64_t* __restrict__ read_len,
                                                                     const uint32_t* __restrict__ row_off, const uint32_t* __restrict__ row_nh,
                                                                     uint32_t n_reads, double log10_rate, double max_error_per_base,
                                                                     uint8_t* __restrict__ keep) {
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_reads) return;
    const uint32_t n_haps = row_nh[r];
    double* row = out + row_off[r];
    double best = -__builtin_inf();
    for (uint32_t h = lane; h < n_haps; h += 64) best = fmax(best, row[h]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off, 64));
    if (!__builtin_isinf(log10_rate) && n_haps > 1) {
        const double cap = best + log10_rate;
        for (uint32_t h = lane; h < n_haps; h += 64) if (row[h] < cap) row[h] = cap;
    }
    if (lane == 0) {
        const double max_err = fmin(2.0, ceil((double)read_len[r] * max_error_per_base));
        keep[r] = !(best < max_err * -4.0);
    }
}

// one wavefront per read over its row of normalised log10 values: bestAllelesBreakingTies, i.e. searchBestAllele with
// canBeReference = true (AlleleLikelihoods.h:92-146) as the two folds of best_allele_rule.h -- lanes stride the row and fold their
// share, a butterfly of shuffles folds the lanes (both merges are commutative: every lane ends with the row's result).  Row r is
// values[row_off[r] .. + row_nh[r]); its priorities are priority[pri_off[r] + h] (pri_off == nullptr: row_off), priority == nullptr
// switches the tie-break off.
__device__ __forceinline__ mgx_best_allele::Top shfl_xor_(mgx_best_allele::Top t, int off) {
    return mgx_best_allele::Top{__shfl_xor(t.v, off, 64), (uint32_t)__shfl_xor((int)t.at, off, 64)};
}
__device__ __forceinline__ mgx_best_allele::Cand shfl_xor_(mgx_best_allele::Cand c, int off) {
    return mgx_best_allele::Cand{__shfl_xor(c.pri, off, 64), (uint32_t)__shfl_xor((int)c.at, off, 64), (uint32_t)__shfl_xor((int)c.entered, off, 64)};
}
__global__ __launch_bounds__(256) void pairhmm_best_allele_rows(const double* __restrict__ values, const uint32_t* __restrict__ row_off,
                                                                const uint32_t* __restrict__ row_nh, const double* __restrict__ priority,
                                                                const uint32_t* __restrict__ pri_off, uint32_t n_rows, int32_t* __restrict__ out_best) {
    namespace BA = mgx_best_allele;
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= n_rows) return;
    const uint32_t n_haps = row_nh[r];
    const double* row = values + row_off[r];
    BA::Top top = BA::top_identity();
    for (uint32_t h = lane; h < n_haps; h += 64) top = BA::merge(top, BA::top_of(row[h], h));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = BA::merge(top, shfl_xor_(top, off));
    uint32_t best = top.at == BA::kNone ? 0u : top.at;
    if (priority && n_haps > 1) {
        const double* pri = priority + (pri_off ? pri_off[r] : row_off[r]);
        BA::Cand cand = BA::cand_identity();
        for (uint32_t h = lane; h < n_haps; h += 64) cand = BA::merge(cand, BA::cand_of(top, BA::top_of(row[h], h).v, pri[h], h));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cand = BA::merge(cand, shfl_xor_(cand, off));
        best = BA::result(top, pri[top.at], cand);
    }
    if (lane == 0) out_best[r] = (int32_t)best;
}

using KernelFn = void (*)(KernelArgs);

// (four code columns: the first fp32 launch of a class -- with the five-operation cell in the classes of up to 16 lanes)
template <typename T, int CODES = kMaxCodes>
KernelFn pick_kernel(int G, int RPL) {
#define MGX_CASE(g, r) if (G == g && RPL == r) return pairhmm_fwd<T, g, r, CODES, (CODES == 4 && g <= kFiveOpMaxG)>;
    MGX_CASE(4, 1) MGX_CASE(4, 2) MGX_CASE(4, 3) MGX_CASE(4, 4) MGX_CASE(4, 5) MGX_CASE(4, 6) MGX_CASE(4, 7) MGX_CASE(4, 8)
    MGX_CASE(8, 1) MGX_CASE(8, 2) MGX_CASE(8, 3) MGX_CASE(8, 4) MGX_CASE(8, 5) MGX_CASE(8, 6) MGX_CASE(8, 7) MGX_CASE(8, 8)
    MGX_CASE(16, 1) MGX_CASE(16, 2) MGX_CASE(16, 3) MGX_CASE(16, 4)
    MGX_CASE(16, 5) MGX_CASE(16, 6) MGX_CASE(16, 7) MGX_CASE(16, 8)
    if constexpr (sizeof(T) == 4) { MGX_CASE(16, 9) MGX_CASE(16, 10) MGX_CASE(16, 11) MGX_CASE(16, 12) }
    if constexpr (sizeof(T) == 8) { MGX_CASE(64, 3) }
    MGX_CASE(64, 4) MGX_CASE(64, 5) MGX_CASE(64, 6) MGX_CASE(64, 7) MGX_CASE(64, 8)
    MGX_CASE(64, 9) MGX_CASE(64, 10) MGX_CASE(64, 11) MGX_CASE(64, 12)
    MGX_CASE(64, 13) MGX_CASE(64, 14) MGX_CASE(64, 15) MGX_CASE(64, 16)
#undef MGX_CASE
    return nullptr;
}

}  // namespace
