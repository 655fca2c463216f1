// pairhmm_cell.h -- the PairHMM cell: a row's model values, the algebraic forms of the cell with the per-row coefficients each needs, and
// the rules around them (which form, what the five-operation form defers, the result, the re-run thresholds).  The one statement of all
// that: pairhmm_body (pairhmm_kernels.hip.inc) computes with these functions in its lane layout, tools/cell_emulator.cpp in a plain
// row-by-row sweep on the CPU, so both round alike by construction.  Plain C++17, no HIP types, nothing that needs a wavefront.
// Every function states ONE expression and takes its arithmetic through a policy `A` (fma, mul, add, sub, div, each rounded on its own):
// Bare below on the device, where the compile flags flush subnormal results; the emulator's flushes them itself.  (Three integer
// expressions -- q7, pMM_of's index, mismatch_of's select -- the kernel writes out itself, for its register allocation: DESIGN.md 3.2.)
//
// The reference's cell (avx-pairhmm-template.h:177-192), M2 X2 Y2 from the row above and the previous column, M1 X1 from the row above,
// Ml Yl from the previous column:
//  plain, 8 ops per cell (fused; `exact` is the same, unfused, for the last fp64 tier):
//      M = ((M2*pMM + X2*pGAPM) + Y2*pGAPM) * e ;  X = M1*pMX + X1*pXX ;  Y = Ml*pMY + Yl*pYY
//  scaled (fp64), 7 ops per cell: rows carry X^ = g'*X and Y^ = g'*Y, g' = pGAPM of the row BELOW
//  (the only consumer of X and Y across rows), so the consumer needs no multiply:
//      M  = (fma(pMM, M2, X^2) + Y^2) * e
//      X^ = A*M1 + B*X^1     A = g'*pMX,  B = g'*pXX/g   (g = this row's pGAPM)
//      Y^ = C*Ml + D*Y^l     C = g'*pMY,  D = pYY
//  Read row R has no row below: g' = 1 there, so its X^ is X and the final sums are unchanged.
//  six (fp32), 6 ops per cell: X^ as in the scaled form, Y carried as y = Y / pMY of its own row.  Y's
//  recurrence runs along the row, so that scale never changes along it and y needs no multiply:
//      M  = fma(q, y2, fma(pMM, M2, X^2)) * e     q = g * pMY' (pMY' = pMY of the row above, 1 for row 0)
//      X^ = A*M1 + B*X^1
//      y  = pYY*yl + Ml
//  The match-to-match path (pMM, e) carries table values only, as in the reference: a rounded per-row
//  product on it (e*g or pMM/g) adds a bias of up to an ulp per row, which over a 1000-row read
//  reaches 1.5e-5 in log10 (tools/dev_cell_emulate.py).  y <= max M / (1 - pYY) <= 4.9 max M for
//  gap-continuation bytes >= 1, and pMY' is a table value, so q has the same bits wherever the row
//  above lives (this lane, the lane above, the previous strip).
//  B divides by g, so a test case with a row of pGAPM == 0 (gap-continuation byte 0) takes the plain form (on the device: its wavefront).
//  five (fp32), 5 ops per cell: each row rescaled once more, m = s*M, x = X^ / A', yb = s*y with s = pMM of
//  the row below (1 for read row R) and A' = g'*pMX / pMM of the row itself:
//      m  = fma(q', yb2, fma(a, x2, m2)) * E     q' = g * pMY' / pMM,  a = A' of the row above,  E = e * s
//      x  = fma(x1, B', m1)                      B' = g' * (pXX / g) * a / A'
//      yb = fma(ybl, pYY, ml)
//  Above read row 0: a = B' = 0 and q' = g (the boundary row keeps y = INITIAL/H unscaled).  Read row R has
//  s = g' = 1, so sum M is sum m and sum X is A' * sum x: one multiply per test case.  E is rounded once, when the
//  table is built: the match-to-match path now carries one rounded product per row, which is why the form stops
//  at the 192 rows of the 16-lane classes (with two such products, form 2 of the emulator, 1000-row reads reach
//  1.5e-5; with one, reads of up to 192 rows stay at the 6-operation cell's 3.8e-6 / 7.6e-6:
//  profiles/pairhmm_fiveop_emulation.txt).  The form divides by pMM and, through A', by g': a test case with a
//  zero among them is deferred before the sweep (five_defers_row), and x is as large as M, not as X, so rows whose
//  insertion qualities differ by tens of dB can overflow fp32: every term is non-negative, an overflow reaches
//  the last row's sums as inf or NaN, and such a result is deferred after the sweep (five_overflowed).  Both per test
//  case, to the second launch of its class, which computes it in the forms above.
//  What crosses from a row to the row below, in the five-operation form.  The row below reads its row above in two expressions only:
//  the three paths into m, fma(q', yb2, fma(a, x2, m2)), whose m2 x2 yb2 are all of ONE column of the row above, and x = fma(x1, B', m1),
//  whose m1 x1 are of one column too.  So the row above can evaluate both itself, with the lower row's a, q' and B', and hand down two
//  values (five_paths_down, five_x_down) instead of three: the same operations on the same operand bits wherever they are computed.
//  Above read row 0 the paths value is the constant five_boundary_paths = round(q' * INITIAL/H) (0 under a row-0 clone, whose q' is 0),
//  and x is 0.
//  Sum of m along read row R.  Nothing reads row R's yb.  With pYY := 1 in that one row (Edge::pYY_sum_row) the row's own
//  yb = fma(ybl, 1, ml) = round(ybl + ml) makes, column by column from yb = 0, the very additions of sum += m: after the last column
//  yb holds the sum of every m but the last, and sum m = five_sum_m(yb, m) = round(yb + m).
// A row-0 clone (a spare row above read row 0) has every coefficient 0 and pYY = 1: it hands the boundary row on unchanged.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MGX_CELL_FN __host__ __device__ __forceinline__
#else
#define MGX_CELL_FN inline
#endif

namespace mgx_hmm_cell {

constexpr double kExactBelow = 1e-280;       // fp64 results below this go to the exact tier (2^-1022 ~ 2.2e-308)
constexpr float kFloatFirstBelow = 1e-28f;   // fp32 results below this are computed again in fp64 (IntelPairHmm.cc:338-350)
constexpr float kFloatMax = 3.402823466e+38f;
constexpr int kCodeN = 4;
template <typename T> MGX_CELL_FN constexpr T initial() { if constexpr (sizeof(T) == 4) return 0x1p120f; else return 0x1p1020; }   // Context.h:183, :142

MGX_CELL_FN int base_code(int b) {       // pairhmm_common.h:75-81 -- A=0 C=1 T=2 G=3 N=4, anything else 0
    int c = 0;
    c = (b == 'C') ? 1 : c;
    c = (b == 'T') ? 2 : c;
    c = (b == 'G') ? 3 : c;
    c = (b == 'N') ? kCodeN : c;
    return c;
}

struct Bare {      // the operations as the compiler rounds them
    static MGX_CELL_FN float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
    static MGX_CELL_FN double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
    template <typename T> static MGX_CELL_FN T mul(T a, T b) { return a * b; }
    template <typename T> static MGX_CELL_FN T add(T a, T b) { return a + b; }
    template <typename T> static MGX_CELL_FN T sub(T a, T b) { return a - b; }
    template <typename T> static MGX_CELL_FN T div(T a, T b) { return a / b; }
};

// ---- a row's model values (ReadForPairHMM.cpp:62-80, avx-pairhmm-template.h:129-171) from the tables and its qualities: q7 of the
// base quality byte (qq), the insertion / deletion quality bytes (qi / qd) and the gap-continuation byte (qc)
MGX_CELL_FN int q7(int byte) { return byte & 127; }                      // seven bits count (ReadForPairHMM.cpp:34-36)
template <typename T> MGX_CELL_FN T pMM_of(const T* mm, int qi, int qd) {
    const int mn = qi <= qd ? qi : qd, mx = qi <= qd ? qd : qi;
    return mm[((mx * (mx + 1)) >> 1) + mn];
}
template <class A, typename T> MGX_CELL_FN T pGAPM_of(const T* ph2pr, int qc) { return A::sub((T)1.0, ph2pr[qc]); }          // g
template <typename T> MGX_CELL_FN T pXX_of(const T* ph2pr, int qc) { return ph2pr[qc]; }                                     // = pYY
template <typename T> MGX_CELL_FN T pMX_of(const T* ph2pr, int qi) { return ph2pr[qi]; }
template <typename T> MGX_CELL_FN T pMY_of(const T* ph2pr, int qd) { return ph2pr[qd]; }
template <class A, typename T> MGX_CELL_FN T match_of(const T* ph2pr, int qq) { return A::sub((T)1.0, ph2pr[qq]); }
template <typename T> MGX_CELL_FN T mismatch_of(const T* ph2pr_div3, int qq, int code, T match) { return code == kCodeN ? match : ph2pr_div3[qq]; }
template <typename T> MGX_CELL_FN T ratio_of(const T* gap_ratio, int qc) { return gap_ratio[qc]; }                          // pXX / g, 0 at g = 0
MGX_CELL_FN bool is_match(int read_code, int hap_code) { return read_code == hap_code || read_code == kCodeN || hap_code == kCodeN; }
template <class A, typename T> MGX_CELL_FN T initial_y(int H) { return A::div(initial<T>(), (T)(H > 0 ? H : 1)); }                // Y of the boundary row

// ---- boundary conventions of the fast forms: below read row R, g' = s = 1; above read row 0, pMY' = 1 and A' = 0 (so a = B' = 0)
template <typename T> struct Edge {
    static MGX_CELL_FN constexpr T g_below() { return 1; }
    static MGX_CELL_FN constexpr T s_below() { return 1; }
    static MGX_CELL_FN constexpr T pMY_above() { return 1; }
    static MGX_CELL_FN constexpr T A_above() { return 0; }
    static MGX_CELL_FN constexpr T pYY_sum_row() { return 1; }      // five: read row R sums its m in its yb
};

// ---- per-row coefficients; gb = g of the row below, every product and quotient rounded on its own
template <class A, typename T> MGX_CELL_FN T scaled_A(T gb, T pMX) { return A::mul(gb, pMX); }
template <class A, typename T> MGX_CELL_FN T scaled_B(T gb, T ratio) { return A::mul(gb, ratio); }          // the five-operation form's g' pXX / g too
template <class A, typename T> MGX_CELL_FN T scaled_C(T gb, T pMY) { return A::mul(gb, pMY); }
template <class A, typename T> MGX_CELL_FN T scaled_Y0(T g_first, T init_y) { return A::mul(g_first, init_y); }   // Y^ of the boundary row, g_first of read row 0
template <class A, typename T> MGX_CELL_FN T six_q(T g, T pMY_above) { return A::mul(g, pMY_above); }
template <class A, typename T> MGX_CELL_FN T five_rcp(T pMM) { return A::div((T)1.0, pMM); }                 // the one reciprocal A' and q' share
template <class A, typename T> MGX_CELL_FN T five_Ap(T gb, T pMX, T rcp) { return A::mul(A::mul(gb, pMX), rcp); }
template <class A, typename T> MGX_CELL_FN T five_q(T g, T pMY_above, T rcp) { return A::mul(A::mul(g, pMY_above), rcp); }   // read row 0: q' = g itself
template <class A, typename T> MGX_CELL_FN T five_Bp(T gr, T A_above, T Ap) { return A::div(A::mul(gr, A_above), Ap); }       // gr = scaled_B
template <class A, typename T> MGX_CELL_FN T five_E(T e, T s) { return A::mul(e, s); }                       // s = pMM of the row below

// ---- the cells, one function per new value.  The six- and five-operation M is emit(paths): the kernel updates a lane's rows in place,
// bottom row first, and puts the row's y update between the two
template <class A, typename T> MGX_CELL_FN T emit(T paths, T e) { return A::mul(paths, e); }
template <class A, typename T> MGX_CELL_FN T plain_M(T M2, T X2, T Y2, T pMM, T g, T e) { return A::mul(A::fma(Y2, g, A::fma(X2, g, A::mul(M2, pMM))), e); }
template <class A, typename T> MGX_CELL_FN T plain_X(T M1, T X1, T pMX, T pXX) { return A::fma(X1, pXX, A::mul(M1, pMX)); }
template <class A, typename T> MGX_CELL_FN T plain_Y(T Ml, T Yl, T pMY, T pYY) { return A::fma(Yl, pYY, A::mul(Ml, pMY)); }
template <class A, typename T> MGX_CELL_FN T exact_M(T M2, T X2, T Y2, T pMM, T g, T e) { return A::mul(A::add(A::add(A::mul(M2, pMM), A::mul(X2, g)), A::mul(Y2, g)), e); }
template <class A, typename T> MGX_CELL_FN T exact_X(T M1, T X1, T pMX, T pXX) { return A::add(A::mul(M1, pMX), A::mul(X1, pXX)); }
template <class A, typename T> MGX_CELL_FN T exact_Y(T Ml, T Yl, T pMY, T pYY) { return A::add(A::mul(Ml, pMY), A::mul(Yl, pYY)); }
template <class A, typename T> MGX_CELL_FN T scaled_M(T M2, T X2, T Y2, T pMM, T e) { return A::mul(A::add(A::fma(M2, pMM, X2), Y2), e); }
template <class A, typename T> MGX_CELL_FN T scaled_X(T M1, T X1, T cA, T cB) { return A::fma(X1, cB, A::mul(M1, cA)); }       // the six-operation form's X^ too
template <class A, typename T> MGX_CELL_FN T scaled_Y(T Ml, T Yl, T cC, T cD) { return A::fma(Yl, cD, A::mul(Ml, cC)); }
template <class A, typename T> MGX_CELL_FN T six_M_paths(T M2, T X2, T y2, T pMM, T q) { return A::fma(q, y2, A::fma(M2, pMM, X2)); }
template <class A, typename T> MGX_CELL_FN T six_y(T Ml, T yl, T pYY) { return A::fma(yl, pYY, Ml); }                          // the five-operation form's yb too
template <class A, typename T> MGX_CELL_FN T five_m_paths(T m2, T x2, T yb2, T a, T q) { return A::fma(q, yb2, A::fma(a, x2, m2)); }
template <class A, typename T> MGX_CELL_FN T five_x(T m1, T x1, T Bp) { return A::fma(x1, Bp, m1); }
// the two values a row hands to the row below (a, q, Bp: the LOWER row's), and what read row 0 gets from the boundary row
template <class A, typename T> MGX_CELL_FN T five_paths_down(T m, T x, T yb, T a_below, T q_below) { return five_m_paths<A>(m, x, yb, a_below, q_below); }
template <class A, typename T> MGX_CELL_FN T five_x_down(T m, T x, T Bp_below) { return five_x<A>(m, x, Bp_below); }
template <class A, typename T> MGX_CELL_FN T five_boundary_paths(T init_y, T a, T q) { return five_m_paths<A>((T)0, (T)0, init_y, a, q); }
template <class A, typename T> MGX_CELL_FN T five_sum_m(T yb_last, T m_last) { return A::add(yb_last, m_last); }      // read row R, pYY = pYY_sum_row

// ---- the rules around the cell
MGX_CELL_FN bool row_needs_plain(int qc) { return qc == 0; }                                    // a test case with such a row takes the plain form
template <typename T> MGX_CELL_FN bool row_has_zero_pMM(T pMM) { return pMM == (T)0; }
// the five-operation form, the static rule: a test case with such a row is deferred before the sweep ...
template <typename T> MGX_CELL_FN bool five_defers_row(T pMM, int qc) { return row_has_zero_pMM(pMM) || row_needs_plain(qc); }
// ... the dynamic rule: so is one whose result is not finite (tested before the float-first comparison)
MGX_CELL_FN bool five_overflowed(float res) { return !(res <= kFloatMax); }
template <class A, typename T> MGX_CELL_FN T result(T sumM, T sumX) { return A::add(sumM, sumX); }
template <class A, typename T> MGX_CELL_FN T five_result(T sum_m, T Ap_last, T sum_x) { return A::add(sum_m, A::mul(Ap_last, sum_x)); }   // Ap_last: A' of read row R

}  // namespace mgx_hmm_cell
