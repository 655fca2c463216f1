// cell_emulator.cpp -- host restatement of the fp32 PairHMM cells of pairhmm_body (csrc/pairhmm_kernels.hip.inc),
// for numerics checks on a machine without a GPU (tools/dev_cell_emulate.py builds and drives it).
//   form 1: the scaled 7-operation cell (X^ = g'X, Y^ = g'Y, g' = pGAPM of the row below) the fp32 kernels ran before
//   form 2: a 6-operation cell with X as it is, y = Y / pMY of its own row, E = e*pGAPM, p = pMM/pGAPM (not used: the two
//           rounded products on the match-to-match path of every row cost up to 1.5e-5 in log10 on reads of ~1000 bases)
//   form 3: the 6-operation cell: X^ = g'X as in form 1, y = Y / pMY of its own row, q = pGAPM * pMY'
//   form 4: the 5-operation cell of the first launch of the classes of up to 16 lanes (reads of at most 192 bases; longer
//           reads stay with form 3): m = s*M, x = X^ / A', yb = s*y with s = pMM of the row below and A' = g'*pMX/pMM, the
//           emission carried as E = e*s.  A test case it cannot take -- statically: a row with pMM == 0 or a
//           gap-continuation byte of 0; dynamically: a result that is not finite -- is deferred to the second launch, as
//           is one whose haplotype holds an N: those are computed in form 3 (form 0 with a gap-continuation byte of 0).
//           cell_emulate_paths / cell_emulate_deferrals tell which way every test case of the last batch went.
// A test case with a gap-continuation byte of 0 takes the plain 8-operation form (form 0), as its wavefront does.
// Every multiply-add is an explicit fmaf, the file is built with -ffp-contract=off, and every rounded result is flushed to
// zero when it is subnormal, as the device does (-fgpu-flush-denormals-to-zero).  The tables are the product's own
// (csrc/mgx_tables.cpp).  A cell's value does not depend on the lane layout on the device, so a plain row-by-row sweep
// gives the kernel's bits up to the final log10f.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mgx_tables.h"

namespace {

inline float ftz(float v) { return std::fabs(v) < 0x1p-126f ? std::copysign(0.0f, v) : v; }
inline float fma_(float a, float b, float c) { return ftz(std::fmaf(a, b, c)); }
inline float mul(float a, float b) { return ftz(a * b); }
inline float add(float a, float b) { return ftz(a + b); }
inline float div(float a, float b) { return ftz(a / b); }

// which way a test case went under form 4
enum Path : uint8_t { kPathFive = 0, kPathStatic = 1, kPathDynamic = 2, kPathHapN = 3, kPathLong = 4 };
constexpr int kFiveOpMaxRows = 192;
std::vector<uint8_t> g_paths;      // of the last cell_emulate_batch call

int code_of(uint8_t b) { return b == 'C' ? 1 : b == 'T' ? 2 : b == 'G' ? 3 : b == 'N' ? 4 : 0; }

// sum_c M[R][c] + sum_c X[R][c] of one test case, scaled by 2^120 (the kernel's `res`)
float forward(int form, int R, const uint8_t* bases, const uint8_t* qual, const uint8_t* ins, const uint8_t* del,
              const uint8_t* gcp, int H, const uint8_t* hap, uint8_t* path = nullptr) {
    const auto& t = mgx::tables<float>();
    const float init_y = 0x1p120f / (float)(H > 0 ? H : 1);
    if (form == 4) {
        // the kernel's order: a haplotype with an N goes to the list whatever the read holds, then the static rule
        uint8_t way = kPathFive;
        if (R > kFiveOpMaxRows) way = kPathLong;
        if (way == kPathFive) for (int c = 0; c < H; ++c) if (hap[c] == 'N') way = kPathHapN;
        if (way == kPathFive)
            for (int i = 0; i < R; ++i) {
                const int qi = ins[i] & 127, qd = del[i] & 127;
                const int mn = qi <= qd ? qi : qd, mx = qi <= qd ? qd : qi;
                if ((gcp[i] & 127) == 0 || t.mm[((mx * (mx + 1)) >> 1) + mn] == 0.0f) way = kPathStatic;
            }
        if (way == kPathFive) {
            const float res = forward(5, R, bases, qual, ins, del, gcp, H, hap);
            if (res <= 3.402823466e+38f) { if (path) *path = way; return res; }
            way = kPathDynamic;
        }
        if (path) *path = way;
        form = 3;
    }
    for (int i = 0; i < R; ++i) if ((gcp[i] & 127) == 0) form = 0;
    std::vector<float> pMM(R), g(R), pMX(R), pXX(R), pMY(R), eM(R), eX(R), gratio(R), ginv(R);
    std::vector<int> rc(R);
    for (int i = 0; i < R; ++i) {
        const int qi = ins[i] & 127, qd = del[i] & 127, qc = gcp[i] & 127, qq = qual[i] & 127;
        const int mn = qi <= qd ? qi : qd, mx = qi <= qd ? qd : qi;
        pMM[i] = t.mm[((mx * (mx + 1)) >> 1) + mn];
        g[i] = 1.0f - t.ph2pr[qc];
        pMX[i] = t.ph2pr[qi];
        pXX[i] = t.ph2pr[qc];
        pMY[i] = t.ph2pr[qd];
        eM[i] = 1.0f - t.ph2pr[qq];
        rc[i] = code_of(bases[i]);
        eX[i] = rc[i] == 4 ? eM[i] : t.ph2pr_div3[qq];
        gratio[i] = t.gap_ratio[qc];
        ginv[i] = g[i] != 0.0f ? 1.0f / g[i] : 0.0f;
    }
    std::vector<int> hc(H);
    for (int c = 0; c < H; ++c) hc[c] = code_of(hap[c]);
    // rows above (index c = 0..H, column 0 is the DP's column 0)
    std::vector<float> Mu(H + 1, 0.0f), Xu(H + 1, 0.0f), Yu(H + 1), Mc(H + 1), Xc(H + 1), Yc(H + 1);
    float sumM = 0.0f, sumX = 0.0f;
    // boundary row: Y = INITIAL / H (form 1: scaled by pGAPM of row 1; form 2: y_0 = Y_0 with pMY_0 := 1)
    for (int c = 0; c <= H; ++c) Yu[c] = form == 1 ? (R > 0 ? mul(g[0], init_y) : init_y) : init_y;
    if (form == 0) {
        for (int i = 0; i < R; ++i) {
            Mc[0] = 0.0f; Xc[0] = 0.0f; Yc[0] = 0.0f;
            for (int c = 1; c <= H; ++c) {
                const bool match = rc[i] == hc[c - 1] || rc[i] == 4 || hc[c - 1] == 4;
                const float e = match ? eM[i] : eX[i];
                Mc[c] = mul(fma_(Yu[c - 1], g[i], fma_(Xu[c - 1], g[i], mul(Mu[c - 1], pMM[i]))), e);
                Xc[c] = fma_(Xu[c], pXX[i], mul(Mu[c], pMX[i]));
                Yc[c] = fma_(Yc[c - 1], pXX[i], mul(Mc[c - 1], pMY[i]));
            }
            std::swap(Mu, Mc); std::swap(Xu, Xc); std::swap(Yu, Yc);
        }
        for (int c = 1; c <= H; ++c) { sumM = add(sumM, Mu[c]); sumX = add(sumX, Xu[c]); }
        return add(sumM, sumX);
    }
    if (form == 5) {
        // the 5-operation sweep itself (form 4 without its deferral rules): Mu, Xu, Yu hold m, x, yb
        float A_above = 0.0f, A_last = 0.0f;
        for (int i = 0; i < R; ++i) {
            Mc[0] = 0.0f; Xc[0] = 0.0f; Yc[0] = 0.0f;
            const float gb = i + 1 < R ? g[i + 1] : 1.0f, s = i + 1 < R ? pMM[i + 1] : 1.0f;
            const float rcp = div(1.0f, pMM[i]);
            const float Ap = mul(mul(gb, pMX[i]), rcp);
            const float q = i > 0 ? mul(mul(g[i], pMY[i - 1]), rcp) : g[0];
            const float a = A_above;
            const float Bp = div(mul(mul(gb, gratio[i]), A_above), Ap);
            const float EM = mul(eM[i], s), EX = mul(eX[i], s);
            for (int c = 1; c <= H; ++c) {
                const bool match = rc[i] == hc[c - 1] || rc[i] == 4 || hc[c - 1] == 4;
                const float E = match ? EM : EX;
                Mc[c] = mul(fma_(q, Yu[c - 1], fma_(a, Xu[c - 1], Mu[c - 1])), E);
                Xc[c] = fma_(Xu[c], Bp, Mu[c]);
                Yc[c] = fma_(Yc[c - 1], pXX[i], Mc[c - 1]);
            }
            std::swap(Mu, Mc); std::swap(Xu, Xc); std::swap(Yu, Yc);
            A_above = Ap; A_last = Ap;
        }
        if (R > 0)
            for (int c = 1; c <= H; ++c) { sumM = add(sumM, Mu[c]); sumX = add(sumX, Xu[c]); }
        return add(sumM, mul(A_last, sumX));
    }
    for (int i = 0; i < R; ++i) {
        Mc[0] = 0.0f; Xc[0] = 0.0f; Yc[0] = 0.0f;
        if (form == 1) {
            const float gb = i + 1 < R ? g[i + 1] : 1.0f;
            const float A = mul(gb, pMX[i]), B = mul(gb, gratio[i]), C = mul(gb, pMY[i]), D = pXX[i];
            for (int c = 1; c <= H; ++c) {
                const bool match = rc[i] == hc[c - 1] || rc[i] == 4 || hc[c - 1] == 4;
                const float e = match ? eM[i] : eX[i];
                Mc[c] = mul(add(fma_(Mu[c - 1], pMM[i], Xu[c - 1]), Yu[c - 1]), e);
                Xc[c] = fma_(Xu[c], B, mul(Mu[c], A));
                Yc[c] = fma_(Yc[c - 1], D, mul(Mc[c - 1], C));
            }
        } else if (form == 3) {
            const float gb = i + 1 < R ? g[i + 1] : 1.0f;
            const float A = mul(gb, pMX[i]), B = mul(gb, gratio[i]), q = mul(g[i], i > 0 ? pMY[i - 1] : 1.0f);
            for (int c = 1; c <= H; ++c) {
                const bool match = rc[i] == hc[c - 1] || rc[i] == 4 || hc[c - 1] == 4;
                const float e = match ? eM[i] : eX[i];
                Mc[c] = mul(fma_(q, Yu[c - 1], fma_(Mu[c - 1], pMM[i], Xu[c - 1])), e);
                Xc[c] = fma_(Xu[c], B, mul(Mu[c], A));
                Yc[c] = fma_(Yc[c - 1], pXX[i], Mc[c - 1]);
            }
        } else {
            const float p = mul(pMM[i], ginv[i]);
            const float my_above = i > 0 ? pMY[i - 1] : 1.0f;
            const float EM = mul(eM[i], g[i]), EX = mul(eX[i], g[i]);
            for (int c = 1; c <= H; ++c) {
                const bool match = rc[i] == hc[c - 1] || rc[i] == 4 || hc[c - 1] == 4;
                const float E = match ? EM : EX;
                Mc[c] = mul(fma_(my_above, Yu[c - 1], fma_(Mu[c - 1], p, Xu[c - 1])), E);
                Xc[c] = fma_(Xu[c], pXX[i], mul(Mu[c], pMX[i]));
                Yc[c] = fma_(Yc[c - 1], pXX[i], Mc[c - 1]);
            }
        }
        std::swap(Mu, Mc); std::swap(Xu, Xc); std::swap(Yu, Yc);
    }
    if (R > 0)
        for (int c = 1; c <= H; ++c) { sumM = add(sumM, Mu[c]); sumX = add(sumX, Xu[c]); }
    return add(sumM, sumX);
}

}  // namespace

extern "C" {
// out_res[k] = the kernel's fp32 `res` of test case k (pair_read / pair_hap index the read and haplotype tables)
void cell_emulate_batch(int form, int n, const uint32_t* pair_read, const uint32_t* pair_hap, const uint64_t* read_off,
                        const uint64_t* hap_off, const uint8_t* bases, const uint8_t* qual, const uint8_t* ins,
                        const uint8_t* del, const uint8_t* gcp, const uint8_t* hap, float* out_res) {
    mgx::tables<float>();
    g_paths.assign((size_t)(n > 0 ? n : 0), (uint8_t)kPathFive);
#pragma omp parallel for schedule(dynamic, 16)
    for (int k = 0; k < n; ++k) {
        const uint64_t r0 = read_off[pair_read[k]], r1 = read_off[pair_read[k] + 1];
        const uint64_t h0 = hap_off[pair_hap[k]], h1 = hap_off[pair_hap[k] + 1];
        out_res[k] = forward(form, (int)(r1 - r0), bases + r0, qual + r0, ins + r0, del + r0, gcp + r0, (int)(h1 - h0), hap + h0,
                             &g_paths[(size_t)k]);
    }
}
// form 4, the last batch: every test case's way (0 five-operation cell, 1 deferred by the static rule, 2 by the dynamic one,
// 3 haplotype with an N, 4 read too long for the form), and the two deferral counts
void cell_emulate_paths(int n, uint8_t* out) {
    for (int k = 0; k < n && (size_t)k < g_paths.size(); ++k) out[k] = g_paths[(size_t)k];
}
void cell_emulate_deferrals(uint64_t* n_static, uint64_t* n_dynamic) {
    *n_static = 0; *n_dynamic = 0;
    for (uint8_t w : g_paths) { *n_static += w == kPathStatic; *n_dynamic += w == kPathDynamic; }
}
}
