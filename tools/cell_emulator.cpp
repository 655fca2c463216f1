// cell_emulator.cpp -- the fp32 PairHMM cells of pairhmm_body (csrc/pairhmm_kernels.hip.inc) on the host, for numerics checks on a
// machine without a GPU (tests/pairhmm_fiveop_cases.py builds and drives it).  The forms, their per-row coefficients, the deferral
// rules and the result are csrc/pairhmm_cell.h, the header the kernel computes with; here they run in a plain row-by-row sweep.
//   form 0: the plain 8-operation cell; whatever form is asked for, a test case with a gap-continuation byte of 0 takes it
//   form 1: the scaled 7-operation cell the fp32 kernels ran before
//   form 2: a 6-operation cell with X as it is, y = Y / pMY of its own row, E = e*pGAPM, p = pMM/pGAPM.  No kernel runs it (the two
//           rounded products on the match-to-match path of every row cost up to 1.5e-5 in log10 on reads of ~1000 bases), so its
//           two coefficients are stated here and not in the header; its cells are the header's
//   form 3: the 6-operation cell
//   form 4: the first launch of the classes of up to 16 lanes: the 5-operation cell for reads of at most kFiveOpMaxRows bases.  A test
//           case it defers (the static or the dynamic rule), one whose haplotype holds an N and a longer read are computed in form 3.
//           cell_emulate_paths / cell_emulate_deferrals tell which way every test case of the last batch went.
// The arithmetic handed to the header (Ftz) flushes every rounded result to zero when it is subnormal, as the device does
// (-fgpu-flush-denormals-to-zero); the file is built with -ffp-contract=off.  The tables are the product's own (csrc/mgx_tables.cpp).
// A cell's value does not depend on the lane layout on the device, so the sweep gives the kernel's bits up to the final log10f.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mgx_tables.h"
#include "pairhmm_cell.h"
#include "pairhmm_plan.h"      // kFiveOpMaxRows

namespace {

namespace cell = mgx_hmm_cell;
using Edge = cell::Edge<float>;

struct Ftz {
    static float ftz(float v) { return std::fabs(v) < 0x1p-126f ? std::copysign(0.0f, v) : v; }
    static float fma(float a, float b, float c) { return ftz(std::fmaf(a, b, c)); }
    static float mul(float a, float b) { return ftz(a * b); }
    static float add(float a, float b) { return ftz(a + b); }
    static float sub(float a, float b) { return ftz(a - b); }
    static float div(float a, float b) { return ftz(a / b); }
};

enum Form { kPlain = 0, kScaled = 1, kSixA = 2, kSix = 3, kFirstLaunch = 4, kFive = 5 };
// which way a test case went under form 4
enum Path : uint8_t { kPathFive = 0, kPathStatic = 1, kPathDynamic = 2, kPathHapN = 3, kPathLong = 4 };
std::vector<uint8_t> g_paths;      // of the last cell_emulate_batch call

struct Rows {                      // a read's model values per row, and the haplotype's codes
    std::vector<float> pMM, g, pMX, pXX, pMY, eM, eX, ratio;
    std::vector<int> rc, hc;
};

// sum_c M[R][c] + sum_c X[R][c] in form F, scaled by 2^120 (the kernel's `res`)
template <int F>
float sweep(const Rows& r) {
    const int R = (int)r.rc.size(), H = (int)r.hc.size();
    const float init_y = cell::initial_y<Ftz, float>(H);
    // rows above (index c = 0..H, column 0 is the DP's column 0); the boundary row: Y = INITIAL / H, Y^ in the scaled form
    std::vector<float> Mu(H + 1, 0.0f), Xu(H + 1, 0.0f), Yu(H + 1, F == kScaled && R > 0 ? cell::scaled_Y0<Ftz>(r.g[0], init_y) : init_y);
    std::vector<float> Mc(H + 1), Xc(H + 1), Yc(H + 1);
    float Ap = Edge::A_above();                  // kFive: A' of the row above, in the end of read row R
    for (int i = 0; i < R; ++i) {
        const bool last = i + 1 == R;
        const float pMM = r.pMM[i], g = r.g[i], pMX = r.pMX[i], pXX = r.pXX[i], pMY = r.pMY[i];
        const float gb = last ? Edge::g_below() : r.g[i + 1], s = last ? Edge::s_below() : r.pMM[i + 1];
        const float my_above = i ? r.pMY[i - 1] : Edge::pMY_above();
        float cA = 0, cB = 0, cC = 0, eM = r.eM[i], eX = r.eX[i];      // the form's coefficients, and its emissions
        if constexpr (F == kScaled || F == kSix) {
            cA = cell::scaled_A<Ftz>(gb, pMX);
            cB = cell::scaled_B<Ftz>(gb, r.ratio[i]);
            cC = F == kSix ? cell::six_q<Ftz>(g, my_above) : cell::scaled_C<Ftz>(gb, pMY);
        } else if constexpr (F == kSixA) {
            cA = Ftz::mul(pMM, g != 0.0f ? 1.0f / g : 0.0f);           // p
            eM = Ftz::mul(eM, g); eX = Ftz::mul(eX, g);                // E
        } else if constexpr (F == kFive) {
            const float rcp = cell::five_rcp<Ftz>(pMM);
            cA = Ap;                                                   // a
            Ap = cell::five_Ap<Ftz>(gb, pMX, rcp);
            cB = cell::five_Bp<Ftz>(cell::scaled_B<Ftz>(gb, r.ratio[i]), cA, Ap);
            cC = i ? cell::five_q<Ftz>(g, my_above, rcp) : g;
            eM = cell::five_E<Ftz>(eM, s); eX = cell::five_E<Ftz>(eX, s);
        }
        Mc[0] = 0.0f; Xc[0] = 0.0f; Yc[0] = 0.0f;
        for (int c = 1; c <= H; ++c) {
            const float e = cell::is_match(r.rc[i], r.hc[c - 1]) ? eM : eX;
            const float M2 = Mu[c - 1], X2 = Xu[c - 1], Y2 = Yu[c - 1], M1 = Mu[c], X1 = Xu[c], Ml = Mc[c - 1], Yl = Yc[c - 1];
            if constexpr (F == kPlain) {
                Mc[c] = cell::plain_M<Ftz>(M2, X2, Y2, pMM, g, e); Xc[c] = cell::plain_X<Ftz>(M1, X1, pMX, pXX); Yc[c] = cell::plain_Y<Ftz>(Ml, Yl, pMY, pXX);
            } else if constexpr (F == kScaled) {
                Mc[c] = cell::scaled_M<Ftz>(M2, X2, Y2, pMM, e); Xc[c] = cell::scaled_X<Ftz>(M1, X1, cA, cB); Yc[c] = cell::scaled_Y<Ftz>(Ml, Yl, cC, pXX);
            } else if constexpr (F == kSix) {
                Mc[c] = cell::emit<Ftz>(cell::six_M_paths<Ftz>(M2, X2, Y2, pMM, cC), e); Xc[c] = cell::scaled_X<Ftz>(M1, X1, cA, cB); Yc[c] = cell::six_y<Ftz>(Ml, Yl, pXX);
            } else if constexpr (F == kSixA) {
                Mc[c] = cell::emit<Ftz>(cell::six_M_paths<Ftz>(M2, X2, Y2, cA, my_above), e); Xc[c] = cell::plain_X<Ftz>(M1, X1, pMX, pXX); Yc[c] = cell::six_y<Ftz>(Ml, Yl, pXX);
            } else {
                // as the kernel hands them down: the paths value and x from the row above (the boundary row above read row 0); read row R
                // sums its m in its yb
                const float paths = i ? cell::five_paths_down<Ftz>(M2, X2, Y2, cA, cC) : cell::five_boundary_paths<Ftz>(Y2, cA, cC);
                Mc[c] = cell::emit<Ftz>(paths, e); Xc[c] = cell::five_x_down<Ftz>(M1, X1, cB);
                Yc[c] = cell::six_y<Ftz>(Ml, Yl, last ? Edge::pYY_sum_row() : pXX);
            }
        }
        std::swap(Mu, Mc); std::swap(Xu, Xc); std::swap(Yu, Yc);
    }
    float sumM = 0.0f, sumX = 0.0f;
    for (int c = 1; c <= H; ++c) { sumM = Ftz::add(sumM, Mu[c]); sumX = Ftz::add(sumX, Xu[c]); }
    if (F == kFive && R > 0) sumM = cell::five_sum_m<Ftz>(Yu[H], Mu[H]);      // the row's yb after the last column, and the last m
    return F == kFive ? cell::five_result<Ftz>(sumM, Ap, sumX) : cell::result<Ftz>(sumM, sumX);
}

float forward(int form, int R, const uint8_t* bases, const uint8_t* qual, const uint8_t* ins, const uint8_t* del,
              const uint8_t* gcp, int H, const uint8_t* hap, uint8_t* path) {
    const auto& t = mgx::tables<float>();
    Rows r;
    for (auto* v : {&r.pMM, &r.g, &r.pMX, &r.pXX, &r.pMY, &r.eM, &r.eX, &r.ratio}) v->resize(R);
    r.rc.resize(R); r.hc.resize(H);
    bool plain = false, five_defers = false, hap_n = false;
    for (int i = 0; i < R; ++i) {
        const int qi = cell::q7(ins[i]), qd = cell::q7(del[i]), qc = cell::q7(gcp[i]), qq = cell::q7(qual[i]);
        r.pMM[i] = cell::pMM_of(t.mm.data(), qi, qd);
        r.g[i] = cell::pGAPM_of<Ftz>(t.ph2pr.data(), qc);
        r.pMX[i] = cell::pMX_of(t.ph2pr.data(), qi);
        r.pXX[i] = cell::pXX_of(t.ph2pr.data(), qc);
        r.pMY[i] = cell::pMY_of(t.ph2pr.data(), qd);
        r.eM[i] = cell::match_of<Ftz>(t.ph2pr.data(), qq);
        r.rc[i] = cell::base_code(bases[i]);
        r.eX[i] = cell::mismatch_of(t.ph2pr_div3.data(), qq, r.rc[i], r.eM[i]);
        r.ratio[i] = cell::ratio_of(t.gap_ratio.data(), qc);
        plain |= cell::row_needs_plain(qc);
        five_defers |= cell::five_defers_row(r.pMM[i], qc);
    }
    for (int c = 0; c < H; ++c) { r.hc[c] = cell::base_code(hap[c]); hap_n |= r.hc[c] == cell::kCodeN; }
    if (form == kFirstLaunch) {
        // the kernel's order: a haplotype with an N goes to the list whatever the read holds, then the static rule
        uint8_t way = R > mgx_hmm_plan::kFiveOpMaxRows ? kPathLong : hap_n ? kPathHapN : five_defers ? kPathStatic : kPathFive;
        if (way == kPathFive) {
            const float res = sweep<kFive>(r);
            if (!cell::five_overflowed(res)) { *path = way; return res; }
            way = kPathDynamic;
        }
        *path = way;
        form = kSix;
    }
    if (plain) form = kPlain;
    switch (form) {
        case kPlain: return sweep<kPlain>(r);
        case kScaled: return sweep<kScaled>(r);
        case kSixA: return sweep<kSixA>(r);
        case kFive: return sweep<kFive>(r);
        default: return sweep<kSix>(r);
    }
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
// the four fp32 tables the cells read (128, 32640, 128 and 128 values), as this machine's libm built them
void cell_emulate_tables(float* ph2pr, float* mm, float* ph2pr_div3, float* gap_ratio) {
    const auto& t = mgx::tables<float>();
    std::memcpy(ph2pr, t.ph2pr.data(), t.ph2pr.size() * sizeof(float));
    std::memcpy(mm, t.mm.data(), t.mm.size() * sizeof(float));
    std::memcpy(ph2pr_div3, t.ph2pr_div3.data(), t.ph2pr_div3.size() * sizeof(float));
    std::memcpy(gap_ratio, t.gap_ratio.data(), t.gap_ratio.size() * sizeof(float));
}
}
