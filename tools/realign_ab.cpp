// realign_ab.cpp -- A/B of mgx_realign_regions against the composition of the calls that existed before it, through libmgx.so
// (driven by tools/dev_realign.py, which builds this into tools/bin/ and writes profiles/realign_ab.txt).
//   composed: mgx_pairhmm_regions; searchBestAllele and lastIndexOf on the host, single thread, as the reference does them;
//             host assembly of the aligner's input; mgx_sw_align_batch; scatter
//   fused:    mgx_realign_regions
// One process, the two take turns: one warm-up each, then `rounds` rounds; per round the wall time of each (host clock around calls
// that end in a device synchronise).  Results of the two are compared once, before the timing.
// With a tenth argument "to_ref" the same workloads, whose haplotypes then carry CIGARs with zero to two indels, go through
//   composed: mgx_realign_regions; then, over the kept reads, the aligner's text parsed and csrc/read_to_ref_rule.h run serially on the
//             host, single thread (what a caller of mgx_realign_regions writes today to finish createReadAlignedToRef)
//   fused:    mgx_realign_regions_to_ref
// usage: realign_ab n_regions n_reads n_haps read_min read_max hap_min hap_max verbatim_percent rounds [to_ref]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mgx_realign.h"
#include "read_to_ref_rule.h"

typedef uint8_t u8; typedef uint32_t u32; typedef uint64_t u64;

static u64 g_state = 0x243F6A8885A308D3ull;
static u32 rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (u32)(g_state >> 33); }
static u32 between(u32 lo, u32 hi) { return lo + rnd() % (hi - lo + 1); }
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define CHECK(call) do { const int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d %s\n", #call, rc_, mgx_last_error()); exit(2); } } while (0)

struct Region {
    std::vector<u64> read_off, hap_off;
    std::vector<u8> bases, qual, ins, del, gcp, haps, mapq;
    std::vector<double> pri;
    mgx_pairhmm_input_t in;
};
struct Outputs {
    std::vector<std::vector<double>> log10; std::vector<std::vector<u8>> keep;
    std::vector<std::vector<int32_t>> best, offset, score; std::vector<std::vector<char>> cigar;
    std::vector<double*> p_log10; std::vector<u8*> p_keep; std::vector<int32_t*> p_best, p_offset, p_score; std::vector<char*> p_cigar;
    void shape(const std::vector<Region>& rs, u32 stride) {
        const size_t n = rs.size();
        log10.resize(n); keep.resize(n); best.resize(n); offset.resize(n); score.resize(n); cigar.resize(n);
        for (size_t g = 0; g < n; ++g) {
            const size_t nr = rs[g].in.n_reads, nh = rs[g].in.n_haps;
            log10[g].assign(nr * nh, 0); keep[g].assign(nr, 0); best[g].assign(nr, 0); offset[g].assign(nr, 0); score[g].assign(nr, 0);
            cigar[g].assign(nr * stride, 0);
            p_log10.push_back(log10[g].data()); p_keep.push_back(keep[g].data()); p_best.push_back(best[g].data());
            p_offset.push_back(offset[g].data()); p_score.push_back(score[g].data()); p_cigar.push_back(cigar[g].data());
        }
    }
};

// AlleleLikelihoods::searchBestAllele(sample, read, canBeReference = true, priorities), sequentially, second-best bookkeeping included
static int search_best_allele(const double* log10, u64 n, const double* pri) {
    static const double ln10 = std::log(10), threshold = 0.2 * ln10;
    const double minus_inf = -std::numeric_limits<double>::infinity();
    int best = 0, second = 0;
    double best_l = log10[0] * ln10, second_l = minus_inf;
    for (u64 a = 1; a < n; ++a) {
        const double l = log10[a] * ln10;
        if (l > best_l) { second = best; best = (int)a; second_l = best_l; best_l = l; }
        else if (l > second_l) { second = (int)a; second_l = l; }
    }
    if (pri && best_l - second_l < threshold) {
        double best_p = pri[best], second_p = pri[second];
        for (u64 a = 0; a < n; ++a) {
            const double l = log10[a] * ln10;
            if ((int)a == best || best_l - l > threshold) continue;
            if (pri[a] > best_p) { second = best; best = (int)a; second_p = best_p; best_p = pri[a]; }
            else if (pri[a] > second_p) { second = (int)a; second_p = pri[a]; }
        }
    }
    (void)second;
    return best;
}
// the last verbatim occurrence of alt in ref, -1 if there is none
static int last_index_of(const u8* ref, u64 n_ref, const u8* alt, u64 n_alt) {
    if (n_alt > n_ref) return -1;
    for (int64_t s = (int64_t)(n_ref - n_alt); s >= 0; --s) if (memcmp(ref + s, alt, n_alt) == 0) return (int)s;
    return -1;
}

// ---- the to-reference leg
struct ToRefPart { std::vector<u64> off; std::vector<u32> el; std::vector<int32_t> hap_start; };
struct ToRefOutputs {
    std::vector<std::vector<int32_t>> start; std::vector<std::vector<u32>> rows, n; std::vector<std::vector<u8>> status;
    std::vector<int32_t*> p_start; std::vector<u32*> p_rows, p_n; std::vector<u8*> p_status;
    void shape(size_t n_regions, size_t n_reads, u32 stride) {
        start.assign(n_regions, std::vector<int32_t>(n_reads, 0)); rows.assign(n_regions, std::vector<u32>(n_reads * stride, 0));
        n.assign(n_regions, std::vector<u32>(n_reads, 0)); status.assign(n_regions, std::vector<u8>(n_reads, 0));
        for (size_t g = 0; g < n_regions; ++g) { p_start.push_back(start[g].data()); p_rows.push_back(rows[g].data()); p_n.push_back(n[g].data()); p_status.push_back(status[g].data()); }
    }
};
struct RowStore { u32* row; u32 room; void operator()(u32 k, u32 e) const { if (k < room) row[k] = e; } };
static int to_ref_ab(const std::vector<Region>& rs, const std::vector<mgx_pairhmm_input_t>& regions, const std::vector<const u8*>& mapq,
                     const std::vector<const double*>& pri, const mgx_read_model_t& model, const mgx_sw_params_t& params, mgx_pairhmm_t* hmm,
                     mgx_pairhmm_t* hmm_timed, mgx_sw_t* sw, u32 stride, u32 rounds, Outputs& A, Outputs& B) {
    namespace R = mgx_to_ref_rule;
    const u32 n_regions = (u32)rs.size(), n_reads = (u32)rs[0].in.n_reads, n_haps = (u32)rs[0].in.n_haps, row_stride = 16;
    // haplotype 0 is the reference haplotype (nM); the others carry zero to two indels, their read length is the haplotype's
    std::vector<ToRefPart> parts(n_regions);
    std::vector<mgx_to_ref_region_t> tr(n_regions);
    for (u32 g = 0; g < n_regions; ++g) {
        ToRefPart& P = parts[g];
        P.off.push_back(0);
        for (u32 h = 0; h < n_haps; ++h) {
            const u32 H = (u32)(rs[g].hap_off[h + 1] - rs[g].hap_off[h]), kind = h ? rnd() % 3 : 0, a = between(1, H / 3), b = between(1, H / 3),
                      l1 = between(1, 5), l2 = between(1, 5);
            if (kind == 0) P.el.push_back(H << 4);
            else if (kind == 1 && (rnd() & 1)) { P.el.push_back(a << 4); P.el.push_back(l1 << 4 | 1); P.el.push_back((H - a - l1) << 4); }
            else if (kind == 1) { P.el.push_back(a << 4); P.el.push_back(l1 << 4 | 2); P.el.push_back((H - a) << 4); }
            else { P.el.push_back(a << 4); P.el.push_back(l1 << 4 | 2); P.el.push_back(b << 4); P.el.push_back(l2 << 4 | 1); P.el.push_back((H - a - b - l2) << 4); }
            P.off.push_back(P.el.size()); P.hap_start.push_back((int32_t)(rnd() % 4));
        }
        tr[g] = mgx_to_ref_region_t{P.off.data(), P.el.data(), P.hap_start.data(), 0, (int32_t)(1000 * g), nullptr};
    }
    ToRefOutputs TA, TB;
    TA.shape(n_regions, n_reads, row_stride); TB.shape(n_regions, n_reads, row_stride);
    double host_pass = 0;
    auto composed = [&]() {
        const double t0 = now_ms();
        CHECK(mgx_realign_regions(hmm, sw, n_regions, regions.data(), mapq.data(), &model, pri.data(), &params, MGX_SW_SOFTCLIP, A.p_log10.data(),
                                  A.p_keep.data(), A.p_best.data(), A.p_offset.data(), A.p_cigar.data(), stride, A.p_score.data()));
        const double t1 = now_ms();
        std::vector<u32> el;
        for (u32 g = 0; g < n_regions; ++g) {
            const Region& Rg = rs[g];
            const ToRefPart& P = parts[g];
            for (u32 r = 0; r < n_reads; ++r) {
                if (!A.keep[g][r]) { TA.status[g][r] = MGX_TO_REF_DROPPED; TA.start[g][r] = 0; TA.n[g][r] = 0; continue; }
                el.clear();
                u32 len = 0;
                for (const char* t = A.cigar[g].data() + (size_t)r * stride; *t; ++t) {
                    if (*t >= '0' && *t <= '9') { len = len * 10 + (u32)(*t - '0'); continue; }
                    el.push_back(len << 4 | (*t == 'M' ? 0u : *t == 'I' ? 1u : *t == 'D' ? 2u : *t == 'S' ? 4u : 9u));
                    len = 0;
                }
                const u32 h = (u32)A.best[g][r];
                const R::Input in{el.data(), (u32)el.size(), A.offset[g][r], P.el.data() + P.off[h], (u32)(P.off[h + 1] - P.off[h]), P.hap_start[h],
                                  Rg.haps.data() + Rg.hap_off[0], (u32)(Rg.hap_off[1] - Rg.hap_off[0]), Rg.bases.data() + Rg.read_off[r],
                                  (u32)(Rg.read_off[r + 1] - Rg.read_off[r]), tr[g].reference_start, 0, 0};
                const R::Result res = R::read_to_ref(in, row_stride, RowStore{TA.rows[g].data() + (size_t)r * row_stride, row_stride}, R::SerialAny{});
                TA.status[g][r] = res.status; TA.start[g][r] = res.status == R::kOk ? res.start : 0;
                TA.n[g][r] = (res.status == R::kOk || res.status == R::kNoRoom) ? res.n : 0;
            }
        }
        const double t2 = now_ms();
        host_pass = t2 - t1;
        return t2 - t0;
    };
    auto fused = [&](mgx_pairhmm_t* ctx) {
        const double t0 = now_ms();
        CHECK(mgx_realign_regions_to_ref(ctx, sw, n_regions, regions.data(), mapq.data(), &model, pri.data(), &params, MGX_SW_SOFTCLIP,
                                         B.p_log10.data(), B.p_keep.data(), B.p_best.data(), B.p_offset.data(), B.p_cigar.data(), stride,
                                         B.p_score.data(), tr.data(), TB.p_start.data(), TB.p_rows.data(), row_stride, TB.p_n.data(), TB.p_status.data()));
        return now_ms() - t0;
    };
    composed(); fused(hmm);
    for (u32 g = 0; g < n_regions; ++g) {
        bool same = A.log10[g] == B.log10[g] && A.keep[g] == B.keep[g] && A.best[g] == B.best[g] && A.offset[g] == B.offset[g] && A.score[g] == B.score[g] &&
                    TA.status[g] == TB.status[g] && TA.start[g] == TB.start[g] && TA.n[g] == TB.n[g];
        for (u32 r = 0; same && r < n_reads; ++r) {
            same = strcmp(A.cigar[g].data() + (size_t)r * stride, B.cigar[g].data() + (size_t)r * stride) == 0;
            if (same && TA.status[g][r] == MGX_TO_REF_OK)
                same = memcmp(TA.rows[g].data() + (size_t)r * row_stride, TB.rows[g].data() + (size_t)r * row_stride, TA.n[g][r] * 4) == 0;
        }
        if (!same) { fprintf(stderr, "region %u: the fused call and the composition differ\n", g); return 3; }
    }
    mgx_realign_stats_t st; mgx_realign_to_ref_stats_t ts;
    CHECK(mgx_realign_stats(hmm, &st)); CHECK(mgx_realign_to_ref_stats(hmm, &ts));
    u64 with_indel = 0;
    for (u32 g = 0; g < n_regions; ++g) for (u32 r = 0; r < n_reads; ++r) {
        bool any = false;
        for (u32 k = 0; TB.status[g][r] == MGX_TO_REF_OK && k < TB.n[g][r]; ++k) any |= (TB.rows[g][(size_t)r * row_stride + k] & 15) != 0;
        with_indel += any;
    }
    printf("reads %llu kept %llu verbatim %llu aligned %llu; results identical\n", (unsigned long long)st.n_reads, (unsigned long long)st.n_kept,
           (unsigned long long)st.n_verbatim, (unsigned long long)st.n_sw_pairs);
    printf("to-reference statuses: ok %llu dropped %llu unchanged %llu throws %llu undefined %llu no_room %llu; %llu results hold an indel\n",
           (unsigned long long)ts.n_status[0], (unsigned long long)ts.n_status[1], (unsigned long long)ts.n_status[2], (unsigned long long)ts.n_status[3],
           (unsigned long long)ts.n_status[4], (unsigned long long)ts.n_status[5], (unsigned long long)with_indel);
    std::vector<double> ta, tb, th;
    for (u32 k = 0; k < rounds; ++k) {
        ta.push_back(composed()); th.push_back(host_pass); tb.push_back(fused(hmm));
        printf("round %u composed %.3f ms (host pass %.3f) fused %.3f ms\n", k, ta.back(), th.back(), tb.back());
    }
    auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]); };
    auto spread = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
    printf("composed median %.3f ms spread %.3f ms (its host pass: median %.3f ms)\n", median(ta), spread(ta), median(th));
    printf("fused    median %.3f ms spread %.3f ms\n", median(tb), spread(tb));
    fused(hmm_timed); fused(hmm_timed);
    CHECK(mgx_realign_to_ref_stats(hmm_timed, &ts));
    printf("fused kernel (HIP events, ms): read_to_ref %.3f\n", ts.ms_to_ref);
    const double diff = median(ta) - median(tb);
    printf("difference composed - fused %.3f ms = %.2f x the yardstick's spread (counts beyond 3 x)\n", diff, spread(ta) > 0 ? diff / spread(ta) : 0.0);
    return 0;
}

int main(int argc, char** argv) {
    const bool to_ref = argc == 11 && strcmp(argv[10], "to_ref") == 0;
    if (argc != 10 && !to_ref) { fprintf(stderr, "usage: %s n_regions n_reads n_haps read_min read_max hap_min hap_max verbatim_percent rounds [to_ref]\n", argv[0]); return 1; }
    const u32 n_regions = atoi(argv[1]), n_reads = atoi(argv[2]), n_haps = atoi(argv[3]), rmin = atoi(argv[4]), rmax = atoi(argv[5]),
              hmin = atoi(argv[6]), hmax = atoi(argv[7]), verbatim_percent = atoi(argv[8]), rounds = atoi(argv[9]);
    const char acgt[] = "ACGT";
    // ---- the workload: haplotypes are copies of one backbone per region with 2 % substitutions; a read is cut out of one of them,
    // verbatim with the given probability, else with one substituted base
    std::vector<Region> rs(n_regions);
    u32 longest = 1;
    for (Region& R : rs) {
        std::vector<u8> backbone(hmax);
        for (u8& b : backbone) b = acgt[rnd() & 3];
        R.hap_off.push_back(0);
        for (u32 h = 0; h < n_haps; ++h) {
            const u32 H = between(hmin, hmax);
            for (u32 x = 0; x < H; ++x) R.haps.push_back(rnd() % 50 == 0 ? (u8)acgt[rnd() & 3] : backbone[x]);
            R.hap_off.push_back(R.haps.size()); R.pri.push_back((double)(rnd() % 3));
            longest = std::max(longest, H);
        }
        R.read_off.push_back(0);
        for (u32 r = 0; r < n_reads; ++r) {
            const u32 h = rnd() % n_haps, H = (u32)(R.hap_off[h + 1] - R.hap_off[h]), len = std::min(between(rmin, rmax), H);
            const u32 at = rnd() % (H - len + 1);
            const size_t first = R.bases.size();
            R.bases.insert(R.bases.end(), R.haps.begin() + R.hap_off[h] + at, R.haps.begin() + R.hap_off[h] + at + len);
            if (rnd() % 100 >= verbatim_percent) { u8& b = R.bases[first + rnd() % len]; b = b == 'A' ? 'C' : 'A'; }
            R.read_off.push_back(R.bases.size());
            longest = std::max(longest, len);
        }
        const size_t nb = R.bases.size();
        R.qual.assign(nb, 30); R.ins.assign(nb, 45); R.del.assign(nb, 45); R.gcp.assign(nb, 10); R.mapq.assign(n_reads, 60);
        R.in = mgx_pairhmm_input_t{n_reads, R.read_off.data(), R.bases.data(), R.qual.data(), R.ins.data(), R.del.data(), R.gcp.data(),
                                   n_haps, R.hap_off.data(), R.haps.data(), 0, nullptr, nullptr};
    }
    std::vector<mgx_pairhmm_input_t> regions; std::vector<const u8*> mapq; std::vector<const double*> pri;
    for (Region& R : rs) { regions.push_back(R.in); mapq.push_back(R.mapq.data()); pri.push_back(R.pri.data()); }
    const u32 stride = 2 * longest + 1;
    const mgx_sw_params_t params{10, -15, -30, -5};
    mgx_read_model_t model; mgx_read_model_defaults(&model);
    mgx_pairhmm_t* hmm = nullptr; mgx_pairhmm_t* hmm_timed = nullptr; mgx_sw_t* sw = nullptr;
    CHECK(mgx_pairhmm_create(0, 0, &hmm)); CHECK(mgx_pairhmm_create(0, MGX_PAIRHMM_TIMING, &hmm_timed)); CHECK(mgx_sw_create(0, 0, &sw));
    Outputs A, B;
    A.shape(rs, stride); B.shape(rs, stride);
    if (to_ref) {
        printf("workload %u regions of %u x %u, reads %u-%u, haplotypes %u-%u, verbatim asked %u %%\n", n_regions, n_reads, n_haps, rmin, rmax, hmin, hmax, verbatim_percent);
        const int rc = to_ref_ab(rs, regions, mapq, pri, model, params, hmm, hmm_timed, sw, stride, rounds, A, B);
        mgx_sw_destroy(sw); mgx_pairhmm_destroy(hmm); mgx_pairhmm_destroy(hmm_timed);
        return rc;
    }

    double stage[4] = {0, 0, 0, 0};      // of the last composed call: pairhmm_regions | best + lastIndexOf | assembly | sw_align_batch + scatter
    u64 n_sw = 0;
    auto composed = [&]() {
        const double t0 = now_ms();
        CHECK(mgx_pairhmm_regions(hmm, n_regions, regions.data(), mapq.data(), &model, A.p_log10.data(), A.p_keep.data()));
        const double t1 = now_ms();
        std::vector<std::pair<u32, u32>> where;
        for (u32 g = 0; g < n_regions; ++g) {
            const Region& R = rs[g];
            for (u32 r = 0; r < n_reads; ++r) {
                const int b = search_best_allele(A.log10[g].data() + (size_t)r * n_haps, n_haps, R.pri.data());
                A.best[g][r] = b;
                char* text = A.cigar[g].data() + (size_t)r * stride;
                if (!A.keep[g][r]) { A.offset[g][r] = MGX_REALIGN_NOT_ALIGNED; text[0] = 0; A.score[g][r] = 0; continue; }
                const u64 len = R.read_off[r + 1] - R.read_off[r];
                const int at = last_index_of(R.haps.data() + R.hap_off[b], R.hap_off[b + 1] - R.hap_off[b], R.bases.data() + R.read_off[r], len);
                if (at >= 0) { A.offset[g][r] = at; snprintf(text, stride, "%lluM", (unsigned long long)len); A.score[g][r] = (int32_t)len * params.match; }
                else where.push_back({g, r});
            }
        }
        const double t2 = now_ms();
        n_sw = where.size();
        std::vector<u64> ref_off(n_sw + 1, 0), alt_off(n_sw + 1, 0);
        std::vector<u8> ref, alt, strategy(n_sw, MGX_SW_SOFTCLIP);
        for (u64 q = 0; q < n_sw; ++q) {
            const Region& R = rs[where[q].first];
            const u32 r = where[q].second, b = (u32)A.best[where[q].first][r];
            ref.insert(ref.end(), R.haps.begin() + R.hap_off[b], R.haps.begin() + R.hap_off[b + 1]);
            alt.insert(alt.end(), R.bases.begin() + R.read_off[r], R.bases.begin() + R.read_off[r + 1]);
            ref_off[q + 1] = ref.size(); alt_off[q + 1] = alt.size();
        }
        const double t3 = now_ms();
        std::vector<int32_t> off(n_sw), sc(n_sw); std::vector<char> cig(n_sw * stride);
        const mgx_sw_input_t in{n_sw, ref_off.data(), ref.data(), alt_off.data(), alt.data(), strategy.data()};
        CHECK(mgx_sw_align_batch(sw, &params, &in, off.data(), cig.data(), stride, sc.data()));
        for (u64 q = 0; q < n_sw; ++q) {
            const u32 g = where[q].first, r = where[q].second;
            A.offset[g][r] = off[q]; A.score[g][r] = sc[q]; memcpy(A.cigar[g].data() + (size_t)r * stride, cig.data() + q * stride, stride);
        }
        const double t4 = now_ms();
        stage[0] = t1 - t0; stage[1] = t2 - t1; stage[2] = t3 - t2; stage[3] = t4 - t3;
        return t4 - t0;
    };
    auto fused = [&](mgx_pairhmm_t* ctx) {
        const double t0 = now_ms();
        CHECK(mgx_realign_regions(ctx, sw, n_regions, regions.data(), mapq.data(), &model, pri.data(), &params, MGX_SW_SOFTCLIP, B.p_log10.data(),
                                  B.p_keep.data(), B.p_best.data(), B.p_offset.data(), B.p_cigar.data(), stride, B.p_score.data()));
        return now_ms() - t0;
    };
    // ---- warm-up, and the results compared
    composed(); fused(hmm);
    for (u32 g = 0; g < n_regions; ++g) {
        bool same = A.log10[g] == B.log10[g] && A.keep[g] == B.keep[g] && A.best[g] == B.best[g] && A.offset[g] == B.offset[g] && A.score[g] == B.score[g];
        for (u32 r = 0; same && r < n_reads; ++r) same = strcmp(A.cigar[g].data() + (size_t)r * stride, B.cigar[g].data() + (size_t)r * stride) == 0;
        if (!same) { fprintf(stderr, "region %u: the fused call and the composition differ\n", g); return 3; }
    }
    mgx_realign_stats_t st;
    CHECK(mgx_realign_stats(hmm, &st));
    printf("workload %u regions of %u x %u, reads %u-%u, haplotypes %u-%u, verbatim asked %u %%\n", n_regions, n_reads, n_haps, rmin, rmax, hmin, hmax, verbatim_percent);
    printf("reads %llu kept %llu verbatim %llu (%.1f %% of kept) aligned %llu; results identical\n", (unsigned long long)st.n_reads, (unsigned long long)st.n_kept,
           (unsigned long long)st.n_verbatim, st.n_kept ? 100.0 * st.n_verbatim / st.n_kept : 0.0, (unsigned long long)st.n_sw_pairs);
    std::vector<double> ta, tb; std::vector<std::vector<double>> stages(4);
    for (u32 k = 0; k < rounds; ++k) {
        ta.push_back(composed()); tb.push_back(fused(hmm));
        for (int s = 0; s < 4; ++s) stages[s].push_back(stage[s]);
        printf("round %u composed %.3f ms fused %.3f ms\n", k, ta.back(), tb.back());
    }
    auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]); };
    auto spread = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
    printf("composed median %.3f ms spread %.3f ms\n", median(ta), spread(ta));
    printf("fused    median %.3f ms spread %.3f ms\n", median(tb), spread(tb));
    printf("composed stages (medians, ms): pairhmm_regions %.3f  best+lastIndexOf %.3f  assembly %.3f  sw_align_batch+scatter %.3f\n",
           median(stages[0]), median(stages[1]), median(stages[2]), median(stages[3]));
    fused(hmm_timed); fused(hmm_timed);      // the stage times of the fused call's own kernels, from a context that records events
    CHECK(mgx_realign_stats(hmm_timed, &st));
    printf("fused kernels (HIP events, ms): best_allele_rows %.3f  verbatim %.3f  gather %.3f\n", st.ms_best, st.ms_verbatim, st.ms_gather);
    const double diff = median(ta) - median(tb);
    printf("difference composed - fused %.3f ms = %.2f x the yardstick's spread (counts beyond 3 x)\n", diff, spread(ta) > 0 ? diff / spread(ta) : 0.0);
    mgx_sw_destroy(sw); mgx_pairhmm_destroy(hmm); mgx_pairhmm_destroy(hmm_timed);
    return 0;
}
