// pairhmm_plan_driver.cpp -- csrc/pairhmm_plan.h on its own, for AddressSanitizer + UBSan (tests/test_pairhmm_plan_host.py).
// Reads the description of a batch as text -- lengths only: the plan never looks at a sequence -- and prints the plan: classes,
// jobs, bins, slab offsets, the cross-product tables, the expansion grid, cuts, and the launches in the order
// mgx_pairhmm_batch_run (mgx_pairhmm.hip) issues them by default.  Every array the header writes is a heap block of exactly the
// documented size, so that one element past an end aborts the run.
//
// Input, one command per line:
//   n_cu N | min_g N | block N | stage 0/1 | model 0/1 | wire QUAL INS DEL GCP GCP_CONST      knobs (defaults 256, 4, 64, 0, 0, no wire)
//   merge_below N                           the folding limit (MGX_PAIRHMM_MERGE_BELOW; default kMergeBelow, 1 folds nothing)
//   reads L...   haps L...                  lengths, appended to the batch's global read / haplotype tables
//   pairs R H R H ...                       test cases (indices), appended
//   region R0 R1 H0 H1                      a region in the cross-product form: the sub-view reads [R0, R1) x haplotypes [H0, H1)
//   classes R...                            print the class of every R
//   merge C0 ... C41                        print the folded counts and the remap
//   plan_pairs | plan_cross                 print the plan of the batch
//   cut LIMIT                               print the cutter's boundaries over the regions
//   chunk TOTAL...                          print the chunk rule's answer
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "pairhmm_plan.h"

using namespace mgx_hmm_plan;

static std::string g_error;
void mgx::set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

template <typename T> static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n]); }      // exactly n elements

struct Knobs {
    int n_cu = 256, min_g = 4;
    uint64_t merge_below = kMergeBelow;
    uint32_t block = 64;
    bool stage = false, model = false, wire = false;
    mgx::wire::Widths ww;
};

struct Batch {
    std::vector<uint64_t> roff{0}, hoff{0};
    std::vector<uint32_t> pr, ph;
    struct Region { uint64_t r0, r1, h0, h1; };
    std::vector<Region> regions;
    std::vector<mgx_pairhmm_input_t> inputs() const {          // sub-views: offset tables that do not start at 0
        std::vector<mgx_pairhmm_input_t> v;
        for (const Region& g : regions) {
            mgx_pairhmm_input_t in{};
            in.n_reads = g.r1 - g.r0; in.read_off = roff.data() + g.r0;
            in.n_haps = g.h1 - g.h0; in.hap_off = hoff.data() + g.h0;
            in.n_pairs = in.n_reads * in.n_haps;
            v.push_back(in);
        }
        return v;
    }
};

static int fail(int rc) { printf("rc %d %s\n", rc, g_error.c_str()); return 0; }

static void print_bins(const std::vector<Bin>& bins) {
    for (size_t k = 0; k < bins.size(); ++k) {
        const Bin& b = bins[k];
        printf("bin %zu %d %d %d %d %d %d %u %u %u %llu %llu %u %u %u %u %u %u %u %u %u\n", k, bin_index(b.G, b.strip ? kStripMarkRPL : b.RPL), b.G, b.RPL, b.Gd,
               b.RPLd, (int)b.strip, b.job_begin, b.job_count, b.max_h, (unsigned long long)b.cells, (unsigned long long)b.alg_bytes, b.block,
               b.lds_stride, b.grid_f32, b.grid_f64, b.grid_f64_all, b.grid_nhap, lds_bytes(b, true, 4), lds_bytes(b, true, kMaxCodes), lds_bytes(b, false));
    }
}

static void print_slab(const SlabLayout& L) {
    const std::pair<const char*, size_t> slots[] = {
        {"rtab", L.rtab}, {"rreg", L.rreg}, {"rpre", L.rpre}, {"gtab", L.gtab}, {"htab", L.htab}, {"jobs", L.jobs},
        {"bases", L.seq[kSeqBases]}, {"qual", L.seq[kSeqQual]}, {"ins", L.seq[kSeqIns]}, {"del", L.seq[kSeqDel]}, {"gcp", L.seq[kSeqGcp]}, {"hap", L.seq[kSeqHap]},
        {"w_bases4", L.wseq[kSeqBases]}, {"w_qual", L.wseq[kSeqQual]}, {"w_ins", L.wseq[kSeqIns]}, {"w_del", L.wseq[kSeqDel]}, {"w_gcp", L.wseq[kSeqGcp]},
        {"w_hap4", L.wseq[kSeqHap]}, {"mapq", L.mapq}, {"rlen", L.rlen}, {"roff", L.roff}, {"rnh", L.rnh}, {"out", L.o_out}, {"used", L.o_used},
        {"keep", L.o_keep}, {"rlist", L.rlist}, {"nlist", L.nlist}, {"rcount", L.rcount}};
    for (const auto& s : slots) printf("slot %s %zu\n", s.first, s.second);
    printf("slab %zu %zu %zu %zu %d %d %d\n", L.total, L.in_bytes, L.result_bytes, L.pin_bytes, (int)L.staged, (int)L.wire, kCounters);
    if (L.wire) {
        uint64_t n[kSeqArrays];
        uint32_t w[kSeqArrays], block_first[kSeqArrays + 1];
        if (const int rc = expand_grid(L, n, w, block_first)) { fail(rc); return; }
        for (int k = 0; k < kSeqArrays; ++k) printf("expand %d %llu %u %u\n", k, (unsigned long long)n[k], w[k], block_first[k]);
        printf("expandgrid %u %u\n", block_first[kSeqArrays], kExpandBlock);
    }
}

// the launches of a default run (no MGX_PAIRHMM_FORCE_DOUBLE, MGX_PAIRHMM_MULTI on), as mgx_pairhmm_batch_run orders them
static void print_run(const std::vector<Bin>& bins, uint64_t n_pairs, int n_cu) {
    std::vector<char> in_multi(bins.size(), 0);
    for (int gset = 0; gset < 2; ++gset) {
        const MultiSet ms = multi_set(bins, gset, n_cu);
        const uint32_t blocks = ms.block_first[ms.members.size()];
        printf("multi %d %u %u", gset, blocks, ms.lds);
        for (size_t k : ms.members) { printf(" %zu", k); in_multi[k] = 1; }
        printf("\nmulti_first %d", gset);
        for (size_t q = 0; q <= ms.members.size(); ++q) printf(" %u", ms.block_first[q]);
        printf("\n");
        if (!ms.members.empty()) printf("launch multi %d 0 4 %u 64 %u\n", gset, blocks, ms.lds);
    }
    const NarrowExtent nw = survey_narrow(bins);
    printf("narrow %zu %u %u %u\n", nw.first, nw.n_jobs, nw.max_h, nw.rows);
    printf("order");
    for (size_t k : class_order(bins)) printf(" %zu", k);
    printf("\n");
    for (size_t k : class_order(bins)) {
        const Bin& b = bins[k];
        if (b.strip) printf("launch strip32 64 16 5 %u %u %u\n", b.grid_f32, b.block, lds_bytes(b, true, kMaxCodes));
        else if (!in_multi[k]) printf("launch f32 %d %d 4 %u %u %u\n", b.G, b.RPL, b.grid_f32, b.block, lds_bytes(b, true, 4));
        if (!b.strip) printf("launch f32 %d %d 5 %u %u %u\n", b.G, b.RPL, b.grid_nhap, b.block, lds_bytes(b, true, kMaxCodes));
        if (is_narrow(b)) continue;
        if (b.strip) printf("launch strip64 64 16 5 %u %u %u\n", b.grid_f64, b.block, lds_bytes(b, false));
        else printf("launch f64 %d %d 5 %u %u %u\n", b.Gd, b.RPLd, b.grid_f64, b.block, lds_bytes(b, false));
    }
    // the last two launches are not the header's: restated from launch_shared_f64 and launch_exact (mgx_pairhmm.hip) on top of
    // the narrow extent and hap_stride, so that the fixed batches' recorded launches are compared whole
    if (nw.n_jobs) printf("launch f64 16 %d 5 %u 64 %u\n", (int)((nw.rows + 15) / 16), std::min<uint32_t>((nw.n_jobs + 3) / 4, (uint32_t)n_cu * 8u), 4u * hap_stride(nw.max_h, 16));
    uint32_t max_h = 0;
    for (const Bin& b : bins) max_h = std::max(max_h, b.max_h);
    const size_t per_wg = 6u * (size_t)((max_h + 63u) & ~63u) * sizeof(double);
    const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)n_pairs, (size_t)n_cu * 2u, (size_t)(256u << 20) / per_wg}));
    printf("launch exact 64 16 5 %u 64 %u\n", grid, hap_stride(max_h, 64));
    printf("exact %u %u %u %zu\n", hap_stride(max_h, 64), (max_h + 63u) & ~63u, grid, per_wg);
}

static int plan_pairs(const Knobs& kn, const Batch& bt) {
    PairView v;
    v.n = bt.pr.size(); v.n_reads = bt.roff.size() - 1; v.n_haps = bt.hoff.size() - 1;
    v.pr = bt.pr.data(); v.ph = bt.ph.data(); v.roff = bt.roff.data(); v.hoff = bt.hoff.data();
    PairClasses pc;
    if (const int rc = classify_pairs(v, kn.min_g, &pc, kn.merge_below)) return fail(rc);
    SlabLayout L;
    L.n = v.n; L.n_reads = v.n_reads; L.n_haps = v.n_haps; L.read_bytes = bt.roff.back(); L.hap_bytes = bt.hoff.back();
    L.wire = kn.wire; L.ww = kn.ww;
    plan_slab(kn.stage, &L);
    auto jobs = block<Job>(v.n);
    std::vector<Bin> bins;
    if (const int rc = sort_pairs(v, pc, kn.n_cu, kn.block, jobs.get(), &bins)) return fail(rc);
    printf("rc 0\n");
    printf("max_h %u\n", pc.max_h);
    for (uint64_t q = 0; q < v.n; ++q)
        printf("job %llu %u %u %u %llu %llu\n", (unsigned long long)q, jobs[q].R, jobs[q].H, jobs[q].pair, (unsigned long long)jobs[q].read_off, (unsigned long long)jobs[q].hap_off);
    print_bins(bins);
    print_slab(L);
    if (v.n) print_run(bins, v.n, kn.n_cu);          // mgx_pairhmm_batch_run launches nothing for an empty batch
    return 0;
}

static int plan_cross(const Knobs& kn, const Batch& bt) {
    const std::vector<mgx_pairhmm_input_t> regs = bt.inputs();
    const uint32_t n_regions = (uint32_t)regs.size();
    CrossPlan p;
    std::vector<uint64_t> out_base;
    if (const int rc = cross_totals(n_regions, regs.data(), &p, &out_base)) return fail(rc);
    uint64_t count[kBins] = {0};
    if (const int rc = cross_tables(n_regions, regs.data(), out_base, kn.min_g, &p, count)) return fail(rc);
    std::vector<Bin> bins;
    if (const int rc = cross_bins(&p, count, kn.n_cu, kn.block, &bins, kn.merge_below)) return fail(rc);
    SlabLayout L;
    L.n = p.n; L.n_reads = p.nr; L.n_haps = p.nh; L.n_regions = n_regions; L.read_bytes = p.read_bytes; L.hap_bytes = p.hap_bytes;
    L.cross = true; L.model = kn.model; L.wire = kn.wire; L.ww = kn.ww;
    plan_slab(true, &L);
    auto rtab = block<SeqRef>(p.nr);
    auto rreg = block<uint32_t>(p.nr), rpre = block<uint32_t>(p.nr + 1);
    cross_write_tables(p, rtab.get(), rreg.get(), rpre.get());
    auto rlen = block<uint64_t>(p.nr);
    auto roff = block<uint32_t>(p.nr), rnh = block<uint32_t>(p.nr);
    cross_write_rows(n_regions, regs.data(), out_base, rlen.get(), roff.get(), rnh.get());
    printf("rc 0\n");
    printf("totals %llu %llu %llu %llu %llu %u\n", (unsigned long long)p.nr, (unsigned long long)p.nh, (unsigned long long)p.n,
           (unsigned long long)p.read_bytes, (unsigned long long)p.hap_bytes, p.max_h);
    for (uint32_t g = 0; g < n_regions; ++g)
        printf("gtab %u %u %u %u %u\n", g, p.regions[g].hap_begin, p.regions[g].n_haps, p.regions[g].read_base, p.regions[g].out_base);
    for (uint64_t h = 0; h < p.nh; ++h) printf("htab %llu %llu %u %u\n", (unsigned long long)h, (unsigned long long)p.haps[h].off, p.haps[h].len, p.haps[h].id);
    for (uint64_t r = 0; r < p.nr; ++r)
        printf("rtab %llu %llu %u %u %u %u\n", (unsigned long long)r, (unsigned long long)rtab[r].off, rtab[r].len, rtab[r].id, rreg[r], rpre[r]);
    printf("rpre_end %u\n", rpre[p.nr]);
    for (uint64_t r = 0; r < p.nr; ++r) printf("row %llu %llu %u %u\n", (unsigned long long)r, (unsigned long long)rlen[r], roff[r], rnh[r]);
    print_bins(bins);
    print_slab(L);
    if (p.n) print_run(bins, p.n, kn.n_cu);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s batch.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Knobs kn;
    Batch bt;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string cmd;
        if (!(ss >> cmd)) continue;
        std::vector<long long> v;
        for (long long x; ss >> x;) v.push_back(x);
        if (cmd == "n_cu") kn.n_cu = (int)v.at(0);
        else if (cmd == "min_g") kn.min_g = (int)v.at(0);
        else if (cmd == "merge_below") kn.merge_below = (uint64_t)v.at(0);
        else if (cmd == "block") kn.block = (uint32_t)v.at(0);
        else if (cmd == "stage") kn.stage = v.at(0) != 0;
        else if (cmd == "model") kn.model = v.at(0) != 0;
        else if (cmd == "wire") {
            kn.wire = true;
            kn.ww.qual = (uint8_t)v.at(0); kn.ww.ins = (uint8_t)v.at(1); kn.ww.del = (uint8_t)v.at(2); kn.ww.gcp = (uint8_t)v.at(3); kn.ww.gcp_const = (uint8_t)v.at(4);
        }
        else if (cmd == "reads") for (long long x : v) bt.roff.push_back(bt.roff.back() + (uint64_t)x);
        else if (cmd == "haps") for (long long x : v) bt.hoff.push_back(bt.hoff.back() + (uint64_t)x);
        else if (cmd == "pairs") for (size_t i = 0; i + 1 < v.size(); i += 2) { bt.pr.push_back((uint32_t)v[i]); bt.ph.push_back((uint32_t)v[i + 1]); }
        else if (cmd == "region") bt.regions.push_back({(uint64_t)v.at(0), (uint64_t)v.at(1), (uint64_t)v.at(2), (uint64_t)v.at(3)});
        else if (cmd == "classes") {
            for (long long R : v) {
                int G, RPL;
                shape_of((uint32_t)R, kn.min_g, &G, &RPL);
                if (!G) { printf("class %lld 0\n", R); continue; }
                Bin b;
                bin_shape(bin_index(G, RPL), &b);
                printf("class %lld %d %d %d %d %d %d %d %d\n", R, G, RPL, bin_index(G, RPL), b.G, b.RPL, b.Gd, b.RPLd, (int)b.strip);
            }
        }
        else if (cmd == "merge") {
            uint64_t count[kBins];
            int remap[kBins];
            for (int k = 0; k < kBins; ++k) count[k] = (uint64_t)v.at((size_t)k);
            merge_small_bins(count, remap, kn.merge_below);
            printf("merged");
            for (int k = 0; k < kBins; ++k) printf(" %llu", (unsigned long long)count[k]);
            printf("\nremap");
            for (int k = 0; k < kBins; ++k) printf(" %d", remap[k]);
            printf("\n");
        }
        else if (cmd == "plan_pairs") plan_pairs(kn, bt);
        else if (cmd == "plan_cross") plan_cross(kn, bt);
        else if (cmd == "cut") {
            const std::vector<mgx_pairhmm_input_t> regs = bt.inputs();
            std::vector<uint32_t> cut;
            cut_regions(regs.data(), (uint32_t)regs.size(), (uint64_t)v.at(0), &cut);
            printf("cut");
            for (uint32_t c : cut) printf(" %u", c);
            printf("\n");
        }
        else if (cmd == "chunk") for (long long t : v) printf("chunk %lld %llu\n", t, (unsigned long long)region_chunk_pairs((uint64_t)t));
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    printf("constants %d %d %d %d %d %llu %zu %zu %d\n", kBins, kExactCount, kSharedCount, kNhapCount, kCounters, (unsigned long long)kMergeBelow, kSlabAlign,
           kStageLimit, kMultiBins);
    return 0;
}
