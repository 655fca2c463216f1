// pairhmm_wire_driver.cpp -- csrc/pairhmm_wire.h on its own, for AddressSanitizer + UBSan (tests/test_pairhmm_wire_host.py).
// Every buffer is a heap block of exactly the documented size -- the sources, each packed array (ceil(n / 2), ceil(n / 8) * w),
// the whole batch (`need`), the expander's outputs (the array lengths rounded up to 8) -- so that one byte read or written
// past an end aborts the run.  The packed bytes are compared with a bit-by-bit restatement of the layout, the expanded ones
// with the canonical form of the plain packer's batch.  Prints "rc 0" when every case passed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <vector>

#include "pairhmm_wire.h"

namespace W = mgx::wire;
using Block = std::unique_ptr<uint8_t[]>;

static int g_failed = 0;
#define CHECK(cond, ...)                                                           \
    do {                                                                           \
        if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); ++g_failed; } \
    } while (0)

static Block block(size_t n) { return Block(new uint8_t[n]); }      // exactly n bytes (n == 0: a valid pointer to none)

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

// a stream whose arrays are heap blocks of exactly their lengths
struct Stream {
    std::vector<uint64_t> roff{0}, hoff{0};
    Block bases, qual, ins, del, gcp, hap;
    std::vector<uint32_t> pr, ph;
    uint64_t rb() const { return roff.back(); }
    uint64_t hb() const { return hoff.back(); }
    mgx_pairhmm_input_t input() const {
        mgx_pairhmm_input_t in{};
        in.n_reads = roff.size() - 1; in.read_off = roff.data(); in.bases = bases.get(); in.qual = qual.get(); in.ins = ins.get();
        in.del = del.get(); in.gcp = gcp.get();
        in.n_haps = hoff.size() - 1; in.hap_off = hoff.data(); in.hap_bases = hap.get();
        in.n_pairs = pr.size(); in.pair_read = pr.data(); in.pair_hap = ph.data();
        return in;
    }
};

static Stream make_stream(const std::vector<int>& rlen, const std::vector<int>& hlen, uint64_t seed, unsigned qmax, int gcp_value) {
    Stream s;
    for (int l : rlen) s.roff.push_back(s.roff.back() + (uint64_t)l);
    for (int l : hlen) s.hoff.push_back(s.hoff.back() + (uint64_t)l);
    const uint64_t rb = s.rb(), hb = s.hb();
    s.bases = block(rb); s.qual = block(rb); s.ins = block(rb); s.del = block(rb); s.gcp = block(rb); s.hap = block(hb);
    Rng g{seed};
    for (uint64_t i = 0; i < rb; ++i) {
        s.bases[i] = (uint8_t)"ACGTN"[g.next() % 5]; s.qual[i] = (uint8_t)(g.next() % (qmax + 1)); s.ins[i] = (uint8_t)(g.next() % (qmax + 1));
        s.del[i] = (uint8_t)(g.next() % (qmax + 1)); s.gcp[i] = gcp_value >= 0 ? (uint8_t)gcp_value : (uint8_t)(g.next() % (qmax + 1));
    }
    for (uint64_t i = 0; i < hb; ++i) s.hap[i] = (uint8_t)"ACGTN"[g.next() % 5];
    const size_t nr = rlen.size(), nh = hlen.size();
    for (size_t i = 0; i < std::max(nr, nh); ++i) { s.pr.push_back((uint32_t)(i % nr)); s.ph.push_back((uint32_t)(i % nh)); }
    return s;
}

// the layout, restated bit by bit
static uint8_t code_of(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'T' ? 2 : b == 'G' ? 3 : b == 'N' ? 4 : 0; }
static std::vector<uint8_t> naive_nibbles(const uint8_t* src, uint64_t n) {
    std::vector<uint8_t> out((n + 1) / 2, 0);
    for (uint64_t p = 0; p < n; ++p) out[p / 2] |= (uint8_t)(code_of(src[p]) << (4 * (p % 2)));
    return out;
}
static std::vector<uint8_t> naive_stream(const uint8_t* src, uint64_t n, unsigned w) {
    std::vector<uint8_t> out((n + 7) / 8 * w, 0);
    for (uint64_t p = 0; p < n; ++p)
        for (unsigned k = 0; k < w; ++k)
            if (((src[p] & 127u) >> k) & 1u) { const uint64_t b = p * w + k; out[b / 8] |= (uint8_t)(1u << (b % 8)); }
    return out;
}
static uint8_t fold(uint8_t b) { return (b == 'C' || b == 'T' || b == 'G' || b == 'N') ? b : (uint8_t)'A'; }

struct Expect { int w_qual = -1, w_ins = -1, w_del = -1, w_gcp = -1, gcp_const = -1; };

static void check_equal(const uint8_t* got, const std::vector<uint8_t>& want, const char* name, const char* what) {
    CHECK(want.empty() || memcmp(got, want.data(), want.size()) == 0, "%s: %s differs", name, what);
}

// test cases [lo, hi) of the stream: pack array by array and as a whole batch, compare, expand, compare
static void check_batch(const char* name, const Stream& s, uint64_t lo, uint64_t hi, const Expect& ex = Expect()) {
    const mgx_pairhmm_input_t in = s.input();
    mgx::PackPlan plan;
    CHECK(mgx::pack_plan(&in, lo, hi, &plan) == 0, "%s: plan", name);
    const uint64_t rb = plan.roff.back(), hb = plan.hoff.back();
    // the plain packer's batch: what the wire form must expand to, after mask and fold
    Block pb = block(rb), pq = block(rb), pi = block(rb), pd = block(rb), pg = block(rb), phap = block(hb);
    mgx::pack_copy(&in, plan, pb.get(), pq.get(), pi.get(), pd.get(), pg.get(), phap.get());

    const W::Widths w = W::scan_widths(&in, &plan);
    if (ex.w_qual >= 0) CHECK(w.qual == ex.w_qual, "%s: w_qual %d", name, w.qual);
    if (ex.w_ins >= 0) CHECK(w.ins == ex.w_ins, "%s: w_ins %d", name, w.ins);
    if (ex.w_del >= 0) CHECK(w.del == ex.w_del, "%s: w_del %d", name, w.del);
    if (ex.w_gcp >= 0) CHECK(w.gcp == ex.w_gcp, "%s: w_gcp %d", name, w.gcp);
    if (ex.gcp_const >= 0) CHECK(w.gcp == 0 && w.gcp_const == ex.gcp_const, "%s: gcp_const %d", name, w.gcp_const);
    for (uint64_t p = 0; p < rb; ++p) {          // the widths are the smallest that hold the masked values
        CHECK((pq[p] & 127) < (1 << w.qual) && (pi[p] & 127) < (1 << w.ins) && (pd[p] & 127) < (1 << w.del), "%s: width too small", name);
        if (w.gcp) CHECK((pg[p] & 127) < (1 << w.gcp), "%s: gcp width too small", name);
        else CHECK((pg[p] & 127) == w.gcp_const, "%s: gcp is not constant", name);
    }

    // array by array, every destination a block of exactly its packed length
    Block b4 = block(W::nibble_bytes(rb)), q = block(W::stream_bytes(rb, w.qual)), i = block(W::stream_bytes(rb, w.ins)),
          d = block(W::stream_bytes(rb, w.del)), g = block(W::stream_bytes(rb, w.gcp)), h4 = block(W::nibble_bytes(hb));
    W::pack_arrays(&in, &plan, w, b4.get(), q.get(), i.get(), d.get(), g.get(), h4.get());
    check_equal(b4.get(), naive_nibbles(pb.get(), rb), name, "bases4");
    check_equal(q.get(), naive_stream(pq.get(), rb, w.qual), name, "qual");
    check_equal(i.get(), naive_stream(pi.get(), rb, w.ins), name, "ins");
    check_equal(d.get(), naive_stream(pd.get(), rb, w.del), name, "del");
    if (w.gcp) check_equal(g.get(), naive_stream(pg.get(), rb, w.gcp), name, "gcp");
    check_equal(h4.get(), naive_nibbles(phap.get(), hb), name, "hap4");

    // the whole batch in a block of exactly `need` bytes
    const W::BufferLayout L = W::buffer_layout(plan.lread.size(), plan.lhap.size(), hi - lo, rb, hb, w);
    const size_t groups = (size_t)((rb + 7) / 8);
    CHECK(L.need == 8 * (plan.lread.size() + 1) + 8 * (plan.lhap.size() + 1) + 8 * (hi - lo) + (rb + 1) / 2 +
                        groups * (size_t)(w.qual + w.ins + w.del + w.gcp) + (hb + 1) / 2, "%s: need %zu", name, L.need);
    Block buf = block(L.need);
    mgx_pairhmm_wire_t wire;
    W::pack_batch(&in, plan, w, L, buf.get(), &wire);
    CHECK(wire.hap4 + W::nibble_bytes(hb) == buf.get() + L.need, "%s: the batch does not end where the block ends", name);
    CHECK(memcmp(wire.bases4, b4.get(), W::nibble_bytes(rb)) == 0 && memcmp(wire.qual, q.get(), W::stream_bytes(rb, w.qual)) == 0 &&
          memcmp(wire.ins, i.get(), W::stream_bytes(rb, w.ins)) == 0 && memcmp(wire.del, d.get(), W::stream_bytes(rb, w.del)) == 0 &&
          memcmp(wire.gcp, g.get(), W::stream_bytes(rb, w.gcp)) == 0 && memcmp(wire.hap4, h4.get(), W::nibble_bytes(hb)) == 0,
          "%s: the batch differs from its arrays packed one by one", name);
    CHECK(wire.n_reads == plan.lread.size() && wire.n_haps == plan.lhap.size() && wire.n_pairs == hi - lo, "%s: counts", name);
    CHECK(memcmp(wire.read_off, plan.roff.data(), 8 * plan.roff.size()) == 0 && memcmp(wire.hap_off, plan.hoff.data(), 8 * plan.hoff.size()) == 0,
          "%s: offsets", name);
    CHECK(hi == lo || (memcmp(wire.pair_read, plan.pair_read.data(), 4 * (hi - lo)) == 0 && memcmp(wire.pair_hap, plan.pair_hap.data(), 4 * (hi - lo)) == 0),
          "%s: pair arrays", name);

    // expansion into blocks of the array lengths rounded up to 8; what lies past the length stays untouched
    const uint64_t rb8 = (rb + 7) / 8 * 8, hb8 = (hb + 7) / 8 * 8;
    Block eb = block(rb8), eq = block(rb8), ei = block(rb8), ed = block(rb8), eg = block(rb8), eh = block(hb8);
    for (Block* b : {&eb, &eq, &ei, &ed, &eg}) memset(b->get(), 0xEE, rb8);
    memset(eh.get(), 0xEE, hb8);
    // ... from packed arrays in blocks of exactly their lengths (an over-read aborts)
    mgx_pairhmm_wire_t tight = wire;
    tight.bases4 = b4.get(); tight.qual = q.get(); tight.ins = i.get(); tight.del = d.get(); tight.gcp = g.get(); tight.hap4 = h4.get();
    W::expand(&tight, eb.get(), eq.get(), ei.get(), ed.get(), eg.get(), eh.get());
    bool same = true, untouched = true;
    for (uint64_t p = 0; p < rb; ++p)
        same = same && eb[p] == fold(pb[p]) && eq[p] == (pq[p] & 127) && ei[p] == (pi[p] & 127) && ed[p] == (pd[p] & 127) && eg[p] == (pg[p] & 127);
    for (uint64_t p = 0; p < hb; ++p) same = same && eh[p] == fold(phap[p]);
    for (uint64_t p = rb; p < rb8; ++p) untouched = untouched && eb[p] == 0xEE && eq[p] == 0xEE && ei[p] == 0xEE && ed[p] == 0xEE && eg[p] == 0xEE;
    for (uint64_t p = hb; p < hb8; ++p) untouched = untouched && eh[p] == 0xEE;
    CHECK(same, "%s: expansion is not the canonical form of the packed batch", name);
    CHECK(untouched, "%s: the expander wrote past an array's length", name);
}

static void seams() {
    // reads of 1, 7, 8, 9, 15, 16 and 17 bases in every order: 7-bit qualities, a varying gcp
    const std::vector<int> lens = {1, 7, 8, 9, 15, 16, 17};
    Stream s = make_stream(lens, {1, 3, 5, 2, 9, 33, 7}, 1, 127, -1);
    for (uint64_t p = 0; p < s.rb(); ++p) { s.ins[p] &= 63; s.del[p] &= 63; }
    std::vector<uint32_t> order(7);
    std::iota(order.begin(), order.end(), 0u);
    int n = 0;
    Expect ex; ex.w_qual = 7; ex.w_ins = 6; ex.w_del = 6; ex.w_gcp = 7;
    do {
        s.pr = order; s.ph = order;
        check_batch("seam order", s, 0, 7, ex);
        ++n;
    } while (std::next_permutation(order.begin(), order.end()));
    CHECK(n == 5040, "orders: %d", n);
    // reads of 3 and of 5 bases: with the above, a read starts at every position of a group of eight
    for (int len : {3, 5}) {
        Stream t = make_stream(std::vector<int>(9, len), {4, 9}, 2, 127, -1);
        check_batch("short reads", t, 0, 9);
        Stream u = make_stream(std::vector<int>(9, len), {4, 9}, 3, 63, 10);
        check_batch("short reads, 6 bits", u, 0, 9);
    }
}

static void small_shapes() {
    for (int n : {1, 7, 8, 9}) {         // total read bases of 1, 7, 8 and 9; haplotypes of 1 and of odd length
        for (unsigned qmax : {63u, 127u}) {
            Stream s = make_stream({n}, {1}, 10 + (uint64_t)n, qmax, 10);
            check_batch("one read", s, 0, 1);
            Stream t = make_stream({n}, {3}, 20 + (uint64_t)n, qmax, -1);
            check_batch("one read, odd haplotype", t, 0, 1);
        }
    }
    Stream a = make_stream({3, 4}, {5, 1}, 31, 63, 10);            check_batch("reads 3 4", a, 0, 2); check_batch("second only", a, 1, 2);
    Stream b = make_stream(std::vector<int>(9, 1), {7}, 32, 63, 10); check_batch("one haplotype only", b, 0, 9);
    Stream c = make_stream({13}, {1, 1, 3, 255, 2}, 33, 63, 10);   check_batch("one read only", c, 0, 5);
    Stream d = make_stream({16, 8}, {1, 31, 257}, 34, 127, -1);    check_batch("odd haplotypes", d, 0, 3);
    check_batch("empty range", d, 2, 2);
    // a stream whose test cases share sequences and skip some: the gather is not the identity
    Stream e = make_stream({5, 16, 20, 9, 33, 2}, {12, 7, 40}, 35, 127, -1);
    e.pr = {4, 4, 1, 0, 4, 1, 5}; e.ph = {2, 0, 0, 2, 1, 1, 2};
    check_batch("shared sequences", e, 0, 7); check_batch("shared sequences, middle", e, 2, 6);
}

static void widths() {
    const std::vector<int> rl = {5, 16, 20, 9}, hl = {12, 7};      // 50 read bases: the last partial group holds positions 48 and 49
    Expect six; six.w_qual = six.w_ins = six.w_del = 6; six.w_gcp = 0; six.gcp_const = 10;
    { Stream s = make_stream(rl, hl, 41, 63, 10); check_batch("all 6", s, 0, 4, six); }
    for (int arr = 0; arr < 3; ++arr) {
        auto at = [&](Stream& s) -> uint8_t* { return arr == 0 ? s.qual.get() : arr == 1 ? s.ins.get() : s.del.get(); };
        auto seven = [&] { Expect e = six; (arr == 0 ? e.w_qual : arr == 1 ? e.w_ins : e.w_del) = 7; return e; };
        for (int pos : {0, 49, 48}) { Stream s = make_stream(rl, hl, 42, 63, 10); at(s)[pos] = 64; check_batch("a single 64", s, 0, 4, seven()); }
        { Stream s = make_stream(rl, hl, 43, 63, 10); at(s)[17] = 127; check_batch("a single 127", s, 0, 4, seven()); }
        { Stream s = make_stream(rl, hl, 44, 63, 10); at(s)[23] = 255; check_batch("a single 255", s, 0, 4, seven()); }
        { Stream s = make_stream(rl, hl, 45, 63, 10); for (int p = 0; p < 50; ++p) at(s)[p] |= 128; check_batch("bit 7 set", s, 0, 4, six); }
        { Stream s = make_stream(rl, hl, 46, 63, 10); at(s)[23] = 0; at(s)[0] = 0; at(s)[49] = 0; check_batch("zeros", s, 0, 4, six); }
    }
    { Stream s = make_stream(rl, hl, 47, 63, 10); for (int p = 0; p < 50; p += 3) s.gcp[p] = 138; check_batch("gcp 10 and 138", s, 0, 4, six); }
    { Stream s = make_stream(rl, hl, 48, 63, 10); s.gcp[31] = 11; Expect e = six; e.w_gcp = 6; e.gcp_const = -1; check_batch("gcp: one differs", s, 0, 4, e); }
    { Stream s = make_stream(rl, hl, 49, 63, 10); s.gcp[31] = 64; Expect e = six; e.w_gcp = 7; e.gcp_const = -1; check_batch("gcp: one 64", s, 0, 4, e); }
    { Stream s = make_stream(rl, hl, 50, 63, 10); s.gcp[49] = 0; Expect e = six; e.w_gcp = 6; e.gcp_const = -1; check_batch("gcp: a zero", s, 0, 4, e); }
    { Stream s = make_stream(rl, hl, 51, 63, 0); Expect e = six; e.gcp_const = 0; check_batch("gcp: all zero", s, 0, 4, e); }
}

static void bases() {
    Stream s = make_stream({9, 6, 11, 256}, {13, 4, 256}, 61, 63, 10);
    const char odd[] = "acgtnRYKMSWBDHVU\x00\xff.-*NNAN";
    for (uint64_t p = 0; p < 26; ++p) s.bases[p] = (uint8_t)odd[p % 25];
    for (uint64_t p = 0; p < 17; ++p) s.hap[p] = (uint8_t)odd[24 - p % 25];
    for (int b = 0; b < 256; ++b) { s.bases[26 + b] = (uint8_t)b; s.hap[17 + b] = (uint8_t)(255 - b); }      // every byte value
    check_batch("odd bases", s, 0, 4);
}

static void ragged() {
    Rng g{77};
    std::vector<int> rl, hl;
    for (int k = 0; k < 300; ++k) { rl.push_back(1 + (int)(g.next() % 130)); hl.push_back(1 + (int)(g.next() % 200)); }
    Stream s = make_stream(rl, hl, 78, 63, 10);
    check_batch("ragged", s, 0, 300); check_batch("ragged, a slice", s, 101, 178);
    Stream t = make_stream(rl, hl, 79, 127, -1);
    check_batch("ragged, 7 bits", t, 0, 300);
}

int main() {
    // squeeze8 / spread8 are inverses on every field value at every position
    for (unsigned v = 0; v < 128; ++v)
        for (int k = 0; k < 8; ++k) {
            const uint64_t x = (uint64_t)v << (8 * k) | 0x8080808080808080ull;      // bit 7 is dropped
            CHECK(W::spread8<7>(W::squeeze8<7>(x)) == (uint64_t)v << (8 * k), "7-bit field %u at %d", v, k);
            if (v < 64) CHECK(W::spread8<6>(W::squeeze8<6>(x)) == (uint64_t)v << (8 * k), "6-bit field %u at %d", v, k);
        }
    seams();
    small_shapes();
    widths();
    bases();
    ragged();
    printf("rc %d\n", g_failed);
    return g_failed ? 1 : 0;
}
