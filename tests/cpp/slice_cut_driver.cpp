// slice_cut_driver.cpp -- the CLI's slice cutters (csrc/cli/slice_cut.cpp) on generated SAM bodies, CPU only, meant to be run
// under AddressSanitizer + UBSan (tests/test_cli_slices_host.py).  For every run it checks that
//   1. the slices, in seq order, concatenate to exactly the body;
//   2. every slice but possibly the last ends in '\n';
//   3. the queryname of the last line of a slice differs from the queryname of the first line of the next one;
//   4. where every group is shorter than half the window, no slice is longer than the window;
//   5. a slice cut in place can be read after the cutter and the source have dropped the piece (ASan sees a buffer
//      that was released too early);
//   6. the header scan returns the same header and the same first body byte wherever the pieces are split.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "slice_cut.h"

using namespace slicecut;

static long g_runs = 0, g_slices = 0;
static const Stopped kNever = [] { return false; };

#define CHECK(cond, ...)                                                                       \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);                \
            fprintf(stderr, __VA_ARGS__);                                                      \
            fprintf(stderr, "\n");                                                             \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

struct Body { std::string text; size_t max_group = 0; };

// Queryname groups of 1, 2 and 3 lines; neighbouring names are prefixes of each other (r1 / r10 / r1x / r100);
// `long_lines` > 0 puts one group of that many lines into the middle.
static Body make_body(std::mt19937& rng, size_t n_groups, size_t long_lines, bool final_newline) {
    Body b;
    std::vector<std::string> names;
    for (size_t k = 1; names.size() < n_groups; ++k) {
        if (k % 10 == 0) continue;
        const std::string r = "r" + std::to_string(k);
        names.push_back(r); names.push_back(r + "0"); names.push_back(r + "x"); names.push_back(r + "00");
    }
    for (size_t g = 0; g < n_groups; ++g) {
        size_t lines = 1 + rng() % 3;
        if (long_lines && g == n_groups / 2) lines = long_lines;
        const size_t start = b.text.size();
        for (size_t l = 0; l < lines; ++l) {
            b.text += names[g]; b.text += '\t'; b.text += std::to_string(rng() % 4096); b.text += '\t';
            b.text.append(4 + rng() % 40, "ACGT"[rng() % 4]);
            b.text += '\n';
        }
        b.max_group = std::max(b.max_group, b.text.size() - start);
    }
    if (!final_newline) b.text.pop_back();
    return b;
}

// The text in pieces of the given sizes (the last piece takes what is left); every piece lives in a buffer of exactly its
// size that nothing but the TextChunk's hold keeps alive.
class MemSource : public PieceSource {
public:
    MemSource(const std::string& text, std::vector<size_t> sizes) : text_(text), sizes_(std::move(sizes)) {}
    bool next(TextChunk* out) override {
        if (at_ >= text_.size()) return false;
        size_t n = k_ < sizes_.size() ? sizes_[k_++] : text_.size() - at_;
        n = std::max<size_t>(1, std::min(n, text_.size() - at_));
        std::shared_ptr<char> buf(new char[n], std::default_delete<char[]>());
        memcpy(buf.get(), text_.data() + at_, n);
        at_ += n;
        out->data = buf.get(); out->size = n; out->hold = buf;
        return true;
    }
    const std::string& err() const override { return err_; }
    void abort() override {}
private:
    const std::string& text_; std::vector<size_t> sizes_; size_t at_ = 0, k_ = 0; std::string err_;
};

static std::string qname_of(const std::string& s, size_t line) {
    size_t e = s.find('\n', line);
    if (e == std::string::npos) e = s.size();
    const size_t t = s.find('\t', line);
    return s.substr(line, std::min(e, t == std::string::npos ? e : t) - line);
}

// Properties 1-4 on the slices' texts.
static void check_slices(const std::vector<std::string>& parts, const Body& body, size_t window, const char* what) {
    std::string all;
    for (const auto& p : parts) all += p;
    CHECK(all == body.text, "%s: window %zu: the slices hold %zu bytes, the body %zu", what, window, all.size(), body.text.size());
    for (size_t k = 0; k < parts.size(); ++k) {
        CHECK(!parts[k].empty(), "%s: window %zu: slice %zu is empty", what, window, k);
        if (k + 1 < parts.size()) {
            CHECK(parts[k].back() == '\n', "%s: window %zu: slice %zu does not end on a line", what, window, k);
            const size_t last = parts[k].size() >= 2 ? parts[k].rfind('\n', parts[k].size() - 2) : std::string::npos;
            const std::string a = qname_of(parts[k], last == std::string::npos ? 0 : last + 1), b = qname_of(parts[k + 1], 0);
            CHECK(a != b, "%s: window %zu: group %s goes on from slice %zu into the next", what, window, a.c_str(), k);
        }
        if (2 * body.max_group < window) CHECK(parts[k].size() <= window, "%s: window %zu: slice %zu has %zu bytes", what, window, k, parts[k].size());
    }
    ++g_runs; g_slices += (long)parts.size();
}

// The piece cutter on header + body in pieces of the given sizes; the slices are read only after the cutter is done and
// the source is gone.
static void run_pieces(const std::string& header, const Body& body, std::vector<size_t> sizes, size_t window, const char* what) {
    const std::string text = header + body.text;
    std::vector<Slice> got;
    {
        MemSource src(text, std::move(sizes));
        PieceHead head;
        CHECK(scan_piece_header(src, &head), "%s: header scan failed", what);
        CHECK(head.text == header, "%s: window %zu: header of %zu bytes read as %zu bytes", what, window, header.size(), head.text.size());
        CHECK(head.have == !body.text.empty(), "%s: body seen: %d", what, (int)head.have);
        if (head.have) CHECK(head.first.data[head.first_off] == body.text[0], "%s: the body starts with another byte", what);
        uint64_t seq = 0;
        CHECK(cut_pieces(src, std::move(head), std::string(), window, [&](Slice sl) { sl.seq = seq++; got.push_back(std::move(sl)); return true; }, kNever),
              "%s: cutter failed", what);
    }
    std::vector<std::string> parts;
    for (size_t k = 0; k < got.size(); ++k) {
        CHECK(got[k].seq == k && !got[k].from_file, "%s: slice %zu out of order", what, k);
        CHECK(!got[k].ext || got[k].hold, "%s: slice %zu is in place without a hold", what, k);
        parts.push_back(got[k].ext ? std::string(got[k].ext, got[k].ext_len) : got[k].text);
    }
    check_slices(parts, body, window, what);
}

static void run_file(const Body& body, size_t window) {
    const std::string& text = body.text;
    std::vector<std::string> parts;
    uint64_t at = 0;
    const ReadAt read = [&](char* dst, size_t n, uint64_t a) {
        CHECK(a + n <= text.size(), "file cutter reads [%llu, +%zu) of %zu bytes", (unsigned long long)a, n, text.size());
        memcpy(dst, text.data() + a, n);
        return true;
    };
    CHECK(cut_file_ranges(read, 0, text.size(), window, [&](Slice sl) {
              CHECK(sl.from_file && sl.file_off == at && sl.file_off + sl.file_len <= text.size(), "file slice at %llu, expected %llu", (unsigned long long)sl.file_off, (unsigned long long)at);
              parts.push_back(text.substr((size_t)sl.file_off, sl.file_len));
              at += sl.file_len;
              return true;
          }), "file cutter: read error");
    check_slices(parts, body, window, "file ranges");
}

// The plain-stream source: the body through a temporary file, after the two bytes the format check takes.
static void run_stream(const Body& body, size_t piece, size_t window) {
    FILE* f = tmpfile();
    CHECK(f, "tmpfile");
    fwrite(body.text.data(), 1, body.text.size(), f);
    rewind(f);
    std::string first;
    for (int c; first.size() < 2 && (c = fgetc(f)) != EOF;) first.push_back((char)c);
    std::vector<Slice> got;
    {
        StreamSource src(f, first, piece);
        PieceHead head;
        CHECK(scan_piece_header(src, &head) && head.text.empty(), "stream: header");
        CHECK(cut_pieces(src, std::move(head), std::string(), window, [&](Slice sl) { got.push_back(std::move(sl)); return true; }, kNever), "stream: cutter failed");
    }
    fclose(f);
    std::vector<std::string> parts;
    for (const Slice& sl : got) parts.push_back(sl.ext ? std::string(sl.ext, sl.ext_len) : sl.text);
    check_slices(parts, body, window, "stream");
}

int main() {
    std::mt19937 rng(20240611);
    const std::string header = "@HD\tVN:1.6\tSO:queryname\n@SQ\tSN:chr1\tLN:1000\n@PG\tID:x\n";
    const size_t windows[] = {64, 100, 256, 1024, 4096};
    for (int variant = 0; variant < 4; ++variant) {
        // a few KB; variants 1 and 3 hold one group longer than most windows, 2 and 3 end without a newline
        const Body body = make_body(rng, 60, variant % 2 ? 45 : 0, variant < 2);
        for (size_t w : windows) {
            run_file(body, w);
            for (size_t cut = 1; cut < body.text.size(); ++cut) run_pieces("", body, {cut}, w, "two pieces");
            for (int rep = 0; rep < 60; ++rep) {
                std::vector<size_t> small, around;
                for (size_t total = 0; total < body.text.size(); total += small.back()) small.push_back(1 + rng() % 64);
                for (size_t total = 0; total < body.text.size(); total += around.back()) around.push_back(w / 2 + rng() % (w + w / 2));
                run_pieces("", body, small, w, "pieces of 1-64 bytes");
                run_pieces("", body, around, w, "pieces around the window");
                run_stream(body, rep % 2 ? 1 + rng() % 64 : w / 2 + rng() % (w + w / 2), w);
            }
        }
        // the header in front: split at every offset (inside an '@' line, at the seam, in the body) and into small pieces
        for (size_t cut = 1; cut < header.size() + 200; ++cut) run_pieces(header, body, {cut}, 256, "header, two pieces");
        for (int rep = 0; rep < 100; ++rep) {
            std::vector<size_t> small;
            for (size_t total = 0; total < header.size() + body.text.size(); total += small.back()) small.push_back(1 + rng() % 24);
            run_pieces(header, body, small, 256, "header, small pieces");
        }
    }
    // bodies many times the window, and a header that nothing follows
    for (int rep = 0; rep < 20; ++rep) {
        const Body big = make_body(rng, 3000, rep % 4 == 0 ? 200 : 0, rep % 3 != 0);
        for (size_t w : {(size_t)1024, (size_t)3000, (size_t)8192}) {
            run_file(big, w);
            run_pieces("", big, {}, w, "one piece");
            run_pieces(header, big, {(size_t)(1 + rng() % big.text.size())}, w, "two pieces");
            run_stream(big, 16384, w);
        }
    }
    run_pieces(header, Body(), {}, 256, "header only");
    run_pieces(header, Body(), {7, 9}, 256, "header only, pieces");
    printf("%ld runs, %ld slices\nrc 0\n", g_runs, g_slices);
    return 0;
}
