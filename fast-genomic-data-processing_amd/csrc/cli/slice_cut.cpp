// slice_cut.cpp -- see slice_cut.h
#include "slice_cut.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace slicecut {

bool StreamSource::next(TextChunk* out) {
    if (eof_) return false;
    std::shared_ptr<char> buf(new char[piece_], std::default_delete<char[]>());
    size_t got = std::min(head_.size(), piece_);
    memcpy(buf.get(), head_.data(), got);
    head_.erase(0, got);
    while (got < piece_) {
        const size_t g = fread(buf.get() + got, 1, piece_ - got, f_);
        if (g == 0) { eof_ = true; break; }
        got += g;
    }
    if (got == 0) return false;
    out->data = buf.get(); out->size = got; out->hold = buf;
    return true;
}

const char* line_qname_end(const char* line, const char* end) {
    const char* t = (const char*)memchr(line, '\t', (size_t)(end - line));
    return t ? t : end;
}

size_t last_group_start(const char* data, size_t size) {
    if (size == 0) return 0;
    size_t line_end = size;                                  // one past the '\n' of the line under inspection
    auto line_begin = [&](size_t e) { size_t b = e - 1; while (b > 0 && data[b - 1] != '\n') --b; return b; };
    size_t b = line_begin(line_end);
    const char* qn = data + b; const size_t qn_len = (size_t)(line_qname_end(qn, data + line_end) - qn);
    size_t group = b;
    while (group > 0) {
        const size_t pb = line_begin(group);
        const char* pq = data + pb; const size_t pl = (size_t)(line_qname_end(pq, data + group) - pq);
        if (pl != qn_len || memcmp(pq, qn, qn_len) != 0) break;
        group = pb;
    }
    return group;
}

bool scan_piece_header(PieceSource& src, PieceHead* head) {
    std::string& text = head->text;
    for (;;) {
        TextChunk t;
        if (!src.next(&t)) return src.err().empty();
        size_t p = 0;
        if (!text.empty() && text.back() != '\n') {         // a header line that goes on in this piece
            const char* nl = (const char*)memchr(t.data, '\n', t.size);
            if (!nl) { text.append(t.data, t.size); continue; }
            p = (size_t)(nl - t.data) + 1;
            text.append(t.data, p);
        }
        while (p < t.size && t.data[p] == '@') {
            const char* nl = (const char*)memchr(t.data + p, '\n', t.size - p);
            const size_t e = nl ? (size_t)(nl - t.data) + 1 : t.size;
            text.append(t.data + p, e - p);
            p = e;
        }
        if (p < t.size) { head->first = std::move(t); head->first_off = p; head->have = true; return true; }
    }
}

bool cut_file_ranges(const ReadAt& read, uint64_t pos, uint64_t size, size_t slice_bytes, const Push& push) {
    size_t window = slice_bytes;                             // grows only while one queryname group fills the whole window
    std::vector<char> tail;
    size_t tail_want = 64u << 10;                            // how much text before a tentative cut is inspected
    while (pos < size) {
        const size_t limit = (size_t)std::min<uint64_t>(size - pos, window);
        size_t cut;
        if (limit == size - pos) cut = limit;
        else {
            // the last complete line before pos + limit, and where its queryname group starts
            const size_t tw = std::min(limit, tail_want);
            const uint64_t a0 = pos + limit - tw;
            tail.resize(tw);
            if (!read(tail.data(), tw, a0)) return false;
            const char* last_nl = (const char*)memrchr(tail.data(), '\n', tw);
            size_t first = 0;                                // first byte of the first COMPLETE line in the tail
            if (a0 > pos) { const char* nl0 = (const char*)memchr(tail.data(), '\n', tw); first = nl0 ? (size_t)(nl0 - tail.data()) + 1 : tw; }
            size_t g = 0;
            const bool have = last_nl && (size_t)(last_nl - tail.data()) + 1 > first;
            if (have) g = first + last_group_start(tail.data() + first, (size_t)(last_nl - tail.data()) + 1 - first);
            if (!have || g == first) {
                // the group reaches the head of what was inspected: look further back, or (the whole window is one
                // group) further ahead
                if (a0 > pos) { tail_want *= 4; continue; }
                if (!have || g == 0) { window *= 2; tail_want = 64u << 10; continue; }
            }
            cut = (size_t)(a0 - pos) + g;
            if (cut == 0) { window *= 2; continue; }
        }
        window = slice_bytes; tail_want = 64u << 10;
        Slice sl;
        sl.from_file = true; sl.file_off = pos; sl.file_len = cut;
        pos += cut;
        if (!push(std::move(sl))) break;
    }
    return true;
}

bool cut_pieces(PieceSource& src, PieceHead head, std::string carry, size_t slice_bytes, const Push& push, const Stopped& stopped) {
    const size_t window = slice_bytes;
    auto in_place = [&](const TextChunk& t, size_t at, size_t n) { Slice sl; sl.ext = t.data + at; sl.ext_len = n; sl.hold = t.hold; return push(std::move(sl)); };
    auto owned = [&](std::string& text) { Slice sl; sl.text.swap(text); text.clear(); return push(std::move(sl)); };
    TextChunk t = std::move(head.first);
    size_t pos = head.first_off;
    bool ok = true;
    for (bool have = head.have; have && ok && !stopped(); t = TextChunk(), pos = 0, have = ok && !stopped() && src.next(&t)) {
        const char* d = t.data;
        const size_t n = t.size;
        if (!carry.empty() && pos < n) {
            // the carried group goes on into this piece up to the first line of another queryname
            size_t p = pos;
            if (carry.back() != '\n') {
                const size_t lb = carry.rfind('\n');               // the carried partial line starts after it
                const char* nl = (const char*)memchr(d + p, '\n', n - p);
                p = nl ? (size_t)(nl - d) + 1 : n;
                carry.append(d + pos, p - pos);
                pos = p;
                // The line is complete now.  Where it starts another group and half a window or more is carried before it,
                // what is carried goes out first.  (Not in the loop this one was moved from: there, pieces shorter than a
                // line carried group after group into one slice without bound, which the host test found.  Pieces are 16 MB
                // and more in the tool; the rule changes a cut only where a carried group is half a window long, that is,
                // with -s below twice the bytes of a queryname group.)
                if (nl && lb != std::string::npos && lb + 1 >= window / 2) {
                    const char* x = carry.data() + lb + 1;
                    const size_t pb = lb ? carry.rfind('\n', lb - 1) : std::string::npos;
                    const char* q = carry.data() + (pb == std::string::npos ? 0 : pb + 1);
                    const size_t xl = (size_t)(line_qname_end(x, carry.data() + carry.size()) - x), ql = (size_t)(line_qname_end(q, x) - q);
                    if (xl != ql || memcmp(x, q, xl)) {
                        std::string line(carry, lb + 1);
                        carry.resize(lb + 1);
                        ok = owned(carry);
                        carry.swap(line);
                    }
                }
            }
            if (ok && carry.back() == '\n') {
                const size_t lb = carry.size() >= 2 ? carry.rfind('\n', carry.size() - 2) : std::string::npos;
                const char* l0 = carry.data() + (lb == std::string::npos ? 0 : lb + 1);
                const std::string qn(l0, line_qname_end(l0, carry.data() + carry.size()));
                bool ended = false;
                while (p < n) {
                    const char* nl = (const char*)memchr(d + p, '\n', n - p);
                    const char* le = nl ? nl : d + n;
                    const char* qe = line_qname_end(d + p, le);
                    if (!nl && qe == le) break;                  // a partial line whose queryname is not complete yet
                    if ((size_t)(qe - (d + p)) != qn.size() || memcmp(d + p, qn.data(), qn.size())) { ended = true; break; }
                    if (!nl) break;
                    p = (size_t)(nl - d) + 1;
                }
                carry.append(d + pos, p - pos);
                pos = p;
                if (ended) ok = owned(carry);
                else if (pos < n) { carry.append(d + pos, n - pos); pos = n; }
            }
        }
        while (ok && pos < n && carry.empty()) {
            const size_t rest = n - pos;
            if (rest > window) {
                size_t lim = window, cut = 0;
                for (;;) {
                    const char* nl = (const char*)memrchr(d + pos, '\n', lim);
                    cut = nl ? last_group_start(d + pos, (size_t)(nl - (d + pos)) + 1) : 0;
                    if (cut || lim == rest) break;
                    lim = std::min(rest, lim * 2);
                }
                if (cut) { ok = in_place(t, pos, cut); pos += cut; continue; }
            }
            // the tail: its complete groups in place; the last group (it may go on in the next piece) is carried
            const char* nl = (const char*)memrchr(d + pos, '\n', rest);
            const size_t g = nl ? last_group_start(d + pos, (size_t)(nl - (d + pos)) + 1) : 0;
            if (g) { ok = in_place(t, pos, g); pos += g; }
            carry.assign(d + pos, n - pos);
            pos = n;
        }
    }
    t = TextChunk();
    if (!src.err().empty()) return false;
    if (ok && !stopped() && !carry.empty()) owned(carry);
    return true;
}

}  // namespace slicecut
