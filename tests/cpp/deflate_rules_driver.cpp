// deflate_rules_driver.cpp -- csrc/deflate_rules.h on the CPU (tests/test_deflate_rules_host.py builds it with -Werror under ASan + UBSan).
// usage: deflate_rules_driver COMMANDS.  One command per line of the file, one or more answer lines each:
//   tables                      every length, distance, symbol, the token grid, the run rule for v = 0 and v = 7
//   limit LIMIT N NSYM sorted[N] depth[NSYM]   limit_lengths, canonical_next_code, reverse_code -> "limit" len[NSYM] | bl_count[16] | code[NSYM]
//   crc PATH                    the file's bytes in 64-byte chunks, combined -> "crc" n value
//   stored N                    emit_stored at payload N + 4, N + 5 -> "stored" a b
//   member PATH                 a stored member around the file's bytes, written to PATH.member
//   bits START v:nb ...         every item through a sink of its own into shared words, as the lanes write -> "bits" end-position words (hex)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "deflate_rules.h"

using namespace mgx_deflate;

static std::vector<u8> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<u8>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct CrcTables {
    std::vector<u32> tab, x2n, tpow, xr;
    CrcTables() : tab(4 * 256), x2n(32), tpow(1024), xr(65) {
        for (u32 i = 0; i < 256; ++i) tab[i] = crc_table0(i);
        for (u32 k = 1; k < 4; ++k) for (u32 i = 0; i < 256; ++i) tab[k * 256 + i] = crc_table_next(tab[(k - 1) * 256 + i], tab.data());
        x2n[0] = kX1;
        for (u32 k = 1; k < 32; ++k) x2n[k] = multmodp(x2n[k - 1], x2n[k - 1]);
        for (u32 j = 0; j < 1024; ++j) tpow[j] = x_pow_512(j, x2n.data());
        for (u32 r = 0; r <= 64; ++r) xr[r] = x_pow_8(r, x2n.data());
    }
    u32 crc(const std::vector<u8>& d) const {            // as the kernel: a register per chunk, then the combination
        const u32 n = (u32)d.size(), nc = crc_chunks(n);
        std::vector<u32> chunk(nc ? nc : 1);
        for (u32 t = 0; t < chunk.size(); ++t) {
            u32 c = crc_chunk_start(t), p = t * kCrcChunk;
            const u32 end = p + kCrcChunk < n ? p + kCrcChunk : n;
            for (; p + 4 <= end; p += 4) c = crc_word(c, (u32)d[p] | (u32)d[p + 1] << 8 | (u32)d[p + 2] << 16 | (u32)d[p + 3] << 24, tab.data());
            for (; p < end; ++p) c = crc_byte(c, d[p], tab.data());
            chunk[t] = c;
        }
        return crc_combine(chunk.data(), n, tpow.data(), xr.data());
    }
};

static void tables() {
    for (u32 l = 3; l <= 258; ++l) { const Code c = length_code(l); printf("L %u %u %u %u\n", l, c.sym, c.eb, c.ev); }
    for (u32 d = 1; d <= 32768; ++d) { const Code c = dist_code(d); printf("D %u %u %u %u\n", d, c.sym, c.eb, c.ev); }
    for (u32 s = 257; s <= 285; ++s) printf("LE %u %u\n", s, length_extra_bits(s));
    for (u32 s = 0; s < 30; ++s) printf("DE %u %u\n", s, dist_extra_bits(s));
    const u32 lens[] = {3, 4, 10, 11, 257, 258}, dists[] = {1, 4, 5, 24576, 24577, 32768};
    for (u32 l : lens) for (u32 d : dists) {
        const u32 t = token_match(l, d);
        printf("T %u %u %u %u %u %u %u %d\n", l, d, t, tok_symbol(t), tok_length_extra(t), tok_dist_symbol(t), tok_dist_extra(t), (int)tok_is_match(t));
    }
    for (u32 b = 0; b < 256; ++b) printf("TL %u %u %d\n", b, tok_symbol(b), (int)tok_is_match(b));
    printf("TN %u\n", kTokNone);
    for (u32 i = 0; i < 19; ++i) printf("O %u %u\n", i, cl_order(i));
    for (u32 v : {0u, 7u}) for (u32 run = 1; run <= 316; ++run) {
        printf("R %u %u %u", v, run, run_symbol_count(v, run));
        run_symbols(v, run, [](u32 sym, u32 extra) { printf(" %u:%u", sym, extra); });
        printf("\n");
    }
}

static void limit(std::istringstream& in) {
    int lim, n, nsym;
    in >> lim >> n >> nsym;
    std::vector<u16> sorted(n);
    std::vector<u8> len(nsym);
    for (auto& s : sorted) { int x; in >> x; s = (u16)x; }
    for (auto& l : len) { int x; in >> x; l = (u8)x; }
    u32 bl_count[16], next_code[16];
    limit_lengths(bl_count, sorted.data(), n, lim, len.data());
    printf("limit");
    for (u8 l : len) printf(" %u", l);
    printf(" |");
    for (u32 c : bl_count) printf(" %u", c);
    canonical_next_code(bl_count, next_code);
    printf(" |");
    for (int s = 0; s < nsym; ++s) {                     // code values as huff_build gives them: the earlier symbols of the same length counted
        u32 c = 0;
        if (len[s]) { c = next_code[len[s]]; for (int j = 0; j < s; ++j) c += len[j] == len[s]; c = reverse_code(c, len[s]); }
        printf(" %u", c);
    }
    printf("\n");
}

static void member(const CrcTables& T, const std::string& path) {
    const std::vector<u8> d = read_file(path);
    const u32 n = (u32)d.size(), payload = kStoredHeader + n;
    std::vector<u8> m(kMemberHeader + payload + kMemberFooter);
    write_stored_header(m.data() + kMemberHeader, n);
    for (u32 i = 0; i < n; ++i) m[kMemberHeader + kStoredHeader + i] = d[i];
    const u32 total = write_member_frame(m.data(), payload, T.crc(d), n);
    std::ofstream(path + ".member", std::ios::binary).write((const char*)m.data(), total);
    printf("member %u %zu\n", total, m.size());
}

static void bits(std::istringstream& in) {
    u32 start;
    in >> start;
    std::vector<std::pair<u32, u32>> items;
    std::string item;
    u32 total = start;
    while (in >> item) { const size_t c = item.find(':'); items.push_back({(u32)std::stoul(item.substr(0, c)), (u32)std::stoul(item.substr(c + 1))}); total += items.back().second; }
    std::vector<u32> words(total / 32 + 2, 0);
    u32 at = start;
    for (size_t i = 0; i < items.size(); ++i) {          // every item by a sink of its own, as the kernel's lanes write
        BitSink<PlainOr> s;
        s.start(words.data(), at);
        s.put(items[i].first, items[i].second);
        at = s.position();
        s.finish();
    }
    printf("bits %u", at);
    for (u32 w : words) printf(" %08x", w);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: deflate_rules_driver COMMANDS\n"); return 2; }
    const CrcTables T;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd, path;
        in >> cmd;
        if (cmd == "tables") tables();
        else if (cmd == "limit") limit(in);
        else if (cmd == "crc") { in >> path; const std::vector<u8> d = read_file(path); printf("crc %zu %u\n", d.size(), T.crc(d)); }
        else if (cmd == "stored") { u32 n; in >> n; printf("stored %d %d\n", (int)emit_stored(n + 4, n), (int)emit_stored(n + 5, n)); }
        else if (cmd == "member") { in >> path; member(T, path); }
        else if (cmd == "bits") bits(in);
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
