// bgzf_scan.cpp -- host-only walk over the BSIZE chain of a BGZF stream (include/mgx_bgzf.h, mgx_bgzf_scan_blocks).
// No device: what the inflate pipeline needs before a batch is submitted (where every block starts, how much it inflates
// to), and the part of the read side that a CPU test can run under AddressSanitizer + UBSan.
#include <cerrno>
#include <cstdint>

#include "../../include/mgx_bgzf.h"
#include "bgzf_inflate_core.h"
#include "mgx_common.h"

extern "C" int mgx_bgzf_scan_blocks(const uint8_t* data, uint64_t n, uint64_t max_blocks, uint64_t* block_offsets, uint32_t* isize,
                                    uint32_t* crc, uint64_t* n_blocks, int* stop) {
    using namespace mgx_inflate;
    if (!block_offsets || !n_blocks || !stop || (n && !data)) { mgx::set_error("NULL argument"); return -EINVAL; }
    uint64_t at = 0, k = 0;
    *stop = MGX_BGZF_SCAN_END;
    while (at < n) {
        if (k == max_blocks) { *stop = MGX_BGZF_SCAN_FULL; break; }
        uint32_t bsize = 0;
        const uint32_t st = parse_header(data + at, n - at, &bsize);
        if (st == kTruncated) {
            // fewer than 18 bytes left: more input, unless what is there already cannot start a BGZF member
            const uint64_t have = n - at;
            const uint8_t magic[3] = {31, 139, 8};
            bool prefix = true;
            for (uint64_t i = 0; i < have && i < 4; ++i) prefix = prefix && (i < 3 ? data[at + i] == magic[i] : (data[at + i] & 4) != 0);
            *stop = prefix ? MGX_BGZF_SCAN_PARTIAL : MGX_BGZF_SCAN_NOT_BGZF;
            break;
        }
        if (st == kBadHeader) { *stop = MGX_BGZF_SCAN_NOT_BGZF; break; }
        if (st != kOk) {
            mgx::set_error("BGZF block %llu at offset %llu: %s", (unsigned long long)k, (unsigned long long)at, status_text(st));
            block_offsets[k] = at; *n_blocks = k;
            return -EILSEQ;
        }
        if (bsize > n - at) { *stop = MGX_BGZF_SCAN_PARTIAL; break; }
        const uint32_t is = rd32(data + at + bsize - 4);
        if (is > kMaxIsize) {
            mgx::set_error("BGZF block %llu at offset %llu: ISIZE %u is above 64 KB", (unsigned long long)k, (unsigned long long)at, is);
            block_offsets[k] = at; *n_blocks = k;
            return -EILSEQ;
        }
        block_offsets[k] = at;
        if (isize) isize[k] = is;
        if (crc) crc[k] = rd32(data + at + bsize - 8);
        ++k;
        at += bsize;
    }
    block_offsets[k] = at;
    *n_blocks = k;
    return 0;
}
