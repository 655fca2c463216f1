// pairhmm_pack_batch.cpp -- mgx_pairhmm_pack_batch, mgx_pairhmm_pack_batch_wire and mgx_pairhmm_wire_expand_host
// (include/mgx_pairhmm.h): the work queue's packer, plain and in the wire form, as host-only entry points.
// No HIP in this translation unit: it is also what tests/test_host_sanitizers.py builds with
// -fsanitize=address,undefined / thread.
#include <cstring>

#include "pairhmm_pack.h"
#include "pairhmm_wire.h"

using mgx::set_error;

namespace {
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
using mgx::validate;
}  // namespace

extern "C" {

// Host-only: test cases [pair_begin, pair_end) of `in` as a self-contained batch laid out in the caller's buffer.
int mgx_pairhmm_pack_batch(const mgx_pairhmm_input_t* in, uint64_t pair_begin, uint64_t pair_end, void* buf, size_t buf_bytes,
                           mgx_pairhmm_input_t* out, size_t* need) {
    int rc = validate(in);
    if (rc) return rc;
    if (!out || !need) { set_error("NULL argument"); return -EINVAL; }
    if (pair_begin > pair_end || pair_end > mgx::pack_n_pairs(in)) { set_error("test-case range outside the stream"); return -EINVAL; }
    mgx::PackPlan plan;
    const uint64_t bad = mgx::pack_plan(in, pair_begin, pair_end, &plan);
    if (bad) { set_error("test case %llu: index out of range", (unsigned long long)(pair_begin + bad - 1)); return -EINVAL; }
    const uint64_t n = pair_end - pair_begin, nr = plan.lread.size(), nh = plan.lhap.size(), rb = plan.roff.back(), hb = plan.hoff.back();
    size_t off = 0;
    const size_t o_roff = off; off = align_up(off + (nr + 1) * 8);
    const size_t o_hoff = off; off = align_up(off + (nh + 1) * 8);
    const size_t o_pr = off;   off = align_up(off + n * 4);
    const size_t o_ph = off;   off = align_up(off + n * 4);
    const size_t o_b = off;    off = align_up(off + rb);
    const size_t o_q = off;    off = align_up(off + rb);
    const size_t o_i = off;    off = align_up(off + rb);
    const size_t o_d = off;    off = align_up(off + rb);
    const size_t o_g = off;    off = align_up(off + rb);
    const size_t o_h = off;    off = align_up(off + hb);
    *need = off;
    if (!buf || buf_bytes < off) { set_error("buffer of %zu bytes needed", off); return -ENOSPC; }
    uint8_t* p = (uint8_t*)buf;
    memcpy(p + o_roff, plan.roff.data(), (nr + 1) * 8); memcpy(p + o_hoff, plan.hoff.data(), (nh + 1) * 8);
    memcpy(p + o_pr, plan.pair_read.data(), n * 4);     memcpy(p + o_ph, plan.pair_hap.data(), n * 4);
    mgx::pack_copy(in, plan, p + o_b, p + o_q, p + o_i, p + o_d, p + o_g, p + o_h);
    mgx_pairhmm_input_t o{};
    o.n_reads = nr; o.read_off = (const uint64_t*)(p + o_roff); o.bases = p + o_b; o.qual = p + o_q; o.ins = p + o_i; o.del = p + o_d; o.gcp = p + o_g;
    o.n_haps = nh; o.hap_off = (const uint64_t*)(p + o_hoff); o.hap_bases = p + o_h;
    o.n_pairs = n; o.pair_read = (const uint32_t*)(p + o_pr); o.pair_hap = (const uint32_t*)(p + o_ph);
    *out = o;
    return 0;
}

// Host-only: the same batch in the wire form (pairhmm_wire.h).
int mgx_pairhmm_pack_batch_wire(const mgx_pairhmm_input_t* in, uint64_t pair_begin, uint64_t pair_end, void* buf, size_t buf_bytes,
                                mgx_pairhmm_wire_t* out, size_t* need) {
    int rc = validate(in);
    if (rc) return rc;
    if (!out || !need) { set_error("NULL argument"); return -EINVAL; }
    *need = 0;
    if (pair_begin > pair_end || pair_end > mgx::pack_n_pairs(in)) { set_error("test-case range outside the stream"); return -EINVAL; }
    mgx::PackPlan plan;
    const uint64_t bad = mgx::pack_plan(in, pair_begin, pair_end, &plan);
    if (bad) { set_error("test case %llu: index out of range", (unsigned long long)(pair_begin + bad - 1)); return -EINVAL; }
    const mgx::wire::Widths w = mgx::wire::scan_widths(in, &plan);
    const mgx::wire::BufferLayout L = mgx::wire::buffer_layout(plan.lread.size(), plan.lhap.size(), pair_end - pair_begin,
                                                               plan.roff.back(), plan.hoff.back(), w);
    *need = L.need;
    if (!buf || buf_bytes < L.need) { set_error("buffer of %zu bytes needed", L.need); return -ENOSPC; }
    if ((uintptr_t)buf & 7u) { set_error("buffer is not 8-byte aligned"); return -EINVAL; }
    mgx::wire::pack_batch(in, plan, w, L, (uint8_t*)buf, out);
    return 0;
}

int mgx_pairhmm_wire_expand_host(const mgx_pairhmm_wire_t* wire, uint8_t* bases, uint8_t* qual, uint8_t* ins, uint8_t* del,
                                 uint8_t* gcp, uint8_t* hap) {
    if (!wire || !wire->read_off || !wire->hap_off) { set_error("NULL argument"); return -EINVAL; }
    const uint64_t rb = wire->read_off[wire->n_reads], hb = wire->hap_off[wire->n_haps];
    if ((rb && (!bases || !qual || !ins || !del || !gcp || !wire->bases4 || !wire->qual || !wire->ins || !wire->del || (wire->w_gcp && !wire->gcp))) ||
        (hb && (!hap || !wire->hap4))) { set_error("NULL argument"); return -EINVAL; }
    const uint8_t ws[3] = {wire->w_qual, wire->w_ins, wire->w_del};
    for (uint8_t w : ws) if (w != 6 && w != 7) { set_error("field width %u is neither 6 nor 7", w); return -EINVAL; }
    if (wire->w_gcp != 0 && wire->w_gcp != 6 && wire->w_gcp != 7) { set_error("gcp width %u is none of 0, 6, 7", wire->w_gcp); return -EINVAL; }
    mgx::wire::expand(wire, bases, qual, ins, del, gcp, hap);
    return 0;
}


}  // extern "C"
