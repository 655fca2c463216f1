// gz_source.cpp -- see gz_source.h
#include "gz_source.h"

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "gang.h"
#include "mgx_pairhmm.h"       // mgx_last_error

using slicecut::TextChunk;

GzSource::GzSource(FILE* f, std::string head, std::string name, int device, int threads, bool host, BamMode bam)
    : f_(f), pending_(head.begin(), head.end()), name_(std::move(name)), device_(device), threads_(std::max(1, threads)), host_(host),
      bam_(host && bam != kNotBam ? kBamHost : bam) {
    // compressed / inflated bytes per batch: by default ~2000 blocks of level-6 SAM text, what the kernel needs to fill
    // the device (tools/dev_bgzf_inflate.py: 2.2 GB/s at 512 blocks per batch, 7.9 GB/s from 2048 on)
    if (const char* e = getenv("MGX_CLI_INFLATE_BATCH")) { const long long v = atoll(e); if (v > 0) in_cap_ = std::max<uint64_t>((uint64_t)v, 256u << 10); }
    out_cap_ = 4 * in_cap_;                  // a batch takes fewer blocks when the text inflates more than 4 x
    max_blocks_ = (uint32_t)std::min<uint64_t>(1u << 18, in_cap_ / 26 + 1);
    // records per batch the device index is made for: ordinary reads are 200-400 bytes; a batch with more falls back to the host walk
    max_records_ = out_cap_ / 96 + 4096;
}
GzSource::~GzSource() {
    for (Slot& s : slots_) {
        if (s.bb) mgx_bam_batch_destroy(ctx_, s.bb);
        if (s.b) mgx_bgzf_inflate_batch_destroy(ctx_, s.b);
    }
    if (ctx_) mgx_bgzf_destroy(ctx_);
    if (zinit_) inflateEnd(&zs_);
}

void GzSource::abort() {
    { std::lock_guard<std::mutex> g(mu_); aborted_ = true; }
    cv_.notify_all();
}

uint64_t GzSource::hbm_bytes_to_come() const {
    int made = 0;
    for (const Slot& s : slots_) made += s.b != nullptr;
    // record offsets and keys; per tile of the index 44 bytes and a slot of 4 bytes per 37 bytes (mgx_bam_batch_create)
    uint64_t tile = 16384;
    if (const char* e = getenv("MGX_BAM_TILE")) { const long long v = atoll(e); if (v >= 256 && v <= 32768) tile = (uint64_t)v; }
    const uint64_t bam = bam_ == kBamDevice ? max_records_ * 40 + (out_cap_ / tile + 1) * (44 + (tile / 37 + 1) * 4) : 0;
    return host_ ? 0 : (uint64_t)(kSlots - made) * (in_cap_ + out_cap_ + 2 * ((uint64_t)max_blocks_ + 1) * 8 + (uint64_t)max_blocks_ * 4 + bam);
}

bool GzSource::next(TextChunk* out) {
    if (!next_piece(out)) return false;
    if (first_ && out->size >= 4 && !memcmp(out->data, "BAM\1", 4)) {
        err_ = name_ + " is BAM, not SAM: sortmardup reads SAM text (plain, gzip or BGZF compressed)";
        *out = TextChunk();
        return false;
    }
    first_ = false;
    return true;
}

// Reads and submits batches until kDepth are in flight, as far as slots are free.  False: err_.
bool GzSource::top_up() {
    while ((int)flight_.size() < kDepth && !bgzf_done_ && free_slot() >= 0) if (!fill_and_submit(free_slot())) return false;
    return true;
}

int GzSource::next_batch() {
    for (;;) {
        if (!top_up()) return -1;
        if (!flight_.empty()) break;
        if (bgzf_done_) return -1;
        std::unique_lock<std::mutex> lk(mu_);                // every batch holds text being parsed: wait for one
        cv_.wait(lk, [&] { if (aborted_) return true; for (const Slot& s : slots_) if (!s.busy) return true; return false; });
        if (aborted_) return -2;
    }
    const int k = flight_.front();
    flight_.pop_front();
    Slot& s = slots_[k];
    if (!host_) {
        const auto w0 = std::chrono::steady_clock::now();
        const uint8_t* o; const uint32_t* st;
        if (mgx_bgzf_inflate_batch_wait(ctx_, s.b, &o, &st)) {
            err_ = std::string("compressed input, at about byte ") + std::to_string(s.at) + ": " + mgx_last_error();
            return -1;
        }
        wait_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
        s.out_ptr = (const char*)o;
    } else s.out_ptr = s.host_out.data();
    return k;
}

bool GzSource::next_piece(TextChunk* out) {
    if (!err_.empty()) return false;
    if (!gzip_) {
        const int k = next_batch();
        if (k == -2) return false;
        if (k >= 0) {
            Slot& s = slots_[k];
            out->data = s.out_ptr; out->size = s.n_out;
            out->hold = std::shared_ptr<void>(static_cast<void*>(&s), [this, k](void*) { release(k); });
            return true;
        }
        if (!err_.empty()) return false;
        if (!pending_.empty() && !gzip_tail_) {
            err_ = "compressed input is truncated: it ends inside a BGZF block";
            return false;
        }
        if (!gzip_tail_) {
            if (!eof_block_) fprintf(stderr, "sortmardup: warning: the BGZF input has no EOF block (truncated file?)\n");
            return false;
        }
        gzip_ = true;                                             // plain gzip from here on
    }
    return next_gzip(out);
}

int GzSource::free_slot() {
    std::lock_guard<std::mutex> g(mu_);
    if (aborted_) return -1;
    for (int i = 0; i < kSlots; ++i) if (!slots_[i].busy) return i;
    return -1;
}
void GzSource::release(int k) {
    { std::lock_guard<std::mutex> g(mu_); slots_[k].busy = false; }
    cv_.notify_all();
}
bool GzSource::setup(Slot& s) {
    if (host_) {
        s.host_in.resize(in_cap_); s.host_out.resize(out_cap_);
        s.io = new uint64_t[max_blocks_ + 1]; s.oo = new uint64_t[max_blocks_ + 1];
        host_off_.emplace_back(s.io); host_off_.emplace_back(s.oo);
        s.in = s.host_in.data();
        return true;
    }
    if (!ctx_ && mgx_bgzf_create(device_, 0, &ctx_)) { err_ = std::string("GPU: ") + mgx_last_error(); return false; }
    if (mgx_bgzf_inflate_batch_create(ctx_, in_cap_, out_cap_, max_blocks_, &s.b) || mgx_bgzf_inflate_batch_offsets(s.b, &s.io, &s.oo)) {
        err_ = std::string("GPU: ") + mgx_last_error(); return false;
    }
    s.in = mgx_bgzf_inflate_batch_input(s.b);
    return true;
}
// Reads compressed bytes into slot k (after what the last batch left over), finds its whole blocks and starts them.
bool GzSource::fill_and_submit(int k) {
    Slot& s = slots_[k];
    if (!s.in && !setup(s)) return false;
    uint64_t n = pending_.size();
    if (n) memcpy(s.in, pending_.data(), n);
    pending_.clear();
    while (n < in_cap_ && !file_eof_) {
        const size_t g = fread(s.in + n, 1, in_cap_ - n, f_);
        if (g == 0) { if (ferror(f_)) { err_ = "read error on the input"; return false; } file_eof_ = true; }
        n += g;
    }
    isize_.resize(max_blocks_);
    uint64_t nb = 0; int stop = 0;
    if (mgx_bgzf_scan_blocks(s.in, n, max_blocks_, s.io, isize_.data(), nullptr, &nb, &stop)) { err_ = std::string("compressed input: ") + mgx_last_error(); return false; }
    uint32_t k_used = 0; uint64_t out = 0;
    s.oo[0] = 0;
    while (k_used < nb && out + isize_[k_used] <= out_cap_) { out += isize_[k_used]; s.oo[++k_used] = out; }
    const uint64_t used = s.io[k_used];
    if (k_used) eof_block_ = isize_[k_used - 1] == 0;
    if (stop == MGX_BGZF_SCAN_NOT_BGZF && k_used == nb) {
        gz_rest_.assign(s.in + used, s.in + n);                    // a plain gzip member (or something else) starts here
        gzip_tail_ = true; bgzf_done_ = true;
    } else {
        pending_.assign(s.in + used, s.in + n);                    // an incomplete block, or what did not fit
        if (file_eof_ && k_used == 0) bgzf_done_ = true;           // nothing more will complete it
    }
    if (k_used == 0) return true;
    s.at = in_bytes_;
    in_bytes_ += used; out_bytes_ += out;
    s.n_out = out;
    { std::lock_guard<std::mutex> g(mu_); s.busy = true; }
    if (!host_) {
        if (mgx_bgzf_inflate_batch_submit(ctx_, s.b, k_used)) { err_ = std::string("GPU: ") + mgx_last_error(); return false; }
    } else if (!host_inflate(s, k_used)) return false;
    flight_.push_back(k);
    return true;
}
// MGX_CLI_INFLATE=host: the batch's blocks with zlib, split over threads_ threads
bool GzSource::host_inflate(Slot& s, uint32_t nb) {
    std::vector<std::string> errs(threads_);
    gang::run_gang((size_t)threads_, [&](size_t t) {
        z_stream z{};
        if (inflateInit2(&z, -15) != Z_OK) { errs[t] = "inflateInit2 failed"; return; }
        const auto part = gang::gang_range(nb, t, (size_t)threads_);
        for (size_t i = part.begin; i < part.end; ++i) {
            const uint8_t* blk = s.in + s.io[i];
            const uint64_t bs = s.io[i + 1] - s.io[i], isize = s.oo[i + 1] - s.oo[i];
            uint8_t* dst = reinterpret_cast<uint8_t*>(s.host_out.data()) + s.oo[i];
            inflateReset(&z);
            z.next_in = const_cast<uint8_t*>(blk + 18); z.avail_in = (uInt)(bs - 26);
            z.next_out = dst; z.avail_out = (uInt)isize;
            const int r = inflate(&z, Z_FINISH);
            uint32_t crc_want;
            memcpy(&crc_want, blk + bs - 8, 4);
            if (r != Z_STREAM_END || z.total_out != isize || (uint32_t)crc32(0L, dst, (uInt)isize) != crc_want) {
                errs[t] = "compressed input: BGZF block at offset " + std::to_string(s.at + s.io[i]) + " is corrupt";
                break;
            }
        }
        inflateEnd(&z);
    });
    for (auto& e : errs) if (!e.empty()) { err_ = e; return false; }
    return true;
}
// plain gzip members, one after the other, with zlib on this thread
bool GzSource::next_gzip(TextChunk* out) {
    if (!zinit_) {
        if (inflateInit2(&zs_, 15 + 16) != Z_OK) { err_ = "inflateInit2 failed"; return false; }
        zinit_ = true;
        zin_.swap(gz_rest_);
        in_bytes_ += zin_.size();
        zs_.next_in = zin_.data(); zs_.avail_in = (uInt)zin_.size();
    }
    auto buf = std::make_shared<std::vector<char>>(slicecut::kPieceBytes);
    size_t got = 0;
    while (got < buf->size()) {
        if (zs_.avail_in == 0) {
            if (file_eof_) break;
            zin_.resize(4u << 20);
            const size_t g = fread(zin_.data(), 1, zin_.size(), f_);
            if (g == 0) { if (ferror(f_)) { err_ = "read error on the input"; return false; } file_eof_ = true; break; }
            zs_.next_in = zin_.data(); zs_.avail_in = (uInt)g;
            in_bytes_ += g;
        }
        if (!in_member_) { inflateReset(&zs_); in_member_ = true; }
        zs_.next_out = reinterpret_cast<Bytef*>(buf->data() + got); zs_.avail_out = (uInt)(buf->size() - got);
        const int r = inflate(&zs_, Z_NO_FLUSH);
        got = buf->size() - zs_.avail_out;
        if (r == Z_STREAM_END) in_member_ = false;
        else if (r != Z_OK && r != Z_BUF_ERROR) { err_ = std::string("compressed input: gzip stream is corrupt (") + (zs_.msg ? zs_.msg : "zlib error") + ")"; return false; }
    }
    if (got == 0) {
        if (in_member_) { err_ = "compressed input is truncated: it ends inside a gzip member"; return false; }
        return false;
    }
    out_bytes_ += got;
    out->data = buf->data(); out->size = got; out->hold = buf;
    return true;
}

// ---- BAM (-b) ------------------------------------------------------------------------------------------------------------
bool GzSource::bgzf_ended_well() {
    if (!pending_.empty() && !gzip_tail_) { err_ = "compressed input is truncated: it ends inside a BGZF block"; return false; }
    if (gzip_tail_) { err_ = name_ + " is not BAM: a plain gzip member where -b reads BGZF blocks"; return false; }
    if (!eof_block_) fprintf(stderr, "sortmardup: warning: the BGZF input has no EOF block (truncated file?)\n");
    return true;
}

bool GzSource::read_bam_header(samtext::Header* hdr) {
    std::vector<uint8_t> head;                               // the bytes of the batches before the one the header ends in
    for (;;) {
        const int k = next_batch();
        if (k < 0) {
            if (err_.empty() && bgzf_ended_well()) err_ = name_ + (head.empty() ? " is not BAM: it holds no data" : " is truncated: it ends inside the BAM header");
            return false;
        }
        Slot& s = slots_[k];
        const uint8_t* data = (const uint8_t*)s.out_ptr; uint64_t n = s.n_out;
        if (!head.empty()) { head.insert(head.end(), data, data + n); data = head.data(); n = head.size(); }
        mgx_bam_header_t h;
        int rc = mgx_bam_parse_header(data, n, &h, 0, nullptr, nullptr, nullptr);
        if (rc < 0) { err_ = name_ + ": " + mgx_last_error(); release(k); return false; }
        if (rc == MGX_BAM_PARTIAL) {
            if (head.empty()) head.assign(data, data + n);
            batch_base_ += s.n_out;
            release(k);
            continue;
        }
        std::vector<uint64_t> name_off(h.n_ref); std::vector<uint32_t> name_len(h.n_ref), ref_len(h.n_ref);
        if ((rc = mgx_bam_parse_header(data, n, &h, h.n_ref, name_off.data(), name_len.data(), ref_len.data()))) { err_ = name_ + ": " + mgx_last_error(); release(k); return false; }
        hdr->text.assign((const char*)data + h.text_off, h.text_len);
        for (uint32_t r = 0; r < h.n_ref; ++r) { hdr->ref_name.emplace_back((const char*)data + name_off[r], name_len[r]); hdr->ref_len.push_back(ref_len[r]); }
        n_ref_ = (int32_t)h.n_ref;
        bam_slot_ = k; bam_first_ = h.first - (n - s.n_out);  // the header ends in this batch (or exactly at its end)
        return true;
    }
}

// Index + keys of slot s's inflated bytes, the chain starting at `first`: on the device behind the inflate kernel, whose
// output is still in device memory, or on this thread.
bool GzSource::index_batch(Slot& s, uint64_t first, BamIndex* ix) {
    if (bam_ == kBamHost) return index_on_host(s, first, ix);
    if (!s.bb && mgx_bam_batch_create(ctx_, s.b, out_cap_, max_records_, n_ref_, &s.bb)) { err_ = std::string("GPU: ") + mgx_last_error(); return false; }
    if (mgx_bam_batch_submit(ctx_, s.bb, s.n_out, first)) { err_ = std::string("GPU: ") + mgx_last_error(); return false; }
    // The next batch's inflate is already queued on the context's one stream, ahead of these kernels: their results come
    // after it.  So read and submit the batch after that one now, while the device works, instead of with the device idle
    // once the wait is over.
    const bool topped = top_up();
    const auto w0 = std::chrono::steady_clock::now();
    const int rc = mgx_bam_batch_wait(ctx_, s.bb, &ix->off, &ix->keys, &ix->n, &ix->next);
    wait_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    if (!topped) return false;
    if (rc == -E2BIG) {                                          // more (tiny) records than the batch's arrays hold
        if (++n_host_batches_ == 1 && getenv("MGX_CLI_TRACE"))
            fprintf(stderr, "  BAM: a batch of %llu bytes holds more than %llu records: walked and keyed on the host (as is every such batch)\n",
                    (unsigned long long)s.n_out, (unsigned long long)max_records_);
        return index_on_host(s, first, ix);
    }
    if (rc == -EBADMSG) {
        const std::string why = mgx_last_error();
        const size_t colon = why.find(": ");
        err_ = "corrupt BAM record at offset " + std::to_string(batch_base_ + ix->next) + " of the uncompressed stream: " + (colon == std::string::npos ? why : why.substr(colon + 2));
        return false;
    }
    if (rc) { err_ = std::string("GPU: ") + mgx_last_error(); return false; }
    return true;
}

bool GzSource::index_on_host(Slot& s, uint64_t first, BamIndex* ix) {
    const uint8_t* data = (const uint8_t*)s.out_ptr;
    int rc = mgx_bam_walk_host(data, s.n_out, first, 0, nullptr, &ix->n, &ix->next);
    if (!rc) {
        s.h_off.resize(ix->n); s.h_keys.resize(ix->n);
        rc = mgx_bam_walk_host(data, s.n_out, first, ix->n, s.h_off.data(), &ix->n, &ix->next);
    }
    if (rc == -EBADMSG) {
        const std::string why = mgx_last_error();
        const size_t colon = why.find(": ");
        err_ = "corrupt BAM record at offset " + std::to_string(batch_base_ + ix->next) + " of the uncompressed stream: " + (colon == std::string::npos ? why : why.substr(colon + 2));
        return false;
    }
    if (!rc) rc = mgx_bam_keys_rules(data, s.h_off.data(), ix->n, s.h_keys.data());      // what is marked redo is the parsers' work, as with device keys
    if (rc) { err_ = std::string("BAM input: ") + mgx_last_error(); return false; }
    ix->off = s.h_off.data(); ix->keys = s.h_keys.data();
    return true;
}

// The record that the batch before left cut (the tail of carry_) takes its remaining bytes from the head of this batch:
// *first = where the chain goes on in this batch.  *whole = false: the batch ends before the record does (all of the batch
// went into carry_).  False: err_.
bool GzSource::seam_record(const uint8_t* data, uint64_t n_out, uint64_t* first, bool* whole) {
    *first = 0; *whole = true;
    uint64_t tail = carry_.size() - carry_whole_;
    if (tail == 0) return true;
    uint64_t used = 0;
    if (tail < 4) {                                          // block_size itself is cut
        used = std::min<uint64_t>(4 - tail, n_out);
        carry_.insert(carry_.end(), data, data + used);
        tail += used;
        if (tail < 4) { *whole = false; return true; }
    }
    int32_t bs;
    memcpy(&bs, &carry_[carry_whole_], 4);
    const uint64_t at = carry_at_ + carry_whole_;
    if (bs < 32 || bs > MGX_BAM_MAX_RECORD) {
        err_ = "corrupt BAM record at offset " + std::to_string(at) + " of the uncompressed stream: block_size is " + std::to_string(bs);
        return false;
    }
    const uint64_t len = 4 + (uint64_t)bs;
    if (len > out_cap_) {
        err_ = "BAM record at offset " + std::to_string(at) + " of the uncompressed stream has " + std::to_string(len) + " bytes: longer than an inflate batch holds (" +
               std::to_string(out_cap_) + " bytes; MGX_CLI_INFLATE_BATCH sets a quarter of that)";
        return false;
    }
    const uint64_t take = std::min<uint64_t>(len - tail, n_out - used);
    carry_.insert(carry_.end(), data + used, data + used + take);
    used += take; tail += take;
    if (tail < len) { *whole = false; return true; }
    carry_whole_ = carry_.size();
    *first = used;
    return true;
}

bool GzSource::cut_bam(size_t slice_bytes, const slicecut::Push& push, const slicecut::Stopped& stopped) {
    auto push_carry = [&]() {                                // the whole records of carry_ as an owned slice
        slicecut::Slice sl;
        sl.bam = true; sl.bam_at = carry_at_;
        sl.text.assign((const char*)carry_.data(), carry_whole_);
        carry_.erase(carry_.begin(), carry_.begin() + (std::ptrdiff_t)carry_whole_);
        carry_at_ += carry_whole_; carry_whole_ = 0;
        return push(std::move(sl));
    };
    int k = bam_slot_;
    uint64_t first = bam_first_;
    bool from_header = true;
    for (;; from_header = false) {
        if (!from_header) {
            if (stopped()) return true;
            k = next_batch();
            if (k == -2) return true;
            if (k < 0) break;
        }
        Slot& s = slots_[k];
        const uint8_t* data = (const uint8_t*)s.out_ptr;
        std::shared_ptr<void> hold(static_cast<void*>(&s), [this, k](void*) { release(k); });
        bool whole = true;
        if (!from_header && !seam_record(data, s.n_out, &first, &whole)) return false;
        if (!whole) { batch_base_ += s.n_out; continue; }
        BamIndex ix;
        if (!index_batch(s, first, &ix)) return false;
        // the records [0, j) may continue the name group carry_ ends with: they join it in an owned slice
        uint64_t j = 0;
        if (carry_whole_) {
            for (j = ix.n ? 1 : 0; j < ix.n && ix.keys[j].same_qname; ++j) {}
            if (j == ix.n) {                                 // no name group ends in this batch: all of it is carried on
                carry_.insert(carry_.end(), data + first, data + s.n_out);
                carry_whole_ += ix.next - first;
                batch_base_ += s.n_out;
                continue;
            }
            carry_.insert(carry_.end(), data + first, data + ix.off[j]);
            carry_whole_ = carry_.size();
            if (!push_carry()) return true;
        } else carry_at_ = batch_base_ + (ix.n ? ix.off[0] : ix.next);
        // the last name group may go on in the next batch: it is carried, with the cut record behind it
        uint64_t lg = ix.n;
        while (lg > j && ix.keys[lg - 1].same_qname) --lg;
        if (lg > j) --lg;
        for (uint64_t a = j; a < lg;) {
            uint64_t b = a + 1;
            while (b < lg && (ix.keys[b].same_qname || ix.off[b] - ix.off[a] < slice_bytes)) ++b;
            slicecut::Slice sl;
            sl.bam = true; sl.bam_data = data; sl.rec_off = ix.off + a; sl.keys = ix.keys + a; sl.n_rec = (size_t)(b - a);
            sl.bam_at = batch_base_ + ix.off[a]; sl.hold = hold;
            if (!push(std::move(sl))) return true;
            a = b;
        }
        const uint64_t from = lg < ix.n ? ix.off[lg] : ix.next;
        carry_.assign(data + from, data + s.n_out);
        carry_whole_ = ix.next - from; carry_at_ = batch_base_ + from;
        batch_base_ += s.n_out;
    }
    if (!err_.empty() || !bgzf_ended_well()) return false;
    if (carry_.size() > carry_whole_) {
        err_ = name_ + " is truncated: it ends inside the BAM record at offset " + std::to_string(carry_at_ + carry_whole_) + " of the uncompressed stream";
        return false;
    }
    if (carry_whole_) push_carry();
    return true;
}
