// gz_source.cpp -- see gz_source.h
#include "gz_source.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "gang.h"
#include "mgx_pairhmm.h"       // mgx_last_error

using slicecut::TextChunk;

GzSource::GzSource(FILE* f, std::string head, std::string name, int device, int threads, bool host)
    : f_(f), pending_(head.begin(), head.end()), name_(std::move(name)), device_(device), threads_(std::max(1, threads)), host_(host) {
    // compressed / inflated bytes per batch: by default ~2000 blocks of level-6 SAM text, what the kernel needs to fill
    // the device (tools/dev_bgzf_inflate.py: 2.2 GB/s at 512 blocks per batch, 7.9 GB/s from 2048 on)
    if (const char* e = getenv("MGX_CLI_INFLATE_BATCH")) { const long long v = atoll(e); if (v > 0) in_cap_ = std::max<uint64_t>((uint64_t)v, 256u << 10); }
    out_cap_ = 4 * in_cap_;                  // a batch takes fewer blocks when the text inflates more than 4 x
    max_blocks_ = (uint32_t)std::min<uint64_t>(1u << 18, in_cap_ / 26 + 1);
}
GzSource::~GzSource() {
    for (Slot& s : slots_) {
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
    return host_ ? 0 : (uint64_t)(kSlots - made) * (in_cap_ + out_cap_ + 2 * ((uint64_t)max_blocks_ + 1) * 8 + (uint64_t)max_blocks_ * 4);
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

bool GzSource::next_piece(TextChunk* out) {
    if (!err_.empty()) return false;
    if (!gzip_) {
        for (;;) {
            while ((int)flight_.size() < kDepth && !bgzf_done_ && free_slot() >= 0) if (!fill_and_submit(free_slot())) return false;
            if (!flight_.empty()) break;
            if (bgzf_done_) break;
            std::unique_lock<std::mutex> lk(mu_);                // every batch holds text being parsed: wait for one
            cv_.wait(lk, [&] { if (aborted_) return true; for (const Slot& s : slots_) if (!s.busy) return true; return false; });
            if (aborted_) return false;
        }
        if (!flight_.empty()) {
            const int k = flight_.front();
            flight_.pop_front();
            Slot& s = slots_[k];
            const char* text = nullptr;
            if (!host_) {
                const auto w0 = std::chrono::steady_clock::now();
                const uint8_t* o; const uint32_t* st;
                if (mgx_bgzf_inflate_batch_wait(ctx_, s.b, &o, &st)) {
                    err_ = std::string("compressed input, at about byte ") + std::to_string(s.at) + ": " + mgx_last_error();
                    return false;
                }
                wait_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
                text = (const char*)o;
            } else text = s.host_out.data();
            out->data = text; out->size = s.n_out;
            out->hold = std::shared_ptr<void>(static_cast<void*>(&s), [this, k](void*) { release(k); });
            return true;
        }
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
