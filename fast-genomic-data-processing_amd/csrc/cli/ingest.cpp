// ingest.cpp -- see ingest.h
#include "ingest.h"

#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mgx_bam.h"
#include "mgx_sam.h"
#include "mgx_pairhmm.h"       // mgx_last_error

using slicecut::Slice;
using clk = std::chrono::steady_clock;

bool sam_on_device() {
    const char* e = getenv("MGX_CLI_SAM");
    return e && !strcmp(e, "device");
}

bool pread_all(int fd, char* dst, size_t n, uint64_t at) {
    while (n) {
        const ssize_t g = pread(fd, dst, n, (off_t)at);
        if (g <= 0) { if (g < 0 && errno == EINTR) continue; return false; }
        dst += g; n -= (size_t)g; at += (uint64_t)g;
    }
    return true;
}

// ---- GpuBringUp --------------------------------------------------------------------------------------------------------
GpuBringUp::GpuBringUp(int device, OutMode mode, uint64_t text_bytes, uint64_t inflate_hbm, uint64_t L) : out_mode(mode) {
    thread_ = std::thread([=]() { run(device, text_bytes, inflate_hbm, L); });
}

void GpuBringUp::run(int device, uint64_t text_bytes, uint64_t inflate_hbm, uint64_t L) {
    bool ok = true;
    bool use_store = out_mode == kOutDevice;
    const bool tr = getenv("MGX_CLI_TRACE") != nullptr;
    const auto i0 = clk::now();
    auto since = [&]() { return std::chrono::duration<double>(clk::now() - i0).count(); };
    // What the parsers wait for comes first: the record store (runtime start, streams, the first piece of HBM) and the
    // sort context; the compressor's own state is set up afterwards, while the text is being parsed.
    if (use_store && text_bytes) {
        // -z device keeps every BAM byte in HBM next to the sort's buffers; when the input cannot fit, say so now and keep
        // the bytes in host memory instead of failing in the middle of the ingest.  BAM bytes are about half
        // the SAM text; the sort and the emit need about 100 bytes per record of ~360 text bytes on top.
        uint64_t free_b = 0, total_b = 0;
        if (mgx_bgzf_device_memory(device, &free_b, &total_b) == 0) {
            if (const char* e = getenv("MGX_CLI_DEVICE_FREE")) free_b = strtoull(e, nullptr, 10);      // tests: pretend
            const uint64_t need = text_bytes * 6 / 10 + (text_bytes / 360) * 100 + (1ull << 30) + inflate_hbm;
            if (need > free_b) {
                fprintf(stderr, "sortmardup: about %.1f GB of device memory needed for -z device, %.1f GB free: keeping the BAM bytes in host memory (-z pinned)\n",
                        need / 1e9, free_b / 1e9);
                use_store = false; out_mode = kOutPinned;
            }
        }
    }
    if (tr) fprintf(stderr, "  bring-up: runtime up, device memory known at %.3f s\n", since());
    if ((use_store || sam_on_device()) && mgx_bgzf_create(device, 0, &zctx)) ok = false;      // the SAM batches hang off it too
    if (tr) fprintf(stderr, "  bring-up: compressor context at %.3f s\n", since());
    if (ok && use_store && (mgx_bgzf_store_create(zctx, &store) || mgx_bgzf_store_reserve(store, text_bytes ? text_bytes * 6 / 10 : (1ull << 30)))) ok = false;
    if (tr) fprintf(stderr, "  bring-up: record store ready at %.3f s\n", since());
    if (ok && (mgx_sortdedup_create(device, 0, &sd) || mgx_sortdedup_upload_begin(sd, L, text_bytes / 256))) ok = false;
    if (tr) fprintf(stderr, "  bring-up: sort context ready at %.3f s\n", since());
    {
        std::lock_guard<std::mutex> g(mu_);
        if (!ok) error_ = mgx_last_error();
        state_ = ok ? 1 : -1;
        cv_.notify_all();
    }
    if (ok && zctx && mgx_bgzf_prepare(zctx)) fprintf(stderr, "sortmardup: %s\n", mgx_last_error());      // not fatal here: the output stage reports it
    if (tr) fprintf(stderr, "  bring-up: compressor ready at %.3f s\n", since());
}

bool GpuBringUp::ready() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return state_ != 0; });
    return state_ == 1;
}

int GpuBringUp::state_now() { std::lock_guard<std::mutex> lk(mu_); return state_; }

// ---- one slice: text -> BAM-ready records -> packed records ------------------------------------------------------------
static void parse_slice(const char* data, size_t size, const samtext::Header& h, Chunk* c) {
    size_t off = 0, hi = size;
    {
        // sized from the text so that the vectors do not grow by doubling (a record is rarely under 100 bytes of text)
        const size_t est = size / 100 + 16;
        c->flag.reserve(est); c->tid.reserve(est); c->pos.reserve(est); c->end.reserve(est);
        c->cigar_off.reserve(est + 1); c->score.reserve(est); c->qname_off.reserve(est + 1); c->blob_off.reserve(est + 1);
        c->cigar.reserve(est * 2); c->qname.reserve(size / 4); c->blob.reserve(size);
    }
    while (off < hi) {
        const char* nl = (const char*)memchr(data + off, '\n', hi - off);
        size_t len = nl ? (size_t)(nl - (data + off)) : hi - off;
        const size_t next = off + len + 1;
        if (len && data[off + len - 1] == '\r') --len;
        if (len) {
            samtext::Parsed pr;
            if (!samtext::parse_record_into(data + off, len, h, &pr, &c->cigar, nullptr, &c->qname, &c->blob, &c->err)) {
                c->err += " at: " + std::string(data + off, std::min<size_t>(len, 80));
                return;
            }
            c->flag.push_back(pr.flag); c->tid.push_back(pr.tid); c->pos.push_back(pr.pos); c->end.push_back(pr.end);
            c->cigar_off.push_back(c->cigar.size()); c->score.push_back(pr.score); c->qname_off.push_back(c->qname.size());
            c->blob_off.push_back(c->blob.size());
        }
        off = next;
    }
    const size_t n = c->flag.size();
    mgx_raw_records_t raw{};
    raw.n_records = n; raw.flag = c->flag.data(); raw.tid = c->tid.data(); raw.pos = c->pos.data();
    raw.cigar_off = c->cigar_off.data(); raw.cigar = c->cigar.data(); raw.qual_off = nullptr; raw.qual = nullptr;      // the score comes from the parser
    raw.qname_off = c->qname_off.data(); raw.qname = c->qname.data();
    raw.n_targets = (uint32_t)h.ref_len.size(); raw.target_len = h.ref_len.data();
    c->recs.resize(n); c->input_index.resize(n);
    uint64_t L = 0;
    if (mgx_sortdedup_pack_scored(&raw, c->score.data(), c->recs.data(), c->input_index.data(), &L)) { c->err = std::string("pack: ") + mgx_last_error(); return; }
    // the parse-time arrays are not needed any more (the keys are in recs); keep what the writer needs
    std::vector<uint32_t>().swap(c->cigar); std::vector<uint16_t>().swap(c->score); std::vector<char>().swap(c->qname);
    std::vector<uint64_t>().swap(c->cigar_off); std::vector<uint64_t>().swap(c->qname_off);
}

// ---- one slice of BAM records (-b): keys -> the same Chunk -------------------------------------------------------------------
// The records are whole and valid (the index walked them); their keys come from the device, or, for an owned slice, from
// the host functions here.  The record bytes go on unchanged, without their block_size field.
// A record that the host key functions refuse (its CIGAR is in a CG tag): the library names its offset in `data`; name it in
// the uncompressed stream, where data[0] is at `base`.  The refused record is the first whose key is still marked redo.
static std::string refused_record(const uint64_t* off, const std::vector<mgx_bam_key_t>& keys, uint64_t base) {
    const std::string why = mgx_last_error();
    const size_t colon = why.find(": ");
    uint64_t i = 0;
    while (i < keys.size() && !keys[i].redo) ++i;
    if (i == keys.size() || colon == std::string::npos) return why;
    return "BAM record at offset " + std::to_string(base + off[i]) + " of the uncompressed stream: " + why.substr(colon + 2);
}

// What a Chunk holds per record besides the bytes, and the pairing, from complete keys (BAM input and SAM text encoded on the
// device end here).  False: c->err.
static bool chunk_from_keys(const std::vector<mgx_bam_key_t>& keys, const samtext::Header& h, Chunk* c) {
    const uint64_t n = keys.size();
    c->flag.resize(n); c->tid.resize(n); c->pos.resize(n); c->end.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        const mgx_bam_key_t& k = keys[i];
        c->flag[i] = k.flag; c->tid[i] = k.tid; c->pos[i] = k.pos; c->end[i] = k.end;
    }
    c->recs.resize(n); c->input_index.resize(n);
    uint64_t L = 0;
    if (mgx_bam_pack_keys(n, keys.data(), (uint32_t)h.ref_len.size(), h.ref_len.data(), c->recs.data(), c->input_index.data(), &L)) {
        c->err = std::string("pack: ") + mgx_last_error();
        return false;
    }
    return true;
}

static void parse_bam_slice(const Slice& sl, const samtext::Header& h, Chunk* c) {
    const uint8_t* data = sl.bam_data;
    const uint64_t* off = sl.rec_off;
    uint64_t n = sl.n_rec;
    std::vector<uint64_t> own_off;
    std::vector<mgx_bam_key_t> keys;
    if (!data) {                                             // owned bytes: what straddled two batches
        data = (const uint8_t*)sl.text.data();
        uint64_t next = 0;
        int rc = mgx_bam_walk_host(data, sl.text.size(), 0, 0, nullptr, &n, &next);
        if (!rc) { own_off.resize(n); rc = mgx_bam_walk_host(data, sl.text.size(), 0, n, own_off.data(), &n, &next); }
        if (rc == -EBADMSG) {                                 // the message names the offset inside the slice: name it in the stream
            const std::string why = mgx_last_error();
            const size_t colon = why.find(": ");
            c->err = "corrupt BAM record at offset " + std::to_string(sl.bam_at + next) + " of the uncompressed stream: " + (colon == std::string::npos ? why : why.substr(colon + 2));
            return;
        }
        if (rc || next != sl.text.size()) { c->err = rc ? mgx_last_error() : "a slice of records does not end with a record"; return; }
        off = own_off.data();
        keys.resize(n);
        if (mgx_bam_keys_host(data, off, n, keys.data())) { c->err = refused_record(off, keys, sl.bam_at); return; }
    } else {
        const mgx_bam_key_t* k = static_cast<const mgx_bam_key_t*>(sl.keys);
        keys.assign(k, k + n);
        // what the device rules declined (tokens that need strtol, the long-CIGAR placeholder) is derived here
        if (mgx_bam_keys_redo(data, off, n, keys.data())) { c->err = refused_record(off, keys, sl.bam_at - off[0]); return; }       // bam_at: where the slice's first record is
    }
    c->blob_off.resize(n + 1);
    uint64_t bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        int32_t bs;
        memcpy(&bs, data + off[i], 4);
        c->blob_off[i] = bytes; bytes += (uint32_t)bs;
    }
    c->blob_off[n] = bytes;
    c->blob.resize(bytes);
    for (uint64_t i = 0; i < n; ++i) memcpy(c->blob.data() + c->blob_off[i], data + off[i] + 4, c->blob_off[i + 1] - c->blob_off[i]);
    if (!chunk_from_keys(keys, h, c)) c->err += " (records of the slice at offset " + std::to_string(sl.bam_at) + " of the uncompressed stream)";
}

// ---- one slice of SAM text, encoded on the device (MGX_CLI_SAM=device) ---------------------------------------
// The thread's batch takes the slice's text, the device gives BAM records and keys; the lines its rule set declined, and the
// few whose key the BAM rules left to the host, are encoded by parse_record_into as always and keyed by mgx_bam_keys_host
// on those bytes.  Records keep the slice's order.  With a record store the device-made records go into it device to
// device and never cross PCIe; otherwise they come back into c->blob.
void Ingest::parse_slice_device(const char* data, size_t size, SamBatch* sb, Chunk* c) {
    if (!gpu_.ready()) { c->err = "GPU: " + gpu_.error(); return; }
    // thread time per step, summed over the slices and threads for MGX_CLI_TRACE: copy in | submit + wait | host lines | records placed | pairing
    auto t_last = clk::now();
    auto lap = [&](int k) { const auto t = clk::now(); sam_ns_[k] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t - t_last).count(); t_last = t; };
    mgx_bgzf_t* ctx = gpu_.zctx;
    mgx_bgzf_store_t* store = gpu_.store;
    uint64_t want_rec = std::max<uint64_t>(sb->max_rec, size / 64 + 1024);      // ordinary lines are a few hundred bytes
    const uint64_t* line_off; const uint32_t* line_len; const uint64_t* rec_off; const mgx_bam_key_t* dkeys; const uint8_t* bytes = nullptr;
    uint64_t n = 0, n_out = 0;
    for (;;) {
        if (!sb->b || sb->cap < size || sb->max_rec < want_rec) {            // grows with the slices (a window that doubled)
            if (sb->b) mgx_sam_batch_destroy(ctx, sb->b);
            sb->b = nullptr;
            sb->cap = std::max<uint64_t>(size, sb->cap * 2); sb->max_rec = want_rec;
            if (mgx_sam_batch_create(ctx, sam_table_, sb->cap, sb->max_rec, &sb->b)) { c->err = std::string("GPU: ") + mgx_last_error(); return; }
        }
        memcpy(mgx_sam_batch_input(sb->b), data, size);
        lap(0);
        int rc = mgx_sam_batch_submit(ctx, sb->b, size);
        if (!rc) rc = mgx_sam_batch_wait(ctx, sb->b, &line_off, &line_len, &rec_off, &dkeys, &n, &n_out, store ? nullptr : &bytes);
        if (rc == -E2BIG && want_rec < size / 2 + 1) { want_rec = std::min<uint64_t>(want_rec * 4, size / 2 + 1); continue; }      // short lines: more of them
        if (rc) { c->err = std::string("GPU: ") + mgx_last_error(); return; }
        break;
    }
    lap(1);
    // the lines left to the host, in order: the first one the parser rejects is the slice's error, worded as parse_slice words it
    std::vector<mgx_bam_key_t> keys(dkeys, dkeys + n);
    std::vector<uint8_t> host;                               // their records, block_size in front
    std::vector<uint64_t> host_line, host_off;
    {
        std::vector<uint32_t> cigar; std::vector<char> qname; std::vector<uint8_t> blob;
        for (uint64_t i = 0; i < n; ++i) {
            if (!keys[i].redo) continue;
            samtext::Parsed pr;
            cigar.clear(); qname.clear(); blob.clear();
            if (!samtext::parse_record_into(data + line_off[i], line_len[i], hdr_, &pr, &cigar, nullptr, &qname, &blob, &c->err)) {
                c->err += " at: " + std::string(data + line_off[i], std::min<size_t>(line_len[i], 80));
                return;
            }
            const uint32_t bs = (uint32_t)blob.size();
            host_line.push_back(i); host_off.push_back(host.size());
            host.insert(host.end(), (const uint8_t*)&bs, (const uint8_t*)&bs + 4);
            host.insert(host.end(), blob.begin(), blob.end());
        }
        if (!host_line.empty()) {
            std::vector<mgx_bam_key_t> hk(host_line.size());
            if (mgx_bam_keys_host(host.data(), host_off.data(), host_off.size(), hk.data())) { c->err = mgx_last_error(); return; }
            for (size_t j = 0; j < hk.size(); ++j) {
                const uint8_t same = keys[host_line[j]].same_qname;      // from the text, by the device: the host saw the record alone
                keys[host_line[j]] = hk[j];
                keys[host_line[j]].same_qname = same;
            }
        }
    }
    sam_lines_device_ += n - host_line.size(); sam_lines_host_ += host_line.size();
    lap(2);
    // where every record is: without its block_size field, as the writer takes it
    std::vector<uint64_t> size_of(n);
    for (uint64_t i = 0; i < n; ++i) size_of[i] = rec_off[i + 1] - rec_off[i];
    for (size_t j = 0; j < host_line.size(); ++j) size_of[host_line[j]] = (j + 1 < host_off.size() ? host_off[j + 1] : host.size()) - host_off[j];
    if (store) {
        uint64_t dev_at = 0, host_at = 0;
        if (mgx_bgzf_store_put_device(store, mgx_sam_batch_device_records(sb->b), n_out, &dev_at) || mgx_bgzf_store_put(store, host.data(), host.size(), &host_at)) {
            c->err = std::string("GPU: ") + mgx_last_error();
            return;
        }
        c->rec_addr.resize(n); c->rec_len.resize(n);
        size_t j = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const bool on_host = j < host_line.size() && host_line[j] == i;
            c->rec_addr[i] = (on_host ? host_at + host_off[j] : dev_at + rec_off[i]) + 4;
            c->rec_len[i] = (uint32_t)(size_of[i] - 4);
            j += on_host;
        }
    } else {
        c->blob_off.resize(n + 1);
        uint64_t total = 0;
        for (uint64_t i = 0; i < n; ++i) { c->blob_off[i] = total; total += size_of[i] - 4; }
        c->blob_off[n] = total;
        c->blob.resize(total);
        size_t j = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const bool on_host = j < host_line.size() && host_line[j] == i;
            memcpy(c->blob.data() + c->blob_off[i], (on_host ? host.data() + host_off[j] : bytes + rec_off[i]) + 4, size_of[i] - 4);
            j += on_host;
        }
    }
    lap(3);
    chunk_from_keys(keys, hdr_, c);
    lap(4);
}

// ---- Ingest ------------------------------------------------------------------------------------------------------------
Ingest::Ingest(const samtext::Header& hdr, GpuBringUp& gpu, int threads, const char* in_base, int in_fd, slicecut::PieceSource* src)
    : hdr_(hdr), gpu_(gpu), in_base_(in_base), in_fd_(in_fd), src_(src), queue_cap_((size_t)threads * 2) {
    if (sam_on_device()) {                                   // the header's names as the device looks them up
        std::string names; std::vector<uint32_t> at(1, 0);
        for (const std::string& nm : hdr.ref_name) { names += nm; at.push_back((uint32_t)names.size()); }
        names.push_back('\0');
        if (mgx_sam_table_create((uint32_t)hdr.ref_name.size(), (const uint8_t*)names.data(), at.data(), &sam_table_)) fail(std::string("SAM table: ") + mgx_last_error());
    }
    for (int t = 0; t < threads; ++t) pool_.emplace_back([this]() { worker(); });
}

bool Ingest::push(Slice sl) {
    sl.seq = seq_++;
    std::unique_lock<std::mutex> lk(mu_);
    cv_room_.wait(lk, [&] { return queue_.size() < queue_cap_ || failed_.load(); });
    if (failed_.load()) return false;
    queue_.push_back(std::move(sl));
    cv_work_.notify_one();
    return true;
}

void Ingest::fail(const std::string& msg) {
    std::deque<Slice> dropped;                               // (released outside the lock: a slice may hold an inflate batch)
    {
        std::lock_guard<std::mutex> g(mu_);
        if (!failed_.exchange(true)) first_error_ = msg;
        dropped.swap(queue_);                                // nothing queued will be parsed now
        cv_work_.notify_all(); cv_room_.notify_all();
    }
    if (src_) src_->abort();                                 // a reader waiting for a batch to come free stops waiting
}

void Ingest::finish() {
    {
        std::lock_guard<std::mutex> g(mu_);
        done_reading_ = true;
        cv_work_.notify_all();
    }
    for (auto& th : pool_) th.join();
    pool_.clear();
    queue_.clear();                                          // (after a failure: slices never parsed still hold inflated text)
    if (sam_table_) {
        if (getenv("MGX_CLI_TRACE"))
            fprintf(stderr, "  sam device: %llu lines encoded on the device, %llu declined and encoded on the host\n",
                    (unsigned long long)sam_lines_device_.load(), (unsigned long long)sam_lines_host_.load());
        if (getenv("MGX_CLI_TRACE"))
            fprintf(stderr, "  sam device: thread seconds over all parsers: %.3f copying text into pinned input, %.3f in submit + wait, %.3f on host-encoded lines, "
                            "%.3f placing the records (store puts / copies into blob), %.3f filling the chunk and pairing\n",
                    sam_ns_[0].load() / 1e9, sam_ns_[1].load() / 1e9, sam_ns_[2].load() / 1e9, sam_ns_[3].load() / 1e9, sam_ns_[4].load() / 1e9);
        mgx_sam_table_destroy(sam_table_);
        sam_table_ = nullptr;
    }
}

// The in-order commit is the one serial step of the ingest: it only turns slice-local mate indices into arrival
// indices and hands the packed records to the upload; what it frees is handed back to die outside the lock.
void Ingest::commit_ready(std::vector<std::vector<mgx_rec_t>>* trash) {
    const auto c0 = clk::now();
    struct Acc { double* d; clk::time_point t; ~Acc() { *d += std::chrono::duration<double>(clk::now() - t).count(); } } acc{&commit_seconds, c0};
    for (;;) {
        auto it = ready_.find(next_commit_);
        if (it == ready_.end()) return;
        std::unique_ptr<Chunk> ch = std::move(it->second);
        ready_.erase(it);
        const uint64_t base = n_total, n = ch->recs.size();
        if (base + n >= 0xFFFFFFF0ull) { fail("more than 2^32 records"); return; }
        for (auto& r : ch->recs) if (r.mate != MGX_NO_MATE) r.mate += (uint32_t)base;        // slice-local -> global arrival index
        const auto u0 = clk::now();
        if (n && mgx_sortdedup_upload_chunk(gpu_.sd, base, n, ch->recs.data())) { fail(std::string("GPU: ") + mgx_last_error()); return; }
        upload_seconds += std::chrono::duration<double>(clk::now() - u0).count();
        ch->arrival_base = base;
        n_total += n;
        trash->emplace_back(std::move(ch->recs));
        kept_chunks.push_back(std::move(ch));
        ++next_commit_;
    }
}

// what a parsed slice still needs of the device: its BAM bytes into the record store, the writer's view of its records, the
// in-order commit (upload of the packed records)
bool Ingest::finish_chunk(std::unique_ptr<Chunk> ch, uint64_t seq) {
    mgx_bgzf_store_t* store = gpu_.store;
    if (store && ch->rec_addr.empty()) {            // the slice's BAM bytes go to HBM now and leave host memory (device-encoded SAM: they are there)
        if (mgx_bgzf_store_put(store, ch->blob.data(), ch->blob.size(), &ch->dev_base)) { fail(std::string("GPU: ") + mgx_last_error()); return false; }
        std::vector<uint8_t>().swap(ch->blob);
    }
    {
        // the writer's view of every record, in the slice's arrival order; the parse-time arrays die here
        const size_t n = ch->recs.size();
        ch->kept.resize(n);
        for (size_t k = 0; k < n; ++k) {
            const uint32_t src = ch->input_index[k];
            const bool addressed = !ch->rec_addr.empty();
            const uint8_t* where = addressed ? (const uint8_t*)(uintptr_t)ch->rec_addr[src]
                                   : store   ? (const uint8_t*)(uintptr_t)(ch->dev_base + ch->blob_off[src]) : ch->blob.data() + ch->blob_off[src];
            ch->kept[k] = Kept{where, addressed ? ch->rec_len[src] : (uint32_t)(ch->blob_off[src + 1] - ch->blob_off[src]), ch->tid[src], (int32_t)ch->pos[src],
                               ch->end[src], (ch->flag[src] & 4) == 0};
        }
        std::vector<uint64_t>().swap(ch->rec_addr); std::vector<uint32_t>().swap(ch->rec_len);
        std::vector<uint32_t>().swap(ch->input_index);
        std::vector<uint16_t>().swap(ch->flag); std::vector<int32_t>().swap(ch->tid); std::vector<int64_t>().swap(ch->pos);
        std::vector<int32_t>().swap(ch->end); std::vector<uint64_t>().swap(ch->blob_off);
    }
    std::vector<std::vector<mgx_rec_t>> trash;
    {
        std::lock_guard<std::mutex> g(commit_mu_);
        ready_.emplace(seq, std::move(ch));
        commit_ready(&trash);
    }
    return !failed_.load();
}

// Parses one slice where its text is: in the mapping of the input file, in this thread's buffer after a pread, in a piece's
// buffer, or in the slice itself.  False after fail().
bool Ingest::parse(const Slice& sl, std::vector<char>* text_buf, SamBatch* sb, Chunk* ch) {
    auto parse_slice = [&](const char* data, size_t size, const samtext::Header& h, Chunk* c) {
        if (sam_table_) parse_slice_device(data, size, sb, c); else ::parse_slice(data, size, h, c);
    };
    if (sl.bam) {
        parse_bam_slice(sl, hdr_, ch);
        if (!ch->err.empty()) { fail("BAM input: " + ch->err); return false; }
        return true;
    }
    if (sl.from_file && in_base_) {
#ifdef MADV_POPULATE_READ
        const uintptr_t a0 = (uintptr_t)(in_base_ + sl.file_off) & ~(uintptr_t)4095, a1 = ((uintptr_t)(in_base_ + sl.file_off + sl.file_len) + 4095) & ~(uintptr_t)4095;
        (void)madvise((void*)a0, a1 - a0, MADV_POPULATE_READ);
        parse_slice(in_base_ + sl.file_off, sl.file_len, hdr_, ch);
        (void)madvise((void*)a0, a1 - a0, MADV_DONTNEED);      // drops this process's entries only: the pages stay in the page cache
#endif
    } else if (sl.from_file) {
        if (text_buf->size() < sl.file_len) text_buf->resize(sl.file_len);
        if (!pread_all(in_fd_, text_buf->data(), sl.file_len, sl.file_off)) { fail("read error on the input file"); return false; }
        parse_slice(text_buf->data(), sl.file_len, hdr_, ch);
    } else if (sl.ext) parse_slice(sl.ext, sl.ext_len, hdr_, ch);
    else parse_slice(sl.text.data(), sl.text.size(), hdr_, ch);
    if (!ch->err.empty()) { fail(ch->err.compare(0, 5, "GPU: ") == 0 ? ch->err : "SAM parse error: " + ch->err); return false; }
    return true;
}

void Ingest::worker() {
    std::vector<char> text_buf;                          // this thread's slice of the input file
    SamBatch sam_batch;                                  // ... and its device batch (MGX_CLI_SAM=device)
    struct Release { Ingest* in; SamBatch* sb; ~Release() { if (sb->b) mgx_sam_batch_destroy(in->gpu_.zctx, sb->b); } } release{this, &sam_batch};
    // The HIP runtime and the contexts take 0.2-0.3 s to come up: until then a parser keeps its parsed slices and goes on with
    // the next one instead of waiting with one slice in hand (round 3: at 4 M records the parse itself is 0.05 s of thread
    // time per thread -- the ingest was the bring-up plus everything that waited for it)
    std::vector<std::pair<uint64_t, std::unique_ptr<Chunk>>> waiting;
    for (;;) {
        Slice sl;
        bool have = false;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_work_.wait(lk, [&] { return !queue_.empty() || done_reading_ || failed_.load(); });
            if (failed_.load()) return;
            if (!queue_.empty()) {
                sl = std::move(queue_.front());
                queue_.pop_front();
                cv_room_.notify_one();
                have = true;
            }
        }
        std::unique_ptr<Chunk> ch;
        if (have) {
            ch.reset(new Chunk);
            const bool parsed = parse(sl, &text_buf, &sam_batch, ch.get());
            std::string().swap(sl.text);
            sl.hold.reset();                             // a piece's buffer goes back to its source once its text is parsed
            if (!parsed) return;
            // (bounded: 12 slices per thread -- ~80 MB of parsed records, 1.3 GB over 16 threads -- cover a 4 M-record input whole;
            // with 32 the peak resident set of a 20 M-record run grew from 5.8 to 9.2 GB for 0.1 s of ingest)
            if (waiting.size() < 12 && gpu_.state_now() == 0) { waiting.emplace_back(sl.seq, std::move(ch)); continue; }
        }
        if (!have && waiting.empty()) return;           // the input is used up and nothing of this thread's waits
        if (!gpu_.ready()) { fail("GPU: " + gpu_.error()); return; }
        for (auto& w : waiting) if (!finish_chunk(std::move(w.second), w.first)) return;
        waiting.clear();
        if (have) { if (!finish_chunk(std::move(ch), sl.seq)) return; }
        else return;
    }
}
