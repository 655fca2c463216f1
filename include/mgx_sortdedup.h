/*
 * mgx_sortdedup.h -- C ABI of the MI355X coordinate-sort + mark-duplicates core (libmgx.so).
 *
 * Drop-in seam: the reference has no FFI on this path -- sortmardup is one 600-line main()
 * (sortmardup/main.cpp) -- so the boundary is cut where its data stops being text/BAM bytes and
 * becomes fixed-size keys: right after a record has been parsed and paired (main.cpp:160-192),
 * up to the point where the output order and the duplicate bitmap are consumed by the writer
 * (main.cpp:359-397).  Reference code replaced, by entry point:
 *
 *   mgx_sortdedup_pack   <- BamParser pairing by adjacent qname   sortmardup/tbb/bam_parser.cpp:54-113
 *                           BAMRecord::score / get_unify_coordinate / prime5_pos
 *                                                                 sortmardup/tbb/bam_record.cpp:7-62
 *                           get_tile_x_y / str_to_uint16          sortmardup/tbb/pair.cpp:11-49
 *                           the arrival order of main.cpp:160-192 with one shuffle thread (-t 1)
 *                           (host code: byte/pointer work next to the parser)
 *   mgx_sortdedup_run    <- SinglePair / DoublePair construction  sortmardup/tbb/pair.cpp:51-108
 *                           double_pair_indicator bitmap          sortmardup/main.cpp:181-192
 *                           pair sorts + duplicate search         sortmardup/main.cpp:249-281, 299-341
 *                           stable coordinate sort                sortmardup/main.cpp:348-357
 *                           duplicate_index lookup per record     sortmardup/main.cpp:385-388
 *                           (device code: radix sorts + segmented best-of-run scan)
 *
 * Not part of this ABI: SAM text parsing and BGZF/BAM/BAI writing -- they live in
 * the sortmardup-compatible CLI built on top of it (fast-genomic-data-processing_amd/csrc/cli/).
 *
 * All functions return 0 or a negative errno-style code; mgx_last_error() has the message.
 */
#ifndef MGX_SORTDEDUP_H
#define MGX_SORTDEDUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgx_sortdedup mgx_sortdedup_t;

#define MGX_NO_MATE 0xFFFFFFFFu

/* One alignment record reduced to what sorting and duplicate marking need: 32 bytes, the unit
 * streamed host -> device.  Records are in ARRIVAL order (see mgx_sortdedup_pack). */
typedef struct mgx_rec {
    uint64_t coord;   /* unified coordinate kTable[tid] + pos; tid < 0 -> L   (bam_record.cpp:18-24) */
    uint64_t prime5;  /* unclipped 5' position, uint64 wrap as in the reference (bam_record.cpp:26-62) */
    uint32_t mate;    /* arrival index of the record paired with this one, or MGX_NO_MATE */
    uint16_t flag;    /* SAM flag */
    uint16_t score;   /* sum of base qualities >= 15, uint16 wrap             (bam_record.cpp:7-16) */
    uint16_t tile, x, y; /* parsed from the qname                             (pair.cpp:22-49) */
    uint16_t pad_;
} mgx_rec_t;

/* Parsed alignment records as a BAM reader holds them (structure of arrays, input order). */
typedef struct mgx_raw_records {
    uint64_t n_records;
    const uint16_t* flag;       /* [n] */
    const int32_t* tid;         /* [n]  (-1 = unmapped '*') */
    const int64_t* pos;         /* [n]  0-based leftmost position */
    const uint64_t* cigar_off;  /* [n+1] offsets into cigar */
    const uint32_t* cigar;      /* BAM encoding: len << 4 | op */
    const uint64_t* qual_off;   /* [n+1] offsets into qual */
    const uint8_t* qual;        /* phred values (not ASCII) */
    const uint64_t* qname_off;  /* [n+1] offsets into qname */
    const char* qname;          /* concatenated, NOT NUL-terminated */
    uint32_t n_targets;
    const uint64_t* target_len; /* [n_targets] @SQ LN */
} mgx_raw_records_t;

typedef struct mgx_sortdedup_stats {
    uint64_t n_records, n_double, n_single, n_dup_records;
    uint32_t key_bits_coord, key_bits_pair1, key_bits_pair2;
    uint32_t n_radix_passes;        /* scatter launches of the last run */
    float ms_total;                 /* HIP events around the whole device pipeline (resident input) */
    float ms_radix_scatter;         /* sum over all radix scatter launches */
    uint64_t radix_scatter_bytes;   /* algorithmic bytes those launches moved (read + write) */
    uint64_t alg_bytes;             /* LSD-8 traffic model of SURVEY.md section 8d for this input */
    /* the dominant kernel: the scatter launches of the record (coordinate) sort */
    float ms_scatter_records;       /* sum of their durations */
    uint32_t n_scatter_records;     /* how many launches */
    uint64_t scatter_records_bytes; /* algorithmic bytes they moved (read + write) */
    uint32_t n_key_hist_launches;   /* histogram passes of the last run that re-read the keys (k_radix_hist); the others (the
                                     * first pass of the record sort) merge the histograms the build kernel left (k_hist_merge) */
    uint32_t pad_;
    /* Which paths the pipeline pass took whose results are returned (after the huge-run fallback: the second pass). */
    uint32_t n_near;                /* double pairs keyed in the one-word near form; n_double - n_near took the two-word form */
    uint32_t n_multi_far;           /* runs of two or more two-word (far) pair entries */
    uint32_t n_multi_single;        /* runs of two or more single-read entries */
    uint32_t n_multi_near;          /* runs of two or more near entries: per start position, or per identity in the exact mode */
    uint32_t n_long_far;            /* far runs beyond the per-lane walk, handed to a whole workgroup */
    uint32_t n_long_single;         /* single-read runs handed to a whole workgroup */
    uint32_t n_long_near;           /* near runs handed to a whole workgroup */
    uint32_t n_builds;              /* 1, or 2 when a device maximum >= 2^32 made the build kernel run again with wide keys */
    uint32_t n_pipeline_runs;       /* 1, or 2 after the huge-run fallback */
    uint32_t bitmap_tiled;          /* 1: tiled bitmap (plain stores, reverse half at a tile boundary); 0: reference layout, atomics */
    uint32_t packed_coord;          /* 1: record sort on coord << 32 | arrival index words */
    uint32_t packed_pair;           /* 1: far entries carry mate end << 32 | record in one word (and near pairs exist at all) */
    uint32_t near_by_position;      /* 1: near pairs sorted on record 1's 5' end only; 0: six-pass sort on the whole identity */
    uint32_t pad2_;
} mgx_sortdedup_stats_t;

/* Host side (B3-B7): pair records by adjacent equal qname exactly as BamParser does, derive the
 * per-record keys and emit them in the reference's single-thread arrival order (mates pulled
 * adjacent).  out_recs and out_input_index must hold n_records entries;
 * out_input_index[k] = index in `raw` of arrival record k.  *out_L = sum of target lengths. */
int mgx_sortdedup_pack(const mgx_raw_records_t* raw, mgx_rec_t* out_recs, uint32_t* out_input_index,
                       uint64_t* out_L);
/* The same for a caller that has each record's BAMRecord::score at hand (sortmardup/tbb/bam_record.cpp:7-14: the base qualities
 * of at least 15 summed in a uint16_t) -- a SAM reader passes over every quality character anyway: score[n] replaces the scan of
 * raw->qual, and raw->qual / raw->qual_off may then be NULL.  score == NULL is mgx_sortdedup_pack. */
int mgx_sortdedup_pack_scored(const mgx_raw_records_t* raw, const uint16_t* score, mgx_rec_t* out_recs, uint32_t* out_input_index,
                              uint64_t* out_L);

/* flags: MGX_CU_PATTERN(p) and MGX_STREAM_HIGH_PRIORITY as for mgx_pairhmm_create (mgx_pairhmm.h), 0 otherwise */
int mgx_sortdedup_create(int device, unsigned flags, mgx_sortdedup_t** out);
void mgx_sortdedup_destroy(mgx_sortdedup_t* ctx);

/* Device side.  upload: stream the packed records into HBM (pinned staging, copy stream).
 * run: radix sorts + duplicate search on the resident records (asynchronous).
 * results: wait, then copy back
 *   out_order[k] = arrival index of the k-th record of the coordinate-sorted output
 *   out_dup[i]   = 1 iff arrival record i gets BAM_FDUP (0x400) set (a pre-existing 0x400 is
 *                  never cleared, main.cpp:385-388 only ever sets it). */
int mgx_sortdedup_upload(mgx_sortdedup_t* ctx, uint64_t L, uint64_t n_records, const mgx_rec_t* recs);
/* The same upload in pieces, for a producer that packs records while it is still parsing (the reference's reader
 * feeds its shuffle threads through a bounded queue of line blocks, sortmardup/main.cpp:505-562; here the pieces go
 * straight to the device, so parsing, staging and the PCIe copy overlap):
 *   begin   n_expected is a capacity hint (0 is fine; the device array grows when a chunk exceeds it)
 *   chunk   records [first_record, first_record + n_records) in arrival order, without gaps (first_record may not lie
 *           beyond what has been uploaded so far; re-sending a range overwrites it); mate indices are GLOBAL arrival
 *           indices; returns once the caller's buffer may be reused (the device copy continues in the background)
 *   end     n_records must equal the extent the chunks covered; waits for the copies */
int mgx_sortdedup_upload_begin(mgx_sortdedup_t* ctx, uint64_t L, uint64_t n_expected);
int mgx_sortdedup_upload_chunk(mgx_sortdedup_t* ctx, uint64_t first_record, uint64_t n_records, const mgx_rec_t* recs);
int mgx_sortdedup_upload_end(mgx_sortdedup_t* ctx, uint64_t n_records);
int mgx_sortdedup_run(mgx_sortdedup_t* ctx);
int mgx_sortdedup_results(mgx_sortdedup_t* ctx, uint32_t* out_order, uint8_t* out_dup);
int mgx_sortdedup_stats(mgx_sortdedup_t* ctx, mgx_sortdedup_stats_t* out);

/* One shot: upload + run + results. */
int mgx_sortdedup_sort_mark(mgx_sortdedup_t* ctx, uint64_t L, uint64_t n_records,
                            const mgx_rec_t* recs, uint32_t* out_order, uint8_t* out_dup);


/* ---- One record set over several GPUs (reference: the three range partitioners and the global
 * double_pair_indicator, sortmardup/tbb/range_partitioner.h:98-100, tbb/bam_partitioner.cpp:31-33,
 * main.cpp:160-192).  The host router cuts the arrival-ordered records into n_shards coordinate ranges of equal
 * width; each shard is TWO subsets of the input plus the marks that cross shard boundaries:
 *   ordering half  the records whose unified coordinate lies in the range (bam_partitioner)
 *   marking half   the templates keyed in the range -- pairs by their smaller 5' end, fragments by their 5' end
 *                  (double_partitioner / single_partitioner) -- as records with shard-local mate indices
 *   marks          5' ends of pairs that live in other shards but fall into this range: what the reference
 *                  writes into the shared bitmap becomes the only data exchanged between shards
 * A shard runs on any context with mgx_sortdedup_upload_shard + run + results; no collective is involved.
 * Concatenating the shards' orders in shard order is the global order; mgx_sortdedup_merge does that and
 * scatters the duplicate flags back to arrival indices.  Results are bit-identical to the single-shard call. */
typedef struct mgx_sortdedup_shard {
    uint64_t n_order;
    const uint64_t* order_coord;     /* [n_order] unified coordinate, arrival order kept */
    const uint32_t* order_arrival;   /* [n_order] global arrival index */
    uint64_t n_mark;
    const mgx_rec_t* mark_recs;      /* [n_mark] records 1 and 2 of a template adjacent, mate = shard-local index */
    const uint32_t* mark_arrival;    /* [n_mark] global arrival index of each marking record */
    uint64_t n_marks;
    const uint64_t* marks;           /* [n_marks] 5' position << 1 | 1 if it belongs to the reverse-strand half */
    uint64_t order_base;             /* where this shard's order starts in the global output */
    uint64_t coord_lo, coord_hi;     /* the shard's range [lo, hi) of coordinates / 5' positions */
} mgx_sortdedup_shard_t;
typedef struct mgx_sortdedup_routed mgx_sortdedup_routed_t;

/* Host side.  only_shard < 0 materialises every shard; otherwise only that one (a process that owns one GPU
 * routes the whole input but keeps its own shard; sizes and order_base of the others are still filled in). */
int mgx_sortdedup_route(uint64_t L, uint64_t n_records, const mgx_rec_t* recs, uint32_t n_shards, int only_shard,
                        mgx_sortdedup_routed_t** out);
int mgx_sortdedup_routed_shard(const mgx_sortdedup_routed_t* routed, uint32_t k, mgx_sortdedup_shard_t* out);
void mgx_sortdedup_routed_free(mgx_sortdedup_routed_t* routed);
/* Device side: upload one shard.  After mgx_sortdedup_run, mgx_sortdedup_results returns
 *   out_order[n_order]  global arrival indices of the shard's records in output order
 *   out_dup[n_mark]     duplicate flag of every marking record (index into mark_recs / mark_arrival) */
int mgx_sortdedup_upload_shard(mgx_sortdedup_t* ctx, uint64_t L, const mgx_sortdedup_shard_t* shard);
/* Host side: shard k's results into the global arrays (out_order[n_records], out_dup[n_records], zero-initialised
 * by the caller; either may be NULL). */
int mgx_sortdedup_merge(const mgx_sortdedup_routed_t* routed, uint32_t k, const uint32_t* shard_order, const uint8_t* shard_dup,
                        uint32_t* out_order, uint8_t* out_dup);

#ifdef __cplusplus
}
#endif
#endif /* MGX_SORTDEDUP_H */
