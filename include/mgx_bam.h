/*
 * mgx_bam.h -- C ABI of BAM input (libmgx.so): the header, where the alignment records of inflated BAM bytes start, and
 * the sort / duplicate keys of every record, on the host and on the MI355X.
 *
 * Inflated BAM (SAMv1 4.2) is a header followed by a chain of length-prefixed records: record i + 1 starts at
 * r_i + 4 + block_size(r_i).  The host functions walk that chain and derive keys serially; they are the definition.
 * The device functions find the same record starts with one wavefront per tile of bytes (a guessed entry per tile,
 * verified against the exit of the tile before it, re-walked where the guess was wrong: the result never depends on a
 * guess) and derive the same keys, behind the inflate kernel of an mgx_bgzf_t context (mgx_bgzf.h), whose output they
 * read in device memory.
 *
 * All functions return 0 or a negative errno-style code; mgx_last_error() has the message.
 */
#ifndef MGX_BAM_H
#define MGX_BAM_H

#include <stdint.h>

#include "mgx_bgzf.h"
#include "mgx_sortdedup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_BAM_MAX_RECORD (1 << 28)   /* the largest block_size accepted */
#define MGX_BAM_PARTIAL 1              /* mgx_bam_parse_header: the bytes end inside the header, more are needed */

/* What sorting and duplicate marking need of one record: 32 bytes. */
typedef struct mgx_bam_key {
    int64_t d5;                  /* prime5 - coord: what unclipped_five_prime() adds to coord (0 without CIGAR) */
    int32_t tid, pos, end;       /* end: pos + max(1, reference length of the CIGAR) */
    uint16_t flag, score, tile, x, y;
    uint8_t same_qname;          /* read name (without NUL) equals the previous record's; 0 for the first record of a call */
    uint8_t redo;                /* non-zero: the device rule set declined the record, mgx_bam_keys_redo derives it:
                                  * bit 0 a tile / x / y token is not 1-18 plain digits, bit 1 the CIGAR has the shape of
                                  * the long-CIGAR placeholder (<l_seq>S <n>N) */
} mgx_bam_key_t;

/* ---- host side (no device call) ---- */
typedef struct mgx_bam_header {
    uint64_t first;              /* offset of the first alignment record */
    uint64_t text_off, text_len; /* the header text inside data, verbatim, trailing NULs dropped */
    uint32_t n_ref;
    uint32_t pad_;
} mgx_bam_header_t;
/* Reads magic, l_text, text, n_ref and the reference list of data[0, n).  The first min(n_ref, max_ref) references go to
 * name_off / name_len (the name inside data, without its NUL) and ref_len; the three may be NULL with max_ref 0.
 * Returns 0, MGX_BAM_PARTIAL when n cuts the header (*hdr is then not filled), -EILSEQ for a bad magic or an impossible
 * length. */
int mgx_bam_parse_header(const uint8_t* data, uint64_t n, mgx_bam_header_t* hdr, uint32_t max_ref, uint64_t* name_off,
                         uint32_t* name_len, uint32_t* ref_len);

/* The serial chain walk: r_0 = first, r_{i+1} = r_i + 4 + block_size(r_i); a record counts when r_i + 4 + block_size <= n.
 * *next = the first r_i that does not count (it may be >= n; first >= n gives no record and *next = first).
 * rec_off may be NULL (count only); with rec_off, more than max_records records are -E2BIG.  A counted record that is
 * invalid is -EBADMSG, the message names its offset and the rule it broke, *n_records counts the records before it and
 * *next is its offset. */
int mgx_bam_walk_host(const uint8_t* data, uint64_t n, uint64_t first, uint64_t max_records, uint64_t* rec_off,
                      uint64_t* n_records, uint64_t* next);
/* Keys of the valid records at rec_off[0, n_records), complete: nothing is left to redo.  A record whose CIGAR has the
 * placeholder shape and which carries a CG:B,I tag is -ENOTSUP (long CIGARs are not read). */
int mgx_bam_keys_host(const uint8_t* data, const uint64_t* rec_off, uint64_t n_records, mgx_bam_key_t* keys);
/* The keys as the rule set shared with the device gives them, redo bits left set: what the device keys must equal. */
int mgx_bam_keys_rules(const uint8_t* data, const uint64_t* rec_off, uint64_t n_records, mgx_bam_key_t* keys);
/* Completes device-made keys in place: every key with redo set is derived again by the host rules, redo is cleared. */
int mgx_bam_keys_redo(const uint8_t* data, const uint64_t* rec_off, uint64_t n_records, mgx_bam_key_t* keys);
/* mgx_sortdedup_pack for a caller that holds keys: the same ignorable rule, mate search, arrival order and threading;
 * name equality is the chained same_qname bits, coord = sum of target_len before tid + pos (L for tid < 0),
 * prime5 = coord + d5.  Keys with redo set and tid >= n_targets are -EINVAL. */
int mgx_bam_pack_keys(uint64_t n, const mgx_bam_key_t* keys, uint32_t n_targets, const uint64_t* target_len,
                      mgx_rec_t* out_recs, uint32_t* out_input_index, uint64_t* out_L);

/* ---- device side ---- */
typedef struct mgx_bam_batch mgx_bam_batch_t;
/* A batch reads the device output of `inflate` (submit it after that batch's submit, wait for both), or, with NULL, bytes
 * the caller puts into mgx_bam_batch_input().  byte_capacity bounds n_bytes, max_records the records of one submit,
 * n_ref is the header's (the guesses use it, the result does not depend on it). */
int mgx_bam_batch_create(mgx_bgzf_t* ctx, mgx_bgzf_inflate_t* inflate, uint64_t byte_capacity, uint64_t max_records,
                         int32_t n_ref, mgx_bam_batch_t** out);
void mgx_bam_batch_destroy(mgx_bgzf_t* ctx, mgx_bam_batch_t* b);
uint8_t* mgx_bam_batch_input(mgx_bam_batch_t* b);   /* pinned [byte_capacity]; NULL for a batch attached to an inflate batch */
/* Enqueues index + keys over bytes [0, n_bytes) with the chain starting at first; does not wait. */
int mgx_bam_batch_submit(mgx_bgzf_t* ctx, mgx_bam_batch_t* b, uint64_t n_bytes, uint64_t first);
/* Waits.  rec_off / keys: pinned, owned by the batch, valid until its next submit.  Results equal mgx_bam_walk_host's;
 * keys may have redo set.  -EBADMSG as mgx_bam_walk_host, -E2BIG for more than max_records; the context stays usable. */
int mgx_bam_batch_wait(mgx_bgzf_t* ctx, mgx_bam_batch_t* b, const uint64_t** rec_off, const mgx_bam_key_t** keys,
                       uint64_t* n_records, uint64_t* next);
/* One shot over pageable memory; rec_off / keys hold max_records entries. */
int mgx_bam_scan(mgx_bgzf_t* ctx, const uint8_t* data, uint64_t n, uint64_t first, int32_t n_ref, uint64_t max_records,
                 uint64_t* rec_off, mgx_bam_key_t* keys, uint64_t* n_records, uint64_t* next);

typedef struct mgx_bam_stats {       /* the last batch waited for */
    uint64_t n_tiles;                /* tiles of MGX_BAM_TILE bytes (environment; a power of two, 256 to 32768) */
    uint64_t n_tiles_rewalked;       /* ... walked again from their true entry: the guess was wrong or there was none to make */
    uint64_t n_redo;                 /* keys with redo set */
    uint32_t n_rounds;               /* stitch passes that found something to re-walk, + 1 if the serial finish ran */
    float ms_index, ms_keys;         /* HIP events: record starts (all phases), keys */
} mgx_bam_stats_t;
int mgx_bam_stats(mgx_bgzf_t* ctx, mgx_bam_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MGX_BAM_H */
