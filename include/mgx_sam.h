/*
 * mgx_sam.h -- C ABI of SAM text input (libmgx.so): the alignment lines of SAM text as BAM alignment records
 * (block_size + record, SAMv1 4.2) with the sort / duplicate key of every line, on the host and on the MI355X
 * (DESIGN.md 4.9).
 *
 * Lines end at '\n', one trailing '\r' is dropped, empty lines are skipped, the last line may lack its newline.  One
 * rule set (csrc/sam_line_core.h) encodes a line or DECLINES it: a declined line has no bytes (rec_off[i + 1] ==
 * rec_off[i]) and bit 2 of its key's redo set, and is left to a full SAM parser.  The list of what is declined is in
 * that header; ordinary lines are not on it.  mgx_sam_encode_rules is the rule set on the host and the definition of
 * what the device gives; mgx_sam_encode_host completes the declined lines and is what a caller finally holds.
 *
 * All functions return 0 or a negative errno-style code; mgx_last_error() has the message.
 */
#ifndef MGX_SAM_H
#define MGX_SAM_H

#include <stdint.h>

#include "mgx_bam.h"
#include "mgx_bgzf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_SAM_MAX_LINE 2048          /* the longest line the device encodes: longer ones are declined */
#define MGX_SAM_REDO_DECLINED 4        /* mgx_bam_key_t.redo bit 2: the line was declined (bits 0, 1: see mgx_bam.h) */
/* the bytes of BAM that n_lines lines of n_text bytes can become: 36 per line + 2 per byte of text */
#define MGX_SAM_OUT_BOUND(n_lines, n_text) (36ull * (n_lines) + 2ull * (n_text))

/* ---- reference names of the header -> lookup table (the lowest index among equal names, as a serial search finds) ---- */
typedef struct mgx_sam_table mgx_sam_table_t;
/* names: the n_ref names back to back, name i = names[name_off[i], name_off[i + 1]).  The lengths of the references are
 * not needed to encode a record and are not taken. */
int mgx_sam_table_create(uint32_t n_ref, const uint8_t* names, const uint32_t* name_off, mgx_sam_table_t** out);
void mgx_sam_table_destroy(mgx_sam_table_t* t);

/* ---- host side (no device call) ---- */
/* Starts and lengths (newline and trailing CR not counted) of the non-empty lines of text[0, n).  line_off / line_len may
 * be NULL (count only); with them, more than max_lines lines are -E2BIG. */
int mgx_sam_lines_host(const uint8_t* text, uint64_t n, uint64_t max_lines, uint64_t* line_off, uint32_t* line_len,
                       uint64_t* n_lines);
/* The rule set over every line.  max_line: longer lines are declined (0 = MGX_SAM_MAX_LINE, what the device uses).
 * rec_off has max_lines + 1 entries: line i's record is out[rec_off[i], rec_off[i + 1]), empty when declined;
 * *n_out = rec_off[n_lines].  keys[i]: mgx_bam_keys_rules' key of the record, same_qname taken from the TEXT (QNAME equals
 * that of the line before, declined or not; 0 for the first line); a declined line's key is zero but for same_qname
 * and redo = MGX_SAM_REDO_DECLINED.  keys and out may be NULL (sizes only).  -E2BIG: more than max_lines lines, or more
 * than out_capacity bytes. */
int mgx_sam_encode_rules(const mgx_sam_table_t* table, const uint8_t* text, uint64_t n, uint32_t max_line, uint64_t max_lines,
                         uint64_t out_capacity, uint64_t* line_off, uint32_t* line_len, uint64_t* rec_off, mgx_bam_key_t* keys,
                         uint8_t* out, uint64_t* n_lines, uint64_t* n_out, uint64_t* n_declined);
/* The same with every declined line encoded by the full SAM parser of the command-line tool (and bit 2 of its key
 * cleared): the bytes are those of that parser for every line.  A line it rejects is -EBADMSG: *bad_line is the line's
 * index and the message is the parser's, followed by " at: " and the first 80 bytes of the line. */
int mgx_sam_encode_host(const mgx_sam_table_t* table, const uint8_t* text, uint64_t n, uint64_t max_lines, uint64_t out_capacity,
                        uint64_t* line_off, uint32_t* line_len, uint64_t* rec_off, mgx_bam_key_t* keys, uint8_t* out,
                        uint64_t* n_lines, uint64_t* n_out, uint64_t* n_declined, uint64_t* bad_line);

/* ---- device side ---- */
typedef struct mgx_sam_batch mgx_sam_batch_t;
/* A batch hangs off a BGZF context (its device) and runs on a stream of its own, so that the batches of several parser
 * threads do not wait for each other.  It keeps a device copy of the table.  text_capacity bounds n_bytes, max_records the
 * lines of one submit; the device buffer for the records holds MGX_SAM_OUT_BOUND(max_records, text_capacity) bytes. */
int mgx_sam_batch_create(mgx_bgzf_t* ctx, const mgx_sam_table_t* table, uint64_t text_capacity, uint64_t max_records,
                         mgx_sam_batch_t** out);
void mgx_sam_batch_destroy(mgx_bgzf_t* ctx, mgx_sam_batch_t* b);
uint8_t* mgx_sam_batch_input(mgx_sam_batch_t* b);     /* pinned [text_capacity] */
/* Enqueues the upload and the kernels over text [0, n_bytes); does not wait. */
int mgx_sam_batch_submit(mgx_bgzf_t* ctx, mgx_sam_batch_t* b, uint64_t n_bytes);
/* Waits.  line_off / line_len / rec_off (n_lines + 1 entries) / keys: pinned, owned by the batch, valid until its next
 * submit, equal to mgx_sam_encode_rules'.  bam: NULL leaves the records on the device; otherwise *bam is a pinned copy of
 * the *n_bytes_out bytes.  -E2BIG for more than max_records lines; the batch and the context stay usable. */
int mgx_sam_batch_wait(mgx_bgzf_t* ctx, mgx_sam_batch_t* b, const uint64_t** line_off, const uint32_t** line_len,
                       const uint64_t** rec_off, const mgx_bam_key_t** keys, uint64_t* n_lines, uint64_t* n_bytes_out,
                       const uint8_t** bam);
/* Device address of the encoded stream of the last submit, valid until the next one. */
uint64_t mgx_sam_batch_device_records(mgx_sam_batch_t* b);
/* One shot over pageable memory; the arrays as in mgx_sam_encode_rules. */
int mgx_sam_encode(mgx_bgzf_t* ctx, const mgx_sam_table_t* table, const uint8_t* text, uint64_t n, uint64_t max_lines,
                   uint64_t out_capacity, uint64_t* line_off, uint32_t* line_len, uint64_t* rec_off, mgx_bam_key_t* keys, uint8_t* out,
                   uint64_t* n_lines, uint64_t* n_out, uint64_t* n_declined);

typedef struct mgx_sam_stats {        /* the last batch waited for */
    uint64_t n_lines, n_declined, bytes_in, bytes_out;
    uint64_t n_tiles;                 /* tiles of MGX_SAM_TILE bytes of the line finder (environment; a power of two, 256 to 32768) */
    float ms_lines, ms_encode, ms_keys; /* HIP events: line finder | size + scan + encode | keys */
} mgx_sam_stats_t;
int mgx_sam_stats(mgx_bgzf_t* ctx, mgx_sam_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MGX_SAM_H */
