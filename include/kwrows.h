/*
 * kwrows.h — C-ABI of the per-ticker match cells built on the GPU (libkwmatch.so,
 * advanced_scrapper_amd/csrc/kwrows.hip).
 *
 * What it replaces.  The reference assembles, per article, the dict
 *     ticker_matches[ticker] = {'text': {name: [pos, ...]}, 'title': {...}}   match_keywords.py:159-187
 * and writes json.dumps of the two inner dicts into the ticker's CSV (:137-138).
 * kw_rows_run turns hit records that are already in device memory (kw_hits'
 * pointer, or any caller buffer of kw_hit) into those rows: one row per
 * (article, ticker) in article order then KB ticker order, each with its
 * text_matches and title_matches JSON text exactly as json.dumps writes it.
 *
 * Rules: a (document, field, pattern) group matches ticker t iff one of the
 * pattern's occurrences for t has lo <= date <= hi (both inclusive); the name's
 * place inside t's dict is the rank of the first such occurrence in table order;
 * names stand in rank order, positions ascending; a record with pos == KW_NOPOS
 * adds no number (a group of only such records prints "[]").  Documents with
 * date_ok == 0 and records with doc >= n_docs give nothing.
 *
 * The CSV rows.  kw_rows_cells + kw_rows_emit go on from there to the finished lines of the per-ticker files
 * (the reference's append_to_csv, match_keywords.py:128-146) without the JSON text reaching the host: the rows
 * in the stable order by KB ticker index (article order kept within a ticker), each
 *     decimal(time_unix),date_time,text_matches,title_matches,title,url,source,source_url,article_text\n
 * byte for byte what kwcsv_emit_mt (csrc/kwcsv.c) writes: every cell in the csv writer's QUOTE_MINIMAL form
 * (wrapped in '"' iff it is non-empty and holds ',', '"' or '\n', every '"' inside then doubled; a lone '\r' does
 * not quote), an NA cell (flag bit 2 of the tokenized cells) empty whatever its bytes are, the stamp a signed
 * decimal int64.  Per row a uint32 of flags: bit c (c = 0 date_time, 3..7 title .. article_text) = that cell is a
 * text witness (not NA, and no number or bool literal: blanks only, or a byte other than 0-9 + - . e E, and
 * not true / false / [+-]inf / [+-]infinity in any case, blanks at both ends dropped); bits 1 and 2 always set
 * (the JSON cells); bit 8 + c = that cell is NA; bit 16 = a written cell holds '\r'.
 *
 * Conventions as kwmatch.h: 0 or a negative KW_E* code; kw_rows_last_error gives
 * the message; one handle per device and host thread.
 */
#ifndef KWROWS_H
#define KWROWS_H

#include <stdint.h>

#include "kwmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kw_rows kw_rows;

/* verdicts of kw_rows_run */
#define KW_ROWS_OK 0
#define KW_ROWS_INVALID_REGEX 1   /* an in-period match of a pattern with invalid_rx set: the run has no
                                     rows (the reference's re.finditer raises re.error there, :178/:180) */

/* Upload one knowledge base's tables to `device` (host arrays, copied).
 *   occ_off[n_patterns + 1]  CSR over patterns of the occurrence table, in the reference's traversal order
 *   occ_ti / occ_rank        per occurrence: KB ticker index (0 <= ti < n_tickers), traversal rank
 *   occ_lo / occ_hi          per occurrence: period bounds in epoch microseconds, open = INT64_MIN / INT64_MAX
 *   invalid_rx[n_patterns]   1: the name's regex does not compile
 *   keys / key_off           json.dumps(name) of pattern p = keys[key_off[p]:key_off[p + 1]] (quotes included) */
int kw_rows_create(int32_t device, const int64_t *occ_off, const int32_t *occ_ti, const int32_t *occ_rank,
                   const int64_t *occ_lo, const int64_t *occ_hi, const uint8_t *invalid_rx, const uint8_t *keys,
                   const int64_t *key_off, int32_t n_patterns, int32_t n_tickers, kw_rows **out);

/* Build the rows of n_hits device records (any order; n_hits < 2^31; d_hits 16-byte aligned, as kw_hits'
 * pointer and any device allocation are) over n_docs documents.  date_us /
 * date_ok: host arrays, per document the article date in epoch microseconds and whether it exists.
 * Returns after the device finished: *n_rows rows and *n_bytes of JSON text are then held by the handle
 * (both 0 when *verdict is KW_ROWS_INVALID_REGEX).  stream: a hipStream_t (NULL = default stream); the
 * records must be complete on it.  A pattern index >= n_patterns in a counted record is KW_EINVAL. */
int kw_rows_run(kw_rows *r, const kw_hit *d_hits, int64_t n_hits, const int64_t *date_us, const uint8_t *date_ok,
                int64_t n_docs, int64_t *n_rows, int64_t *n_bytes, int32_t *verdict, void *stream);

/* Copy the last run's result into host buffers: row_doc[n_rows], row_ti[n_rows] (KB ticker index),
 * json[n_bytes], json_off[2 * n_rows + 1] (row r: text_matches = json[off[2r]:off[2r+1]], title_matches =
 * json[off[2r+1]:off[2r+2]]; json_off[0] = 0 also for an empty result). */
int kw_rows_copy(kw_rows *r, int32_t *row_doc, int32_t *row_ti, uint8_t *json, int64_t *json_off);

/* Device times (ms) of the last run, up to 4 values: [0] order (count, scan, scatter and sort of the
 * records), [1] expand (groups -> entries and their order), [2] render (byte lengths, scans, fill), [3] all. */
int kw_rows_last_ms(kw_rows *r, float *ms, int32_t n);

/* The last run's row index alone: row_doc[n_rows], row_ti[n_rows] (what kw_rows_copy gives, without the text). */
int kw_rows_copy_index(kw_rows *r, int32_t *row_doc, int32_t *row_ti);

/* verdicts of kw_rows_emit */
#define KW_EMIT_OK 0
#define KW_EMIT_NUL 1   /* a NUL byte in a non-NA cell of an article that has a rendered row (or in a JSON cell):
                           no output; the csv writer raises there, the caller takes its per-row path */

/* Upload one chunk's tokenized cells (host arrays, copied before the call returns; device buffers kept across
 * chunks): cell c of document d is cells[coff[d * ncols + c], coff[d * ncols + c + 1]) with flags
 * cfl[d * ncols + c]; coff has n_docs * ncols + 1 non-decreasing entries from coff[0] >= 0 (KW_EINVAL
 * otherwise).  Before or after kw_rows_run. */
int kw_rows_cells(kw_rows *r, const uint8_t *cells, const int64_t *coff, const uint8_t *cfl, int64_t n_docs,
                  int32_t ncols, void *stream);

/* kw_rows_cells on cells that are already in device memory (kw_ingest_cells' buffers, kwingest.h): nothing is
 * copied, the handle borrows the three buffers, which must stay valid and unchanged through the next
 * kw_rows_emit.  The same layout and the same checks (the offsets are checked on the device; the call returns
 * after that check). */
int kw_rows_cells_device(kw_rows *r, const uint8_t *d_cells, const int64_t *d_coff, const uint8_t *d_cfl,
                         int64_t n_docs, int32_t ncols, void *stream);

/* Render the first n_rows_use rows (in kw_rows_run's document order: any prefix, 0 included) of the last run.
 * cols[6]: the cells' columns of date_time, title, url, source, source_url, article_text; stamp_by_doc: host
 * int64[n_docs], each document's time_unix.  Returns after the lines are in the handle's pinned host buffers:
 * *n_out_bytes of them (0 when *verdict is KW_EMIT_NUL).  KW_EINVAL, before anything is launched: a null
 * pointer, a column outside [0, ncols), n_rows_use outside [0, n_rows].  KW_ESTATE: no kw_rows_run that
 * succeeded with KW_ROWS_OK, no kw_rows_cells, or their n_docs differ from this one. */
int kw_rows_emit(kw_rows *r, const int32_t *cols, const int64_t *stamp_by_doc, int64_t n_docs, int64_t n_rows_use,
                 int64_t *n_out_bytes, int32_t *verdict, void *stream);

/* kw_rows_emit with the per-document stamps already in device memory: d_stamp_by_doc, device int64[n_docs] (e.g.
 * kw_ingest_stamps_device's, kwingest.h), borrowed through the call and complete on `stream`.  No host array is
 * uploaded; the same checks, verdicts and result buffers as kw_rows_emit. */
int kw_rows_emit_stamps_device(kw_rows *r, const int32_t *cols, const int64_t *d_stamp_by_doc, int64_t n_docs,
                               int64_t n_rows_use, int64_t *n_out_bytes, int32_t *verdict, void *stream);

/* The last emit's result in pinned host memory owned by the handle, valid until the next kw_rows_emit or
 * kw_rows_destroy: n = n_rows_use rows (0 after KW_EMIT_NUL) in output order; row i's line is
 * out[line_off[i], line_off[i + 1]) (line_off[0] = 0 always), flags[i] as above, row_doc / row_ti / stamps[i] its
 * document, KB ticker index and time_unix. */
int kw_rows_emit_result(kw_rows *r, const uint8_t **out, const int64_t **line_off, const uint32_t **flags,
                        const int32_t **row_doc, const int32_t **row_ti, const int64_t **stamps);

/* Device times (ms) of the last emit, up to 4 values: [0] order (the rows by ticker), [1] measure (cell and line
 * lengths, flags, scans), [2] fill (cells into scratch, lines), [3] the copy to the pinned buffers. */
int kw_rows_emit_last_ms(kw_rows *r, float *ms, int32_t n);

const char *kw_rows_last_error(kw_rows *r);
int kw_rows_destroy(kw_rows *r);

#ifdef __cplusplus
}
#endif
#endif
