/*
 * kwsort.h — C-ABI of the output sort on the GPU (libkwmatch.so, advanced_scrapper_amd/csrc/kwsort.hip).
 *
 * What it replaces.  sort_matched_csv re-reads a per-ticker CSV file, sorts it by `time_unix` and writes it again
 * (reference match_keywords.py:195-217).  The host route (match_keywords._sort_native) tokenizes the file and
 * then slices, converts and joins it row by row in Python.  Here the file's body is parsed by kw_ingest_parse
 * (kwingest.h), kw_sort_keys reads the keys and decides whether the rewrite is provably a permutation of the
 * file's own records, the host makes pandas' own np.argsort(kind='quicksort') call on the keys (its order among
 * equal keys cannot be reproduced by another sort), and kw_sort_gather lays the records out in that order.  No
 * cell is rendered: a file that would need it is refused and stays with the host routes.
 *
 * The take rule (restated in tests/sort_rule.py).  Over the rows of an OK final parse that consumed
 * the whole text, the verdict is the first of these conditions, in this order, that has an offender:
 *   KW_SORT_KEY    a row whose time_unix cell is NA or QUOTED, or is not the canonical decimal form `0` or
 *                  `-?[1-9][0-9]*` (so `-0`, `+1`, `01`, ` 1`, `1.0`, `1e3` and the empty cell offend), or whose
 *                  value lies outside int64.  bad_row: the first such row; bad_col: the time_unix column.
 *   KW_SORT_FORM   a row with a cell that lacks KWCSV_CANON, or an NA cell of non-zero length (an unquoted empty
 *                  cell is NA and CANON and passes: pandas writes NaN back as the empty cell).  bad_row: the first
 *                  such row; bad_col: its first such cell.
 *   KW_SORT_DTYPE  over the blocks of block_rows consecutive rows (the last one shorter): a column other than
 *                  time_unix in which no cell of the block carries KWCSV_TEXT and not every cell of it is NA
 *                  (pandas infers a column's type block by block and would render such a block's cells again).
 *                  bad_row: the block's first row, of the first such block; bad_col: its lowest such column.
 * A row that passes is written by pandas byte for byte as it stands in the file, with "\n" as its terminator.
 *
 * A file of any size.  kw_ingest_parse takes less than 2^31 bytes, and kw_sort_gather lays out less than 2^31.
 * A larger body -- or any body the caller wants staged in pieces -- is parsed in windows (final == 0, the
 * unconsumed tail opens the next window): kw_sort_begin reserves a store in device memory, kw_sort_window appends
 * each parsed window's text and spans to it and works its rows at their global row numbers (a block's witnesses
 * may lie in another window than its numeric cells; the ascending test carries the last key over a window's
 * edge, and equal keys there are not ascending), and kw_sort_finish gives the whole file's verdict: exactly what
 * kw_sort_keys gives on the same body parsed as one text.  kw_sort_gather_begin then scans an order of any total
 * size with 64-bit offsets, and kw_sort_gather_slab hands the output over one slab at a time through two pinned
 * host slabs; a record, its '\n' and a lane's 16-byte store may straddle a slab's edge at any phase.  Two limits
 * remain: a single record of 2^31 - 2^20 bytes or more (no window holds it), and a body larger than the device's
 * free memory (kw_sort_begin: KW_EOVERFLOW).
 *
 * Conventions as kwingest.h: 0 or a negative KW_E* code; kw_sort_last_error gives the message; one handle per
 * device and host thread.  The kw_ingest handle's parse, and the text it parsed, must stand from kw_sort_keys
 * until the last kw_sort_gather of that file; after kw_sort_window the handle is free at once.
 */
#ifndef KWSORT_H
#define KWSORT_H

#include <stdint.h>

#include "kwingest.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kw_sort kw_sort;

/* verdicts of kw_sort_keys, in the order the conditions are tested */
#define KW_SORT_OK 0
#define KW_SORT_KEY 1
#define KW_SORT_FORM 2
#define KW_SORT_DTYPE 3

int kw_sort_create(int32_t device, kw_sort **out);

/* The keys and the verdict of the rows of ig's last parse (OK, final, the whole text consumed; at least one row).
 * time_col: the time_unix column; block_rows >= 1.  Returns after the device finished: *verdict, for another
 * verdict than KW_SORT_OK *bad_row and *bad_col, and for KW_SORT_OK *keys (n_rows int64 in a pinned host buffer
 * of the handle, valid until the next kw_sort_keys), *body_bytes (the bytes of the body that holds every row
 * once: each record's bytes + 1) and *ascending (1: the keys increase strictly from row to row, the rows are in
 * order as they stand).  stream: the parse's stream. */
int kw_sort_keys(kw_sort *h, kw_ingest *ig, int32_t time_col, int64_t block_rows, const int64_t **keys,
                 int64_t *n_rows, int64_t *body_bytes, int32_t *verdict, int64_t *bad_row, int32_t *bad_col,
                 int32_t *ascending, void *stream);

/* After a kw_sort_keys with the verdict KW_SORT_OK: the body whose record j is the text's record order[j] followed
 * by "\n", j = 0 .. n - 1 (order: a host array; 1 <= n <= n_rows of the parse; an entry may repeat).  Every
 * entry is checked on the device before anything is copied: one outside [0, n_rows) gives KW_EINVAL, a body of
 * 2^31 bytes or more KW_EOVERFLOW, and neither writes the output buffer.  *out: a pinned host buffer of the
 * handle holding *out_bytes bytes, valid until the next kw_sort_gather. */
int kw_sort_gather(kw_sort *h, const int64_t *order, int64_t n, const uint8_t **out, int64_t *out_bytes);

/* ---- a file of several windows -------------------------------------------------------------------------------
 * Start a file whose body is parsed window by window: time_col and block_rows as kw_sort_keys; expect_bytes >= 1:
 * the bytes of body text the windows will hand over at most.  Reserves the store for them (a store the handle
 * already has is kept when it is large enough) and resets what the windows accumulate.  KW_EOVERFLOW, with
 * nothing allocated: the store, a quarter of it again for what is kept per row, and 64 MiB do not fit in the
 * device's free memory (hipMemGetInfo), or expect_bytes exceeds the tests' KW_TEST_SORT_STORE_MAX. */
int kw_sort_begin(kw_sort *h, int32_t time_col, int64_t block_rows, int64_t expect_bytes);

/* After an OK kw_ingest_parse of the file's next window (final or not; at least one row; every window's handle
 * has the same ncols): bytes [0, consumed) of the parse's text -- consumed as the parse gave it -- go to the end
 * of the store, the rows' spans with them, and the rows' keys, conditions and witnesses to their global rows.
 * Returns after the device finished: the ingest handle may then take the next window.  KW_EOVERFLOW: more bytes
 * than kw_sort_begin was told.  An error ends the file. */
int kw_sort_window(kw_sort *h, kw_ingest *ig, int64_t consumed, void *stream);

/* After the last window: the outputs of kw_sort_keys, over all the windows' rows as one text (*body_bytes: the
 * sum over the windows).  With the verdict KW_SORT_OK the store stands for kw_sort_gather_begin, or for
 * kw_sort_gather where the body stays under 2^31 bytes, until the next kw_sort_begin or kw_sort_keys. */
int kw_sort_finish(kw_sort *h, const int64_t **keys, int64_t *n_rows, int64_t *body_bytes, int32_t *verdict,
                   int64_t *bad_row, int32_t *bad_col, int32_t *ascending);

/* ---- a file described by its write index ---------------------------------------------------------------------
 * A run that wrote a file itself holds every record's length (egress.RunFiles) and has decided on the host that
 * the sorted file is a permutation of the written records: such a body needs no parse and no take rule, only the
 * records' places.  This route ends in the state a taken kw_sort_finish leaves -- the body in the store, the
 * records' spans, n_rows -- so kw_sort_gather, kw_sort_gather_begin and kw_sort_gather_slab follow it unchanged.
 * It needs no kw_ingest handle: the body comes through two pinned staging slots of the sort handle.
 *
 * kw_sort_index_begin: lens[i] >= 1 is record i's bytes in the body, its terminator included (a host array of
 * n_rows >= 1 entries); body_bytes >= 1 their sum.  Reserves the store by kw_sort_begin's rule (KW_EOVERFLOW as
 * there, nothing allocated), uploads lens and computes on the device, from their 64-bit exclusive scan, the spans
 * rs[i] = the bytes before record i and re[i] = rs[i] + lens[i] - 1, the place of the terminator (which the copy
 * kernel writes itself).  KW_EINVAL, with *bad_row and the message naming the row: the first row whose length is
 * below 1 or which ends beyond body_bytes; n_rows when the lengths end before body_bytes.  Returns after the
 * device finished. */
#define KW_INDEX_OK 0
#define KW_INDEX_TERM 1
int kw_sort_index_begin(kw_sort *h, const int64_t *lens, int64_t n_rows, int64_t body_bytes, int64_t *bad_row);

/* *host: staging slot `slot` (0 or 1), pinned, of n_bytes at least (a slot that grows does not keep its
 * contents).  Waits for the slot's last kw_sort_index_window copy first: the caller may fill the slot when the
 * call returns, from any thread.  Valid until the next call for that slot with a larger size, or the destroy. */
int kw_sort_index_stage(kw_sort *h, int32_t slot, int64_t n_bytes, uint8_t **host);

/* The slot's first n_bytes go to the store, behind the bytes the windows before gave.  A window ends anywhere, in
 * the middle of a record too: nothing is parsed.  The copy is asynchronous on `stream`: the other slot may be
 * filled meanwhile, and kw_sort_index_stage for this slot waits for it.  KW_EOVERFLOW: more bytes than
 * body_bytes.  An error ends the file. */
int kw_sort_index_window(kw_sort *h, int32_t slot, int64_t n_bytes, void *stream);

/* After the last window.  KW_ESTATE: the windows gave another number of bytes than body_bytes.  Else, one lane a
 * record, the store's byte at re[i] must be '\n': *verdict is KW_INDEX_OK, and the handle stands as after a taken
 * kw_sort_finish; or KW_INDEX_TERM with *bad_row the first record that does not end so -- the index does not
 * describe the file, a refusal and no error, after which no gather is possible (KW_ESTATE).  Returns after the
 * device finished.  kw_sort_last_ms: the spans and this check under [0] keys, lens and the windows under [3]
 * copies. */
int kw_sort_index_finish(kw_sort *h, int32_t *verdict, int64_t *bad_row);

/* ---- the output in slabs -------------------------------------------------------------------------------------
 * After a taken kw_sort_keys or kw_sort_finish: kw_sort_gather's range check, lengths and scan for `order`
 * (n entries), and nothing copied.  slab_bytes: a positive multiple of 1024, below 2^31.  *total_bytes: the
 * body's bytes, of any size; *n_slabs: ceil(total / slab_bytes).  KW_EINVAL for an order entry outside
 * [0, n_rows): no slab can then be fetched. */
int kw_sort_gather_begin(kw_sort *h, const int64_t *order, int64_t n, int64_t slab_bytes, int64_t *total_bytes,
                         int64_t *n_slabs);

/* Bytes [k * slab_bytes, min((k + 1) * slab_bytes, total)) of that body, 0 <= k < n_slabs in any order: *out is
 * one of two pinned host slabs of the handle, in turn, holding *out_bytes bytes, valid until the next
 * kw_sort_gather_slab.  Before it returns the call starts slab k + 1 into the other slab: asked for next, it is
 * laid out and copied while the caller writes slab k away. */
int kw_sort_gather_slab(kw_sort *h, int64_t k, const uint8_t **out, int64_t *out_bytes);

/* Device times (ms) of the last kw_sort_keys and kw_sort_gather, or summed over a file's windows and slabs, up to
 * 4 values: [0] keys (the rows' keys and conditions), [1] scan (the order's range check, the records' lengths and
 * their scan), [2] gather (the copy kernel), [3] copies (the text into the store, the order to the device, the
 * keys and the body to the host). */
int kw_sort_last_ms(kw_sort *h, float *ms, int32_t n);

const char *kw_sort_last_error(kw_sort *h);
int kw_sort_destroy(kw_sort *h);

#ifdef __cplusplus
}
#endif
#endif
