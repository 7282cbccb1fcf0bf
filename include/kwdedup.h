/* libkwmatch — CDX link-row normalise + keep-first dedup on the GPU (gfx950).
 *
 * Replaces the pandas steps of the reference's link harvester
 * (lwowlwowl/advanced_scrapper yahoo_links_selenium.py):
 *
 *   :63       df[df['url'].str.contains('.html')]                  (regex: any code point but '\n', then "html")
 *   :66       df['url'].str.split('.html').str[0] + '.html'        (cut before the first such match)
 *   :67       .str.replace(':80', '', regex=False)
 *   :68       .str.replace('http:', 'https:', regex=False)
 *   :75-76    drop rows containing 'news/%' or "news/'"
 *   :79, :174 drop_duplicates(subset=['url']) keep='first'           (per part, then over the glob-ordered concat)
 *
 * Keep-first over the concatenation of the parts equals the per-part dedup
 * followed by the merge dedup, so one call over all rows (parts concatenated
 * in glob order) gives the final yfin_urls.csv rows.
 *
 * Rows are UTF-8 URL strings in a caller-owned device arena: row i is
 * d_arena[d_off[i], d_off[i+1]); the arena must be readable 32 bytes past
 * d_off[n].  Every function returns 0 or a negative KW_E* code (kwmatch.h);
 * kw_dedup_last_error gives the message.  A handle is not thread-safe.
 */
#ifndef KWDEDUP_H
#define KWDEDUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-row outcome codes written to d_code */
#define KW_URL_NO_HTML 0      /* dropped by :63 */
#define KW_URL_KEPT 1         /* first occurrence of its normalised URL */
#define KW_URL_FILTERED 2     /* dropped by :75-76 */
#define KW_URL_DUPLICATE 3    /* dropped by :79 / :174 */

typedef struct kw_dedup kw_dedup;

int kw_dedup_create(int32_t device, kw_dedup **out);

/* flags of kw_dedup_run */
#define KW_DEDUP_NORMALIZE 1  /* apply :63-76 before the keep-first; without it the keep-first runs on the raw
                                 strings (the merge step :174 over part CSVs that are already normalised) */

/* Classify n rows; d_code (caller-owned, n bytes) receives one KW_URL_* code per
 * row.  Runs on `stream` (a hipStream_t, NULL = default) and returns when the
 * codes are final (the rare 64-bit hash-tag collisions are resolved by an exact
 * host pass over the colliding rows). */
int kw_dedup_run(kw_dedup *h, const uint8_t *d_arena, const int64_t *d_off, int64_t n, int32_t flags,
                 uint8_t *d_code, void *stream);

/* Row counts per code of the last run: counts[KW_URL_*] (4 values). */
int kw_dedup_counts(kw_dedup *h, int64_t *counts);

/* The kernels' compile-time geometry, for tests that aim at its edges (no handle, no device): out[0..10) =
 * the transform's LDS stage (bytes a wave), the groups of 64 rows a wave claims at once, the rows of a scan tile,
 * the lanes a compared pair takes, the words a lane has in flight per row, the kept rows of a copy task, the copy's
 * input and output stages (bytes), the lane-per-row copy's stage (bytes), the rows the collision list holds;
 * n <= 10 values. */
int kw_dedup_geometry(int32_t *out, int32_t n);

/* Routes of the last run: out[0] rows that took the byte-serial rewrite, [1] compared pairs that differed, [2] rows
 * that shared a hash tag with a different URL (decided by the exact host pass), [3] such rows as the device listed
 * them; n <= 4 values. */
int kw_dedup_route_counts(kw_dedup *h, int64_t *out, int32_t n);

/* Size of the last run's kept rows: their number and the bytes of their normalised URLs. */
int kw_dedup_kept_size(kw_dedup *h, int64_t *n_kept, int64_t *n_bytes);

/* The kept rows, dense and in row order, into caller-owned device buffers:
 * d_bytes (n_bytes), d_off (n_kept + 1 offsets into d_bytes), d_rows (n_kept source row indices). */
int kw_dedup_kept_copy(kw_dedup *h, uint8_t *d_bytes, int64_t *d_off, int64_t *d_rows, void *stream);

/* Device times (ms) of the last run: [0] transform + hash + table insert, [1] the byte-serial rows
 * (rewrite + insert), [2] decide (rep compare), [3] kept compaction, [4] total; k <= 5 values. */
int kw_dedup_last_ms(kw_dedup *h, float *ms, int32_t k);

const char *kw_dedup_last_error(kw_dedup *h);
int kw_dedup_destroy(kw_dedup *h);

/* One-shot form: d_keep_mask[i] = 1 iff row i is kept. */
int dedup_urls(const uint8_t *d_arena, const int64_t *d_off, int64_t n, uint8_t *d_keep_mask, void *stream);

/* ---- CDX listings parsed and the URL CSVs rendered on the device (csrc/cdx.hip) ----
 *
 * Raw listing bytes in, final CSV bytes out: the handle owns a row store (UTF-8 URL arena, int64 offsets, int64
 * timestamps, in the layout kw_dedup_run takes); kw_cdx_append parses one device-resident text into it,
 * kw_cdx_run is kw_dedup_run over the store, kw_cdx_csv_* render the kept rows as the bytes of pandas'
 * DataFrame.to_csv(index=False) over columns date_time,url.
 *
 * A text is taken only where the parse provably equals pandas' ("CDX ingest"); otherwise the
 * verdict names the first failed condition and nothing is appended. */
typedef struct {
    uint8_t delim;         /* the field delimiter: ' ' or ',' */
    int32_t ts_col;        /* 0-based field of the timestamp */
    int32_t url_col;       /* 0-based field of the URL */
    int32_t skip_lines;    /* 0, or 1: the text starts with the line "date_time,url" */
    int32_t exact_fields;  /* 0: at least max(ts_col, url_col) + 1 fields a line; else exactly this many */
} kw_cdx_dialect;
/* CDX listing:  {' ', 1, 2, 0, 0}   read_csv(delimiter=' ', header=None, usecols=[1, 2])   (:59)
 * part CSV:     {',', 0, 1, 1, 2}   read_csv(part) under the header line "date_time,url"    (:164-167) */

/* verdicts of kw_cdx_append, in the order they are tested: the three byte conditions over the whole text
 * (bad_line: the line of the first such byte), the header, then the first offending line (within a line:
 * UTF8, FIELDS, TS, URL).  Lines are counted from 0 by the '\n' bytes before them. */
#define KW_CDX_OK 0
#define KW_CDX_QUOTE 1    /* a '"' byte */
#define KW_CDX_CR 2       /* a '\r' byte */
#define KW_CDX_NUL 3      /* a NUL byte */
#define KW_CDX_FIELDS 4   /* a non-blank line with too few (exact_fields: not exactly that many) fields */
#define KW_CDX_TS 5       /* a timestamp cell that is not 1-18 ASCII digits */
#define KW_CDX_URL 6      /* a URL cell without ':' */
#define KW_CDX_UTF8 7     /* a line that is not valid UTF-8 */
#define KW_CDX_HEADER 8   /* skip_lines = 1 and the text does not start with the line "date_time,url" */

/* Empty the handle's row store (its buffers are kept). */
int kw_cdx_begin(kw_dedup *h);

/* Parse n_bytes of text at d_text (device memory, 16-byte aligned, readable up to the next multiple of 16 past
 * its end) and append its rows to the store; rows of successive appends are numbered consecutively.  Blank
 * lines are dropped; a final line needs no '\n'.  *verdict receives a KW_CDX_* code, *bad_line the offending
 * line (-1 when OK), *n_rows the rows appended (0 unless OK).  Returns when the rows are in the store.
 * KW_EUNSUPPORTED when the store would pass the 2^32 - 1 rows of kw_dedup_run. */
int kw_cdx_append(kw_dedup *h, const uint8_t *d_text, int64_t n_bytes, const kw_cdx_dialect *d, int64_t *n_rows,
                  int32_t *verdict, int64_t *bad_line, void *stream);

/* Rows and URL bytes in the store. */
int kw_cdx_rows(kw_dedup *h, int64_t *n_rows, int64_t *n_bytes);

/* The store's rows into caller-owned device buffers (any may be NULL): d_arena (n_bytes), d_off (n_rows + 1),
 * d_ts (n_rows). */
int kw_cdx_store_copy(kw_dedup *h, uint8_t *d_arena, int64_t *d_off, int64_t *d_ts, void *stream);

/* kw_dedup_run over the store (flags: KW_DEDUP_NORMALIZE); kw_dedup_counts / kept_size / kept_copy then
 * describe this run. */
int kw_cdx_run(kw_dedup *h, int32_t flags, void *stream);

/* The CSV of the last kw_cdx_run's kept rows, in row order: "date_time,url\n", then per row decimal(timestamp),
 * ',', the normalised URL (wrapped in '"' when it contains ','), '\n'.  kw_cdx_csv_size computes the line
 * lengths (on `stream`) and gives the size; kw_cdx_csv_copy writes the bytes to d_out (16-byte aligned, n_bytes
 * of kw_cdx_csv_size) and returns when they are written. */
int kw_cdx_csv_size(kw_dedup *h, int64_t *n_bytes, void *stream);
int kw_cdx_csv_copy(kw_dedup *h, uint8_t *d_out, void *stream);

/* Device times (ms): [0] parse and [1] compaction into the store, both summed over the appends since
 * kw_cdx_begin, [2] the last render (kw_cdx_csv_size + kw_cdx_csv_copy); k <= 3 values. */
int kw_cdx_last_ms(kw_dedup *h, float *ms, int32_t k);

/* The parser's tile: bytes of text a block classifies at once. */
int kw_cdx_tile_bytes(void);

/* ---- the scraper's resume filter (constant_rate_scrapper.py:312-360): quoted CSV in, the links not yet scraped out
 *
 *   scraped  = set(success["url"]) | set(failed["url"])
 *   df_links = df_links[~df_links["url"].isin(scraped)]
 *
 * kw_csv_append parses one device-resident CSV text in pandas' default dialect (',' delimiter, '"' quotes that
 * may hold delimiters, "" pairs and raw line breaks, records ended by '\n' or "\r\n") and appends the cells of one
 * column to the row store of kw_cdx_*.  The success and failed files are appended first, the links file last;
 * kw_cdx_run_exclude then drops every link row whose string is among the rows before it.
 *
 * A text is taken only where the parse provably equals pd.read_csv(text)[column].astype(str) ("Resume
 * filter"; restated in tests/resume_rule.py); otherwise the verdict names the first failed condition, *bad_pos is
 * the byte position of its first offender, and nothing is appended.  The conditions are tested in the order of the
 * codes below, each over the whole text (the numbers in the comments are those of DESIGN.md's list).  Quote state
 * is the parity of the '"' bytes before a byte. */
#define KW_CSV_OK 0
#define KW_CSV_NUL 1      /* 1. a NUL byte (its position) */
#define KW_CSV_UTF8 2     /* 1. the text is not valid UTF-8 (the first byte a strict decoder stops at) */
#define KW_CSV_HEADER 3   /* 2. the text does not start with header_line followed by '\n' or "\r\n" (position 0) */
#define KW_CSV_QUOTE 4    /* 3. an opening '"' that neither starts a field nor follows a '"'; a closing '"' not
                                followed by ',', '\n', '\r', '"' or the end of the text (the quote's position); a text
                                that ends inside quotes (position n_bytes) */
#define KW_CSV_CR 5       /* 4. a '\r' outside quotes that is not followed by '\n' (its position) */
#define KW_CSV_ROWS 6     /* 5. no record after the header, or the store would pass the 2^32 - 1 rows of
                                kw_dedup_run (position n_bytes) */
#define KW_CSV_FIELDS 7   /* 6. a record that is not zero-length and has not exactly n_fields fields (the position
                                of its first byte); records of no bytes but the terminator are skipped */
#define KW_CSV_URL 8      /* 7. a cell of the column that, outer quotes removed, holds no ':', or holds a '"', '\n'
                                or '\r' (the position of its record's first byte) */

/* Parse n_bytes of text at d_text (as kw_cdx_append: 16-byte aligned, readable up to the next multiple of 16 past
 * its end) and append the cells of column url_col (0-based, of n_fields) to the store, outer quotes removed; the
 * rows' timestamps are 0.  header_line: the file's first line without its terminator, NUL-terminated (n_fields
 * names separated by ','; no '"').  *verdict receives a KW_CSV_* code, *bad_pos the offender's byte position (-1 when
 * OK), *n_rows the rows appended (0 unless OK).  Returns when the rows are in the store.  kw_cdx_last_ms [0] and
 * [1] include these appends (event spans that hold the call's host round trips, not kernel time alone). */
int kw_csv_append(kw_dedup *h, const uint8_t *d_text, int64_t n_bytes, const char *header_line, int32_t url_col,
                  int32_t n_fields, int64_t *n_rows, int32_t *verdict, int64_t *bad_pos, void *stream);

/* ---- kw_csv_append window by window: a file of any size through device texts of a fixed size
 *
 * kw_csv_stream_begin takes kw_csv_append's header arguments, notes the store's rows and bytes and sets the stream's
 * file position to 0.  One stream a handle at a time; kw_csv_append and a second begin return KW_ESTATE while one is
 * open, kw_cdx_begin drops it.
 *
 * kw_csv_stream_window parses one window (alignment and readable bytes as kw_csv_append).  The text begins at a record
 * start outside quotes: the first window with the header line, every later one at the byte where the previous
 * window's *consumed ended.  *consumed is the position after the terminator of the last record that ends inside the
 * window, outside quotes (after the last '\n' outside quotes); with final != 0 it is n_bytes, and the end of the text
 * ends a record that has bytes.  A window that is not final and holds no record end gives *consumed = 0, verdict OK and
 * no rows: the caller comes back with more bytes.  So does a first window that is not final and is shorter than the
 * header line plus one terminator byte.
 *
 * Only the bytes before *consumed are judged, by kw_csv_append's conditions in its order, except that
 *   - HEADER is tested in the first window only (the first with *consumed > 0);
 *   - "the text ends inside quotes" is tested at a final window only;
 *   - ROWS is tested against the store's running total; "no record after the header" is kw_csv_stream_end's;
 *   - an offender at or beyond *consumed belongs to the next window (the bytes of a UTF-8 sequence the window cuts, a
 *     '\r' or a closing '"' that is the window's last byte): the first NUL and the first UTF-8 offender of the window
 *     count iff they lie before *consumed;
 *   - *bad_pos is a position in the file: the sum of the *consumed so far plus the offender's position in the window.
 * After a verdict other than OK, a KW_E* code or a final window the stream takes no more windows (KW_ESTATE).
 *
 * kw_csv_stream_end closes the stream.  With commit = 0, or after a window that was refused or failed, the store is
 * put back to the rows and bytes noted by begin and the call returns KW_OK (*n_rows_total = 0).  With commit != 0
 * after OK windows the last of which was final it returns KW_OK and the rows the stream appended, or, when it appended
 * none, the positive code KW_CSV_ROWS (the one-piece call's verdict for "no record after the header"; KW_E* codes are
 * negative, so the return value names it without a verdict parameter).  commit != 0 before a final window: KW_ESTATE,
 * the store put back.
 *
 * For a text cut into windows in this way, at any window sizes: every verdict is OK iff kw_csv_append over the whole
 * text says OK, and the store then holds exactly the same rows (arena bytes, offsets, timestamps 0); for a text with
 * one single offender the code and file position equal the whole-text call's ("Windowed CSV append").
 * kw_cdx_last_ms [0] and [1] go on summing over the windows. */
int kw_csv_stream_begin(kw_dedup *h, const char *header_line, int32_t url_col, int32_t n_fields);
int kw_csv_stream_window(kw_dedup *h, const uint8_t *d_text, int64_t n_bytes, int32_t final, int64_t *consumed,
                         int64_t *n_rows, int32_t *verdict, int64_t *bad_pos, void *stream);
int kw_csv_stream_end(kw_dedup *h, int32_t commit, int64_t *n_rows_total);

/* per-row code of a link row of kw_cdx_run_exclude whose string is among the exclude rows (KW_URL_* above are
 * 0..3; libkwmatch keeps 4 for itself) */
#define KW_URL_SEEN 5

/* The set difference over the store: its first n_exclude rows are the exclude rows, the rest the link rows.  Runs
 * kw_dedup_run over the raw strings (no KW_DEDUP_NORMALIZE), then codes every link row KW_URL_SEEN when the first
 * row holding its bytes is an exclude row, else KW_URL_KEPT: a link row whose first holder is another link row is
 * kept, as isin does not deduplicate.  kw_dedup_counts keeps describing the keep-first run; the kept-rows buffers
 * of the handle then hold the remaining link rows (kw_dedup_kept_size / kw_dedup_kept_copy give the same as
 * kw_cdx_remaining_*), and kw_cdx_csv_* need a new kw_cdx_run. */
int kw_cdx_run_exclude(kw_dedup *h, int64_t n_exclude, void *stream);

/* The link rows' codes of the last kw_cdx_run_exclude into d_code (caller-owned, n_links bytes). */
int kw_cdx_exclude_codes(kw_dedup *h, uint8_t *d_code, void *stream);

/* counts[0..3) of the last kw_cdx_run_exclude: link rows, those seen, those remaining. */
int kw_cdx_exclude_counts(kw_dedup *h, int64_t *counts);

/* The remaining link rows, dense and in row order, as kw_dedup_kept_size / kw_dedup_kept_copy give the kept rows:
 * d_bytes (n_bytes), d_off (n_rows + 1 offsets into d_bytes), d_rows (n_rows indices among the link rows, from 0). */
int kw_cdx_remaining_size(kw_dedup *h, int64_t *n_rows, int64_t *n_bytes);
int kw_cdx_remaining_copy(kw_dedup *h, uint8_t *d_bytes, int64_t *d_off, int64_t *d_rows, void *stream);

/* Device times (ms) of the last kw_cdx_run_exclude: [0] the keep-first run, [1] the set-difference pass, [2] the
 * remaining rows' compaction; k <= 3 values. */
int kw_cdx_exclude_last_ms(kw_dedup *h, float *ms, int32_t k);

/* ---- the link list's refresh and split (experiental/drop.py, experiental/split.py): the set difference that also
 * drops repeats, the survivors' timestamps as sort keys, and a renderer that writes them in a given order into
 * several files
 *
 *   d = new[~new.url.isin(prev.url)].drop_duplicates('url')
 *
 * kw_cdx_run_exclude_unique is kw_cdx_run_exclude (the same layout: the first n_exclude store rows are the exclude
 * rows, the rest the link rows) except that a link row whose first holder f is an earlier link row is dropped too:
 * f < n_exclude -> KW_URL_SEEN, f == the row itself -> KW_URL_KEPT, else KW_URL_DUPLICATE.  The kept-rows buffers
 * then hold the KEPT link rows, dense and in row order; kw_cdx_exclude_codes, kw_cdx_remaining_* and
 * kw_cdx_exclude_last_ms describe this run as they describe kw_cdx_run_exclude, and so does kw_cdx_exclude_counts
 * (link rows, seen, remaining = KEPT).  kw_cdx_exclude_duplicates gives the DUPLICATE rows (0 after
 * kw_cdx_run_exclude). */
int kw_cdx_run_exclude_unique(kw_dedup *h, int64_t n_exclude, void *stream);
int kw_cdx_exclude_duplicates(kw_dedup *h, int64_t *n_duplicate);

/* The unique-URL counts of experiental/new_links.py (len(set(...))), after kw_cdx_run_exclude or
 * kw_cdx_run_exclude_unique: *n_distinct_seen = the distinct strings among the link rows coded KW_URL_SEEN (each such
 * row marks its first holder among the exclude rows, every index checked before use; the marks are counted),
 * *n_exclude_kept = the exclude rows the keep-first run coded KW_URL_KEPT (the distinct strings of the exclude rows).
 * With kw_dedup_counts' KEPT total U over the union: the link rows hold U - *n_exclude_kept + *n_distinct_seen
 * distinct strings, of which U - *n_exclude_kept are in no exclude row.  Returns when both are final. */
int kw_cdx_exclude_distinct_seen(kw_dedup *h, int64_t *n_distinct_seen, int64_t *n_exclude_kept, void *stream);

/* The "surviving rows" of the last run over the store are kw_cdx_run's kept rows, kw_cdx_run_exclude's remaining
 * rows or kw_cdx_run_exclude_unique's KEPT rows: n of them (kw_dedup_kept_size), numbered in row order.  The three
 * functions below are valid after any of the three runs, until the store changes or another run starts; otherwise
 * KW_ESTATE.
 *
 * kw_cdx_selected_ts: their timestamps into d_ts (caller-owned device memory, n values), enqueued on `stream`. */
int kw_cdx_selected_ts(kw_dedup *h, int64_t *d_ts, void *stream);

/* Surviving rows rendered in a given order into n_seg files that lie back to back.  d_order (device): n_order
 * indices among the surviving rows, any subset in any order, repeats allowed.  d_seg (device): n_seg + 1 ascending
 * bounds into d_order, d_seg[0] = 0 and d_seg[n_seg] = n_order; file s is "date_time,url\n" followed by the lines
 * of d_order[d_seg[s], d_seg[s + 1]), each decimal(timestamp), ',', the URL (wrapped in '"' when it contains ','),
 * '\n' as kw_cdx_csv_* render a row.  An empty file is the header alone.  n_seg >= 1 unless n_order = 0.
 *
 * kw_cdx_csv_select_size checks every index (0 <= i < n) and every bound on the device before anything is read
 * through them: a bad one returns KW_EINVAL with the first offender named in kw_dedup_last_error.  It writes the
 * files' sizes to d_seg_bytes (device, n_seg values), gives their sum in *n_bytes and returns when both are final.
 * kw_cdx_csv_select_copy writes the bytes of that call to d_out (16-byte aligned, *n_bytes) and returns when they
 * are written.  Offsets are 64-bit throughout. */
int kw_cdx_csv_select_size(kw_dedup *h, const int64_t *d_order, int64_t n_order, const int64_t *d_seg, int64_t n_seg,
                           int64_t *d_seg_bytes, int64_t *n_bytes, void *stream);
int kw_cdx_csv_select_copy(kw_dedup *h, uint8_t *d_out, void *stream);

/* Device times (ms) of the last kw_cdx_csv_select_size [0] and kw_cdx_csv_select_copy [1]; k <= 2 values. */
int kw_cdx_select_last_ms(kw_dedup *h, float *ms, int32_t k);

#ifdef __cplusplus
}
#endif

#endif
