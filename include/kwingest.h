/*
 * kwingest.h — C-ABI of the article ingest on the GPU (libkwmatch.so,
 * advanced_scrapper_amd/csrc/kwingest.hip).
 *
 * What it replaces.  The host ingest (advanced_scrapper_amd/ingest.py over csrc/kwcsv.c) finds a chunk's
 * records (kwcsv_records), tokenizes them (kwcsv_parse), packs the matcher's arena (kwcsv_pack) and parses the
 * dates (kwcsv_dates); the arena and the cells are then uploaded.  kw_ingest_parse takes the raw CSV bytes in
 * device memory instead and leaves, in device buffers of the handle, the cells, the arena and the dates byte for
 * byte as those four functions give them -- wherever the take rule below holds; where it does not, nothing is
 * produced and the caller runs the host route on that chunk.
 *
 * The take rule (restated in tests/ingest_rule.py).  The quote state of a byte is the parity of
 * the '"' bytes before it.  Outside quotes ',' ends a field and '\n' ends a record ("\r\n": the '\r' belongs to
 * the terminator); a record of no bytes but its terminator is skipped.  With final == 0 the records are those
 * whose '\n' lies in the window; with final == 1 the text's end also ends a record that has bytes.  The first
 * max_rows records are taken; `consumed` is the position after the last taken record's '\n' (the text's length
 * when final == 1 and the text has fewer than max_rows records).  The conditions are tested over the bytes
 * before a limit -- `consumed`, or the text's length when final == 1 and the text has fewer than max_rows
 * records -- in this order; the verdict is the first condition that has an offender, the position its first
 * offender's:
 *   KW_INGEST_NUL     a NUL byte (its position)
 *   KW_INGEST_UTF8    not strict UTF-8 (the first byte of the sequence a strict decoder stops at)
 *   KW_INGEST_QUOTE   a '"' outside quotes whose previous byte is none of ',' '\n' '"' (the text starts after
 *                     a virtual '\n'); a '"' inside quotes whose next byte is none of ',' '\n' '\r' '"' (the
 *                     window's last byte has no next byte and passes); a final text that ends inside quotes
 *                     (position: the text's length)
 *   KW_INGEST_CR      a '\r' outside quotes whose next byte is not '\n' (the last byte of a window that is
 *                     not final passes)
 *   KW_INGEST_BLANK   a record of spaces and tabs only (the record's first byte)
 *   KW_INGEST_FIELDS  a record whose field count is not ncols (the position of its terminating '\n', or the
 *                     text's length for the final record)
 *   KW_INGEST_ROWS    2^31 rows or cells, or more
 * A cell's bytes are its record bytes without the field and record separators, the opening and closing quote
 * and the first '"' of every "" pair.
 *
 * The ISO rule of the date cell (restated in tests/dates_rule.py).  A date cell that is not NA is
 * native iff its bytes are, as a whole cell,
 *   YYYY-MM-DD[ T]HH:MM:SS ( '.' 1-9 digits )? ( 'Z' | [+-]HH ( ':'? MM )? )?
 * with ASCII digits, year >= 1000, month, day, hour, minute and second valid by the calendar, offset HH <= 23 and
 * MM <= 59: 19 to 35 bytes.  dateutil parses such a cell to those fields, the fraction's first six digits as
 * microseconds (further digits dropped, not rounded) and the zone as a fixed offset.  Its kind is
 *   1  the 19-byte layout:       us = the wall clock's epoch microseconds read as UTC, off_s = 0
 *   4  naive with a fraction:    us = the wall clock's epoch microseconds, off_s = 0
 *   3  with 'Z' or an offset:    us = the instant's epoch microseconds (wall clock minus offset),
 *                                off_s = +-(HH * 3600 + MM * 60), 0 for 'Z'
 * an NA cell's is 2 and every other cell's 0 (us = off_s = 0: the caller asks dateutil).  The rule never reads
 * the process's time zone: what a zero offset means to dateutil there is the caller's to decide (dates.py).
 *
 * Conventions as kwmatch.h: 0 or a negative KW_E* code; kw_ingest_last_error gives the message; one handle
 * per device and host thread.  Every device buffer a call returns belongs to the handle and stays valid until
 * the next kw_ingest_parse or kw_ingest_destroy.
 */
#ifndef KWINGEST_H
#define KWINGEST_H

#include <stdint.h>

#include "kwmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kw_ingest kw_ingest;

/* verdicts of kw_ingest_parse, in the order the conditions are tested */
#define KW_INGEST_OK 0
#define KW_INGEST_NUL 1
#define KW_INGEST_UTF8 2
#define KW_INGEST_QUOTE 3
#define KW_INGEST_CR 4
#define KW_INGEST_BLANK 5
#define KW_INGEST_FIELDS 6
#define KW_INGEST_ROWS 7

/* ncols: the CSV's columns (6 <= ncols <= 4096); cols[6]: the columns of article_text, title, date_time, url,
 * source, source_url (distinct, each in [0, ncols)); na / na_off / n_na: the NA strings as one byte buffer and
 * n_na + 1 int32 offsets (host arrays, copied; n_na <= 64, each at most 16 bytes). */
int kw_ingest_create(int32_t device, int32_t ncols, const int32_t *cols, const uint8_t *na, const int32_t *na_off,
                     int32_t n_na, kw_ingest **out);

/* The parser's tile: the bytes one block classifies at once. */
int kw_ingest_tile_bytes(void);

/* Parse the first max_rows complete records of d_text[0, n_bytes) (device memory, 16-byte aligned, readable up
 * to the next multiple of 16; the text starts at a record start).  0 <= n_bytes < 2^31, max_rows >= 1.
 * Returns after the device finished: *verdict, and for KW_INGEST_OK *n_rows and *consumed (see above; n_rows == 0
 * with final == 0: the window holds no complete record); otherwise *n_rows = *consumed = 0 and *bad_pos is the
 * offender's position.  stream: a hipStream_t (NULL = default stream); the text must be complete on it. */
int kw_ingest_parse(kw_ingest *h, const uint8_t *d_text, int64_t n_bytes, int32_t final, int64_t max_rows,
                    int64_t *n_rows, int64_t *consumed, int32_t *verdict, int64_t *bad_pos, void *stream);

/* A pinned host window of the handle (slot 0 or 1) of n_bytes at least (0 <= n_bytes < 2^31): the reader fills
 * one while the other's chunk is at work.  A slot that grows loses its contents. */
int kw_ingest_stage(kw_ingest *h, int32_t slot, int64_t n_bytes, uint8_t **host);

/* Copy bytes [start, start + n_bytes) of a slot to the start of the handle's device text buffer on `stream`
 * (asynchronous; a text for kw_ingest_parse on the same stream).  What a window holds beyond one chunk serves
 * the next from the same slot.  The slot may be refilled once the parse has returned. */
int kw_ingest_upload(kw_ingest *h, int32_t slot, int64_t start, int64_t n_bytes, const uint8_t **d_text,
                     void *stream);

/* After an OK parse: the cells of all ncols columns as kwcsv_parse gives them -- *d_cells (cell_bytes bytes),
 * *d_coff (n_rows * ncols + 1 int64) and *d_cfl (n_rows * ncols bytes of KWCSV_* flags). */
int kw_ingest_cells(kw_ingest *h, const uint8_t **d_cells, const int64_t **d_coff, const uint8_t **d_cfl,
                    int64_t *cell_bytes);

/* After an OK parse: the matcher's arena as kwcsv_pack gives it -- per row the article_text cell then the title
 * cell, an NA cell as "nan"; *d_off: 2 * n_rows + 1 int64; 64 zero bytes follow the arena's arena_bytes. */
int kw_ingest_arena(kw_ingest *h, const uint8_t **d_arena, const int64_t **d_off, int64_t *arena_bytes);

/* After an OK parse: kwcsv_dates' arrays of the date_time column into host arrays us[n_rows], kind[n_rows]
 * (2: NA; 1: the layout 'YYYY-MM-DD[ T]HH:MM:SS', us = its epoch microseconds; 0: neither). */
int kw_ingest_dates(kw_ingest *h, int64_t *us, uint8_t *kind);

/* After an OK parse: kwcsv_dates_iso's arrays of the date_time column, the ISO rule above, into host arrays
 * us[n_rows], kind[n_rows], off_s[n_rows].  (kw_ingest_dates is this with kinds 3 and 4 given as kind 0, us 0.) */
int kw_ingest_dates_iso(kw_ingest *h, int64_t *us, uint8_t *kind, int32_t *off_s);

/* After an OK parse: witness[k] = 1 iff some taken row's cell of column cols[k] carries KWCSV_TEXT. */
int kw_ingest_column_flags(kw_ingest *h, int32_t *witness);

/* After an OK parse: the cells into host arrays cells[cell_bytes], coff[n_rows * ncols + 1], cfl[n_rows * ncols]. */
int kw_ingest_copy_cells(kw_ingest *h, uint8_t *cells, int64_t *coff, uint8_t *cfl);

/* After an OK parse: the arena into host arrays arena[arena_bytes + 64] (its zero pad included), off[2 * n_rows + 1]. */
int kw_ingest_copy_arena(kw_ingest *h, uint8_t *arena, int64_t *off);

/* After an OK parse: column col's cells, dense, into host arrays bytes[cap], off[n_rows + 1], fl[n_rows]
 * (KW_EOVERFLOW when the column holds more than cap bytes; cell_bytes always suffices). */
int kw_ingest_copy_column(kw_ingest *h, int32_t col, uint8_t *bytes, int64_t cap, int64_t *off, uint8_t *fl);

/* After an OK parse, while its text still stands in device memory: every taken record's byte span in that text as
 * kwcsv_parse's rspan gives it -- (*d_start)[r] the record's first byte, (*d_end)[r] the byte after its last, the
 * terminator ("\n" or "\r\n") excluded; records of no bytes are skipped by the take rule, so a start is not the
 * previous end + 1.  n_rows int64 each, device memory of the handle, written on the parse's stream (asynchronous:
 * read them on that stream or after synchronising it).  Also the parse's own shape: *n_rows, *ncols, *d_text and
 * *n_bytes. */
int kw_ingest_spans(kw_ingest *h, const int64_t **d_start, const int64_t **d_end, int64_t *n_rows, int32_t *ncols,
                    const uint8_t **d_text, int64_t *n_bytes);

/* kw_ingest_spans into host arrays start[n_rows], end[n_rows]. */
int kw_ingest_copy_spans(kw_ingest *h, int64_t *start, int64_t *end);

/* The process's zone table (kwstamps.h: at[n_trans + 1] ascending instants, off[n_trans] UTC offsets in seconds,
 * 1 <= n_trans <= 1024; host arrays, copied to the device and kept across parses).  Every OK parse from now on
 * also computes each row's time_unix = int(datetime.timestamp()) under it (ig_stamps_kernel, after the dates, on
 * the parse's stream): the rule of kwstamps.h on the row's us / kind, native[r] = 1 where the value is final
 * (kinds 1, 3, 4 inside the table's range), 0 where the caller must ask timestamp() itself (stamps[r] = 0).  The
 * rule never reads the process's zone: the caller masks the rows it hands back to dateutil (the zero-offset
 * guard, dates.py).  Calling it again replaces the table; n_trans == 0 (at, off may be null) takes it away.
 * KW_EINVAL: n_trans outside [0, 1024], a null array, instants that do not ascend. */
int kw_ingest_zone(kw_ingest *h, const int64_t *at, const int32_t *off, int32_t n_trans);

/* After an OK parse that had a zone table: the rows' stamps into host arrays stamps[n_rows], native[n_rows].
 * KW_ESTATE: no such parse. */
int kw_ingest_stamps(kw_ingest *h, int64_t *stamps, uint8_t *native);

/* After an OK parse that had a zone table: *d_stamps = the stamps in device memory (n_rows int64; for
 * kw_rows_emit_stamps_device, kwrows.h).  KW_ESTATE: no such parse. */
int kw_ingest_stamps_device(kw_ingest *h, const int64_t **d_stamps);

/* Device times (ms) of the last parse, up to 5 values: [0] classify (quote counts, NUL, UTF-8, their scan),
 * [1] cells (counts, scans, offsets and the kept bytes, the verdict, the flags), [2] arena + dates + stamps,
 * [3] all, [4] the stamps kernel alone (0 without a zone table; a part of [2] and [3]). */
int kw_ingest_last_ms(kw_ingest *h, float *ms, int32_t n);

const char *kw_ingest_last_error(kw_ingest *h);
int kw_ingest_destroy(kw_ingest *h);

#ifdef __cplusplus
}
#endif
#endif
