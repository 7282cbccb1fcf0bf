"""Drop-ins for the two steps between the link harvest and the scraper (experiental/drop.py, experiental/split.py),
on the GPU.

    refresh_links(new_csv, prev_csv, out_csv)                   drop.py:3-11    the links not yet in the article dataset,
                                                                                first of each URL, newest first
    split_links(input_file, output_prefix, num_parts, drop_file)  split.py:10-32  the links not in a scraper's success
                                                                                file, dealt round-robin into num_parts files
    find_new_urls(new_file, old_file, output_file)              new_links.py:4-39  the links not in an older link list,
                                                                                repeats kept, and three unique-URL counts

All upload each file once.  The exclude file (the article dataset, the success file) is parsed on the device for its
``url`` column alone (quoted CSV: csrc/cdx.hip ``kw_csv_append``), the links file for its ``date_time,url`` rows
(``kw_cdx_append``, the part dialect), the set difference runs on the keep-first hash table
(``kw_cdx_run_exclude_unique`` / ``kw_cdx_run_exclude``), and the surviving rows are rendered on the device in the order
and into the files asked for (``kw_cdx_csv_select_*``).  The refresh brings 8 bytes a surviving row to the host, their
timestamps, and computes the descending order there exactly as pandas does (``descending_order``): among equal
timestamps the order is numpy's, on either route.

The device route is taken only when the existing parsers accept every file (the rules: DESIGN.md §7, "Link refresh and
split"), the exclude file's header names exactly one column ``url``, and ``num_parts >= 1``.  A refused, missing or
empty file, a links file whose URLs hold ``"``, and everything under ``KW_LINKS_NATIVE=0`` run the reference's pandas
lines as they stand, so its exceptions are unchanged.  The output files are byte-identical on either route.

A file of ``stream_from`` bytes or more goes to the device window by window (``cdx_dedup.GpuUrlDedup.csv_append_file``
for the exclude file, ``cdx_append_file`` for the links file): two pinned slots of ``window_bytes``, a reader thread one
window ahead, the unconsumed tail carried on the device, so host and device memory for text do not depend on the
file's size.  A record longer than ``max_record_bytes`` that no window holds sends the call down the pandas route.
Smaller files keep the one-piece upload.  ``LinksResult.windows`` holds the windows each file took.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np

from . import _native, cdx_dedup

WINDOW_BYTES = 256 << 20       # a window of a streamed file (as the per-ticker sort's)
MAX_RECORD_BYTES = 64 << 20    # the longest unconsumed tail carried between windows; a longer record: the pandas route
# Files of this size or more are streamed.  At a few hundred MB the streamed route ties the one-piece route within the
# run-to-run spread (refresh 0.222 s against 0.225 s, resume 0.159 s against 0.173 s; profiles/e2e_links_stream.json,
# profiles/e2e_resume_stream.json) and holds its two pinned windows on top, so smaller files stay in one piece; at two
# windows the one-piece route's host copy is as large as the pinned slots ("Windowed CSV append").
STREAM_FROM = 2 * WINDOW_BYTES


class LinksResult:
    """What a call did: the route and the row counts."""

    def __init__(self, route: str, n_links: int, seen: int, duplicate: int, written: int,
                 parts: Optional[List[int]] = None, windows: Tuple[int, int] = (0, 0)):
        self.route = route          # 'device' or 'pandas'
        self.n_links = n_links      # rows of the links file
        self.seen = seen            # those whose URL is in the exclude file
        self.duplicate = duplicate  # refresh: those left whose URL an earlier link row holds (split: 0)
        self.written = written      # rows written, over all files
        self.parts = parts          # split: rows per file
        self.windows = windows      # the windows the exclude file and the links file took (0: in one piece, or pandas)

    def counts(self) -> Tuple[int, int, int, int]:
        return self.n_links, self.seen, self.duplicate, self.written

    def __repr__(self):
        return (f"LinksResult(route={self.route!r}, n_links={self.n_links}, seen={self.seen}, "
                f"duplicate={self.duplicate}, written={self.written}, parts={self.parts}, windows={self.windows})")


def native_enabled() -> bool:
    """The device route is on unless ``KW_LINKS_NATIVE=0`` (then: the reference's pandas lines)."""
    return os.environ.get('KW_LINKS_NATIVE', '1') != '0'


def descending_order(keys: np.ndarray) -> np.ndarray:
    """The row order of ``DataFrame.sort_values(by=..., ascending=False)`` over an integer column: pandas' nargsort
    reverses the keys, sorts them ascending with numpy's default kind, and reverses the result."""
    keys = np.asarray(keys)
    idx = np.arange(len(keys), dtype=np.int64)
    return idx[::-1][np.argsort(keys[::-1], kind='quicksort')][::-1]


def _header_url_col(data: np.ndarray) -> Optional[Tuple[str, int]]:
    """(the file's first line, the index of its one ``url`` name), or None when kw_csv_append cannot be given it."""
    nl = np.flatnonzero(data[:1 << 20] == 0x0A)
    end = int(nl[0]) if len(nl) else (len(data) if len(data) <= 1 << 20 else -1)
    if end < 0:
        return None
    line = data[:end].tobytes()
    if line.endswith(b'\r'):
        line = line[:-1]
    if b'"' in line or b'\0' in line:
        return None
    try:
        header = line.decode('utf-8')
    except UnicodeDecodeError:
        return None
    names = header.split(',')
    if names.count('url') != 1:
        return None
    return header, names.index('url')


def _out_dir_ok(path: str) -> bool:
    return os.path.isdir(os.path.dirname(path) or '.')


def _file_head(path: str) -> Optional[np.ndarray]:
    """The file's first bytes, enough for ``_header_url_col`` to judge as it judges the whole file."""
    try:
        return np.fromfile(path, dtype=np.uint8, count=(1 << 20) + 1)
    except (OSError, ValueError):
        return None


def _load(exclude_csv: str, links_csv: str, stream_from: int = STREAM_FROM, window_bytes: int = WINDOW_BYTES,
          max_record_bytes: int = MAX_RECORD_BYTES):
    """Both files in the store, the exclude rows first: (handle, exclude rows, link rows, windows of either file), or
    None when a file is not eligible.  A file of ``stream_from`` bytes or more is streamed."""
    sizes = []
    for path in (exclude_csv, links_csv):
        try:
            size = os.path.getsize(path)
        except OSError:
            return None
        if not size:
            return None
        sizes.append(size)
    streamed = [size >= stream_from for size in sizes]
    files = [None if streamed[k] else cdx_dedup._file_bytes(path) for k, path in enumerate((exclude_csv, links_csv))]
    if any(f is None and not streamed[k] for k, f in enumerate(files)):
        return None
    head_bytes = _file_head(exclude_csv) if streamed[0] else files[0]
    head = _header_url_col(head_bytes) if head_bytes is not None else None
    if head is None:
        return None
    g = cdx_dedup._dedup()
    g.cdx_begin()
    windows = [0, 0]
    if streamed[0]:
        verdict, n_ex, stats = g.csv_append_file(exclude_csv, head[0], head[1], window_bytes, max_record_bytes)
        windows[0] = stats['windows']
    else:
        verdict, _, n_ex = g.csv_append(files[0], head[0], head[1])
    if verdict != _native.KW_CSV_OK:
        return None
    if streamed[1]:
        verdict, n_links, stats = g.cdx_append_file(links_csv, 'part', window_bytes, max_record_bytes)
        windows[1] = stats['windows']
    else:
        verdict, _, n_links = g.cdx_append(files[1], 'part')
    if verdict != _native.KW_CDX_OK or n_links == 0:   # (no rows: left to pandas, as in cdx_dedup)
        return None
    return g, n_ex, n_links, tuple(windows)


# ------------------------------------------------------------------ refresh (drop.py)
def _refresh_pandas(new_csv: str, prev_csv: str, out_csv: str) -> LinksResult:
    """drop.py:3-11 as they stand."""
    import pandas as pd
    df_new = pd.read_csv(new_csv)
    df_prev = pd.read_csv(prev_csv)
    df_new_filtered = df_new[~df_new['url'].isin(df_prev['url'])]
    n_unseen = len(df_new_filtered)
    df_new_filtered = df_new_filtered.drop_duplicates(subset='url')
    df_new_filtered['date_time'] = df_new_filtered['date_time'].astype(int)
    df_new_filtered = df_new_filtered.sort_values(by='date_time', ascending=False)
    df_new_filtered.reset_index(drop=True, inplace=True)
    df_new_filtered.to_csv(out_csv, index=False)
    return LinksResult('pandas', len(df_new), len(df_new) - n_unseen, n_unseen - len(df_new_filtered),
                       len(df_new_filtered))


def _refresh_device(new_csv: str, prev_csv: str, out_csv: str, **stream) -> Optional[LinksResult]:
    if not _out_dir_ok(out_csv):
        return None   # (the pandas route raises the reference's error)
    loaded = _load(prev_csv, new_csv, **stream)
    if loaded is None:
        return None
    g, n_ex, _, windows = loaded
    n_links, seen, duplicate, kept = g.run_exclude_unique(n_ex)
    order = descending_order(g.selected_ts())
    csv = g.csv_select(order)[0]
    with open(out_csv, 'wb') as fh:
        fh.write(csv)
    return LinksResult('device', n_links, seen, duplicate, kept, windows=windows)


def refresh_links(new_csv: str = 'yahoo_links_1.csv', prev_csv: str = 'yahoo_articles_all.csv',
                  out_csv: str = 'yahoo_links_new.csv', *, stream_from: int = STREAM_FROM,
                  window_bytes: int = WINDOW_BYTES, max_record_bytes: int = MAX_RECORD_BYTES) -> LinksResult:
    """drop.py:3-11: the rows of ``new_csv`` whose URL is not in ``prev_csv``, the first of each URL, sorted by
    ``date_time`` descending, written to ``out_csv``.  A file of ``stream_from`` bytes or more is streamed in windows
    of ``window_bytes``."""
    res = _refresh_device(new_csv, prev_csv, out_csv, stream_from=stream_from, window_bytes=window_bytes,
                          max_record_bytes=max_record_bytes) if native_enabled() else None
    if res is None:
        res = _refresh_pandas(new_csv, prev_csv, out_csv)
    return res


# ------------------------------------------------------------------ split (split.py)
def _split_pandas(input_file: str, output_prefix: str, num_parts: int, drop_file: str) -> LinksResult:
    """split.py:10-30 as they stand (its frame dumps included)."""
    import pandas as pd
    df = pd.read_csv(input_file)
    drop_df = pd.read_csv(drop_file)
    print(df)
    n_links = len(df)
    df = df[~df['url'].isin(drop_df['url'])]
    print(df)
    part_numbers = np.arange(num_parts)
    df['part'] = np.tile(part_numbers, len(df) // num_parts + 1)[:len(df)]
    parts = []
    for i in range(num_parts):
        part_df = df[df['part'] == i].drop('part', axis=1)
        print(i)
        print(part_df)
        part_df.to_csv(f"{output_prefix}_{i}.csv", index=False)
        parts.append(len(part_df))
    return LinksResult('pandas', n_links, n_links - len(df), 0, len(df), parts)


def _split_device(input_file: str, output_prefix: str, num_parts: int, drop_file: str,
                  **stream) -> Optional[LinksResult]:
    if isinstance(num_parts, bool) or not isinstance(num_parts, (int, np.integer)) or num_parts < 1:
        return None
    if not _out_dir_ok(f"{output_prefix}_0.csv"):
        return None
    loaded = _load(drop_file, input_file, **stream)
    if loaded is None:
        return None
    g, n_ex, _, windows = loaded
    k = int(num_parts)
    n_links, seen, remaining = g.run_exclude(n_ex)
    # file i holds surviving rows i, i + k, i + 2k, ...: built on the device
    t = g.torch
    idx = t.arange(remaining, dtype=t.int64, device=t.device('cuda', g.device))
    order = t.cat([idx[i::k] for i in range(k)])
    parts = [len(range(i, remaining, k)) for i in range(k)]
    seg = np.concatenate([[0], np.cumsum(np.asarray(parts, dtype=np.int64))]).astype(np.int64)
    files = g.csv_select(order, seg)
    for i, csv in enumerate(files):
        with open(f"{output_prefix}_{i}.csv", 'wb') as fh:
            fh.write(csv)
    return LinksResult('device', n_links, seen, 0, remaining, parts, windows=windows)


def split_links(input_file: str, output_prefix: str, num_parts: int, drop_file: str, *,
                stream_from: int = STREAM_FROM, window_bytes: int = WINDOW_BYTES,
                max_record_bytes: int = MAX_RECORD_BYTES) -> LinksResult:
    """split.py:10-32: the rows of ``input_file`` whose URL is not in ``drop_file``, dealt round-robin into
    ``"{output_prefix}_{i}.csv"`` for i < num_parts, and the reference's closing line.  The reference also prints
    the frames it reads and writes (``print(df)``); those dumps are not reproduced on the device route, which
    holds no frame."""
    res = _split_device(input_file, output_prefix, num_parts, drop_file, stream_from=stream_from,
                        window_bytes=window_bytes, max_record_bytes=max_record_bytes) if native_enabled() else None
    if res is None:
        res = _split_pandas(input_file, output_prefix, num_parts, drop_file)
    print(f"CSV file has been split into {num_parts} parts.")
    return res


# ------------------------------------------------------------------ new links (new_links.py)
class NewUrls(LinksResult):
    """``find_new_urls``' counts beside the row counts: the three numbers the reference prints, all of unique URLs."""

    def __init__(self, route: str, n_links: int, seen: int, written: int, unique_new: int, unique_old: int,
                 unique_only_new: int, windows: Tuple[int, int] = (0, 0)):
        super().__init__(route, n_links, seen, 0, written, windows=windows)
        self.unique_new = unique_new            # distinct URLs of the new file
        self.unique_old = unique_old            # distinct URLs of the old file
        self.unique_only_new = unique_only_new  # distinct URLs of the new file that the old one does not hold


def _new_urls_pandas(new_file: str, old_file: str, output_file: str) -> Optional[NewUrls]:
    """new_links.py:8-39 as they stand (the first line is printed by the caller)."""
    import pandas as pd
    try:
        new_df = pd.read_csv(new_file)
        old_df = pd.read_csv(old_file)
    except Exception as e:
        print(f"Error reading CSV files: {e}")
        return None
    if 'url' not in new_df.columns or 'url' not in old_df.columns:
        print("Error: One or both CSV files missing 'url' column")
        print(f"New file columns: {new_df.columns.tolist()}")
        print(f"Old file columns: {old_df.columns.tolist()}")
        return None
    new_urls = set(new_df['url'].tolist())
    old_urls = set(old_df['url'].tolist())
    unique_new_urls = new_urls - old_urls
    print(f"Total URLs in new file: {len(new_urls)}")
    print(f"Total URLs in old file: {len(old_urls)}")
    print(f"URLs unique to new file: {len(unique_new_urls)}")
    result_df = new_df[new_df['url'].isin(unique_new_urls)]
    result_df.to_csv(output_file, index=False)
    print(f"New URLs saved to {output_file}")
    return NewUrls('pandas', len(new_df), len(new_df) - len(result_df), len(result_df), len(new_urls), len(old_urls),
                   len(unique_new_urls))


def _new_urls_device(new_file: str, old_file: str, output_file: str, **stream) -> Optional[NewUrls]:
    if not _out_dir_ok(output_file):
        return None   # (the pandas route raises the reference's error)
    loaded = _load(old_file, new_file, **stream)
    if loaded is None:
        return None
    g, n_ex, _, windows = loaded
    n_links, seen, remaining = g.run_exclude(n_ex)
    union = g.counts()[_native.KW_URL_KEPT]           # distinct URLs over both files
    distinct_seen, unique_old = g.exclude_distinct_seen()
    t = g.torch
    csv = g.csv_select(t.arange(remaining, dtype=t.int64, device=t.device('cuda', g.device)))[0]
    with open(output_file, 'wb') as fh:
        fh.write(csv)
    only_new = union - unique_old
    return NewUrls('device', n_links, seen, remaining, only_new + distinct_seen, unique_old, only_new, windows)


def find_new_urls(new_file: str, old_file: str, output_file: str, *, stream_from: int = STREAM_FROM,
                  window_bytes: int = WINDOW_BYTES, max_record_bytes: int = MAX_RECORD_BYTES) -> Optional[NewUrls]:
    """new_links.py:4-39: the rows of ``new_file`` whose URL is not in ``old_file``, in file order with repeats kept,
    written to ``output_file``, and the reference's printed lines (its three counts are of unique URLs).  None where
    the reference returns early (unreadable files, a missing ``url`` column)."""
    print(f"Comparing URLs in {new_file} and {old_file}...")
    res = _new_urls_device(new_file, old_file, output_file, stream_from=stream_from, window_bytes=window_bytes,
                           max_record_bytes=max_record_bytes) if native_enabled() else None
    if res is None:
        return _new_urls_pandas(new_file, old_file, output_file)
    print(f"Total URLs in new file: {res.unique_new}")
    print(f"Total URLs in old file: {res.unique_old}")
    print(f"URLs unique to new file: {res.unique_only_new}")
    print(f"New URLs saved to {output_file}")
    return res
