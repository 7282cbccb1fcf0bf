"""Drop-ins for the two steps between the link harvest and the scraper (experiental/drop.py, experiental/split.py),
on the GPU.

    refresh_links(new_csv, prev_csv, out_csv)                   drop.py:3-11    the links not yet in the article dataset,
                                                                                first of each URL, newest first
    split_links(input_file, output_prefix, num_parts, drop_file)  split.py:10-32  the links not in a scraper's success
                                                                                file, dealt round-robin into num_parts files

Both upload each file once.  The exclude file (the article dataset, the success file) is parsed on the device for its
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

Whole files are uploaded in one piece: an exclude file larger than device memory is not windowed here.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np

from . import _native, cdx_dedup


class LinksResult:
    """What a call did: the route and the row counts."""

    def __init__(self, route: str, n_links: int, seen: int, duplicate: int, written: int,
                 parts: Optional[List[int]] = None):
        self.route = route          # 'device' or 'pandas'
        self.n_links = n_links      # rows of the links file
        self.seen = seen            # those whose URL is in the exclude file
        self.duplicate = duplicate  # refresh: those left whose URL an earlier link row holds (split: 0)
        self.written = written      # rows written, over all files
        self.parts = parts          # split: rows per file

    def counts(self) -> Tuple[int, int, int, int]:
        return self.n_links, self.seen, self.duplicate, self.written

    def __repr__(self):
        return (f"LinksResult(route={self.route!r}, n_links={self.n_links}, seen={self.seen}, "
                f"duplicate={self.duplicate}, written={self.written}, parts={self.parts})")


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


def _load(exclude_csv: str, links_csv: str):
    """Both files in the store, the exclude rows first: (handle, exclude rows, link rows), or None when a file is
    not eligible."""
    files = []
    for path in (exclude_csv, links_csv):
        data = cdx_dedup._file_bytes(path) if os.path.exists(path) else None
        if data is None or not len(data):
            return None
        files.append(data)
    head = _header_url_col(files[0])
    if head is None:
        return None
    g = cdx_dedup._dedup()
    g.cdx_begin()
    verdict, _, n_ex = g.csv_append(files[0], head[0], head[1])
    if verdict != _native.KW_CSV_OK:
        return None
    verdict, _, n_links = g.cdx_append(files[1], 'part')
    if verdict != _native.KW_CDX_OK or n_links == 0:   # (no rows: left to pandas, as in cdx_dedup)
        return None
    return g, n_ex, n_links


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


def _refresh_device(new_csv: str, prev_csv: str, out_csv: str) -> Optional[LinksResult]:
    if not _out_dir_ok(out_csv):
        return None   # (the pandas route raises the reference's error)
    loaded = _load(prev_csv, new_csv)
    if loaded is None:
        return None
    g, n_ex, _ = loaded
    n_links, seen, duplicate, kept = g.run_exclude_unique(n_ex)
    order = descending_order(g.selected_ts())
    csv = g.csv_select(order)[0]
    with open(out_csv, 'wb') as fh:
        fh.write(csv)
    return LinksResult('device', n_links, seen, duplicate, kept)


def refresh_links(new_csv: str = 'yahoo_links_1.csv', prev_csv: str = 'yahoo_articles_all.csv',
                  out_csv: str = 'yahoo_links_new.csv') -> LinksResult:
    """drop.py:3-11: the rows of ``new_csv`` whose URL is not in ``prev_csv``, the first of each URL, sorted by
    ``date_time`` descending, written to ``out_csv``."""
    res = _refresh_device(new_csv, prev_csv, out_csv) if native_enabled() else None
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


def _split_device(input_file: str, output_prefix: str, num_parts: int, drop_file: str) -> Optional[LinksResult]:
    if isinstance(num_parts, bool) or not isinstance(num_parts, (int, np.integer)) or num_parts < 1:
        return None
    if not _out_dir_ok(f"{output_prefix}_0.csv"):
        return None
    loaded = _load(drop_file, input_file)
    if loaded is None:
        return None
    g, n_ex, _ = loaded
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
    return LinksResult('device', n_links, seen, 0, remaining, parts)


def split_links(input_file: str, output_prefix: str, num_parts: int, drop_file: str) -> LinksResult:
    """split.py:10-32: the rows of ``input_file`` whose URL is not in ``drop_file``, dealt round-robin into
    ``"{output_prefix}_{i}.csv"`` for i < num_parts, and the reference's closing line.  The reference also prints
    the frames it reads and writes (``print(df)``); those dumps are not reproduced on the device route, which
    holds no frame."""
    res = _split_device(input_file, output_prefix, num_parts, drop_file) if native_enabled() else None
    if res is None:
        res = _split_pandas(input_file, output_prefix, num_parts, drop_file)
    print(f"CSV file has been split into {num_parts} parts.")
    return res
