"""Drop-in for the scraper's resume filter (constant_rate_scrapper.py:312-360), on the GPU.

    remaining_urls(links_csv='yfin_urls.csv', website='yfin')   the links not yet in the success / failed files

The reference reads ``yfin_urls.csv``, builds a Python ``set`` of every URL in ``success_articles_<website>.csv`` and
``failed_articles_<website>.csv`` and filters the links with an object-dtype ``isin``.  Here the three files are
uploaded once each, parsed on the device (quoted CSV: csrc/cdx.hip ``kw_csv_append``) into the dedup handle's row
store, and the set difference runs on the keep-first hash table (csrc/dedup.hip ``kw_cdx_run_exclude``); nothing
per row runs on the host except in ``Resume.urls()``.

The device parser is used only where its result provably equals ``pd.read_csv(file)["url"].astype(str)`` (the rule:
DESIGN.md §7, tests/resume_rule.py).  A file it refuses, and everything under ``KW_RESUME_NATIVE=0``, sends the whole
call down the reference's pandas lines, so its exceptions and messages stay as they are (a missing links file
included).  What ``csv.writer`` / ``csv.DictWriter`` write is always eligible.

A file of ``stream_from`` bytes or more goes to the device window by window
(``cdx_dedup.GpuUrlDedup.csv_append_file``: two pinned slots of ``window_bytes``, a reader thread one window ahead), so
host and device memory for text do not depend on the file's size; ``Resume.windows`` holds the windows each file took.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np

from . import _native, cdx_dedup
from .links import MAX_RECORD_BYTES, STREAM_FROM, WINDOW_BYTES   # (the streamed route's geometry and threshold)

SUCCESS_FIELDS = ["url", "datetime", "ticker_symbols", "author", "source", "source_url", "title", "article"]
FAILED_FIELDS = ["url", "error"]
LINKS_FIELDS = ["date_time", "url"]


class Resume:
    """What the reference knows after :312-360."""

    def __init__(self, initial_total: int, scraped_success: int, scraped_fails: int, remaining: int, route: str,
                 urls: Optional[List[str]] = None, arrays: Optional[Tuple[np.ndarray, np.ndarray]] = None,
                 windows: Tuple[int, int, int] = (0, 0, 0)):
        self.initial_total = initial_total      # rows of the links file
        self.scraped_success = scraped_success  # rows of the success file (0: missing)
        self.scraped_fails = scraped_fails      # rows of the failed file (0: missing)
        self.remaining = remaining              # links whose URL is in neither
        self.route = route                      # 'device' or 'pandas'
        self.windows = windows                  # the windows the success, failed and links files took (0: one piece)
        self._urls, self._arrays = urls, arrays

    def arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        """The remaining URLs in file order: (UTF-8 bytes, int64 offsets [remaining + 1])."""
        if self._arrays is None:
            enc = [u.encode('utf-8', 'surrogatepass') for u in self._urls]
            off = np.zeros(len(enc) + 1, dtype=np.int64)
            if enc:
                np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=off[1:])
            self._arrays = (np.frombuffer(b''.join(enc), dtype=np.uint8), off)
        return self._arrays

    def urls(self) -> List[str]:
        """The remaining URLs in file order (the reference's ``urls`` list)."""
        if self._urls is None:
            b, off = self._arrays
            raw = b.tobytes()
            self._urls = [raw[off[k]:off[k + 1]].decode('utf-8') for k in range(len(off) - 1)]
        return self._urls

    def write(self, path: str) -> None:
        """One remaining URL a line."""
        b, off = self.arrays()
        n = len(off) - 1
        out = np.full(len(b) + n, 0x0A, dtype=np.uint8)
        if n:
            out[np.arange(len(b), dtype=np.int64) + np.repeat(np.arange(n, dtype=np.int64), np.diff(off))] = b
        with open(path, 'wb') as fh:
            fh.write(out.tobytes())


def native_enabled() -> bool:
    """The device route is on unless ``KW_RESUME_NATIVE=0`` (then: the reference's pandas lines)."""
    return os.environ.get('KW_RESUME_NATIVE', '1') != '0'


def _pandas_route(links_csv: str, success_csv: str, failed_csv: str) -> Resume:
    """constant_rate_scrapper.py:312-357 as they stand."""
    import pandas as pd
    df_links = pd.read_csv(links_csv)
    all_urls = df_links["url"].astype(str).tolist()
    initial_total = len(all_urls)
    scraped_urls = set()
    if os.path.exists(success_csv):
        df_success_existing = pd.read_csv(success_csv)
        scraped_success = len(df_success_existing)
        scraped_urls.update(df_success_existing["url"].astype(str).tolist())
    else:
        scraped_success = 0
    if os.path.exists(failed_csv):
        df_failed_existing = pd.read_csv(failed_csv)
        scraped_fails = len(df_failed_existing)
        scraped_urls.update(df_failed_existing["url"].astype(str).tolist())
    else:
        scraped_fails = 0
    df_links = df_links[~df_links["url"].astype(str).isin(scraped_urls)]
    urls = df_links["url"].astype(str).tolist()
    return Resume(initial_total, scraped_success, scraped_fails, len(urls), 'pandas', urls=urls)


def _device_route(links_csv: str, success_csv: str, failed_csv: str, stream_from: int = STREAM_FROM,
                  window_bytes: int = WINDOW_BYTES, max_record_bytes: int = MAX_RECORD_BYTES) -> Optional[Resume]:
    """The result when every file there is is eligible, else None."""
    if not os.path.exists(links_csv):
        return None   # (the pandas route raises the reference's error)
    files = [(success_csv, SUCCESS_FIELDS), (failed_csv, FAILED_FIELDS), (links_csv, LINKS_FIELDS)]
    g = None
    rows, windows = [], [0, 0, 0]
    for k, (path, fields) in enumerate(files):
        if k < 2 and not os.path.exists(path):
            rows.append(0)
            continue
        try:
            size = os.path.getsize(path)
        except OSError:
            return None
        data = None
        if size < stream_from:
            data = cdx_dedup._file_bytes(path)
            size = 0 if data is None else len(data)
        if not size:
            return None
        if g is None:
            g = cdx_dedup._dedup()
            g.cdx_begin()
        if data is None:
            verdict, n, stats = g.csv_append_file(path, ','.join(fields), fields.index('url'), window_bytes,
                                                  max_record_bytes)
            windows[k] = stats['windows']
        else:
            verdict, _, n = g.csv_append(data, ','.join(fields), fields.index('url'))
        if verdict != _native.KW_CSV_OK:
            return None
        rows.append(n)
    n_links, _, remaining = g.run_exclude(rows[0] + rows[1])
    b, off, _ = g.remaining()
    return Resume(n_links, rows[0], rows[1], remaining, 'device', arrays=(b, off), windows=tuple(windows))


def remaining_urls(links_csv: str = 'yfin_urls.csv', website: str = 'yfin', success_csv: Optional[str] = None,
                   failed_csv: Optional[str] = None, *, stream_from: int = STREAM_FROM,
                   window_bytes: int = WINDOW_BYTES, max_record_bytes: int = MAX_RECORD_BYTES) -> Resume:
    """constant_rate_scrapper.py:312-360: the links whose URL is in neither the success nor the failed file, with
    the reference's counts (rows, not unique URLs) and its three printed lines."""
    success_csv = success_csv or f"success_articles_{website}.csv"
    failed_csv = failed_csv or f"failed_articles_{website}.csv"
    res = _device_route(links_csv, success_csv, failed_csv, stream_from, window_bytes,
                        max_record_bytes) if native_enabled() else None
    if res is None:
        res = _pandas_route(links_csv, success_csv, failed_csv)
    print(f"Total URLs in CSV: {res.initial_total}")
    print(f"Already scraped (Success + Fails): {res.scraped_success + res.scraped_fails}")
    print(f"Remaining URLs to scrape: {res.remaining}")
    return res
