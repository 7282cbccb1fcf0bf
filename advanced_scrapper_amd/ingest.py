"""Article ingest without pandas on the hot path (reference match_keywords.py:230, :150-152).

``read_chunks(path, chunksize)`` yields the article CSV in ``chunksize``-row chunks, like
``pd.read_csv(path, chunksize=...)``.  Each chunk is tokenized by the C tokenizer (csrc/kwcsv.c,
``lib/libkwcsv.so``) into unescaped cell bytes, offsets and per-cell flags; the matcher's byte arena
(text then title of every row, NaN -> ``"nan"``) is packed in C straight from the cells, and the host
only decodes the cells it needs as Python ``str`` (dates of every row, the output cells of matched
rows).  A chunk comes back as a :class:`NativeChunk` when the tokenizer's result provably equals
pandas' for the six columns the path reads -- every record has the header's field count, no
malformed quoting, valid UTF-8, and each needed column holds a cell that keeps it dtype ``object``
(pandas infers dtypes per chunk) -- and otherwise as the ``pandas.DataFrame`` pandas itself parses
from the same bytes, so every consumer sees pandas' values.
"""
from __future__ import annotations

import ctypes
import io
import math
import os
from typing import Iterator, List, Optional, Sequence, Union

import numpy as np
import pandas as pd

NEEDED = ('article_text', 'title', 'date_time', 'url', 'source', 'source_url')
QUOTED, NA, TEXT, CANON = 1, 2, 4, 8

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'libkwcsv.so')
        if not os.path.exists(path):
            raise RuntimeError(f'{path} is missing: run __graft_entry__.build()')
        L = ctypes.CDLL(path)
        P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        L.kwcsv_parse.restype = i64
        L.kwcsv_parse.argtypes = [P, i64, i64, i64, i32, P, P, i32, P, i64, P, P, P, P]
        L.kwcsv_pack.restype = i64
        L.kwcsv_pack.argtypes = [P, P, P, i64, i32, i32, i32, P, i64, P]
        L.kwcsv_utf8_ok.restype = i32
        L.kwcsv_utf8_ok.argtypes = [P, P, P, i64, i32, i32]
        L.kwcsv_records.restype = i64
        L.kwcsv_records.argtypes = [P, i64, i64, i64, i32, P]
        L.kwcsv_parse_mt.restype = i64
        L.kwcsv_parse_mt.argtypes = [P, i64, P, i64, i32, P, P, i32, P, P, P, i32]
        L.kwcsv_utf8_ok_mt.restype = None
        L.kwcsv_utf8_ok_mt.argtypes = [P, P, P, i64, i32, P, i32, P, i32]
        L.kwcsv_pack_mt.restype = i64
        L.kwcsv_pack_mt.argtypes = [P, P, P, i64, i32, i32, i32, P, i64, P, i32]
        L.kwcsv_dates.restype = None
        L.kwcsv_dates.argtypes = [P, P, P, i64, i32, i32, P, P, i32]
        L.kwcsv_dates_iso.restype = None
        L.kwcsv_dates_iso.argtypes = [P, P, P, i64, i32, i32, P, P, P, i32]
        _LIB = L
    return _LIB


def host_threads() -> int:
    """Host threads of the native ingest / egress: the CPUs this process may use (affinity), at most 16, or
    ``KW_HOST_THREADS``."""
    env = os.environ.get('KW_HOST_THREADS')
    if env:
        return max(1, int(env))
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    return max(1, min(16, n))


def _na_table():
    """pandas' own default NA strings (the parser's STR_NA_VALUES) as one byte buffer + offsets."""
    from pandas._libs.parsers import STR_NA_VALUES
    vals = sorted(v.encode('utf-8') for v in STR_NA_VALUES)
    off = np.zeros(len(vals) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in vals])
    return np.frombuffer(b''.join(vals) or b'\0', dtype=np.uint8).copy(), off, len(vals)


def _p(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


class Cells:
    """Tokenized records of one chunk: cell c of row r is ``buf[off[r*ncols+c]:off[r*ncols+c+1]]``."""

    def __init__(self, buf: np.ndarray, off: np.ndarray, flags: np.ndarray, nrows: int, ncols: int):
        self.buf, self.off, self.flags, self.nrows, self.ncols = buf, off, flags, nrows, ncols
        self._mv = memoryview(buf)

    def value(self, r: int, c: int):
        """The cell as pandas gives it in an object column: ``str``, or NaN for an NA string."""
        k = r * self.ncols + c
        if self.flags[k] & NA:
            return math.nan
        return bytes(self._mv[self.off[k]:self.off[k + 1]]).decode('utf-8')

    def column(self, c: int) -> List:
        off = self.off.tolist()
        fl = self.flags.tolist()
        mv, n = self._mv, self.ncols
        out = []
        for r in range(self.nrows):
            k = r * n + c
            out.append(math.nan if fl[k] & NA else bytes(mv[off[k]:off[k + 1]]).decode('utf-8'))
        return out


class NativeChunk:
    """One chunk read by the native tokenizer (the columns the path reads, decoded on demand)."""

    stats = None      # the counters of the read this chunk belongs to (read_chunks_device's; dates() adds dates_slow)

    def __init__(self, cells: Cells, columns: Sequence[str], index0: int):
        self.cells = cells
        self.columns = list(columns)
        self.col = {c: i for i, c in enumerate(self.columns)}
        self.index0 = index0          # row number of the chunk's first row in the file (pandas' index)
        self._cache = {}

    def __len__(self):
        return self.cells.nrows

    def column_list(self, name: str) -> List:
        v = self._cache.get(name)
        if v is None:
            v = self._cache[name] = self.cells.column(self.col[name])
        return v

    def value(self, r: int, name: str):
        v = self._cache.get(name)
        return v[r] if v is not None else self.cells.value(r, self.col[name])

    def arena(self, pad: int = 64):
        """The matcher's arena and 2n+1 offsets (text, title per row; NaN -> "nan")."""
        c = self.cells
        n = c.nrows
        cap = int(c.off[-1]) + 3 * 2 * n + pad
        arena = np.empty(cap, dtype=np.uint8)
        off = np.zeros(2 * n + 1, dtype=np.int64)
        got = _lib().kwcsv_pack_mt(_p(c.buf), _p(c.off), _p(c.flags), n, c.ncols, self.col['article_text'],
                                   self.col['title'], _p(arena), cap - pad, _p(off), host_threads())
        if got < 0:
            raise RuntimeError('kwcsv_pack: arena too small')
        arena[got:got + pad] = 0
        return arena[:got + pad], off

    def dates(self):
        """The reference's per-row ``dateutil.parse(str(v)) if notna(v) else None`` (match_keywords.py:152) of
        the ``date_time`` column up to the first row that raises: (:class:`dates.Dates`, that exception or
        ``None``).  Cells of the ISO rule are parsed in C (kwcsv_dates_iso; with ``KW_DATES_ISO=0`` the 19-byte
        layout alone, kwcsv_dates), the others by dates.parse_date (dateutil)."""
        from .dates import iso_enabled
        c = self.cells
        n = c.nrows
        us = np.empty(max(n, 1), dtype=np.int64)
        kind = np.empty(max(n, 1), dtype=np.uint8)
        off = np.zeros(max(n, 1), dtype=np.int32)
        if iso_enabled():
            _lib().kwcsv_dates_iso(_p(c.buf), _p(c.off), _p(c.flags), n, c.ncols, self.col['date_time'], _p(us),
                                   _p(kind), _p(off), host_threads())
        else:
            _lib().kwcsv_dates(_p(c.buf), _p(c.off), _p(c.flags), n, c.ncols, self.col['date_time'], _p(us), _p(kind),
                               host_threads())
        return _dates_of(us[:n], kind[:n], off[:n], lambda rows: (str(self.value(r, 'date_time')) for r in rows),
                         self.stats)

    def frame(self) -> pd.DataFrame:
        """The chunk as pandas would give it (object columns; for the drop-in process_chunk API)."""
        data = {name: self.column_list(name) for name in self.columns}
        return pd.DataFrame(data, index=pd.RangeIndex(self.index0, self.index0 + len(self)))


def _dates_of(us, kind, off, strings, stats=None):
    """(:class:`dates.Dates`, the first parse error or ``None``) from the date arrays of a chunk's rows
    (kwcsv_dates_iso's or kwcsv_dates').  A kind-3 row with a zero offset becomes kind 0 where dateutil reads such a
    zone as the local one and that is not UTC (dates.zero_offset_is_local, asked on every call); the kind-0 rows
    go through dates.parse_date, ``strings(rows)`` yielding their cells; ``stats['dates_slow']`` (the counters of the
    read the chunk came from, if it keeps any) grows by the rows that went there, the one that raised included."""
    from .dates import Dates, parse_date, zero_offset_is_local
    if zero_offset_is_local():
        back = (kind == 3) & (off == 0)
        if back.any():
            kind[back] = 0
            us[back] = 0
    rows = np.flatnonzero(kind == 0).tolist()
    slow = {}
    for i, (r, s) in enumerate(zip(rows, strings(rows))):
        try:
            slow[r] = parse_date(s)
        except Exception as exc:   # noqa: BLE001 - match_keywords.py:152 raises here for this row
            if stats is not None:
                stats['dates_slow'] = stats.get('dates_slow', 0) + i + 1
            return Dates(us[:r], kind[:r], {k: v for k, v in slow.items() if k < r}, off[:r], stats), exc
    if stats is not None and rows:
        stats['dates_slow'] = stats.get('dates_slow', 0) + len(rows)
    return Dates(us, kind, slow, off, stats), None


def _split_header(buf: bytes):
    """Header fields and the byte position after the header record (simple unquoted or quoted names)."""
    nl = buf.find(b'\n')
    cr = buf.find(b'\r', 0, nl if nl >= 0 else len(buf))    # only within the first line (not the whole file)
    ends = [k for k in (nl, cr) if k >= 0]
    end = min(ends) if ends else len(buf)
    head = bytes(buf[:end]).decode('utf-8')
    pos = end
    if buf[pos:pos + 2] == b'\r\n':
        pos += 2
    elif pos < len(buf):
        pos += 1
    import csv
    names = next(csv.reader([head])) if head else []
    return names, head, pos


def _map(path: str):
    """The file's bytes, memory-mapped read-only (ranks of one node share the page cache; nothing is copied)."""
    import mmap
    with open(path, 'rb') as fh:
        if os.fstat(fh.fileno()).st_size == 0:
            return b''
        return mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)


def read_chunks(path: str, chunksize: int) -> Iterator[Union[NativeChunk, pd.DataFrame]]:
    """Chunks of the article CSV: :class:`NativeChunk` where the fast path equals pandas, else the
    ``DataFrame`` pandas parses from the same rows (see the module doc)."""
    yield from read_chunks_bytes(_map(path), chunksize, path)


def _pandas_rows(data, pos: int, end: int, index0: int, head_end: int) -> pd.DataFrame:
    """pandas on exactly the records in data[pos:end) (dtype inference is per chunk): the header + these bytes."""
    frame = pd.read_csv(io.BytesIO(bytes(data[:head_end]) + bytes(data[pos:end])))
    frame.index = pd.RangeIndex(index0, index0 + len(frame))
    return frame


def _pandas_rest(data, pos: int, chunksize: int, index0: int, head_end: int):
    """A record the tokenizer does not reproduce: pandas takes the rest of the file, chunk by chunk."""
    tail = bytes(data[:head_end]) + bytes(data[pos:])
    for frame in pd.read_csv(io.BytesIO(tail), chunksize=chunksize):
        frame.index = pd.RangeIndex(index0, index0 + len(frame))
        index0 += len(frame)
        yield frame


def _header_ok(names) -> bool:
    return len(names) > 0 and len(set(names)) == len(names) and all(n in names for n in NEEDED)


_NA = None


def _tokenize(buf: np.ndarray, starts: np.ndarray, ncols: int):
    """kwcsv_parse_mt of the records whose starts kwcsv_records found (``starts`` = rows + 1 entries, the last
    = the position after the last record) -> Cells, or None when a record is not reproduced exactly."""
    global _NA
    if _NA is None:
        _NA = _na_table()
    na_buf, na_off, n_na = _NA
    rows = len(starts) - 1
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    out = np.empty(int(starts[-1] - starts[0]) + 16, dtype=np.uint8)     # a record's cells take at most its bytes
    coff = np.empty(rows * ncols + 1, dtype=np.int64)
    cfl = np.empty(max(rows * ncols, 1), dtype=np.uint8)
    got = _lib().kwcsv_parse_mt(_p(buf), len(buf), _p(starts), rows, ncols, _p(na_buf), _p(na_off), n_na, _p(out),
                                _p(coff), _p(cfl), host_threads())
    if got != rows:
        return None
    return Cells(out, coff[:rows * ncols + 1], cfl[:rows * ncols], int(rows), ncols)


def _native_flags(cells: Cells, need_idx) -> np.ndarray:
    """Per needed column: [no text witness among these rows, invalid UTF-8 among them] (0 / 1)."""
    n, nc = cells.nrows, cells.ncols
    fl = cells.flags.reshape(n, nc) if n else np.zeros((0, nc), np.uint8)
    cols = np.asarray(need_idx, dtype=np.int32)
    ok = np.zeros(len(cols), dtype=np.int32)
    _lib().kwcsv_utf8_ok_mt(_p(cells.buf), _p(cells.off), _p(cells.flags), n, nc, _p(cols), len(cols), _p(ok),
                            host_threads())
    out = np.zeros(2 * len(need_idx), dtype=np.int64)
    for k, c in enumerate(need_idx):
        out[2 * k] = 0 if (n and (fl[:, c] & TEXT).any()) else 1
        out[2 * k + 1] = 0 if ok[k] else 1
    return out


def read_chunks_bytes(data, chunksize: int, path: Optional[str] = None) -> Iterator[Union[NativeChunk, pd.DataFrame]]:
    names, head, pos = _split_header(data)
    ncols = len(names)
    if not _header_ok(names):
        yield from pd.read_csv(io.BytesIO(bytes(data)) if path is None else path, chunksize=chunksize)
        return
    need_idx = [names.index(n) for n in NEEDED]
    buf = np.frombuffer(data, dtype=np.uint8)
    head_end = pos
    L = _lib()
    index0 = 0
    starts = np.empty(chunksize + 1, dtype=np.int64)
    while pos < len(data):
        rows = L.kwcsv_records(_p(buf), len(buf), pos, chunksize, ncols, _p(starts))
        if rows == 0:
            break
        if rows < 0:
            yield from _pandas_rest(data, pos, chunksize, index0, head_end)
            return
        end = int(starts[rows])
        cells = _tokenize(buf, starts[:rows + 1], ncols)
        if cells is None:
            yield from _pandas_rest(data, pos, chunksize, index0, head_end)
            return
        if not _native_flags(cells, need_idx).any():
            yield NativeChunk(cells, names, index0)
        else:
            yield _pandas_rows(data, pos, end, index0, head_end)
        index0 += int(rows)
        pos = end


class ShardChunk(NativeChunk):
    """This rank's byte-balanced share [lo, hi) of one chunk's rows (``--gpus N``): its cells only; the chunk
    has ``chunk_rows`` rows starting at file row ``chunk_index0``."""

    def __init__(self, cells: Cells, columns, chunk_index0: int, lo: int, hi: int, chunk_rows: int):
        super().__init__(cells, columns, chunk_index0 + lo)
        self.chunk_index0, self.lo, self.hi, self.chunk_rows = chunk_index0, lo, hi, chunk_rows


def balanced_cuts(starts: np.ndarray, world: int):
    """Contiguous row ranges of ~equal record bytes (starts = rows + 1 record start offsets)."""
    n = len(starts) - 1
    total = float(starts[-1] - starts[0])
    cuts = [0]
    for r in range(1, world):
        cuts.append(int(np.searchsorted(starts[1:], starts[0] + total * r / world, side='left')) + 1)
    cuts.append(n)
    cuts = [min(max(c, 0), n) for c in cuts]
    for i in range(1, len(cuts)):
        cuts[i] = max(cuts[i], cuts[i - 1])
    return [(cuts[i], cuts[i + 1]) for i in range(world)]


def read_chunks_sharded(path: str, chunksize: int, rank: int, world: int, allreduce_min
                        ) -> Iterator[Union[ShardChunk, pd.DataFrame]]:
    """The ``--gpus N`` reader: every rank memory-maps the file and finds each chunk's record boundaries
    (kwcsv_records, no cell copies), then tokenizes only its own byte-balanced share of the chunk's
    records.  Whether the chunk equals pandas' (a text witness in each needed column, valid UTF-8) is
    decided over the whole chunk by ``allreduce_min`` (an element-wise MIN of small int64 vectors over the
    ranks).  Every rank gets the same sequence: a :class:`ShardChunk` (its rows) per native chunk, the
    whole chunk as pandas' DataFrame otherwise."""
    data = _map(path)
    names, head, pos = _split_header(data)
    ncols = len(names)
    if not _header_ok(names):
        yield from pd.read_csv(path, chunksize=chunksize)
        return
    need_idx = [names.index(n) for n in NEEDED]
    buf = np.frombuffer(data, dtype=np.uint8)
    head_end = pos
    L = _lib()
    index0 = 0
    starts = np.empty(chunksize + 1, dtype=np.int64)
    while pos < len(data):
        rows = L.kwcsv_records(_p(buf), len(buf), pos, chunksize, ncols, _p(starts))
        if rows == 0:
            break
        if rows < 0:
            yield from _pandas_rest(data, pos, chunksize, index0, head_end)
            return
        rows = int(rows)
        end = int(starts[rows])
        lo, hi = balanced_cuts(starts[:rows + 1], world)[rank]
        if hi > lo:
            # the share's last record ends where the next share's first begins (blank lines are skipped)
            tok = _tokenize(buf, starts[lo:hi + 1], ncols)
        else:   # no rows on this rank: nothing to witness, nothing invalid
            tok = Cells(np.zeros(16, np.uint8), np.zeros(1, np.int64), np.zeros(1, np.uint8), 0, ncols)
        local = np.zeros(2 * len(need_idx) + 1, dtype=np.int64)
        if tok is None:
            local[-1] = 1
        else:
            local[:-1] = _native_flags(tok, need_idx)
        # witness: some rank has one (MIN of "no witness" = 0); UTF-8 and tokenizing: every rank is fine
        # (MIN of the negated flags, i.e. MAX of the failures, through -x)
        red = allreduce_min(np.concatenate([local[0:-1:2], -local[1:-1:2], -local[-1:]]))
        k = len(need_idx)
        native = not red[:k].any() and not (red[k:] < 0).any()
        if native:
            yield ShardChunk(tok, names, index0, lo, hi, rows)
        else:
            yield _pandas_rows(data, pos, end, index0, head_end)
        index0 += rows
        pos = end


def parse_all(data: bytes):
    """Every record of a whole CSV file: (column names, Cells, record byte spans [n, 2]) or ``None``
    when the tokenizer cannot reproduce pandas' split of the file (the caller falls back to pandas)."""
    names, _head, pos = _split_header(data)
    ncols = len(names)
    if ncols == 0 or len(set(names)) != ncols:
        return None
    na_buf, na_off, n_na = _na_table()
    buf = np.frombuffer(data, dtype=np.uint8)
    # records <= terminators + 1; cells <= bytes
    max_rows = data.count(b'\n') + data.count(b'\r') + 1
    out = np.empty(len(data) + 16, dtype=np.uint8)
    coff = np.empty(max_rows * ncols + 1, dtype=np.int64)
    cfl = np.empty(max(max_rows * ncols, 1), dtype=np.uint8)
    span = np.empty(2 * max_rows + 2, dtype=np.int64)
    newpos = ctypes.c_int64(pos)
    rows = _lib().kwcsv_parse(_p(buf), len(data), pos, max_rows, ncols, _p(na_buf), _p(na_off), n_na, _p(out),
                              len(data) + 16, _p(coff), _p(cfl), ctypes.byref(newpos), _p(span))
    if rows < 0 or newpos.value != len(data):
        return None
    cells = Cells(out, coff[:rows * ncols + 1], cfl[:rows * ncols], int(rows), ncols)
    return names, cells, span[:2 * rows].reshape(-1, 2)


# --------------------------------------------------------------------- the ingest on the device (include/kwingest.h)
INGEST_DEVICE_DEFAULT = '1'
DEFAULT_WINDOW = 32 << 20          # the least bytes of CSV uploaded at once (KW_INGEST_WINDOW sets them)
MAX_WINDOW = (1 << 31) - (1 << 20)
LAST_STATS = None                  # the counters of the last read_chunks_device (its chunks count into them)


def ingest_on_device() -> bool:
    """The article CSV is tokenized on the device where that route applies (match_keywords.run, one GPU):
    ``KW_INGEST_DEVICE=1`` asks for it, ``KW_INGEST_DEVICE=0`` keeps the host tokenizer
    (profiles/e2e_ingest.json holds the measurement behind the default)."""
    return os.environ.get('KW_INGEST_DEVICE', INGEST_DEVICE_DEFAULT) != '0'


class DeviceIngest:
    """One ``kw_ingest`` handle: raw CSV bytes in, the cells, the arena and the dates in device memory."""

    def __init__(self, device: int, ncols: int, cols6: Sequence[int], na=None):
        """``na``: the NA strings as a ``(buf, off, n)`` triple in :func:`_na_table`'s shape (pandas' own by default)."""
        from . import _native
        global _NA
        if na is not None:
            na_buf = np.ascontiguousarray(na[0], dtype=np.uint8)
            na_off = np.ascontiguousarray(na[1], dtype=np.int32)
            n_na = int(na[2])
            if n_na < 0 or len(na_off) < n_na + 1 or len(na_buf) < int(na_off[n_na]):
                raise ValueError('na: (buf, off, n) with n + 1 offsets into buf')
        else:
            if _NA is None:
                _NA = _na_table()
            na_buf, na_off, n_na = _NA
        self._n = _native
        self.h = None
        self.ncols = int(ncols)
        self.cols = np.ascontiguousarray(cols6, dtype=np.int32)
        if self.cols.shape != (6,):
            raise ValueError('cols: six column indexes')
        h = ctypes.c_void_p()
        rc = _native.lib().kw_ingest_create(int(device), self.ncols, _p(self.cols), _p(na_buf), _p(na_off), n_na,
                                            ctypes.byref(h))
        if rc != _native.KW_OK:
            raise _native.KwError(rc, 'kw_ingest_create: bad arguments or no device')
        self.h = h
        self.gen = 0               # parses so far: a DeviceChunk belongs to one
        self.n_rows = 0
        self.zone_key = None       # the table kw_ingest_zone holds (set_zone), None: none
        self._stage = [None, None]

    def _check(self, rc: int) -> None:
        if rc != self._n.KW_OK:
            msg = self._n.lib().kw_ingest_last_error(self.h)
            raise self._n.KwError(rc, msg.decode('utf-8', 'replace') if msg else '')

    def stage(self, slot: int, n_bytes: int) -> np.ndarray:
        """The pinned staging window ``slot`` (0 / 1) as a uint8 array of ``n_bytes``."""
        have = self._stage[slot]
        if have is not None and len(have) >= n_bytes:
            return have[:n_bytes]
        p = ctypes.c_void_p()
        want = min(int(n_bytes) + int(n_bytes) // 8, (1 << 31) - 1)      # (kw_ingest_stage takes less than 2^31)
        self._check(self._n.lib().kw_ingest_stage(self.h, slot, want, ctypes.byref(p)))
        arr = np.frombuffer((ctypes.c_uint8 * max(want, 1)).from_address(p.value), dtype=np.uint8)
        self._stage[slot] = arr
        return arr[:n_bytes]

    def upload(self, slot: int, start: int, n_bytes: int, stream=None):
        """Bytes [start, start + n_bytes) of a staging window to the device text buffer; its device pointer."""
        p = ctypes.c_void_p()
        self._check(self._n.lib().kw_ingest_upload(self.h, slot, int(start), int(n_bytes), ctypes.byref(p), stream))
        return p

    def parse(self, d_text, n_bytes: int, final: bool, max_rows: int, stream=None):
        """kw_ingest_parse: ``(verdict, bad_pos, n_rows, consumed)``."""
        if not isinstance(d_text, (int, ctypes.c_void_p)):
            d_text = self._n.ptr(d_text)
        n_rows, consumed, verdict, bad = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
        self.gen += 1
        self._check(self._n.lib().kw_ingest_parse(self.h, d_text, int(n_bytes), 1 if final else 0, int(max_rows),
                                                  ctypes.byref(n_rows), ctypes.byref(consumed), ctypes.byref(verdict),
                                                  ctypes.byref(bad), stream))
        self.n_rows = int(n_rows.value)
        return int(verdict.value), int(bad.value), self.n_rows, int(consumed.value)

    def cells_device(self):
        """``(d_cells, d_coff, d_cfl, cell_bytes)``: device pointers, valid until the next parse."""
        a, b, c, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._n.lib().kw_ingest_cells(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                  ctypes.byref(n)))
        return a, b, c, int(n.value)

    def arena_device(self):
        """``(d_arena, d_off, arena_bytes)``: device pointers, valid until the next parse."""
        a, b, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._n.lib().kw_ingest_arena(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return a, b, int(n.value)

    def dates(self):
        us = np.zeros(max(self.n_rows, 1), dtype=np.int64)
        kind = np.zeros(max(self.n_rows, 1), dtype=np.uint8)
        self._check(self._n.lib().kw_ingest_dates(self.h, _p(us), _p(kind)))
        return us[:self.n_rows], kind[:self.n_rows]

    def dates_iso(self):
        """kw_ingest_dates_iso: ``(us int64[n], kind uint8[n], off_s int32[n])`` by the ISO rule (include/kwingest.h)."""
        us = np.zeros(max(self.n_rows, 1), dtype=np.int64)
        kind = np.zeros(max(self.n_rows, 1), dtype=np.uint8)
        off = np.zeros(max(self.n_rows, 1), dtype=np.int32)
        self._check(self._n.lib().kw_ingest_dates_iso(self.h, _p(us), _p(kind), _p(off)))
        return us[:self.n_rows], kind[:self.n_rows], off[:self.n_rows]

    def set_zone(self, tab) -> None:
        """kw_ingest_zone: the zone table ``(at, off)`` (zone.table) the parses from now on compute the rows' stamps
        under; ``None`` takes it away.  The same table again is not uploaded twice."""
        key = None if tab is None else (tab[0].tobytes(), tab[1].tobytes())
        if key == self.zone_key:
            return
        if tab is None:
            self._check(self._n.lib().kw_ingest_zone(self.h, None, None, 0))
        else:
            at = np.ascontiguousarray(tab[0], dtype=np.int64)
            off = np.ascontiguousarray(tab[1], dtype=np.int32)
            if len(at) != len(off) + 1:
                raise ValueError('zone table: n + 1 instants for n offsets')
            self._check(self._n.lib().kw_ingest_zone(self.h, _p(at), _p(off), len(off)))
        self.zone_key = key

    def stamps(self):
        """kw_ingest_stamps: ``(stamps int64[n], native uint8[n])`` of the last parse's rows under the handle's zone
        table (include/kwstamps.h); only after a parse that had one."""
        st = np.zeros(max(self.n_rows, 1), dtype=np.int64)
        na = np.zeros(max(self.n_rows, 1), dtype=np.uint8)
        self._check(self._n.lib().kw_ingest_stamps(self.h, _p(st), _p(na)))
        return st[:self.n_rows], na[:self.n_rows]

    def stamps_device(self):
        """kw_ingest_stamps_device: the device pointer of the last parse's stamps, valid until the next parse."""
        p = ctypes.c_void_p()
        self._check(self._n.lib().kw_ingest_stamps_device(self.h, ctypes.byref(p)))
        return p

    def column_flags(self) -> np.ndarray:
        w = np.zeros(6, dtype=np.int32)
        self._check(self._n.lib().kw_ingest_column_flags(self.h, _p(w)))
        return w

    def copy_cells(self) -> Cells:
        n, nc = self.n_rows, self.n_rows * self.ncols
        nb = self.cells_device()[3]
        buf = np.empty(nb + 16, dtype=np.uint8)
        coff = np.empty(nc + 1, dtype=np.int64)
        cfl = np.empty(max(nc, 1), dtype=np.uint8)
        self._check(self._n.lib().kw_ingest_copy_cells(self.h, _p(buf), _p(coff), _p(cfl)))
        return Cells(buf, coff, cfl[:nc], n, self.ncols)

    def copy_arena(self):
        """The matcher's arena (its 64 zero bytes included) and 2n+1 offsets, as :meth:`NativeChunk.arena`."""
        nb = self.arena_device()[2]
        arena = np.empty(nb + 64, dtype=np.uint8)
        off = np.empty(2 * self.n_rows + 1, dtype=np.int64)
        self._check(self._n.lib().kw_ingest_copy_arena(self.h, _p(arena), _p(off)))
        return arena, off

    def copy_column(self, col: int):
        """One column's cells, dense: ``(bytes, off int64[n + 1], flags uint8[n])``."""
        n = self.n_rows
        cap = self.cells_device()[3]
        buf = np.empty(cap + 16, dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.int64)
        fl = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._n.lib().kw_ingest_copy_column(self.h, int(col), _p(buf), cap, _p(off), _p(fl)))
        return buf[:int(off[n])], off, fl[:n]

    def copy_spans(self):
        """The taken records' byte spans in the parsed text: ``(start int64[n], end int64[n])``, the terminator
        excluded (kwcsv_parse's rspan); the text must still stand in device memory."""
        start = np.zeros(max(self.n_rows, 1), dtype=np.int64)
        end = np.zeros(max(self.n_rows, 1), dtype=np.int64)
        self._check(self._n.lib().kw_ingest_copy_spans(self.h, _p(start), _p(end)))
        return start[:self.n_rows], end[:self.n_rows]

    def last_ms(self):
        """Device times (ms) of the last parse: classify, cells, arena (+ dates), all."""
        v = np.zeros(4, dtype=np.float32)
        self._check(self._n.lib().kw_ingest_last_ms(self.h, _p(v), 4))
        return dict(zip(('classify', 'cells', 'arena', 'all'), (float(x) for x in v)))

    def stamps_ms(self) -> float:
        """kw_ingest_last_ms' fifth value: the device time (ms) of the last parse's stamps kernel (0 without a zone
        table; a part of ``arena`` and of ``all``)."""
        v = np.zeros(5, dtype=np.float32)
        self._check(self._n.lib().kw_ingest_last_ms(self.h, _p(v), 5))
        return float(v[4])

    def close(self):
        if self.h is not None and self.h.value:
            self._n.lib().kw_ingest_destroy(self.h)
        self.h = None
        self._stage = [None, None]

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class DeviceChunk(NativeChunk):
    """One chunk tokenized on the device: the cells, the arena and the dates lie in the buffers of a
    :class:`DeviceIngest` until its next parse; the host sees the date arrays, and the cells only when a
    consumer reads them as ``str`` (downloaded once, on first use)."""

    def __init__(self, dev: DeviceIngest, n_rows: int, columns: Sequence[str], index0: int):
        self.dev, self.gen, self.n = dev, dev.gen, int(n_rows)
        self.columns = list(columns)
        self.col = {c: i for i, c in enumerate(self.columns)}
        self.index0 = index0
        self._cache = {}
        self._cells = None

    def _live(self) -> DeviceIngest:
        if self.dev.h is None or self.dev.gen != self.gen:
            raise RuntimeError('the device buffers of this chunk were taken by a later chunk')
        return self.dev

    @property
    def cells(self) -> Cells:
        if self._cells is None:
            self._cells = self._live().copy_cells()
        return self._cells

    def __len__(self):
        return self.n

    def device_arena(self):
        return self._live().arena_device()

    def arena(self, pad: int = 64):
        if pad != 64 or self._cells is not None:
            return super().arena(pad)
        return self._live().copy_arena()

    def device_cells(self):
        return self._live().cells_device()

    def device_stamps(self):
        """The device pointer of the rows' stamps (kw_ingest_stamps_device), while the chunk's buffers stand."""
        return self._live().stamps_device()

    def column_values(self, name: str, limit: Optional[int] = None) -> List:
        """The first ``limit`` cells of one column as pandas gives them (``str`` / NaN), from that column alone."""
        if self._cells is not None:
            return [self._cells.value(r, self.col[name]) for r in range(min(self.n, self.n if limit is None else limit))]
        buf, off, fl = self._live().copy_column(self.col[name])
        mv, o = memoryview(buf), off.tolist()
        k = self.n if limit is None else min(self.n, limit)
        return [math.nan if fl[r] & NA else bytes(mv[o[r]:o[r + 1]]).decode('utf-8') for r in range(k)]

    def dates(self):
        from .dates import iso_enabled
        dev = self._live()
        if iso_enabled():
            us, kind, off = dev.dates_iso()
        else:
            us, kind = dev.dates()
            off = np.zeros(len(kind), dtype=np.int32)

        def strings(rows):
            buf, o, _fl = dev.copy_column(self.col['date_time'])
            mv, o = memoryview(buf), o.tolist()
            return (bytes(mv[o[r]:o[r + 1]]).decode('utf-8') for r in rows)

        dates, error = _dates_of(us, kind, off, strings, self.stats)
        if dev.zone_key is not None:
            # the device's stamps of these rows; native only where the host's kinds still say so (the zero-offset
            # guard and KW_DATES_ISO=0 hand rows back to dateutil)
            st, na = dev.stamps()
            n = len(dates)
            k = dates.kind
            dates.device = (st[:n], (na[:n] != 0) & ((k == 1) | (k == 3) | (k == 4)), self.device_stamps)
        return dates, error


def _host_chunk(data, buf, pos, chunksize, ncols, names, need_idx, index0, head_end, starts):
    """One chunk on the host route, as read_chunks_bytes reads it: (item or None at the end, rows, end); rows < 0:
    pandas takes the rest of the file."""
    rows = _lib().kwcsv_records(_p(buf), len(buf), pos, chunksize, ncols, _p(starts))
    if rows <= 0:
        return None, int(rows), pos
    end = int(starts[rows])
    cells = _tokenize(buf, starts[:rows + 1], ncols)
    if cells is None:
        return None, -2, pos
    if not _native_flags(cells, need_idx).any():
        return NativeChunk(cells, names, index0), int(rows), end
    return _pandas_rows(data, pos, end, index0, head_end), int(rows), end


def read_chunks_device(path: str, chunksize: int, device: int = 0) -> Iterator[Union[NativeChunk, pd.DataFrame]]:
    """:func:`read_chunks` with the tokenizing on the device: a window of the memory-mapped file goes through a
    pinned staging buffer to the GPU once, ``kw_ingest_parse`` takes the next ``chunksize`` records there, and
    the chunk comes back as a :class:`DeviceChunk`.  A window that ends before the chunk does is grown; what a
    window holds beyond the chunk serves the next one; while a chunk is at work a background thread fills the
    other staging buffer.  A chunk the device refuses (the take rule, include/kwingest.h) goes through the host
    route alone, with its own pandas decisions, and the device resumes where that ended; a chunk without a
    text witness in a needed column is parsed by pandas, as on the host route.  ``LAST_STATS`` counts the routes and, as
    ``dates_slow``, the rows of this read's chunks that went to dateutil, as ``stamps_slow`` the rendered documents whose
    ``time_unix`` came from a per-row ``timestamp()`` (a read on the host route keeps no counters).  The rows' stamps
    are computed on the device under the process's zone table (zone.table) as it is when the read starts."""
    global LAST_STATS
    from . import _native
    from concurrent.futures import ThreadPoolExecutor
    stats = LAST_STATS = {'device': 0, 'host': 0, 'pandas': 0, 'grown': 0, 'reused': 0, 'routes': [], 'ms': [],
                          'bytes': 0, 'wall_s': 0.0, 'wall_ms': [], 'dates_slow': 0, 'stamps_slow': 0,
                          'stamps_ms': []}
    data = _map(path)
    names, head, pos = _split_header(data)
    ncols = len(names)
    if not _header_ok(names) or ncols < 6:
        yield from pd.read_csv(path, chunksize=chunksize)
        return
    need_idx = [names.index(n) for n in NEEDED]
    buf = np.frombuffer(data, dtype=np.uint8)
    total = len(buf)
    if pos >= total:       # a header alone: no record, and no device is touched (as on the host route)
        return
    head_end = pos
    index0 = 0
    starts = np.empty(chunksize + 1, dtype=np.int64)
    env = os.environ.get('KW_INGEST_WINDOW')
    if env:
        window = max(64, int(env))
    else:
        # a chunk and a third, from the line ends outside quotes of the first MB (a window that is too small is
        # grown; the later windows follow the chunks' own sizes)
        probe = np.frombuffer(data, dtype=np.uint8, count=min(1 << 20, total - pos), offset=pos)
        inside = np.cumsum(probe == 0x22) & 1
        ends = int(np.count_nonzero((probe == 0x0A) & (inside == 0)))
        per_row = len(probe) / max(1, ends)
        window = int(min(MAX_WINDOW, max(DEFAULT_WINDOW, 1.34 * chunksize * per_row)))
    dev = DeviceIngest(device, ncols, need_idx)
    from . import zone
    dev.set_zone(zone.table())
    pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='kw-ingest')
    import time

    def copy(view, slot, lo, n):
        np.copyto(view, buf[lo:lo + n])     # (releases the GIL)
        return slot, lo, n

    def fill(slot, lo, n):
        return copy(dev.stage(slot, n), slot, lo, n)

    try:
        have = None        # (slot, file position, bytes) of the filled staging window
        ahead = None       # the same, being filled by the background thread
        est = window       # the bytes a chunk is expected to take: the last one's
        while pos < total:
            t0 = time.perf_counter()
            want = window
            verdict = _native.KW_INGEST_OK
            first = True
            while True:
                need = min(want, total - pos)
                rem = have[1] + have[2] - pos if (have is not None and have[1] <= pos < have[1] + have[2]) else 0
                if not (rem >= need or (first and rem >= min(est, total - pos))):
                    got = None
                    if ahead is not None:
                        got = ahead.result()
                        ahead = None
                    if got is not None and got[1] == pos and got[2] >= need:
                        have = got
                    else:
                        have = fill(0 if have is None else 1 - have[0], pos, need)
                first = False
                slot, lo, n = have
                final = lo + n == total
                d_text = dev.upload(slot, pos - lo, lo + n - pos)
                verdict, _bad, n_rows, consumed = dev.parse(d_text, lo + n - pos, final, chunksize)
                if verdict == _native.KW_INGEST_OK and n_rows < chunksize and not final:
                    if lo + n - pos >= want:           # the whole window was not enough: a larger one
                        if want >= MAX_WINDOW:
                            verdict = -1               # no chunk within the largest window: the host route
                            break
                        want = min(2 * want, MAX_WINDOW)
                    stats['grown'] += 1
                    continue
                break
            if verdict != _native.KW_INGEST_OK:
                if ahead is not None:
                    ahead.result()
                    ahead = None
                item, rows, end = _host_chunk(data, buf, pos, chunksize, ncols, names, need_idx, index0, head_end, starts)
                if rows == 0:
                    break
                if rows < 0:
                    stats['routes'].append('pandas-rest')
                    yield from _pandas_rest(data, pos, chunksize, index0, head_end)
                    return
                stats['host'] += 1
                stats['routes'].append('host')
                if isinstance(item, NativeChunk):
                    item.stats = stats
                yield item
                index0 += rows
                pos = end
                continue
            if n_rows == 0:
                break
            end = pos + consumed
            if lo < pos:
                stats['reused'] += 1
            est = consumed
            if not env:
                window = max(DEFAULT_WINDOW, consumed + consumed // 4)
            # the next window, unless this one still holds a chunk's worth beyond `end`
            if end < total and lo + n - end < min(est, total - end) and ahead is None:
                nxt = min(window, total - end)
                ahead = pool.submit(copy, dev.stage(1 - slot, nxt), 1 - slot, end, nxt)
            if dev.column_flags().all():
                stats['device'] += 1
                stats['routes'].append('device')
                stats['ms'].append(dev.last_ms())
                stats['stamps_ms'].append(round(dev.stamps_ms(), 4))
                stats['bytes'] += consumed
                stats['wall_s'] += time.perf_counter() - t0
                stats['wall_ms'].append(round(1e3 * (time.perf_counter() - t0), 3))
                chunk = DeviceChunk(dev, n_rows, names, index0)
                chunk.stats = stats
                yield chunk
            else:
                stats['pandas'] += 1
                stats['routes'].append('pandas')
                yield _pandas_rows(data, pos, end, index0, head_end)
            index0 += n_rows
            pos = end
    finally:
        if ahead is not None:
            try:
                ahead.result()
            except Exception:   # noqa: BLE001 - the reader is leaving
                pass
        pool.shutdown(wait=True)
        dev.close()
