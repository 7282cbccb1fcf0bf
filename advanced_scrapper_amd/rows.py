"""Output rows' ``text_matches`` / ``title_matches`` cells built in C from the device hit records.

``assemble_json_rows`` is the write path's form of ``group_hits`` + ``assemble_ticker_matches`` +
``json.dumps`` (match_keywords.py:159-187, :137-138): it returns, in document order and KB ticker order,
``(doc, ticker, text_json, title_json)`` for every (article, ticker) the reference writes a row for.  The
C routine (csrc/kwrows.c, ``lib/libkwrows.so``) applies the period filter on integer epoch-µs bounds
(``kb.period_us``) and writes the JSON text exactly as ``json.dumps`` does.  It returns ``None`` when only
the Python path can answer: a date or period bound without a UTC offset, or an in-period name whose regex
does not compile (the Python path raises the reference's ``re.error``).

``assemble_json_device`` builds the same arrays on the GPU from the records the scan left in HBM
(csrc/kwrows.hip, include/kwrows.h); the host route above stays the fallback.  ``DeviceRows.cells`` + ``emit``
go on from there to the finished CSV lines (csrc/kwemit.hip) without the JSON text reaching the host.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .kb import CompiledKB, epoch_us

_LIB = None
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def _lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'libkwrows.so')
        if not os.path.exists(path):
            raise RuntimeError(f'{path} is missing: run __graft_entry__.build()')
        lib = ctypes.CDLL(path)
        P = ctypes.c_void_p
        lib.kwrows_assemble.restype = ctypes.c_int64
        lib.kwrows_assemble.argtypes = [P, ctypes.c_int64, P, P, ctypes.c_int64, P, P, P, P, P, P, P, P,
                                        ctypes.c_int32, P, P, ctypes.c_int64, P, P, ctypes.c_int64]
        lib.kwrows_assemble_mt.restype = ctypes.c_int64
        lib.kwrows_assemble_mt.argtypes = [P, ctypes.c_int64, P, P, ctypes.c_int64, P, P, P, P, P, P, P, P,
                                           ctypes.c_int32, P, P, ctypes.c_int64, P, P, ctypes.c_int64, P, ctypes.c_int32]
        _LIB = lib
    return _LIB


def _kb_tables(ckb: CompiledKB):
    """Occurrence CSR + JSON keys of a compiled KB (built once per KB), or ``None`` (see module doc)."""
    cached = ckb.__dict__.get('_rows_tables', False)
    if cached is not False:
        return cached
    occ = ckb.occurrences_us()
    if occ is None:
        ckb.__dict__['_rows_tables'] = None
        return None
    flat = [o for lst in occ for o in lst]
    off = np.zeros(len(occ) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(lst) for lst in occ])
    ti = np.array([o[0] for o in flat], dtype=np.int32)
    rank = np.array([o[1] for o in flat], dtype=np.int32)
    lo = np.array([max(o[2], _I64_MIN) for o in flat], dtype=np.int64)
    hi = np.array([min(o[3], _I64_MAX) for o in flat], dtype=np.int64)
    keys = [json.dumps(n).encode('ascii') for n in ckb.names]
    key_off = np.zeros(len(keys) + 1, dtype=np.int64)
    key_off[1:] = np.cumsum([len(k) for k in keys])
    key_buf = np.frombuffer(b''.join(keys) or b'\0', dtype=np.uint8).copy()
    invalid = np.array(ckb.invalid_regex, dtype=np.uint8)
    tables = (off, ti, rank, lo, hi, invalid, key_buf, key_off)
    ckb.__dict__['_rows_tables'] = tables
    return tables


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def assemble_json_rows(ckb: CompiledKB, hits: np.ndarray, dates: Sequence) -> Optional[List[Tuple[int, str, str, str]]]:
    """``[(doc, ticker, text_json, title_json), ...]`` of one chunk, or ``None`` (use the Python path)."""
    raw = assemble_json_raw(ckb, hits, dates)
    if raw is None:
        return None
    row_doc, row_ti, buf, off = raw
    n = len(row_doc)
    text = buf.tobytes().decode('ascii')
    oo = off.tolist()
    tickers = ckb.tickers
    return [(int(row_doc[r]), tickers[row_ti[r]], text[oo[2 * r]:oo[2 * r + 1]], text[oo[2 * r + 1]:oo[2 * r + 2]])
            for r in range(n)]


def _empty():
    return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(1, np.int64))


def date_arrays(dates: Sequence):
    """Per document the article date as epoch microseconds (int64) and whether it exists (uint8), or ``None``
    when a date has no integer form (no UTC offset)."""
    try:
        if hasattr(dates, 'epoch_us_arrays'):            # dates.Dates: integer forms without datetimes
            return dates.epoch_us_arrays()
        n_docs = len(dates)
        date_us = np.zeros(n_docs, dtype=np.int64)
        date_ok = np.zeros(n_docs, dtype=np.uint8)
        for i, d in enumerate(dates):
            if d is not None:
                date_us[i] = epoch_us(d)
                date_ok[i] = 1
        return date_us, date_ok
    except TypeError:
        return None


def assemble_json_device(matcher, dates: Sequence):
    """:func:`assemble_json_raw` of the records of ``matcher``'s last scan, built on the device from the
    records in HBM (csrc/kwrows.hip, ``kw_rows_run`` on ``kw_hits``' pointer): the same four arrays, byte for
    byte.  ``None`` as :func:`assemble_json_raw` (no integer periods or dates, an in-period name whose regex
    does not compile)."""
    tables = _kb_tables(matcher.ckb)
    if tables is None:
        return None
    if len(dates) == 0:
        return _empty()
    prepared = date_arrays(dates)
    if prepared is None:
        return None
    return matcher.rows_device(prepared[0], prepared[1])


def emit_on_device() -> bool:
    """The CSV lines are rendered on the device where that route applies (match_keywords._native_rows):
    the default, ``KW_EMIT_DEVICE=0`` keeps the host emitter (profiles/e2e_emit.json holds the measurement
    behind the default)."""
    return os.environ.get('KW_EMIT_DEVICE', EMIT_DEVICE_DEFAULT) != '0'


EMIT_DEVICE_DEFAULT = '1'


class DeviceRows:
    """One KB's occurrence tables on one GPU (a ``kw_rows`` handle, include/kwrows.h)."""

    def __init__(self, device: int, tables, n_tickers: int):
        off, ti, rank, lo, hi, invalid, key_buf, key_off = tables
        self.h = None
        h = ctypes.c_void_p()
        L = _native.lib()
        rc = L.kw_rows_create(int(device), _ptr(off), _ptr(ti), _ptr(rank), _ptr(lo), _ptr(hi), _ptr(invalid),
                              _ptr(key_buf), _ptr(key_off), len(off) - 1, int(n_tickers), ctypes.byref(h))
        if rc != _native.KW_OK:
            msg = L.kw_rows_last_error(h)
            if h.value:
                L.kw_rows_destroy(h)
            raise _native.KwError(rc, msg.decode() if msg else '')
        self.h = h
        self.n_docs = self.n_rows = 0      # of the last run

    def _check(self, rc: int) -> None:
        if rc != _native.KW_OK:
            msg = _native.lib().kw_rows_last_error(self.h)
            raise _native.KwError(rc, msg.decode('utf-8', 'replace') if msg else '')

    def run(self, d_hits, n_hits: int, date_us: np.ndarray, date_ok: np.ndarray, stream=None, copy_json: bool = True):
        """The four arrays of :func:`assemble_json_raw` for ``n_hits`` device records at ``d_hits`` (a raw
        pointer, or a tensor), or ``None`` on the verdict KW_ROWS_INVALID_REGEX.  ``copy_json=False`` leaves the
        JSON text on the device (for :meth:`emit`): ``(row_doc, row_ti, None, None)``."""
        date_us = np.ascontiguousarray(date_us, dtype=np.int64)
        date_ok = np.ascontiguousarray(date_ok, dtype=np.uint8)
        if len(date_ok) != len(date_us):
            raise ValueError('date_us and date_ok differ in length')
        if not isinstance(d_hits, (int, ctypes.c_void_p)):
            d_hits = _native.ptr(d_hits)
        n_rows, n_bytes, verdict = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        L = _native.lib()
        self._check(L.kw_rows_run(self.h, d_hits, int(n_hits), _ptr(date_us), _ptr(date_ok), len(date_us),
                                  ctypes.byref(n_rows), ctypes.byref(n_bytes), ctypes.byref(verdict), stream))
        self.n_docs, self.n_rows = len(date_us), int(n_rows.value)
        if verdict.value == _native.KW_ROWS_INVALID_REGEX:
            return None
        n = int(n_rows.value)
        row_doc = np.empty(n, dtype=np.int32)
        row_ti = np.empty(n, dtype=np.int32)
        if not copy_json:
            self._check(L.kw_rows_copy_index(self.h, _ptr(row_doc), _ptr(row_ti)))
            return row_doc, row_ti, None, None
        out = np.empty(int(n_bytes.value), dtype=np.uint8)
        out_off = np.empty(2 * n + 1, dtype=np.int64)
        self._check(L.kw_rows_copy(self.h, _ptr(row_doc), _ptr(row_ti), _ptr(out), _ptr(out_off)))
        return row_doc, row_ti, out, out_off

    def cells(self, cells, n_docs: Optional[int] = None, stream=None) -> None:
        """Upload the tokenized cells (an ``ingest.Cells``: ``buf`` / ``off`` / ``flags`` / ``nrows`` / ``ncols``) of
        the chunk's first ``n_docs`` rows (all by default) for :meth:`emit`."""
        n = cells.nrows if n_docs is None else int(n_docs)
        if not 0 <= n <= cells.nrows:
            raise ValueError('n_docs outside the cells')
        nc = n * cells.ncols
        buf = np.ascontiguousarray(cells.buf, dtype=np.uint8)
        off = np.ascontiguousarray(cells.off[:nc + 1], dtype=np.int64)
        fl = np.ascontiguousarray(cells.flags[:nc], dtype=np.uint8)
        if len(off) != nc + 1 or len(fl) != nc or (nc and len(buf) < off[nc]):
            raise ValueError('the cells are shorter than their offsets say')
        self._check(_native.lib().kw_rows_cells(self.h, _ptr(buf), _ptr(off), _ptr(fl), n, int(cells.ncols), stream))

    def cells_device(self, d_cells, d_coff, d_cfl, n_docs: int, ncols: int, stream=None) -> None:
        """:meth:`cells` on device-resident cells (raw pointers, as ``kw_ingest_cells`` gives them): borrowed, they
        must stay valid through the next :meth:`emit`."""
        self._check(_native.lib().kw_rows_cells_device(self.h, d_cells, d_coff, d_cfl, int(n_docs), int(ncols), stream))

    def emit(self, cols, stamp_by_doc, n_rows_use: int, stream=None, d_stamps=None):
        """The first ``n_rows_use`` rows of the last :meth:`run` as CSV lines, rendered on the device from the cells
        of :meth:`cells` (``cols``: their columns of date_time, title, url, source, source_url, article_text;
        ``stamp_by_doc[d]`` = article d's time_unix), in the stable order by KB ticker index: ``(lines, line_off
        int64[n + 1], flags uint32[n], row_doc int32[n], row_ti int32[n], stamps int64[n])``, or ``None`` on the
        verdict KW_EMIT_NUL.  ``lines`` is a memoryview over the handle's pinned buffer, valid until the next
        emit; the arrays are copies.  ``d_stamps``: the stamps of the run's documents in device memory instead (a raw
        pointer to int64[n_docs], e.g. ``kw_ingest_stamps_device``'s; ``kw_rows_emit_stamps_device``: nothing is
        uploaded, ``stamp_by_doc`` is not read)."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        if cols.shape != (6,):
            raise ValueError('cols: six column indexes')
        nb, verdict = ctypes.c_int64(), ctypes.c_int32()
        L = _native.lib()
        if d_stamps is not None:
            self._check(L.kw_rows_emit_stamps_device(self.h, _ptr(cols), d_stamps, self.n_docs, int(n_rows_use),
                                                     ctypes.byref(nb), ctypes.byref(verdict), stream))
        else:
            stamps = np.ascontiguousarray(stamp_by_doc, dtype=np.int64)
            self._check(L.kw_rows_emit(self.h, _ptr(cols), _ptr(stamps), len(stamps), int(n_rows_use), ctypes.byref(nb),
                                       ctypes.byref(verdict), stream))
        if verdict.value == _native.KW_EMIT_NUL:
            return None
        p = [ctypes.c_void_p() for _ in range(6)]
        self._check(L.kw_rows_emit_result(self.h, *[ctypes.byref(x) for x in p]))
        n = int(n_rows_use)

        def arr(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            raw = (ctypes.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr.value)
            return np.frombuffer(raw, dtype=dtype).copy()
        lines = memoryview((ctypes.c_uint8 * int(nb.value)).from_address(p[0].value)).cast('B') if nb.value else memoryview(b'')
        return (lines, arr(p[1], n + 1, np.int64), arr(p[2], n, np.uint32), arr(p[3], n, np.int32),
                arr(p[4], n, np.int32), arr(p[5], n, np.int64))

    def emit_last_ms(self):
        """Device times (ms) of the last emit: order, measure, fill, copy (to the pinned host buffers)."""
        v = np.zeros(4, dtype=np.float32)
        self._check(_native.lib().kw_rows_emit_last_ms(self.h, _ptr(v), 4))
        return dict(zip(('order', 'measure', 'fill', 'copy'), (float(x) for x in v)))

    def last_ms(self):
        """Device times (ms) of the last run: order, expand, render, total."""
        v = np.zeros(4, dtype=np.float32)
        self._check(_native.lib().kw_rows_last_ms(self.h, _ptr(v), 4))
        return dict(zip(('order', 'expand', 'render', 'total'), (float(x) for x in v)))

    def close(self):
        if self.h is not None and self.h.value:
            _native.lib().kw_rows_destroy(self.h)
        self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def assemble_json_raw(ckb: CompiledKB, hits: np.ndarray, dates: Sequence):
    """The rows of :func:`assemble_json_rows` as arrays: (row_doc int32[n], row_ti int32[n] (KB ticker
    index), JSON bytes uint8, offsets int64[2n + 1]: row r's text_matches then title_matches), or ``None``."""
    tables = _kb_tables(ckb)
    if tables is None:
        return None
    n_docs = len(dates)
    if len(hits) == 0 or n_docs == 0:
        return _empty()
    prepared = date_arrays(dates)
    if prepared is None:
        return None
    date_us, date_ok = prepared
    h = np.ascontiguousarray(hits[np.lexsort((hits['pos'], hits['pattern'], hits['field'], hits['doc']))])
    assert h.dtype == _native.HIT_DTYPE
    off, ti, rank, lo, hi, invalid, key_buf, key_off = tables
    from .ingest import host_threads
    row_cap = max(1024, len(h) + len(h) // 2)
    out_cap = max(1 << 16, 48 * len(h))
    need = np.zeros(2, dtype=np.int64)
    for _attempt in range(2):      # -1: the rows / text need more room than guessed (need = the exact sizes)
        row_doc = np.empty(row_cap, dtype=np.int32)
        row_ti = np.empty(row_cap, dtype=np.int32)
        out = np.empty(out_cap, dtype=np.uint8)
        out_off = np.empty(2 * row_cap + 1, dtype=np.int64)
        n = _lib().kwrows_assemble_mt(_ptr(h), len(h), _ptr(date_us), _ptr(date_ok), n_docs, _ptr(off), _ptr(ti),
                                      _ptr(rank), _ptr(lo), _ptr(hi), _ptr(invalid), _ptr(key_buf), _ptr(key_off),
                                      len(ckb.tickers), _ptr(row_doc), _ptr(row_ti), row_cap, _ptr(out),
                                      _ptr(out_off), out_cap, _ptr(need), host_threads())
        if n == -2:
            return None
        if n == -3:
            raise MemoryError('kwrows_assemble: allocation failed')
        if n == -1:
            row_cap, out_cap = int(need[0]) + 1, int(need[1]) + 1
            continue
        break
    else:
        raise RuntimeError('kwrows_assemble: output kept overflowing')
    return row_doc[:n], row_ti[:n], out[:out_off[2 * n]], out_off[:2 * n + 1]
