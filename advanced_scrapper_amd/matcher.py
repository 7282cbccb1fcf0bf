"""Device matcher: arena packing, the libkwmatch handle, and result assembly.

Data flow of one batch of articles:

    str fields --pack_fields--> uint8 arena + int64 offsets (host)
               --torch--> HBM (caller-owned tensors)
               --kw_scan--> per-(doc, field, pattern) records in HBM
               --fetch--> numpy records --assemble_ticker_matches--> the
                  reference's ``ticker_matches`` dicts (match_keywords.py:183-187)

PyTorch is only used to own device memory and streams.
"""
from __future__ import annotations

import ctypes
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .kb import CompiledKB, compile_kb, epoch_us, is_within_period, word_bitmap

ARENA_PAD = 64   # bytes readable past the last field (kw_scan reads 16-B tiles)


# --------------------------------------------------------------------- packing
def field_str(value) -> str:
    """The reference's ``str(v) if v else ""`` (match_keywords.py:150-151)."""
    return str(value) if value else ""


def background_sample(texts: Sequence[str], limit: int = 4 << 20) -> bytes:
    """UTF-8 sample of article text for the anchor statistics (first `limit` bytes)."""
    out, n = [], 0
    for t in texts:
        b = t.encode('utf-8', 'surrogatepass')
        out.append(b)
        n += len(b) + 1
        if n >= limit:
            break
    return b'\n'.join(out)[:limit]


def pack_fields(texts: Sequence[str], titles: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """Interleave text/title UTF-8 into one arena; offsets have 2n+1 entries."""
    n = len(texts)
    if len(titles) != n:
        raise ValueError("texts and titles differ in length")
    parts: List[bytes] = [b''] * (2 * n)
    for i in range(n):
        parts[2 * i] = texts[i].encode('utf-8', 'surrogatepass')
        parts[2 * i + 1] = titles[i].encode('utf-8', 'surrogatepass')
    lens = np.fromiter((len(p) for p in parts), dtype=np.int64, count=2 * n)
    off = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    arena = np.zeros(int(off[-1]) + ARENA_PAD, dtype=np.uint8)
    if off[-1]:
        arena[:off[-1]] = np.frombuffer(b''.join(parts), dtype=np.uint8)
    return arena, off


# --------------------------------------------------------------------- device handle
class GpuMatcher:
    """One compiled knowledge base on one GPU (libkwmatch handle)."""

    def __init__(self, ckb: CompiledKB, device: Optional[int] = None, background: Optional[bytes] = None):
        """``background``: a sample of the article text whose 4-byte statistics
        price the anchor choice (speed only; results never depend on it).

        No torch is needed for the host-buffer methods (:meth:`scan_host`, :meth:`fetch_host`,
        :meth:`match_strings`); the device-tensor methods import it on first use."""
        import sys
        if _native.device_count() == 0:
            raise RuntimeError("GpuMatcher needs a ROCm GPU (no HIP device visible)")
        self.ckb = ckb
        if device is None:
            torch = sys.modules.get('torch')
            device = torch.cuda.current_device() if torch is not None and torch.cuda.is_initialized() else 0
        self.device = int(device)
        L = _native.lib()
        h = ctypes.c_void_p()
        rx = np.ascontiguousarray(ckb.rx_atoms, dtype=np.int32)
        wb = word_bitmap()
        bg = np.frombuffer(background, dtype=np.uint8) if background else np.zeros(0, np.uint8)
        rc = L.kw_compile(_native.ptr(ckb.pat_bytes), _native.ptr(ckb.pat_off), _native.ptr(ckb.pat_class),
                          ckb.n_patterns, _native.ptr(rx) if rx.size else None, _native.ptr(ckb.rx_off),
                          _native.ptr(wb), _native.ptr(bg) if bg.size else None, int(bg.size), self.device,
                          ctypes.byref(h))
        if rc != _native.KW_OK:
            msg = L.kw_last_error(h)
            if h.value:
                L.kw_destroy(h)
            raise _native.KwError(rc, msg.decode() if msg else '')
        self.h = h
        self._keep = None
        self._rows = None         # rows.DeviceRows of this KB, made on first use
        self.rows_copy_json = True  # rows_device copies the JSON text to the host (False: it stays for rows_emit)
        self._fetched = None      # the array the last fetch_host() / fetch() returned

    @property
    def torch(self):
        import torch
        return torch

    @classmethod
    def from_processed_data(cls, processed_data, device=None, background=None) -> "GpuMatcher":
        return cls(compile_kb(processed_data), device, background)

    def close(self):
        if getattr(self, '_rows', None) is not None:
            self._rows.close()
            self._rows = None
        if getattr(self, 'h', None) is not None and self.h.value:
            _native.lib().kw_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- device-resident inputs
    def upload(self, arena: np.ndarray, off: np.ndarray):
        t = self.torch
        dev = t.device('cuda', self.device)
        return (t.from_numpy(arena).to(dev, non_blocking=False), t.from_numpy(off).to(dev, non_blocking=False))

    def scan(self, d_arena, d_off, n_docs: int, stream=None) -> None:
        """Launch kw_scan on device tensors (asynchronous)."""
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device)
        sp = ctypes.c_void_p(stream.cuda_stream) if hasattr(stream, 'cuda_stream') else ctypes.c_void_p(stream)
        self._keep = (d_arena, d_off)
        self._fetched = None
        _native.check(_native.lib().kw_scan(self.h, _native.ptr(d_arena), _native.ptr(d_off), int(n_docs), sp), self.h)

    def n_hits(self) -> int:
        n = ctypes.c_int64()
        p = ctypes.c_void_p()
        _native.check(_native.lib().kw_hits(self.h, ctypes.byref(n), ctypes.byref(p)), self.h)
        return int(n.value)

    def hits_device(self):
        """Records of the last scan as a device tensor [n, 4] (uint32 viewed as int32)."""
        t = self.torch
        n = self.n_hits()
        out = t.empty((max(n, 1), 4), dtype=t.int32, device=t.device('cuda', self.device))
        cnt = ctypes.c_int64()
        st = t.cuda.current_stream(self.device)
        _native.check(_native.lib().kw_hits_copy(self.h, _native.ptr(out), n, ctypes.byref(cnt),
                                                 ctypes.c_void_p(st.cuda_stream)), self.h)
        return out[:n]

    def hits_copy_into(self, dst, stream=None) -> int:
        """Copy the last scan's records into the device tensor ``dst`` ([cap, 4] int32) on ``stream``
        (asynchronous); returns the record count."""
        t = self.torch
        st = stream if stream is not None else t.cuda.current_stream(self.device)
        cnt = ctypes.c_int64()
        _native.check(_native.lib().kw_hits_copy(self.h, _native.ptr(dst), int(dst.shape[0]), ctypes.byref(cnt),
                                                 ctypes.c_void_p(st.cuda_stream)), self.h)
        return int(cnt.value)

    def fetch(self) -> np.ndarray:
        """Records of the last scan on the host (structured HIT_DTYPE array)."""
        self._fetched = records_from_tensor(self.hits_device())
        return self._fetched

    def doc_routes(self, n_docs: int) -> np.ndarray:
        """Per document of the last scan: which kernel finished it (_native.KW_ROUTE_*)."""
        out = np.zeros(max(n_docs, 1), dtype=np.uint8)
        _native.check(_native.lib().kw_doc_routes(self.h, _native.ptr(out), int(n_docs)), self.h)
        return out[:n_docs]

    def doc_items(self, n_docs: int) -> np.ndarray:
        """Per document of the last scan: the probe's items of its text and of its title ([n, 2] uint32)."""
        out = np.zeros((max(n_docs, 1), 2), dtype=np.uint32)
        _native.check(_native.lib().kw_scan_counts(self.h, _native.ptr(out), int(n_docs), None, 0), self.h)
        return out[:n_docs]

    def filter_variant(self) -> int:
        """The stage-1 gate the filter kernel runs for this KB (kw_filter_variant: fk_stage1<0..6>; 4-6 only
        when a background sample made kw_compile choose a box with one more value beside a range)."""
        v = ctypes.c_int32(-1)
        _native.check(_native.lib().kw_filter_variant(self.h, ctypes.byref(v)), self.h)
        return int(v.value)

    TASK_KEYS = ('verify', 'edge', 'short', 'regex', 'regex_early')

    def task_counts(self) -> Dict[str, int]:
        """Task queues of the last scan: ``regions``, and per queue its total and its largest region's count
        (``regex_early``: the regex tasks the epilogue queued, which run beside the verify and short kernels)."""
        v = np.zeros(11, dtype=np.int64)
        _native.check(_native.lib().kw_scan_counts(self.h, None, 0, _native.ptr(v), 11), self.h)
        out = {'regions': int(v[0])}
        for i, k in enumerate(self.TASK_KEYS):
            out[k], out[k + '_max'] = int(v[1 + 2 * i]), int(v[2 + 2 * i])
        return out

    STAT_KEYS = ('candidates', 'anchor_hits', 'lcs_windows', 'verifications', 'deferred_docs', 'deferred_items',
                 'deferred_long_nonascii', 'edge_items', 'candidates_stage2', 'resolved_docs', 'regex_searches',
                 'regex_backtracking', 'regex_rounds', 'deferred_long_run', 'deferred_item_caps', 'deferred_flagged',
                 'big_docs', 'rescans', 'transcoded_docs', 'resolve_fallback_docs', 'rescan_causes')

    def stats(self) -> Dict[str, int]:
        v = np.zeros(_native.KW_N_STATS, dtype=np.int64)
        _native.check(_native.lib().kw_stats(self.h, _native.ptr(v), _native.KW_N_STATS), self.h)
        return {k: int(x) for k, x in zip(self.STAT_KEYS, v)}

    def kernel_times(self) -> Dict[str, float]:
        """Per-kernel device times (ms) of the last scan."""
        keys = ('scan', 'resolve', 'generic', 'compact', 'total', 'filter', 'probe', 'epilogue', 'resolve_kernel', 'tasks')
        v = np.zeros(len(keys), dtype=np.float32)
        _native.check(_native.lib().kw_last_kernel_times(self.h, _native.ptr(v), len(keys)), self.h)
        return dict(zip(keys, (float(x) for x in v)))

    def kernel_ms(self) -> Tuple[float, float, float]:
        """(fast kernel, generic kernel, all kernels incl. compaction) in ms for the last scan."""
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _native.check(_native.lib().kw_last_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                      self.h)
        return float(a.value), float(b.value), float(c.value)

    def match_strings(self, texts: Sequence[str], titles: Sequence[str]) -> np.ndarray:
        """Convenience: pack, scan through the host-buffer entry points, fetch (no torch)."""
        arena, off = pack_fields(texts, titles)
        self.scan_host(arena, off, len(texts))
        return self.fetch_host()

    # -- host buffers (kw_scan_host / kw_hits_host): the drop-in driver's single-GPU path, no torch
    def scan_host(self, arena: np.ndarray, off: np.ndarray, n_docs: int) -> None:
        """Copy a host arena (its padding included) and its 2n+1 offsets to library-owned device buffers and
        scan them (asynchronous until :meth:`fetch_host`)."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(off[:2 * int(n_docs) + 1], dtype=np.int64)
        self._keep = (arena, off)
        self._fetched = None
        _native.check(_native.lib().kw_scan_host(self.h, _native.ptr(arena), int(arena.size), _native.ptr(off),
                                                 int(n_docs)), self.h)

    def scan_ptr(self, d_arena, d_off, n_docs: int, keep=None) -> None:
        """Launch kw_scan on raw device pointers (an ingest.DeviceChunk's arena; ``keep`` is held until the next
        scan) on the default stream: no torch in this path.  Asynchronous until :meth:`fetch_host`."""
        self._keep = keep
        self._fetched = None
        _native.check(_native.lib().kw_scan(self.h, d_arena, d_off, int(n_docs), None), self.h)

    def fetch_host(self) -> np.ndarray:
        """Records of the last scan on the host (structured HIT_DTYPE array)."""
        n = self.n_hits()
        out = np.empty(max(n, 1), dtype=_native.HIT_DTYPE)
        cnt = ctypes.c_int64()
        _native.check(_native.lib().kw_hits_host(self.h, _native.ptr(out), n, ctypes.byref(cnt)), self.h)
        self._fetched = out[:cnt.value]
        return self._fetched

    # -- the per-ticker match cells from the records in HBM (include/kwrows.h)
    def fetched_is(self, hits) -> bool:
        """``hits`` is, unchanged in identity, what the last :meth:`fetch_host` / :meth:`fetch` returned: the
        records of the last scan still in device memory are then these."""
        return hits is not None and hits is self._fetched

    def rows_handle(self):
        """The KB's ``kw_rows`` handle (rows.DeviceRows), or ``None`` when its periods have no integer form."""
        if self._rows is None:
            from . import rows
            tables = rows._kb_tables(self.ckb)
            if tables is None:
                return None
            self._rows = rows.DeviceRows(self.device, tables, len(self.ckb.tickers))
        return self._rows

    def rows_device(self, date_us: np.ndarray, date_ok: np.ndarray):
        """rows.assemble_json_raw's arrays of the last scan's records, built on the device (``None``: an
        in-period name whose regex does not compile, or no integer periods)."""
        handle = self.rows_handle()
        if handle is None:
            return None
        n = ctypes.c_int64()
        p = ctypes.c_void_p()
        _native.check(_native.lib().kw_hits(self.h, ctypes.byref(n), ctypes.byref(p)), self.h)
        return handle.run(p, int(n.value), date_us, date_ok, copy_json=self.rows_copy_json)

    def rows_emit(self, cells, cols, stamp_by_doc: np.ndarray, n_rows_use: int):
        """The first ``n_rows_use`` rows of the last :meth:`rows_device` as CSV lines rendered on the device from
        the chunk's tokenized ``cells`` (rows.DeviceRows.cells + emit; ``None`` on the verdict KW_EMIT_NUL)."""
        handle = self.rows_handle()
        handle.cells(cells, handle.n_docs)
        return handle.emit(cols, np.asarray(stamp_by_doc, dtype=np.int64)[:handle.n_docs], n_rows_use)

    def rows_emit_device(self, chunk, cols, stamp_by_doc, n_rows_use: int, d_stamps=None):
        """:meth:`rows_emit` from the cells of an ingest.DeviceChunk where they lie in device memory
        (``kw_rows_cells_device``: no download, no upload); with ``d_stamps`` (the chunk's stamps in device memory,
        ingest.DeviceChunk.device_stamps) the stamps are read there too and ``stamp_by_doc`` is not."""
        handle = self.rows_handle()
        d_cells, d_coff, d_cfl, _nb = chunk.device_cells()
        handle.cells_device(d_cells, d_coff, d_cfl, handle.n_docs, len(chunk.columns))
        if d_stamps is not None:
            return handle.emit(cols, None, n_rows_use, d_stamps=d_stamps)
        return handle.emit(cols, np.asarray(stamp_by_doc, dtype=np.int64)[:handle.n_docs], n_rows_use)

    def match_device(self, texts: Sequence[str], titles: Sequence[str]):
        """Pack, upload and scan; the records as a device tensor [n, 4] (int32 view of kw_hit)."""
        arena, off = pack_fields(texts, titles)
        d_arena, d_off = self.upload(arena, off)
        self.scan(d_arena, d_off, len(texts))
        return self.hits_device()


def records_from_tensor(t) -> np.ndarray:
    """[n, 4] int32 records (device or host tensor) -> structured HIT_DTYPE array on the host."""
    host = t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)
    return np.ascontiguousarray(host).view(np.uint32).reshape(-1, 4).copy().view(_native.HIT_DTYPE).reshape(-1)


# --------------------------------------------------------------------- host regex positions
def resolve_host_positions(ckb: CompiledKB, hits: np.ndarray, field_text) -> np.ndarray:
    """The records with the positions of the host-resolved names filled in.

    A name with ``ckb.host_regex`` set runs the KW_RX_NOPOS program on the device: every decided (doc, field,
    name) comes back as one KW_NOPOS record.  Each such record is replaced by one record per
    ``re.finditer(name, field)`` position (code-point offsets, match_keywords.py:177-180), and kept when there
    is none.  ``field_text(doc, field)`` gives the field as the reference matched it (field 0 =
    article_text, 1 = title).  Other names' records, invalid-regex names included, pass through; the order
    of the records is kept.
    """
    host = getattr(ckb, 'host_regex', None)
    if hits is None or not len(hits) or not host or not any(host):
        return hits
    host_pat = np.asarray(host, dtype=bool)
    sel = np.flatnonzero(host_pat[hits['pattern']] & (hits['pos'] == _native.KW_NOPOS))
    if not len(sel):
        return hits
    compiled: Dict[int, "re.Pattern"] = {}
    pieces: List[np.ndarray] = []
    prev = 0
    for k in sel.tolist():
        rec = hits[k]
        pat = int(rec['pattern'])
        rx = compiled.get(pat)
        if rx is None:
            rx = compiled[pat] = re.compile(ckb.names[pat])
        pos = [m.start() for m in rx.finditer(field_text(int(rec['doc']), int(rec['field'])))]
        if not pos:
            continue
        pieces.append(hits[prev:k])
        new = np.empty(len(pos), dtype=hits.dtype)
        new[:] = rec
        new['pos'] = pos
        pieces.append(new)
        prev = k + 1
    if not pieces:
        return hits
    pieces.append(hits[prev:])
    return np.concatenate(pieces)


# --------------------------------------------------------------------- assembly
def group_hits(hits: np.ndarray) -> Dict[int, Dict[int, Dict[int, List[int]]]]:
    """doc -> field -> pattern -> sorted positions ([] for a position-less match)."""
    out: Dict[int, Dict[int, Dict[int, List[int]]]] = {}
    if len(hits) == 0:
        return out
    order = np.lexsort((hits['pos'], hits['pattern'], hits['field'], hits['doc']))
    h = hits[order]
    docs = h['doc'].tolist()
    fields = h['field'].tolist()
    pats = h['pattern'].tolist()
    poss = h['pos'].tolist()
    nopos = _native.KW_NOPOS
    for d, f, p, q in zip(docs, fields, pats, poss):
        lst = out.setdefault(d, {}).setdefault(f, {}).setdefault(p, [])
        if q != nopos:
            lst.append(q)
    return out


def _rank_order(d):
    """Items of pattern -> (rank, positions) in rank order (dict order when there is at most one)."""
    return sorted(d.items(), key=lambda kv: kv[1][0]) if len(d) > 1 else d.items()


def assemble_ticker_matches(ckb: CompiledKB, doc_fields: Dict[int, Dict[int, List[int]]], article_date):
    """The reference's per-article ``ticker_matches`` (match_keywords.py:153-187).

    ``doc_fields`` holds the device results of one article (field -> pattern
    -> positions).  Each pattern's (ticker, attribute, name) occurrences are
    filtered by ``is_within_period``; inside a ticker a name takes the dict
    position of its first in-period occurrence.
    """
    if article_date is None:
        return {}
    occ_us = ckb.occurrences_us()
    a_us = None
    if occ_us is not None:
        try:
            a_us = epoch_us(article_date)
        except TypeError:
            a_us = None
    per_ticker: Dict[int, Tuple[dict, dict]] = {}
    for field_idx in (0, 1):
        pats = doc_fields.get(field_idx)
        if not pats:
            continue
        for pat, positions in pats.items():
            best: Dict[int, int] = {}
            if a_us is not None:
                # integer form of is_within_period (kb.epoch_us): exact, no per-occurrence tz conversion
                for (ti, rank, lo, hi) in occ_us[pat]:
                    if lo <= a_us <= hi and ti not in best:
                        best[ti] = rank
            else:
                for (ti, rank, start, end) in ckb.occurrences[pat]:
                    if ti in best:
                        continue   # occurrences are in rank order: the first in-period one wins
                    if is_within_period(article_date, start, end):
                        best[ti] = rank
            if best and ckb.invalid_regex[pat]:
                # the reference's re.finditer(name, s) raises re.error here (:178/:180)
                re.compile(ckb.names[pat])
            for ti, rank in best.items():
                slot = per_ticker.setdefault(ti, ({}, {}))
                slot[field_idx][pat] = (rank, positions)
    result = {}
    for ti in sorted(per_ticker):
        text_d, title_d = per_ticker[ti]
        if not text_d and not title_d:
            continue
        text = {ckb.names[p]: list(v[1]) for p, v in _rank_order(text_d)}
        title = {ckb.names[p]: list(v[1]) for p, v in _rank_order(title_d)}
        result[ckb.tickers[ti]] = {'text': text, 'title': title}
    return result
