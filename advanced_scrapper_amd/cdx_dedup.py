"""Drop-in for the CDX link-parts normalise + keep-first dedup of the reference
(yahoo_links_selenium.py:59-82 per part, :160-179 merge), on the GPU.

    process_part(txt_path, csv_path)      :59-82   one yahoo_XY.txt CDX listing -> yahoo_XY.csv
    merge_parts(folder, out='yfin_urls.csv')  :160-179  glob order, concat, keep-first -> yfin_urls.csv
    GpuUrlDedup                           the libkwmatch handle (include/kwdedup.h)

Raw listing bytes in, final CSV bytes out: the file's bytes are uploaded once,
parsed on the device into a UTF-8 URL arena + int64 offsets + int64 timestamps
(csrc/cdx.hip), the rewrite + keep-first runs in HIP kernels (csrc/dedup.hip),
and the kept rows' ``timestamp,url`` lines are rendered on the device; nothing
per row runs on the host.  The device parser is used only where its result
provably equals the reference's pandas call (``read_csv(delimiter=' ',
header=None, usecols=[1, 2])``; the rule: DESIGN.md §7, tests/cdx_rule.py).  Any
other text, and everything under ``KW_CDX_NATIVE=0``, takes the pandas parse +
``to_csv(index=False)`` around the same kernels, so the reference's exceptions
and messages stay as they are and the output files are byte-identical on either
route.  There is no CPU fallback: without a GPU or without libkwmatch.so the
entry points raise.

``python -m advanced_scrapper_amd.cdx_dedup [folder]`` runs the reference's
post-scrape pipeline: every ``yahoo_links_1/*.txt`` -> part CSV, then the merge.
"""
from __future__ import annotations

import ctypes
import glob
import io
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native

ARENA_PAD = 64

# kw_cdx_dialect values (delimiter, ts_col, url_col, skip_lines, exact_fields) of the two texts the reference reads
CDX_DIALECTS = {
    'listing': (ord(' '), 1, 2, 0, 0),   # read_csv(delimiter=' ', header=None, usecols=[1, 2])   (:59)
    'part': (ord(','), 0, 1, 1, 2),      # read_csv(part) under the header line "date_time,url"    (:164-167)
}


def pack_urls(urls: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """UTF-8 arena (padded: readable 64 B past the end, kw_dedup_run needs 32) + int64 offsets (n + 1)."""
    enc = [u.encode('utf-8', 'surrogatepass') for u in urls]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=off[1:])
    arena = np.zeros(int(off[-1]) + ARENA_PAD, dtype=np.uint8)
    if off[-1]:
        arena[:off[-1]] = np.frombuffer(b''.join(enc), dtype=np.uint8)
    return arena, off


class GpuUrlDedup:
    """One libkwmatch dedup handle on one GPU."""

    def __init__(self, device: Optional[int] = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("GpuUrlDedup needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.torch = torch
        self.device = torch.cuda.current_device() if device is None else int(device)
        L = _native.lib()
        h = ctypes.c_void_p()
        rc = L.kw_dedup_create(self.device, ctypes.byref(h))
        if rc != _native.KW_OK:
            raise _native.KwError(rc, L.kw_dedup_last_error(h).decode() if h.value else 'create failed')
        self.h = h

    def close(self):
        if getattr(self, 'h', None) is not None and self.h.value:
            _native.lib().kw_dedup_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != _native.KW_OK:
            raise _native.KwError(rc, _native.lib().kw_dedup_last_error(self.h).decode())

    def upload(self, arena: np.ndarray, off: np.ndarray):
        t = self.torch
        dev = t.device('cuda', self.device)
        return t.from_numpy(arena).to(dev), t.from_numpy(off).to(dev)

    def run(self, d_arena, d_off, n: int, normalize: bool = True, stream=None):
        """Codes (uint8 device tensor, KW_URL_*) of n device-resident rows."""
        t = self.torch
        code = t.empty(max(n, 1), dtype=t.uint8, device=t.device('cuda', self.device))
        if stream is None:
            stream = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_dedup_run(self.h, _native.ptr(d_arena), _native.ptr(d_off), int(n),
                                               _native.KW_DEDUP_NORMALIZE if normalize else 0, _native.ptr(code),
                                               ctypes.c_void_p(stream.cuda_stream)))
        return code[:n]

    def counts(self) -> List[int]:
        c = np.zeros(4, dtype=np.int64)
        self._check(_native.lib().kw_dedup_counts(self.h, _native.ptr(c)))
        return [int(x) for x in c]

    def kept_device(self):
        """(normalised URL bytes, offsets [n_kept + 1], source row indices [n_kept]) of the last run's kept rows,
        dense and in row order, as device tensors."""
        t = self.torch
        nk, nb = ctypes.c_int64(), ctypes.c_int64()
        self._check(_native.lib().kw_dedup_kept_size(self.h, ctypes.byref(nk), ctypes.byref(nb)))
        dev = t.device('cuda', self.device)
        b = t.empty(max(nb.value, 1), dtype=t.uint8, device=dev)
        o = t.empty(nk.value + 1, dtype=t.int64, device=dev)
        r = t.empty(max(nk.value, 1), dtype=t.int64, device=dev)
        st = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_dedup_kept_copy(self.h, _native.ptr(b), _native.ptr(o), _native.ptr(r),
                                                     ctypes.c_void_p(st.cuda_stream)))
        st.synchronize()
        return b[:nb.value], o, r[:nk.value]

    def kept(self) -> Tuple[np.ndarray, List[str]]:
        """(source row indices, normalised URLs) of the last run's kept rows, on the host."""
        b, o, r = self.kept_device()
        hb, ho, hr = b.cpu().numpy().tobytes(), o.cpu().numpy(), r.cpu().numpy()
        urls = [hb[ho[k]:ho[k + 1]].decode('utf-8', 'surrogatepass') for k in range(len(hr))]
        return hr, urls

    def last_ms(self) -> List[float]:
        """Device times (ms) of the last run: transform + hash + table insert, the byte-serial rows, decide,
        kept compaction, total (include/kwdedup.h kw_dedup_last_ms)."""
        v = np.zeros(5, dtype=np.float32)
        self._check(_native.lib().kw_dedup_last_ms(self.h, _native.ptr(v), 5))
        return [float(x) for x in v]

    # ---- raw text in, CSV bytes out (include/kwdedup.h kw_cdx_*; csrc/cdx.hip)
    def cdx_begin(self) -> None:
        """Empty the handle's row store."""
        self._check(_native.lib().kw_cdx_begin(self.h))

    def cdx_text_device(self, data):
        """The text as a device tensor kw_cdx_append takes (16-byte aligned, padded), and its length: bytes-like,
        a uint8 numpy array or a uint8 device tensor."""
        t = self.torch
        dev = t.device('cuda', self.device)
        if isinstance(data, t.Tensor):
            src = data.to(dev).contiguous().view(-1)
        else:
            a = data if isinstance(data, np.ndarray) else np.frombuffer(bytearray(data), dtype=np.uint8)
            src = t.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))
        d = t.empty(src.numel() + ARENA_PAD, dtype=t.uint8, device=dev)
        d[:src.numel()].copy_(src)
        return d, int(src.numel())

    def cdx_append(self, data, dialect='listing') -> Tuple[int, int, int]:
        """Parse one text on the device and append its rows to the store: (verdict KW_CDX_*, offending line or
        -1, rows appended).  Nothing is appended unless the verdict is KW_CDX_OK."""
        t = self.torch
        d_text, n = self.cdx_text_device(data)
        dia = dialect if isinstance(dialect, _native.CdxDialect) else _native.CdxDialect(*CDX_DIALECTS[dialect])
        rows, verdict, bad = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
        st = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_append(self.h, _native.ptr(d_text), n, ctypes.byref(dia), ctypes.byref(rows),
                                                ctypes.byref(verdict), ctypes.byref(bad),
                                                ctypes.c_void_p(st.cuda_stream)))
        return int(verdict.value), int(bad.value), int(rows.value)

    def cdx_rows(self):
        """The store on the host: (URL arena bytes, offsets [n + 1], timestamps [n])."""
        t = self.torch
        n, nb = ctypes.c_int64(), ctypes.c_int64()
        self._check(_native.lib().kw_cdx_rows(self.h, ctypes.byref(n), ctypes.byref(nb)))
        dev = t.device('cuda', self.device)
        a = t.empty(max(nb.value, 1), dtype=t.uint8, device=dev)
        o = t.zeros(n.value + 1, dtype=t.int64, device=dev)
        ts = t.empty(max(n.value, 1), dtype=t.int64, device=dev)
        st = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_store_copy(self.h, _native.ptr(a), _native.ptr(o), _native.ptr(ts),
                                                    ctypes.c_void_p(st.cuda_stream)))
        st.synchronize()
        return a[:nb.value].cpu().numpy().tobytes(), o.cpu().numpy(), ts[:n.value].cpu().numpy()

    def cdx_run(self, normalize: bool = True) -> None:
        """kw_dedup_run over the store; counts() and kept() then describe this run."""
        st = self.torch.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_run(self.h, _native.KW_DEDUP_NORMALIZE if normalize else 0,
                                             ctypes.c_void_p(st.cuda_stream)))

    def cdx_csv(self) -> bytes:
        """The last cdx_run's kept rows as the bytes of ``to_csv(index=False)`` (columns date_time, url),
        rendered on the device."""
        t = self.torch
        st = t.cuda.current_stream(self.device)
        nb = ctypes.c_int64()
        self._check(_native.lib().kw_cdx_csv_size(self.h, ctypes.byref(nb), ctypes.c_void_p(st.cuda_stream)))
        out = t.empty(nb.value + 16, dtype=t.uint8, device=t.device('cuda', self.device))
        self._check(_native.lib().kw_cdx_csv_copy(self.h, _native.ptr(out), ctypes.c_void_p(st.cuda_stream)))
        return out[:nb.value].cpu().numpy().tobytes()

    def cdx_last_ms(self) -> List[float]:
        """Device times (ms): parse and compaction (summed over the appends since cdx_begin), the last render."""
        v = np.zeros(3, dtype=np.float32)
        self._check(_native.lib().kw_cdx_last_ms(self.h, _native.ptr(v), 3))
        return [float(x) for x in v]

    @staticmethod
    def cdx_tile_bytes() -> int:
        return int(_native.lib().kw_cdx_tile_bytes())

    # ---- the scraper's resume filter (include/kwdedup.h kw_csv_append, kw_cdx_run_exclude; resume.py)
    def csv_append(self, data, header: str, url_col: int) -> Tuple[int, int, int]:
        """Parse one quoted CSV text (pandas' default dialect) on the device and append the cells of column
        `url_col` to the store: (verdict KW_CSV_*, the first offender's byte position or -1, rows appended).
        `header` is the file's first line.  Nothing is appended unless the verdict is KW_CSV_OK."""
        t = self.torch
        d_text, n = self.cdx_text_device(data)
        rows, verdict, bad = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
        st = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_csv_append(self.h, _native.ptr(d_text), n, header.encode('utf-8'), int(url_col),
                                                header.count(',') + 1, ctypes.byref(rows), ctypes.byref(verdict),
                                                ctypes.byref(bad), ctypes.c_void_p(st.cuda_stream)))
        return int(verdict.value), int(bad.value), int(rows.value)

    # ---- files of any size: fixed file ranges through two pinned slots, a reader thread one window ahead, two
    # device texts used in turn (include/kwdedup.h kw_csv_stream_*; DESIGN.md §7, "Windowed CSV append")
    def _stream_buffers(self, window_bytes: int, max_record_bytes: int):
        """Two pinned host slots of a window and two device texts of a tail plus a window, kept for the next file
        of the same geometry."""
        t = self.torch
        W, cap = int(window_bytes), (int(window_bytes) + int(max_record_bytes) + ARENA_PAD + 15) & ~15
        have = getattr(self, '_stream_bufs', None)
        if have is None or have[0][0].numel() != W or have[1][0].numel() != cap:
            self._stream_bufs = have = None   # (the old ones go first)
            dev = t.device('cuda', self.device)
            slots = [t.empty(W, dtype=t.uint8, pin_memory=True) for _ in range(2)]
            texts = [t.empty(cap, dtype=t.uint8, device=dev) for _ in range(2)]
            have = self._stream_bufs = (slots, texts)
        return have

    def _stream_mark(self):
        """An event after the work enqueued so far (its ``synchronize`` waits for it)."""
        t = self.torch
        ev = t.cuda.Event()
        ev.record(t.cuda.current_stream(self.device))
        return ev

    def _stream_ptr(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _stream_sync(self) -> None:
        self.torch.cuda.current_stream(self.device).synchronize()

    def _stream_file(self, path: str, window_bytes: int, max_record_bytes: int, take, find_cut: bool = False):
        """The file's ranges [k * window_bytes, (k + 1) * window_bytes) to the device one after the other.  Device
        text k is the unconsumed tail of text k - 1 (copied device-to-device to offset 0, so every text starts
        16-byte aligned) and range k behind it (an async copy from a pinned slot on the current stream); the reader
        thread fills the other slot with range k + 1 meanwhile.  ``take(d_text, n, final, cut) -> consumed`` (a
        negative value stops the stream) is given the text, its bytes, whether it ends the file and, with
        ``find_cut``, the position after the last '\\n' of the text (found on the reader thread).  Returns (stats,
        stopped): stopped is None, the value ``take`` stopped with, or 'record' when a tail outgrew
        ``max_record_bytes``."""
        import concurrent.futures
        import time
        W, R = int(window_bytes), int(max_record_bytes)
        if W < 1 or R < 0:
            raise ValueError('window_bytes >= 1, max_record_bytes >= 0')
        slots, texts = self._stream_buffers(W, R)
        views = [s.numpy() for s in slots]
        size = os.path.getsize(path)
        n_win = max(1, -(-size // W))
        stats = {'windows': 0, 'file_bytes': size, 'read_s': 0.0, 'wait_s': 0.0, 'tail_max': 0, 'consumed': [],
                 'pinned_bytes': 2 * int(slots[0].numel()), 'device_text_bytes': 2 * int(texts[0].numel())}
        fd = os.open(path, os.O_RDONLY)

        def read(k: int):
            t0 = time.perf_counter()
            m = min(W, size - k * W)
            mv, got = memoryview(views[k & 1]), 0
            while got < m:
                g = os.preadv(fd, [mv[got:m]], k * W + got)
                if not g:
                    raise OSError(f'{path}: the file shrank while it was read')
                got += g
            last_nl = -1
            if find_cut:   # (backwards in pieces: the last line end lies near the end)
                hi = m
                while hi > 0 and last_nl < 0:
                    lo = max(0, hi - (1 << 16))
                    hit = np.flatnonzero(views[k & 1][lo:hi] == 0x0A)
                    if len(hit):
                        last_nl = lo + int(hit[-1])
                    hi = lo
            return m, last_nl, time.perf_counter() - t0

        pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
        stopped = None
        copied = [None, None]   # the event after each slot's last copy to the device
        try:
            ahead = pool.submit(read, 0)
            tail = 0
            for k in range(n_win):
                t0 = time.perf_counter()
                m, last_nl, dt = ahead.result()
                stats['wait_s'] += time.perf_counter() - t0
                stats['read_s'] += dt
                # (slot (k + 1) & 1 held range k - 1: its copy has ended before the reader writes there again)
                if copied[(k + 1) & 1] is not None:
                    copied[(k + 1) & 1].synchronize()
                ahead = pool.submit(read, k + 1) if k + 1 < n_win else None
                cur, n = texts[k & 1], tail + m
                if m:
                    cur[tail:n].copy_(slots[k & 1][:m], non_blocking=True)
                    copied[k & 1] = self._stream_mark()
                final = k == n_win - 1
                cut = n if final else (tail + last_nl + 1 if last_nl >= 0 else 0)
                consumed = take(cur, n, final, cut)
                stats['windows'] += 1
                if consumed < 0:
                    stopped = consumed
                    break
                tail = n - consumed
                stats['consumed'].append(consumed)
                stats['tail_max'] = max(stats['tail_max'], tail)
                if final:
                    break
                if tail > R:
                    stopped = 'record'
                    break
                if tail:
                    texts[(k + 1) & 1][:tail].copy_(cur[consumed:n], non_blocking=True)
        finally:
            pool.shutdown(wait=True)   # (the reader has left before anything is raised)
            os.close(fd)
        self._stream_sync()   # (the slots and texts are free for the next file)
        return stats, stopped

    def csv_stream_begin(self, header: str, url_col: int) -> None:
        """kw_csv_stream_begin: open the windowed form of ``csv_append`` over the store as it stands."""
        self._check(_native.lib().kw_csv_stream_begin(self.h, header.encode('utf-8'), int(url_col),
                                                      header.count(',') + 1))

    def csv_stream_window(self, data, final: bool) -> Tuple[int, int, int, int]:
        """kw_csv_stream_window over one window's bytes (as ``csv_append`` takes a text): (verdict, the first
        offender's position in the file or -1, rows appended, consumed)."""
        d_text, n = self.cdx_text_device(data)
        consumed, rows, verdict, bad = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
        st = self.torch.cuda.current_stream(self.device)
        self._check(_native.lib().kw_csv_stream_window(self.h, _native.ptr(d_text), n, 1 if final else 0,
                                                       ctypes.byref(consumed), ctypes.byref(rows), ctypes.byref(verdict),
                                                       ctypes.byref(bad), ctypes.c_void_p(st.cuda_stream)))
        return int(verdict.value), int(bad.value), int(rows.value), int(consumed.value)

    def csv_stream_end(self, commit: bool) -> Tuple[int, int]:
        """kw_csv_stream_end: (KW_CSV_OK, or KW_CSV_ROWS when a committed stream appended no row; the rows that
        stay appended)."""
        total = ctypes.c_int64()
        rc = _native.lib().kw_csv_stream_end(self.h, 1 if commit else 0, ctypes.byref(total))
        if rc == _native.KW_CSV_ROWS:
            return rc, 0
        self._check(rc)
        return _native.KW_CSV_OK, int(total.value)

    def csv_append_file(self, path: str, header: str, url_col: int, window_bytes: int, max_record_bytes: int):
        """``csv_append`` over a file of any size, window by window: (verdict KW_CSV_* or None, rows appended, stats).
        Device memory for text is two windows plus two tails whatever the file's size.  A record that no text of
        ``window_bytes + max_record_bytes`` holds (or a stray quote that swallows the rest) ends the stream with
        nothing appended, verdict None and ``stats['refusal'] == 'record'``: more conservative than the one-piece
        call, never wrong.  ``stats['bad_pos']``: the first offender's position in the file (-1).  A KW_E* error
        or an exception of the reader is raised after the reader thread has been joined; nothing stays appended."""
        L = _native.lib()
        st = self._stream_ptr()
        self._check(L.kw_csv_stream_begin(self.h, header.encode('utf-8'), int(url_col), header.count(',') + 1))
        state = {'verdict': _native.KW_CSV_OK, 'bad': -1}

        def take(d_text, n, final, _cut):
            consumed, rows, verdict, bad = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
            self._check(L.kw_csv_stream_window(self.h, _native.ptr(d_text), n, 1 if final else 0, ctypes.byref(consumed),
                                               ctypes.byref(rows), ctypes.byref(verdict), ctypes.byref(bad),
                                               st))
            if verdict.value != _native.KW_CSV_OK:
                state['verdict'], state['bad'] = int(verdict.value), int(bad.value)
                return -1
            return int(consumed.value)

        try:
            stats, stopped = self._stream_file(path, window_bytes, max_record_bytes, take)
        except BaseException:
            L.kw_csv_stream_end(self.h, 0, None)
            raise
        total = ctypes.c_int64()
        rc = L.kw_csv_stream_end(self.h, 1 if stopped is None else 0, ctypes.byref(total))
        stats['refusal'], stats['bad_pos'] = None, state['bad']
        if stopped == 'record':
            stats['refusal'] = 'record'
            return None, 0, stats
        if stopped is not None:
            return state['verdict'], 0, stats
        if rc == _native.KW_CSV_ROWS:   # (no record after the header: the one-piece call's verdict, at the file's end)
            stats['bad_pos'] = stats['file_bytes']
            return _native.KW_CSV_ROWS, 0, stats
        self._check(rc)
        return _native.KW_CSV_OK, int(total.value), stats

    def cdx_append_file(self, path: str, dialect, window_bytes: int, max_record_bytes: int):
        """``cdx_append`` over a file of any size in a dialect without quotes (the part CSVs): every window is cut on
        the host at its last '\\n', the rest is carried in front of the next, and the header line is skipped once.
        (verdict KW_CDX_* or None, rows appended, stats); a line that no text holds: verdict None and
        ``stats['refusal'] == 'record'``.  Unlike the CSV stream a refused window leaves the earlier windows' rows
        in the store: the caller starts over with ``cdx_begin``."""
        L = _native.lib()
        st = self._stream_ptr()
        base = list(CDX_DIALECTS[dialect])
        state = {'verdict': _native.KW_CDX_OK, 'rows': 0, 'first': True}

        def take(d_text, n, final, cut):
            if cut == 0 and not (final and state['first']):
                return 0
            dia = _native.CdxDialect(*(base[:3] + [base[3] if state['first'] else 0] + base[4:]))
            rows, verdict, bad = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
            self._check(L.kw_cdx_append(self.h, _native.ptr(d_text), cut, ctypes.byref(dia), ctypes.byref(rows),
                                        ctypes.byref(verdict), ctypes.byref(bad), st))
            if verdict.value != _native.KW_CDX_OK:
                state['verdict'] = int(verdict.value)
                return -1
            state['first'] = False
            state['rows'] += int(rows.value)
            return cut

        stats, stopped = self._stream_file(path, window_bytes, max_record_bytes, take, find_cut=True)
        stats['refusal'] = 'record' if stopped == 'record' else None
        if stopped == 'record':
            return None, 0, stats
        if stopped is not None:
            return state['verdict'], 0, stats
        return _native.KW_CDX_OK, state['rows'], stats

    def exclude_distinct_seen(self) -> Tuple[int, int]:
        """After run_exclude: (the distinct URLs among the link rows that were seen, the distinct URLs of the exclude
        rows), the unique-URL counts of experiental/new_links.py."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        st = self.torch.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_exclude_distinct_seen(self.h, ctypes.byref(a), ctypes.byref(b),
                                                               ctypes.c_void_p(st.cuda_stream)))
        return int(a.value), int(b.value)

    def run_exclude(self, n_exclude: int) -> Tuple[int, int, int]:
        """The set difference over the store, whose first `n_exclude` rows are the exclude rows and the rest the
        link rows: (link rows, those whose string is among the exclude rows, those remaining)."""
        st = self.torch.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_run_exclude(self.h, int(n_exclude), ctypes.c_void_p(st.cuda_stream)))
        c = np.zeros(3, dtype=np.int64)
        self._check(_native.lib().kw_cdx_exclude_counts(self.h, _native.ptr(c)))
        return int(c[0]), int(c[1]), int(c[2])

    def exclude_codes(self) -> np.ndarray:
        """The link rows' codes (KW_URL_KEPT / KW_URL_SEEN) of the last run_exclude."""
        t = self.torch
        c = np.zeros(3, dtype=np.int64)
        self._check(_native.lib().kw_cdx_exclude_counts(self.h, _native.ptr(c)))
        code = t.empty(max(int(c[0]), 1), dtype=t.uint8, device=t.device('cuda', self.device))
        st = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_exclude_codes(self.h, _native.ptr(code), ctypes.c_void_p(st.cuda_stream)))
        st.synchronize()
        return code[:int(c[0])].cpu().numpy()

    def remaining(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The last run_exclude's remaining link rows, dense and in row order, on the host: (bytes, offsets
        [n + 1], indices among the link rows [n])."""
        t = self.torch
        nk, nb = ctypes.c_int64(), ctypes.c_int64()
        self._check(_native.lib().kw_cdx_remaining_size(self.h, ctypes.byref(nk), ctypes.byref(nb)))
        dev = t.device('cuda', self.device)
        b = t.empty(max(nb.value, 1), dtype=t.uint8, device=dev)
        o = t.zeros(nk.value + 1, dtype=t.int64, device=dev)
        r = t.empty(max(nk.value, 1), dtype=t.int64, device=dev)
        st = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_remaining_copy(self.h, _native.ptr(b), _native.ptr(o), _native.ptr(r),
                                                        ctypes.c_void_p(st.cuda_stream)))
        st.synchronize()
        return b[:nb.value].cpu().numpy(), o.cpu().numpy(), r[:nk.value].cpu().numpy()

    def exclude_last_ms(self) -> List[float]:
        """Device times (ms) of the last run_exclude: the keep-first run, the set-difference pass, the remaining
        rows' compaction."""
        v = np.zeros(3, dtype=np.float32)
        self._check(_native.lib().kw_cdx_exclude_last_ms(self.h, _native.ptr(v), 3))
        return [float(x) for x in v]

    # ---- the link list's refresh and split (include/kwdedup.h kw_cdx_run_exclude_unique, kw_cdx_csv_select_*; links.py)
    def run_exclude_unique(self, n_exclude: int) -> Tuple[int, int, int, int]:
        """run_exclude that also drops the repeats among the link rows
        (``new[~new.url.isin(prev.url)].drop_duplicates('url')``): (link rows, those seen, those whose first holder
        is an earlier link row, those kept)."""
        st = self.torch.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_run_exclude_unique(self.h, int(n_exclude), ctypes.c_void_p(st.cuda_stream)))
        c = np.zeros(3, dtype=np.int64)
        self._check(_native.lib().kw_cdx_exclude_counts(self.h, _native.ptr(c)))
        d = ctypes.c_int64()
        self._check(_native.lib().kw_cdx_exclude_duplicates(self.h, ctypes.byref(d)))
        return int(c[0]), int(c[1]), int(d.value), int(c[2])

    def selected_ts(self) -> np.ndarray:
        """The timestamps of the last run's surviving rows (cdx_run's kept rows, run_exclude's remaining rows,
        run_exclude_unique's kept rows), in row order, on the host."""
        t = self.torch
        nk, nb = ctypes.c_int64(), ctypes.c_int64()
        self._check(_native.lib().kw_dedup_kept_size(self.h, ctypes.byref(nk), ctypes.byref(nb)))
        ts = t.empty(max(nk.value, 1), dtype=t.int64, device=t.device('cuda', self.device))
        st = t.cuda.current_stream(self.device)
        self._check(_native.lib().kw_cdx_selected_ts(self.h, _native.ptr(ts), ctypes.c_void_p(st.cuda_stream)))
        st.synchronize()
        return ts[:nk.value].cpu().numpy()

    def csv_select(self, order, seg=None) -> List[bytes]:
        """The surviving rows ``order`` (indices among them: any subset, any order) rendered on the device as the
        bytes of ``to_csv(index=False)`` over columns date_time, url; ``seg`` (ascending bounds into ``order``, from
        0 to its length) cuts them into one file per pair of bounds, each with its own header.  A list of the
        files' bytes (one file without ``seg``).  ``order`` and ``seg``: int64 numpy arrays or device tensors."""
        t = self.torch
        dev = t.device('cuda', self.device)

        def on_device(a):
            if isinstance(a, t.Tensor):
                return a.to(device=dev, dtype=t.int64).contiguous().view(-1)
            return t.from_numpy(np.ascontiguousarray(a, dtype=np.int64).reshape(-1)).to(dev)
        d_order = on_device(order)
        n_order = int(d_order.numel())
        d_seg = on_device(np.array([0, n_order], dtype=np.int64) if seg is None else seg)
        n_seg = int(d_seg.numel()) - 1
        if n_seg < 0:
            raise ValueError("csv_select: seg needs at least one bound")
        d_size = t.zeros(max(n_seg, 1), dtype=t.int64, device=dev)
        st = t.cuda.current_stream(self.device)
        nb = ctypes.c_int64()
        self._check(_native.lib().kw_cdx_csv_select_size(self.h, _native.ptr(d_order), n_order, _native.ptr(d_seg), n_seg,
                                                         _native.ptr(d_size), ctypes.byref(nb),
                                                         ctypes.c_void_p(st.cuda_stream)))
        out = t.empty(nb.value + 16, dtype=t.uint8, device=dev)
        self._check(_native.lib().kw_cdx_csv_select_copy(self.h, _native.ptr(out), ctypes.c_void_p(st.cuda_stream)))
        raw = out[:nb.value].cpu().numpy().tobytes()
        cut = np.concatenate([[0], np.cumsum(d_size[:n_seg].cpu().numpy())])
        if int(cut[-1]) != nb.value:
            raise RuntimeError(f"csv_select: the files' sizes sum to {int(cut[-1])}, the total is {nb.value}")
        return [raw[cut[k]:cut[k + 1]] for k in range(n_seg)]

    def select_last_ms(self) -> List[float]:
        """Device times (ms) of the last csv_select: the size pass, the copy pass."""
        v = np.zeros(2, dtype=np.float32)
        self._check(_native.lib().kw_cdx_select_last_ms(self.h, _native.ptr(v), 2))
        return [float(x) for x in v]

    def dedup_strings(self, urls: Sequence[str], normalize: bool = True) -> Tuple[np.ndarray, List[str]]:
        """Pack, upload, classify: (kept row indices, their normalised URLs)."""
        arena, off = pack_urls(urls)
        d_arena, d_off = self.upload(arena, off)
        self.run(d_arena, d_off, len(urls), normalize)
        return self.kept()


_DEDUP: Optional[GpuUrlDedup] = None


def _dedup() -> GpuUrlDedup:
    global _DEDUP
    if _DEDUP is None:
        _DEDUP = GpuUrlDedup()
    return _DEDUP


def read_cdx(path_or_text: str, is_text: bool = False):
    """The reference's parse of a CDX listing (yahoo_links_selenium.py:59)."""
    import pandas as pd
    src = io.StringIO(path_or_text) if is_text else path_or_text
    return pd.read_csv(src, delimiter=' ', header=None, usecols=[1, 2], names=['date_time', 'url'])


def dedup_frame(df, normalize: bool = True):
    """Rows of df (columns date_time, url) the reference keeps, with url rewritten (:63-79)."""
    import pandas as pd
    urls = df['url'].tolist()
    if any(not isinstance(u, str) for u in urls):
        # the reference's str.contains yields NaN there and the boolean mask raises (:63)
        raise ValueError("Cannot mask with non-boolean array containing NA / NaN values")
    rows, new = _dedup().dedup_strings(urls, normalize)
    out = df.iloc[rows].copy()
    out['url'] = new
    return out


def native_enabled() -> bool:
    """The device parse + render route is on unless ``KW_CDX_NATIVE=0`` (then: pandas parse and to_csv, for A/B
    runs and tests).  Output files are byte-identical on either route."""
    return os.environ.get('KW_CDX_NATIVE', '1') != '0'


def _file_bytes(path: str) -> Optional[np.ndarray]:
    try:
        return np.fromfile(path, dtype=np.uint8)
    except (OSError, ValueError):
        return None   # the pandas route raises the reference's error


def _native_part(txt_path: str) -> Optional[bytes]:
    """The part CSV's bytes when the listing is eligible (the rule: DESIGN.md §7), else None."""
    data = _file_bytes(txt_path)
    if data is None:
        return None
    g = _dedup()
    g.cdx_begin()
    verdict, _, rows = g.cdx_append(data, 'listing')
    if verdict != _native.KW_CDX_OK or rows == 0:   # (no rows: left to pandas, which decides what an empty file is)
        return None
    g.cdx_run(normalize=True)
    return g.cdx_csv()


def process_part(txt_path: str, csv_path: str) -> None:
    """yahoo_links_selenium.py:59-82 for one scraped CDX listing."""
    if native_enabled():
        csv = _native_part(txt_path)
        if csv is not None:
            with open(csv_path, 'wb') as fh:
                fh.write(csv)
            return
    dedup_frame(read_cdx(txt_path)).to_csv(csv_path, index=False)


def _native_merge(files: Sequence[str]):
    """(messages of the unreadable parts, parts appended, merged CSV bytes, kept rows) when every readable part
    is eligible, else None.  A part the device parser does not take is read with pandas: one that raises is
    unreadable (skipped, as the reference does), one that reads sends the whole merge down the pandas route."""
    import pandas as pd
    g = None   # (the handle only once a part has bytes: without parts the reference's messages need no GPU)
    errors, parts = [], 0
    for f in files:
        data = _file_bytes(f)
        verdict = -1
        if data is not None and len(data):
            if g is None:
                g = _dedup()
                g.cdx_begin()
            verdict = g.cdx_append(data, 'part')[0]
        if verdict == _native.KW_CDX_OK:
            parts += 1
            continue
        try:
            pd.read_csv(f)
        except Exception as e:
            errors.append(f"Error reading {f}: {e}")
            continue
        return None
    if not parts:
        return errors, 0, b'', 0
    g.cdx_run(normalize=False)
    csv = g.cdx_csv()
    return errors, parts, csv, g.counts()[_native.KW_URL_KEPT]


def merge_parts(folder: str = 'yahoo_links_1', out: str = 'yfin_urls.csv') -> Optional[int]:
    """yahoo_links_selenium.py:160-179: part CSVs in glob order, concat, keep-first."""
    import pandas as pd
    files = glob.glob(os.path.join(folder, '*.csv'))
    res = _native_merge(files) if native_enabled() else None
    if res is not None:
        errors, parts, csv, kept = res
        for line in errors:
            print(line)
        if not parts:
            print("No CSV files were processed. Check if the scraping was successful.")
            return None
        print(f"Found {kept} unique URLs")
        with open(out, 'wb') as fh:
            fh.write(csv)
        print(f"Results saved to {out}")
        return kept
    dfs = []
    for f in files:
        try:
            dfs.append(pd.read_csv(f))
        except Exception as e:  # the reference prints and skips unreadable parts (:168-169)
            print(f"Error reading {f}: {e}")
    if not dfs:
        print("No CSV files were processed. Check if the scraping was successful.")
        return None
    merged = pd.concat(dfs, ignore_index=True)
    merged = dedup_frame(merged, normalize=False)
    print(f"Found {len(merged)} unique URLs")
    merged.to_csv(out, index=False)
    print(f"Results saved to {out}")
    return len(merged)


def main(argv=None) -> None:
    folder = (argv or sys.argv[1:] or ['yahoo_links_1'])[0]
    for txt in sorted(glob.glob(os.path.join(folder, 'yahoo_*.txt'))):
        try:
            process_part(txt, txt[:-len('.txt')] + '.csv')
        except Exception as e:   # the reference prints and goes on (:86-88)
            print(f"Error scraping {txt}: {e}")
    merge_parts(folder)


if __name__ == '__main__':
    main()
