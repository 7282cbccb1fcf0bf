"""sort_matched_csv on the device (include/kwsort.h; reference match_keywords.py:195-217).

``sort_file(path)`` re-reads one per-ticker CSV file, sorts it by ``time_unix`` and writes it again with the
bytes pandas' ``read_csv`` -> ``sort_values('time_unix')`` -> ``to_csv`` would write -- where that is provably
a permutation of the file's own records (the take rule of kwsort.h): the body goes through a pinned staging
window to the GPU, ``kw_ingest_parse`` tokenizes it, ``kw_sort_keys`` reads the keys and the verdict, the host
makes pandas' own ``np.argsort(keys, kind='quicksort')`` call (ties keep pandas' order), and ``kw_sort_gather``
lays the records out in that order.  No cell is rendered on this route: every other file is refused, untouched,
and stays with ``match_keywords._sort_native`` and pandas.

A body of ``ingest.MAX_WINDOW`` bytes or more does not fit one parse.  It is read in windows through the ingest
handle's two pinned slots (:func:`read_windows`), each window parsed and handed to ``kw_sort_window``, which
gathers the text in a store in device memory; ``kw_sort_finish`` gives the whole file's keys and verdict, and
``kw_sort_gather_slab`` the output slab by slab, written into a sibling temporary file that takes the target's
place after the last slab.  Only a single record that no window holds (``'size'``) and a body that the device's
free memory does not hold (``'memory'``) are refused for their size.

``LAST_STATS`` counts the files by route (``device``: rewritten here, ``unchanged``: found in order here,
``native`` and ``pandas``: the host routes, noted by ``match_keywords.sort_matched_csv``), the refusals by
reason, the bytes the device route took, its summed device times, and the ``windows`` and ``slabs`` of the
files that went in pieces.

``DeviceSorter.sort_indexed`` is the way in for the files a run wrote itself (egress.RunFiles.finish): their
records' lengths are known from the write index and the order is decided on the host, so the body goes to the
store unparsed (``kw_sort_index_begin`` / ``_window`` / ``_finish``) and the same gather lays it out.
``LAST_STATS`` counts those files under ``indexed`` (``index_host``: rewritten by the host branch instead) and
adds their bytes, windows, slabs and times to the entries above.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading
import time
from typing import Dict, Optional

import numpy as np

from . import egress, ingest

SORT_DEVICE_DEFAULT = '1'
FINISH_DEVICE_DEFAULT = '1'
_HEAD_PROBE = 1 << 16              # the header line lies within the file's first bytes, or the file is refused
INGEST_VERDICTS = ('OK', 'NUL', 'UTF8', 'QUOTE', 'CR', 'BLANK', 'FIELDS', 'ROWS')
SORT_VERDICTS = ('OK', 'KEY', 'FORM', 'DTYPE')


WINDOW_BYTES = 256 << 20           # a large file's body goes to the device in windows of this size ...
SLAB_BYTES = 64 << 20              # ... and comes back in slabs of this one (a multiple of 1024)
HEADROOM = 1 << 20                 # the bytes kept free before a window that is read ahead, for the last one's tail


def _new_stats() -> dict:
    return {'device': 0, 'unchanged': 0, 'native': 0, 'pandas': 0, 'indexed': 0, 'index_host': 0, 'refused': {}, 'bytes': 0,
            'gather_bytes': 0,
            'prefetched': 0, 'windows': 0, 'slabs': 0,
            'ms': {'parse': 0.0, 'keys': 0.0, 'scan': 0.0, 'gather': 0.0, 'copies': 0.0},
            'wall_s': {'read': 0.0, 'device': 0.0, 'argsort': 0.0, 'write': 0.0}, 'last': None}


LAST_STATS = _new_stats()


def reset_stats() -> dict:
    global LAST_STATS
    LAST_STATS = _new_stats()
    return LAST_STATS


def note(route: str) -> None:
    """A file that took a host route (``native`` / ``pandas``)."""
    LAST_STATS[route] += 1


def sort_on_device() -> bool:
    """``KW_SORT_DEVICE=0`` keeps every file on the host routes; ``KW_SORT_DEVICE=1`` asks for the device route
    (profiles/e2e_sort.json holds the measurement behind the default)."""
    return os.environ.get('KW_SORT_DEVICE', SORT_DEVICE_DEFAULT) != '0'


def finish_on_device() -> bool:
    """``KW_FINISH_DEVICE=0`` keeps the rewrite of a run's own files (egress.RunFiles.finish) on the host;
    profiles/e2e_finish.json holds the measurement behind the default."""
    return os.environ.get('KW_FINISH_DEVICE', FINISH_DEVICE_DEFAULT) != '0'


# set (``.on = True``) on a thread whose files stay on the host routes: run()'s sharded form (--gpus N)
HOST_ONLY = threading.local()


class Refusal(Exception):
    """A file the windowed route leaves to the host routes: ``reason`` as ``LAST_STATS['refused']`` counts it."""

    def __init__(self, reason: str, keep_last: bool = False):
        super().__init__(reason)
        self.reason, self.keep_last = reason, keep_last


class _Done:
    """The future of a call that ran at once."""

    def __init__(self, value):
        self._value = value

    def result(self):
        return self._value


def read_windows(nbody: int, window_bytes: int, fill, move, parse, submit=None,
                 max_window: int = ingest.MAX_WINDOW) -> int:
    """A body of ``nbody`` bytes through two staging slots, window by window; the windows that gave rows.

    ``fill(slot, at, lo, n)``: the body's bytes [lo, lo + n) into the slot's bytes [at, at + n).
    ``move(src, src_at, dst, dst_at, n)``: n bytes from one slot to the other.
    ``parse(slot, at, n, final, start) -> (n_rows, consumed)``: the window that stands in the slot's bytes
    [at, at + n) is the body's [start, start + n); ``final``: it ends the body.  ``n_rows == 0`` of a window that
    is not final: it holds no complete record.
    ``submit(fn, *args)`` runs ``fill`` on the reader thread and returns its future (None: at once).

    Every window starts where the last one's consumed bytes end, so at a record start.  While a window is with
    ``parse`` the body's next ``window_bytes`` are read ahead into the other slot, behind ``HEADROOM`` free bytes:
    the unconsumed tail is moved in front of them and opens the next window.  A tail that is longer, and a window
    without a complete record, read the next window again from its start, the latter at twice the size; a window
    of ``max_window`` bytes that still holds no record raises ``Refusal('size')``."""
    run = submit if submit is not None else (lambda fn, *a: _Done(fn(*a)))
    head = min(window_bytes, HEADROOM)
    pos, slot, at, n = 0, 0, head, min(window_bytes, nbody)
    fill(slot, at, 0, n)
    ahead = None               # (future, bytes) of the body's bytes after this window, on their way to the other slot
    taken = 0

    def settle():
        nonlocal ahead
        if ahead is not None:
            ahead[0].result()
        ahead = None

    try:
        while True:
            end = pos + n
            final = end == nbody
            if not final and ahead is None:
                m = min(window_bytes, nbody - end)
                ahead = (run(fill, 1 - slot, head, end, m), m)
            n_rows, consumed = parse(slot, at, n, final, pos)
            if n_rows == 0 and not final:
                if n >= max_window:
                    raise Refusal('size')          # a single record that no window holds
                settle()
                slot, at, n = 1 - slot, 0, min(2 * n, max_window, nbody - pos)
                fill(slot, at, pos, n)
                continue
            taken += n_rows > 0
            pos += consumed
            if final:
                return taken
            tail = end - pos
            if ahead is not None and tail <= head:
                m = ahead[1]
                settle()
                move(slot, at + consumed, 1 - slot, head - tail, tail)
                slot, at, n = 1 - slot, head - tail, tail + m
            else:
                settle()
                slot, at, n = 1 - slot, 0, min(max(window_bytes, tail), nbody - pos)
                fill(slot, at, pos, n)
    finally:
        try:
            settle()
        except Exception:   # noqa: BLE001 - the reader is leaving
            pass


class _Job:
    """One file on its way to the device: the header's decisions, the staging slot its body is read into."""

    def __init__(self, path):
        self.path = path
        self.windowed = False          # a body of large_from bytes or more: window by window (DeviceSorter._windowed)
        self.refusal: Optional[str] = None
        self.future = None
        self.dev = self.view = self.names = None
        self.slot = self.pos = self.nbody = 0
        self.head = (b'', b'')         # the header line as the file holds it, and as the csv writer renders it

    def read(self):
        """The body into the staging window (runs on the reader thread: no device call)."""
        t0 = time.perf_counter()
        with open(self.path, 'rb', buffering=0) as fh:
            fh.seek(self.pos)
            mv, got = memoryview(self.view), 0
            while got < self.nbody:
                k = fh.readinto(mv[got:])
                if not k:
                    raise OSError(f'{self.path}: the file shrank while it was read')
                got += k
        return time.perf_counter() - t0


class DeviceSorter:
    """One ``kw_sort`` handle and the ``DeviceIngest`` handles (keyed by the header's shape) of one device and
    host thread.  ``sort_file(path, next_path)`` sorts a file; with ``next_path`` the next file's body is read
    into the other staging slot by a background thread while this one is on the device.

    A body of ``large_from`` bytes or more that does not fit one window of ``window_bytes`` goes to the device window
    by window and comes back in slabs of ``slab_bytes`` (:meth:`_windowed`): pinned host memory stays at two windows
    and two slabs whatever the file's size."""

    def __init__(self, device: int = 0, large_from: int = ingest.MAX_WINDOW, window_bytes: int = WINDOW_BYTES,
                 slab_bytes: int = SLAB_BYTES):
        from . import _native
        if large_from < 0 or large_from > ingest.MAX_WINDOW or window_bytes < 1 or slab_bytes < 1024 or slab_bytes % 1024:
            raise ValueError('large_from in [0, MAX_WINDOW], window_bytes >= 1, slab_bytes a positive multiple of 1024')
        self.large_from = int(large_from)
        self.window_bytes = min(int(window_bytes), ingest.MAX_WINDOW - 2 * HEADROOM)
        self.slab_bytes = min(int(slab_bytes), 1 << 30)
        self._n = _native
        self.device = int(device)
        self.h = None
        self._ingests: Dict[tuple, ingest.DeviceIngest] = {}
        self._slot: Dict[tuple, int] = {}
        self._ahead: Optional[_Job] = None
        self._index_ahead = None       # (path, header bytes, body bytes, slot, bytes read, future): sort_indexed's next file
        self._pool = None
        h = ctypes.c_void_p()
        rc = _native.lib().kw_sort_create(self.device, ctypes.byref(h))
        if rc != _native.KW_OK:
            raise _native.KwError(rc, 'kw_sort_create: no device')
        self.h = h

    def _check(self, rc: int) -> None:
        if rc != self._n.KW_OK:
            msg = self._n.lib().kw_sort_last_error(self.h)
            raise self._n.KwError(rc, msg.decode('utf-8', 'replace') if msg else '')

    # ------------------------------------------------------------------ the header's decisions (no device work)
    def _prepare(self, path: str) -> _Job:
        job = _Job(path)
        size = os.path.getsize(path)
        with open(path, 'rb') as fh:
            head = fh.read(_HEAD_PROBE)
        if size > len(head) and b'\n' not in head:
            job.refusal = 'header'
            return job
        try:
            names, _line, pos = ingest._split_header(head)
        except UnicodeDecodeError:
            job.refusal = 'header'
            return job
        ncols = len(names)
        if ncols == 0:
            job.refusal = 'header-empty'
        elif len(set(names)) != ncols:
            job.refusal = 'header-duplicate'
        elif 'time_unix' not in names:
            job.refusal = 'header-no-time_unix'
        elif ncols < 6 or not all(c in names for c in ingest.NEEDED):
            job.refusal = 'header-columns'
        elif pos >= size:
            job.refusal = 'header-only'
        if job.refusal is None:
            line = egress._join(list(names))
            if line is None:
                job.refusal = 'header'
        if job.refusal is not None:
            return job
        job.names, job.pos, job.nbody = names, pos, size - pos
        job.head = (head[:pos], line.encode('utf-8'))
        key = (ncols, tuple(names.index(c) for c in ingest.NEEDED))
        dev = self._ingests.get(key)
        if dev is None:
            dev = self._ingests[key] = ingest.DeviceIngest(self.device, ncols, key[1])
        job.dev = dev
        # (a body that one window holds takes the whole-body route whatever its size: large_from <= MAX_WINDOW and
        # window_bytes < MAX_WINDOW, so that route never sees a body it cannot stage)
        job.windowed = job.nbody >= self.large_from and job.nbody > self.window_bytes
        if not job.windowed:
            job.slot = self._slot[key] = 1 - self._slot.get(key, 1)
            job.view = dev.stage(job.slot, job.nbody)
        return job

    def _start(self, path: str) -> _Job:
        job = self._prepare(path)
        if job.refusal is None and not job.windowed:   # (a windowed file's reads take both slots: in its own turn)
            if self._pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='kw-sort')
            job.future = self._pool.submit(job.read)
        return job

    def _drop_ahead(self):
        job, self._ahead = self._ahead, None
        if job is not None and job.future is not None:
            try:
                job.future.result()
            except Exception:   # noqa: BLE001 - that file is read again when its turn comes
                pass

    # ------------------------------------------------------------------ the two device calls
    def keys(self, dev: ingest.DeviceIngest, time_col: int, block_rows: int = egress.PANDAS_BLOCK_ROWS):
        """kw_sort_keys over ``dev``'s last parse: ``(verdict, bad_row, bad_col, keys, body_bytes, ascending)``;
        ``keys`` (None unless the verdict is OK) is a view of the handle's pinned buffer, valid until the next call."""
        keys_p, nr, body = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        sv, bad_row, bad_col, asc = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._n.lib().kw_sort_keys(self.h, dev.h, int(time_col), int(block_rows), ctypes.byref(keys_p),
                                               ctypes.byref(nr), ctypes.byref(body), ctypes.byref(sv),
                                               ctypes.byref(bad_row), ctypes.byref(bad_col), ctypes.byref(asc), None))
        keys = None
        if sv.value == self._n.KW_SORT_OK:
            keys = np.frombuffer((ctypes.c_int64 * nr.value).from_address(keys_p.value), dtype=np.int64)
        return sv.value, int(bad_row.value), int(bad_col.value), keys, int(body.value), bool(asc.value)

    def gather(self, order) -> np.ndarray:
        """kw_sort_gather: the body in ``order`` as a uint8 view of the handle's pinned buffer (valid until the
        next gather)."""
        order = np.ascontiguousarray(order, dtype=np.int64)
        out_p, out_n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._n.lib().kw_sort_gather(self.h, self._n.ptr(order), len(order), ctypes.byref(out_p),
                                                 ctypes.byref(out_n)))
        return np.frombuffer((ctypes.c_uint8 * out_n.value).from_address(out_p.value), dtype=np.uint8)

    def last_ms(self) -> dict:
        v = np.zeros(4, dtype=np.float32)
        self._check(self._n.lib().kw_sort_last_ms(self.h, self._n.ptr(v), 4))
        return dict(zip(('keys', 'scan', 'gather', 'copies'), (float(x) for x in v)))

    # ------------------------------------------------------------------ one file
    def sort_file(self, path: str, next_path: Optional[str] = None) -> bool:
        """Sort ``path`` on the device; ``False`` (the file untouched): the file is left to the host routes.
        A ``KW_E*`` error raises ``KwError``, the file untouched."""
        stats = LAST_STATS
        n = self._n
        L = n.lib()
        job = self._ahead
        if job is not None and job.path == path:
            self._ahead = None
            stats['prefetched'] += 1
        else:
            self._drop_ahead()
            job = self._prepare(path)
        try:
            if job.refusal is not None:
                return self._refuse(job.refusal)
            if job.windowed:
                try:
                    return self._windowed(job)
                except Refusal as r:
                    return self._refuse(r.reason, keep_last=r.keep_last)
            stats['wall_s']['read'] += job.future.result() if job.future is not None else job.read()
        finally:
            # the next file's body, into the other slot, while this one is on the device
            if next_path is not None:
                try:
                    self._ahead = self._start(next_path)
                except OSError:   # (that file's own turn reports it)
                    self._ahead = None
        t0 = time.perf_counter()
        dev, nbody = job.dev, job.nbody
        d_text = dev.upload(job.slot, 0, nbody)
        max_rows = int(np.count_nonzero(job.view == 0x0A)) + 1     # (while the upload runs)
        verdict, _bad, n_rows, consumed = dev.parse(d_text, nbody, True, max_rows)
        if verdict != n.KW_INGEST_OK:
            return self._refuse('ingest-' + INGEST_VERDICTS[verdict])
        if n_rows < 1 or consumed != nbody:
            return self._refuse('ingest-EMPTY')
        ms = dev.last_ms()
        sv, bad_row, bad_col, keys, body, asc = self.keys(dev, job.names.index('time_unix'))
        if sv != n.KW_SORT_OK:
            stats['last'] = {'verdict': SORT_VERDICTS[sv], 'row': bad_row, 'col': bad_col}
            return self._refuse('sort-' + SORT_VERDICTS[sv], keep_last=True)
        t1 = time.perf_counter()
        order = None
        if not asc:
            order = np.argsort(keys, kind='quicksort')       # pandas' own call: its order among equal keys
            if (order == np.arange(n_rows)).all():
                order = None
        t2 = time.perf_counter()
        raw_head, head = job.head
        # The file already holds the result when the rows are in order, the header stands as the writer renders
        # it, the body ends with '\n' and holds the records' bytes + 1 each: with the last record terminated every
        # record has a terminator of one byte at least, so the equality leaves no room for a "\r\n" or an empty
        # line.  (Without the last byte's test an extra terminator byte and a missing final '\n' cancel out.)
        if (order is None and raw_head == head and body == nbody and int(job.view[nbody - 1]) == 0x0A):
            self._account(stats, ms, nbody, t0, t1, t2, t2, 'unchanged')
            return True
        if order is None:
            order = np.arange(n_rows, dtype=np.int64)
        out = self.gather(order)
        t3 = time.perf_counter()
        # (the whole body is on the host: only now is the file opened for writing)
        with open(path, 'wb') as fh:
            fh.write(head)
            fh.write(out)
        self._account(stats, ms, nbody, t0, t1, t2, t3, 'device')
        stats['gather_bytes'] += len(out)
        stats['wall_s']['write'] += time.perf_counter() - t3
        return True

    # ------------------------------------------------------------------ a file of several windows
    def begin(self, time_col: int, expect_bytes: int, block_rows: int = egress.PANDAS_BLOCK_ROWS) -> None:
        """kw_sort_begin; ``Refusal('memory')`` where the store does not fit."""
        rc = self._n.lib().kw_sort_begin(self.h, int(time_col), int(block_rows), int(expect_bytes))
        if rc == self._n.KW_EOVERFLOW:
            raise Refusal('memory')
        self._check(rc)

    def window(self, dev: ingest.DeviceIngest, consumed: int) -> None:
        """kw_sort_window over ``dev``'s last parse, which consumed ``consumed`` bytes."""
        self._check(self._n.lib().kw_sort_window(self.h, dev.h, int(consumed), None))

    def finish(self):
        """kw_sort_finish: as :meth:`keys`, over all the windows' rows."""
        keys_p, nr, body = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        sv, bad_row, bad_col, asc = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._n.lib().kw_sort_finish(self.h, ctypes.byref(keys_p), ctypes.byref(nr), ctypes.byref(body),
                                                 ctypes.byref(sv), ctypes.byref(bad_row), ctypes.byref(bad_col),
                                                 ctypes.byref(asc)))
        keys = None
        if sv.value == self._n.KW_SORT_OK:
            keys = np.frombuffer((ctypes.c_int64 * nr.value).from_address(keys_p.value), dtype=np.int64)
        return sv.value, int(bad_row.value), int(bad_col.value), keys, int(body.value), bool(asc.value)

    def gather_begin(self, order, slab_bytes: int):
        """kw_sort_gather_begin: ``(total bytes, slabs)`` of the body in ``order``."""
        order = np.ascontiguousarray(order, dtype=np.int64)
        total, slabs = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._n.lib().kw_sort_gather_begin(self.h, self._n.ptr(order), len(order), int(slab_bytes),
                                                       ctypes.byref(total), ctypes.byref(slabs)))
        return int(total.value), int(slabs.value)

    def gather_slab(self, k: int) -> np.ndarray:
        """kw_sort_gather_slab: slab ``k`` as a uint8 view of a pinned slab of the handle (valid until the next one)."""
        out_p, out_n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._n.lib().kw_sort_gather_slab(self.h, int(k), ctypes.byref(out_p), ctypes.byref(out_n)))
        return np.frombuffer((ctypes.c_uint8 * out_n.value).from_address(out_p.value), dtype=np.uint8)

    def _windowed(self, job: _Job) -> bool:
        """:meth:`sort_file` for a body that goes to the device in windows; raises :class:`Refusal`."""
        stats, n = LAST_STATS, self._n
        dev, nbody, path = job.dev, job.nbody, job.path
        t0 = time.perf_counter()
        self.begin(job.names.index('time_unix'), nbody)
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='kw-sort')
        seen = {'rows': 0, 'last': 0, 'parse_ms': 0.0, 'read_s': 0.0}
        for slot in (0, 1):   # (here, so that the reader thread finds both slots at their size and makes no device call)
            dev.stage(slot, min(self.window_bytes, HEADROOM) + min(self.window_bytes, nbody))
        with open(path, 'rb', buffering=0) as fh:

            def fill(slot, at, lo, k):
                t = time.perf_counter()
                mv, got = memoryview(dev.stage(slot, at + k))[at:at + k], 0
                while got < k:
                    r = os.preadv(fh.fileno(), [mv[got:]], job.pos + lo + got)
                    if not r:
                        raise OSError(f'{path}: the file shrank while it was read')
                    got += r
                seen['read_s'] += time.perf_counter() - t

            def move(src, src_at, dst, dst_at, k):
                dev.stage(dst, dst_at + k)[dst_at:dst_at + k] = dev.stage(src, src_at + k)[src_at:src_at + k]

            def parse(slot, at, k, final, _start):
                view = dev.stage(slot, at + k)[at:at + k]
                d_text = dev.upload(slot, at, k)
                max_rows = int(np.count_nonzero(view == 0x0A)) + 1     # (while the upload runs)
                verdict, _bad, n_rows, consumed = dev.parse(d_text, k, final, max_rows)
                if verdict != n.KW_INGEST_OK:
                    raise Refusal('ingest-' + INGEST_VERDICTS[verdict])
                if final and consumed != k:
                    raise Refusal('ingest-EMPTY')
                seen['parse_ms'] += dev.last_ms()['all']
                if n_rows:
                    self.window(dev, consumed)
                    seen['rows'] += n_rows
                if final:
                    seen['last'] = int(view[k - 1])
                return n_rows, consumed

            stats['windows'] += read_windows(nbody, self.window_bytes, fill, move, parse, self._pool.submit)
        if seen['rows'] < 1:
            raise Refusal('ingest-EMPTY')
        sv, bad_row, bad_col, keys, body, asc = self.finish()
        if sv != n.KW_SORT_OK:
            stats['last'] = {'verdict': SORT_VERDICTS[sv], 'row': bad_row, 'col': bad_col}
            raise Refusal('sort-' + SORT_VERDICTS[sv], keep_last=True)
        t1 = time.perf_counter()
        order = None
        if not asc:
            order = np.argsort(keys, kind='quicksort')       # pandas' own call: its order among equal keys
            if (order == np.arange(len(keys))).all():
                order = None
        t2 = time.perf_counter()
        raw_head, head = job.head
        ms = {'all': seen['parse_ms']}
        stats['wall_s']['read'] += seen['read_s']
        # (the unchanged-file test of sort_file, with the bytes and the last byte the windows added up)
        if order is None and raw_head == head and body == nbody and seen['last'] == 0x0A:
            self._account(stats, ms, nbody, t0, t1, t2, t2, 'unchanged')
            return True
        if order is None:
            order = np.arange(len(keys), dtype=np.int64)
        total, slabs, t_write = self._write_slabs(path, head, order)
        t3 = time.perf_counter()
        self._account(stats, ms, nbody, t0, t1, t2, t3 - t_write, 'device')
        stats['slabs'] += slabs
        stats['gather_bytes'] += total
        stats['wall_s']['write'] += t_write
        return True

    def _write_slabs(self, path: str, head: bytes, order):
        """``head`` and the body in ``order``, slab by slab, into a sibling file that carries the target's mode and
        takes its place after the last slab (removed on any failure): ``(body bytes, slabs, seconds writing)``."""
        import stat
        import tempfile
        total, slabs = self.gather_begin(order, self.slab_bytes)
        mode = stat.S_IMODE(os.stat(path).st_mode)
        fd, tmp = tempfile.mkstemp(prefix='.' + os.path.basename(path) + '.', suffix='.tmp',
                                   dir=os.path.dirname(os.path.abspath(path)))
        t_write = 0.0
        try:
            with os.fdopen(fd, 'wb') as out:
                os.fchmod(out.fileno(), mode)
                out.write(head)
                for k in range(slabs):
                    piece = self.gather_slab(k)
                    t = time.perf_counter()
                    out.write(piece)
                    t_write += time.perf_counter() - t
            os.replace(tmp, path)
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise
        return total, slabs, t_write

    # ------------------------------------------------------------------ a file described by its write index
    def index_begin(self, lens, body_bytes: int) -> None:
        """kw_sort_index_begin; ``Refusal('memory')`` where the store does not fit."""
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        bad = ctypes.c_int64()
        rc = self._n.lib().kw_sort_index_begin(self.h, self._n.ptr(lens), len(lens), int(body_bytes), ctypes.byref(bad))
        if rc == self._n.KW_EOVERFLOW:
            raise Refusal('memory')
        self._check(rc)

    def index_stage(self, slot: int, n_bytes: int) -> np.ndarray:
        """kw_sort_index_stage: the slot's first ``n_bytes`` as a uint8 view, free to be filled."""
        p = ctypes.c_void_p()
        self._check(self._n.lib().kw_sort_index_stage(self.h, int(slot), int(n_bytes), ctypes.byref(p)))
        return np.frombuffer((ctypes.c_uint8 * int(n_bytes)).from_address(p.value), dtype=np.uint8)

    def index_window(self, slot: int, n_bytes: int) -> None:
        self._check(self._n.lib().kw_sort_index_window(self.h, int(slot), int(n_bytes), None))

    def index_finish(self):
        """kw_sort_index_finish: ``(verdict, bad_row)``."""
        v, bad = ctypes.c_int32(), ctypes.c_int64()
        self._check(self._n.lib().kw_sort_index_finish(self.h, ctypes.byref(v), ctypes.byref(bad)))
        return int(v.value), int(bad.value)

    @staticmethod
    def _fill(path: str, at: int, view: np.ndarray) -> float:
        """The file's bytes from ``at`` into ``view`` (runs on the reader thread: no device call); the seconds."""
        t0 = time.perf_counter()
        mv, got = memoryview(view), 0
        with open(path, 'rb', buffering=0) as fh:
            while got < len(mv):
                r = os.preadv(fh.fileno(), [mv[got:]], at + got)
                if not r:
                    raise OSError(f'{path}: the file shrank while it was read')
                got += r
        return time.perf_counter() - t0

    def _drop_index_ahead(self):
        job, self._index_ahead = self._index_ahead, None
        if job is not None:
            try:
                job[-1].result()
            except Exception:   # noqa: BLE001 - that file is read again when its turn comes
                pass

    def sort_indexed(self, path: str, header_len: int, lens, order, next_file=None) -> bool:
        """Rewrite ``path`` -- ``header_len`` bytes of header, then records of ``lens`` bytes each, the terminator
        included -- with its records in ``order``, the header as the file holds it.  The caller has decided that
        this is the sorted file (egress.RunFiles.finish): nothing is parsed.  The body is read through the sort
        handle's two pinned slots, one filled by the reader thread while the other is uploaded.  A body below
        ``large_from`` that one window holds is gathered whole and written in place, the file opened for writing
        only when the whole result is on the host; any other body comes back in slabs, into a sibling temporary
        file that takes the target's place after the last one.  ``next_file``: ``(path, header_len, body bytes)``
        of the file that comes next, whose first window is read while this one is on the device.

        ``False`` (the file untouched): refused -- ``'memory'`` (the store does not fit the device) or
        ``'index-TERM'`` (a record of the index does not end with a line end in the file).  A ``KW_E*`` error
        raises ``KwError``, the file untouched."""
        stats, n = LAST_STATS, self._n
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        order = np.ascontiguousarray(order, dtype=np.int64)
        nbody = int(lens.sum())
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='kw-sort')
        W = self.window_bytes
        t0 = time.perf_counter()
        ahead = self._index_ahead
        if ahead is not None and ahead[:3] == (path, header_len, nbody):
            self._index_ahead = None
            stats['prefetched'] += 1
            slot, k, fut = ahead[3:]
        else:
            self._drop_index_ahead()
            slot, k = 0, min(W, nbody)
            fut = None
        read_s, windows = 0.0, 0
        try:
            try:
                self.index_begin(lens, nbody)
            except Refusal as r:
                return self._refuse(r.reason)
            with open(path, 'rb') as fh:
                head = fh.read(header_len)
            if fut is None:
                fut = self._pool.submit(self._fill, path, header_len, self.index_stage(slot, k))
            pos = 0
            while True:
                read_s += fut.result()
                fut = None
                self.index_window(slot, k)       # (asynchronous: the next read runs beside it)
                windows += 1
                pos += k
                if pos == nbody:
                    break
                slot, k = 1 - slot, min(W, nbody - pos)
                fut = self._pool.submit(self._fill, path, header_len + pos, self.index_stage(slot, k))
            # the next file's first window, into the slot this file's last window left free
            if next_file is not None:
                try:
                    npath, nhead, nbytes = next_file
                    m = min(W, int(nbytes))
                    view = self.index_stage(1 - slot, m)
                    self._index_ahead = (npath, nhead, int(nbytes), 1 - slot, m,
                                         self._pool.submit(self._fill, npath, nhead, view))
                except OSError:   # (that file's own turn reports it)
                    self._index_ahead = None
            verdict, _bad = self.index_finish()
        finally:
            if fut is not None:   # (an error left a read under way)
                try:
                    fut.result()
                except Exception:   # noqa: BLE001 - the route is leaving
                    pass
        stats['wall_s']['read'] += read_s
        if verdict != n.KW_INDEX_OK:
            return self._refuse('index-TERM')
        slabs = 0
        if nbody < self.large_from and nbody <= W:
            out = self.gather(order)
            t2 = time.perf_counter()
            # (the whole body is on the host: only now is the file opened for writing)
            with open(path, 'wb') as fh:
                fh.write(head)
                fh.write(out)
            total, t_write = len(out), time.perf_counter() - t2
        else:
            total, slabs, t_write = self._write_slabs(path, head, order)
        t3 = time.perf_counter()
        stats['indexed'] += 1
        stats['bytes'] += nbody
        stats['windows'] += windows
        stats['slabs'] += slabs
        stats['gather_bytes'] += total
        for name, v in self.last_ms().items():
            stats['ms'][name] += v
        stats['wall_s']['device'] += (t3 - t0) - read_s - t_write
        stats['wall_s']['write'] += t_write
        stats['last'] = {'verdict': 'OK', 'route': 'indexed'}
        return True

    def _account(self, stats, parse_ms, nbody, t0, t1, t2, t3, route):
        stats[route] += 1
        stats['bytes'] += nbody
        stats['ms']['parse'] += parse_ms['all']
        for name, v in self.last_ms().items():
            stats['ms'][name] += v
        stats['wall_s']['device'] += (t1 - t0) + (t3 - t2)
        stats['wall_s']['argsort'] += t2 - t1
        stats['last'] = {'verdict': 'OK', 'route': route}

    @staticmethod
    def _refuse(reason: str, keep_last: bool = False) -> bool:
        ref = LAST_STATS['refused']
        ref[reason] = ref.get(reason, 0) + 1
        if not keep_last:
            LAST_STATS['last'] = {'verdict': reason}
        return False

    def close(self):
        self._drop_ahead()
        self._drop_index_ahead()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        if self.h is not None and self.h.value:
            self._n.lib().kw_sort_destroy(self.h)
        self.h = None
        for dev in self._ingests.values():
            dev.close()
        self._ingests = {}


_SORTER: Optional[DeviceSorter] = None
_AVAILABLE: Optional[bool] = None
_PLAN: Dict[str, str] = {}          # a file run() is about to sort -> the one it sorts next
_PLAN_DEVICE: Optional[int] = None


def plan(paths, device: Optional[int] = None) -> None:
    """The files the caller sorts next, in order, one :func:`sort_file` call each: while one is on the device the
    one after it is read ahead.  :func:`close` forgets the plan."""
    global _PLAN, _PLAN_DEVICE
    paths = list(paths)
    _PLAN = dict(zip(paths, paths[1:]))
    _PLAN_DEVICE = device


def available() -> bool:
    """The library is built and a device answers (decided once a process)."""
    global _AVAILABLE
    if _AVAILABLE is None:
        try:
            from . import _native
            _AVAILABLE = _native.device_count() > 0
        except Exception:   # noqa: BLE001 - no library, no runtime: the host routes
            _AVAILABLE = False
    return _AVAILABLE


def sorter(device: Optional[int] = None) -> Optional[DeviceSorter]:
    """The process's sorter (created on first use, closed by :func:`close` or at exit); ``None``: no device."""
    global _SORTER
    if not available():
        return None
    device = 0 if device is None else int(device)
    if _SORTER is not None and _SORTER.device != device:
        close()
    if _SORTER is None:
        _SORTER = DeviceSorter(device)
    return _SORTER


def close() -> None:
    global _SORTER, _PLAN, _PLAN_DEVICE
    _PLAN, _PLAN_DEVICE = {}, None
    s, _SORTER = _SORTER, None
    if s is not None:
        s.close()


atexit.register(close)


def sort_file(path: str, next_path: Optional[str] = None, device: Optional[int] = None) -> bool:
    """:meth:`DeviceSorter.sort_file` on the process's sorter; ``False`` without a device or the library."""
    if next_path is None:
        next_path = _PLAN.pop(path, None)
    s = sorter(_PLAN_DEVICE if device is None else device)
    if s is None:
        return DeviceSorter._refuse('no-device')
    return s.sort_file(path, next_path)
