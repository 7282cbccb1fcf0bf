"""The process's zone table: what ``time_unix = int(parse(date_time).timestamp())`` (match_keywords.py:131-132)
needs of the local time zone, as arrays (include/kwstamps.h).

A naive datetime's ``timestamp()`` reads it in the process's local zone.  :func:`table` gives that zone as
ascending instants ``at[0..n]`` and UTC offsets ``off[0..n-1]`` (``off[i]`` valid on ``[at[i], at[i+1])``), built in
C by ``kwcsv_zone_table`` from ``localtime_r(...).tm_gmtoff`` -- the libc state Python's own ``time`` module reads
after ``time.tzset()`` -- over 1970-01-01 .. 2100-01-01 UTC: the offset sampled every :data:`STEP_S` seconds, each
change bisected to the second.  A process in UTC (dates.local_zone_is_utc) has one unbounded entry.  A zone with more
than :data:`CAPACITY` entries has no table (``None``): its rows keep the per-row ``timestamp()``.

The table is cached under the zone's identity as the ``time`` module shows it plus ``TZ`` itself, and rebuilt when
that changes (``time.tzset()`` inside one process).  ``KW_STAMPS_NATIVE=0`` switches the native stamps off
everywhere: no table, the routing before them.
"""
from __future__ import annotations

import ctypes
import os
import threading
import time

import numpy as np

CAPACITY = 1024
STEP_S = 21600           # the sampling step: six hours
LAST_BUILD_MS = None     # the wall time of the last build (kwcsv_zone_table alone)

_LOCK = threading.Lock()
_CACHE = {}              # key -> (at, off) or None
_BOUND = False


def stamps_native() -> bool:
    """The native ``time_unix`` is in force (``KW_STAMPS_NATIVE=0``: the routing before it)."""
    return os.environ.get('KW_STAMPS_NATIVE', '1') != '0'


def _key():
    return (os.environ.get('TZ'), time.tzname, time.timezone, time.altzone, time.daylight)


def _bind():
    global _BOUND
    from .ingest import _lib
    L = _lib()
    if not _BOUND:
        P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        L.kwcsv_zone_table.restype = i32
        L.kwcsv_zone_table.argtypes = [i32, i64, P, P, i32]
        L.kwcsv_stamps_local.restype = None
        L.kwcsv_stamps_local.argtypes = [P, P, P, i64, P, P, i32, P, P, i32]
        _BOUND = True
    return L


def build(capacity: int = CAPACITY, step_s: int = STEP_S):
    """``(at int64[n + 1], off int32[n])`` of the zone as libc has it now, or ``None`` when it has more than
    ``capacity`` entries.  The C call runs with the GIL released."""
    global LAST_BUILD_MS
    from .dates import local_zone_is_utc
    L = _bind()
    at = np.zeros(capacity + 1, dtype=np.int64)
    off = np.zeros(capacity, dtype=np.int32)
    t0 = time.perf_counter()
    n = L.kwcsv_zone_table(1 if local_zone_is_utc() else 0, int(step_s), ctypes.c_void_p(at.ctypes.data),
                           ctypes.c_void_p(off.ctypes.data), int(capacity))
    LAST_BUILD_MS = 1e3 * (time.perf_counter() - t0)
    if n < 1:
        return None
    return at[:n + 1].copy(), off[:n].copy()


def table():
    """The current zone's table (cached, see the module doc), or ``None``: the zone is over the capacity, or
    ``KW_STAMPS_NATIVE=0``."""
    if not stamps_native():
        return None
    key = _key()
    with _LOCK:
        if key not in _CACHE:
            _CACHE.clear()                 # one zone at a time
            _CACHE[key] = build()
        return _CACHE[key]


def stamps_local(us, kind, off_s, tab, threads: int = 1):
    """``kwcsv_stamps_local``: ``(stamps int64[n], native uint8[n])`` of date rows under the table ``tab``."""
    L = _bind()
    at, off = tab
    us = np.ascontiguousarray(us, dtype=np.int64)
    kind = np.ascontiguousarray(kind, dtype=np.uint8)
    off_s = np.ascontiguousarray(off_s, dtype=np.int32)
    at = np.ascontiguousarray(at, dtype=np.int64)
    off = np.ascontiguousarray(off, dtype=np.int32)
    n = len(us)
    if len(kind) != n or len(off_s) != n or len(at) != len(off) + 1 or not 1 <= len(off) <= CAPACITY:
        raise ValueError('stamps_local: arrays of one length, a table of 1..%d entries' % CAPACITY)
    stamps = np.zeros(max(n, 1), dtype=np.int64)
    native = np.zeros(max(n, 1), dtype=np.uint8)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)    # noqa: E731
    L.kwcsv_stamps_local(P(us), P(kind), P(off_s), n, P(at), P(off), len(off), P(stamps), P(native), int(threads))
    return stamps[:n], native[:n]
