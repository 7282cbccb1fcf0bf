"""Article date parsing for the period filter and ``time_unix`` (match_keywords.py:131,152).

The reference calls ``dateutil.parser.parse(str(date_time))`` once per article
(:152) and again per output row (:131): tens of microseconds each, which at
GPU scan rates is the host's largest per-article cost.  The scraped dataset's
``date_time`` cells are ISO-8601: ``YYYY-MM-DD HH:MM:SS``,
or what the scraper stores verbatim from ``<time datetime=…>``, with a fraction
and a zone (``2023-06-05T14:23:11.000Z``).  The ISO rule (include/kwingest.h,
tests/dates_rule.py) names the cells parsed directly:

    YYYY-MM-DD[ T]HH:MM:SS ( '.' 1-9 digits )? ( 'Z' | [+-]HH ( ':'? MM )? )?

with ASCII digits, year >= 1000, valid calendar fields, offset HH <= 23 and
MM <= 59.  For such a string dateutil returns those fields, the fraction's
first six digits as microseconds and the zone as a fixed offset, which is what
the fast path builds; the ``tzinfo`` is dateutil's own object for that offset
(one real dateutil call per distinct offset, cached).  Every other string goes
to dateutil itself, so results (and exceptions) are dateutil's by construction.

The zero-offset guard.  Whenever ``'UTC' in time.tzname`` dateutil answers
``Z`` and a zero offset with ``tzlocal()``: the same instant in a UTC process,
hours off under a zone that is merely *named* UTC (``TZ=UTC+5``).  The
reference inherits that, so such cells go to dateutil there
(:func:`zero_offset_is_local`, checked on every call: ``TZ`` may change).

``KW_DATES_ISO=0`` keeps the 19-byte layout as the only direct one, here and in
the ingest (the A/B baseline, and an escape hatch).
"""
from __future__ import annotations

import os
import re
import time
from datetime import datetime, timedelta

import numpy as np
from dateutil import parser as _dparser

_ISO = re.compile(r'([0-9]{4})-([0-9]{2})-([0-9]{2})[ T]([0-9]{2}):([0-9]{2}):([0-9]{2})'
                  r'(?:\.([0-9]{1,9}))?(?:(Z)|([+-])([0-9]{2})(?::?([0-9]{2}))?)?')
_ISO19 = re.compile(r'(\d{4})-(\d{2})-(\d{2})[ T](\d{2}):(\d{2}):(\d{2})')      # KW_DATES_ISO=0: the 19-byte layout alone
_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
STAMP_BOUND = 1 << 52      # below it (and from 0) a date with a fraction has int(timestamp()) == us // 10**6


def iso_enabled() -> bool:
    """The ISO rule is in force (``KW_DATES_ISO=0``: the 19-byte layout alone, as before it)."""
    return os.environ.get('KW_DATES_ISO', '1') != '0'


def local_zone_is_utc() -> bool:
    """The process's local time zone is UTC without transitions (``time.timezone == time.altzone == 0``, no
    DST, zone name UTC/UCT/GMT): then a naive datetime's ``timestamp()`` equals its epoch seconds read as UTC.
    Checked on every call (TZ may change with ``time.tzset``)."""
    return (time.timezone == 0 and time.altzone == 0 and not time.daylight and
            time.tzname[0] in ('UTC', 'UCT', 'GMT', 'Etc/UTC', 'Universal', 'Zulu'))


def zero_offset_is_local() -> bool:
    """The zero-offset guard: dateutil reads ``Z`` / ``+00:00`` as the local zone (``'UTC' in time.tzname``) and
    that zone is not UTC, so only dateutil itself gives the reference's answer for such a cell."""
    return 'UTC' in time.tzname and not local_zone_is_utc()


_TZINFO = {}


def _tzinfo(off_s: int):
    """dateutil's own tzinfo for a UTC offset of ``off_s`` seconds (whole minutes), in the process's zone as it is
    now (a zero offset: ``tzlocal()`` or ``tzutc()`` by ``'UTC' in time.tzname``).  ``tzlocal()`` keeps the zone's
    offsets of the moment it was made, so the key holds them: after a ``time.tzset()`` to another zone a zero offset
    gets a tzinfo made there, also for a :class:`Dates` built before it."""
    key = (off_s, 'UTC' in time.tzname, time.timezone, time.altzone, time.daylight) if off_s == 0 else off_s
    tz = _TZINFO.get(key)
    if tz is None:
        a = abs(off_s)
        tz = _TZINFO[key] = _dparser.parse('2000-01-01T00:00:00%s%02d:%02d' % ('-' if off_s < 0 else '+', a // 3600,
                                                                             a % 3600 // 60)).tzinfo
    return tz


def parse_date(s: str) -> datetime:
    """``dateutil.parser.parse(s)`` for a ``str``, with the ISO rule's layouts parsed directly."""
    if not iso_enabled():                 # the routing before the ISO rule, at its cost: one short match, then dateutil
        m = _ISO19.fullmatch(s)
        if m is not None:
            y, mo, d, hh, mi, ss = (int(x) for x in m.groups())
            if y >= 1000 and 1 <= mo <= 12 and hh < 24 and mi < 60 and ss < 60:
                dim = 29 if mo == 2 and y % 4 == 0 and (y % 100 != 0 or y % 400 == 0) else _DAYS[mo - 1]
                if 1 <= d <= dim:
                    return datetime(y, mo, d, hh, mi, ss)
        return _dparser.parse(s)
    m = _ISO.fullmatch(s)
    if m is not None:
        y, mo, d, hh, mi, ss = (int(x) for x in m.groups()[:6])
        frac, z, sign, oh, om = m.groups()[6:]
        if y >= 1000 and 1 <= mo <= 12 and hh < 24 and mi < 60 and ss < 60:
            dim = 29 if mo == 2 and y % 4 == 0 and (y % 100 != 0 or y % 400 == 0) else _DAYS[mo - 1]
            if 1 <= d <= dim:
                if frac is None and z is None and sign is None:
                    return datetime(y, mo, d, hh, mi, ss)
                us = int((frac + '00000')[:6]) if frac else 0
                if z is None and sign is None:
                    return datetime(y, mo, d, hh, mi, ss, us)
                h, mm = (int(oh), int(om or 0)) if sign else (0, 0)
                if h <= 23 and mm <= 59:
                    off = (h * 3600 + mm * 60) * (-1 if sign == '-' else 1)
                    if off or not zero_offset_is_local():
                        return datetime(y, mo, d, hh, mi, ss, us, _tzinfo(off))
    return _dparser.parse(s)


_EPOCH_NAIVE = datetime(1970, 1, 1)


class Dates:
    """The parsed article dates of a native chunk's rows (ingest.NativeChunk.dates): a sequence of ``datetime`` /
    ``None`` / dateutil results like the list ``[parse_date(str(v)) if notna(v) else None]``, held as arrays for
    the rows of the ISO rule (kind 1: the 19-byte layout, epoch µs, naive read as UTC; kind 4: the same with a
    fraction; kind 3: aware, the instant's epoch µs and ``off`` its UTC offset in seconds; kind 2: None) and as
    objects for the others (kind 0: ``slow[row]``, dateutil's result).  ``epoch_us_arrays``, ``utc_stamps`` and
    ``local_stamps`` give the write path integer forms without building a ``datetime`` per row.  ``stats``: the
    counters of the read the chunk came from, if it keeps any (``stamps_slow``); ``device``: the rows' stamps as the
    ingest's device computed them, ``(stamps, native, pointer getter)`` (ingest.DeviceChunk.dates), or ``None``."""

    __slots__ = ('us', 'kind', 'slow', 'off', 'stats', 'device', 'stamps_slow')

    def __init__(self, us, kind, slow, off=None, stats=None):
        self.us, self.kind, self.slow = us, kind, slow
        self.stats, self.device, self.stamps_slow = stats, None, 0
        if off is None:
            off = np.zeros(len(kind), dtype=np.int32)
        self.off = off

    def __len__(self):
        return len(self.kind)

    def __getitem__(self, i):
        k = self.kind[i]
        if k == 1 or k == 4:
            return _EPOCH_NAIVE + timedelta(microseconds=int(self.us[i]))
        if k == 2:
            return None
        if k == 3:
            off = int(self.off[i])
            wall = _EPOCH_NAIVE + timedelta(microseconds=int(self.us[i]), seconds=off)
            return wall.replace(tzinfo=_tzinfo(off))
        return self.slow[int(i)]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def epoch_us_arrays(self):
        """(epoch µs int64[n], has-date uint8[n]) as kb.epoch_us gives them (naive = UTC; an aware date's is its
        instant's, which is what kind 3 holds); raises TypeError for a date whose tzinfo has no UTC offset, as
        epoch_us does."""
        from .kb import epoch_us
        us = np.array(self.us, dtype=np.int64, copy=True)
        ok = (self.kind != 2).astype(np.uint8)
        for r, d in self.slow.items():
            us[r] = epoch_us(d)
        return us, ok

    def utc_stamps(self, rows):
        """``(stamps, k, exc)``: ``int(d.timestamp())`` of the given rows' dates when the arrays can give it: the
        process's local time zone is UTC (a naive datetime's timestamp() reads it in local time,
        match_keywords.py:131-132), or every given row is aware (kind 3: its instant is the same in every zone);
        else ``None``.  A row of the ISO rule takes ``us // 10**6`` when it has no fraction or
        ``0 <= us < 2**52`` (timestamp() goes through a double and int() rounds toward zero: outside that the next
        second is possible); the others call timestamp(), and the first of them that raises (e.g. a year-1 date)
        stops there: ``k`` is its index in ``rows`` and ``exc`` the exception (``k = len(rows)``, ``exc = None``
        when none raises; ``stamps[:k]`` are valid)."""
        rows = np.asarray(rows, dtype=np.int64)
        kind = self.kind[rows]
        if not local_zone_is_utc() and not (len(rows) and bool((kind == 3).all())):
            return None
        us = self.us[rows]
        out = us // 1000000
        direct = ((kind == 1) | (kind == 3) | (kind == 4)) & ((us % 1000000 == 0) | ((us >= 0) & (us < STAMP_BOUND)))
        for j in np.flatnonzero(~direct).tolist():
            try:
                out[j] = int(self[int(rows[j])].timestamp())
            except Exception as exc:   # noqa: BLE001 - the reference's append_to_csv raises here (:131-132)
                return out, j, exc
        return out, len(rows), None

    def _count_slow(self, n: int) -> None:
        self.stamps_slow += n
        if self.stats is not None and n:
            self.stats['stamps_slow'] = self.stats.get('stamps_slow', 0) + n

    def finish_stamps(self, rows, out, native):
        """``out`` with the rows that are not ``native`` filled by ``timestamp()``, one by one, in order: the
        ``(stamps, k, exc)`` of :meth:`utc_stamps`.  Counts those rows (``stamps_slow``), the raising one included."""
        slow = np.flatnonzero(~native).tolist()
        for i, j in enumerate(slow):
            try:
                out[j] = int(self[int(rows[j])].timestamp())
            except Exception as exc:   # noqa: BLE001 - the reference's append_to_csv raises here (:131-132)
                self._count_slow(i + 1)
                return out, j, exc
        self._count_slow(len(slow))
        return out, len(rows), None

    def local_stamps(self, rows):
        """``(stamps, k, exc)`` as :meth:`utc_stamps` gives them, in every local time zone: ``int(d.timestamp())`` of
        the given rows' dates, the rows of the ISO rule from the integer arrays under the process's zone table
        (zone.table, ``kwcsv_stamps_local``: include/kwstamps.h), the others -- kinds 0, and dates the table does not
        answer for -- by ``timestamp()`` itself, one by one, in order; the first of them that raises stops there
        (``k`` its index in ``rows``, ``stamps[:k]`` valid).  Without a table (``KW_STAMPS_NATIVE=0``, a zone over
        the table's capacity) the routing before it: :meth:`utc_stamps` where that answers, else every row's
        ``timestamp()``.  ``stamps_slow`` (here and in ``stats``) grows by the rows that called ``timestamp()``."""
        from . import zone
        from .ingest import host_threads
        rows = np.asarray(rows, dtype=np.int64)
        tab = zone.table()
        if tab is not None:
            out, native = zone.stamps_local(self.us[rows], self.kind[rows], self.off[rows], tab, host_threads())
            return self.finish_stamps(rows, out, native.astype(bool))
        fast = self.utc_stamps(rows)
        if fast is not None:
            kind, us = self.kind[rows], self.us[rows]
            direct = ((kind == 1) | (kind == 3) | (kind == 4)) & ((us % 1000000 == 0) | ((us >= 0) & (us < STAMP_BOUND)))
            self._count_slow(int((~direct[:fast[1] + (fast[2] is not None)]).sum()))
            return fast
        return self.finish_stamps(rows, np.zeros(len(rows), dtype=np.int64), np.zeros(len(rows), dtype=bool))
