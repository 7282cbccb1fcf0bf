"""The time_unix rule restated in plain Python (include/kwingest.h): ``int(d.timestamp())`` of the ISO
rule's rows from the integer date arrays, in any local time zone.

A *zone table* is ``(at, off)``: ascending instants ``at[0..n]`` and UTC offsets ``off[0..n-1]`` in seconds,
``off[i]`` valid on ``[at[i], at[i+1])``.  ``utcoff(u)`` is read from it for ``at[0] + MARGIN <= u < at[n] - MARGIN``
only; a row whose solve probes an instant outside that is *not native* (the caller asks ``timestamp()`` itself).

CPython solves ``t = local(u)`` for a naive datetime (``local_to_seconds``, fold = 0); :func:`solve` is that
algorithm over the table.  :func:`stamp` adds the kinds of the ISO rule:

  kind 1   the solved ``u``
  kind 4   ``timestamp()`` is the double ``u + frac / 1e6`` and ``int()`` rounds toward zero: the solved ``u`` when the
           fraction is zero, or when ``u >= 0`` and the instant's microseconds are below 2**52 (then the double
           never reaches ``u + 1``); else not native
  kind 3   ``us // 10**6`` when the fraction is zero or ``0 <= us < 2**52`` (no table needed); else not native
  0, 2     never native
"""
import bisect
import time
from datetime import datetime, timedelta

ZONES = ('UTC', 'UTC+5', 'EST5EDT,M3.2.0,M11.1.0', 'IST-5:30', 'AEST-10AEDT,M10.1.0,M4.1.0/3',
         '<+1030>-10:30<+11>-11,M10.1.0,M4.1.0', 'NST3:30NDT,M3.2.0/0:01,M11.1.0/0:01')
CAPACITY = 1024
MARGIN = 2 * 86400
SPAN = (0, 4102444800)            # 1970-01-01 .. 2100-01-01 UTC
STAMP_BOUND = 1 << 52
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
UTC_TABLE = ([I64_MIN, I64_MAX], [0])
EDGES = (0, 1, 1799, 1800, 3599, 3600, 3601)
_EPOCH = datetime(1970, 1, 1)


def utcoff(table, u):
    """The table's offset at instant ``u``, or ``None`` outside the range the table answers for."""
    at, off = table
    if not at[0] + MARGIN <= u < at[-1] - MARGIN:
        return None
    return off[bisect.bisect_right(at, u, 0, len(off)) - 1]


def solve(table, t):
    """CPython's ``local_to_seconds`` (fold = 0) for the wall clock ``t`` (read as UTC, whole seconds) over the
    table: the instant, or ``None`` when a probe leaves the table."""
    a = utcoff(table, t)
    if a is None:
        return None
    u1 = t - a
    o1 = utcoff(table, u1)
    if o1 is None:
        return None
    t1 = u1 + o1
    if t1 == t:
        u2 = u1 - 86400
        b = utcoff(table, u2)
        if b is None:
            return None
        if a == b:
            return u1
    else:
        b = t1 - u1
    u2 = t - b
    o2 = utcoff(table, u2)
    if o2 is None:
        return None
    if u2 + o2 == t:
        return u2
    if t1 == t:
        return u1
    return max(u1, u2)            # t lies in a gap


def stamp(table, us, kind, off_s=0):
    """``(time_unix, native)`` of one row of the date arrays (``native`` False: the value is 0, ask timestamp())."""
    if kind == 3:
        if us % 1000000 == 0 or 0 <= us < STAMP_BOUND:
            return us // 1000000, True
        return 0, False
    if kind not in (1, 4):
        return 0, False
    t, frac = divmod(us, 1000000)
    u = solve(table, t)
    if u is None:
        return 0, False
    if frac and not (u >= 0 and u * 1000000 + frac < STAMP_BOUND):
        return 0, False
    return u, True


def naive(us):
    """The naive datetime whose wall clock has ``us`` epoch microseconds read as UTC."""
    return _EPOCH + timedelta(microseconds=us)


def python_table(lo=SPAN[0], hi=SPAN[1], step=86400):
    """The current zone's table over [lo, hi] from ``time.localtime`` alone: sampled every ``step`` seconds, every
    change bisected to the second (what kwcsv_zone_table builds in C)."""
    gm = lambda u: time.localtime(u).tm_gmtoff    # noqa: E731
    at, off = [lo], [gm(lo)]
    u = lo
    while u < hi:
        v = min(u + step, hi)
        if gm(v) != off[-1]:
            a, b = u, v
            while b - a > 1:
                m = (a + b) // 2
                if gm(m) == off[-1]:
                    a = m
                else:
                    b = m
            at.append(b)
            off.append(gm(b))
            v = b                      # (the next step starts at the change)
        u = v
    at.append(hi)
    return at, off


def edge_walls(table, around=None):
    """The wall clocks (seconds read as UTC) of the edge set: every transition +- EDGES on both of its sides."""
    at, off = table
    out = []
    for i in range(1, len(off)):
        if around is not None and i not in around:
            continue
        for o in (off[i - 1], off[i]):
            for e in EDGES:
                out += [at[i] + o + e, at[i] + o - e]
    return out
