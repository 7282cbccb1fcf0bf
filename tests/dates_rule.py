"""Pure-Python restatement of the ISO rule of the article dates (csrc/kwcsv.c kwcsv_dates_iso, csrc/kwingest.hip
ig_rows_kernel, dates.parse_date; include/kwingest.h) and the generators of its tests.

A non-NA date cell is native iff its bytes match, as a whole cell,

    YYYY-MM-DD[ T]HH:MM:SS ( '.' 1-9 digits )? ( 'Z' | [+-]HH ( ':'? MM )? )?

with ASCII digits, year >= 1000, month / day / hour / minute / second valid by the calendar, offset HH <= 23 and
MM <= 59 (19 to 35 bytes).  ``classify(cell)`` gives ``(kind, us, off_s)``:

  0  neither: the caller asks dateutil                                  (0, 0)
  1  the 19-byte layout: us = the wall clock's epoch µs read as UTC     off_s = 0
  2  (an NA cell; decided by the tokenizer's flag, not by the bytes)
  3  aware ('Z' or an offset): us = the instant's epoch µs (wall clock minus offset), off_s = the offset in seconds
  4  naive with a fraction: us = the wall clock's epoch µs, the fraction's first six digits included (more digits
     are dropped, not rounded)

The C and HIP code never looks at the process's time zone.  dateutil answers 'Z' and a zero offset with
``tzlocal()`` whenever ``'UTC' in time.tzname``: harmless in a UTC process, an instant hours off under a zone that
is only *named* UTC (``TZ=UTC+5``).  ``demoted(kind, off_s)`` says when Python hands such a row back to dateutil.

``time_unix(kind, us, utc)`` is ``int(parse(s).timestamp())`` where the arrays give it: a kind-3 row in every zone,
kinds 1 and 4 in a UTC process; with a zero fraction ``us // 10**6`` exactly, with a fraction only for
``0 <= us < 2**52`` (timestamp() goes through a double, and int() rounds toward zero); else ``None``.
"""
import calendar
import datetime
import random
import re
import time

_NATIVE = re.compile(rb'([0-9]{4})-([0-9]{2})-([0-9]{2})[ T]([0-9]{2}):([0-9]{2}):([0-9]{2})'
                     rb'(?:\.([0-9]{1,9}))?(?:(Z)|([+-])([0-9]{2})(?::?([0-9]{2}))?)?')
BOUND = 1 << 52
EPOCH = datetime.datetime(1970, 1, 1)


def classify(cell: bytes):
    """(kind, us, off_s) of a non-NA date cell."""
    m = _NATIVE.fullmatch(cell)
    if m is None:
        return 0, 0, 0
    f = [int(x) for x in m.groups()[:6]]
    if f[0] < 1000:
        return 0, 0, 0
    try:
        datetime.datetime(*f)
    except ValueError:
        return 0, 0, 0
    us = calendar.timegm(tuple(f)) * 10 ** 6
    frac, z, sign, oh, om = m.groups()[6:]
    if frac is not None:
        us += int((frac + b'00000')[:6])
    if z is None and sign is None:
        return (1 if frac is None else 4), us, 0
    off = 0
    if sign is not None:
        h, mi = int(oh), int(om or b'0')
        if h > 23 or mi > 59:
            return 0, 0, 0
        off = (h * 3600 + mi * 60) * (-1 if sign == b'-' else 1)
    return 3, us - off * 10 ** 6, off


def zone_is_utc() -> bool:
    return (time.timezone == 0 and time.altzone == 0 and not time.daylight and
            time.tzname[0] in ('UTC', 'UCT', 'GMT', 'Etc/UTC', 'Universal', 'Zulu'))


def demoted(kind: int, off_s: int) -> bool:
    """The zero-offset guard: this row goes to dateutil although its bytes are native."""
    return kind == 3 and off_s == 0 and 'UTC' in time.tzname and not zone_is_utc()


def time_unix(kind: int, us: int, utc: bool):
    if kind == 3 or (kind in (1, 4) and utc):
        if us % 10 ** 6 == 0 or 0 <= us < BOUND:
            return us // 10 ** 6
    return None


def as_datetime(kind: int, us: int, off_s: int):
    """The naive wall clock and the UTC offset (None for a naive date) the arrays stand for."""
    wall = EPOCH + datetime.timedelta(microseconds=us + off_s * 10 ** 6)
    return wall, (datetime.timedelta(seconds=off_s) if kind == 3 else None)


# ------------------------------------------------------------------ the table
ZONES = ('UTC', 'UTC+5', 'EST5EDT,M3.2.0,M11.1.0', 'IST-5:30')        # POSIX TZ strings: no tzdata needed
BASE = '2023-06-05T14:23:11'
FRACTIONS = ('', '.5', '.123456', '.1234567', '.123456789', '.1234567891', '.000', '.000000000', '.999999999',
             '.9999999', '.')
OFFSETS = ('', 'Z', '+00:00', '-00:00', '+0000', '-00', '+00', '+05:30', '-05:30', '+0530', '-0800', '+05', '-11',
           '+23:59', '-23:59', '+24:00', '+05:60', '+99:00', '+2360', '+053', '+05:3', '+05:', '+5:30', 'z', ' Z',
           'UTC', ' UTC', '+05:30Z', 'Z+05:30', '+05:300', '+', '-')


def table():
    """The explicit cells (str): every row of the behaviour table, the length, fraction, offset, year and leap-day
    edges, digits that are not ASCII."""
    cells = []
    for base in (BASE, BASE.replace('T', ' ')):
        for fr in FRACTIONS:
            for off in OFFSETS:
                cells.append(base + fr + off)
    cells += [BASE + ',5', BASE + ',500Z', BASE + '.Z', BASE + '.+05:30', BASE + '.5.5', BASE + '.5 ', ' ' + BASE + 'Z',
              BASE + 'Z ', BASE[:-1], BASE[:-1] + 'Z', BASE + '0', BASE + 'x']
    # lengths 18 / 19 / 20 / 35 / 36
    cells += ['2023-06-05T14:23:1', '2023-06-05 14:23:11', '2023-06-05 14:23:11Z', '2023-06-05 14:23:11.123456789+05:30',
              '2023-06-05 14:23:11.123456789-05:30', '2023-06-05 14:23:11.1234567891+05:30',
              '2023-06-05 14:23:11.123456789+05:300']
    assert [len(c) for c in cells[-7:]] == [18, 19, 20, 35, 35, 36, 36]
    for y in ('0999', '1000', '9999'):
        for rest in ('-01-01 00:00:00', '-12-31T23:59:59'):
            for tail in ('', '.999999', 'Z', '+23:59', '-23:59', '.000001-00:01'):
                cells.append(y + rest + tail)
    for y in (1900, 2000, 2023, 2024):
        for tail in ('', '.25', 'Z', '+05:30'):
            cells.append('%04d-02-29 12:00:00%s' % (y, tail))
    for bad in ('2021-00-04 05:06:07', '2021-13-04 05:06:07', '2021-03-00 05:06:07', '2021-04-31 05:06:07',
                '2021-03-04 24:06:07', '2021-03-04 05:60:07', '2021-03-04 05:06:60'):
        for tail in ('', '.5', 'Z', '+01:00'):
            cells.append(bad + tail)
    # 2**52 µs = 2112-09-17 23:53:47.370496
    cells += ['2112-09-17 23:53:47.370495', '2112-09-17 23:53:47.370496', '2112-09-17T23:53:47.370495Z',
              '2112-09-17T23:53:47.370496Z', '1969-12-31 23:59:59.5', '1969-12-31 23:59:59.5Z', '1970-01-01 00:00:00.5+00:01',
              '9999-12-31 23:59:59.999999', '9999-12-31 23:59:59.999999Z']
    # digits that are not ASCII (2- and 3-byte code points), in the fields, the fraction and the offset
    cells += ['2021-03-04 05:06:0٧Z', '٢021-03-04 05:06:07.5', '2021-03-04 05:06:07.٥', '2021-03-04 05:06:07+0٥:30',
              '2021-03-04 05:06:07+05:3²', '２０２１-03-04 05:06:07Z']
    return cells


def fuzz(seed: int, n: int):
    """n seeded cells (str) around the rule: boundary years, fields one past their range, 0 to 10 fraction digits
    (all-9 and all-0 among them), every zone spelling of the table, offsets up to 99:60."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        y = rng.choice((999, 1000, 1001, 1899, 1900, 1969, 1970, 2000, 2023, 2024, 2038, 2112, 2113, 9999,
                        rng.randrange(1000, 10000)))
        mo = rng.choice((0, 13)) if rng.random() < 0.03 else rng.randrange(1, 13)
        last = calendar.monthrange(max(y, 1), mo)[1] if 1 <= mo <= 12 else 31
        d = rng.choice((0, last + 1)) if rng.random() < 0.04 else rng.choice((1, last, rng.randrange(1, last + 1)))
        hh = 24 if rng.random() < 0.02 else rng.choice((0, 23, rng.randrange(24)))
        mi = 60 if rng.random() < 0.02 else rng.choice((0, 59, rng.randrange(60)))
        ss = 60 if rng.random() < 0.02 else rng.choice((0, 59, rng.randrange(60)))
        s = '%04d-%02d-%02d%s%02d:%02d:%02d' % (y, mo, d, rng.choice(' T'), hh, mi, ss)
        nf = rng.choice((0, 0, 0, 1, 2, 3, 3, 6, 6, 7, 9, 10, rng.randrange(11)))
        if nf:
            s += rng.choice('...,') if rng.random() < 0.1 else '.'
            s += rng.choice(('0' * nf, '9' * nf, ''.join(rng.choice('0123456789') for _ in range(nf))))
        elif rng.random() < 0.02:
            s += '.'
        z = rng.random()
        if z < 0.25:
            pass
        elif z < 0.40:
            s += rng.choice(('Z', 'Z', 'Z', 'z', ' Z', 'UTC', ' UTC'))
        elif z < 0.50:
            s += rng.choice(('+00:00', '-00:00', '+0000', '-0000', '+00', '-00'))
        else:
            h = rng.choice((5, 23, 24, 99, rng.randrange(24), rng.randrange(24)))
            m = rng.choice((0, 30, 59, 60, rng.randrange(60)))
            form = rng.choice(('%s%02d:%02d', '%s%02d:%02d', '%s%02d%02d', '%s%02d', '%s%d:%02d', '%s%02d%d'))
            args = (rng.choice('+-'), h, m)
            s += form % (args if form.count('%') == 3 else args[:2])
        out.append(s)
    return out


# ------------------------------------------------------------------ the table as a CSV text, and the host's answer
NA_CELLS = ('', 'NA', 'nan', 'NULL')        # (of pandas' default NA strings: kind 2)
QUOTED_ROW = 1                              # text() quotes this row's date cell besides those that hold a ','


def cases():
    """The table, a few NA cells and a slice of the fuzz: more than 256 cells (str), NA cells included."""
    return table() + list(NA_CELLS) + fuzz(11, 300)


def expect(cells):
    """[(kind, us, off_s)] of the cells by the rule, an NA cell as (2, 0, 0)."""
    return [(2, 0, 0) if c in NA_CELLS else classify(c.encode('utf-8')) for c in cells]


def text(cells, ncols: int = 7, col: int = 2, final_newline: bool = True) -> bytes:
    """The cells as column ``col`` of an ``ncols``-column text, a record a cell."""
    rows = []
    for i, c in enumerate(cells):
        assert '"' not in c and '\n' not in c
        d = '"%s"' % c if (i == QUOTED_ROW or ',' in c) else c
        f = ['a%d' % i if k == 0 else 'f%d' % k for k in range(ncols)]
        f[col] = d
        rows.append(','.join(f))
    return ('\n'.join(rows) + ('\n' if final_newline else '')).encode('utf-8')


def host_arrays(data: bytes, ncols: int, col: int, threads: int):
    """(us, kind, off_s) of kwcsv_dates_iso and (us, kind) of kwcsv_dates over kwcsv_parse's cells of the text."""
    import ctypes
    import numpy as np
    from advanced_scrapper_amd import ingest
    na_buf, na_off, n_na = ingest._na_table()
    p, L = ingest._p, ingest._lib()
    buf = np.frombuffer(data + b'\0' * 16, dtype=np.uint8)
    cap = data.count(b'\n') + 1
    out = np.empty(len(data) + 16, dtype=np.uint8)
    coff = np.zeros(cap * ncols + 1, dtype=np.int64)
    cfl = np.zeros(cap * ncols, dtype=np.uint8)
    pos = ctypes.c_int64(0)
    rows = int(L.kwcsv_parse(p(buf), len(data), 0, cap, ncols, p(na_buf), p(na_off), n_na, p(out), len(data) + 16,
                             p(coff), p(cfl), ctypes.byref(pos), None))
    assert rows >= 0, rows
    us, kind, off = np.full(rows, -1, np.int64), np.full(rows, 9, np.uint8), np.full(rows, -1, np.int32)
    L.kwcsv_dates_iso(p(out), p(coff), p(cfl), rows, ncols, col, p(us), p(kind), p(off), threads)
    us19, kind19 = np.full(rows, -1, np.int64), np.full(rows, 9, np.uint8)
    L.kwcsv_dates(p(out), p(coff), p(cfl), rows, ncols, col, p(us19), p(kind19), threads)
    return (us, kind, off), (us19, kind19)
