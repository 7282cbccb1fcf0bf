"""The time_unix rule (tests/stamps_rule.py, include/kwstamps.h) against CPython itself, per POSIX zone: the zone
table kwcsv_zone_table builds, the restatement, and the host routine kwcsv_stamps_local."""
import bisect
import random
import time

import numpy as np
import pytest

from tests import stamps_rule as R
from advanced_scrapper_amd import zone as Z
from advanced_scrapper_amd.dates import local_zone_is_utc

FRACS = (1, 500000, 999999)


@pytest.fixture
def zone(monkeypatch):
    def set_zone(tz):
        monkeypatch.setenv('TZ', tz)
        time.tzset()
    yield set_zone
    monkeypatch.undo()
    time.tzset()


def _table():
    at, off = Z.table()
    return [int(x) for x in at], [int(x) for x in off]


def _cases(table, seed=7, n_random=1500):
    """(us, kind) rows: the edge set around every transition, seeded wall clocks inside the table's span and over the
    years 1019 .. 9892, the table's two ends, instants around zero, each as kind 1 and as kind 4 with a fraction;
    and every fraction at the ends and around instant zero."""
    at, off = table
    rng = random.Random(seed)
    walls = R.edge_walls(table)
    if at[0] > R.I64_MIN:
        lo, hi = at[0] + R.MARGIN, at[-1] - R.MARGIN
        walls += [lo + d for d in (-90000, -1, 0, 1, 90000)] + [hi + d for d in (-90000, -50000, -1, 0, 1, 90000)]
    walls += [rng.randrange(*R.SPAN) for _ in range(n_random)]
    walls += [rng.randrange(-3 * 10**10, 25 * 10**10) for _ in range(n_random // 3)]    # years 1019 .. 9892
    walls += [-86400, -3601, -1, 0, 1, 3600, 86400]
    rows = []
    for t in walls:
        rows.append((t * 1000000, 1))
        rows.append((t * 1000000 + rng.choice(FRACS), 4))
    ends = [-1, 0] + ([at[-1] - R.MARGIN - 1 - max(off) - 86400, at[-1] - R.MARGIN - 90000] if at[0] > R.I64_MIN
                      else [4102444799, R.STAMP_BOUND // 1000000 - 1, R.STAMP_BOUND // 1000000])
    for t in ends + [-max(off) - 1, -min(off) - 1, -min(off), -max(off)]:
        rows += [(t * 1000000 + f, 4) for f in FRACS + (0,)]
    return rows


@pytest.mark.parametrize('tz', R.ZONES)
def test_table_equals_localtime(zone, tz):
    zone(tz)
    at, off = _table()
    if local_zone_is_utc():
        assert (at, off) == R.UTC_TABLE
        return
    assert at[0] == R.SPAN[0] and at[-1] == R.SPAN[1] and at == sorted(set(at)) and 1 <= len(off) <= R.CAPACITY
    assert all(a != b for a, b in zip(off, off[1:]))
    for i in range(len(off)):
        assert time.localtime(at[i]).tm_gmtoff == off[i]
        assert time.localtime(at[i + 1] - 1).tm_gmtoff == off[i]
    rng = random.Random(3)
    for u in (rng.randrange(*R.SPAN) for _ in range(2000)):
        assert time.localtime(u).tm_gmtoff == off[bisect.bisect_right(at, u) - 1]
    assert (at, off) == tuple(R.python_table())      # the C build is the sample-and-bisect build (any step finds these)
    assert Z.LAST_BUILD_MS is not None


def test_table_sizes_of_the_posix_zones(zone):
    zone('EST5EDT,M3.2.0,M11.1.0')
    assert len(_table()[1]) == 261                   # 130 years, two changes each, and the first entry
    zone('IST-5:30')
    assert _table() == ([R.SPAN[0], R.SPAN[1]], [19800])
    zone('UTC')
    assert _table() == R.UTC_TABLE


@pytest.mark.parametrize('tz', R.ZONES)
def test_rule_equals_timestamp(zone, tz):
    """Wherever the rule answers, its value is CPython's; and it answers exactly where it says it does: not outside
    the table's range, not for a fraction whose double may round (a negative instant, 2**52 microseconds or more),
    and always when the wall clock lies three days inside the range and the fraction is safe."""
    zone(tz)
    table = _table()
    lo, hi = table[0][0] + R.MARGIN, table[0][-1] - R.MARGIN
    n_native = n_not = 0
    for us, kind in _cases(table):
        v, native = R.stamp(table, us, kind)
        t, frac = divmod(us, 1000000)
        if native:
            assert v == int(R.naive(us).timestamp()), (tz, us, kind)
            n_native += 1
        else:
            assert v == 0
            n_not += 1
        deep = lo + 3 * 86400 <= t < hi - 3 * 86400
        u = int(R.naive(us - frac).timestamp()) if deep else None       # the instant, by CPython
        safe = frac == 0 or (deep and 0 <= u and u * 1000000 + frac < R.STAMP_BOUND)
        if deep and safe:
            assert native, (tz, us, kind)
        if not lo <= t < hi or (deep and not safe):
            assert not native, (tz, us, kind)
    assert n_native > 1000 and n_not > 0
    for kind in (0, 2, 5):
        assert R.stamp(table, 1600000000 * 1000000, kind) == (0, False)


@pytest.mark.parametrize('tz', R.ZONES)
def test_fractions_at_the_table_ends_and_below_zero(zone, tz):
    """``.999999`` at the table's upper end still truncates to the solved second (so does every fraction at its lower
    end); just below instant zero int() rounds up to 0, which is why those rows are not native."""
    zone(tz)
    table = _table()
    at, off = table
    bounded = at[0] > R.I64_MIN
    top = at[-1] - R.MARGIN - 90001 if bounded else R.STAMP_BOUND // 1000000 - 1
    bottom = at[0] + R.MARGIN + 90000 if bounded else 0
    for u in (top, bottom):
        for f in FRACS:
            us = (u + R.utcoff(table, u)) * 1000000 + f
            assert R.stamp(table, us, 4) == (u, True)
            assert int(R.naive(us).timestamp()) == u
    below = -1 + off[0]                               # the wall clock of instant -1
    for f in FRACS:
        assert R.stamp(table, below * 1000000 + f, 4) == (0, False)
        assert int(R.naive(below * 1000000 + f).timestamp()) == 0          # (-0.5 -> 0, not the second -1)
    if not bounded:
        assert R.stamp(table, -1000000, 4) == (-1, True)                   # a zero fraction is exact
        assert R.stamp(table, R.STAMP_BOUND + 1, 4) == (0, False)


@pytest.mark.parametrize('tz', R.ZONES)
@pytest.mark.parametrize('threads', [1, 16])
def test_host_routine_equals_the_rule(zone, tz, threads):
    zone(tz)
    tab = Z.table()
    table = _table()
    rows = _cases(table, seed=11)
    rng = random.Random(5)
    rows += [(rng.randrange(0, 4 * 10**15), 3) for _ in range(200)] + [(-1500000, 3), (-2000000, 3), (R.STAMP_BOUND + 1, 3),
                                                                       (R.STAMP_BOUND - 1, 3), (5 * 10**17, 3)]
    rows += [(1600000000 * 1000000, 0), (0, 2)]
    us = np.array([r[0] for r in rows], dtype=np.int64)
    kind = np.array([r[1] for r in rows], dtype=np.uint8)
    st, na = Z.stamps_local(us, kind, np.zeros(len(rows), np.int32), tab, threads)
    want = [R.stamp(table, u, k) for u, k in rows]
    assert st.tolist() == [w[0] for w in want]
    assert na.tolist() == [int(w[1]) for w in want]
    assert 0 < int(na.sum()) < len(rows)


def test_table_rebuilds_after_tzset(zone):
    zone('EST5EDT,M3.2.0,M11.1.0')
    a = _table()
    assert Z.table() is Z.table()                    # cached
    zone('AEST-10AEDT,M10.1.0,M4.1.0/3')
    b = _table()
    assert a != b and b[1][0] == 39600 and a[1][0] == -18000      # 1970-01-01: AEDT, EST
    zone('EST5EDT,M3.2.0,M11.1.0')
    assert _table() == a


def test_table_over_the_capacity_is_refused(zone):
    zone('EST5EDT,M3.2.0,M11.1.0')
    assert Z.build(capacity=260) is None
    at, off = Z.build(capacity=261)
    assert len(off) == 261 and len(at) == 262
    with pytest.raises(ValueError):
        Z.stamps_local([0], [1], [0], (np.zeros(R.CAPACITY + 2, np.int64), np.zeros(R.CAPACITY + 1, np.int32)))


def test_switch_takes_the_table_away(zone, monkeypatch):
    zone('EST5EDT,M3.2.0,M11.1.0')
    monkeypatch.setenv('KW_STAMPS_NATIVE', '0')
    assert Z.table() is None
    monkeypatch.setenv('KW_STAMPS_NATIVE', '1')
    assert Z.table() is not None
