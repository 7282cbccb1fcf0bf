"""time_unix on the host routes: dates.Dates.local_stamps against ``int(d.timestamp())`` per row in every zone, its
stop at the first raising row, its agreement with utc_stamps, the ``stamps_slow`` counter and ``KW_STAMPS_NATIVE=0``."""
import io
import time

import numpy as np
import pandas as pd
import pytest
from dateutil import parser

from tests import dates_rule as DR
from tests import stamps_rule as R

EST = 'EST5EDT,M3.2.0,M11.1.0'


@pytest.fixture
def zone(monkeypatch):
    def set_zone(tz):
        monkeypatch.setenv('TZ', tz)
        time.tzset()
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    monkeypatch.delenv('KW_STAMPS_NATIVE', raising=False)
    yield set_zone
    monkeypatch.undo()
    time.tzset()


def _chunk_of(cells):
    from advanced_scrapper_amd import ingest
    rows = [{'article_text': 'a', 'title': 't', 'date_time': d, 'url': 'u', 'source': 's', 'source_url': 'x'}
            for d in cells]
    buf = io.StringIO()
    pd.DataFrame(rows).to_csv(buf, index=False)
    (chunk,) = list(ingest.read_chunks_bytes(buf.getvalue().encode('utf-8'), len(cells) + 1))
    assert isinstance(chunk, ingest.NativeChunk)
    return chunk


def _stamp(s):
    """int(dateutil.parse(s).timestamp()), or None when either raises."""
    try:
        return int(parser.parse(s).timestamp())
    except Exception:   # noqa: BLE001
        return None


def _fmt(wall, frac=None, sep=' '):
    d = R.naive(wall * 1000000)
    return d.strftime('%Y-%m-%d' + sep + '%H:%M:%S') + ('' if frac is None else '.' + frac)


def _mixed_cells(table):
    """Date cells of kinds 0, 1, 3 and 4 whose timestamp() answers: the ISO table and a fuzz of tests/dates_rule.py, and
    naive cells on the edge set of a few transitions of the zone (gaps and folds), with and without a fraction.  Kind 2
    (an NA cell: the date is None) is left out on purpose: None has no timestamp(), such a document renders no row,
    and the write path never asks for its stamp; the kernel-level tests hold that kind 2 is never native."""
    cells = [s for s in DR.table() + DR.fuzz(13, 200) if _stamp(s) is not None]
    n = len(table[1])
    around = {1, 2, n // 2, n - 2, n - 1} if n > 1 else set()
    walls = R.edge_walls(table, around) + [0, 1, 86400 * 365, 4102444800 - 86400, 4102444800 - 3 * 86400,
                                           4102444800 + 86400, 2 * 86400, 3 * 86400]
    for i, w in enumerate(walls):
        cells.append(_fmt(w, None, ' T'[i & 1]))
        cells.append(_fmt(w, ('5', '000001', '999999', '999999999')[i & 3]))
    return cells


@pytest.mark.parametrize('tz', R.ZONES)
def test_local_stamps_equals_timestamp(zone, tz):
    from advanced_scrapper_amd import zone as Z
    zone(tz)
    table = tuple([int(x) for x in a] for a in Z.table())
    cells = _mixed_cells(table)
    chunk = _chunk_of(cells)
    got, exc = chunk.dates()
    assert exc is None and len(got) == len(cells)
    assert {0, 1, 3, 4} <= set(got.kind.tolist())
    want = [_stamp(s) for s in cells]
    rows = np.arange(len(cells))
    st, k, e = got.local_stamps(rows)
    assert k == len(cells) and e is None
    assert st.tolist() == want == [int(d.timestamp()) for d in got]
    # the rows that called timestamp() are the rule's not-native ones, no more
    rule = [R.stamp(table, int(u), int(kd), int(o)) for u, kd, o in zip(got.us, got.kind, got.off)]
    assert got.stamps_slow == sum(1 for _v, native in rule if not native)
    assert 0 < got.stamps_slow < len(cells)
    # a subset, out of order
    sub = rows[::-3]
    st, k, e = got.local_stamps(sub)
    assert k == len(sub) and e is None and st.tolist() == [want[i] for i in sub]
    # utc_stamps, wherever it answers, says the same
    aware = np.flatnonzero(got.kind == 3)
    assert got.utc_stamps(aware)[0].tolist() == got.local_stamps(aware)[0].tolist()
    fast = got.utc_stamps(rows)
    assert (fast is not None) == (tz == 'UTC')
    if fast is not None:
        assert fast[1] == len(cells) and fast[0].tolist() == want


@pytest.mark.parametrize('tz', ['UTC', EST])
@pytest.mark.parametrize('native', ['1', '0'])
def test_local_stamps_stops_at_the_first_raising_row(zone, monkeypatch, tz, native):
    """A date whose timestamp() raises (an offset of 24 h, dateutil's own row): the rows before it are valid."""
    zone(tz)
    monkeypatch.setenv('KW_STAMPS_NATIVE', native)
    cells = ['2023-06-05 14:23:11', '2023-06-05T14:23:11.5+05:30', '1000-01-01 00:00:00', '2023-06-05T14:23:11+24:00',
             '2023-06-05 14:23:12', '2023-06-05T14:23:11+24:00']
    chunk = _chunk_of(cells)
    got, exc = chunk.dates()
    assert exc is None and got.kind.tolist() == [1, 3, 1, 0, 1, 0]
    st, k, e = got.local_stamps([0, 1, 2, 3, 4, 5])
    assert k == 3 and isinstance(e, ValueError)
    assert st[:3].tolist() == [_stamp(c) for c in cells[:3]]
    st, k, e = got.local_stamps([4, 0])
    assert k == 2 and e is None and st.tolist() == [_stamp(cells[4]), _stamp(cells[0])]


def test_naive_chunk_under_est_counts_no_slow_stamp(zone, monkeypatch):
    """A chunk of the dataset's naive dates in a zone that is not UTC: no row calls timestamp(), in the chunk's own
    counter and in the counters of the read it belongs to; with KW_STAMPS_NATIVE=0 every row does, as before."""
    from advanced_scrapper_amd import ingest
    zone(EST)
    cells = [_fmt(1262304000 + 7919 * 3600 * i // 10) for i in range(300)]      # 2010 onwards, across DST changes
    want = [_stamp(c) for c in cells]
    assert len({w - (1262304000 + 7919 * 3600 * i // 10) for i, w in enumerate(want)}) == 2       # EST and EDT
    for native, slow in (('1', 0), ('0', len(cells))):
        monkeypatch.setenv('KW_STAMPS_NATIVE', native)
        chunk = _chunk_of(cells)
        chunk.stats = {'dates_slow': 0, 'stamps_slow': 0}         # (as read_chunks_device binds its counters)
        stale = {'stamps_slow': 0}
        monkeypatch.setattr(ingest, 'LAST_STATS', stale)
        got, exc = chunk.dates()
        assert exc is None and (got.kind == 1).all()
        st, k, e = got.local_stamps(np.arange(len(cells)))
        assert k == len(cells) and e is None and st.tolist() == want
        assert got.stamps_slow == slow and chunk.stats['stamps_slow'] == slow and stale == {'stamps_slow': 0}


def test_years_outside_the_table_keep_the_per_row_call(zone):
    zone(EST)
    cells = ['1000-01-01 00:00:00', '1969-12-31 23:59:59', '1970-01-02 23:59:59', '2023-06-05 14:23:11',
             '2099-12-29 00:00:00', '2100-01-01 00:00:00', '9999-12-31 23:59:59', '2023-06-05 14:23:11.25']
    got, exc = _chunk_of(cells).dates()
    st, k, e = got.local_stamps(np.arange(len(cells)))
    assert exc is None and e is None and st.tolist() == [_stamp(c) for c in cells]
    assert got.stamps_slow == 5                       # all but 2023 (twice) and 2099-12-29: two days inside the table
