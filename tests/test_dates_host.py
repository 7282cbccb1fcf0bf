"""The ISO rule on the host: dates.parse_date against dateutil, NativeChunk.dates and dates.Dates against the per-row
list, the ``dates_slow`` counter and ``KW_DATES_ISO=0``."""
import io
import time

import numpy as np
import pandas as pd
import pytest
from dateutil import parser

from tests import dates_rule as DR


@pytest.fixture
def zone(monkeypatch):
    def set_zone(tz):
        monkeypatch.setenv('TZ', tz)
        time.tzset()
    yield set_zone
    monkeypatch.undo()
    time.tzset()


def _outcome(fn, s):
    try:
        d = fn(s)
    except Exception as exc:   # noqa: BLE001
        return type(exc), str(exc)
    try:
        off = d.utcoffset()
    except ValueError as exc:                   # an offset of 24 h or more: the parser accepts it, utcoffset() does not
        off = str(exc)
    return d.replace(tzinfo=None), off, repr(d), type(d.tzinfo)


@pytest.mark.parametrize('tz', DR.ZONES)
def test_parse_date_equals_dateutil(tz, zone, monkeypatch):
    from advanced_scrapper_amd.dates import parse_date
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    zone(tz)
    cells = DR.table() + DR.fuzz(5, 1500)
    bad = [(s, _outcome(parse_date, s), _outcome(parser.parse, s)) for s in cells
           if _outcome(parse_date, s) != _outcome(parser.parse, s)]
    assert not bad, bad[:5]
    # the zone may change under a process that has parsed already: the cached tzinfo follows
    for other in DR.ZONES:
        zone(other)
        for s in ('2023-06-05T14:23:11Z', '2023-06-05T14:23:11.5+00:00', '2023-06-05T14:23:11+05:30'):
            assert _outcome(parse_date, s) == _outcome(parser.parse, s), (tz, other, s)


def test_parse_date_without_the_rule(zone, monkeypatch):
    """KW_DATES_ISO=0: the same answers, dateutil's own for everything but the 19-byte layout."""
    from advanced_scrapper_amd import dates
    zone('UTC')
    monkeypatch.setenv('KW_DATES_ISO', '0')
    calls = []
    real = dates._dparser.parse
    monkeypatch.setattr(dates._dparser, 'parse', lambda s: calls.append(s) or real(s))
    assert dates.parse_date('2023-06-05 14:23:11') == real('2023-06-05 14:23:11') and not calls
    for s in ('2023-06-05T14:23:11.000Z', '2023-06-05 14:23:11.5', '2023-06-05 14:23:11+05:30'):
        assert _outcome(dates.parse_date, s) == _outcome(real, s)
    assert len(calls) == 3
    monkeypatch.delenv('KW_DATES_ISO')
    dates._TZINFO.clear()
    del calls[:]
    for s in ('2023-06-05T14:23:11.000Z', '2023-06-05 14:23:11.5', '2023-06-05 14:23:11+05:30', '2023-06-05T01:02:03Z'):
        assert _outcome(dates.parse_date, s) == _outcome(real, s)
    assert len(calls) == 2                                  # one per distinct offset, for its tzinfo


def _chunk_of(cells):
    from advanced_scrapper_amd import ingest
    rows = [{'article_text': 'a', 'title': 't', 'date_time': d, 'url': 'u', 'source': 's', 'source_url': 'x'}
            for d in cells]
    buf = io.StringIO()
    pd.DataFrame(rows).to_csv(buf, index=False)
    data = buf.getvalue().encode('utf-8')
    (chunk,) = list(ingest.read_chunks_bytes(data, len(cells) + 1))
    assert isinstance(chunk, ingest.NativeChunk)
    return chunk, pd.read_csv(io.BytesIO(data))['date_time'].tolist()


def _parses(s):
    try:
        parser.parse(s)
    except Exception:   # noqa: BLE001
        return False
    return True


def _usable(s):
    """dateutil parses the cell to a date with a usable UTC offset (below 24 h)."""
    return _parses(s) and _stamps_ok(parser.parse(s))


def _stamps_ok(d):
    try:
        d.timestamp()
    except Exception:   # noqa: BLE001
        return False
    return True


@pytest.mark.parametrize('tz', DR.ZONES)
def test_native_chunk_dates(tz, zone, monkeypatch):
    from advanced_scrapper_amd.dates import local_zone_is_utc
    from advanced_scrapper_amd.kb import epoch_us
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    zone(tz)
    cells = [s for s in DR.table() + ['', 'NA'] + DR.fuzz(9, 300) if s in ('', 'NA') or _usable(s)]
    chunk, vals = _chunk_of(cells)
    want = [parser.parse(str(v)) if pd.notna(v) else None for v in vals]
    got, exc = chunk.dates()
    assert exc is None and len(got) == len(want)
    bad = [(v, g, w) for v, g, w in zip(vals, got, want) if g != w or repr(g) != repr(w)]
    assert not bad, bad[:5]
    # the arrays hold what the rule says, the guard's rows handed back
    rule = [(2, 0, 0) if not pd.notna(v) else DR.classify(str(v).encode('utf-8')) for v in vals]
    rule = [(0, 0, 0) if DR.demoted(k, o) else (k, u, o) for k, u, o in rule]
    assert list(zip(got.kind.tolist(), got.us.tolist(), got.off.tolist())) == rule
    assert sorted(got.slow) == [i for i, r in enumerate(rule) if r[0] == 0]
    us, ok = got.epoch_us_arrays()
    assert ok.tolist() == [d is not None for d in want]
    assert [int(u) for u, d in zip(us, want) if d is not None] == [epoch_us(d) for d in want if d is not None]
    # time_unix
    good = [i for i, d in enumerate(want) if d is not None and _stamps_ok(d)]
    aware = [i for i in good if got.kind[i] == 3]
    assert len(aware) > 50 and len(good) > len(aware) + 50
    st, k, e = got.utc_stamps(aware)                       # every row aware: the zone does not matter
    assert k == len(aware) and e is None and st.tolist() == [int(want[i].timestamp()) for i in aware]
    if local_zone_is_utc():
        st, k, e = got.utc_stamps(good)
        assert k == len(good) and e is None and st.tolist() == [int(want[i].timestamp()) for i in good]
    else:
        assert got.utc_stamps(good) is None                # a naive row in a zone that is not UTC
        assert got.utc_stamps(aware + [cells.index('2023-06-05 14:23:11')]) is None
        assert got.utc_stamps([]) is None


def test_stamp_that_raises(zone, monkeypatch):
    """A date whose timestamp() raises (an offset of 24 h, dateutil's own row): the first such row stops the answer."""
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    zone('UTC')
    cells = ['2023-06-05T14:23:11Z', '2023-06-05T14:23:11.5+05:30', '2023-06-05T14:23:11+24:00', '2023-06-05T14:23:12Z']
    chunk, _vals = _chunk_of(cells)
    got, exc = chunk.dates()
    assert exc is None and got.kind.tolist() == [3, 3, 0, 3] and not _stamps_ok(got[2])
    st, k, e = got.utc_stamps([0, 1, 2, 3])
    assert k == 2 and isinstance(e, ValueError) and st[:2].tolist() == [1685974991, 1685955191]


def test_stamp_bound(zone, monkeypatch):
    """A row with a fraction answers from the arrays for 0 <= us < 2**52 alone; without one, always."""
    from advanced_scrapper_amd import dates
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    calls = []

    class Counting(dates.Dates):
        __slots__ = ()

        def __getitem__(self, i):
            calls.append(int(i))
            return dates.Dates.__getitem__(self, i)

    cells = ['2112-09-17 23:53:47.370495', '2112-09-17 23:53:47.370496', '2112-09-17T23:53:47.370495Z',
             '2112-09-17T23:53:47.370496Z', '1969-12-31 23:59:59.5', '1969-12-31 23:59:59.5Z', '1970-01-01 00:00:00.000001',
             '9999-12-31 23:59:59', '9999-12-31 23:59:59Z', '1000-01-01 00:00:00', '1000-01-01T00:00:00-23:59',
             '9999-12-31 23:59:59.999999', '9999-12-31 23:59:59.999999Z', '2262-04-11 23:47:16.854775+00:00']
    rule = [DR.classify(c.encode()) for c in cells]
    assert [u for _k, u, _o in rule[:4]] == [DR.BOUND - 1, DR.BOUND, DR.BOUND - 1, DR.BOUND]
    d = Counting(np.array([u for _k, u, _o in rule], dtype=np.int64), np.array([k for k, _u, _o in rule], dtype=np.uint8),
                 {}, np.array([o for _k, _u, o in rule], dtype=np.int32))
    for tz in ('UTC', 'EST5EDT,M3.2.0,M11.1.0'):
        zone(tz)
        rows = list(range(len(cells))) if tz == 'UTC' else [i for i, r in enumerate(rule) if r[0] == 3]
        del calls[:]
        st, k, e = d.utc_stamps(rows)
        assert k == len(rows) and e is None
        assert st.tolist() == [int(parser.parse(cells[i]).timestamp()) for i in rows]
        want_calls = [i for i in rows if rule[i][1] % 10 ** 6 and not 0 <= rule[i][1] < DR.BOUND]
        assert calls == want_calls and (tz != 'UTC' or set(want_calls) == {1, 3, 4, 5, 11, 12, 13})
    zone('UTC')
    assert -1 == rule[4][1] // 10 ** 6 != int(parser.parse(cells[4]).timestamp()) == 0     # why the bound starts at 0


def _synth_chunk(layout, n=120):
    from advanced_scrapper_amd import ingest, synth
    from advanced_scrapper_amd.kb import compile_kb
    from tests import golden_data
    names, kinds = synth.injectable_names(compile_kb(golden_data.kb_processed()))
    frame = synth.to_dataframe(synth.generate(n, names, kinds, seed=41, doc_base=0), date_layout=layout)
    buf = io.StringIO()
    frame.to_csv(buf, index=False)
    (chunk,) = list(ingest.read_chunks_bytes(buf.getvalue().encode('utf-8'), n + 1))
    assert isinstance(chunk, ingest.NativeChunk) and len(chunk) == n
    return chunk, frame


def test_synth_layouts_and_dates_slow(zone, monkeypatch):
    from advanced_scrapper_amd import ingest
    from advanced_scrapper_amd.kb import epoch_us
    zone('UTC')
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    n = 120
    naive, frame = _synth_chunk('naive', n)
    assert frame['date_time'].str.fullmatch(r'\d{4}-\d\d-\d\d \d\d:\d\d:\d\d').all()
    base, _ = naive.dates()[0].epoch_us_arrays()
    shapes = {'z_ms': r'\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d\.000Z', 'offset': r'\d{4}-\d\d-\d\d \d\d:\d\d:\d\d\+00:00',
              'mixed': r'\d{4}-\d\d-\d\d[ T]\d\d:\d\d:\d\d(\.0+)?[+-]\d\d(:?\d\d)?'}
    for layout, shape in shapes.items():
        for iso, slow in ((None, 0), ('0', n)):
            if iso is None:
                monkeypatch.delenv('KW_DATES_ISO', raising=False)
            else:
                monkeypatch.setenv('KW_DATES_ISO', iso)
            chunk, frame = _synth_chunk(layout, n)
            assert frame['date_time'].str.fullmatch(shape).all(), layout
            stale = {'dates_slow': 0}
            monkeypatch.setattr(ingest, 'LAST_STATS', stale)
            chunk.stats = {'dates_slow': 0}                  # (as read_chunks_device binds its counters)
            got, exc = chunk.dates()
            assert exc is None and chunk.stats['dates_slow'] == slow == len(got.slow), (layout, iso)
            assert stale == {'dates_slow': 0}                # an earlier read's counters are not this chunk's
            assert (got.kind == (3 if iso is None else 0)).all()
            us, ok = got.epoch_us_arrays()
            assert ok.all() and np.array_equal(us, base), layout           # the same instants in every layout
            assert [epoch_us(d) for d in got] == base.tolist()
            if layout == 'mixed':
                offs = {d.utcoffset().total_seconds() for d in got}
                assert 0 not in offs and len(offs) > 5
                assert len(set(frame['date_time'].str.len())) >= 3
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    with pytest.raises(ValueError):
        _synth_chunk('nope', 4)


def test_dates_indexed_after_a_zone_change(zone, monkeypatch):
    """A Dates built in a UTC process and indexed after TZ changed: a zero offset's tzinfo is dateutil's of the zone
    as it is then (tzlocal() keeps the offsets of the moment it was made; the cache key holds them)."""
    monkeypatch.delenv('KW_DATES_ISO', raising=False)
    zone('UTC')
    cells = ['2023-06-05T14:23:11Z', '2023-06-05 14:23:11.5+00:00', '2023-06-05T14:23:11+05:30']
    chunk, _vals = _chunk_of(cells)
    got, exc = chunk.dates()
    assert exc is None and got.kind.tolist() == [3, 3, 3]
    assert [repr(d) for d in got] == [repr(parser.parse(s)) for s in cells]
    for tz in ('UTC+5', 'IST-5:30', 'UTC'):
        zone(tz)
        for d, s in zip(got, cells):
            w = parser.parse(s)
            assert repr(d) == repr(w) and d.utcoffset() == w.utcoffset() and d.timestamp() == w.timestamp(), (tz, s)
