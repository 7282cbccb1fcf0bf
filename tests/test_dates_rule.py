"""The ISO rule of the article dates (tests/dates_rule.py) against dateutil itself, and csrc/kwcsv.c against the rule."""
import time

import numpy as np
import pytest
from dateutil import parser

from tests import dates_rule as DR

FUZZ_N = 6000


@pytest.fixture
def zone(monkeypatch):
    def set_zone(tz):
        monkeypatch.setenv('TZ', tz)
        time.tzset()
    yield set_zone
    monkeypatch.undo()
    time.tzset()


def _against_dateutil(cells):
    """(native, demoted, [disagreements]) of the rule on the cells in the process's zone as it is."""
    utc = DR.zone_is_utc()
    native = demoted = 0
    bad = []
    for s in cells:
        kind, us, off = DR.classify(s.encode('utf-8'))
        if kind == 0:
            continue
        native += 1
        if DR.demoted(kind, off):
            demoted += 1
            continue
        d = parser.parse(s)                     # (a native cell never raises)
        wall, uo = DR.as_datetime(kind, us, off)
        if d.replace(tzinfo=None) != wall or d.utcoffset() != uo:
            bad.append((s, d, wall, uo))
            continue
        t = DR.time_unix(kind, us, utc)
        if t is not None and t != int(d.timestamp()):
            bad.append((s, t, int(d.timestamp())))
    return native, demoted, bad


# what the rule must call native (the behaviour table's native rows, the length / fraction / offset / year edges) ...
MUST = {
    '2023-06-05T14:23:11': (1, 0), '2023-06-05 14:23:11Z': (3, 0), '2023-06-05T14:23:11.5': (4, 0),
    '2023-06-05T14:23:11.000Z': (3, 0), '2023-06-05 14:23:11+00:00': (3, 0), '2023-06-05T14:23:11-00:00': (3, 0),
    '2023-06-05T14:23:11-00': (3, 0), '2023-06-05T14:23:11+0000': (3, 0), '2023-06-05T14:23:11+05:30': (3, 19800),
    '2023-06-05T14:23:11+0530': (3, 19800), '2023-06-05T14:23:11+05': (3, 18000), '2023-06-05T14:23:11-0800': (3, -28800),
    '2023-06-05T14:23:11+23:59': (3, 86340), '2023-06-05T14:23:11.123456789-23:59': (3, -86340),
    '2023-06-05 14:23:11.123456789+05:30': (3, 19800), '2023-06-05T14:23:11.1234567': (4, 0),
    '2023-06-05T14:23:11.999999999': (4, 0), '1000-01-01 00:00:00+23:59': (3, 86340),
    '9999-12-31T23:59:59-23:59': (3, -86340), '2000-02-29 12:00:00.25': (4, 0), '2024-02-29 12:00:00+05:30': (3, 19800),
}
# ... and what it must leave to dateutil
MUST_NOT = ['2023-06-05T14:23:11+24:00', '2023-06-05T14:23:11+05:60', '2023-06-05T14:23:11+99:00',
            '2023-06-05T14:23:11.Z', '2023-06-05T14:23:11+053', '2023-06-05T14:23:11,5', '2023-06-05T14:23:11z',
            '2023-06-05T14:23:11 Z', '2023-06-05T14:23:11UTC', '2023-06-05T14:23:11+5:30', '2023-06-05T14:23:1',
            '2023-06-05 14:23:11.1234567891+05:30', '2023-06-05 14:23:11.123456789+05:300',
            '2023-06-05T14:23:11.1234567891', '0999-01-01 00:00:00Z', '1900-02-29 12:00:00Z', '2023-02-29 12:00:00.25',
            '2021-03-04 05:06:0٧Z', '2021-03-04 05:06:07.٥', '2021-03-04 05:06:07+0٥:30', '２０２１-03-04 05:06:07Z']


def test_table_verdicts():
    table = DR.table()
    for s, (kind, off) in MUST.items():
        assert s in table, s
        got = DR.classify(s.encode('utf-8'))
        assert (got[0], got[2]) == (kind, off), s
    for s in MUST_NOT:
        assert s in table, s
        assert DR.classify(s.encode('utf-8')) == (0, 0, 0), s
    assert DR.classify(b'2023-06-05T14:23:11.1234567')[1] % 10 ** 6 == 123456          # dropped, not rounded
    assert DR.classify(b'2023-06-05T14:23:11.999999999')[1] % 10 ** 6 == 999999
    assert DR.classify(b'2023-06-05T14:23:11.5')[1] % 10 ** 6 == 500000
    # kind 3 holds the instant
    assert DR.classify(b'2023-06-05T14:23:11+05:30')[1] == DR.classify(b'2023-06-05T08:53:11Z')[1]
    assert DR.classify(b'2112-09-17T23:53:47.370496Z')[1] == DR.BOUND


@pytest.mark.parametrize('tz', DR.ZONES)
def test_rule_equals_dateutil(tz, zone):
    zone(tz)
    fuzz = DR.fuzz(20231, FUZZ_N)
    native, demoted, bad = _against_dateutil(fuzz)
    assert not bad, bad[:10]
    assert native >= 0.40 * len(fuzz), native         # the rule alone: the generator stays around the rule
    if tz == 'UTC+5':                                 # a zone named UTC that is not: the guard hands zero offsets back
        assert demoted > 0.05 * len(fuzz) and DR.demoted(3, 0) and not DR.demoted(3, 60)
    else:
        assert demoted == 0 and not DR.demoted(3, 0)
    _n, _d, bad = _against_dateutil(DR.table())
    assert not bad, bad[:10]


def test_guard_is_needed(zone):
    """Without the guard the rule's answer for 'Z' is not dateutil's under a zone merely named UTC."""
    zone('UTC+5')
    kind, us, off = DR.classify(b'2023-06-05T14:23:11Z')
    assert (kind, off) == (3, 0) and us // 10 ** 6 == 1685974991
    assert int(parser.parse('2023-06-05T14:23:11Z').timestamp()) == 1685992991


# ------------------------------------------------------------------ csrc/kwcsv.c
CASES = DR.cases()
WANT = DR.expect(CASES)


def _check_host(data, ncols, col, threads, want):
    (us, kind, off), (us19, kind19) = DR.host_arrays(data, ncols, col, threads)
    assert len(kind) == len(want)
    got = list(zip(kind.tolist(), us.tolist(), off.tolist()))
    bad = [(CASES[i], w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not bad, bad[:10]
    # kwcsv_dates on the same cells: the 19-byte layout alone, as before the ISO rule
    want19 = [(k, u) if k in (1, 2) else (0, 0) for k, u, _o in want]
    assert list(zip(kind19.tolist(), us19.tolist())) == want19


@pytest.mark.parametrize('threads', [1, 5])
def test_kwcsv_dates_iso_equals_rule(threads):
    assert len(CASES) > 256 and {k for k, _u, _o in WANT} == {0, 1, 2, 3, 4}
    assert WANT[DR.QUOTED_ROW][0] != 0                                  # the quoted cell is a native one
    _check_host(DR.text(CASES), 7, 2, threads, WANT)
    # the date as the last cell of the last row, the text ending with it
    order = CASES[1:] + CASES[:1]
    assert DR.classify(order[-1].encode())[0] == 1
    data = DR.text(order, 7, 6, final_newline=False)
    assert data.endswith(order[-1].encode())
    (us, kind, off), (us19, kind19) = DR.host_arrays(data, 7, 6, threads)
    want = DR.expect(order)
    assert list(zip(kind.tolist(), us.tolist(), off.tolist())) == want
    assert list(zip(kind19.tolist(), us19.tolist())) == [(k, u) if k in (1, 2) else (0, 0) for k, u, _o in want]


def test_kwcsv_dates_iso_long_cells():
    """Cells of 35 native bytes followed by more, and far longer ones: nothing past 35 bytes is native."""
    cells = ['2023-06-05 14:23:11.123456789+05:30', '2023-06-05 14:23:11.123456789+05:30' + '0' * 40,
             '2023-06-05 14:23:11' + '.1' * 200, 'x' * 5000]
    (us, kind, off), _ = DR.host_arrays(DR.text(cells), 7, 2, 1)
    assert kind.tolist() == [3, 0, 0, 0] and us.tolist()[1:] == [0, 0, 0] and off.tolist() == [19800, 0, 0, 0]
    assert np.int64(us[0]) == DR.classify(cells[0].encode())[1]
