"""kw_ingest_dates_iso (csrc/kwingest.hip, the rows kernel) against kwcsv_dates_iso and the ISO rule
(tests/dates_rule.py); kw_ingest_dates of the same parse against kwcsv_dates."""
import numpy as np
import pytest

from tests import dates_rule as DR
from tests import ingest_rule as R
from tests.test_gpu_ingest import COLS7, _parse, torch_gpu   # noqa: F401

pytestmark = pytest.mark.gpu
HOOK = 'KW_TEST_INGEST_GRID'
CASES = DR.cases()
WANT = DR.expect(CASES)
TEXT = DR.text(CASES)
LAST = CASES[1:] + CASES[:1]                     # ends with a 19-byte cell
COLS_LAST = [0, 1, 6, 3, 4, 5]                   # date_time the last column
TEXT_LAST = DR.text(LAST, 7, 6, final_newline=False)


@pytest.fixture(scope='module')
def devs(torch_gpu):   # noqa: F811
    from advanced_scrapper_amd import ingest
    a, b = ingest.DeviceIngest(0, 7, COLS7), ingest.DeviceIngest(0, 7, COLS_LAST)
    yield a, b
    a.close()
    b.close()


def _check(torch, dev, text, col, want, max_rows=1 << 20, rows=None):
    rows = len(want) if rows is None else rows
    v, bad, n_rows, _consumed = _parse(torch, dev, text, True, max_rows)
    assert (v, n_rows) == (R.OK, rows), (R.NAMES[v], bad, n_rows)
    us, kind, off = dev.dates_iso()
    got = list(zip(kind.tolist(), us.tolist(), off.tolist()))
    diff = [(i, w, g) for i, (w, g) in enumerate(zip(want[:rows], got)) if w != g]
    assert not diff and len(got) == rows, diff[:10]                       # the rule
    (hus, hkind, hoff), (hus19, hkind19) = DR.host_arrays(text, 7, col, 3)
    assert np.array_equal(us, hus[:rows]) and np.array_equal(kind, hkind[:rows]) and np.array_equal(off, hoff[:rows])
    us19, kind19 = dev.dates()                                             # the same parse, the 19-byte contract
    assert np.array_equal(us19, hus19[:rows]) and np.array_equal(kind19, hkind19[:rows])
    assert set(kind19.tolist()) <= {0, 1, 2}


def test_table(torch_gpu, devs, monkeypatch):   # noqa: F811
    monkeypatch.delenv(HOOK, raising=False)
    assert len(CASES) > 256 and {k for k, _u, _o in WANT} == {0, 1, 2, 3, 4}
    assert WANT[DR.QUOTED_ROW][0] == 3 and b'"' + CASES[DR.QUOTED_ROW].encode() + b'"' in TEXT
    _check(torch_gpu, devs[0], TEXT, 2, WANT)
    # the last record's last column the date, the text ending with it
    assert TEXT_LAST.endswith(b',' + LAST[-1].encode()) and DR.classify(LAST[-1].encode())[0] == 1
    _check(torch_gpu, devs[1], TEXT_LAST, 6, DR.expect(LAST))
    # ... and a 35-byte one there
    long = LAST[:-1] + ['2023-06-05 14:23:11.123456789-05:30']
    _check(torch_gpu, devs[1], DR.text(long, 7, 6, final_newline=False), 6, DR.expect(long))


@pytest.mark.parametrize('grid', [1, 2])
def test_several_trips(torch_gpu, devs, monkeypatch, grid):   # noqa: F811
    """A launch grid of one or two blocks: the rows kernel's loop makes a second trip over the table's rows."""
    monkeypatch.setenv(HOOK, str(grid))
    _check(torch_gpu, devs[0], TEXT, 2, WANT)
    _check(torch_gpu, devs[1], TEXT_LAST, 6, DR.expect(LAST))


def test_max_rows(torch_gpu, devs, monkeypatch):   # noqa: F811
    monkeypatch.delenv(HOOK, raising=False)
    _check(torch_gpu, devs[0], TEXT, 2, WANT, max_rows=5, rows=5)
    _check(torch_gpu, devs[1], TEXT_LAST, 6, DR.expect(LAST), max_rows=5, rows=5)
