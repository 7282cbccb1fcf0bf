"""match_keywords.run on the device route in fresh processes whose zone has transitions (tests/stamps_e2e_worker.py):
every written time_unix is CPython's, the files are byte for byte those of ``KW_STAMPS_NATIVE=0``, no rendered
document calls timestamp() -- and one whose year the zone table does not hold still does, alone."""
import csv
import io
import json
import os
import subprocess
import sys
import time

import pytest
from dateutil import parser

from tests import golden_data
from tests.test_gpu_ingest import torch_gpu   # noqa: F401

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EST = 'EST5EDT,M3.2.0,M11.1.0'
LHI = '<+1030>-10:30<+11>-11,M10.1.0,M4.1.0'          # a 30-minute step
# wall clocks inside a gap and inside a fold of each zone (2021), and on the edges of both
SPECIAL = {EST: ['2021-03-14 02:30:00', '2021-11-07 01:30:00', '2021-03-14 01:59:59', '2021-03-14 03:00:00',
                 '2021-11-07 00:59:59', '2021-11-07 02:00:00'],
           LHI: ['2021-10-03 02:15:00', '2021-04-04 01:45:00', '2021-10-03 01:59:59', '2021-10-03 02:30:00',
                 '2021-04-04 01:29:59', '2021-04-04 02:00:00']}


def _articles(special, extra=()) -> bytes:
    """The golden articles, a few dates rewritten to ``special``; one more article per ``special`` and ``extra``
    date whose text names a company whatever the date (so each has a rendered row)."""
    frame = golden_data.articles_frame().copy()
    for k, d in enumerate(special):
        frame.loc[frame.index[40 + 55 * k], 'date_time'] = d
    buf = io.StringIO()
    frame.to_csv(buf, index=False)
    w = csv.writer(buf, lineterminator='\n')
    for k, d in enumerate(list(special) + list(extra)):
        w.writerow(['Apple Incorporated and Walt Disney said on day %d that nothing changed.' % k, 'Note %d' % k, d,
                    'https://example.org/stamps/%d' % k, 'yahoo', 'https://finance.yahoo.com'])
    return buf.getvalue().encode('utf-8')


def _worker(src: bytes, work, tz: str, native: str):
    from advanced_scrapper_amd import _native
    work.mkdir()
    (work / 'articles.csv').write_bytes(src)
    env = dict(os.environ, TZ=tz, KW_STAMPS_NATIVE=native, KW_INGEST_DEVICE='1')
    for k in ('KW_ROWS_DEVICE', 'KW_EMIT_DEVICE', 'KW_DATES_ISO', 'KW_INGEST_WINDOW', 'KW_TEST_INGEST_GRID'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, '-m', 'tests.stamps_e2e_worker', str(work)], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    assert line['rc'] == 0 and line['tz'] == tz and line['lib'] == _native.DEFAULT_LIB
    out = work / 'yahoo_ticker_matched_articles'
    return {fn: (out / fn).read_bytes() for fn in os.listdir(out)}, line


def _rows(files):
    for fn, data in sorted(files.items()):
        yield from csv.DictReader(io.StringIO(data.decode('utf-8')))


@pytest.fixture
def zone(monkeypatch):
    def set_zone(tz):
        monkeypatch.setenv('TZ', tz)
        time.tzset()
    yield set_zone
    monkeypatch.undo()
    time.tzset()


@pytest.mark.parametrize('tz', [EST, LHI], ids=['est', 'half-hour'])
def test_run_in_a_zone_with_transitions(torch_gpu, tmp_path, zone, tz):   # noqa: F811
    src = _articles(SPECIAL[tz])
    files, line = _worker(src, tmp_path / 'native', tz, '1')
    base, base_line = _worker(src, tmp_path / 'base', tz, '0')
    assert set(line['routes']) == {'device'} and set(base_line['routes']) == {'device'}
    assert line['stamps_slow'] == 0 and line['dates_slow'] == 0
    assert len(line['stamps_ms']) == len(line['routes']) and all(v > 0 for v in line['stamps_ms'])
    assert len(files) > 3 and sorted(files) == sorted(base) and all(files[f] == base[f] for f in base)
    rows = list(_rows(files))
    docs = {r['url'] for r in rows}
    assert base_line['stamps_slow'] == len(docs) > 50           # before: every rendered document called timestamp()
    zone(tz)                                                    # the children's zone, for CPython's own answer
    bad = [(r['date_time'], r['time_unix']) for r in rows
           if int(r['time_unix']) != int(parser.parse(r['date_time']).timestamp())]
    assert not bad, bad[:5]
    written = {r['date_time'] for r in rows}
    assert set(SPECIAL[tz]) <= written                          # the gap and the fold were written


def test_a_year_outside_the_table_takes_the_per_row_call(torch_gpu, tmp_path, zone):   # noqa: F811
    src = _articles((), extra=['1000-01-01 00:00:00'])
    files, line = _worker(src, tmp_path / 'native', EST, '1')
    base, _base_line = _worker(src, tmp_path / 'base', EST, '0')
    assert set(line['routes']) == {'device'} and line['stamps_slow'] == 1
    assert sorted(files) == sorted(base) and all(files[f] == base[f] for f in base)
    zone(EST)
    old = [r for r in _rows(files) if r['date_time'] == '1000-01-01 00:00:00']
    assert old and all(int(r['time_unix']) == int(parser.parse(r['date_time']).timestamp()) for r in old)
