"""match_keywords.run on the device routes over article CSVs whose dates are written in the ISO rule's layouts: the
same per-ticker files whatever the layout, byte for byte those of ``KW_DATES_ISO=0``, and no row through dateutil."""
import csv
import io
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import golden_data
from tests.test_gpu_ingest import torch_gpu   # noqa: F401

pytestmark = pytest.mark.gpu
N = 400
LAYOUTS = ('naive', 'z_ms', 'offset', 'mixed')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _articles(layout: str) -> bytes:
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    names, kinds = synth.injectable_names(compile_kb(golden_data.kb_processed()))
    frame = synth.to_dataframe(synth.generate(N, names, kinds, seed=23, doc_base=0), date_layout=layout)
    frame.loc[frame.index % 37 == 5, 'date_time'] = np.nan
    buf = io.StringIO()
    frame.to_csv(buf, index=False)
    return buf.getvalue().encode('utf-8')


def _run(csv_bytes: bytes, work, env: dict):
    """match_keywords.run in this process (TZ=UTC unless ``env`` says otherwise): ({file: bytes}, ingest.LAST_STATS)."""
    from advanced_scrapper_amd import ingest, match_keywords as mk
    work.mkdir()
    (work / 'articles.csv').write_bytes(csv_bytes)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('TZ', 'UTC')
        for k in ('KW_DATES_ISO', 'KW_ROWS_DEVICE', 'KW_INGEST_WINDOW', 'KW_TEST_INGEST_GRID'):
            mp.delenv(k, raising=False)
        mp.setenv('KW_INGEST_DEVICE', '1')
        for k, v in env.items():
            mp.setenv(k, v)
        time.tzset()
        mp.chdir(work)
        mp.setattr(mk, 'read_and_process_json_files', lambda _d: golden_data.kb_processed())
        ingest.LAST_STATS = None
        args = mk._parse(['--info-dir', 'unused', '--articles', str(work / 'articles.csv'), '--chunksize', '128'])
        assert mk.run(args, 0, 1, None, None) == 0
        out = work / 'yahoo_ticker_matched_articles'
        files = {fn: (out / fn).read_bytes() for fn in os.listdir(out)}
    time.tzset()
    return files, ingest.LAST_STATS


def _without_date(files):
    out = {}
    for fn, data in files.items():
        rows = list(csv.reader(io.StringIO(data.decode('utf-8'))))
        k = rows[0].index('date_time')
        out[fn] = [r[:k] + r[k + 1:] for r in rows]
    return out


@pytest.fixture(scope='module')
def naive_run(torch_gpu, tmp_path_factory):   # noqa: F811
    files, stats = _run(_articles('naive'), tmp_path_factory.mktemp('dates') / 'naive', {})
    assert len(files) > 3 and stats['routes'] == ['device'] * 4 and stats['dates_slow'] == 0
    return files


@pytest.mark.parametrize('layout', LAYOUTS[1:])
def test_layouts_give_the_same_files(naive_run, tmp_path, layout):
    src = _articles(layout)
    files, stats = _run(src, tmp_path / 'iso', {})
    assert stats['routes'] == ['device'] * 4 and stats['dates_slow'] == 0, stats
    base, base_stats = _run(src, tmp_path / 'base', {'KW_DATES_ISO': '0'})
    assert base_stats['dates_slow'] == N - len([i for i in range(N) if i % 37 == 5])
    assert sorted(files) == sorted(base) and all(files[f] == base[f] for f in base)
    assert _without_date(files) == _without_date(naive_run)


def _boundary_csv():
    """Two articles a second apart across Bob Chapek's Start bound (2020-01-01, read as UTC), written with +05:30:
    by the wall clock both lie inside the period."""
    rows = [('Disney chief Bob Chapek spoke to investors today.', 'Parks update', '2020-01-01 05:29:59+05:30', 'u1'),
            ('Disney chief Bob Chapek spoke to analysts today.', 'Parks update', '2020-01-01T05:30:00.000+0530', 'u2')]
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator='\n')
    w.writerow(['article_text', 'title', 'date_time', 'url', 'source', 'source_url'])
    for text, title, date, url in rows:
        w.writerow([text, title, date, url, 'yahoo', 'https://finance.yahoo.com'])
    return buf.getvalue().encode('utf-8')


@pytest.mark.parametrize('rows_device', ['1', '0'])
def test_period_boundary(torch_gpu, tmp_path, rows_device):   # noqa: F811
    kb = golden_data.kb_processed()
    start, _end = kb['DIS']['ceos']['Bob Chapek']
    assert start.isoformat() == '2020-01-01T00:00:00'
    files, stats = _run(_boundary_csv(), tmp_path / 'b', {'KW_ROWS_DEVICE': rows_device})
    assert stats['dates_slow'] == 0
    rows = list(csv.DictReader(io.StringIO(files['DIS_match.csv'].decode('utf-8'))))
    hit = [r for r in rows if 'Bob Chapek' in r['text_matches']]
    assert [r['url'] for r in hit] == ['u2'] and hit[0]['time_unix'] == '1577836800'
    assert not any('Bob Chapek' in r['text_matches'] for r in rows if r['url'] == 'u1')


def test_mixed_in_a_zone_with_transitions(torch_gpu, tmp_path):   # noqa: F811
    """Fresh processes whose zone has transitions (tests/dates_e2e_worker.py): the arrays answer time_unix for the
    aware rows there, and the files are those of KW_DATES_ISO=0, where every row calls timestamp()."""
    from advanced_scrapper_amd import _native
    src = _articles('mixed')
    got = {}
    for name, iso in (('iso', '1'), ('base', '0')):
        work = tmp_path / name
        work.mkdir()
        (work / 'articles.csv').write_bytes(src)
        env = dict(os.environ, TZ='EST5EDT,M3.2.0,M11.1.0', KW_DATES_ISO=iso, KW_INGEST_DEVICE='1')
        for k in ('KW_ROWS_DEVICE', 'KW_INGEST_WINDOW', 'KW_TEST_INGEST_GRID'):
            env.pop(k, None)
        p = subprocess.run([sys.executable, '-m', 'tests.dates_e2e_worker', str(work)], cwd=REPO, env=env,
                           capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
        assert line['rc'] == 0 and line['tz'] == env['TZ'] and set(line['routes']) == {'device'}
        assert line['lib'] == _native.DEFAULT_LIB                    # the child ran this tree's library
        out = work / 'yahoo_ticker_matched_articles'
        got[name] = ({fn: (out / fn).read_bytes() for fn in os.listdir(out)}, line['dates_slow'])
    assert got['iso'][1] == 0 and got['base'][1] == N - len([i for i in range(N) if i % 37 == 5])
    assert len(got['iso'][0]) > 3 and got['iso'][0] == got['base'][0]
