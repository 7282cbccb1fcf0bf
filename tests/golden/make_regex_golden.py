"""Generate tests/golden/regex/ by running the REFERENCE match_keywords.py on a KB of regex names.

Runs only in the build container, where /root/reference exists, with make_golden.py's protocol: the reference
is imported (not copied), rapidfuzz.fuzz.partial_ratio is stubbed by the oracle's restatement (the reference
only uses ``> 95``), single process, process_chunk chunk by chunk in file order, fresh output directory,
TZ=UTC, unique article timestamps.  The KB holds names whose regex goes beyond literals and '.' (sets,
categories, assertions, lazy repeats, branches) and names only ``re`` can run (quantified groups,
backreferences, look-ahead); the ~200 articles come from tests/regex_docs.py.

Outputs (tests/golden/regex/, data only):
  kb/*.json      the KB files the reference read
  articles.csv   the article CSV it read
  out/*.csv      its per-ticker CSVs after sort_matched_csv
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import random
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
OUT = os.path.join(HERE, 'regex')
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

N_ROWS = 200
SEED = 20261019
CHUNKSIZE = 80


def kb_files():
    from tests import regex_docs as rd
    names = [n for n in rd.NAMES if ' (' not in n]
    host = [n for n in rd.HOST_NAMES if ' (' not in n and len(n) > 2]
    assert len(names) == len(rd.NAMES)
    half = len(names) // 2
    period = ' (Start: 2012-01-01T00:00:00Z) (End: 2018-12-31T00:00:00Z)'
    a = {'ticker': 'RXA', 'country': ['United States'], 'id_label': ['Regex Holdings A'], 'aliases': names[:half],
         'products': [names[half] + period]}
    b = {'ticker': 'RXB', 'country': ['Canada'], 'id_label': ['Regex Holdings B'], 'aliases': names[half:],
         'subsidiaries': [names[0] + ' (Start: 2016-01-01T00:00:00Z)'], 'ceos': [host[0]]}
    h = {'ticker': 'RXH', 'country': ['United States'], 'id_label': ['Regex Holdings H'], 'aliases': host,
         'board_members': [names[1] + ' (End: 2010-06-30T00:00:00Z)']}
    return {'RXA_info.json': [a], 'RXB_info.json': [b], 'RXH_info.json': [h]}


def articles():
    import pandas as pd
    from tests import regex_docs as rd
    rng = random.Random(SEED)
    texts, titles = rd.documents()
    small = [t for t in texts if len(t) < 160]
    host_forms = ['(Wal|K)+mart Inc: WalKmart Inc, Kmart Inc and mart Inc', '(Tic)-\\1 Tac vs Tic-Tic Tac vs Tic-Tac',
                  'Jim(my)? Dean Inc, Jimmy Dean Inc, Jim Dean Inc', 'é Jim(my)? Dean Inc 中 Jimmy Dean Inc',
                  'Acme (?=Corp)Corp and Acme Corp']
    rows = []
    for i in range(N_ROWS):
        text = rng.choice(small)
        if i % 4 == 0:
            text = rng.choice(host_forms) + ' ' + text
        title = rng.choice(small)[:90] if i % 5 else rng.choice(host_forms)
        year = 2005 + i % 16
        date = f'{year}-{1 + i % 12:02d}-{1 + i % 28:02d} {i % 24:02d}:{i % 60:02d}:{(i * 7) % 60:02d}'
        rows.append({'article_text': text, 'title': title, 'date_time': date,
                     'url': f'https://example.invalid/regex/{i}.html', 'source': 'yahoo',
                     'source_url': 'https://finance.yahoo.com'})
    rows[3]['title'] = None
    rows[5]['date_time'] = None
    assert len({r['date_time'] for r in rows}) == N_ROWS
    return pd.DataFrame(rows)


def main():
    os.environ['TZ'] = 'UTC'
    time.tzset()
    from make_golden import _stub_rapidfuzz
    _stub_rapidfuzz()
    sys.path.insert(0, REF)
    import match_keywords as ref      # the reference, imported (not copied)
    import pandas as pd

    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(os.path.join(OUT, 'kb'))
    os.makedirs(os.path.join(OUT, 'out'))
    for fn, data in kb_files().items():
        with open(os.path.join(OUT, 'kb', fn), 'w', encoding='utf-8') as fh:
            json.dump(data, fh, ensure_ascii=False, indent=1)
    csv_bytes = articles().to_csv(index=False).encode('utf-8')
    with open(os.path.join(OUT, 'articles.csv'), 'wb') as fh:
        fh.write(csv_bytes)
    with contextlib.redirect_stdout(io.StringIO()):
        processed = ref.read_and_process_json_files(os.path.join(OUT, 'kb'))
    assert sorted(processed) == ['RXA', 'RXB', 'RXH']
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            os.makedirs('yahoo_ticker_matched_articles')
            with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
                for chunk in pd.read_csv(io.BytesIO(csv_bytes), chunksize=CHUNKSIZE):
                    ref.process_chunk('yahoo', chunk, processed)
                for fn in os.listdir('yahoo_ticker_matched_articles'):
                    ref.sort_matched_csv(f'yahoo_ticker_matched_articles/{fn}')
            for fn in os.listdir('yahoo_ticker_matched_articles'):
                shutil.copy(os.path.join('yahoo_ticker_matched_articles', fn), os.path.join(OUT, 'out', fn))
        finally:
            os.chdir(cwd)
    total = sum(os.path.getsize(os.path.join(d, f)) for d, _s, fs in os.walk(OUT) for f in fs)
    print(json.dumps({'files': sorted(os.listdir(os.path.join(OUT, 'out'))), 'bytes': total}))
    assert total < 200 * 1024, total


if __name__ == '__main__':
    main()
