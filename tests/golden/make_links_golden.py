"""Generate the link refresh / split golden fixture by running the REFERENCE experiental/drop.py and split.py.

Runs only where a checkout of the reference exists: ``KW_REFERENCE=<its directory> python
tests/golden/make_links_golden.py`` (the committed fixture is what the tests read).  Nothing of the reference's source
is copied: both scripts are run with ``runpy.run_path`` in a temporary directory that holds seeded inputs under the
file names the scripts hard-code, and the inputs and the files they wrote are stored as data.

    drop.py    yahoo_links_1.csv, yahoo_articles_all.csv            -> yahoo_links_new.csv
    split.py   yahoo_new_urls_2025.csv, success_articles_2025_yfin.csv -> parts/yfin_2025_{0,1}.csv   (num_parts = 2)

The inputs hold URLs with ',', URLs present in both files, repeats among the links, a leading-zero timestamp, and
only distinct date_time values, so the expected order does not depend on a numpy build's order among ties.  A links
file with a ',' in a URL holds '"' bytes, which the device parser of ``date_time,url`` files refuses, so the drop-ins
read that set with pandas; a second set, "plain", is the same without the ',' URLs among the links (the exclude
files keep theirs) and is what the device route can take.  The reference's scripts ran over both.

Output: tests/golden/links_golden.json (the files as text): inputs / outputs, and the same under "plain".
"""
from __future__ import annotations

import contextlib
import csv
import io
import json
import os
import random
import runpy
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20260114
ARTICLE_FIELDS = ["url", "datetime", "ticker_symbols", "author", "source", "source_url", "title", "article"]


def _url(k: int) -> str:
    return 'https://finance.yahoo.com/news/story-%d-%s.html' % (k, 'abcdefghijklmnopqrstuvwxyz'[:k % 27])


def _links(rng, ids, extra=()):
    """date_time,url text over the URL ids (repeats as given), with distinct timestamps."""
    stamps = rng.sample(range(20150101000000, 20251231235959), len(ids) + len(extra))
    rows = [(str(ts), _url(k)) for ts, k in zip(stamps, ids)]
    rows += [(str(ts), u) for ts, u in zip(stamps[len(ids):], extra)]
    rng.shuffle(rows)
    rows[3] = ('0' + rows[3][0][1:], rows[3][1])      # a leading-zero timestamp (still distinct: 14 digits, first 0)
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator='\n')
    w.writerow(['date_time', 'url'])
    w.writerows(rows)
    return buf.getvalue()


def _articles(rng, urls):
    buf = io.StringIO()
    w = csv.writer(buf)   # (csv.DictWriter's default dialect, as the scraper writes: "\r\n", minimal quoting)
    w.writerow(ARTICLE_FIELDS)
    for u in urls:
        body = 'Shares rose, then fell.\n"Quoted," it said.' * rng.randint(1, 3)
        w.writerow([u, '2024-01-02 03:04:05', "['ACME']", 'A. Writer', 'Wire', 'http://wire', 'Title, with comma', body])
    return buf.getvalue()


def run_set(ref, with_commas):
    rng = random.Random(SEED)
    comma = ['https://finance.yahoo.com/news/a,b.html', 'https://finance.yahoo.com/news/x,y,z.html',
             'https://finance.yahoo.com/news/only-in-links,1.html']
    # refresh: 70 URL ids, 25 of them drawn twice or more; ids 0..29 and two comma URLs are already articles
    ids = list(range(70)) + [rng.randrange(70) for _ in range(25)]
    extra = comma + comma[:1] if with_commas else []
    files = {'yahoo_links_1.csv': _links(rng, ids, extra),
             'yahoo_articles_all.csv': _articles(rng, [_url(k) for k in range(0, 30)] + comma[:2] + [_url(5)])}
    # split: 41 link rows (repeats stay: isin does not deduplicate), 12 ids and one comma URL already scraped
    ids = list(range(100, 135)) + [rng.randrange(100, 135) for _ in range(4)]
    files['yahoo_new_urls_2025.csv'] = _links(rng, ids, comma[:2] if with_commas else [])
    files['success_articles_2025_yfin.csv'] = _articles(rng, [_url(k) for k in range(100, 135, 3)] + comma[1:2])
    out = {'inputs': files, 'outputs': {}}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for name, text in files.items():
                with open(name, 'w', encoding='utf-8', newline='') as fh:
                    fh.write(text)
            os.makedirs('parts')
            with contextlib.redirect_stdout(io.StringIO()) as said:
                runpy.run_path(os.path.join(ref, 'experiental', 'drop.py'), run_name='__main__')
                runpy.run_path(os.path.join(ref, 'experiental', 'split.py'), run_name='__main__')
            out['split_last_line'] = said.getvalue().splitlines()[-1]
            for name in ('yahoo_links_new.csv', 'parts/yfin_2025_0.csv', 'parts/yfin_2025_1.csv'):
                with open(name, encoding='utf-8', newline='') as fh:
                    out['outputs'][name] = fh.read()
        finally:
            os.chdir(cwd)
    return out


def main():
    ref = os.environ.get('KW_REFERENCE')
    if not ref or not os.path.exists(os.path.join(ref, 'experiental', 'drop.py')):
        raise SystemExit("set KW_REFERENCE to a checkout of the reference (it holds experiental/drop.py)")
    out = run_set(ref, True)
    out.update(seed=SEED, num_parts=2, plain=run_set(ref, False))
    path = os.path.join(HERE, 'links_golden.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(out, f, indent=0)
    for o in (out, out['plain']):
        print({k: len(v.splitlines()) - 1 for k, v in o['outputs'].items()})
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
