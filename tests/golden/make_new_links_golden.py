"""Generate the new-links golden fixture by running the REFERENCE experiental/new_links.py.

Runs only where a checkout of the reference exists: ``KW_REFERENCE=<its directory> python
tests/golden/make_new_links_golden.py`` (the committed fixture is what the tests read).  Nothing of the reference's
source is copied: the script is loaded with ``runpy.run_path`` (not as ``__main__``, whose file names are hard-coded)
and its ``find_new_urls`` is called in a temporary directory over seeded inputs; the inputs, what it printed and the
file it wrote are stored as data.

    plain            two date_time,url files; repeats in either and in the intersection, so the three printed
                     counts (unique URLs) differ from every row count
    articles         the old file is an article dataset: url first of eight columns, quoted multi-line cells
    missing_column   the old file has no url column: the reference prints the columns and writes nothing
    unreadable       the old file does not exist: the reference prints the error and writes nothing

Output: tests/golden/new_links_golden.json: per case the input files as text (null: absent), "stdout" and "output"
(null: no file written).
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import random
import runpy
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20260301
NEW, OLD, OUT = 'yahoo_links_new.csv', 'yahoo_links_old.csv', 'yahoo_new_urls.csv'


def _url(k: int) -> str:
    return 'https://finance.yahoo.com/news/item-%d-%s.html' % (k, 'abcdefghijklmnopqrstuvwxyz'[:k % 27])


def _links(rng, ids) -> str:
    stamps = rng.sample(range(20150101000000, 20251231235959), len(ids))
    return 'date_time,url\n' + ''.join('%d,%s\n' % (ts, _url(k)) for ts, k in zip(stamps, ids))


def _articles(rng, ids) -> str:
    import csv
    buf = io.StringIO()
    w = csv.writer(buf)
    w.writerow(["url", "datetime", "ticker_symbols", "author", "source", "source_url", "title", "article"])
    for k in ids:
        body = 'Shares rose, then fell.\n"Quoted," it said.' * rng.randint(1, 3)
        w.writerow([_url(k), '2024-01-02 03:04:05', "['ACME']", 'A. Writer', 'Wire', 'http://wire', 'Title, %d' % k, body])
    return buf.getvalue()


def cases():
    rng = random.Random(SEED)
    # ids 0..54 new, 40..99 old: 40..54 in both; repeats in the new file (in and out of the intersection) and the old
    new_ids = list(range(55)) + [rng.randrange(55) for _ in range(30)] + [45, 45, 45, 3, 3]
    rng.shuffle(new_ids)
    old_ids = list(range(40, 100)) + [rng.randrange(40, 100) for _ in range(20)] + [45, 50]
    rng.shuffle(old_ids)
    new = _links(rng, new_ids)
    return {'plain': {NEW: new, OLD: _links(rng, old_ids)},
            'articles': {NEW: new, OLD: _articles(rng, old_ids)},
            'missing_column': {NEW: new, OLD: 'date_time,link\n' + _links(rng, old_ids[:5]).split('\n', 1)[1]},
            'unreadable': {NEW: new, OLD: None}}


def main():
    ref = os.environ.get('KW_REFERENCE')
    script = os.path.join(ref or '', 'experiental', 'new_links.py')
    if not ref or not os.path.exists(script):
        raise SystemExit("set KW_REFERENCE to a checkout of the reference (it holds experiental/new_links.py)")
    find_new_urls = runpy.run_path(script, run_name='new_links')['find_new_urls']
    out = {'seed': SEED, 'names': [NEW, OLD, OUT], 'cases': {}}
    cwd = os.getcwd()
    for name, files in cases().items():
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                for fname, text in files.items():
                    if text is not None:
                        with open(fname, 'w', encoding='utf-8', newline='') as fh:
                            fh.write(text)
                with contextlib.redirect_stdout(io.StringIO()) as said:
                    find_new_urls(NEW, OLD, OUT)
                written = None
                if os.path.exists(OUT):
                    with open(OUT, encoding='utf-8', newline='') as fh:
                        written = fh.read()
                out['cases'][name] = {'inputs': files, 'stdout': said.getvalue(), 'output': written}
            finally:
                os.chdir(cwd)
        print(name, out['cases'][name]['stdout'].splitlines()[1:4])
    path = os.path.join(HERE, 'new_links_golden.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(out, f, indent=0)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
