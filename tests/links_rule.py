"""The link refresh and split restated (advanced_scrapper_amd/links.py; reference: experiental/drop.py, split.py).

    descending(keys)        the row order of DataFrame.sort_values(by=..., ascending=False) over an integer column:
                            pandas' nargsort reverses the keys, calls argsort(kind='quicksort'), and reverses the result
    refresh_frame(new, prev)   drop.py:6-10 over two frames
    split_frames(df, drop, k)  split.py:15-27 over two frames: the k frames written

tests/test_links_rule.py holds descending() against pandas itself and the drop-ins' pandas routes against fixtures the
reference's own scripts wrote (tests/golden/make_links_golden.py).
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'links_golden.json')
SPLIT_NAMES = {'input_file': 'yahoo_new_urls_2025.csv', 'output_prefix': 'parts/yfin_2025',
               'drop_file': 'success_articles_2025_yfin.csv'}
ARTICLE_FIELDS = ["url", "datetime", "ticker_symbols", "author", "source", "source_url", "title", "article"]


def descending(keys):
    keys = np.asarray(keys)
    idx = np.arange(len(keys), dtype=np.int64)
    return idx[::-1][np.argsort(keys[::-1], kind='quicksort')][::-1]


def tied_keys(n, seed=0):
    """n int64 keys drawn from about n / 4 values: many ties."""
    rng = np.random.RandomState(seed + n)
    return rng.randint(0, max(2, n // 4), n).astype(np.int64) + 20200101000000


def refresh_frame(new, prev):
    d = new[~new['url'].isin(prev['url'])].drop_duplicates(subset='url')
    d = d.iloc[descending(d['date_time'].to_numpy())]
    return d.reset_index(drop=True)


def split_frames(df, drop, k):
    d = df[~df['url'].isin(drop['url'])]
    return [d.iloc[i::k] for i in range(k)]


def golden():
    with open(GOLDEN, encoding='utf-8') as fh:
        return json.load(fh)


def write_inputs(files):
    """The fixture's input files into the current directory, byte for byte, and the split's output folder."""
    for name, text in files.items():
        with open(name, 'w', encoding='utf-8', newline='') as fh:
            fh.write(text)
    os.makedirs('parts', exist_ok=True)


def read_bytes(name):
    with open(name, 'rb') as fh:
        return fh.read()


def links_text(rows):
    """date_time,url text of (timestamp, url) rows as to_csv writes it."""
    out = ['date_time,url\n']
    for ts, u in rows:
        out.append('%s,%s\n' % (ts, '"%s"' % u if ',' in u else u))
    return ''.join(out)


def articles_text(urls):
    """A success / article file as csv.DictWriter writes it, with cells that hold ',', '"' and line breaks."""
    import csv
    import io
    buf = io.StringIO()
    w = csv.writer(buf)
    w.writerow(ARTICLE_FIELDS)
    for k, u in enumerate(urls):
        w.writerow([u, 'd', "['T']", 'a', 's', 'http://s', 'Title, %d' % k, 'Line, one.\n"Quoted," two.'])
    return buf.getvalue()
