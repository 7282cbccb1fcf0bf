"""The CDX ingest rule (tests/cdx_rule.py) against pandas: whenever the rule takes a text, its rows equal the
reference's read_csv and its rendering equals to_csv.  This pins the rule itself, not the kernel
(tests/test_gpu_cdx.py runs the kernel against the rule).
"""
import io

import pandas as pd
import pytest

from advanced_scrapper_amd import cdx_dedup
from oracle import dedup_oracle as dd
from tests import cdx_rule as R

N_FUZZ = 300


def _kept_rows(rows, normalize=True):
    urls = [u.decode('utf-8') for _, u in rows]
    if normalize:
        kept, new = dd.dedup_rows(urls)
    else:
        kept = dd.keep_first(urls)
        new = [urls[i] for i in kept]
    return [(rows[i][0], u) for i, u in zip(kept, new)]


@pytest.fixture(scope='module')
def listings():
    return [(t,) + R.parse(t, R.LISTING) for t in R.fuzz_listings(N_FUZZ, R.LISTING)]


@pytest.fixture(scope='module')
def parts():
    return [(t,) + R.parse(t, R.PART) for t in R.fuzz_listings(N_FUZZ, R.PART)]


def test_fuzz_reaches_every_verdict(listings, parts):
    seen = {v for _, v, _, _ in listings} | {v for _, v, _, _ in parts}
    assert seen == set(range(9)), sorted(R.NAMES[v] for v in set(range(9)) - seen)
    ok = [t for t, v, _, rows in listings if v == R.OK and rows]
    assert len(ok) >= N_FUZZ // 4
    assert any(len(t.split(b'\n')) >= 150 for t in ok)
    assert all(len(t.split(b'\n')) <= 201 for t, _, _, _ in listings + parts)   # at most 200 lines (+ the final '\n')
    # what the fuzz has to cover among the eligible texts
    blob = b'\n'.join(ok)
    assert b'\n\n\n' in blob and b',' in blob and 'é'.encode() in blob and b' 000' in blob
    assert any(not t.endswith(b'\n') for t in ok) and any(t.endswith(b'\n') for t in ok)
    assert any(len({len(ln.split(b' ')) for ln in t.split(b'\n') if ln}) > 1 for t in ok)   # varying field counts


def test_listing_rows_equal_pandas(listings):
    for text, v, bad, rows in listings:
        if v != R.OK:
            assert rows is None and bad >= 0
            continue
        assert bad == -1
        if not rows:   # no rows: an empty frame (its columns are object, so only the rendering is compared)
            df = cdx_dedup.read_cdx(text.decode('utf-8'), is_text=True)
            assert len(df) == 0 and df.to_csv(index=False).encode() == R.render_csv([])
            continue
        df = cdx_dedup.read_cdx(text.decode('utf-8'), is_text=True)
        assert str(df['date_time'].dtype) == 'int64' and df['url'].dtype == object
        assert df['date_time'].tolist() == [t for t, _ in rows]
        assert df['url'].tolist() == [u.decode('utf-8') for _, u in rows]
        # the same through a byte stream, as a file is read
        df2 = pd.read_csv(io.BytesIO(text), delimiter=' ', header=None, usecols=[1, 2], names=['date_time', 'url'])
        assert df2.equals(df)


def test_listing_csv_equals_pandas(listings):
    n = 0
    for text, v, _, rows in listings:
        if v != R.OK or not rows:
            continue
        want = dd.part_csv_bytes(dd.cdx_part(text.decode('utf-8')))
        assert R.render_csv(_kept_rows(rows)) == want
        n += b'"' in want
    assert n >= 3   # quoted URLs (commas) were rendered


def test_part_rows_and_merge_equal_pandas(parts):
    ok = []
    for text, v, bad, rows in parts:
        if v != R.OK:
            assert rows is None and bad >= 0
            continue
        df = pd.read_csv(io.BytesIO(text))
        assert list(df.columns) == ['date_time', 'url']
        assert df['date_time'].tolist() == [t for t, _ in rows]
        assert df['url'].tolist() == [u.decode('utf-8') for _, u in rows]
        ok.append((text, rows))
    assert len(ok) >= N_FUZZ // 4
    header_only = [t for t, rows in ok if not rows]
    assert header_only
    # merges of several parts, a header-only part among them
    for k in range(0, len(ok) - 3, 3):
        group = ok[k:k + 3] + [(header_only[0], [])]
        group = group[1:] + group[:1] if k % 2 else group
        want = dd.merge_parts(t for t, _ in group).to_csv(index=False).encode('utf-8')
        rows = [r for _, rs in group for r in rs]
        assert R.render_csv(_kept_rows(rows, normalize=False)) == want
    # only header-only parts
    want = dd.merge_parts([header_only[0], header_only[0]]).to_csv(index=False).encode('utf-8')
    assert R.render_csv([]) == want


@pytest.mark.parametrize('text,verdict,line', [
    (b'k 1 u:1\nk "2" u:2\n', R.QUOTE, 1),
    (b'k 1 u:1\r\nk 2 u:2\n', R.CR, 0),
    (b'\n\nk 1 u:1\nk 2 u\0:2\n', R.NUL, 3),
    (b'k 1 u:1\n\nk 2\n', R.FIELDS, 2),
    (b'   \n', R.TS, 0),
    (b'k 1 u:1\nk -2 u:2\n', R.TS, 1),
    (b'k 1 u:1\nk 1234567890123456789 u:2\n', R.TS, 1),
    (b'k 1 u:1\nk 2 nan\n', R.URL, 1),
    (b'k 1 u:1\nk 2 u:\xff\n', R.UTF8, 1),
    (b'k\xc3 1 u:1\n', R.UTF8, 0),
    (b'k x nocolon\nk 2 u:\xff\n', R.TS, 0),       # the first offending line decides
    (b'k x u:\xff\n', R.UTF8, 0),                  # within a line: UTF8, FIELDS, TS, URL
    (b'k 2 u:2\nk "2" u:\r\n', R.QUOTE, 1),        # the byte conditions come first, QUOTE before CR
    (b'\xff\nk 2 u:"\n', R.QUOTE, 1),
])
def test_listing_verdicts(text, verdict, line):
    assert R.parse(text, R.LISTING)[:2] == (verdict, line)


@pytest.mark.parametrize('text,verdict,line', [
    (b'', R.HEADER, 0),
    (b'\ndate_time,url\n1,u:1\n', R.HEADER, 0),
    (b'date_time,url,x\n1,u:1\n', R.HEADER, 0),
    (b'date_time,url\n1,u:1,x\n', R.FIELDS, 1),
    (b'date_time,url\n1\n', R.FIELDS, 1),
    (b'date_time,url\n\n1,u:1\n1.0,u:2', R.TS, 3),
    (b'date_time,url\n1,u 1\n', R.URL, 1),
])
def test_part_verdicts(text, verdict, line):
    assert R.parse(text, R.PART)[:2] == (verdict, line)


def test_ok_shapes():
    assert R.parse(b'', R.LISTING) == (R.OK, -1, [])
    assert R.parse(b'\n\n', R.LISTING) == (R.OK, -1, [])
    assert R.parse(b'date_time,url', R.PART) == (R.OK, -1, [])
    assert R.parse(b' 007 a:b', R.LISTING) == (R.OK, -1, [(7, b'a:b')])
    assert R.parse(b'date_time,url\n20200101,http://x/a b\n', R.PART) == (R.OK, -1, [(20200101, b'http://x/a b')])
    assert R.render_csv([(7, b'a:b'), (123456789012345678, 'http://x/é,1'.encode())]) == \
        b'date_time,url\n7,a:b\n123456789012345678,"http://x/\xc3\xa9,1"\n'
