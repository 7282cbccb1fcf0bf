"""GPU: the scraper's resume filter (kw_csv_append in csrc/cdx.hip, kw_cdx_run_exclude in csrc/dedup.hip, resume.py).

Bar: bit-exact.  The parser's verdict, offender position, rows and bytes equal tests/resume_rule.py's (which
tests/test_resume_rule.py pins against pandas) and, for the texts it takes, pandas' own read; the set difference
equals ``~isin``; the drop-in gives the same on the device route and on the pandas route (KW_RESUME_NATIVE=0).
"""
import csv
import io

import numpy as np
import pandas as pd
import pytest

from tests import resume_rule as R
from tests.test_resume_host import write_files

pytestmark = pytest.mark.gpu
FH, FC = R.FILES['failed']     # url,error
SH, SC = R.FILES['success']
LH, LC = R.FILES['links']      # date_time,url


@pytest.fixture(scope='module')
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.cdx_dedup import GpuUrlDedup
    return GpuUrlDedup()


@pytest.fixture(scope='module')
def T(gpu):
    return gpu.cdx_tile_bytes()


def _store(gpu):
    arena, off, ts = gpu.cdx_rows()
    assert off[0] == 0 and len(off) == len(ts) + 1 and off[-1] == len(arena) and not ts.any()
    return [arena[off[i]:off[i + 1]] for i in range(len(ts))]


def _check(gpu, text, header=FH, col=FC, pandas=True):
    """One text through the kernels: everything equals the rule's (and pandas' when taken)."""
    v, pos, cells = R.parse(text, header, col)
    gpu.cdx_begin()
    got = gpu.csv_append(text, header.decode(), col)
    assert got == (v, pos, len(cells) if v == R.OK else 0), (R.NAMES[v], pos, got, text[:200])
    rows = _store(gpu)
    if v != R.OK:
        assert rows == []
        return v
    assert rows == cells
    if pandas:
        assert [c.decode('utf-8') for c in cells] == R.pandas_urls(text, header, col)
    return v


def _fill(size, k0=0):
    """Records of the failed file, `size` bytes in all (size >= 62)."""
    out = []
    while size > 120:
        out.append(b'http://f/%04d' % (k0 + len(out)) + b'a' * 43 + b',e\n')
        size -= 59
    out.append(b'http://f/' + b'z' * (size - 12) + b',e\n')
    return b''.join(out)


def _at(pos, body, header=FH):
    """The header, records up to byte `pos`, then `body`."""
    head = header + b'\n'
    text = head + _fill(pos - len(head)) + body
    assert text[pos:] == body
    return text


# ------------------------------------------------------------------ the parser across tiles
def test_fill_is_eligible(gpu, T):
    assert _check(gpu, _at(3 * T + 5, b'')) == R.OK


def test_quoted_cell_spans_a_tile_boundary(gpu, T):
    body = b'http://a/1,"quoted, with ""pairs"" and\nline breaks,' + b'y,\n' * 40 + b'"\nhttp://a/2,e\n'
    assert _check(gpu, _at(T - 50, body) + _fill(T)) == R.OK


def test_doubled_quote_across_a_tile_boundary(gpu, T):
    body = b'http://a/1,"ab""cd"\nhttp://a/2,"x"\n'
    for shift in (0, 1):   # the closing quote is a tile's last byte / the pair starts the next tile
        text = _at(T - 1 - 14 + shift, body)
        assert text[T - 1 + shift:T + 1 + shift] == b'""'
        assert _check(gpu, text + _fill(100)) == R.OK


def test_crlf_across_a_tile_boundary(gpu, T):
    text = _at(T - 1 - 12, b'http://a/1,e\r\nhttp://a/2,e\r\n')
    assert text[T - 1:T + 1] == b'\r\n'
    assert _check(gpu, text) == R.OK
    # and a '\r' that ends a tile without its '\n'
    bad = _at(T - 1 - 12, b'http://a/1,e\rxhttp://a/2,e\r\n')
    assert _check(gpu, bad) == R.CR


def test_record_longer_than_two_tiles(gpu, T):
    article = ('Line, one.\n"Quoted," she said.\r\n' * (2 * T // 30 + 40))
    buf = io.StringIO()
    w = csv.writer(buf)
    w.writerow(SH.decode().split(','))
    w.writerow(['http://a/1', 'd', 't', 'a', 's', 'su', 'title, "x"', article])
    w.writerow(['http://a/2', '', '', '', '', '', '', 'short'])
    w.writerow(['http://a,3', '', '', '', '', '', '', article + 'tail'])
    text = buf.getvalue().encode()
    assert len(text) > 4 * T
    assert _check(gpu, text, SH, SC) == R.OK
    # one field short, far from the record's start: the count is taken across the tiles
    assert _check(gpu, text.replace(b',su,', b';su,', 1), SH, SC) == R.FIELDS


def test_record_end_exactly_at_a_tile_boundary(gpu, T):
    text = _at(T, b'http://a/1,e\nhttp://a/2,e\n')
    assert text[T - 1:T] == b'\n'
    assert _check(gpu, text) == R.OK
    assert _check(gpu, _at(2 * T, b'')) == R.OK   # the text ends with the tile


def test_url_cell_straddles_a_tile_boundary(gpu, T):
    assert _check(gpu, _at(T - 10, b'http://straddle/abcdefghij,e\n')) == R.OK
    assert _check(gpu, _at(T - 10, b'"http://straddle/abc,defghij",e\n')) == R.OK
    head = LH + b'\n'   # the links file: the column is the record's last field
    fill = _fill(T - 40 - len(head)).replace(b',e\n', b'\n').replace(b'http://f/', b'1,http://f/')
    text = head + fill + b'20200102030405,http://straddle/' + b'q' * 40 + b'\n'
    assert len(head + fill) == T - 40
    assert _check(gpu, text, LH, LC) == R.OK


def test_quoted_url_cell_with_comma_and_final_record_without_terminator(gpu, T):
    assert _check(gpu, FH + b'\r\n"http://a/1,2",e\r\n"http://b/,",""\r\nhttp://c/,"x""y"') == R.OK
    assert _check(gpu, _at(T - 5, b'http://last/1,e')) == R.OK
    assert _check(gpu, LH + b'\n1,"http://a/1,2"\n2,http://b\n3,"http://c,"', LH, LC) == R.OK


def test_blank_line_runs(gpu, T):
    assert _check(gpu, FH + b'\n\n\n\r\n\nhttp://a/1,e\n\n\r\n\r\nhttp://a/2,e\r\n\r\n\n') == R.OK
    for shift in range(4):   # a run of blank lines across the boundary
        assert _check(gpu, _at(T - 3 + shift, b'\n\r\n\n\r\n\nhttp://a/1,e\n\n')) == R.OK
    assert _check(gpu, FH + b'\n\n\r\n\n') == R.ROWS


def test_text_crosses_a_chunk_of_the_tile_scan(gpu, T):
    """More than 1024 tiles: the tile scans run over two chunks, and a quoted cell opened in the text's first
    record is still open at the chunk boundary (the carried quote parity is odd there)."""
    cell = 'Line, one.\nand two, three\r\n' * ((1024 * T + 5000) // 27)
    buf = io.StringIO()
    w = csv.writer(buf)
    w.writerow(['url', 'error'])
    w.writerow(['http://a/0', cell])
    text = buf.getvalue().encode() + _fill(40000, 7) + b'"http://q/1,2","a\n""b"""\r\n' + _fill(3 * T, 9000)
    assert len(text) > 1025 * T and text.count(b'"', 0, 1024 * T) == 1
    assert _check(gpu, text) == R.OK
    # the same with the cell's closing quote gone: every later quote changes sides
    assert _check(gpu, text.replace(b'\r\n"\r\n', b'\r\n\r\n', 1), pandas=False) == R.QUOTE


@pytest.mark.parametrize('kind', ['success', 'failed', 'links'])
def test_fuzz_texts(gpu, kind):
    header, col = R.FILES[kind]
    seen = set()
    for seed in range(40):
        assert _check(gpu, R.fuzz_clean(seed, kind), header, col) == R.OK
    for seed in range(2 * len(R.VIOLATIONS)):
        what, text = R.fuzz_dirty(seed, kind)
        v = _check(gpu, text, header, col)
        assert v == R.EXPECT[what]
        seen.add(v)
    assert seen == set(range(9))


def test_every_verdict_with_its_position_past_the_first_tile(gpu, T):
    o = 2 * T - 10   # the offending record starts here (its byte 10 starts a tile)
    cases = [(b'http://a/1,e\0\n', R.NUL, o + 12), (b'http://a/\xe2\x82,e\n', R.UTF8, o + 9),
             (b'http:/\xf0\x9f\x98\x80\x80,e\n', R.UTF8, o + 10), (b'http://a/1,e"\n', R.QUOTE, o + 12),
             (b'http://a/1,"e"x\n', R.QUOTE, o + 13), (b'http://a/1,"e\n', R.QUOTE, None),
             (b'http://a/1\r,e\n', R.CR, o + 10), (b'http://a/1,e,f\n', R.FIELDS, o), (b'http://a/1\n', R.FIELDS, o),
             (b'nocolon,e\n', R.URL, o), (b'"http://a""b",e\n', R.URL, o), (b'"http://a\nb",e\n', R.URL, o)]
    for body, verdict, pos in cases:
        text = _at(o, body) + _fill(200)
        v, p, _ = R.parse(text, FH, FC)
        assert (v, p) == (verdict, len(text) if pos is None else pos), body
        assert _check(gpu, text) == verdict
    assert _check(gpu, b'url,error \n' + _fill(100)) == R.HEADER
    assert _check(gpu, FH) == R.HEADER and _check(gpu, b'') == R.HEADER
    assert _check(gpu, FH + b'\r\n') == R.ROWS
    # an earlier condition wins over an earlier position
    assert _check(gpu, _at(o, b'nocolon,e\nx\r,e\nhttp://a,e\0\n')) == R.NUL


def test_refused_text_leaves_the_store_alone(gpu):
    gpu.cdx_begin()
    assert gpu.csv_append(FH + b'\nhttp://a/1,e\n', FH.decode(), FC) == (R.OK, -1, 1)
    assert gpu.csv_append(FH + b'\nhttp://a/2,e\nnocolon,e\n', FH.decode(), FC) == (R.URL, 23, 0)
    assert gpu.csv_append(LH + b'\n1,http://a/3\n', LH.decode(), LC) == (R.OK, -1, 1)
    assert _store(gpu) == [b'http://a/1', b'http://a/3']


# ------------------------------------------------------------------ the set difference
def _exclude(gpu, exclude, links):
    """Exclude strings and link strings through the parser and kw_cdx_run_exclude: everything equals ~isin."""
    gpu.cdx_begin()
    for header, col, urls in ((FH, FC, exclude), (LH, LC, links)):
        if not urls:
            continue
        buf = io.StringIO()
        w = csv.writer(buf)
        w.writerow(header.decode().split(','))
        w.writerows([u, 'e'] if col == 0 else [7, u] for u in urls)
        assert gpu.csv_append(buf.getvalue().encode(), header.decode(), col) == (R.OK, -1, len(urls))
    keep = ~pd.Series(links, dtype=object).isin(set(exclude)).to_numpy()
    want = [u for u, k in zip(links, keep) if k]
    assert gpu.run_exclude(len(exclude)) == (len(links), len(links) - len(want), len(want))
    from advanced_scrapper_amd import _native
    assert (gpu.exclude_codes() == np.where(keep, _native.KW_URL_KEPT, _native.KW_URL_SEEN)).all()
    b, off, rows = gpu.remaining()
    assert (rows == np.flatnonzero(keep)).all() and off[0] == 0 and off[-1] == len(b)
    assert [b.tobytes()[off[k]:off[k + 1]].decode() for k in range(len(rows))] == want
    return want


def _u(k):
    return 'https://finance.yahoo.com/news/article-%d-%s.html' % (k, 'x' * (k % 23))


def test_exclude_edge_cases(gpu):
    links = [_u(k) for k in range(10)]
    assert _exclude(gpu, [], links + links[:3]) == links + links[:3]            # m = 0: duplicates stay
    assert _exclude(gpu, links[::-1], links + links) == []                      # every link seen
    assert _exclude(gpu, [_u(100 + k) for k in range(10)], links) == links      # no link seen
    assert _exclude(gpu, [links[1]], [links[0], links[0], links[1], links[0]]) == [links[0]] * 3   # kept twice
    assert _exclude(gpu, [links[1], links[2], links[1], links[1]], links) == links[:1] + links[3:]  # duplicate excludes
    # equal only in a prefix, either way round; the empty-suffix neighbours
    assert _exclude(gpu, [links[4][:-1], links[5] + 'l', 'a:'], [links[4], links[5], 'a:b', 'a:', ':']) == \
        [links[4], links[5], 'a:b', ':']
    assert _exclude(gpu, links, []) == []


@pytest.mark.parametrize('n_ex', [1, 63, 64, 65, 8 * 64 + 1])
@pytest.mark.parametrize('n_links', [1, 63, 64, 65, 8 * 64 + 1])
def test_exclude_row_counts(gpu, n_ex, n_links):
    rng = np.random.RandomState(n_ex * 1000 + n_links)
    pool = [_u(k) for k in range(300)]
    exclude = [pool[i] for i in rng.randint(0, 200, n_ex)]
    links = [pool[i] for i in rng.randint(100, 300, n_links)]
    _exclude(gpu, exclude, links)


def test_exclude_after_tag_collisions(gpu, monkeypatch):
    """A 4-bit hash: nearly every row shares its tag with other URLs, so the host's exact pass resolves them and
    kw_cdx_run_exclude asks it for the first holders."""
    monkeypatch.setenv('KW_TEST_DEDUP_WEAK_HASH', '1')
    rng = np.random.RandomState(5)
    pool = [_u(k) for k in range(120)]
    _exclude(gpu, [pool[i] for i in rng.randint(0, 80, 70)], [pool[i] for i in rng.randint(40, 120, 130)])
    _exclude(gpu, [], [pool[i] for i in rng.randint(0, 50, 130)])


def test_exclude_after_tag_collisions_many_waves(gpu, monkeypatch):
    """The same over several thousand rows: many waves insert at once, so a row may be paired with a holder of its
    own URL that another URL's earlier row displaces afterwards.  Such a row is coded DUPLICATE without being one
    of the exact pass's rows, and the pass has to find its first holder by its bytes."""
    monkeypatch.setenv('KW_TEST_DEDUP_WEAK_HASH', '1')
    rng = np.random.RandomState(11)
    pool = [_u(k) for k in range(700)]
    _exclude(gpu, [pool[i] for i in rng.randint(0, 500, 3000)], [pool[i] for i in rng.randint(200, 700, 4000)])


# ------------------------------------------------------------------ the drop-in
@pytest.fixture()
def dropin(gpu, monkeypatch, tmp_path):
    from advanced_scrapper_amd import cdx_dedup, resume
    monkeypatch.setattr(cdx_dedup, '_DEDUP', gpu)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('KW_RESUME_NATIVE', raising=False)
    return resume


def _both_routes(resume, monkeypatch, capsys, route):
    capsys.readouterr()
    a = resume.remaining_urls()
    out_a = capsys.readouterr().out
    monkeypatch.setenv('KW_RESUME_NATIVE', '0')
    b = resume.remaining_urls()
    out_b = capsys.readouterr().out
    monkeypatch.delenv('KW_RESUME_NATIVE')
    assert (a.route, b.route) == (route, 'pandas') and out_a == out_b and out_a.count('\n') == 3
    assert (a.initial_total, a.scraped_success, a.scraped_fails, a.remaining, a.urls()) == \
        (b.initial_total, b.scraped_success, b.scraped_fails, b.remaining, b.urls())
    assert a.arrays()[0].tobytes() == b.arrays()[0].tobytes() and (a.arrays()[1] == b.arrays()[1]).all()
    return a


def test_remaining_urls_on_both_routes(dropin, monkeypatch, capsys):
    links = [_u(k % 150) for k in range(400)] + ['http://l/x,y', 'http://l/é']
    write_files(links, success=[_u(k) for k in range(0, 90, 2)] + [_u(4)], failed=[_u(k) for k in range(1, 60, 3)] + ['http://l/x,y'])
    a = _both_routes(dropin, monkeypatch, capsys, 'device')
    assert a.initial_total == 402 and a.scraped_success == 46 and 0 < a.remaining < 402
    a.write('rest.txt')
    assert open('rest.txt', encoding='utf-8').read().splitlines() == a.urls()
    # without the success file; with neither
    import os
    os.remove('success_articles_yfin.csv')
    assert _both_routes(dropin, monkeypatch, capsys, 'device').scraped_success == 0
    os.remove('failed_articles_yfin.csv')
    assert _both_routes(dropin, monkeypatch, capsys, 'device').remaining == 402


def test_ineligible_file_falls_back_and_agrees(dropin, monkeypatch, capsys):
    links = [_u(k) for k in range(30)]
    write_files(links, failed=[_u(3)])
    with open('failed_articles_yfin.csv', 'ab') as fh:
        fh.write(b'%s,mid"field quote\r\n' % _u(5).encode())
    a = _both_routes(dropin, monkeypatch, capsys, 'pandas')
    assert a.scraped_fails == 2 and a.remaining == 28
