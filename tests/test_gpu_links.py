"""GPU: the link list's refresh and split (kw_cdx_run_exclude_unique in csrc/dedup.hip, kw_cdx_selected_ts and
kw_cdx_csv_select_* in csrc/cdx.hip, links.py).

Bar: bit-exact.  The unique set difference equals ``new[~new.url.isin(prev.url)].drop_duplicates('url')``; the select
renderer's bytes equal ``df.iloc[order].to_csv(index=False)`` file by file; the drop-ins write the same bytes and
report the same counts on the device route and on the pandas route (KW_LINKS_NATIVE=0), and the reference's own
outputs (tests/golden/links_golden.json) on both.
"""
import numpy as np
import pandas as pd
import pytest

from tests import links_rule as R

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 8 * 64 + 1]


@pytest.fixture(scope='module')
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.cdx_dedup import GpuUrlDedup
    return GpuUrlDedup()


def _u(k):
    return 'https://finance.yahoo.com/news/article-%d-%s.html' % (k, 'x' * (k % 23))


def _load(gpu, exclude, links):
    """Exclude URLs (a url,error file) and (timestamp, url) link rows into the store.  The links go in as a part
    CSV; with a ',' in a URL, which a part CSV would quote and its parser refuse, as a space-delimited listing."""
    from advanced_scrapper_amd import _native
    gpu.cdx_begin()
    if exclude:
        text = 'url,error\n' + ''.join('%s,e\n' % ('"%s"' % u if ',' in u else u) for u in exclude)
        assert gpu.csv_append(text.encode(), 'url,error', 0) == (_native.KW_CSV_OK, -1, len(exclude))
    if links and any(',' in u for _, u in links):
        text = ''.join('x %s %s\n' % row for row in links)
        assert gpu.cdx_append(text.encode(), 'listing') == (_native.KW_CDX_OK, -1, len(links))
    elif links:
        assert gpu.cdx_append(R.links_text(links).encode(), 'part') == (_native.KW_CDX_OK, -1, len(links))
    return pd.DataFrame({'date_time': np.array([int(ts) for ts, _ in links], dtype=np.int64),
                         'url': pd.Series([u for _, u in links], dtype=object)})


# ------------------------------------------------------------------ the unique set difference
def _unique(gpu, exclude, urls):
    from advanced_scrapper_amd import _native
    links = [(1000 + 7 * i, u) for i, u in enumerate(urls)]
    new = _load(gpu, exclude, links)
    prev = pd.Series(exclude, dtype=object)
    seen = new['url'].isin(prev).to_numpy()
    d = new[~seen].drop_duplicates('url')
    kept = np.zeros(len(new), dtype=bool)
    kept[d.index.to_numpy()] = True
    want = np.where(seen, _native.KW_URL_SEEN, np.where(kept, _native.KW_URL_KEPT, _native.KW_URL_DUPLICATE))
    n_dup = int((~seen & ~kept).sum())
    assert gpu.run_exclude_unique(len(exclude)) == (len(new), int(seen.sum()), n_dup, len(d))
    assert gpu.exclude_codes().tolist() == want.tolist()
    b, off, rows = gpu.remaining()
    assert rows.tolist() == d.index.tolist() and off[0] == 0 and off[-1] == len(b)
    assert [b.tobytes()[off[k]:off[k + 1]].decode() for k in range(len(rows))] == d['url'].tolist()
    assert gpu.selected_ts().tolist() == d['date_time'].tolist()
    return d['url'].tolist()


@pytest.mark.parametrize('n_ex', SIZES)
@pytest.mark.parametrize('n_links', SIZES)
def test_exclude_unique_row_counts(gpu, n_ex, n_links):
    rng = np.random.RandomState(n_ex * 1000 + n_links)
    pool = [_u(k) for k in range(300)]
    _unique(gpu, [pool[i] for i in rng.randint(0, 200, n_ex)], [pool[i] for i in rng.randint(100, 300, n_links)])


def test_exclude_unique_adversarial_rows(gpu):
    a = [_u(k) for k in range(10)]
    # a link equal to an exclude row and to an earlier link: SEEN both times, never DUPLICATE
    assert _unique(gpu, [a[1]], [a[1], a[0], a[1], a[0], a[1]]) == [a[0]]
    assert _unique(gpu, [a[2]], [a[2]] * 200) == []                       # every link equal, and seen
    assert _unique(gpu, [a[3]], [a[2]] * 200) == [a[2]]                   # every link equal, none seen
    assert _unique(gpu, [_u(100 + k) for k in range(10)], a) == a         # no link equal to anything
    assert _unique(gpu, [], a + a[:3]) == a                               # no exclude rows: plain keep-first
    assert _unique(gpu, a, []) == []
    # a repeat whose first holder sits in another wave (and another block)
    far = [_u(1000 + k) for k in range(700)]
    assert _unique(gpu, [a[0]], [a[5]] + far + [a[5], a[0], far[3]]) == [a[5]] + far
    # equal only in a prefix
    assert _unique(gpu, [a[4][:-1], a[5] + 'l'], [a[4], a[5], 'a:b', 'a:', 'a:b']) == [a[4], a[5], 'a:b', 'a:']


def test_exclude_unique_after_tag_collisions(gpu, monkeypatch):
    """A 4-bit hash: nearly every row shares its tag with other URLs, so the host's exact pass resolves them and
    the pass asks it for the first holders."""
    monkeypatch.setenv('KW_TEST_DEDUP_WEAK_HASH', '1')
    rng = np.random.RandomState(5)
    pool = [_u(k) for k in range(120)]
    _unique(gpu, [pool[i] for i in rng.randint(0, 80, 70)], [pool[i] for i in rng.randint(40, 120, 130)])
    _unique(gpu, [], [pool[i] for i in rng.randint(0, 50, 130)])
    pool = [_u(k) for k in range(700)]
    rng = np.random.RandomState(11)
    _unique(gpu, [pool[i] for i in rng.randint(0, 500, 3000)], [pool[i] for i in rng.randint(200, 700, 4000)])


# ------------------------------------------------------------------ the select renderer
def _rows(n, seed=0):
    """n distinct link rows: URL lengths from 1 to beyond 48 bytes (lines start at every residue mod 16 and straddle
    lanes), some with ',', timestamps of 1 and 18 digits and 0."""
    rng = np.random.RandomState(seed + n)
    stamps = [0, 7, 10 ** 17 + 23, 999999999999999999, 20240102030405]
    rows = [(0, ':'), (999999999999999999, 'a:'), (7, 'b:c'), (10 ** 17, 'h:,d')][:n]
    for i in range(4, n):
        length = max(len('%d' % i), (i * 7 + int(rng.randint(0, 3))) % 70)
        body = ('%d' % i + ('a,b' if i % 5 == 0 else 'abc') * 30)[:length]
        rows.append((stamps[i % 5] if i % 3 else int(rng.randint(0, 10 ** 9)), 'h:' + body))
    assert len({u for _, u in rows}) == n and (n < 100 or max(len(u) for _, u in rows) > 48)
    return rows


def _segments(n_order, n_seg, rng):
    return np.sort(np.concatenate([[0, n_order], rng.randint(0, n_order + 1, n_seg - 1)])).astype(np.int64)


def _select(gpu, df, order, seg=None):
    """One csv_select against pandas, file by file."""
    order = np.asarray(order, dtype=np.int64)
    files = gpu.csv_select(order, seg)
    bounds = [0, len(order)] if seg is None else list(seg)
    assert len(files) == len(bounds) - 1
    for s, got in enumerate(files):
        want = df.iloc[order[bounds[s]:bounds[s + 1]]].to_csv(index=False).encode()
        assert got == want, (s, bounds[s], bounds[s + 1], got[:120], want[:120])
    return files


def _orders(n, rng):
    ident = np.arange(n, dtype=np.int64)
    out = {'identity': ident, 'reverse': ident[::-1].copy(), 'random': rng.permutation(n).astype(np.int64),
           'subset': rng.permutation(n)[:n // 2].astype(np.int64), 'empty': ident[:0]}
    if n:
        out['repeated'] = rng.randint(0, n, 2 * n + 3).astype(np.int64)
    return out


@pytest.mark.parametrize('n', SIZES + [1100])   # 1100 lines and their headers cross a chunk of the tile scan
def test_select_orders_and_segments(gpu, n):
    rng = np.random.RandomState(n)
    df = _load(gpu, [], _rows(n))
    gpu.cdx_run(normalize=False)
    assert gpu.selected_ts().tolist() == df['date_time'].tolist()
    for name, order in _orders(n, rng).items():
        _select(gpu, df, order)
        for n_seg in (1, 2, 3, 7):
            _select(gpu, df, order, _segments(len(order), n_seg, rng))
    order = rng.permutation(n).astype(np.int64)
    # more files than rows; empty first, middle and last files; a bound in the middle of a wave
    _select(gpu, df, order, np.minimum(np.arange(n + 4, dtype=np.int64), n))
    _select(gpu, df, order, np.array([0, 0, n // 2, n // 2, n, n], dtype=np.int64))
    if n > 40:
        _select(gpu, df, order, np.array([0, 37, 37 + 64 * (n > 200), n], dtype=np.int64))


def test_select_sizes_sum_to_the_total(gpu):
    """d_seg_bytes and the total straight from the C-ABI."""
    import ctypes
    import torch
    from advanced_scrapper_amd import _native
    df = _load(gpu, [], _rows(65))
    gpu.cdx_run(normalize=False)
    dev = torch.device('cuda', gpu.device)
    order = torch.arange(64, -1, -1, dtype=torch.int64, device=dev)
    seg = torch.tensor([0, 10, 10, 65], dtype=torch.int64, device=dev)
    size = torch.full((3,), -1, dtype=torch.int64, device=dev)
    total = ctypes.c_int64(-1)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu.device).cuda_stream)
    L = _native.lib()
    assert L.kw_cdx_csv_select_size(gpu.h, _native.ptr(order), 65, _native.ptr(seg), 3, _native.ptr(size),
                                    ctypes.byref(total), st) == 0
    want = [len(df.iloc[list(range(64, -1, -1))[a:b]].to_csv(index=False).encode()) for a, b in ((0, 10), (10, 10), (10, 65))]
    assert size.cpu().tolist() == want and total.value == sum(want) and want[1] == len('date_time,url\n')
    ms = gpu.select_last_ms()
    assert ms[0] > 0 and ms[1] == 0
    out = torch.zeros(total.value + 16, dtype=torch.uint8, device=dev)
    assert L.kw_cdx_csv_select_copy(gpu.h, _native.ptr(out), st) == 0
    assert out[total.value:].cpu().tolist() == [0] * 16          # nothing written past the end
    assert gpu.select_last_ms()[1] > 0


def test_select_is_valid_after_each_run_and_leaves_the_row_order_renderer_alone(gpu):
    from advanced_scrapper_amd import _native
    rng = np.random.RandomState(3)
    rows = _rows(300)
    rows = rows + [(5, rows[k][1]) for k in (3, 3, 40, 299)]     # repeats among the links
    exclude = [rows[k][1] for k in range(0, 300, 4)] + ['h:not-a-link']
    # kw_cdx_run: the kept rows; kw_cdx_csv_* gives what it gave before, before and after a select
    df = _load(gpu, [], rows)
    gpu.cdx_run(normalize=False)
    kept = df.drop_duplicates('url')
    whole = kept.to_csv(index=False).encode()
    assert gpu.cdx_csv() == whole
    _select(gpu, kept, rng.permutation(len(kept)), _segments(len(kept), 3, rng))
    assert gpu.cdx_csv() == whole
    assert _select(gpu, kept, np.arange(len(kept)))[0] == whole
    # kw_cdx_run_exclude: the remaining rows, repeats included
    df = _load(gpu, exclude, rows)
    gpu.run_exclude(len(exclude))
    rest = df[~df['url'].isin(exclude)]
    assert rest['url'].duplicated().any()
    assert gpu.selected_ts().tolist() == rest['date_time'].tolist()
    _select(gpu, rest, rng.permutation(len(rest)), _segments(len(rest), 2, rng))
    with pytest.raises(_native.KwError):      # (the row-order renderer still needs a kw_cdx_run)
        gpu.cdx_csv()
    # kw_cdx_run_exclude_unique
    gpu.run_exclude_unique(len(exclude))
    uniq = rest.drop_duplicates('url')
    assert len(uniq) < len(rest) and gpu.selected_ts().tolist() == uniq['date_time'].tolist()
    _select(gpu, uniq, rng.permutation(len(uniq)), _segments(len(uniq), 7, rng))
    # a changed store ends the validity
    gpu.cdx_append(b'date_time,url\n1,h:more\n', 'part')
    with pytest.raises(_native.KwError) as e:
        gpu.csv_select(np.arange(3))
    assert e.value.code == _native.KW_ESTATE
    with pytest.raises(_native.KwError):
        gpu.selected_ts()


def test_select_rejects_bad_indices_and_bounds(gpu):
    """An argument check on the device: the index is rejected before anything is read through it."""
    from advanced_scrapper_amd import _native
    df = _load(gpu, [], _rows(130))
    gpu.cdx_run(normalize=False)
    for pos, bad in ((0, 130), (129, -1), (64, 1 << 40), (77, -(1 << 62))):
        order = np.arange(130, dtype=np.int64)
        order[pos] = bad
        if pos == 129:
            order[100] = 5     # (a valid repeat before it)
        with pytest.raises(_native.KwError) as e:
            gpu.csv_select(order, np.array([0, 50, 130], dtype=np.int64))
        assert e.value.code == _native.KW_EINVAL and 'd_order[%d] = %d' % (pos, bad) in str(e.value)
    two_bad = np.arange(130, dtype=np.int64)
    two_bad[[90, 20]] = [500, 131]
    with pytest.raises(_native.KwError) as e:
        gpu.csv_select(two_bad)
    assert 'd_order[20] = 131' in str(e.value)             # the first offender
    for seg, who in (([1, 130], 0), ([0, 129], 1), ([0, 70, 60, 130], 2), ([0, -5, 130], 1), ([0, 1 << 50, 130], 1)):
        with pytest.raises(_native.KwError) as e:
            gpu.csv_select(np.arange(130), np.array(seg, dtype=np.int64))
        assert e.value.code == _native.KW_EINVAL and 'd_seg[%d]' % who in str(e.value)
    with pytest.raises(_native.KwError):                    # a refused size pass leaves nothing to copy
        import ctypes
        import torch
        out = torch.zeros(64, dtype=torch.uint8, device=torch.device('cuda', gpu.device))
        gpu._check(_native.lib().kw_cdx_csv_select_copy(gpu.h, _native.ptr(out), ctypes.c_void_p(0)))
    _select(gpu, df, np.arange(130)[::-1])                  # and the handle goes on working


# ------------------------------------------------------------------ the drop-ins
@pytest.fixture()
def links(gpu, monkeypatch, tmp_path):
    from advanced_scrapper_amd import cdx_dedup, links
    monkeypatch.setattr(cdx_dedup, '_DEDUP', gpu)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('KW_LINKS_NATIVE', raising=False)
    return links


def _write(name, text):
    with open(name, 'w', encoding='utf-8', newline='') as fh:
        fh.write(text)


def _refresh_both(links, monkeypatch, route):
    a = links.refresh_links('new.csv', 'prev.csv', 'out_a.csv')
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    b = links.refresh_links('new.csv', 'prev.csv', 'out_b.csv')
    monkeypatch.delenv('KW_LINKS_NATIVE')
    assert (a.route, b.route) == (route, 'pandas') and a.counts() == b.counts()
    assert R.read_bytes('out_a.csv') == R.read_bytes('out_b.csv')
    return a


def _split_both(links, monkeypatch, capsys, k, route):
    capsys.readouterr()
    a = links.split_links('in.csv', 'a', k, 'drop.csv')
    out_a = capsys.readouterr().out
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    b = links.split_links('in.csv', 'b', k, 'drop.csv')
    out_b = capsys.readouterr().out
    monkeypatch.delenv('KW_LINKS_NATIVE')
    assert (a.route, b.route) == (route, 'pandas') and a.counts() == b.counts() and a.parts == b.parts
    last = 'CSV file has been split into %d parts.' % k
    assert out_a.splitlines()[-1] == last == out_b.splitlines()[-1]
    if route == 'device':
        assert out_a == last + '\n'
    for i in range(k):
        assert R.read_bytes('a_%d.csv' % i) == R.read_bytes('b_%d.csv' % i), i
    return a


def _many(n, n_urls, n_stamps, seed):
    rng = np.random.RandomState(seed)
    pool = [_u(k) for k in range(n_urls)] + ['http://l/xy', 'http://l/é', 'http://l/abc']
    stamps = 20200101000000 + rng.randint(0, n_stamps, n)
    stamps[5] = 7      # (written with a leading zero below)
    rows = [(int(ts), pool[i]) for ts, i in zip(stamps, rng.randint(0, len(pool), n))]
    text = R.links_text(rows).replace('\n7,', '\n007,', 1)
    assert '\n007,' in text
    return text, pool


def test_refresh_links_on_both_routes(links, monkeypatch):
    text, pool = _many(4000, 1500, 40, 1)       # heavy timestamp ties: both routes call numpy on this host
    _write('new.csv', text)
    _write('prev.csv', R.articles_text(pool[100:700] + pool[-2:] + pool[100:110] + ['http://l/x,y']))
    a = _refresh_both(links, monkeypatch, 'device')
    assert a.n_links == 4000 and a.seen > 0 and a.duplicate > 0 and a.written > 500
    assert a.n_links == a.seen + a.duplicate + a.written
    got = pd.read_csv('out_a.csv')
    assert got['url'].is_unique and (np.diff(got['date_time'].to_numpy()) <= 0).all() and len(got) == a.written


def test_split_links_on_both_routes(links, monkeypatch, capsys):
    text, pool = _many(3001, 4000, 10 ** 6, 2)
    gone = pool[0:4000:3] + pool[-1:]
    lines = text.splitlines(keepends=True)
    gone_set = set(gone)
    stays = [ln.rstrip('\n').split(',', 1)[1].strip('"') not in gone_set for ln in lines[1:]]
    while sum(stays) % 6 != 5:   # the surviving count is divisible by neither 2 nor 3
        lines.pop()
        stays.pop()
    _write('in.csv', ''.join(lines))
    _write('drop.csv', R.articles_text(gone))
    for k in (1, 2, 3):
        a = _split_both(links, monkeypatch, capsys, k, 'device')
        assert sum(a.parts) == a.written == a.n_links - a.seen and max(a.parts) - min(a.parts) <= 1
        assert a.written % 6 == 5 and a.n_links == len(lines) - 1 > 2900
    rest = pd.read_csv('in.csv')
    rest = rest[~rest['url'].isin(gone)]
    assert len(rest) == a.written and rest['url'].duplicated().any()
    assert pd.read_csv('a_1.csv')['url'].tolist() == rest['url'].tolist()[1::3]


@pytest.mark.parametrize('which', ['plain', 'commas'])
def test_golden_fixture_through_the_default_route(links, capsys, which):
    """The reference's own outputs.  The set whose links hold ',' URLs (quoted in the file) is one the part dialect
    refuses, so the take rule sends it to pandas; the plain set runs on the device."""
    g = R.golden()
    route = 'device' if which == 'plain' else 'pandas'
    fx = g['plain'] if which == 'plain' else g
    assert ('"' in fx['inputs']['yahoo_links_1.csv']) == (which == 'commas')
    R.write_inputs(fx['inputs'])
    res = links.refresh_links()
    assert res.route == route and R.read_bytes('yahoo_links_new.csv') == fx['outputs']['yahoo_links_new.csv'].encode()
    assert res.seen > 0 and res.duplicate > 0
    capsys.readouterr()
    res = links.split_links(num_parts=g['num_parts'], **R.SPLIT_NAMES)
    said = capsys.readouterr().out
    assert res.route == route and said.splitlines()[-1] == g['split_last_line']
    assert route == 'pandas' or said == g['split_last_line'] + '\n'
    for i in range(2):
        name = 'parts/yfin_2025_%d.csv' % i
        assert R.read_bytes(name) == fx['outputs'][name].encode()


def test_ineligible_files_fall_back_and_agree(links, monkeypatch, capsys):
    rows = [(100 + k, _u(k)) for k in range(30)]
    # a '"' in the links file: the part dialect refuses it
    _write('new.csv', R.links_text(rows) + '5,"http://a/""q"\n')
    _write('in.csv', R.links_text(rows) + '5,"http://a/""q"\n')
    _write('prev.csv', R.articles_text([_u(3), _u(4)]))
    _write('drop.csv', R.articles_text([_u(3), _u(4)]))
    a = _refresh_both(links, monkeypatch, 'pandas')
    assert a.counts() == (31, 2, 0, 29) and b'"http://a/""q"' in R.read_bytes('out_a.csv')
    assert _split_both(links, monkeypatch, capsys, 2, 'pandas').parts == [15, 14]
    # an exclude header with two `url` names: pandas reads the first
    _write('new.csv', R.links_text(rows))
    _write('in.csv', R.links_text(rows))
    for name in ('prev.csv', 'drop.csv'):
        _write(name, 'url,url\n%s,%s\n' % (_u(3), _u(9)))
    assert _refresh_both(links, monkeypatch, 'pandas').counts() == (30, 1, 0, 29)
    assert _split_both(links, monkeypatch, capsys, 3, 'pandas').written == 29
    # a header without `url`: the reference's KeyError on either route
    for name in ('prev.csv', 'drop.csv'):
        _write(name, 'link,error\n%s,e\n' % _u(3))
    for native in ('1', '0'):
        monkeypatch.setenv('KW_LINKS_NATIVE', native)
        with pytest.raises(KeyError):
            links.refresh_links('new.csv', 'prev.csv', 'out_a.csv')
        with pytest.raises(KeyError):
            links.split_links('in.csv', 'a', 2, 'drop.csv')
    monkeypatch.delenv('KW_LINKS_NATIVE')
    # num_parts = 0, a missing file, an empty file: the reference's exceptions
    _write('drop.csv', R.articles_text([_u(3)]))
    with pytest.raises(ZeroDivisionError):
        links.split_links('in.csv', 'a', 0, 'drop.csv')
    with pytest.raises(FileNotFoundError):
        links.refresh_links('new.csv', 'nowhere.csv', 'out_a.csv')
    _write('prev.csv', '')
    with pytest.raises(pd.errors.EmptyDataError):
        links.refresh_links('new.csv', 'prev.csv', 'out_a.csv')


def test_all_excluded_writes_headers_only(links, monkeypatch, capsys):
    rows = [(100 + k, _u(k % 20)) for k in range(50)]
    _write('new.csv', R.links_text(rows))
    _write('in.csv', R.links_text(rows))
    _write('prev.csv', R.articles_text([_u(k) for k in range(25)]))
    _write('drop.csv', R.articles_text([_u(k) for k in range(25)]))
    assert _refresh_both(links, monkeypatch, 'device').counts() == (50, 50, 0, 0)
    assert R.read_bytes('out_a.csv') == b'date_time,url\n'
    a = _split_both(links, monkeypatch, capsys, 3, 'device')
    assert a.parts == [0, 0, 0] and [R.read_bytes('a_%d.csv' % i) for i in range(3)] == [b'date_time,url\n'] * 3
