"""GPU: the streamed routes of refresh_links, split_links, remaining_urls and find_new_urls (links.py, resume.py over
GpuUrlDedup.csv_append_file / cdx_append_file), and find_new_urls' counts (kw_cdx_exclude_distinct_seen in
csrc/dedup.hip).

Bar: bit-exact.  With ``stream_from=0`` and windows of a few tiles every file takes several windows, and the files
written, the counts and the printed lines equal the pandas route's (KW_LINKS_NATIVE=0 / KW_RESUME_NATIVE=0) and, for
find_new_urls, the reference's own run (tests/golden/new_links_golden.json).
"""
import json
import os

import numpy as np
import pandas as pd
import pytest

from tests import links_rule as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'new_links_golden.json')


@pytest.fixture(scope='module')
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.cdx_dedup import GpuUrlDedup
    return GpuUrlDedup()


@pytest.fixture()
def env(gpu, monkeypatch, tmp_path):
    from advanced_scrapper_amd import cdx_dedup
    monkeypatch.setattr(cdx_dedup, '_DEDUP', gpu)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('KW_LINKS_NATIVE', raising=False)
    monkeypatch.delenv('KW_RESUME_NATIVE', raising=False)
    T = gpu.cdx_tile_bytes()
    return {'stream_from': 0, 'window_bytes': 2 * T + 16, 'max_record_bytes': 2 * T}


def _u(k):
    return 'https://finance.yahoo.com/news/article-%d-%s.html' % (k, 'x' * (k % 23))


def _write(name, text):
    with open(name, 'w', encoding='utf-8', newline='') as fh:
        fh.write(text)


def _inputs(n_links=700, n_articles=300):
    """A links file of a few hundred rows with repeats, and an article file with multi-line cells that holds a
    third of its URLs, some twice."""
    rng = np.random.RandomState(7)
    stamps = rng.permutation(np.arange(20200101000000, 20200101000000 + 5 * n_links, 5))[:n_links]
    ids = rng.randint(0, 400, n_links)
    links = R.links_text([(int(ts), _u(int(k))) for ts, k in zip(stamps, ids)])
    articles = R.articles_text([_u(int(k)) for k in rng.randint(250, 600, n_articles)])
    return links, articles


def test_refresh_and_split_streamed(env, monkeypatch, capsys):
    from advanced_scrapper_amd import links
    text, articles = _inputs()
    _write('new.csv', text)
    _write('prev.csv', articles)
    assert len(text) > 3 * env['window_bytes'] and len(articles) > 2 * env['window_bytes']
    a = links.refresh_links('new.csv', 'prev.csv', 'out_a.csv', **env)
    one = links.refresh_links('new.csv', 'prev.csv', 'out_1.csv')
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    b = links.refresh_links('new.csv', 'prev.csv', 'out_b.csv', **env)
    monkeypatch.delenv('KW_LINKS_NATIVE')
    assert (a.route, one.route, b.route) == ('device', 'device', 'pandas')
    assert min(a.windows) > 1 and one.windows == b.windows == (0, 0)
    assert a.counts() == b.counts() == one.counts() and a.seen > 0 and a.duplicate > 0 and a.written > 0
    assert R.read_bytes('out_a.csv') == R.read_bytes('out_b.csv') == R.read_bytes('out_1.csv')
    # the split, round-robin into three files
    capsys.readouterr()
    a = links.split_links('new.csv', 'a', 3, 'prev.csv', **env)
    said = capsys.readouterr().out
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    b = links.split_links('new.csv', 'b', 3, 'prev.csv', **env)
    monkeypatch.delenv('KW_LINKS_NATIVE')
    assert (a.route, b.route) == ('device', 'pandas') and min(a.windows) > 1 and b.windows == (0, 0)
    assert a.counts() == b.counts() and a.parts == b.parts and said == 'CSV file has been split into 3 parts.\n'
    for i in range(3):
        assert R.read_bytes('a_%d.csv' % i) == R.read_bytes('b_%d.csv' % i)


def test_refresh_record_refusal_takes_pandas(env, monkeypatch):
    """An article longer than a window plus max_record_bytes: the streamed route leaves the call to pandas; the
    one-piece route takes the same files on the device; the bytes agree."""
    from advanced_scrapper_amd import links
    text, articles = _inputs(60, 20)
    articles += '%s,d,t,a,s,u,t,"%s"\r\n' % (_u(3), 'long, line\n' * (env['window_bytes'] // 2))
    _write('new.csv', text)
    _write('prev.csv', articles)
    a = links.refresh_links('new.csv', 'prev.csv', 'out_a.csv', **env)
    b = links.refresh_links('new.csv', 'prev.csv', 'out_b.csv')
    assert (a.route, b.route) == ('pandas', 'device') and a.counts() == b.counts()
    assert R.read_bytes('out_a.csv') == R.read_bytes('out_b.csv')


def test_remaining_urls_streamed(env, monkeypatch, capsys):
    from advanced_scrapper_amd import resume
    from tests.test_resume_host import write_files
    urls = [_u(k % 500) for k in range(900)]
    write_files(urls, success=[_u(k) for k in range(0, 500, 3)] * 2, failed=[_u(k) for k in range(1, 400, 7)] * 30)
    sizes = [os.path.getsize(f) for f in ('success_articles_yfin.csv', 'failed_articles_yfin.csv', 'yfin_urls.csv')]
    assert min(sizes) > 2 * env['window_bytes']
    capsys.readouterr()
    a = resume.remaining_urls(**env)
    out_a = capsys.readouterr().out
    one = resume.remaining_urls()
    capsys.readouterr()
    monkeypatch.setenv('KW_RESUME_NATIVE', '0')
    b = resume.remaining_urls(**env)
    out_b = capsys.readouterr().out
    assert (a.route, one.route, b.route) == ('device', 'device', 'pandas') and out_a == out_b
    assert min(a.windows) > 1 and one.windows == b.windows == (0, 0, 0)
    assert a.urls() == b.urls() == one.urls() and 0 < a.remaining < a.initial_total
    assert (a.initial_total, a.scraped_success, a.scraped_fails) == (b.initial_total, b.scraped_success, b.scraped_fails)


# ------------------------------------------------------------------ find_new_urls
def _new_urls_both(links, monkeypatch, capsys, env):
    capsys.readouterr()
    a = links.find_new_urls('new.csv', 'old.csv', 'out_a.csv', **env)
    said_a = capsys.readouterr().out
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    b = links.find_new_urls('new.csv', 'old.csv', 'out_b.csv', **env)
    said_b = capsys.readouterr().out
    monkeypatch.delenv('KW_LINKS_NATIVE')
    assert (a.route, b.route) == ('device', 'pandas')
    assert said_a.replace('out_a.csv', 'out_b.csv') == said_b
    assert R.read_bytes('out_a.csv') == R.read_bytes('out_b.csv')
    assert (a.counts(), a.unique_new, a.unique_old, a.unique_only_new) == \
        (b.counts(), b.unique_new, b.unique_old, b.unique_only_new)
    return a


def test_find_new_urls_streamed_counts_differ_from_rows(env, monkeypatch, capsys):
    """Repeats in both files and in the intersection: the three printed numbers are of unique URLs."""
    from advanced_scrapper_amd import links
    text, articles = _inputs()
    _write('new.csv', text)
    _write('old.csv', articles)
    a = _new_urls_both(links, monkeypatch, capsys, env)
    assert min(a.windows) > 1
    new, old = pd.read_csv('new.csv')['url'], pd.read_csv('old.csv')['url']
    assert (a.unique_new, a.unique_old, a.unique_only_new) == (new.nunique(), old.nunique(), len(set(new) - set(old)))
    assert a.unique_new < a.n_links and a.unique_old < len(old) and a.unique_only_new < a.written
    assert 0 < a.seen and new[new.isin(old)].nunique() < a.seen        # repeats inside the intersection
    # an old file in the links' own dialect, in one piece
    _write('old.csv', R.links_text([(5, _u(k)) for k in list(range(100, 300)) + [120, 120, 130]]))
    b = _new_urls_both(links, monkeypatch, capsys, {})
    assert b.windows == (0, 0) and b.unique_old == 200


def test_find_new_urls_adversarial_layouts(env, monkeypatch, capsys):
    """The layouts of test_exclude_unique_adversarial_rows, as files."""
    from advanced_scrapper_amd import links
    a = [_u(k) for k in range(10)]
    far = [_u(1000 + k) for k in range(700)]
    layouts = [([a[1]], [a[1], a[0], a[1], a[0], a[1]]),
               ([a[2]], [a[2]] * 200),
               ([a[3]], [a[2]] * 200),
               ([_u(100 + k) for k in range(10)], a),
               (a, a + a[:3]),
               ([a[0]], [a[5]] + far + [a[5], a[0], far[3]]),
               ([a[4][:-1], a[5] + 'l', a[4][:-1]], [a[4], a[5], 'a:b', 'a:', 'a:b'])]
    for k, (old, new) in enumerate(layouts):
        _write('old.csv', R.links_text([(7, u) for u in old]))
        _write('new.csv', R.links_text([(100 + i, u) for i, u in enumerate(new)]))
        res = _new_urls_both(links, monkeypatch, capsys, env if k % 2 else {})
        assert (res.unique_new, res.unique_old, res.unique_only_new) == \
            (len(set(new)), len(set(old)), len(set(new) - set(old))), k
        assert res.written == sum(u not in set(old) for u in new)


def test_find_new_urls_after_tag_collisions(env, monkeypatch, capsys):
    """A 4-bit hash: the seen rows' first holders come from the host's exact pass."""
    from advanced_scrapper_amd import links
    monkeypatch.setenv('KW_TEST_HOOKS', '1')
    monkeypatch.setenv('KW_TEST_DEDUP_WEAK_HASH', '1')
    rng = np.random.RandomState(11)
    pool = [_u(k) for k in range(700)]
    old = [pool[i] for i in rng.randint(0, 500, 3000)]
    new = [pool[i] for i in rng.randint(200, 700, 4000)]
    _write('old.csv', R.links_text([(7, u) for u in old]))
    _write('new.csv', R.links_text([(100 + i, u) for i, u in enumerate(new)]))
    res = _new_urls_both(links, monkeypatch, capsys, {})
    assert (res.unique_new, res.unique_old, res.unique_only_new) == \
        (len(set(new)), len(set(old)), len(set(new) - set(old)))


@pytest.mark.parametrize('case', ['plain', 'articles', 'missing_column', 'unreadable'])
def test_find_new_urls_against_the_golden(env, capsys, case):
    from advanced_scrapper_amd import links
    with open(GOLDEN, encoding='utf-8') as fh:
        g = json.load(fh)
    new, old, out = g['names']
    R.write_inputs({k: v for k, v in g['cases'][case]['inputs'].items() if v is not None})
    for kw in ({}, dict(env, window_bytes=1024, max_record_bytes=4096)):
        if os.path.exists(out):
            os.remove(out)
        capsys.readouterr()
        res = links.find_new_urls(new, old, out, **kw)
        assert capsys.readouterr().out == g['cases'][case]['stdout']
        want = g['cases'][case]['output']
        if want is None:
            assert res is None and not os.path.exists(out)
            continue
        assert res.route == 'device' and (min(res.windows) > 1) == bool(kw)
        assert R.read_bytes(out) == want.encode()
