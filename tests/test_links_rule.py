"""CPU: the link refresh / split rule (tests/links_rule.py) against pandas, and the drop-ins' pandas routes against
fixtures the reference's own experiental/drop.py and split.py wrote (tests/golden/make_links_golden.py)."""
import io
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import links_rule as R


@pytest.mark.parametrize('n', [0, 1, 2, 16, 17, 300, 5000])
def test_descending_order_is_pandas(n):
    """Keys with many ties, at sizes on both sides of numpy's small-array and vectorised sorts."""
    keys = R.tied_keys(n)
    assert n < 3 or len(np.unique(keys)) < n
    df = pd.DataFrame({'date_time': keys, 'row': np.arange(n, dtype=np.int64)})
    want = df.sort_values(by='date_time', ascending=False)['row'].to_numpy()
    got = R.descending(keys)
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    from advanced_scrapper_amd import links
    assert links.descending_order(keys).tolist() == want.tolist()
    # all keys equal, and already descending / ascending
    for k in (np.full(n, 7, dtype=np.int64), np.arange(n, dtype=np.int64)[::-1].copy(), np.arange(n, dtype=np.int64)):
        d = pd.DataFrame({'date_time': k, 'row': np.arange(n)})
        assert R.descending(k).tolist() == d.sort_values(by='date_time', ascending=False)['row'].tolist()


def test_golden_fixture_is_what_the_issue_asks_for():
    g = R.golden()
    new = pd.read_csv(io.StringIO(g['inputs']['yahoo_links_1.csv']))
    prev = pd.read_csv(io.StringIO(g['inputs']['yahoo_articles_all.csv']))
    assert new['date_time'].is_unique                                       # no tie: the order is numpy-independent
    assert new['url'].str.contains(',').any() and new['url'].duplicated().any()
    assert new['url'].isin(prev['url']).any() and not new['url'].isin(prev['url']).all()
    assert re.search(r'^0\d+,', g['inputs']['yahoo_links_1.csv'], re.M)     # a leading-zero timestamp
    assert g['num_parts'] == 2 and g['split_last_line'] == 'CSV file has been split into 2 parts.'
    # the restated frames give the reference's files
    assert R.refresh_frame(new, prev).to_csv(index=False) == g['outputs']['yahoo_links_new.csv']
    df = pd.read_csv(io.StringIO(g['inputs'][R.SPLIT_NAMES['input_file']]))
    drop = pd.read_csv(io.StringIO(g['inputs'][R.SPLIT_NAMES['drop_file']]))
    assert df['url'].duplicated().any() and len(df[~df['url'].isin(drop['url'])]) % 2 == 1
    for i, part in enumerate(R.split_frames(df, drop, 2)):
        assert part.to_csv(index=False) == g['outputs']['parts/yfin_2025_%d.csv' % i]


@pytest.mark.parametrize('which', ['commas', 'plain'])
def test_pandas_routes_against_the_golden_fixture(monkeypatch, tmp_path, capsys, which):
    from advanced_scrapper_amd import links
    g = R.golden()
    if which == 'plain':      # the set without ',' URLs among the links (the one the device route can take)
        g = dict(g, **g['plain'])
        assert '"' not in g['inputs']['yahoo_links_1.csv'] + g['inputs'][R.SPLIT_NAMES['input_file']]
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    R.write_inputs(g['inputs'])
    res = links.refresh_links()
    assert R.read_bytes('yahoo_links_new.csv') == g['outputs']['yahoo_links_new.csv'].encode()
    new = pd.read_csv('yahoo_links_1.csv')
    prev = pd.read_csv('yahoo_articles_all.csv')
    seen = int(new['url'].isin(prev['url']).sum())
    written = g['outputs']['yahoo_links_new.csv'].count('\n') - 1
    assert res.route == 'pandas' and res.counts() == (len(new), seen, len(new) - seen - written, written)
    assert res.duplicate > 0 and res.seen > 0
    capsys.readouterr()
    res = links.split_links(num_parts=2, **R.SPLIT_NAMES)
    said = capsys.readouterr().out
    assert said.splitlines()[-1] == g['split_last_line']
    for i in range(2):
        name = 'parts/yfin_2025_%d.csv' % i
        assert R.read_bytes(name) == g['outputs'][name].encode()
    assert res.route == 'pandas' and res.duplicate == 0 and res.written == sum(res.parts)
    assert res.parts == [g['outputs']['parts/yfin_2025_%d.csv' % i].count('\n') - 1 for i in range(2)]
    assert res.n_links - res.seen == res.written


def test_pandas_route_keeps_the_reference_exceptions(monkeypatch, tmp_path):
    from advanced_scrapper_amd import links
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    with pytest.raises(FileNotFoundError):
        links.refresh_links()
    R.write_inputs(R.golden()['inputs'])
    with pytest.raises(ZeroDivisionError):
        links.split_links(num_parts=0, **R.SPLIT_NAMES)


def test_new_symbols_are_exported():
    from advanced_scrapper_amd import _native
    L = _native.lib()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True).stdout
    for f in ('kw_cdx_run_exclude_unique', 'kw_cdx_exclude_duplicates', 'kw_cdx_selected_ts', 'kw_cdx_csv_select_size',
              'kw_cdx_csv_select_copy', 'kw_cdx_select_last_ms'):
        assert f in _native.EXPORTS and hasattr(L, f), f
        assert getattr(L, f).argtypes is not None, f
        assert re.search(rf'\bT {f}\b', out), f
