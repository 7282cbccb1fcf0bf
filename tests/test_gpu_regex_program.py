"""GPU tests of the extended regex programs (sets, categories, assertions, lazy repeats, branches, host-resolved
names): positions against the CPU oracle, the engines' seams, the routes, and the reference's own output files."""
import io
import os
from collections import Counter

import pandas as pd
import pytest

from tests import regex_docs as rd

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'regex')


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _maps(m, texts, titles):
    from advanced_scrapper_amd.matcher import group_hits
    g = group_hits(m.match_strings(texts, titles))
    names = m.ckb.names
    return [tuple({names[p]: v for p, v in g.get(d, {}).get(f, {}).items()} for f in (0, 1)) for d in range(len(texts))]


@pytest.fixture(scope='module')
def oracle_results():
    """The documents and the oracle's results for them, computed once."""
    from oracle import kwmatch_oracle as orc
    texts, titles = rd.documents()
    o = orc.Oracle(rd.processed(rd.NAMES))
    return texts, titles, [o.field_results(s) for s in texts], [o.field_results(s) for s in titles]


def test_oracle_covers_every_construct(oracle_results):
    """Before any GPU result counts: per construct class the oracle alone decides at least 5 fields with a
    position and at least 1 with none."""
    _texts, _titles, want_t, want_i = oracle_results
    pos, empty = Counter(), Counter()
    for r in want_t + want_i:
        for name, v in r.items():
            (pos if v else empty)[rd.NAMES[name][0]] += 1
    for cls in rd.CLASSES:
        assert pos[cls] >= 5 and empty[cls] >= 1, (cls, pos[cls], empty[cls])


def test_regex_programs_vs_oracle(oracle_results):
    _gpu()
    from advanced_scrapper_amd import _native
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    test_oracle_covers_every_construct(oracle_results)
    texts, titles, want_t, want_i = oracle_results
    ckb = compile_kb(rd.processed(rd.NAMES))
    assert not any(ckb.host_regex)
    m = GpuMatcher(ckb)
    got = _maps(m, texts, titles)
    bad = [d for d in range(len(texts)) if got[d] != (want_t[d], want_i[d])]
    for d in bad[:4]:
        print(f'doc {d} {texts[d][:80]!r}: text {got[d][0]} want {want_t[d]}; title {got[d][1]} want {want_i[d]}')
    assert not bad, f'GPU differs from the oracle on docs {bad[:20]}'
    st = m.stats()
    assert st['regex_backtracking'] > 0 and st['regex_rounds'] > 0
    # the non-ASCII documents went both ways: names the view loses (sets with non-ASCII members, \b) to the
    # resolve kernel
    routes = Counter(m.doc_routes(len(texts)).tolist())
    assert routes[_native.KW_ROUTE_RESOLVE] > 0, routes
    m.close()


def test_ascii_set_programs_take_the_shift_and_search():
    """A KB of only ASCII-set fixed programs never runs the backtracking engine, on either view."""
    _gpu()
    from oracle import kwmatch_oracle as orc
    from advanced_scrapper_amd import _native
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    texts, titles = rd.documents(rd.FIXED_SET_NAMES)
    processed = rd.processed(rd.FIXED_SET_NAMES)
    m = GpuMatcher(compile_kb(processed))
    got = _maps(m, texts, titles)
    o = orc.Oracle(processed)
    bad = [d for d in range(len(texts)) if got[d] != (o.field_results(texts[d]), o.field_results(titles[d]))]
    assert not bad, f'GPU differs from the oracle on docs {bad[:20]}'
    st = m.stats()
    assert st['regex_backtracking'] == 0 and st['regex_rounds'] > 0, st
    routes = Counter(m.doc_routes(len(texts)).tolist())
    assert routes[_native.KW_ROUTE_TRANSCODE] > 0, routes      # ASCII sets stay decidable on the one-byte view
    m.close()


def _host_frame():
    texts, titles = rd.documents(['[24]7.ai', 'Toy|Toys R Us'])
    rows = []
    forms = ['Joe (Jr)? Joe Jr Joe ', 'a? banana', '(Wal|K)+mart Inc WalKmart Inc Kmart Inc mart Inc', 'Joe (Jr)? only Jo',
             'Acme (?=Corp)Corp Acme Corp', '(Tic)-\\1 Tac Tic-Tic Tac Tic-Tac', 'é (Wal|K)+mart Inc 中 WalWalmart Inc',
             'Joe (Jr)?', 'nothing here']
    for i in range(50):
        text = forms[i % len(forms)] + ' ' + texts[i * 7 % len(texts)][:200]
        title = forms[(i * 5 + 2) % len(forms)] if i % 3 else titles[i][:80]
        rows.append({'article_text': text, 'title': title, 'date_time': f'2019-03-01 10:{i:02d}:00', 'url': f'u{i}',
                     'source': 'yahoo', 'source_url': 's'})
    rows[7]['title'] = float('nan')
    return pd.DataFrame(rows)


def test_host_resolved_names_through_process_chunk(tmp_path, monkeypatch):
    """Names whose regex only re can run: the GPU decides, the writer finds the positions; the per-ticker files
    of process_chunk hold the oracle's ticker_matches for every article."""
    _gpu()
    import json
    from dateutil import parser
    from oracle import kwmatch_oracle as orc
    from advanced_scrapper_amd import match_keywords as mk
    processed = {'HOST': {'aliases': {n: (None, None) for n in rd.HOST_NAMES}},
                 'MIX': {'aliases': {'[24]7.ai': (None, None), 'Joe (Jr)?': (None, None), 'Toy|Toys R Us': (None, None)}}}
    frame = _host_frame()
    monkeypatch.chdir(tmp_path)
    os.makedirs('yahoo_ticker_matched_articles')
    mk.process_chunk('yahoo', frame, processed)
    o = orc.Oracle(processed)
    want = {}
    for i, row in frame.iterrows():
        tm = o.ticker_matches(mk.field_str(row['article_text']), mk.field_str(row['title']), parser.parse(row['date_time']))
        for t, v in tm.items():
            want.setdefault(t, []).append((row['url'], v['text'], v['title']))
    assert sorted(want) == ['HOST', 'MIX']
    assert any(p for _u, text, _t in want['HOST'] for p in text.values())      # positions, not only []
    for t in want:
        out = pd.read_csv(f'yahoo_ticker_matched_articles/{t}_match.csv')
        got = [(r['url'], json.loads(r['text_matches']), json.loads(r['title_matches'])) for _i, r in out.iterrows()]
        assert got == want[t], t
        assert [list(g[1]) for g in got] == [list(w[1]) for w in want[t]]       # and the names' order
    # the same rows through the in-memory API
    results, _err = mk.match_chunk(frame, processed)
    for i, row in frame.iterrows():
        assert results[i] == o.ticker_matches(mk.field_str(row['article_text']), mk.field_str(row['title']),
                                              parser.parse(row['date_time'])), i


def test_dropin_writes_the_references_files(tmp_path, monkeypatch):
    """The per-ticker CSVs of the drop-in equal, byte for byte, what the reference's process_chunk +
    sort_matched_csv wrote for the same KB and articles (tests/golden/make_regex_golden.py)."""
    _gpu()
    from advanced_scrapper_amd import match_keywords as mk
    processed = mk.read_and_process_json_files(os.path.join(GOLDEN, 'kb'))
    monkeypatch.chdir(tmp_path)
    os.makedirs('yahoo_ticker_matched_articles')
    with open(os.path.join(GOLDEN, 'articles.csv'), 'rb') as fh:
        data = fh.read()
    for chunk in pd.read_csv(io.BytesIO(data), chunksize=80):
        mk.process_chunk('yahoo', chunk, processed)
    for fn in os.listdir('yahoo_ticker_matched_articles'):
        mk.sort_matched_csv(f'yahoo_ticker_matched_articles/{fn}')
    want = {fn: open(os.path.join(GOLDEN, 'out', fn), 'rb').read() for fn in os.listdir(os.path.join(GOLDEN, 'out'))}
    got = {fn: open(os.path.join('yahoo_ticker_matched_articles', fn), 'rb').read()
           for fn in os.listdir('yahoo_ticker_matched_articles')}
    assert sorted(got) == sorted(want) and len(want) >= 3
    for fn in want:
        assert got[fn] == want[fn], fn
