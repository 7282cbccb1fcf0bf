"""GPU: the per-ticker match cells built on the device (csrc/kwrows.hip, include/kwrows.h) equal
rows.assemble_json_raw (csrc/kwrows.c) on the same records: the four arrays, element for element.

The cases are those of tests/rows_rule.py (the CPU tests hold its numpy restatement against the same host
route), the golden corpus through the real scan, and the drop-in with and without ``KW_ROWS_DEVICE=0``.
"""
import io
import os
import time

import numpy as np
import pandas as pd
import pytest

from tests import rows_rule as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


def _upload(torch, hits):
    """HIT_DTYPE records as a device tensor [max(n, 1), 4] (int32 view of kw_hit)."""
    a = np.zeros((max(len(hits), 1), 4), dtype=np.int32)
    a[:len(hits)] = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4).view(np.int32)
    return torch.from_numpy(a).to('cuda:0')


def _device(torch, case, handle=None):
    from advanced_scrapper_amd import rows as R
    t, hits, date_us, date_ok = case
    h = handle or R.DeviceRows(0, t.tuple(), t.n_tickers)
    try:
        d_hits = _upload(torch, hits)
        return h.run(d_hits, len(hits), np.asarray(date_us, np.int64), np.asarray(date_ok, np.uint8))
    finally:
        if handle is None:
            h.close()


def _check(torch, case, handle=None):
    want = RR.host_raw(*case)
    got = _device(torch, case, handle)
    assert RR.same(got, want)
    return want


# ------------------------------------------------------------------ 1. the golden corpus
@pytest.fixture(scope='module')
def env(golden, torch_gpu):
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    processed = golden.kb_processed()
    m = GpuMatcher(compile_kb(processed))
    yield {'processed': processed, 'm': m}
    m.close()


def test_golden_corpus(env, golden):
    from advanced_scrapper_amd import rows as R
    from advanced_scrapper_amd.dates import parse_date
    from advanced_scrapper_amd.matcher import field_str
    m = env['m']
    frame = golden.articles_frame()
    assert len(frame) == 642 and len(m.ckb.tickers) == 216
    hits = m.match_strings([field_str(v) for v in frame['article_text'].tolist()],
                           [field_str(v) for v in frame['title'].tolist()])
    dates = [parse_date(str(v)) if pd.notna(v) else None for v in frame['date_time'].tolist()]
    assert any(d is None for d in dates)
    assert m.fetched_is(hits)
    got = R.assemble_json_device(m, dates)
    want = R.assemble_json_raw(m.ckb, hits, dates)
    assert want is not None and len(want[0]) > 500
    assert RR.same(got, want)
    assert RR.cells_equal_in_order(RR.raw_cells(got, m.ckb.tickers, len(frame)), golden.matches())
    ms = m.rows_handle().last_ms()
    assert ms['total'] > 0 and ms['order'] + ms['expand'] + ms['render'] <= ms['total'] * 1.01 + 0.01


# ------------------------------------------------------------------ 2. hand-made records
def test_hand_made_records(torch_gpu):
    want = _check(torch_gpu, RR.hand_case())
    assert len(want[0]) == 11
    t, hits, date_us, date_ok = RR.hand_case()
    for h in (hits[:0], RR.records([(0, 0, 42, 1)])):
        _check(torch_gpu, (t, h, date_us, date_ok))
    none = _device(torch_gpu, (t, hits, [], []))
    assert [len(a) for a in none] == [0, 0, 0, 1] and none[3][0] == 0


# ------------------------------------------------------------------ 3. size boundaries
@pytest.mark.parametrize('m', [63, 64, 65, 512, 513, 1500, 20000])
def test_one_name_documents(torch_gpu, m):
    """Around a wave, around two blocks, several blocks, and far beyond any tile: one path, always exact."""
    _check(torch_gpu, RR.one_name_case(m))


def test_many_tickers_in_one_document(torch_gpu):
    want = _check(torch_gpu, RR.many_tickers_case(300))
    assert (want[0] == 1).sum() == 300


def test_random_records(torch_gpu):
    want = _check(torch_gpu, RR.random_case(4))
    assert len(want[0]) > 5000


# ------------------------------------------------------------------ 4. handle reuse
def test_handle_reuse(torch_gpu):
    from advanced_scrapper_amd import rows as R
    big = RR.random_case(5)
    t = big[0]
    small = (t, big[1][:700], big[2][:90], big[3][:90])
    h = R.DeviceRows(0, t.tuple(), t.n_tickers)
    try:
        first = _check(torch_gpu, big, h)
        _check(torch_gpu, small, h)
        _check(torch_gpu, (t, big[1][:0], big[2], big[3]), h)
        again = _device(torch_gpu, big, h)
        assert RR.same(again, first)
    finally:
        h.close()


# ------------------------------------------------------------------ 5. invalid regex
@pytest.mark.parametrize('in_period', [True, False])
def test_invalid_regex_verdict(torch_gpu, in_period):
    want = _check(torch_gpu, RR.invalid_case(in_period))
    assert (want is None) == in_period


# ------------------------------------------------------------------ 6. the drop-in
def _run_main(golden, tmp_path, monkeypatch, name):
    """match_keywords.run over the golden article CSV (the native chunk path); {file: bytes} and how often
    each route built the JSON cells."""
    from advanced_scrapper_amd import match_keywords as mk
    work = tmp_path / name
    work.mkdir()
    (work / 'articles.csv').write_bytes(golden.articles_csv_bytes())
    monkeypatch.setenv('TZ', 'UTC')
    time.tzset()
    monkeypatch.chdir(work)
    processed = golden.kb_processed()
    monkeypatch.setattr(mk, 'read_and_process_json_files', lambda _d: processed)
    calls = {'device': 0, 'host': 0}
    device, host = mk.assemble_json_device, mk.assemble_json_raw

    def spy_device(matcher, dates):
        calls['device'] += 1
        return device(matcher, dates)

    def spy_host(ckb, hits, dates):
        calls['host'] += 1
        return host(ckb, hits, dates)
    monkeypatch.setattr(mk, 'assemble_json_device', spy_device)
    monkeypatch.setattr(mk, 'assemble_json_raw', spy_host)
    args = mk._parse(['--info-dir', 'unused', '--articles', str(work / 'articles.csv'),
                      '--chunksize', str(golden.chunksize())])
    assert mk.run(args, 0, 1, None, None) == 0
    out = work / 'yahoo_ticker_matched_articles'
    return {fn: (out / fn).read_bytes() for fn in os.listdir(out)}, calls


def test_dropin_routes(torch_gpu, golden, tmp_path, monkeypatch):
    want = golden.outputs()
    monkeypatch.delenv('KW_ROWS_DEVICE', raising=False)
    got, calls = _run_main(golden, tmp_path, monkeypatch, 'device')
    assert calls['device'] > 0 and calls['host'] == 0
    assert sorted(got) == sorted(want) and all(got[fn] == want[fn] for fn in want)
    monkeypatch.setenv('KW_ROWS_DEVICE', '0')
    got, calls = _run_main(golden, tmp_path, monkeypatch, 'host')
    assert calls['host'] > 0 and calls['device'] == 0
    assert sorted(got) == sorted(want) and all(got[fn] == want[fn] for fn in want)


def test_only_the_last_fetch_takes_the_device_route(env, monkeypatch):
    from advanced_scrapper_amd import match_keywords as mk
    monkeypatch.delenv('KW_ROWS_DEVICE', raising=False)
    m = env['m']
    hits = m.match_strings(['ACME Widgets rose'], ['ACME'])
    assert mk._rows_on_device(m, hits, [None])
    assert not mk._rows_on_device(m, hits.copy(), [None])       # e.g. records gathered from other ranks
    m.scan_host(*_packed(['x'], ['y']), 1)
    assert not mk._rows_on_device(m, hits, [None])              # a newer scan's records are in HBM now
    m.fetch_host()
    monkeypatch.setenv('KW_ROWS_DEVICE', '0')
    assert not mk._rows_on_device(m, m.fetch_host(), [None])


def _packed(texts, titles):
    from advanced_scrapper_amd.matcher import pack_fields
    return pack_fields(texts, titles)


def test_host_regex_kb_takes_the_host_route(torch_gpu, monkeypatch):
    from advanced_scrapper_amd import match_keywords as mk
    from advanced_scrapper_amd import rows as R
    from advanced_scrapper_amd.dates import parse_date
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher, field_str
    monkeypatch.delenv('KW_ROWS_DEVICE', raising=False)
    golden_rx = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'regex')
    ckb = compile_kb(mk.read_and_process_json_files(os.path.join(golden_rx, 'kb')))
    assert sum(map(bool, ckb.host_regex)) >= 1
    frame = pd.read_csv(io.BytesIO(open(os.path.join(golden_rx, 'articles.csv'), 'rb').read()))
    m = GpuMatcher(ckb)
    try:
        hits = m.match_strings([field_str(v) for v in frame['article_text'].tolist()],
                               [field_str(v) for v in frame['title'].tolist()])
        dates = [parse_date(str(v)) if pd.notna(v) else None for v in frame['date_time'].tolist()]
        assert m.fetched_is(hits) and len(hits) and not mk._rows_on_device(m, hits, dates)
        monkeypatch.setattr(mk, 'assemble_json_device', lambda *_a: pytest.fail('the device route ran'))
        assert RR.same(mk._json_raw(m, hits, dates), R.assemble_json_raw(ckb, hits, dates))
    finally:
        m.close()

