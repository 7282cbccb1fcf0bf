"""CPU: the rule of the per-ticker CSV rows (tests/emit_rule.py) equals the host emitter kwcsv_emit_mt on every
case the GPU tests use -- bytes, line_off, flags and the rows' order -- and, on a seeded subset, the reference's
own writer (one single-row DataFrame.to_csv per row).  This pins the yardstick before the GPU sees it.  Also
here, without a GPU: the library exports the emit entry points, and match_keywords._native_rows keeps the host
emitter where the device route does not apply.
"""
import datetime
import io
import re
import subprocess
import types

import numpy as np
import pandas as pd
import pytest

from tests import emit_rule as ER

CASES = ER.cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_rule_equals_host_emitter(name):
    case = CASES[name]()
    want = ER.host_emit(case)
    assert ER.same(ER.rule(case), want)
    if name.startswith('nul_rows'):
        assert want is None
    elif name in ('nul_no_rows', 'nul_beyond_prefix'):
        assert want is not None and len(want[0]) > 0
    if name == 'no_rows' or name == 'prefix_0':
        assert want[1].tolist() == [0] and want[0] == b''


def test_rule_equals_host_emitter_fuzz():
    nul = 0
    for seed in range(200):
        case = ER.fuzz_case(seed)
        want = ER.host_emit(case)
        assert ER.same(ER.rule(case), want), seed
        nul += want is None
    assert 0 < nul < 100


def test_flag_bits_of_known_cells():
    """The flag rule on cells whose class is known by hand."""
    w = {b: ER.witness(b) for b in ER.WITNESS}
    for b in (b'12', b'-1.5e3', b' 7 ', b'TRUE', b'false', b'+inf', b'Infinity', b'1e', b'-Infinity', b'\t-INF\t', b'e',
              b'.', b'--'):
        assert not w[b], b
    for b in (b'   ', b' \t ', b'1,2', 'é'.encode(), b'', b'+true', b'inf inity', b'1 2', b'infinit', b'tru', b'0x10',
              b'1_000', b'nan'):
        assert w[b], b
    got = ER.rule(ER.geometry_case('cr_only'))
    assert (got[2] & (1 << 16)).all() and got[0][:got[1][1]].endswith(b',\r\r\r\r\r\n')      # written as it is
    got = ER.rule(ER.na_case())
    all_na = got[2][got[3] == 2]
    assert len(all_na) == 1 and (int(all_na[0]) >> 8) & 0xFF == 0b11111001 and int(all_na[0]) & 0xFF == 6


def _pandas_lines(case):
    """The reference's writer: one single-row frame per row (match_keywords.py:131-146), NA cells as NaN."""
    row_doc, row_ti, jbuf, joff = case.raw()
    order = np.argsort(row_ti[:case.use()], kind='stable')
    c, jb = case.cells, jbuf.tobytes().decode('ascii')
    names = list(__import__('advanced_scrapper_amd.egress', fromlist=['x'])._HEADER_COLUMNS)
    out = []
    for r in order.tolist():
        d = int(row_doc[r])
        vals = [c.value(d, int(col)) for col in case.cols]
        row = [int(case.stamps[d]), vals[0], jb[joff[2 * r]:joff[2 * r + 1]], jb[joff[2 * r + 1]:joff[2 * r + 2]]] + vals[1:]
        s = io.StringIO()
        pd.DataFrame([dict(zip(names, row))]).to_csv(s, header=False, index=False)
        out.append(s.getvalue().encode('utf-8'))
    return b''.join(out)


@pytest.mark.parametrize('name', ['len_65', 'geo_quote_63_64', 'geo_cr_only', 'geo_crlf_inside', 'geo_utf8_straddle',
                                  'na_cells', 'witness', 'json', 'stamps', 'prefix_4', 'cols_9', 'gaps'])
def test_rule_equals_the_reference_writer(name):
    case = CASES[name]()
    if name == 'na_cells':
        assert ER.rule(case) is not None
    assert ER.rule(case)[0] == _pandas_lines(case)


def test_rule_equals_the_reference_writer_fuzz():
    seen = 0
    for seed in range(0, 200, 5):
        case = ER.fuzz_case(seed)
        got = ER.rule(case)
        if got is None:
            continue
        seen += 1
        assert got[0] == _pandas_lines(case), seed
    assert seen > 20


# ------------------------------------------------------------------ the library and the route
NEW_SYMBOLS = ('kw_rows_cells', 'kw_rows_emit', 'kw_rows_emit_result', 'kw_rows_copy_index', 'kw_rows_emit_last_ms')


def test_library_exports_the_emit_symbols():
    from advanced_scrapper_amd import _native
    L = _native.lib()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True).stdout
    for f in NEW_SYMBOLS:
        assert f in _native.EXPORTS and hasattr(L, f), f
        assert re.search(rf'\bT {f}\b', out), f


def _native_chunk():
    from advanced_scrapper_amd import ingest
    data = (b'date_time,title,url,source,source_url,article_text\n'
            b'2024-01-02 03:04:05,One,http://a,src,http://s,ACME rose\n'
            b'2024-01-03 03:04:05,Two,http://b,src,http://s,"ACME, again"\n')
    chunk = next(iter(ingest.read_chunks_bytes(data, 100)))
    assert isinstance(chunk, ingest.NativeChunk)
    return chunk


def _route(monkeypatch, chunk, env, on_device):
    """Which renderer _native_rows takes; the renderers and the JSON routes are stand-ins."""
    from advanced_scrapper_amd import egress, match_keywords as mk
    if env is None:
        monkeypatch.delenv('KW_EMIT_DEVICE', raising=False)
    else:
        monkeypatch.setenv('KW_EMIT_DEVICE', env)
    monkeypatch.setenv('TZ', 'UTC')
    calls = []
    raw = (np.array([0, 1], np.int32), np.array([0, 0], np.int32), np.frombuffer(b'{}{}{}{}', np.uint8), np.arange(0, 9, 2))
    matcher = types.SimpleNamespace(ckb=types.SimpleNamespace(tickers=['T0'], host_regex=[False]), rows_copy_json=True)

    def index_only(m, _dates):
        calls.append(('index', m.rows_copy_json))
        return raw[0], raw[1], None, None
    monkeypatch.setattr(mk, '_rows_on_device', lambda *_a: on_device)
    monkeypatch.setattr(mk, 'assemble_json_device', index_only)
    monkeypatch.setattr(mk, 'assemble_json_raw', lambda *_a: calls.append(('json_host',)) or raw)
    monkeypatch.setattr(egress, 'render_native', lambda *_a: calls.append(('host',)) or [])
    monkeypatch.setattr(egress, 'render_device', lambda _c, _m, _s, k: calls.append(('device', k)) or [])
    dates = [datetime.datetime(2024, 1, 2, tzinfo=datetime.timezone.utc), datetime.datetime(2024, 1, 3, tzinfo=datetime.timezone.utc)]
    got = mk._native_rows(chunk, matcher, np.zeros(1), dates, None)
    assert matcher.rows_copy_json is True
    return got, calls


def test_native_rows_keeps_the_host_emitter(monkeypatch):
    chunk = _native_chunk()
    got, calls = _route(monkeypatch, chunk, '0', True)
    assert got is not None and ('host',) in calls and not any(c[0] == 'device' for c in calls)
    got, calls = _route(monkeypatch, chunk, '1', False)
    assert got is not None and calls == [('json_host',), ('host',)]
    got, calls = _route(monkeypatch, chunk.frame(), '1', True)
    assert got is None and calls == []


def test_native_rows_takes_the_device_emitter_when_asked(monkeypatch):
    got, calls = _route(monkeypatch, _native_chunk(), '1', True)
    assert got is not None and calls == [('index', False), ('device', 2)]     # the JSON text was not asked for
