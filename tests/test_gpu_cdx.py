"""GPU: CDX listings parsed and the URL CSVs rendered on the device (csrc/cdx.hip, kw_cdx_* of include/kwdedup.h).

Bar: bit-exact.  The kernel's verdict, offending line, rows and CSV bytes equal tests/cdx_rule.py's (which
tests/test_cdx_rule.py pins against pandas); the golden part and merged CSVs are the reference's own outputs; the
drop-in writes byte-identical files on the device route and on the pandas route (KW_CDX_NATIVE=0).
"""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

from oracle import dedup_oracle as dd
from tests import cdx_rule as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'dedup_golden.json.gz')
DIALECT = {R.LISTING: 'listing', R.PART: 'part'}


@pytest.fixture(scope='module')
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.cdx_dedup import GpuUrlDedup
    return GpuUrlDedup()


@pytest.fixture(scope='module')
def gold():
    with gzip.open(GOLD, 'rt', encoding='utf-8') as f:
        return json.load(f)


@pytest.fixture()
def dropin(gpu, monkeypatch):
    """cdx_dedup on the module's handle, with the pandas parse counted."""
    from advanced_scrapper_amd import cdx_dedup
    monkeypatch.setattr(cdx_dedup, '_DEDUP', gpu)
    calls = {'read_cdx': 0}
    real = cdx_dedup.read_cdx

    def counted(*a, **k):
        calls['read_cdx'] += 1
        return real(*a, **k)
    monkeypatch.setattr(cdx_dedup, 'read_cdx', counted)
    return cdx_dedup, calls


def _kept(rows, normalize=True):
    urls = [u.decode('utf-8') for _, u in rows]
    if normalize:
        kept, new = dd.dedup_rows(urls)
    else:
        kept = dd.keep_first(urls)
        new = [urls[i] for i in kept]
    return [(rows[i][0], u) for i, u in zip(kept, new)]


def _store_rows(gpu):
    arena, off, ts = gpu.cdx_rows()
    assert off[0] == 0 and len(off) == len(ts) + 1 and off[-1] == len(arena)
    return [(int(ts[i]), arena[off[i]:off[i + 1]]) for i in range(len(ts))]


def _check_text(gpu, text, dialect=R.LISTING, normalize=True):
    """One text through the kernel: everything equals the rule's."""
    v, bad, rows = R.parse(text, dialect)
    gpu.cdx_begin()
    got = gpu.cdx_append(text, DIALECT[dialect])
    assert got == (v, bad, len(rows) if v == R.OK else 0), (R.NAMES[v], bad, got, text[:200])
    if v != R.OK:
        assert _store_rows(gpu) == []
        return v
    assert _store_rows(gpu) == rows
    gpu.cdx_run(normalize)
    want = _kept(rows, normalize)
    assert gpu.cdx_csv() == R.render_csv(want)
    assert gpu.counts()[1] == len(want)
    return v


def _line(k, url=None, ts='20200102030405'):
    return ('k%d %s %s text/html 200 D 9' % (k, ts, url or 'https://finance.yahoo.com/news/a-%d.html' % k)).encode()


def _pad_to(size, k0=0):
    """Good lines of exactly `size` bytes in all, the last '\\n' included (size >= 40)."""
    out, k = [], k0
    while size - sum(len(x) + 1 for x in out) > 400:
        out.append(_line(k))
        k += 1
    rest = size - sum(len(x) + 1 for x in out)
    stem = b'p 1 http://p/'
    assert rest > len(stem) + 1
    out.append(stem + b'a' * (rest - len(stem) - 1))
    text = b'\n'.join(out) + b'\n'
    assert len(text) == size
    return text


# ------------------------------------------------------------------ golden
def test_golden_parts(gpu, gold):
    for p in gold['parts']:
        gpu.cdx_begin()
        v, bad, n = gpu.cdx_append(gold['cdx'][p].encode('utf-8'), 'listing')
        assert (v, bad) == (R.OK, -1) and n > 0, p
        gpu.cdx_run(normalize=True)
        assert gpu.cdx_csv() == gold['part_csv'][p].encode('utf-8'), p


def test_golden_merge_of_part_csvs(gpu, gold):
    order = [n[len('yahoo_'):-len('.csv')] for n in gold['glob_order']]
    gpu.cdx_begin()
    for p in order:
        assert gpu.cdx_append(gold['part_csv'][p].encode('utf-8'), 'part')[:2] == (R.OK, -1), p
    gpu.cdx_run(normalize=False)
    assert gpu.cdx_csv() == gold['merged_csv'].encode('utf-8')


def test_golden_merge_of_raw_listings(gpu, gold):
    order = [n[len('yahoo_'):-len('.csv')] for n in gold['glob_order']]
    gpu.cdx_begin()
    for p in order:
        assert gpu.cdx_append(gold['cdx'][p].encode('utf-8'), 'listing')[:2] == (R.OK, -1), p
    gpu.cdx_run(normalize=True)
    assert gpu.cdx_csv() == gold['merged_csv'].encode('utf-8')


# ------------------------------------------------------------------ the kernel against the rule
@pytest.mark.parametrize('dialect', [R.LISTING, R.PART], ids=['listing', 'part'])
def test_fuzz_kernel_equals_rule(gpu, dialect):
    seen = set()
    for text in R.fuzz_listings(300, dialect):
        seen.add(_check_text(gpu, text, dialect, normalize=dialect is R.LISTING))
    assert R.OK in seen and len(seen) >= 8


def test_refused_text_leaves_the_store_unchanged(gpu):
    good_a = b'\n'.join(_line(k) for k in range(70)) + b'\n'
    good_b = b'\n'.join(_line(k, ts='7') for k in range(35, 140))
    rows_a, rows_b = R.parse(good_a)[2], R.parse(good_b)[2]
    bad = [t for t in R.fuzz_listings(300) if R.parse(t)[0] != R.OK]
    picked = {}
    for t in bad:
        picked.setdefault(R.parse(t)[0], t)
    assert len(picked) == 7   # every listing-dialect verdict
    gpu.cdx_begin()
    assert gpu.cdx_append(good_a) == (R.OK, -1, len(rows_a))
    for v, t in sorted(picked.items()):
        want = R.parse(t)
        assert gpu.cdx_append(t) == (want[0], want[1], 0)
        assert _store_rows(gpu) == rows_a
    assert gpu.cdx_append(b'nonsense', 'part') == (R.HEADER, 0, 0)
    assert gpu.cdx_append(good_b) == (R.OK, -1, len(rows_b))
    assert _store_rows(gpu) == rows_a + rows_b   # consecutive numbering across the appends
    gpu.cdx_run()
    assert gpu.cdx_csv() == R.render_csv(_kept(rows_a + rows_b))


# ------------------------------------------------------------------ boundaries
def test_length_sweep_around_tile_edges(gpu):
    T = gpu.cdx_tile_bytes()
    for k in (1, 2):
        for d in (-2, -1, 0, 1, 2):
            text = _pad_to(k * T + d)
            assert _check_text(gpu, text) == R.OK
            assert _check_text(gpu, text[:-1] + b'b') == R.OK   # the same length without the final '\n'


@pytest.mark.parametrize('what', ['line_end', 'delimiter', 'ts_first', 'ts_last'])
def test_byte_kinds_on_a_tile_edge(gpu, what):
    T = gpu.cdx_tile_bytes()
    probe = _line(7, ts='12345678901234')
    at = {'line_end': len(probe), 'delimiter': probe.index(b' '), 'ts_first': probe.index(b'1234'),
          'ts_last': probe.index(b'1234') + 13}[what]
    tail = b'\n' + b'\n'.join(_line(k) for k in range(100, 110)) + b'\n'
    for pos in (T - 1, T):
        text = _pad_to(pos - at) + probe + tail
        assert text[pos:pos + 1] == (probe + b'\n')[at:at + 1]
        assert _check_text(gpu, text) == R.OK
        # the same with a non-digit there: refused with the rule's verdict
        if what.startswith('ts'):
            assert _check_text(gpu, text[:pos] + b'x' + text[pos + 1:]) == R.TS


def test_line_longer_than_tiles(gpu):
    T = gpu.cdx_tile_bytes()
    url = ('https://finance.yahoo.com/news/' + 'q' * (3 * T) + ',é.html?z').encode('utf-8')
    text = _line(1) + b'\n' + _line(2, url.decode()) + b'\n' + _line(3) + b'\n' + _line(2, url.decode())
    assert len(_line(2, url.decode())) > 3 * T
    assert _check_text(gpu, text) == R.OK
    assert _check_text(gpu, text, normalize=False) == R.OK


def test_blank_line_run_across_a_tile_edge(gpu):
    T = gpu.cdx_tile_bytes()
    for lead in (T - 3, T - 1, T, 2 * T - 2):
        text = _pad_to(lead) + b'\n' * 6 + _line(1) + b'\n\n' + _line(2)
        assert _check_text(gpu, text) == R.OK
    assert _check_text(gpu, b'\n' * (T + 5) + _line(1) + b'\n' * T) == R.OK


def test_no_rows_and_one_row(gpu):
    for text in (b'', b'\n', b'\n\n\n'):
        assert _check_text(gpu, text) == R.OK
        assert gpu.cdx_csv() == b'date_time,url\n'
    assert _check_text(gpu, b'date_time,url', R.PART, normalize=False) == R.OK
    assert _check_text(gpu, b'date_time,url\n', R.PART, normalize=False) == R.OK
    assert _check_text(gpu, _line(1)) == R.OK
    assert _check_text(gpu, b' 5 a:b.html') == R.OK
    assert gpu.cdx_csv() == b'date_time,url\n5,a:b.html\n'


@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257])
def test_row_counts(gpu, n):
    text = b'\n'.join(_line(k) for k in range(n))
    assert _check_text(gpu, text) == R.OK
    assert len(_store_rows(gpu)) == n


# ------------------------------------------------------------------ rendering
def test_render_commas_digits_non_ascii(gpu):
    urls = ['http://x/a,b.html', 'https://x/,.html?q', 'https://x/é,ü-€.html', 'https://x/\U0001F600.html',
            'https://x/plain.html', 'https://x/nocomma.html,after', ',:x.html', 'https://x/a,b.html']
    tss = ['0', '5', '20200102030405', '00000000000007', '123456789012345678', '999999999999999999', '1' + '0' * 17, '10']
    text = '\n'.join('k %s %s m' % (t, u) for t, u in zip(tss, urls)).encode('utf-8')
    assert _check_text(gpu, text) == R.OK
    csv = gpu.cdx_csv()
    assert b'\n0,"https://x/a,b.html"\n' in csv and b'\n7,' in csv and b'\n999999999999999999,' in csv
    assert csv.count(b'"') == 2 * 4
    assert _check_text(gpu, text, normalize=False) == R.OK


@pytest.mark.parametrize('n', [255, 256, 257, 1023, 1024, 1025, 2049])
def test_render_kept_counts_around_scan_edges(gpu, n):
    text = b'\n'.join(_line(k, 'https://x/%d%s.html' % (k, ',' * (k % 3 == 0)), ts=str(10 ** (k % 18))) for k in range(n))
    assert _check_text(gpu, text) == R.OK
    assert gpu.counts()[1] == n


# ------------------------------------------------------------------ synthetic rows
def test_synthetic_listing_equals_pandas_route(gpu, dropin):
    from advanced_scrapper_amd import synth
    cdx_dedup, _ = dropin
    text = synth.generate_urls(60000, seed=1).cdx_text()
    gpu.cdx_begin()
    assert gpu.cdx_append(text.encode('utf-8'), 'listing') == (R.OK, -1, 60000)
    gpu.cdx_run()
    got = gpu.cdx_csv()
    want = cdx_dedup.dedup_frame(cdx_dedup.read_cdx(text, is_text=True)).to_csv(index=False).encode('utf-8')
    assert got == want
    ms = gpu.cdx_last_ms()
    assert len(ms) == 3 and all(m > 0 for m in ms)


# ------------------------------------------------------------------ the drop-in
def test_dropin_routes_write_the_same_files(gpu, gold, dropin, tmp_path, monkeypatch, capsys):
    cdx_dedup, calls = dropin
    outs = {}
    d = tmp_path / 'yahoo_links_1'   # one folder for both routes: the same glob order
    os.makedirs(d)
    for p in gold['parts']:
        (d / f'yahoo_{p}.txt').write_bytes(gold['cdx'][p].strip().encode('utf-8'))
        (d / f'yahoo_{p}.csv').write_bytes(b'')
    (d / 'yahoo_empty.csv').write_bytes(b'')                      # unreadable: printed and skipped
    (d / 'yahoo_hdr.csv').write_bytes(b'date_time,url\n')         # header only
    for route in ('native', 'pandas'):
        if route == 'native':
            monkeypatch.delenv('KW_CDX_NATIVE', raising=False)
        else:
            monkeypatch.setenv('KW_CDX_NATIVE', '0')
        calls['read_cdx'] = 0
        for p in gold['parts']:
            cdx_dedup.process_part(str(d / f'yahoo_{p}.txt'), str(d / f'yahoo_{p}.csv'))
        assert calls['read_cdx'] == (0 if route == 'native' else len(gold['parts']))   # no silent fall-back
        capsys.readouterr()
        n = cdx_dedup.merge_parts(str(d), str(tmp_path / f'yfin_{route}.csv'))
        printed = capsys.readouterr().out.replace(f'yfin_{route}.csv', 'yfin.csv')
        outs[route] = (n, printed, {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.endswith('.csv')},
                       (tmp_path / f'yfin_{route}.csv').read_bytes())
    assert outs['native'] == outs['pandas']
    n, printed, files, merged = outs['native']
    assert 'Error reading' in printed and f'Found {n} unique URLs' in printed
    for p in gold['parts']:
        assert files[f'yahoo_{p}.csv'] == gold['part_csv'][p].encode('utf-8')
    assert merged.count(b'\n') == n + 1


_INELIGIBLE = {
    R.QUOTE: b'k 1 "https://x/a.html"\nk 2 https://x/b.html\n',
    R.CR: b'k 1 https://x/a.html\r\nk 2 https://x/b.html\r\n',
    R.NUL: b'k 1 https://x/a.html\nk 2 https://x/\0b.html\n',
    R.FIELDS: b'k 1 https://x/a.html\nk 2\n',
    R.TS: b'k 1 https://x/a.html\nk 2020-01-02 https://x/b.html\n',
    R.URL: b'k 1 https://x/a.html\nk 2 nan\n',
    R.UTF8: b'k 1 https://x/a.html\nk 2 https://x/\xffb.html\n',
}


@pytest.mark.parametrize('verdict', sorted(_INELIGIBLE), ids=lambda v: R.NAMES[v])
def test_ineligible_listing_takes_the_pandas_route(gpu, dropin, tmp_path, monkeypatch, verdict):
    cdx_dedup, calls = dropin
    text = _INELIGIBLE[verdict]
    gpu.cdx_begin()
    assert gpu.cdx_append(text)[0] == verdict == R.parse(text)[0]
    (tmp_path / 'in.txt').write_bytes(text)
    res = {}
    for route in ('native', 'pandas'):
        if route == 'native':
            monkeypatch.delenv('KW_CDX_NATIVE', raising=False)
        else:
            monkeypatch.setenv('KW_CDX_NATIVE', '0')
        out = tmp_path / f'{route}.csv'
        try:
            cdx_dedup.process_part(str(tmp_path / 'in.txt'), str(out))
            res[route] = ('file', out.read_bytes())
        except Exception as e:
            res[route] = (type(e), str(e))
    assert calls['read_cdx'] == 2
    assert res['native'] == res['pandas']


def test_ineligible_part_takes_the_pandas_route(gpu, dropin, tmp_path, monkeypatch, capsys):
    cdx_dedup, _ = dropin
    d = tmp_path / 'parts'
    os.makedirs(d)
    (d / 'a.csv').write_bytes(b'date_time,url\n1,https://x/a.html\n2,https://x/b.html\n')
    (d / 'b.csv').write_bytes(b'date_time,url\n3,"https://x/a,b.html"\n4,https://x/a.html\n')   # quoted: the pandas route
    gpu.cdx_begin()
    assert gpu.cdx_append((d / 'b.csv').read_bytes(), 'part')[0] == R.QUOTE
    res = {}
    for route in ('native', 'pandas'):
        if route == 'native':
            monkeypatch.delenv('KW_CDX_NATIVE', raising=False)
        else:
            monkeypatch.setenv('KW_CDX_NATIVE', '0')
        n = cdx_dedup.merge_parts(str(d), str(tmp_path / f'{route}.csv'))
        res[route] = (n, capsys.readouterr().out.replace(route, ''), (tmp_path / f'{route}.csv').read_bytes())
    assert res['native'] == res['pandas'] and res['native'][0] == 3


# ------------------------------------------------------------------ the C-ABI's argument checks
def test_bad_arguments_are_refused_on_the_host(gpu):
    import torch
    from advanced_scrapper_amd import _native
    L = _native.lib()
    dia = _native.CdxDialect(ord(' '), 1, 2, 0, 0)
    rows, verdict, bad = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
    out = (ctypes.byref(rows), ctypes.byref(verdict), ctypes.byref(bad))
    text = torch.zeros(64, dtype=torch.uint8, device='cuda')
    assert L.kw_cdx_begin(None) == _native.KW_EINVAL
    assert L.kw_cdx_append(None, _native.ptr(text), 8, ctypes.byref(dia), *out, None) == _native.KW_EINVAL
    assert L.kw_cdx_append(gpu.h, None, 8, ctypes.byref(dia), *out, None) == _native.KW_EINVAL
    assert L.kw_cdx_append(gpu.h, _native.ptr(text), -1, ctypes.byref(dia), *out, None) == _native.KW_EINVAL
    assert L.kw_cdx_append(gpu.h, _native.ptr(text), 8, None, *out, None) == _native.KW_EINVAL
    assert L.kw_cdx_append(gpu.h, _native.ptr(text), 8, ctypes.byref(dia), None, None, None, None) == _native.KW_EINVAL
    assert L.kw_cdx_append(gpu.h, ctypes.c_void_p(text.data_ptr() + 1), 8, ctypes.byref(dia), *out, None) == _native.KW_EINVAL
    for d in (_native.CdxDialect(ord(':'), 1, 2, 0, 0), _native.CdxDialect(ord(' '), -1, 2, 0, 0),
              _native.CdxDialect(ord(' '), 1, 1, 0, 0), _native.CdxDialect(ord(' '), 1, 2, 2, 0),
              _native.CdxDialect(ord(','), 0, 1, 1, 1)):
        assert L.kw_cdx_append(gpu.h, _native.ptr(text), 8, ctypes.byref(d), *out, None) == _native.KW_EINVAL
    assert b'kw_cdx_append' in L.kw_dedup_last_error(gpu.h)
    nb = ctypes.c_int64()
    assert L.kw_cdx_csv_size(gpu.h, None, None) == _native.KW_EINVAL
    assert L.kw_cdx_last_ms(gpu.h, None, 3) == _native.KW_EINVAL
    # the renderer only follows a kw_cdx_run over the store
    gpu.cdx_begin()
    assert gpu.cdx_append(_line(1)) == (R.OK, -1, 1)
    assert L.kw_cdx_csv_size(gpu.h, ctypes.byref(nb), None) == _native.KW_ESTATE
    gpu.cdx_run()
    assert L.kw_cdx_csv_copy(gpu.h, _native.ptr(text), None) == _native.KW_ESTATE   # no size yet
    assert L.kw_cdx_csv_size(gpu.h, ctypes.byref(nb), None) == _native.KW_OK
    assert L.kw_cdx_csv_copy(gpu.h, None, None) == _native.KW_EINVAL
    gpu.dedup_strings(['https://x/other.html'])   # another run on the handle: the kept rows are no longer the store's
    assert L.kw_cdx_csv_size(gpu.h, ctypes.byref(nb), None) == _native.KW_ESTATE
    assert L.kw_cdx_tile_bytes() % 16 == 0
