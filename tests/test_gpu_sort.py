"""GPU: the output sort on the device (csrc/kwsort.hip, advanced_scrapper_amd/sortfiles.py) against the plain
Python rule of tests/sort_rule.py and against pandas: every case of the rule's table through ``sort_file`` and
``sort_matched_csv``; the ingest's record spans against the host tokenizer's; the gather kernel's geometry (tiny
rows, rows past a wave's and a block's span, all 16 source phases, a ragged end, several trips of every grid)
against the plain permutation of the spans; the order's range check; and a re-run of ``main()`` into a directory
that already holds the first run's files."""
import contextlib
import io
import os
import time

import numpy as np
import pytest

from tests import sort_rule as S

pytestmark = pytest.mark.gpu
SORT_HOOK, INGEST_HOOK = 'KW_TEST_SORT_GRID', 'KW_TEST_INGEST_GRID'

_DECIDED = {}


def decided(name, data):
    """(outcome, row, the rule's bytes, pandas' bytes -- None where the reference's pandas raises)."""
    if name not in _DECIDED:
        try:
            pandas = S.pandas_bytes(data)
        except Exception:   # noqa: BLE001 - the reference prints the error and leaves the file as it is
            pandas = None
        _DECIDED[name] = S.decide(data) + (pandas,)
    return _DECIDED[name]


@pytest.fixture(scope='module')
def gpu():
    """A device and the built library (libkwmatch's own hipGetDeviceCount: these tests run on the product's own
    staging, upload and kernels, without torch)."""
    from advanced_scrapper_amd import _native
    if _native.device_count() < 1:
        pytest.skip('no GPU')
    return _native


@pytest.fixture(scope='module')
def sorter(gpu):
    from advanced_scrapper_amd import sortfiles
    s = sortfiles.DeviceSorter(0)
    yield s
    s.close()


# ------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize('name,data', S.CASES, ids=[n for n, _ in S.CASES])
def test_table_case(gpu, sorter, tmp_path, monkeypatch, name, data):
    from advanced_scrapper_amd import match_keywords as mk
    from advanced_scrapper_amd import sortfiles
    outcome, row, expected, pandas = decided(name, data)
    path = tmp_path / 'X_match.csv'
    path.write_bytes(data)
    sortfiles.reset_stats()
    took = sorter.sort_file(str(path))
    last = sortfiles.LAST_STATS['last']
    assert took == (outcome == 'OK'), (name, outcome, last)
    if took:
        assert expected == pandas
        assert path.read_bytes() == pandas
        assert last['verdict'] == 'OK'
        assert last['route'] == ('unchanged' if data == pandas else 'device')
    else:
        assert path.read_bytes() == data, 'a refused file was touched'
        if outcome.startswith('sort-'):
            assert ('sort-' + last['verdict'], last['row']) == (outcome, row)
        else:
            assert last['verdict'] == outcome
        assert sortfiles.LAST_STATS['refused'] == {outcome: 1}
    # the drop-in then ends at pandas' bytes whichever route the file takes (where the reference's pandas raises,
    # at the reference's own end: the error printed, the file as it was), and where the host routes alone end
    path.write_bytes(data)
    monkeypatch.setattr(sortfiles, '_SORTER', sorter)
    monkeypatch.setattr(sortfiles, '_AVAILABLE', True)
    monkeypatch.setenv('KW_SORT_DEVICE', '1')
    with contextlib.redirect_stdout(io.StringIO()) as out:
        mk.sort_matched_csv(str(path))
    if pandas is None:
        assert out.getvalue().startswith('Error processing') and path.read_bytes() == data
    else:
        assert 'Error' not in out.getvalue(), out.getvalue()
        assert path.read_bytes() == pandas
    st = sortfiles.LAST_STATS
    assert st['device'] + st['unchanged'] == 2 * took and st['native'] + st['pandas'] == (not took and pandas is not None)
    host = tmp_path / 'Y_match.csv'
    host.write_bytes(data)
    monkeypatch.setenv('KW_SORT_DEVICE', '0')
    with contextlib.redirect_stdout(io.StringIO()):
        mk.sort_matched_csv(str(host))
    assert path.read_bytes() == host.read_bytes()


# ------------------------------------------------------------------ 2. the record spans
def _upload(dev, body):
    """The body in the handle's device text buffer (kw_ingest_stage + kw_ingest_upload) with 16 readable bytes of
    junk after it; it stands until the handle's next upload."""
    junk = b'",\n\r" ,\n"\0\xff,,"\n\r'
    view = dev.stage(0, len(body) + len(junk))
    view[:] = np.frombuffer(body + junk, dtype=np.uint8)
    return dev.upload(0, 0, len(body) + len(junk))


def _ingest_for(sorter, names):
    from advanced_scrapper_amd import ingest
    key = (len(names), tuple(names.index(c) for c in ingest.NEEDED))
    dev = sorter._ingests.get(key)
    if dev is None:
        dev = sorter._ingests[key] = ingest.DeviceIngest(0, key[0], key[1])
    return dev


def test_record_spans_equal_the_host_tokenizers(gpu, sorter, monkeypatch):
    from advanced_scrapper_amd import _native, ingest
    checked = 0
    for grid in (None, '1'):
        if grid:
            monkeypatch.setenv(INGEST_HOOK, grid)
        for name, data in S.SMALL_CASES:
            outcome = decided(name, data)[0]
            if outcome.startswith(('header-', 'ingest-')):
                continue
            names, _head, pos = ingest._split_header(data)
            body = data[pos:]
            dev = _ingest_for(sorter, names)
            t = _upload(dev, body)
            v, _bad, n_rows, consumed = dev.parse(t, len(body), True, body.count(b'\n') + 1)
            assert v == _native.KW_INGEST_OK and consumed == len(body), name
            start, end = dev.copy_spans()
            span = ingest.parse_all(data)[2] - pos
            assert n_rows == len(span), name
            assert np.array_equal(start, span[:, 0]) and np.array_equal(end, span[:, 1]), name
            checked += 1
    assert checked >= 60


# ------------------------------------------------------------------ 3. the gather's geometry
GEO_HEAD = b'time_unix,article_text,title,date_time,url,source_url,source\n'


def _geometry_body():
    """Records of 7 cells: 11-byte ones by the hundred, 18 consecutive ones of 1 100 and 1 107 bytes in turn (a wave's
    fast path at every source phase once their order is reversed), one past a wave's KiB, one past a block's 4 KiB, quoted cells with line breaks, and a
    last record without its line end; 8 tiles and more."""
    rows = []
    for i in range(700):
        rows.append(b'%d,t,t,d,,,s' % (i % 10) if i % 10 else b'7,t,t,d,u,v,s')
    assert all(len(r) == 11 for r in rows[1:10])
    # (reversed, two neighbours' phases differ by the sum of their lengths + 2: 1 100 + 1 107 + 2 = 1 mod 16)
    for k in range(18):
        rows.append(b'%d,%s,t,d,u,v,s' % (100 + k, b'a' * ((1107 if k % 2 else 1100) - 14)))
    rows.append(b'5,' + bytes(range(0x30, 0x7B)).replace(b'"', b'') * 20 + b',t,d,u,v,s')
    rows.append(b'3,"' + b'long, ""quoted""\nline\r\n' * 420 + b'",t,d,u,v,s')
    for i in range(300):
        rows.append(b'%d,t,t,d,,,s' % (i % 7))
    rows.append(b'4,"x\ny",t,d,u,v,s')
    rows.append(b'2,' + b'z' * 2000 + b',t,d,u,v,s')
    body = b'\n'.join(rows[:400]) + b'\r\n\n' + b'\n'.join(rows[400:])   # (no line end after the last record)
    return body, len(rows)


def _phases(spans, order):
    """(source - destination) mod 16 of every record longer than a wave's KiB + 32, laid out in `order`."""
    out, dst = set(), 0
    for r in order:
        a, b = spans[r]
        if b - a > 1024 + 32:
            out.add((a - dst) % 16)
        dst += b - a + 1
    return out


def test_gather_geometry(gpu, sorter, monkeypatch):
    from advanced_scrapper_amd import _native, ingest
    body, n = _geometry_body()
    T = _native.lib().kw_ingest_tile_bytes()
    assert T == 4096 and len(body) >= 8 * T
    names = GEO_HEAD.decode().strip().split(',')
    span = (ingest.parse_all(GEO_HEAD + body)[2] - len(GEO_HEAD)).tolist()
    assert len(span) == n
    lens = [b - a for a, b in span]
    assert lens.count(11) > 900 and lens.count(13) >= 70 and max(lens) > 4096 + 1024 and sum(1024 < x <= 4096 for x in lens) >= 16
    rng = np.random.default_rng(20251)
    orders = {'reverse': np.arange(n)[::-1].copy(), 'rotate': np.roll(np.arange(n), -1),
              'shuffle': rng.permutation(n), 'identity': np.arange(n), 'prefix': np.arange(n // 3),
              'repeats': rng.integers(0, n, n)}
    seen = set()
    for o in ('reverse', 'rotate', 'shuffle'):
        seen |= _phases(span, orders[o].tolist())
    assert seen == set(range(16)), sorted(seen)
    want = {k: b''.join(body[span[r][0]:span[r][1]] + b'\n' for r in o.tolist()) for k, o in orders.items()}
    assert any(len(w) % 16 for w in want.values()) and len(want['reverse']) % 16 != 0
    dev = _ingest_for(sorter, names)
    for sort_grid, ingest_grid in ((None, None), ('1', None), ('3', None), ('1', '1'), ('3', '3')):
        for hook, v in ((SORT_HOOK, sort_grid), (INGEST_HOOK, ingest_grid)):
            if v is None:
                monkeypatch.delenv(hook, raising=False)
            else:
                monkeypatch.setenv(hook, v)
        t = _upload(dev, body)
        v, _bad, n_rows, consumed = dev.parse(t, len(body), True, n + 8)
        assert (v, n_rows, consumed) == (_native.KW_INGEST_OK, n, len(body))
        sv, _r, _c, keys, body_bytes, asc = sorter.keys(dev, 0)
        assert sv == _native.KW_SORT_OK and not asc
        assert keys.tolist() == [int(body[a:body.index(b',', a)]) for a, _b in span]
        assert body_bytes == sum(lens) + n
        for k, o in orders.items():
            got = sorter.gather(o)
            assert got.tobytes() == want[k], (k, sort_grid, ingest_grid)


def test_block_rows(gpu, sorter):
    """DTYPE block by block, with a block of a few rows: the offender is the block's first row, lowest column."""
    from advanced_scrapper_amd import _native
    names = GEO_HEAD.decode().strip().split(',')
    dev = _ingest_for(sorter, names)
    rows = [b'%d,text,t,d,u,v,s' % i for i in range(10)]
    rows[7] = b'7,text,12,d,u,,s'
    rows[6] = b'6,text,13,d,u,,s'
    body = b'\n'.join(rows) + b'\n'
    t = _upload(dev, body)
    assert dev.parse(t, len(body), True, 20)[0] == _native.KW_INGEST_OK
    assert sorter.keys(dev, 0, 65536)[0] == _native.KW_SORT_OK
    assert sorter.keys(dev, 0, 3)[0] == _native.KW_SORT_OK           # blocks 0-2, 3-5, 6-8: row 8 is the witness
    assert sorter.keys(dev, 0, 2)[:3] == (_native.KW_SORT_DTYPE, 6, 2)   # block 6-7: title has no witness
    assert sorter.keys(dev, 0, 1)[:3] == (_native.KW_SORT_DTYPE, 6, 2)
    v = sorter.keys(dev, 0, 4)                                        # blocks 0-3, 4-7, 8-9
    assert v[0] == _native.KW_SORT_OK and v[5] is True and v[3].tolist() == list(range(10))


# ------------------------------------------------------------------ 4. the order's range check
def test_order_out_of_range_is_refused(gpu, sorter):
    from advanced_scrapper_amd import _native
    names = GEO_HEAD.decode().strip().split(',')
    dev = _ingest_for(sorter, names)
    rows = [b'%d,text %d,t,d,u,v,s' % (50 - i, i) for i in range(40)]
    body = b'\n'.join(rows) + b'\n'
    t = _upload(dev, body)
    assert dev.parse(t, len(body), True, 64)[:3] == (_native.KW_INGEST_OK, 0, 40)
    assert sorter.keys(dev, 0)[0] == _native.KW_SORT_OK
    good = np.arange(40)[::-1].copy()
    out = sorter.gather(good)
    want = b''.join(r + b'\n' for r in rows[::-1])
    assert out.tobytes() == want
    for bad in (40, -1, 1 << 40, -(1 << 62)):
        order = good.copy()
        order[17] = bad
        with pytest.raises(_native.KwError) as err:
            sorter.gather(order)
        assert err.value.code == _native.KW_EINVAL
        assert out.tobytes() == want, 'the output buffer was written'
    with pytest.raises(_native.KwError) as err:
        sorter.gather(np.arange(41))                      # more entries than rows
    assert err.value.code == _native.KW_EINVAL
    assert sorter.gather(good).tobytes() == want          # and the handle goes on


# ------------------------------------------------------------------ 5. a second run into the first run's directory
def _rerun(golden, root, device_flag, monkeypatch):
    from advanced_scrapper_amd import match_keywords as mk
    from advanced_scrapper_amd import sortfiles
    root.mkdir()
    golden.materialize_kb(str(root / 'kb'))
    frame = golden.articles_frame()
    rng = np.random.default_rng(11)
    frame['date_time'] = frame['date_time'].to_numpy()[rng.permutation(len(frame))]
    half = len(frame) // 2
    frame.iloc[:half].to_csv(root / 'a1.csv', index=False)
    frame.iloc[half:].to_csv(root / 'a2.csv', index=False)
    monkeypatch.chdir(root)
    monkeypatch.setenv('KW_SORT_DEVICE', device_flag)
    out = root / 'yahoo_ticker_matched_articles'
    pre = None
    for part in ('a1.csv', 'a2.csv'):
        if part == 'a2.csv':
            pre = {fn: (out / fn).read_bytes() for fn in os.listdir(out)}
        with contextlib.redirect_stdout(io.StringIO()) as log:
            rc = mk.main(['--info-dir', str(root / 'kb'), '--articles', str(root / part), '--chunksize',
                          str(golden.chunksize()), '--device', '0'])
        assert rc in (0, None) and 'Error' not in log.getvalue()
    return pre, {fn: (out / fn).read_bytes() for fn in os.listdir(out)}, dict(sortfiles.LAST_STATS)


def test_rerun_sorts_the_existing_files_on_the_device(gpu, golden, tmp_path, monkeypatch):
    t0 = time.perf_counter()
    pre_d, got_d, stats_d = _rerun(golden, tmp_path / 'dev', '1', monkeypatch)
    pre_h, got_h, stats_h = _rerun(golden, tmp_path / 'host', '0', monkeypatch)
    assert pre_d == pre_h and len(pre_d) > 3
    assert sorted(got_d) == sorted(got_h)
    for fn in got_h:
        assert got_d[fn] == got_h[fn], fn
    grew = [fn for fn in pre_d if got_d[fn] != pre_d[fn]]
    assert grew, 'the second half reached none of the first half\'s files'
    # every file the first run left goes through the device route, none through the host routes
    assert stats_d['device'] + stats_d['unchanged'] == len(pre_d), stats_d
    assert stats_d['native'] == stats_d['pandas'] == 0 and stats_d['refused'] == {}, stats_d
    assert stats_d['device'] >= 1 and stats_d['bytes'] > 0 and stats_d['ms']['gather'] > 0
    assert stats_h['device'] == stats_h['unchanged'] == 0 and stats_h['native'] + stats_h['pandas'] == len(pre_h)
    print(f'rerun: {len(pre_d)} files, {stats_d}, {time.perf_counter() - t0:.1f} s')
