"""GPU: a run's own files finished on the device from the write index (csrc/kwsort.hip: kw_sort_index_begin /
kw_sort_index_window / kw_sort_index_finish in front of the gather calls; sortfiles.DeviceSorter.sort_indexed;
egress.RunFiles.finish): the spans, the terminator check and the gather at the C-ABI against bytes built in numpy;
the verdicts and errors; finish on the device against its host branch and against pandas; the windowed write path;
main() on corpora whose dates do not follow the articles."""
import contextlib
import io
import os
import stat

import numpy as np
import pytest

from tests.test_finish_route import build, expected, shuffled

pytestmark = pytest.mark.gpu
LENGTHS = (2, 15, 16, 17, 33, 1023, 1024, 1025, 3000, 17000)      # a record's bytes, its terminator included
ROWS = (1, 2, 255, 256, 257, 65539)                                # 65 539: 257 tiles, ks_scan_kernel's second trip
ORDERS = ('identity', 'reverse', 'shuffle', 'prefix')
NAME = 'T_match.csv'


@pytest.fixture(scope='module')
def gpu():
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


@pytest.fixture(scope='module')
def small(gpu):
    """The sorter of the windowed write path: every body in windows of 4096 bytes, out in slabs of 1024."""
    from advanced_scrapper_amd import sortfiles
    s = sortfiles.DeviceSorter(0, large_from=0, window_bytes=4096, slab_bytes=1024)
    yield s
    s.close()


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv('KW_TEST_HOOKS', '1')
    monkeypatch.delenv('KW_TEST_SORT_GRID', raising=False)
    monkeypatch.delenv('KW_TEST_SORT_STORE_MAX', raising=False)
    return monkeypatch


# ------------------------------------------------------------------ 1. spans, check and gather at the C-ABI
_BODIES = {}


def _body(n):
    """(body uint8, lens, starts) of n records: letters, a line end inside some (a quoted one is legal: only a
    record's last byte is its terminator).  The large case draws the short lengths far more often, so that its
    body stays near 2 MB; every length occurs where n allows."""
    if n not in _BODIES:
        rng = np.random.default_rng(1000 + n)
        p = None if n < 1000 else np.asarray([0.2] * 5 + [0.0002] * 5) / (5 * 0.2 + 5 * 0.0002)
        lens = rng.choice(LENGTHS, size=n, p=p).astype(np.int64)
        if n >= len(LENGTHS):
            lens[rng.permutation(n)[:len(LENGTHS)]] = LENGTHS
        ends = np.cumsum(lens)
        body = rng.integers(0x61, 0x7B, int(ends[-1]), dtype=np.uint8)
        body[rng.integers(0, len(body), len(body) // 50)] = 0x0A
        body[ends - 1] = 0x0A
        _BODIES[n] = (body, lens, ends - lens)
    return _BODIES[n]


def _order(kind, n):
    rng = np.random.default_rng(77 + n)
    if kind == 'identity':
        return np.arange(n, dtype=np.int64)
    if kind == 'reverse':
        return np.arange(n, dtype=np.int64)[::-1].copy()
    if kind == 'shuffle':
        return rng.permutation(n).astype(np.int64)
    return rng.permutation(n).astype(np.int64)[:max(1, n // 2)]          # a prefix of a permutation: fewer than n_rows


def _expect(body, lens, starts, order):
    return np.concatenate([body[starts[r]:starts[r] + lens[r]] for r in order.tolist()]).tobytes()


def _push(sorter, body, lens, window=None):
    """The body through begin, one kw_sort_index_window a window (the two slots in turn) and finish."""
    sorter.index_begin(lens, len(body))
    window = window or len(body)
    slot = 0
    for lo in range(0, len(body), window):
        k = min(window, len(body) - lo)
        sorter.index_stage(slot, k)[:] = body[lo:lo + k]
        sorter.index_window(slot, k)
        slot = 1 - slot
    return sorter.index_finish()


@pytest.mark.parametrize('kind', ORDERS)
@pytest.mark.parametrize('n', ROWS)
def test_spans_check_and_gather(gpu, sorter, hooks, n, kind):
    body, lens, starts = _body(n)
    if n >= len(LENGTHS):
        assert set(lens.tolist()) == set(LENGTHS)
    assert (body[starts + lens - 1] == 0x0A).all()
    if n >= 255:
        assert np.count_nonzero(body == 0x0A) > n, 'no line end inside a record'
    order = _order(kind, n)
    want = _expect(body, lens, starts, order)
    for grid in (None, '1', '3'):
        if grid is None:
            hooks.delenv('KW_TEST_SORT_GRID', raising=False)
        else:
            hooks.setenv('KW_TEST_SORT_GRID', grid)
        for window in (None, 1000, 4097):
            assert _push(sorter, body, lens, window) == (gpu.KW_INDEX_OK, -1), (grid, window)
            assert sorter.gather(order).tobytes() == want, (grid, window, 'gather')
            for slab in (1024, 65536):
                total, count = sorter.gather_begin(order, slab)
                assert total == len(want) and count == -(-total // slab)
                got = b''.join(sorter.gather_slab(k).tobytes() for k in range(count))
                assert got == want, (grid, window, slab)
    ms = sorter.last_ms()
    assert ms['keys'] > 0 and ms['copies'] > 0 and ms['gather'] > 0


# ------------------------------------------------------------------ 2. verdicts and errors
def _begin_raw(gpu, sorter, lens, body_bytes):
    import ctypes
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    bad = ctypes.c_int64(-7)
    rc = gpu.lib().kw_sort_index_begin(sorter.h, gpu.ptr(lens), len(lens), int(body_bytes), ctypes.byref(bad))
    return rc, int(bad.value), gpu.lib().kw_sort_last_error(sorter.h).decode()


def test_verdicts_and_errors(gpu, sorter, hooks):
    from advanced_scrapper_amd import sortfiles
    body, lens, starts = _body(257)
    order = _order('reverse', 257)
    want = _expect(body, lens, starts, order)
    for grid in (None, '1'):
        if grid:
            hooks.setenv('KW_TEST_SORT_GRID', grid)
        # two records without their terminator: TERM names the lower one, and nothing can be gathered
        hurt = body.copy()
        for r in (201, 70):
            hurt[starts[r] + lens[r] - 1] = 0x61
        assert _push(sorter, hurt, lens, 4097) == (gpu.KW_INDEX_TERM, 70)
        for call in (lambda: sorter.gather(order), lambda: sorter.gather_begin(order, 1024)):
            with pytest.raises(gpu.KwError) as err:
                call()
            assert err.value.code == gpu.KW_ESTATE
        # a length of 0; a sum off by one, either way
        bad = lens.copy()
        bad[133] = 0
        rc, row, msg = _begin_raw(gpu, sorter, bad, len(body))
        assert (rc, row) == (gpu.KW_EINVAL, 133) and 'row 133' in msg
        bad[[5, 133]] = -3, 0
        assert _begin_raw(gpu, sorter, bad, len(body))[:2] == (gpu.KW_EINVAL, 5)
        rc, row, msg = _begin_raw(gpu, sorter, lens, len(body) + 1)          # the lengths end one byte short
        assert (rc, row) == (gpu.KW_EINVAL, 257) and 'row 257' in msg
        rc, row, msg = _begin_raw(gpu, sorter, lens, len(body) - 1)          # the last record ends beyond the body
        assert (rc, row) == (gpu.KW_EINVAL, 256) and 'row 256' in msg
        long_ = lens.copy()
        long_[100] += 1
        rc, row, msg = _begin_raw(gpu, sorter, long_, len(body))
        assert rc == gpu.KW_EINVAL and row == 256
        with pytest.raises(gpu.KwError) as err:                             # (a refused begin opens nothing)
            sorter.index_window(0, 1)
        assert err.value.code == gpu.KW_ESTATE
        # fewer bytes than the body, and more
        sorter.index_begin(lens, len(body))
        sorter.index_stage(0, len(body))[:] = body
        sorter.index_window(0, len(body) - 1)
        with pytest.raises(gpu.KwError) as err:
            sorter.index_finish()
        assert err.value.code == gpu.KW_ESTATE
        sorter.index_begin(lens, len(body))
        sorter.index_window(0, len(body) - 1)
        sorter.index_stage(1, 2)[:] = body[-2:]
        with pytest.raises(gpu.KwError) as err:
            sorter.index_window(1, 2)
        assert err.value.code == gpu.KW_EOVERFLOW
        with pytest.raises(gpu.KwError) as err:
            sorter.index_finish()
        assert err.value.code == gpu.KW_ESTATE
        # a store cap below the body: the 'memory' refusal
        hooks.setenv('KW_TEST_SORT_STORE_MAX', str(len(body) - 1))
        with pytest.raises(sortfiles.Refusal) as ref:
            sorter.index_begin(lens, len(body))
        assert ref.value.reason == 'memory'
        hooks.delenv('KW_TEST_SORT_STORE_MAX')
        # and the handle goes on with a correct file
        assert _push(sorter, body, lens, 1000) == (gpu.KW_INDEX_OK, -1)
        assert sorter.gather(order).tobytes() == want


# ------------------------------------------------------------------ 3. RunFiles.finish: the device against the host branch
def _stamps(layout, n):
    if layout == 'descending':
        return (1_700_000_000 - 60 * np.arange(n)).astype(np.int64)
    if layout == 'shuffle':
        perm = np.random.default_rng(4).permutation(n)
        if (np.diff(perm) > 0).all():
            perm = np.roll(perm, 1)                                      # (a small draw came out in order)
        return (1_600_000_000 + perm * 60).astype(np.int64)
    return shuffled(n, seed=3)                                           # 'ties': every fifth row shares one stamp


def _finish_both(tmp_path, monkeypatch, stamps, use):
    """finish() of the same hand-built file on the device route (sorter ``use``) and with KW_FINISH_DEVICE=0:
    (the device's bytes, the host's, the device run's stats, the host run's, the file as written)."""
    from advanced_scrapper_amd import sortfiles
    monkeypatch.setattr(sortfiles, '_SORTER', use)
    monkeypatch.setattr(sortfiles, '_AVAILABLE', True)
    got = []
    for flag in ('1', '0'):
        root = tmp_path / ('dev' if flag == '1' else 'host')
        root.mkdir()
        monkeypatch.setenv('KW_FINISH_DEVICE', flag)
        run, header, lines = build(root, stamps, NAME)
        os.chmod(root / NAME, 0o640)
        sortfiles.reset_stats()
        assert run.finish(NAME) is True
        assert os.listdir(root) == [NAME], 'a temporary file was left'
        assert stat.S_IMODE(os.stat(root / NAME).st_mode) == 0o640
        got.append(((root / NAME).read_bytes(), dict(sortfiles.LAST_STATS)))
    assert got[1][0] == expected(header, lines, stamps)
    return got[0][0], got[1][0], got[0][1], got[1][1], header + b''.join(lines)


@pytest.mark.parametrize('n', (3, 257, 65539))
@pytest.mark.parametrize('layout', ('descending', 'shuffle', 'ties'))
def test_finish_device_equals_host(gpu, sorter, tmp_path, monkeypatch, layout, n):
    stamps = _stamps(layout, n)
    if layout == 'ties' and n > 5:
        assert np.count_nonzero(stamps == stamps[0]) == -(-n // 5)
    dev, host, st_d, st_h, raw = _finish_both(tmp_path, monkeypatch, stamps, sorter)
    assert dev == host
    assert (st_d['indexed'], st_d['index_host'], st_d['refused']) == (1, 0, {})
    assert st_d['bytes'] == len(dev) - dev.index(b'\n') - 1 == st_d['gather_bytes'] and st_d['windows'] == 1
    assert (st_h['indexed'], st_h['index_host'], st_h['bytes']) == (0, 1, 0)
    if (layout, n) == ('descending', 257):
        import pandas as pd
        frame = pd.read_csv(io.BytesIO(raw))
        assert raw != dev and frame.sort_values('time_unix').to_csv(index=False).encode('utf-8') == dev


def test_finish_in_order_makes_no_device_call(gpu, sorter, tmp_path, monkeypatch):
    from advanced_scrapper_amd import egress, sortfiles
    monkeypatch.setattr(sortfiles, '_SORTER', sorter)
    monkeypatch.setattr(sortfiles, '_AVAILABLE', True)
    monkeypatch.setenv('KW_FINISH_DEVICE', '1')
    run, header, lines = build(tmp_path, 1_600_000_000 + 60 * np.arange(257), NAME)
    path = tmp_path / NAME
    old = 1_500_000_000_000_000_000
    os.utime(path, ns=(old, old))
    ino = os.stat(path).st_ino
    sortfiles.reset_stats()
    monkeypatch.setattr(sorter, 'sort_indexed', lambda *a, **k: pytest.fail('a device call'))
    monkeypatch.setattr(egress, 'open', lambda *a, **k: pytest.fail('the file was opened'), raising=False)
    assert run.finish(NAME) is True
    assert (os.stat(path).st_mtime_ns, os.stat(path).st_ino) == (old, ino)
    st = sortfiles.LAST_STATS
    assert (st['indexed'], st['index_host'], st['bytes'], st['windows']) == (0, 0, 0, 0)


# ------------------------------------------------------------------ 4. the windowed write path
@pytest.mark.parametrize('n', (3, 257, 65539))
def test_windowed_write_path(gpu, small, tmp_path, monkeypatch, n):
    stamps = _stamps('ties', n)
    dev, host, st_d, st_h, _raw = _finish_both(tmp_path, monkeypatch, stamps, small)
    assert dev == host
    nbody = len(dev) - dev.index(b'\n') - 1
    assert st_d['indexed'] == 1 and st_d['index_host'] == 0
    assert st_d['windows'] == -(-nbody // 4096) and st_d['slabs'] == -(-nbody // 1024)


def test_damaged_terminator_falls_to_the_host_branch(gpu, small, tmp_path, monkeypatch):
    from advanced_scrapper_amd import sortfiles
    monkeypatch.setattr(sortfiles, '_SORTER', small)
    monkeypatch.setattr(sortfiles, '_AVAILABLE', True)
    monkeypatch.setenv('KW_FINISH_DEVICE', '1')
    stamps = _stamps('shuffle', 257)
    run, header, lines = build(tmp_path, stamps, NAME)
    lines[140] = lines[140][:-1] + b'!'                                  # (after the index was built; the size stands)
    (tmp_path / NAME).write_bytes(header + b''.join(lines))
    sortfiles.reset_stats()
    assert run.finish(NAME) is True
    assert (tmp_path / NAME).read_bytes() == expected(header, lines, stamps)
    st = sortfiles.LAST_STATS
    assert st['refused'] == {'index-TERM': 1} and (st['indexed'], st['index_host']) == (0, 1)
    assert os.listdir(tmp_path) == [NAME]
    # the refusal itself leaves the bytes and the modification time alone
    (tmp_path / NAME).write_bytes(header + b''.join(lines))
    old = 1_500_000_000_000_000_000
    os.utime(tmp_path / NAME, ns=(old, old))
    lens = np.asarray([len(x) for x in lines], dtype=np.int64)
    assert small.sort_indexed(str(tmp_path / NAME), len(header), lens, np.argsort(stamps, kind='quicksort')) is False
    assert (tmp_path / NAME).read_bytes() == header + b''.join(lines) and os.stat(tmp_path / NAME).st_mtime_ns == old


def test_memory_refusal_leaves_the_file(gpu, small, tmp_path, hooks):
    from advanced_scrapper_amd import sortfiles
    hooks.setattr(sortfiles, '_SORTER', small)
    hooks.setattr(sortfiles, '_AVAILABLE', True)
    hooks.setenv('KW_FINISH_DEVICE', '1')
    stamps = _stamps('descending', 257)
    run, header, lines = build(tmp_path, stamps, NAME)
    hooks.setenv('KW_TEST_SORT_STORE_MAX', '100')
    sortfiles.reset_stats()
    assert run.finish(NAME) is True
    assert (tmp_path / NAME).read_bytes() == expected(header, lines, stamps)
    st = sortfiles.LAST_STATS
    assert st['refused'] == {'memory': 1} and (st['indexed'], st['index_host']) == (0, 1)


# ------------------------------------------------------------------ 5. main() on a corpus out of order
_CORPUS = {}


def _articles(golden):
    """2000 synthetic articles whose dates are a permutation of the documents' (multiplier coprime with the span),
    and the same articles newest first."""
    if not _CORPUS:
        import math
        from advanced_scrapper_amd import synth
        from advanced_scrapper_amd.kb import compile_kb
        names, kinds = synth.injectable_names(compile_kb(golden.kb_processed()))
        corpus = synth.generate(2000, names, kinds, seed=20251021, doc_base=0)
        assert math.gcd(1237, 2000) == 1
        perm = synth.to_dataframe(corpus, span_docs=2000, date_perm=(1237, 77))
        asc = synth.to_dataframe(corpus, span_docs=2000)
        _CORPUS['perm'] = perm.to_csv(index=False).encode('utf-8')
        _CORPUS['newest-first'] = asc.iloc[::-1].to_csv(index=False).encode('utf-8')
    return _CORPUS


def _main(golden, root, src, flag, monkeypatch):
    from advanced_scrapper_amd import match_keywords as mk
    from advanced_scrapper_amd import sortfiles
    root.mkdir()
    golden.materialize_kb(str(root / 'kb'))
    (root / 'articles.csv').write_bytes(src)
    monkeypatch.chdir(root)
    monkeypatch.setenv('KW_FINISH_DEVICE', flag)
    with contextlib.redirect_stdout(io.StringIO()) as log:
        rc = mk.main(['--info-dir', str(root / 'kb'), '--articles', str(root / 'articles.csv'), '--chunksize', '500',
                      '--device', '0'])
    assert rc in (0, None) and 'Error' not in log.getvalue()
    out = root / 'yahoo_ticker_matched_articles'
    return {fn: (out / fn).read_bytes() for fn in os.listdir(out)}, dict(sortfiles.LAST_STATS)


@pytest.mark.parametrize('corpus', ('perm', 'newest-first'))
def test_main_on_a_corpus_out_of_order(gpu, golden, tmp_path, monkeypatch, corpus):
    src = _articles(golden)[corpus]
    dev, st_d = _main(golden, tmp_path / 'dev', src, '1', monkeypatch)
    host, st_h = _main(golden, tmp_path / 'host', src, '0', monkeypatch)
    assert len(dev) > 3 and sorted(dev) == sorted(host)
    for fn in host:
        assert dev[fn] == host[fn], fn
    assert st_d['indexed'] >= 1 and st_d['index_host'] == 0 and st_d['refused'] == {}, st_d
    assert st_h['indexed'] == 0 and st_h['index_host'] == st_d['indexed'], st_h
    import pandas as pd
    for fn, data in dev.items():
        assert pd.read_csv(io.BytesIO(data))['time_unix'].is_monotonic_increasing, fn
