"""GPU: the output sort of a file of any size (csrc/kwsort.hip: kw_sort_begin / kw_sort_window / kw_sort_finish,
kw_sort_gather_begin / kw_sort_gather_slab; sortfiles.DeviceSorter's windowed route) on the product's own staging
and kernels: the rule's table through windows smaller than a record and up; the gather's geometry across window
and slab edges against the plain permutation of the host tokenizer's spans; verdicts that are decided across
windows against kw_sort_keys on the same body as one text; store and output positions past 2^31 and 2^32; the
limits, and the rewrite's atomicity."""
import contextlib
import io
import os

import numpy as np
import pytest

from tests import sort_rule as S
from tests.test_gpu_sort import GEO_HEAD, _geometry_body, _ingest_for, _phases, _upload, decided

pytestmark = pytest.mark.gpu
SORT_HOOK, INGEST_HOOK = 'KW_TEST_SORT_GRID', 'KW_TEST_INGEST_GRID'
GEO_NAMES = GEO_HEAD.decode().strip().split(',')


@pytest.fixture(scope='module')
def gpu():
    from advanced_scrapper_amd import _native
    if _native.device_count() < 1:
        pytest.skip('no GPU')
    return _native


_SORTERS = {}


@pytest.fixture(scope='module')
def sorters(gpu):
    """DeviceSorter(0, large_from=0, window_bytes=W, slab_bytes=1024) by W, made on first use."""
    from advanced_scrapper_amd import sortfiles

    def get(window):
        if window not in _SORTERS:
            _SORTERS[window] = sortfiles.DeviceSorter(0, large_from=0, window_bytes=window, slab_bytes=1024)
        return _SORTERS[window]

    yield get
    for s in _SORTERS.values():
        s.close()
    _SORTERS.clear()


@pytest.fixture(scope='module')
def sorter(sorters):
    return sorters(4096)


def feed(sorter, dev, body, window, block_rows=S.BLOCK_ROWS, time_col=0):
    """``body`` through kw_sort_begin and one kw_sort_window a window, over the product's window reader and the
    ingest handle's two pinned slots; the rows every window gave."""
    from advanced_scrapper_amd import _native, sortfiles
    data = np.frombuffer(body, dtype=np.uint8)
    for slot in (0, 1):
        dev.stage(slot, sortfiles.HEADROOM + len(body))
    sorter.begin(time_col, len(body), block_rows)
    rows = []

    def fill(slot, at, lo, k):
        dev.stage(slot, at + k)[at:at + k] = data[lo:lo + k]

    def move(src, src_at, dst, dst_at, k):
        dev.stage(dst, dst_at + k)[dst_at:dst_at + k] = dev.stage(src, src_at + k)[src_at:src_at + k]

    def parse(slot, at, k, final, start):
        d_text = dev.upload(slot, at, k)
        v, _bad, n_rows, consumed = dev.parse(d_text, k, final, body.count(b'\n', start, start + k) + 1)
        assert v == _native.KW_INGEST_OK
        if n_rows:
            sorter.window(dev, consumed)
            rows.append(n_rows)
        return n_rows, consumed

    sortfiles.read_windows(len(body), window, fill, move, parse)
    return rows


# ------------------------------------------------------------------ 1. the rule's table, windowed
@pytest.mark.parametrize('window', (64, 256, 4096))
@pytest.mark.parametrize('name,data', S.CASES, ids=[n for n, _ in S.CASES])
def test_table_case_windowed(gpu, sorters, tmp_path, monkeypatch, name, data, window):
    """Every case of the table at every window.  The four ``block-*`` cases hold 65 546 rows of 36 bytes, one or
    two to a window of 64 bytes: about 45 000 parses a pass, 13 s a case on an MI355X (3 s at 256 bytes)."""
    from advanced_scrapper_amd import match_keywords as mk
    from advanced_scrapper_amd import sortfiles
    sorter = sorters(window)
    outcome, row, expected, pandas = decided(name, data)
    path = tmp_path / 'X_match.csv'
    path.write_bytes(data)
    old = 1_500_000_000_000_000_000
    os.utime(path, ns=(old, old))
    sortfiles.reset_stats()
    took = sorter.sort_file(str(path))
    last = sortfiles.LAST_STATS['last']
    assert took == (outcome == 'OK'), (name, outcome, last)
    assert os.listdir(tmp_path) == ['X_match.csv'], 'a temporary file was left'
    if took:
        assert expected == pandas
        assert path.read_bytes() == pandas
        assert last['verdict'] == 'OK'
        assert last['route'] == ('unchanged' if data == pandas else 'device')
    else:
        assert path.read_bytes() == data, 'a refused file was touched'
        assert os.stat(path).st_mtime_ns == old, 'a refused file was written'
        if outcome.startswith('sort-'):
            assert ('sort-' + last['verdict'], last['row']) == (outcome, row)
        elif outcome.startswith('ingest-'):
            assert last['verdict'].startswith('ingest-')
            assert list(sortfiles.LAST_STATS['refused']) == [last['verdict']]
        else:
            assert last['verdict'] == outcome
    if took and len(data) - data.index(b'\n') - 1 > window:
        assert sortfiles.LAST_STATS['windows'] >= 1, 'not the windowed route'
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
    assert os.listdir(tmp_path) == ['X_match.csv']


# ------------------------------------------------------------------ 2. the gather across window and slab edges
def _geometry():
    from advanced_scrapper_amd import ingest
    body, n = _geometry_body()
    span = (ingest.parse_all(GEO_HEAD + body)[2] - len(GEO_HEAD)).tolist()
    assert len(span) == n
    rng = np.random.default_rng(20252)
    tiny = [r for r, (a, b) in enumerate(span) if b - a == 11]
    orders = {'reverse': np.arange(n)[::-1].copy(), 'rotate': np.roll(np.arange(n), -1),
              'shuffle': rng.permutation(n), 'identity': np.arange(n), 'repeats': rng.integers(0, n, n),
              # 256 records of 11 bytes and their line ends: 3 072 bytes, whole slabs of 1 024 and of 3 072
              'tiny-repeats': np.asarray(tiny, dtype=np.int64)[rng.integers(0, len(tiny), 256)]}
    want = {k: b''.join(body[span[r][0]:span[r][1]] + b'\n' for r in o.tolist()) for k, o in orders.items()}
    return body, n, span, orders, want


def _edge_kinds(span, order, slab):
    """Where the slab edges of the body laid out in `order` fall: inside a record, on its '\\n', on its first byte."""
    kinds, starts, dst = set(), [], 0
    for r in order:
        starts.append(dst)
        dst += span[r][1] - span[r][0] + 1
    starts = np.asarray(starts + [dst])
    for e in range(slab, dst, slab):
        j = int(np.searchsorted(starts, e, side='right')) - 1
        kinds.add('first' if e == starts[j] else 'newline' if e == starts[j + 1] - 1 else 'inside')
    return kinds


def test_gather_geometry_across_windows_and_slabs(gpu, sorter, monkeypatch):
    from advanced_scrapper_amd import _native
    body, n, span, orders, want = _geometry()
    lens = [b - a for a, b in span]
    slabs = (1024, 3072, 16384)
    # the inputs themselves: the edges' places, the long records' phases, the totals
    kinds, seen = set(), set()
    for k, o in orders.items():
        for slab in slabs:
            kinds |= _edge_kinds(span, o.tolist(), slab)
        seen |= _phases(span, o.tolist())
    assert kinds == {'inside', 'newline', 'first'}, kinds
    assert seen == set(range(16)), sorted(seen)
    assert any(len(w) % s for w in want.values() for s in slabs)
    assert all(len(want['tiny-repeats']) % s == 0 for s in (1024, 3072)) and len(want['reverse']) % 1024
    dev = _ingest_for(sorter, GEO_NAMES)
    for sort_grid, ingest_grid in ((None, None), ('1', '1'), ('3', '3')):
        for hook, v in ((SORT_HOOK, sort_grid), (INGEST_HOOK, ingest_grid)):
            if v is None:
                monkeypatch.delenv(hook, raising=False)
            else:
                monkeypatch.setenv(hook, v)
        for window in (2048, 4096, 5000):
            rows = feed(sorter, dev, body, window)
            assert len(rows) > 4 and sum(rows) == n
            sv, _r, _c, keys, body_bytes, asc = sorter.finish()
            assert sv == _native.KW_SORT_OK and not asc
            assert keys.tolist() == [int(body[a:body.index(b',', a)]) for a, _b in span]
            assert body_bytes == sum(lens) + n
            for k, o in orders.items():
                for slab in slabs:
                    total, count = sorter.gather_begin(o, slab)
                    assert total == len(want[k]) and count == -(-total // slab)
                    ks = list(range(count))
                    if (k, slab) in (('shuffle', 1024), ('reverse', 3072), ('repeats', 16384)):
                        ks.reverse()
                    for j in ks:
                        got = sorter.gather_slab(j).tobytes()
                        assert got == want[k][j * slab:(j + 1) * slab], (k, slab, j, window, sort_grid)


# ------------------------------------------------------------------ 3. verdicts across windows
def _rows12(keys=None, title=None, url=None):
    """12 records of 20 bytes (their line end included), keys 100, 110, ...; `title` / `url`: row -> cell (2 bytes)."""
    keys = keys or [100 + 10 * i for i in range(12)]
    title, url = title or {}, url or {}
    rows = [b'%03d,txt,%s,d,%s,v,s\n' % (keys[i], title.get(i, b'tt'), url.get(i, b'uu')) for i in range(12)]
    assert all(len(r) == 20 for r in rows)
    return b''.join(rows)


def _both(sorter, dev, body, window, block_rows):
    """(the windows' result, kw_sort_keys' on the body as one text, the first row of every window)."""
    from advanced_scrapper_amd import _native
    rows = feed(sorter, dev, body, window, block_rows)
    a = sorter.finish()
    a = a[:3] + (None if a[3] is None else a[3].tolist(),) + a[4:]
    t = _upload(dev, body)
    assert dev.parse(t, len(body), True, body.count(b'\n') + 1)[0] == _native.KW_INGEST_OK
    b = sorter.keys(dev, 0, block_rows)
    b = b[:3] + (None if b[3] is None else b[3].tolist(),) + b[4:]
    return a, b, np.cumsum([0] + rows).tolist()


def _window_of(firsts, row):
    return int(np.searchsorted(firsts, row, side='right')) - 1


@pytest.mark.parametrize('block_rows', (3, 4))
@pytest.mark.parametrize('window', (50, 70))
def test_verdicts_across_windows(gpu, sorter, block_rows, window):
    n = gpu
    dev = _ingest_for(sorter, GEO_NAMES)
    B = block_rows
    # strictly ascending; the windows cut inside a block
    a, b, firsts = _both(sorter, dev, _rows12(), window, B)
    assert a == b and a[0] == n.KW_SORT_OK and a[5] is True and a[4] == 240
    assert len(firsts) > 4 and any(f % B for f in firsts[1:-1]), firsts
    blk = next(k for k in range(1, 12 // B) if _window_of(firsts, k * B) != _window_of(firsts, k * B + B - 1))
    lo, hi = blk * B, blk * B + B - 1          # a block that spans two windows, its first and last row
    # its only text witnesses lie in another window than its numeric cells
    apart = {r: b'12' for r in range(lo, hi + 1) if _window_of(firsts, r) != _window_of(firsts, hi)}
    assert apart and len(apart) < B
    a, b, f2 = _both(sorter, dev, _rows12(title=apart), window, B)
    assert f2 == firsts and a == b and a[0] == n.KW_SORT_OK
    # no witness at all: DTYPE at the block's first global row, its lowest column
    numeric = {r: b'12' for r in range(lo, hi + 1)}
    a, b, _f = _both(sorter, dev, _rows12(title=numeric, url=numeric), window, B)
    assert a == b and a[:3] == (n.KW_SORT_DTYPE, lo, 2)
    # a KEY offender in the last window beats a DTYPE offender in the first
    body = _rows12(title={r: b'12' for r in range(B)})[:-20] + b'+10,txt,tt,d,uu,v,s\n'
    a, b, _f = _both(sorter, dev, body, window, B)
    assert a == b and a[:3] == (n.KW_SORT_KEY, 11, 0)
    assert _both(sorter, dev, _rows12(title={r: b'12' for r in range(B)}), window, B)[0][:3] == (n.KW_SORT_DTYPE, 0, 2)
    # a FORM offender's global row and column (a needlessly quoted cell of a later window)
    bad = firsts[2] + 1
    body = _rows12()
    body = body[:20 * bad] + b'%03d,tx,tt,d,"u",v,s\n' % (100 + 10 * bad) + body[20 * bad + 20:]
    assert len(body) == 240
    a, b, _f = _both(sorter, dev, body, window, B)
    assert a == b and a[:3] == (n.KW_SORT_FORM, bad, 4)
    # keys that descend, and keys that are equal, only across a window's edge
    for edge in firsts[1:-1]:
        for delta in (-5, 0):
            keys = [100 + 10 * i for i in range(12)]
            keys[edge] = keys[edge - 1] + delta
            a, b, f3 = _both(sorter, dev, _rows12(keys), window, B)
            assert f3 == firsts and a == b and a[0] == n.KW_SORT_OK and a[5] is False, (edge, delta)
            assert a[3] == keys


# ------------------------------------------------------------------ 4. positions past 2^31 and 2^32
def test_store_and_output_past_4_gib(gpu):
    from advanced_scrapper_amd import ingest, sortfiles
    R, W, COPIES = 32768, 2048, 70
    i = np.arange(R, dtype=np.int64)[:, None]
    j = np.arange(W, dtype=np.int64)[None, :]
    # (letters; every record's text differs from its neighbours', and the key in it from every other record's)
    rows = (((i * 31 + (i >> 5)) % 26).astype(np.uint8) + ((j * 7) % 26).astype(np.uint8)) % 26 + 0x61
    keys = np.char.zfill((1000000000 + i[:, 0]).astype('U10'), 10)
    rows[:, :10] = np.frombuffer(''.join(keys.tolist()).encode(), dtype=np.uint8).reshape(R, 10)
    rows[:, 10] = 0x2C
    keep = j < W - (i % 7) - 11                                             # records of 2 042 .. 2 048 bytes
    tail = np.frombuffer(b',t,d,u,v,s\n', dtype=np.uint8)
    lens = (W - (i[:, 0] % 7)).astype(np.int64)                             # (the line end included)
    flat = np.concatenate([np.where(keep, rows, 0), np.broadcast_to(tail, (R, 11))], axis=1)
    mask = np.concatenate([keep, np.ones((R, 11), dtype=bool)], axis=1)
    win = flat[mask]
    off = np.concatenate([[0], np.cumsum(lens)])
    Wn = int(off[R])
    assert len(win) == Wn and 60 << 20 < Wn <= 64 << 20 and COPIES * Wn > (1 << 32) + (64 << 20)
    winb = win.tobytes()
    assert winb[off[5]:off[6]].endswith(b',t,d,u,v,s\n') and winb[off[5]:off[5] + 11] == b'1000000005,'
    sorter = sortfiles.DeviceSorter(0)
    try:
        dev = _ingest_for(sorter, GEO_NAMES)
        try:
            sorter.begin(0, COPIES * Wn)
        except sortfiles.Refusal as r:
            pytest.skip(f'kw_sort_begin: a store of {COPIES * Wn} bytes does not fit on this device ({r.reason})')
        dev.stage(0, Wn)[:] = win
        for _c in range(COPIES):
            d_text = dev.upload(0, 0, Wn)
            v, _bad, n_rows, consumed = dev.parse(d_text, Wn, False, R + 1)
            assert (v, n_rows, consumed) == (0, R, Wn)
            sorter.window(dev, consumed)
        sv, _r, _c, got_keys, body_bytes, asc = sorter.finish()
        N = COPIES * R
        assert sv == 0 and len(got_keys) == N and body_bytes == COPIES * Wn and not asc
        assert got_keys[:R].tolist() == (1000000000 + i[:, 0]).tolist() and (got_keys[-R:] == got_keys[:R]).all()
        # the full reversed order: the reversed window, COPIES times
        rev = b''.join(winb[off[r]:off[r + 1]] for r in range(R - 1, -1, -1))
        slab = 16 << 20
        total, count = sorter.gather_begin(np.arange(N, dtype=np.int64)[::-1].copy(), slab)
        assert total == COPIES * Wn and count == -(-total // slab)

        def expect(lo, hi):
            out, p = [], lo
            while p < hi:
                q = p % Wn
                k = min(hi - p, Wn - q)
                out.append(rev[q:q + k])
                p += k
            return b''.join(out)

        for k in (0, count - 1, (1 << 31) // slab, (1 << 32) // slab, (1 << 31) // slab - 1, (1 << 32) // slab - 1):
            lo, hi = k * slab, min((k + 1) * slab, total)
            got = sorter.gather_slab(k)
            assert len(got) == hi - lo
            assert got.tobytes() == expect(lo, hi), k
        # sources just below and above store positions 2^31 and 2^32
        order = []
        for edge in (1 << 31, 1 << 32):
            c, q = divmod(edge, Wn)
            g = c * R + int(np.searchsorted(off, q, side='right')) - 1      # the record that holds the position
            assert c * Wn + off[g % R] <= edge < c * Wn + off[g % R + 1]
            order += list(range(g - 250, g + 250))
        rng = np.random.default_rng(5)
        order = np.asarray(order, dtype=np.int64)[rng.permutation(1000)]
        want = b''.join(winb[off[g % R]:off[g % R + 1]] for g in order.tolist())
        total, count = sorter.gather_begin(order, 1 << 20)
        assert total == len(want) and count == 2
        assert b''.join(sorter.gather_slab(k).tobytes() for k in range(count)) == want
    finally:
        sorter.close()
    assert ingest.MAX_WINDOW < (1 << 31)


# ------------------------------------------------------------------ 5. limits and atomicity
def _file(rows):
    return S._file([S._row(k, i) for i, k in enumerate(rows)])


def test_store_cap_refuses_with_memory(gpu, sorters, tmp_path, monkeypatch):
    from advanced_scrapper_amd import match_keywords as mk
    from advanced_scrapper_amd import sortfiles
    sorter = sorters(256)
    data = _file([(37 * i) % 101 for i in range(60)])
    pandas = S.pandas_bytes(data)
    path = tmp_path / 'X_match.csv'
    path.write_bytes(data)
    old = 1_500_000_000_000_000_000
    os.utime(path, ns=(old, old))
    monkeypatch.setenv('KW_TEST_HOOKS', '1')
    monkeypatch.setenv('KW_TEST_SORT_STORE_MAX', str(len(data) // 2))
    sortfiles.reset_stats()
    assert sorter.sort_file(str(path)) is False
    assert sortfiles.LAST_STATS['refused'] == {'memory': 1} and sortfiles.LAST_STATS['last'] == {'verdict': 'memory'}
    assert path.read_bytes() == data and os.stat(path).st_mtime_ns == old
    monkeypatch.setattr(sortfiles, '_SORTER', sorter)
    monkeypatch.setattr(sortfiles, '_AVAILABLE', True)
    monkeypatch.setenv('KW_SORT_DEVICE', '1')
    with contextlib.redirect_stdout(io.StringIO()):
        mk.sort_matched_csv(str(path))
    assert path.read_bytes() == pandas
    st = sortfiles.LAST_STATS
    assert st['native'] + st['pandas'] == 1 and st['device'] == 0 and st['refused'] == {'memory': 2}
    assert os.listdir(tmp_path) == ['X_match.csv']
    # and with the cap above the body the same file goes through the windows
    monkeypatch.setenv('KW_TEST_SORT_STORE_MAX', str(len(data)))
    path.write_bytes(data)
    sortfiles.reset_stats()
    assert sorter.sort_file(str(path)) is True and path.read_bytes() == pandas
    assert sortfiles.LAST_STATS['windows'] > 10 and sortfiles.LAST_STATS['slabs'] == -(-(len(pandas) - len(S.HEAD)) // 1024)
    assert os.listdir(tmp_path) == ['X_match.csv']


def test_bad_order_leaves_no_slab(gpu, sorter):
    n = gpu
    dev = _ingest_for(sorter, GEO_NAMES)
    rows = [b'%d,text %d,t,d,u,v,s' % (50 - i, i) for i in range(40)]
    body = b'\n'.join(rows) + b'\n'
    feed(sorter, dev, body, 100)
    assert sorter.finish()[0] == n.KW_SORT_OK
    good = np.arange(40)[::-1].copy()
    want = b''.join(r + b'\n' for r in rows[::-1])
    total, count = sorter.gather_begin(good, 1024)
    assert total == len(want) and sorter.gather_slab(0).tobytes() == want[:1024]
    for bad in (40, -1, 1 << 40, -(1 << 62)):
        order = good.copy()
        order[17] = bad
        with pytest.raises(n.KwError) as err:
            sorter.gather_begin(order, 1024)
        assert err.value.code == n.KW_EINVAL
        with pytest.raises(n.KwError) as err:
            sorter.gather_slab(0)
        assert err.value.code == n.KW_ESTATE
    for slab in (0, 1000, 1025):
        with pytest.raises(n.KwError) as err:
            sorter.gather_begin(good, slab)
        assert err.value.code == n.KW_EINVAL
    total, count = sorter.gather_begin(good, 1024)                # and the handle goes on
    assert b''.join(sorter.gather_slab(k).tobytes() for k in range(count)) == want
    assert sorter.gather(good).tobytes() == want                  # (the whole body at once, from the store)


@pytest.mark.parametrize('last_row', (S._row('+1', 99), b'3,too,few,fields\n'), ids=('sort-KEY', 'ingest-FIELDS'))
def test_refusal_in_the_last_window_leaves_the_file(gpu, sorters, tmp_path, last_row):
    from advanced_scrapper_amd import sortfiles
    sorter = sorters(256)
    data = _file([90 - i for i in range(60)]) + last_row
    path = tmp_path / 'X_match.csv'
    path.write_bytes(data)
    old = 1_500_000_000_000_000_000
    os.utime(path, ns=(old, old))
    sortfiles.reset_stats()
    assert sorter.sort_file(str(path)) is False
    reason, = sortfiles.LAST_STATS['refused']
    assert reason == ('sort-KEY' if last_row.startswith(b'+1') else 'ingest-FIELDS')
    if reason == 'sort-KEY':
        assert sortfiles.LAST_STATS['last'] == {'verdict': 'KEY', 'row': 60, 'col': 0}
    assert path.read_bytes() == data and os.stat(path).st_mtime_ns == old
    assert os.listdir(tmp_path) == ['X_match.csv']
