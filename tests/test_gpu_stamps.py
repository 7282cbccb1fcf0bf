"""GPU: the stamps kernel (csrc/kwingest.hip, ig_stamps_kernel after kw_ingest_zone) against the rule of
tests/stamps_rule.py and kwcsv_stamps_local, value for value, over the lane, wave and trip boundaries and the table
sizes up to the LDS limit; kw_rows_emit_stamps_device against kw_rows_emit; the new calls' argument and state errors."""
import ctypes
import random
import time

import numpy as np
import pytest

from tests import dates_rule as DR
from tests import emit_rule as ER
from tests import ingest_rule as IR
from tests import stamps_rule as R
from tests.test_gpu_ingest import COLS7, _parse, torch_gpu   # noqa: F401

pytestmark = pytest.mark.gpu
HOOK = 'KW_TEST_INGEST_GRID'
BLOCK = 256
GRID = 2
ROWS = (0, 1, 63, 64, 65, 257, GRID * BLOCK + 1)      # lanes, waves, blocks, and a second trip under HOOK = GRID
SPECIALS = ['', 'NA', 'June 5 2023', '2023-06-05T14:23:11Z', '2023-06-05 14:23:11.5+05:30', '1969-12-31T23:59:59.5Z',
            '2023-13-05 14:23:11', '2262-04-11T23:47:16.854775-00:01', '9999-12-31T23:59:59.999999Z']


def _est_table():
    """The 261 entries of EST5EDT 1970-2100, built by kwcsv_zone_table under that zone (the zone put back after)."""
    import os
    from advanced_scrapper_amd import zone as Z
    old = os.environ.get('TZ')
    os.environ['TZ'] = 'EST5EDT,M3.2.0,M11.1.0'
    time.tzset()
    try:
        at, off = Z.build()
    finally:
        if old is None:
            del os.environ['TZ']
        else:
            os.environ['TZ'] = old
        time.tzset()
    return [int(x) for x in at], [int(x) for x in off]


def _tables():
    full = [i * 4000000 for i in range(R.CAPACITY)] + [R.SPAN[1]]
    return {
        'utc': R.UTC_TABLE,
        'ist': ([R.SPAN[0], R.SPAN[1]], [19800]),
        'two': ([R.SPAN[0], 1000000000, R.SPAN[1]], [3600, 7200]),
        'est': _est_table(),
        'full': (full, [(-18000, -14400, -16200, -12600)[i & 3] for i in range(R.CAPACITY)]),    # 60- and 30-minute steps
    }


TABLE_NAMES = ('est', 'full', 'ist', 'two', 'utc')


@pytest.fixture(scope='module')
def tables():
    """The tables of the cases, built once when the first GPU test needs them (not at collection: building the
    EST5EDT one switches the process's zone for a moment and loads libkwcsv)."""
    t = _tables()
    assert tuple(sorted(t)) == TABLE_NAMES
    return t


def _fmt(wall, frac=None, sep=' '):
    return R.naive(wall * 1000000).strftime('%Y-%m-%d' + sep + '%H:%M:%S') + ('' if frac is None else '.' + frac)


def _cells(table, n, seed=3):
    """n date cells for the table: the edge set around its first, a middle and its last transition (gaps and folds),
    the range's two ends, years outside it, seeded wall clocks; as kind 1 and as kind 4; SPECIALS (kinds 0, 2, 3) among them."""
    at, off = table
    rng = random.Random(seed)
    m = len(off)
    walls = R.edge_walls(table, {1, m // 2, m - 1}) if m > 1 else []
    if at[0] > R.I64_MIN:
        lo, hi = at[0] + R.MARGIN, at[-1] - R.MARGIN
        walls += [lo - 1, lo, lo + 90000, hi - 90001, hi - 1, hi, hi + 90000]
    walls += [-30610224000, 253402300799, -1, 0, 1, R.SPAN[1], R.STAMP_BOUND // 1000000 - 1, R.STAMP_BOUND // 1000000]
    walls += [rng.randrange(*R.SPAN) for _ in range(max(0, n - len(walls)))]
    dates = []
    for i, w in enumerate(walls):
        dates.append(_fmt(w, None, ' T'[i & 1]))
        dates.append(_fmt(w, ('5', '000001', '999999', '999999999')[i & 3]))
    rng.shuffle(dates)
    out = []
    for i in range(n):
        out.append(SPECIALS[(i // 7) % len(SPECIALS)] if i % 7 == 3 else dates[i % len(dates)])
    return out


def _want(table, text, rows):
    """The rule's and kwcsv_stamps_local's answers on kwcsv_dates_iso's arrays of the text."""
    from advanced_scrapper_amd import zone as Z
    if rows == 0:
        return [], []
    (us, kind, off), _ = DR.host_arrays(text, 7, 2, 3)
    rule = [R.stamp(table, int(u), int(k), int(o)) for u, k, o in zip(us[:rows], kind[:rows], off[:rows])]
    st, na = Z.stamps_local(us[:rows], kind[:rows], off[:rows],
                            (np.asarray(table[0], np.int64), np.asarray(table[1], np.int32)), 4)
    assert st.tolist() == [v for v, _n in rule] and na.tolist() == [int(n) for _v, n in rule]
    for (v, native), k in zip(rule, kind[:rows].tolist()):
        assert native or v == 0
        assert k in (1, 3, 4) or not native            # kinds 0 and 2 are never native
    return [v for v, _n in rule], [int(n) for _v, n in rule]


@pytest.fixture(scope='module')
def dev(torch_gpu):   # noqa: F811
    from advanced_scrapper_amd import ingest
    h = ingest.DeviceIngest(0, 7, COLS7)
    yield h
    h.close()


def _set(dev, table):
    dev.set_zone((np.asarray(table[0], np.int64), np.asarray(table[1], np.int32)))


def _check(torch, dev, table, n, seed=3):
    text = DR.text(_cells(table, n, seed)) if n else b'\n'        # (a record of no bytes is skipped: no row)
    v, bad, n_rows, _consumed = _parse(torch, dev, text, True, 1 << 20)
    assert (v, n_rows) == (IR.OK, n), (IR.NAMES[v], bad, n_rows)
    st, na = dev.stamps()
    want_st, want_na = _want(table, text, n)
    assert len(st) == len(na) == n
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(zip(st.tolist(), na.tolist()), zip(want_st, want_na))) if g != w]
    assert not diff, diff[:10]
    return na


@pytest.mark.parametrize('name', TABLE_NAMES)
@pytest.mark.parametrize('n', ROWS)
def test_stamps_equal_the_rule(torch_gpu, dev, tables, monkeypatch, name, n):   # noqa: F811
    monkeypatch.setenv(HOOK, str(GRID))
    table = tables[name]
    assert len(table[1]) == {'utc': 1, 'ist': 1, 'two': 2, 'est': 261, 'full': R.CAPACITY}[name]
    _set(dev, table)
    na = _check(torch_gpu, dev, table, n)
    if n >= 257:
        assert 0 < int(na.sum()) < n                   # native and not native rows both
        assert dev.stamps_ms() > 0
        assert set(dev.last_ms()) == {'classify', 'cells', 'arena', 'all'}


def test_default_grid_and_out_of_range_rows(torch_gpu, dev, tables, monkeypatch):   # noqa: F811
    monkeypatch.delenv(HOOK, raising=False)
    table = tables['est']
    _set(dev, table)
    _check(torch_gpu, dev, table, 600, seed=9)
    cells = ['1000-01-01 00:00:00', '1969-12-31 23:59:59', '1970-01-02 23:59:59', '2023-06-05 14:23:11',
             '2099-12-29 00:00:00', '2100-01-01 00:00:00', '9999-12-31 23:59:59', '2023-06-05 14:23:11.25', 'NA', 'soon']
    text = DR.text(cells)
    assert _parse(torch_gpu, dev, text, True, 100)[:3:2] == (IR.OK, len(cells))
    st, na = dev.stamps()
    assert na.tolist() == [0, 0, 0, 1, 1, 0, 0, 1, 0, 0]
    assert st.tolist() == [0, 0, 0, 1685989391, 4102203600, 0, 0, 1685989391, 0, 0]


def test_table_replaced_between_parses(torch_gpu, dev, tables, monkeypatch):   # noqa: F811
    monkeypatch.setenv(HOOK, str(GRID))
    for name in ('full', 'two', 'est', 'utc'):
        _set(dev, tables[name])
        _check(torch_gpu, dev, tables[name], 130, seed=5)
    # the same text under two tables: the stamps follow the table
    text = DR.text(['2023-06-05 14:23:11'] * 3)
    got = []
    for name in ('ist', 'est'):
        _set(dev, tables[name])
        _parse(torch_gpu, dev, text, True, 10)
        got.append(dev.stamps()[0].tolist())
    assert got == [[1685955191] * 3, [1685989391] * 3]


def _code(fn, *a, **kw):
    from advanced_scrapper_amd import _native
    with pytest.raises(_native.KwError) as e:
        fn(*a, **kw)
    return e.value.code


def test_zone_errors(torch_gpu, tables):   # noqa: F811
    from advanced_scrapper_amd import _native, ingest
    EINVAL, ESTATE = _native.KW_EINVAL, _native.KW_ESTATE
    L = _native.lib()
    h = ingest.DeviceIngest(0, 7, COLS7)
    try:
        text = DR.text(['2023-06-05 14:23:11'])
        assert _code(h.stamps) == ESTATE and _code(h.stamps_device) == ESTATE                  # no parse
        _parse(torch_gpu, h, text, True, 10)
        assert _code(h.stamps) == ESTATE and _code(h.stamps_device) == ESTATE                  # a parse without a table
        assert h.stamps_ms() == 0
        at = np.arange(R.CAPACITY + 2, dtype=np.int64)
        off = np.zeros(R.CAPACITY + 1, dtype=np.int32)
        P = lambda a: ctypes.c_void_p(a.ctypes.data)    # noqa: E731
        assert L.kw_ingest_zone(h.h, P(at), P(off), R.CAPACITY + 1) == EINVAL
        assert L.kw_ingest_zone(h.h, P(at), P(off), -1) == EINVAL
        assert L.kw_ingest_zone(h.h, None, P(off), 1) == EINVAL
        assert L.kw_ingest_zone(h.h, P(at), None, 1) == EINVAL
        assert L.kw_ingest_zone(h.h, P(np.array([5, 5], dtype=np.int64)), P(off), 1) == EINVAL
        assert L.kw_ingest_zone(None, P(at), P(off), 1) == EINVAL
        _set(h, tables['ist'])
        assert _code(h.stamps) == ESTATE                                                        # the table came after the parse
        _parse(torch_gpu, h, text, True, 10)
        assert h.stamps()[0].tolist() == [1685955191]
        assert L.kw_ingest_stamps(h.h, None, None) == EINVAL
        assert L.kw_ingest_stamps_device(h.h, None) == EINVAL
        h.set_zone(None)
        _parse(torch_gpu, h, text, True, 10)
        assert _code(h.stamps) == ESTATE
    finally:
        h.close()


# ------------------------------------------------------------------ kw_rows_emit_stamps_device
def _upload(torch, hits):
    a = np.zeros((max(len(hits), 1), 4), dtype=np.int32)
    a[:len(hits)] = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4).view(np.int32)
    return torch.from_numpy(a).to('cuda:0')


def _copy(got):
    return None if got is None else (bytes(got[0]),) + tuple(np.array(a) for a in got[1:])


@pytest.mark.parametrize('make', [ER.one_row_case, lambda: ER.prefix_case(4), lambda: ER.prefix_case(0),
                                  lambda: ER.large_case(seed=12, n=300)], ids=['one', 'prefix4', 'prefix0', 'large'])
def test_emit_from_device_stamps(torch_gpu, make):   # noqa: F811
    from advanced_scrapper_amd import rows as RW
    case = make()
    rng = np.random.default_rng(2)
    case.stamps = rng.integers(-10**11, 10**12, size=case.n_docs).astype(np.int64)     # signs and widths
    h = RW.DeviceRows(0, case.t.tuple(), case.t.n_tickers)
    try:
        h.run(_upload(torch_gpu, case.hits), len(case.hits), case.date_us, case.date_ok, copy_json=False)
        h.cells(case.cells)
        host = _copy(h.emit(case.cols, case.stamps, case.use()))
        d_stamps = torch_gpu.from_numpy(case.stamps.copy()).to('cuda:0')
        dev = _copy(h.emit(case.cols, None, case.use(), d_stamps=ctypes.c_void_p(d_stamps.data_ptr())))
        assert ER.same(dev, host) and ER.same(dev, ER.rule(case))
    finally:
        h.close()


def test_emit_device_errors(torch_gpu):   # noqa: F811
    from advanced_scrapper_amd import _native, rows as RW
    L = _native.lib()
    case = ER.prefix_case(6)
    h = RW.DeviceRows(0, case.t.tuple(), case.t.n_tickers)
    try:
        d_stamps = torch_gpu.from_numpy(case.stamps.copy()).to('cuda:0')
        ptr = ctypes.c_void_p(d_stamps.data_ptr())
        cols = np.ascontiguousarray(case.cols, dtype=np.int32)
        nb, verdict = ctypes.c_int64(), ctypes.c_int32()

        def call(d, n_docs, n_use=1):
            return L.kw_rows_emit_stamps_device(h.h, ctypes.c_void_p(cols.ctypes.data), d, n_docs, n_use,
                                                ctypes.byref(nb), ctypes.byref(verdict), None)
        assert call(ptr, case.n_docs) == _native.KW_ESTATE                 # no run
        h.run(_upload(torch_gpu, case.hits), len(case.hits), case.date_us, case.date_ok, copy_json=False)
        h.cells(case.cells)
        assert call(None, case.n_docs) == _native.KW_EINVAL                # a null pointer
        assert L.kw_rows_last_error(h.h).startswith(b'kw_rows_emit_stamps_device:')   # the message names the call
        assert call(ptr, case.n_docs + 1) == _native.KW_ESTATE             # n_docs differs from the run's
        assert call(ptr, case.n_docs, 7) == _native.KW_EINVAL              # more rows than the run has
        assert call(ptr, case.n_docs, 6) == _native.KW_OK and verdict.value == _native.KW_EMIT_OK and nb.value > 0
        assert L.kw_rows_emit(h.h, ctypes.c_void_p(cols.ctypes.data), None, case.n_docs, 1, ctypes.byref(nb),
                              ctypes.byref(verdict), None) == _native.KW_EINVAL    # kw_rows_emit still refuses a null array
        assert L.kw_rows_last_error(h.h).startswith(b'kw_rows_emit:')
    finally:
        h.close()
