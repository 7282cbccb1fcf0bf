"""GPU: the device ingest (csrc/kwingest.hip) where its loops make more than one trip, its scans more than one
pass, the needed columns lie anywhere in the record, the NA table is at its limits and the calendar is Python's --
the generators and tables of tests/ingest_geometry.py (held on the CPU by tests/test_ingest_geometry_cases.py)
through ``kw_ingest_parse`` against the host tokenizer, byte for byte.

``KW_TEST_INGEST_GRID`` (read by every parse and copy_column) caps the launch grids, so a text of 8 tiles goes
through 8, 4, 3 and 2 trips of a block; the two real-size texts reach the second trip with the production cap."""
import ctypes
import time

import numpy as np
import pytest

from tests import ingest_geometry as G
from tests import ingest_rule as R
from tests.test_gpu_ingest import COLS7, _check, _device_result, _parse, _sweep_text, torch_gpu   # noqa: F401

pytestmark = pytest.mark.gpu
HOOK = 'KW_TEST_INGEST_GRID'


@pytest.fixture(scope='module')
def dev7(torch_gpu):   # noqa: F811
    from advanced_scrapper_amd import ingest
    h = ingest.DeviceIngest(0, 7, COLS7)
    T = h._n.lib().kw_ingest_tile_bytes()
    # the generators' constants are the library's (TILE = BLOCK * 16): a retune fails here, loudly
    assert T == G.T and T // 16 == G.BLOCK == 256 and G.MAX_GRID == 2048
    yield h
    h.close()


def _check_columns(dev, want, ncols):
    for col in range(ncols):
        buf, off, fl = dev.copy_column(col)
        wb, wo, wf = G.column_of(want, ncols, col)
        assert buf.tobytes() == wb and np.array_equal(off, wo) and np.array_equal(fl, wf), col


# ------------------------------------------------------------------ 1. several trips on a small text
def test_trips_small(torch_gpu, dev7, monkeypatch):   # noqa: F811
    shifts = G.trip_shifts()
    texts = [G.trip_text(k) for k in shifts]
    rows = G.trip_rows()
    for g in (1, 2, 3, 5):
        monkeypatch.setenv(HOOK, str(g))
        for text in texts:
            _check(torch_gpu, dev7, text, True, 1 << 20, rows, len(text))
            want = _check(torch_gpu, dev7, text, False, 1 << 20)
            assert want['n_rows'] == rows - 1 and want['consumed'] == text.rfind(b'\n') + 1
        # every column through ig_collen_kernel and ig_gather_kernel<false>, on the parse that stands
        _check_columns(dev7, want, 7)
        # a cap of 5 rows under hundreds of records: every later cell is dropped by the guards
        for final in (True, False):
            want = _check(torch_gpu, dev7, texts[-1], final, 5)
            assert want['n_rows'] == 5 and len(want['coff']) == 36
        _check_columns(dev7, want, 7)
    # values outside [1, 2048] are ignored, and with the variable unset the same texts give the same bytes
    for v in ('0', '2049', '-1', '3x', ''):
        monkeypatch.setenv(HOOK, v)
        _check(torch_gpu, dev7, texts[0], True, 1 << 20, rows, len(texts[0]))
    monkeypatch.delenv(HOOK)
    for text in texts:
        _check(torch_gpu, dev7, text, True, 1 << 20, rows, len(text))
        _check(torch_gpu, dev7, text, False, 1 << 20, rows - 1, text.rfind(b'\n') + 1)
    # without the gate the variable is not read
    monkeypatch.delenv('KW_TEST_HOOKS')
    monkeypatch.setenv(HOOK, '1')
    _check(torch_gpu, dev7, texts[1], True, 1 << 20, rows, len(texts[1]))


def test_trips_edge_lengths(torch_gpu, dev7, monkeypatch):   # noqa: F811
    """No text at all; exactly one tile; a tile and a byte."""
    base = len(_sweep_text(0))
    for g in (None, 1):
        if g:
            monkeypatch.setenv(HOOK, str(g))
        for final in (True, False):
            assert _parse(torch_gpu, dev7, b'', final, 1 << 20) == (R.OK, 0, 0, 0)
        for n in (G.T, G.T + 1):
            text = _sweep_text(n - base)
            assert len(text) == n
            _check(torch_gpu, dev7, text, True, 1 << 20, 12, n)
            _check(torch_gpu, dev7, text, False, 1 << 20, 11, text.rfind(b'\n') + 1)
            # ... and the last byte a record's '\n'
            text = text[:-1] + b'\n'
            _check(torch_gpu, dev7, text, True, 1 << 20, 12, n)
            _check(torch_gpu, dev7, text, False, 1 << 20, 12, n)


# ------------------------------------------------------------------ 2. the real-size texts (numpy compares)
def _check_np(torch, dev, text, final, max_rows, cols=COLS7):
    """_check for millions of cells: the arrays stay numpy arrays.  Returns (the host's result, CPU seconds of the
    oracle and the compares)."""
    v, bad, n_rows, consumed = _parse(torch, dev, text, final, max_rows)
    assert v == R.OK, (R.NAMES[v], bad)
    t0 = time.perf_counter()
    want = G.host_np(text if final else text[:consumed], dev.ncols, cols, max_rows)
    cpu = time.perf_counter() - t0
    assert (n_rows, consumed) == (want['n_rows'], want['consumed'])
    cells = dev.copy_cells()
    arena, off = dev.copy_arena()
    us, kind = dev.dates()
    t0 = time.perf_counter()
    nb = int(cells.off[-1])
    assert dev.cells_device()[3] == nb and dev.arena_device()[2] == int(off[-1])
    assert np.array_equal(cells.off, want['coff']), 'coff'
    assert np.array_equal(cells.flags, want['cfl']), 'cfl'
    assert cells.buf[:nb].tobytes() == want['cells'], 'cells'
    assert np.array_equal(off, want['off']), 'off'
    assert arena.tobytes() == want['arena'], 'arena'
    assert np.array_equal(us, want['us']) and np.array_equal(kind, want['kind']), 'dates'
    assert np.array_equal(dev.column_flags(), want['witness']), 'witness'
    return want, cpu + time.perf_counter() - t0


def test_real_size_many_rows(torch_gpu, dev7, monkeypatch):   # noqa: F811
    """More than MAX_GRID * BLOCK rows in more than MAX_GRID tiles, the production grid cap: the tile kernels, the
    flags and the rows kernel make a second trip, the scans a ninth pass (and the offset scan 4097 passes)."""
    monkeypatch.delenv(HOOK, raising=False)
    text, rows = G.many_rows_text(), G.many_rows_count()
    want, cpu = _check_np(torch_gpu, dev7, text, True, rows + 100)
    assert want['n_rows'] == rows > G.MAX_GRID * G.BLOCK and want['consumed'] == len(text) > G.MAX_GRID * G.T
    # 1000 rows of them: some 3.6 million cells lie beyond the cap
    part, c = _check_np(torch_gpu, dev7, text, False, 1000)
    assert part['n_rows'] == 1000 and part['consumed'] == 125 * len(b''.join(G.MANY_CYCLE))
    cpu += c
    # all but the last, unterminated one
    part, c = _check_np(torch_gpu, dev7, text, True, rows - 1)
    assert part['n_rows'] == rows - 1 and part['consumed'] == text.rfind(b'\n') + 1
    print(f'many_rows: {cpu + c:.2f} s of CPU work in the oracle and the compares')


def test_real_size_long_rows(torch_gpu, dev7, monkeypatch):   # noqa: F811
    """More than 8 scan passes of tiles and an arena above MAX_GRID * BLOCK * 16 bytes: both gathers make a second
    trip; a '""' pair, a 4-byte code point and a quoted "\\r\\n" lie across the scan-pass edges."""
    monkeypatch.delenv(HOOK, raising=False)
    text = G.long_rows_text()
    cpu = 0.0
    for t in (text[:1] + text[2:], text[:1] + b'p' + text[1:], text):
        want, c = _check_np(torch_gpu, dev7, t, True, 1 << 20)
        cpu += c
        assert want['n_rows'] == G.LONG_ROWS and len(want['arena']) - 64 > G.MAX_GRID * G.BLOCK * 16
    buf, off, fl = dev7.copy_column(0)
    wb, wo, wf = G.column_of(want, 7, 0)
    assert len(wb) > G.MAX_GRID * G.BLOCK * 16
    assert buf.tobytes() == wb and np.array_equal(off, wo) and np.array_equal(fl, wf)
    print(f'long_rows: {cpu:.2f} s of CPU work in the oracle and the compares')


# ------------------------------------------------------------------ 3. column layouts, create-time refusals
def test_layouts(torch_gpu, monkeypatch):   # noqa: F811
    from advanced_scrapper_amd import ingest
    monkeypatch.delenv(HOOK, raising=False)
    for ncols, cols in G.layouts():
        text = G.layout_text(ncols, cols)
        rows = 3 if ncols > 64 else 5
        dev = ingest.DeviceIngest(0, ncols, cols)
        try:
            # (_check compares the witness vector and the arena -- article then title -- with the oracle's)
            want = _check(torch_gpu, dev, text, True, 1 << 20, rows, len(text), cols=cols)
            assert want['kind'][:3] == [1, 2, 0] and want['off'][-1] > 0
            # not final: the records before the last one's, up to the '\n' that ends them
            _check(torch_gpu, dev, text, False, 1 << 20, rows - 1, want['spans'][rows - 2][1] + 1, cols=cols)
            monkeypatch.setenv(HOOK, '1')
            _check(torch_gpu, dev, text, True, 2, cols=cols)
            monkeypatch.delenv(HOOK)
        finally:
            dev.close()


def test_create_refusals(torch_gpu):   # noqa: F811
    from advanced_scrapper_amd import _native, ingest
    L, p = _native.lib(), ingest._p
    na_buf, na_off, n_na = ingest._na_table()

    def create(ncols, cols, na=(na_buf, na_off, n_na)):
        h = ctypes.c_void_p(0xDEAD)
        c = np.ascontiguousarray(cols, dtype=np.int32)
        rc = L.kw_ingest_create(0, ncols, p(c), p(na[0]), p(na[1]), na[2], ctypes.byref(h))
        return rc, h

    big = G.na_table([b'%02d' % i for i in range(65)])
    long17 = G.na_table([b'ab', b'A' * 17])
    off1 = (na_buf, na_off + 1, n_na)
    for name, args in (('ncols 5', (5, [0, 1, 2, 3, 4, 4])), ('ncols 4097', (4097, COLS7)),
                       ('a duplicated column', (7, [0, 1, 2, 3, 4, 0])), ('a column = ncols', (7, [0, 1, 2, 3, 4, 7])),
                       ('a negative column', (7, [0, -1, 2, 3, 4, 5])), ('n_na 65', (7, COLS7, big)),
                       ('a 17-byte NA string', (7, COLS7, long17)), ('na_off[0] != 0', (7, COLS7, off1)),
                       ('a negative n_na', (7, COLS7, (na_buf, na_off, -1)))):
        rc, h = create(*args)
        assert rc == _native.KW_EINVAL and not h.value, name
    # the limits themselves are taken
    for args in ((6, COLS7), (4096, COLS7), (7, COLS7, G.NA_64), (7, COLS7, G.NA_EMPTY)):
        rc, h = create(*args)
        assert rc == _native.KW_OK and h.value
        L.kw_ingest_destroy(h)


# ------------------------------------------------------------------ 4. NA tables
def test_na_tables(torch_gpu, monkeypatch):   # noqa: F811
    from advanced_scrapper_amd import ingest
    monkeypatch.delenv(HOOK, raising=False)
    for na, text, rows in ((G.NA_64, G.na64_text(), 7), (G.NA_EMPTY, G.empty_na_text(), len(G.empty_na_rows()))):
        dev = ingest.DeviceIngest(0, 7, COLS7, na=na)
        try:
            for g in (None, 1):
                if g:
                    monkeypatch.setenv(HOOK, str(g))
                for final in (True, False):
                    v, bad, n_rows, consumed = _parse(torch_gpu, dev, text, final, 1 << 20)
                    assert (v, n_rows) == (R.OK, rows - (0 if final or text.endswith(b'\n') else 1)), R.NAMES[v]
                    want = R.host_oracle(text if final else text[:consumed], 7, COLS7, 1 << 20, na)
                    got = _device_result(dev, n_rows, consumed)
                    for k in ('n_rows', 'consumed', 'coff', 'cfl', 'cells', 'off', 'arena', 'us', 'kind', 'witness'):
                        assert got[k] == want[k], k
                    if na is G.NA_EMPTY:
                        # zero-length segments: runs of equal offsets at the arena's start, at multiples of 16, its end
                        assert got['off'] == G.empty_na_offsets() and len(got['arena']) == got['off'][-1] + 64
                        assert got['arena'][-64:] == b'\0' * 64 and b'nan' not in got['arena']
                        assert not any(f & R.F_NA for f in got['cfl'])
                    else:
                        fl = np.array(got['cfl']).reshape(n_rows, 7)
                        assert fl[0, 0] & R.F_NA and not fl[0, 1] & R.F_NA and not fl[2, 0] & R.F_NA
                        assert got['kind'][:4] == [2, 0, 0, 2]
                monkeypatch.delenv(HOOK, raising=False)
        finally:
            dev.close()


# ------------------------------------------------------------------ 5. the calendar
def test_dates_calendar(torch_gpu, dev7, monkeypatch):   # noqa: F811
    cases = G.date_cases()
    text = G.date_text()
    assert len(cases) > G.BLOCK                       # a grid of one block: the rows kernel makes a second trip
    want = R.host_oracle(text, 7, COLS7, 1 << 20)
    for g in (None, 1):
        if g:
            monkeypatch.setenv(HOOK, str(g))
        else:
            monkeypatch.delenv(HOOK, raising=False)
        v, bad, n_rows, consumed = _parse(torch_gpu, dev7, text, True, 1 << 20)
        assert (v, n_rows, consumed) == (R.OK, len(cases), len(text)), R.NAMES[v]
        us, kind = dev7.dates()
        # Python's calendar first
        bad = [(c, (k, u), (int(kind[i]), int(us[i]))) for i, (c, k, u) in enumerate(cases)
               if (k, u) != (int(kind[i]), int(us[i]))]
        assert not bad, bad[:10]
        # ... then the host's
        assert us.tolist() == want['us'] and kind.tolist() == want['kind']
        assert kind[G.DATE_QUOTED_ROW] == 1


# ------------------------------------------------------------------ 6. the text witness
def test_witness_table(torch_gpu, dev7, monkeypatch):   # noqa: F811
    monkeypatch.delenv(HOOK, raising=False)
    cells = G.witness_cells()
    na = R.na_set()
    expect = [G.witness_expect(c, na) for c in cells]
    text = G.witness_text(cells)
    want = _check(torch_gpu, dev7, text, True, 1 << 20, len(cells), len(text))
    fl = np.array(_device_result(dev7, len(cells), len(text))['cfl']).reshape(len(cells), 7)
    assert (fl[:, 0] & (R.F_NA | R.F_TEXT)).tolist() == expect
    assert (fl[:, 4] & (R.F_NA | R.F_TEXT)).tolist() == expect[::-1]
    assert dev7.column_flags().tolist() == want['witness'] == [1, 0, 1, 0, 1, 0]
    quiet = [c for c, w in zip(cells, expect) if w != R.F_TEXT]
    text = G.witness_text(quiet)
    want = _check(torch_gpu, dev7, text, True, 1 << 20, len(quiet), len(text))
    assert dev7.column_flags().tolist() == want['witness'] == [0, 0, 1, 0, 0, 0]
