"""GPU: the article ingest on the device (csrc/kwingest.hip, include/kwingest.h) against the project's host
tokenizer (csrc/kwcsv.c through advanced_scrapper_amd.ingest): cells, offsets, flags, arena, dates, witnesses,
n_rows and consumed byte for byte; the refusals of the take rule (tests/ingest_rule.py, held against kwcsv_parse
by tests/test_ingest_rule.py); kw_rows_cells_device; the drop-in on either route (``KW_INGEST_DEVICE``)."""
import os
import time

import numpy as np
import pytest

from tests import emit_rule as ER
from tests import ingest_rule as R

pytestmark = pytest.mark.gpu

COLS7 = [0, 1, 2, 3, 4, 5]      # article_text, title, date_time, url, source, source_url of the 7-column texts


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


@pytest.fixture(scope='module')
def dev7(torch_gpu):
    """One handle for every 7-column case (so the buffers are reused)."""
    from advanced_scrapper_amd import ingest
    h = ingest.DeviceIngest(0, 7, COLS7)
    yield h
    h.close()


def _parse(torch, dev, text, final, max_rows):
    """kw_ingest_parse of text uploaded with 16 bytes of junk after it (readable, never part of the text)."""
    t = torch.from_numpy(np.frombuffer(text + b'",\n\r" ,\n"\0\xff,,"\n\r', dtype=np.uint8).copy()).to('cuda:0')
    assert t.data_ptr() % 16 == 0
    return dev.parse(t, len(text), final, max_rows)


def _device_result(dev, n_rows, consumed):
    cells = dev.copy_cells()
    arena, off = dev.copy_arena()
    us, kind = dev.dates()
    nb = int(cells.off[-1])
    assert dev.cells_device()[3] == nb and dev.arena_device()[2] == int(off[-1])
    return {'n_rows': n_rows, 'consumed': consumed, 'cells': cells.buf[:nb].tobytes(), 'coff': cells.off.tolist(),
            'cfl': cells.flags.tolist(), 'arena': arena.tobytes(), 'off': off.tolist(), 'us': us.tolist(),
            'kind': kind.tolist(), 'witness': dev.column_flags().tolist()}


def _check(torch, dev, text, final, max_rows, want_rows=None, want_consumed=None, cols=COLS7):
    """A taken parse equals the host tokenizer on the same records; returns the host's result."""
    v, bad, n_rows, consumed = _parse(torch, dev, text, final, max_rows)
    assert v == R.OK, (R.NAMES[v], bad)
    want = R.host_oracle(text if final else text[:consumed], dev.ncols, cols, max_rows)
    if want_rows is not None:
        assert (n_rows, consumed) == (want_rows, want_consumed)
    got = _device_result(dev, n_rows, consumed)
    for k in ('n_rows', 'consumed', 'coff', 'cfl', 'cells', 'off', 'arena', 'us', 'kind', 'witness'):
        assert got[k] == want[k], k
    return want


# ------------------------------------------------------------------ 1. the golden articles
def test_golden_articles(torch_gpu, golden):
    from advanced_scrapper_amd import ingest
    data, cs = golden.articles_csv_bytes(), golden.chunksize()
    names, _head, pos = ingest._split_header(data)
    cols = [names.index(n) for n in ingest.NEEDED]
    dev = ingest.DeviceIngest(0, len(names), cols)
    try:
        rows = 0
        while pos < len(data):
            want = _check(torch_gpu, dev, data[pos:], True, cs, cols=cols)
            assert want['n_rows'] > 0 and all(want['witness'])
            rows += want['n_rows']
            pos += want['consumed']
        assert rows == 642
        ms = dev.last_ms()
        assert set(ms) == {'classify', 'cells', 'arena', 'all'} and all(v > 0 for v in ms.values())
    finally:
        dev.close()


# ------------------------------------------------------------------ 2. the byte-geometry sweep
SWEEP_ROWS = [
    ['first', 'Title one', '2021-03-04 05:06:07', 'http://a/1', 'src', 'http://s/1', 'x'],
    ['a, quoted "cell" with\nbreaks\r\nof both kinds', '', '2021-03-04T05:06:07', 'u', '', 'NA', ''],
    ['', '', '', '', '', '', ''],
    ['café €9 \U0001F600 Ελ', '\U0001F600\U0001F600\U0001F600\U0001F600', 'March 4, 2021', 'u', 's', 't', '1'],
    ['nan', 'NULL', 'N/A', '<NA>', 'n/a', '#N/A N/A', 'None'],
    ['nan ', 'NUL', 'N/A.', '<NA', ' n/a', 'NaNs', 'none'],
    ['12', '-3.5e7', '2021-02-30 00:00:00', 'true', 'FALSE', '+inf', 'Infinity'],
    [' 42 ', 'tru', '0999-01-01 00:00:00', '1 2', 'e', '-', '.'],
    ['""', '"', '2020-02-29 23:59:59', '","', '\n', ',', '"\n"'],
    ['x' * 70, 'y' * 33, '2021-13-01 00:00:00', 'z' * 17, 'w' * 16, 'v' * 15, 'u' * 1],
    ['last but one', 't', '2021-03-04 24:00:00', 'u', 's', 'r', 'q'],
    ['the last', 'record', '1999-12-31 23:59:60', 'has', 'no', 'terminator', 'at all'],
]


def _sweep_text(k: int) -> bytes:
    import csv
    import io
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator='\n', quoting=csv.QUOTE_MINIMAL)
    for i, row in enumerate(SWEEP_ROWS):
        row = list(row)
        if i == 0:
            row[0] = 'f' * k + row[0]
        w.writerow(row)
    text = buf.getvalue().encode('utf-8')
    # quoted forms the writer does not produce: a quoted NA string, an empty quoted cell, a quoted plain cell, "\r\n"
    text = text.replace(b'\nnan,NULL,', b'\r\n"nan","NULL",').replace(b',u,,NA,\n', b',u,"",NA,"q"\r\n')
    assert text.count(b'"nan","NULL"') == 1 and text.count(b',u,"",NA,"q"\r\n') == 1
    return text[:-1]       # the last record ends with the text


CONSTRUCTS = ('pair', 'crlf', 'close+comma', 'cp2', 'cp3', 'cp4')


def _straddled(text: bytes, T: int):
    """The (construct, edge kind) pairs this text puts across an edge: a "" pair, a "\\r\\n", a closing quote + ','
    and a 2-, 3- and 4-byte code point, with a byte on either side of a tile edge (a multiple of T), a wave edge
    (64 lanes = 1024 bytes, inside a tile) or a lane edge (16 bytes, inside a wave)."""
    found = set()

    def mark(name, i, length):
        for j in range(1, length):
            e = i + j
            if e % 16 == 0:
                found.add((name, 'tile' if e % T == 0 else ('wave' if e % 1024 == 0 else 'lane')))
    for name, pat in (('pair', b'""'), ('crlf', b'\r\n'), ('close+comma', b'",')):
        i = text.find(pat)
        while i >= 0:
            mark(name, i, 2)
            i = text.find(pat, i + 1)
    for i, c in enumerate(text):
        if 0xC2 <= c <= 0xDF:
            mark('cp2', i, 2)
        elif 0xE0 <= c <= 0xEF:
            mark('cp3', i, 3)
        elif 0xF0 <= c <= 0xF4:
            mark('cp4', i, 4)
    return found


def sweep_shifts(T: int):
    """The filler lengths of the sweep: every lane offset, every byte of the text across a tile edge (the text's
    byte x lies at k + x: k = T - x - 1 and T - x for each x) and across a wave edge inside the first tile."""
    n = len(_sweep_text(0))
    return sorted(set(range(0, 34)) | set(range(T - n - 1, T + 41)) | set(range(1024 - n - 1, 1025)))


def test_byte_geometry_sweep(torch_gpu, dev7):
    T = dev7._n.lib().kw_ingest_tile_bytes()
    assert T % 1024 == 0 and T > 1024
    base = R.host_oracle(_sweep_text(0), 7, COLS7, 1 << 20)
    assert base['n_rows'] == 12 and sorted(set(base['kind'])) == [0, 1, 2]
    assert base['kind'][6] == 0 and base['kind'][7] == 0 and base['kind'][8] == 1      # invalid day, year 0999, leap day
    shifts = sweep_shifts(T)
    seen = set()
    for k in shifts:
        text = _sweep_text(k)
        seen |= _straddled(text, T)
        want = _check(torch_gpu, dev7, text, True, 1 << 20, 12, len(text))
        assert want['cfl'][7:] == base['cfl'][7:] and want['us'] == base['us']
    assert any(len(_sweep_text(k)) % 16 for k in shifts)
    # each construct really lay across each kind of edge for some shift
    assert seen == {(c, e) for c in CONSTRUCTS for e in ('lane', 'wave', 'tile')}


# ------------------------------------------------------------------ 3. a quoted cell across more than three tiles
def test_quoted_cell_across_tiles(torch_gpu, dev7):
    T = dev7._n.lib().kw_ingest_tile_bytes()
    head = b'a,b,2021-03-04 05:06:07,c,d,e,f\n1,2,3,4,5,6,"'
    body = bytearray()
    while len(body) < 3 * T + 500:
        body += b'lorem, ipsum\n dolor '
    body = bytes(body)
    for shift in range(0, 3):
        # a "" pair across every tile edge the cell crosses: its first quote the tile's last byte
        cell = bytearray(b'p' * shift + body)
        for edge in range(T, len(head) + len(cell), T):
            i = edge - 1 - len(head)
            cell[i:i + 2] = b'""'
        text = head + bytes(cell) + b'"'
        assert all(text[e - 1:e + 1] == b'""' for e in range(T, len(text) - 1, T)) and len(cell) > 3 * T
        want = _check(torch_gpu, dev7, text, True, 1 << 20, 2, len(text))
        assert want['coff'][-1] - want['coff'][-2] == len(cell) - text.count(b'""')
        # not final: the closing quote as the window's last byte proves nothing
        _check(torch_gpu, dev7, text, False, 1 << 20, 1, 32)


# ------------------------------------------------------------------ 4. window semantics
WINDOW_TEXT = (b'a,b,2021-03-04 05:06:07,c,d,e,f\r\n'
               b'"q ""x"" y","line\nbreak\r\nhere",,u,s,t,"z"\r\n'
               b'\n'
               b'1,2,3,4,5,6,"tail ""quote"""\n'
               b'caf\xc3\xa9,\xf0\x9f\x98\x80,NA,"",x,y,z\r\n'
               b'k,l,m,n,o,p,q')


def test_window_cut_at_every_byte(torch_gpu, dev7):
    text = WINDOW_TEXT
    assert len(text) <= 300
    full = R.host_oracle(text, 7, COLS7, 1 << 20)
    assert full['n_rows'] == 5
    # where each record's terminator ends
    term = []
    for _a, b in full['spans']:
        term.append(b + 2 if text[b:b + 2] == b'\r\n' else (b + 1 if text[b:b + 1] == b'\n' else None))
    assert term[-1] is None
    for cut in range(len(text) + 1):
        done = [t for t in term if t is not None and t <= cut]
        v, bad, n_rows, consumed = _parse(torch_gpu, dev7, text[:cut], False, 1 << 20)
        assert (v, n_rows, consumed) == (R.OK, len(done), done[-1] if done else 0), (cut, R.NAMES[v], bad)
        assert R.parse(text[:cut], 7, False, 1 << 20)[:4] == (R.OK, 0, n_rows, consumed)
        if n_rows:
            _check(torch_gpu, dev7, text[:cut], False, 1 << 20, n_rows, consumed)
    _check(torch_gpu, dev7, text, True, 1 << 20, 5, len(text))


# ------------------------------------------------------------------ 5. max_rows
def test_max_rows(torch_gpu, dev7):
    text = _sweep_text(5) + b'\n\n\r\n'
    full = R.host_oracle(text, 7, COLS7, 1 << 20)
    n = full['n_rows']
    assert n == 12
    for m in (1, 2, n - 1, n, n + 1):
        for final in (True, False):
            want = _check(torch_gpu, dev7, text, final, m)
            assert want['n_rows'] == min(m, n) and len(want['coff']) == min(m, n) * 7 + 1
            # kwcsv_records' starts[min(m, n)] on the same bytes: after the last taken record's terminator, or the
            # end of a final text that has fewer records
            if m <= n:
                assert want['consumed'] == full['spans'][m - 1][1] + (2 if m == 2 else 1)
            else:
                assert want['consumed'] == (len(text) if final else len(text) - 3)


# ------------------------------------------------------------------ 6. refusals
GOOD = b'a,b,c,d,e,f,g\n1,"x,y",3,4,5,6,7\r\nu,v,w,x,y,z,"z""q"\n'


def _refusal_cases():
    n = len(GOOD)
    return [
        ('nul', GOOD[:14] + b'\0' + GOOD[14:], True, R.NUL, 14),
        ('utf8', GOOD[:14] + b'\xe2\x82' + GOOD[14:], True, R.UTF8, 14),
        ('utf8 overlong', GOOD[:14] + b'\xc0\xaf' + GOOD[14:], True, R.UTF8, 14),
        ('utf8 truncated at the end', GOOD + b'a,b,c,d,e,f,\xf0\x9f\x98', True, R.UTF8, n + 12),
        ('quote mid-field', GOOD[:15] + b'"' + GOOD[15:], True, R.QUOTE, 15),
        ('after a closing quote', GOOD[:21] + b'z' + GOOD[21:], True, R.QUOTE, 20),
        ('lone cr', GOOD[:15] + b'\r' + GOOD[15:], True, R.CR, 15),
        ('cr at the end of a final text', GOOD + b'1,2,3,4,5,6,7\r', True, R.CR, n + 13),
        ('blank line', GOOD[:14] + b' \t \n' + GOOD[14:], True, R.BLANK, 14),
        ('blank tail', GOOD + b' \t', True, R.BLANK, n),
        ('short record', GOOD[:14] + b'1,2,3,4,5,6\n' + GOOD[14:], True, R.FIELDS, 25),
        ('long record', GOOD[:14] + b'1,2,3,4,5,6,7,8\n' + GOOD[14:], True, R.FIELDS, 29),
        ('short final record', GOOD + b'1,2,3', True, R.FIELDS, n + 5),
        ('unterminated quote', GOOD + b'1,2,3,4,5,6,"7', True, R.QUOTE, n + 14),
        ('nul before utf8', b'a\xff,"\0\n', True, R.NUL, 4),
    ]


def test_refusals(torch_gpu, dev7):
    for name, text, final, verdict, pos in _refusal_cases():
        assert R.parse(text, 7, final, 1 << 20)[:4] == (verdict, pos, 0, 0), name
        got = _parse(torch_gpu, dev7, text, final, 1 << 20)
        assert got == (verdict, pos, 0, 0), (name, got)
        with pytest.raises(dev7._n.KwError) as e:
            dev7.cells_device()
        assert e.value.code == dev7._n.KW_ESTATE
        # the same handle then parses a clean text correctly
        _check(torch_gpu, dev7, GOOD, True, 1 << 20, 3, len(GOOD))
    # an offender beyond the taken records does not refuse them
    _check(torch_gpu, dev7, GOOD + b'x"y\0\n', True, 3, 3, len(GOOD))
    # seeded fuzz: the kernels give the rule's verdict, position, n_rows and consumed on every text
    seen = set()
    for seed in range(120):
        text, ncols = R.fuzz_text(seed)
        if ncols != 7:
            continue
        for final, m in ((True, 1 << 20), (False, 1 << 20), (True, 2)):
            want = R.parse(text, 7, final, m)[:4]
            assert _parse(torch_gpu, dev7, text, final, m) == want, (seed, final, m)
            seen.add(want[0])
    assert len(seen) >= 4


# ------------------------------------------------------------------ 7. kw_rows_cells_device
def test_rows_cells_device(torch_gpu):
    """kw_rows_emit after kw_rows_cells_device on an ingest's device cells gives the same lines, line_off and flags as
    after kw_rows_cells of the downloaded cells."""
    from advanced_scrapper_amd import ingest, rows as RW
    case = ER.large_case(seed=5, n=40)
    cells = case.cells
    # the case's cells as CSV text (QUOTE_MINIMAL; NA cells by their bytes), through the device ingest
    import csv
    import io
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator='\n', quoting=csv.QUOTE_MINIMAL)
    for r in range(cells.nrows):
        w.writerow([bytes(cells.buf[cells.off[r * cells.ncols + c]:cells.off[r * cells.ncols + c + 1]]).decode('utf-8')
                    for c in range(cells.ncols)])
    text = buf.getvalue().encode('utf-8')
    assert R.parse(text, cells.ncols, True, 1 << 20)[:3] == (R.OK, 0, cells.nrows)
    dev = ingest.DeviceIngest(0, cells.ncols, list(range(6)))
    h = RW.DeviceRows(0, case.t.tuple(), case.t.n_tickers)
    try:
        a = np.zeros((max(len(case.hits), 1), 4), dtype=np.int32)
        a[:len(case.hits)] = np.ascontiguousarray(case.hits).view(np.uint32).reshape(-1, 4).view(np.int32)
        d_hits = torch_gpu.from_numpy(a).to('cuda:0')
        v, _bad, n_rows, _c = _parse(torch_gpu, dev, text, True, 1 << 20)
        assert (v, n_rows) == (R.OK, cells.nrows)
        down = dev.copy_cells()
        h.run(d_hits, len(case.hits), case.date_us, case.date_ok, copy_json=False)
        h.cells(down)
        want = h.emit(case.cols, case.stamps, case.use())
        want = (bytes(want[0]),) + tuple(x.copy() for x in want[1:])
        d_cells, d_coff, d_cfl, _nb = dev.cells_device()
        h.cells_device(d_cells, d_coff, d_cfl, cells.nrows, cells.ncols)
        got = h.emit(case.cols, case.stamps, case.use())
        assert len(want[0]) > 0 and bytes(got[0]) == want[0]
        for x, y in zip(got[1:], want[1:]):
            assert np.array_equal(x, y)
        # the argument checks of kw_rows_cells
        L, EINVAL = dev._n.lib(), dev._n.KW_EINVAL
        assert L.kw_rows_cells_device(h.h, d_cells, None, d_cfl, cells.nrows, cells.ncols, None) == EINVAL
        assert L.kw_rows_cells_device(h.h, d_cells, d_coff, d_cfl, -1, cells.ncols, None) == EINVAL
        bad = torch_gpu.from_numpy(np.array([0, 5, 4, 9, 9, 9, 9], dtype=np.int64)).to('cuda:0')
        assert L.kw_rows_cells_device(h.h, d_cells, dev._n.ptr(bad), d_cfl, 1, 6, None) == EINVAL
        assert b'offsets decrease at cell 1' in L.kw_rows_last_error(h.h)
    finally:
        h.close()
        dev.close()


# ------------------------------------------------------------------ 8. the reader's chunks
def test_device_chunk_equals_native_chunk(torch_gpu, tmp_path, monkeypatch):
    """read_chunks_device's items answer as the host reader's do: a DeviceChunk every NativeChunk question -- dates
    (the fast path, dateutil's rows through kw_ingest_copy_column, the row that raises), arena, cells, columns -- and
    a chunk without a text witness in a needed column comes as pandas' DataFrame on both routes."""
    import pandas as pd
    from advanced_scrapper_amd import ingest
    path = tmp_path / 'articles.csv'
    path.write_bytes(','.join(R.names_for(7, COLS7)).encode() + b'\n' + _sweep_text(3) + b'\n')
    monkeypatch.setenv('KW_INGEST_WINDOW', '150')
    raised = frames = 0
    for chunksize in (4, 1):
        host = list(ingest.read_chunks(str(path), chunksize))
        got = []
        for chunk in ingest.read_chunks_device(str(path), chunksize, 0):
            want = host[len(got)]
            got.append(chunk)
            if isinstance(want, pd.DataFrame):
                assert isinstance(chunk, pd.DataFrame) and chunk.equals(want)
                frames += 1
                continue
            assert type(chunk) is ingest.DeviceChunk and type(want) is ingest.NativeChunk
            assert len(chunk) == len(want) and chunk.index0 == want.index0 and chunk.columns == want.columns
            d, e = chunk.dates()
            dw, ew = want.dates()
            assert len(d) == len(dw) and [d[i] for i in range(len(d))] == [dw[i] for i in range(len(dw))]
            assert type(e) is type(ew) and str(e) == str(ew)
            raised += e is not None
            assert chunk.column_values('article_text', 3) == want.column_list('article_text')[:3]
            a, o = chunk.arena()
            aw, ow = want.arena()
            assert a.tobytes() == aw.tobytes() and o.tolist() == ow.tolist()
            assert chunk._cells is None                       # nothing so far needed the cells on the host
            nb = int(want.cells.off[-1])
            assert chunk.cells.buf[:nb].tobytes() == want.cells.buf[:nb].tobytes()
            assert chunk.cells.off.tolist() == want.cells.off.tolist()
            assert chunk.cells.flags.tolist() == want.cells.flags.tolist()
            assert chunk.frame().equals(want.frame())
        assert len(got) == len(host) == 12 // chunksize
        st = ingest.LAST_STATS
        assert st['grown'] >= 1 and st['host'] == 0 and st['device'] + st['pandas'] == len(got)
        if chunksize == 4:
            assert type(got[0]) is ingest.DeviceChunk
            with pytest.raises(RuntimeError):
                got[0].device_arena()                          # a later chunk took the buffers
    assert raised >= 2 and frames >= 2


# ------------------------------------------------------------------ 9. the drop-in
def _run_main(csv_bytes, chunksize, processed, tmp_path, monkeypatch, name, ingest_env, window=None):
    """match_keywords.run over an article CSV: {file: bytes} and the device reader's counters (None on the host route)."""
    from advanced_scrapper_amd import ingest, match_keywords as mk
    work = tmp_path / name
    work.mkdir()
    (work / 'articles.csv').write_bytes(csv_bytes)
    monkeypatch.setenv('TZ', 'UTC')
    time.tzset()
    monkeypatch.chdir(work)
    monkeypatch.setenv('KW_INGEST_DEVICE', ingest_env)
    if window is None:
        monkeypatch.delenv('KW_INGEST_WINDOW', raising=False)
    else:
        monkeypatch.setenv('KW_INGEST_WINDOW', str(window))
    monkeypatch.setattr(mk, 'read_and_process_json_files', lambda _d: processed)
    ingest.LAST_STATS = None
    args = mk._parse(['--info-dir', 'unused', '--articles', str(work / 'articles.csv'), '--chunksize', str(chunksize)])
    assert mk.run(args, 0, 1, None, None) == 0
    out = work / 'yahoo_ticker_matched_articles'
    return {fn: (out / fn).read_bytes() for fn in os.listdir(out)}, ingest.LAST_STATS


def _first_records(data: bytes, n: int) -> bytes:
    from advanced_scrapper_amd import ingest
    names, _head, pos = ingest._split_header(data)
    got = R.host_parse(data[pos:], len(names), n)
    assert got[0] == n
    return data[:pos + got[1]]


def test_dropin(torch_gpu, golden, tmp_path, monkeypatch):
    src = _first_records(golden.articles_csv_bytes(), 300)
    kb = golden.kb_processed()
    host, stats = _run_main(src, 64, kb, tmp_path, monkeypatch, 'host', '0')
    assert stats is None and len(host) > 0
    # the chunks' bytes: a window that holds the first two chunks and, beyond them, as many bytes as the second took
    # -- it serves two chunks, and what is left of it looks like a chunk's worth but ends inside the third, which is
    # larger: that chunk needs a grown window
    from advanced_scrapper_amd import ingest
    names, _head, pos = ingest._split_header(src)
    size = []
    while pos < len(src):
        size.append(R.host_parse(src[pos:], len(names), 64)[1])
        pos += size[-1]
    assert len(size) == 5 and size[2] > size[1]
    window = size[0] + 2 * size[1]
    dev, stats = _run_main(src, 64, kb, tmp_path, monkeypatch, 'device', '1', window)
    assert stats['routes'] == ['device'] * 5 and stats['reused'] >= 1 and stats['grown'] >= 1, stats
    assert sorted(dev) == sorted(host) and all(dev[f] == host[f] for f in host)
    # a window smaller than any chunk: grown before the first chunk is taken
    dev, stats = _run_main(src, 64, kb, tmp_path, monkeypatch, 'small', '1', 4096)
    assert stats['routes'] == ['device'] * 5 and stats['grown'] >= 5
    assert sorted(dev) == sorted(host) and all(dev[f] == host[f] for f in host)


def test_dropin_refused_chunk(torch_gpu, golden, tmp_path, monkeypatch):
    """One record with a '"' mid-field in the third chunk: that chunk alone takes the host route."""
    from advanced_scrapper_amd import ingest
    src = _first_records(golden.articles_csv_bytes(), 300)
    names, _head, pos = ingest._split_header(src)
    spans = R.host_parse(src[pos:], len(names), 300)[5]
    at = pos + spans[150][1]                      # the end of record 150's last cell, source_url: unquoted
    assert src[at - 1:at] != b'"' and src[at:at + 1] in (b'\n', b'\r')
    bad = src[:at - 1] + b'"' + src[at - 1:]
    kb = golden.kb_processed()
    host, _ = _run_main(bad, 64, kb, tmp_path, monkeypatch, 'host', '0')
    dev, stats = _run_main(bad, 64, kb, tmp_path, monkeypatch, 'device', '1')
    assert stats['routes'] == ['device', 'device', 'host', 'device', 'device'], stats
    assert len(host) > 0 and sorted(dev) == sorted(host) and all(dev[f] == host[f] for f in host)
