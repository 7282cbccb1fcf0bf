"""Generators and expectation tables for the device ingest's multi-trip, multi-pass, column, NA and date paths
(csrc/kwingest.hip): pure Python / numpy.  tests/test_ingest_geometry_cases.py holds them against the take rule
(tests/ingest_rule.py) and the host tokenizer where no GPU is needed; tests/test_gpu_ingest_geometry.py runs them
through ``kw_ingest_parse``.

The kernels launch capped grids and loop (``tile += gridDim.x``; ``i += gridDim.x * BLOCK``); the cap is MAX_GRID
blocks, or ``KW_TEST_INGEST_GRID``.  ``trip_text`` is a small text for a lowered cap; the two
real-size texts reach a second trip and a ninth scan pass with the production constants.  The date table's
expectations come from ``datetime`` and ``calendar.timegm`` alone.
"""
import calendar
import csv
import datetime
import io
import re

import numpy as np

from tests import ingest_rule as R
from tests.test_gpu_ingest import CONSTRUCTS, SWEEP_ROWS, _sweep_text

T = 4096                   # kw_ingest_tile_bytes() (the GPU test asserts the two are equal)
BLOCK = 256
MAX_GRID = 2048
PASS = BLOCK * T           # bytes of text whose tiles one pass of ig_scan_kernel's loop scans
COLS7 = [0, 1, 2, 3, 4, 5]


# ------------------------------------------------------------------ constructs and the edges they lie across
def construct_spans(text: bytes):
    """(name, first byte, length) of every "" pair, "\\r\\n", closing quote + ',' and 2-, 3-, 4-byte code point."""
    for name, pat in (('pair', b'""'), ('crlf', b'\r\n'), ('close+comma', b'",')):
        i = text.find(pat)
        while i >= 0:
            yield name, i, 2
            i = text.find(pat, i + 1)
    arr = np.frombuffer(text, dtype=np.uint8)
    for i in np.flatnonzero(arr >= 0xC2).tolist():
        c = text[i]
        if c <= 0xDF:
            yield 'cp2', i, 2
        elif 0xE0 <= c <= 0xEF:
            yield 'cp3', i, 3
        elif 0xF0 <= c <= 0xF4:
            yield 'cp4', i, 4


def straddled(text: bytes, edge_bytes: int = T):
    """{(construct, e)}: the construct has a byte on either side of position e * edge_bytes."""
    found = set()
    for name, i, length in construct_spans(text):
        e = (i + length - 1) // edge_bytes
        if e != i // edge_bytes:
            found.add((name, e))
    return found


def owner(tile: int, g: int):
    """(block, trip) of a tile under a grid of g blocks (``tile = blockIdx.x; tile += gridDim.x``)."""
    return tile % g, tile // g


def tile_census(text: bytes):
    """Per tile of text (from R.parse's byte classes, restated with numpy): (kept bytes, cell ends, record ends)."""
    a = np.frombuffer(text, dtype=np.uint8)
    q = a == 0x22
    inside = (np.cumsum(q) - q) & 1
    prev = np.concatenate([[0x0A], a[:-1]])
    prev2 = np.concatenate([[0x0A, 0x0A], a[:-2]])
    out = inside == 0
    delim = (a == 0x2C) & out
    nl = (a == 0x0A) & out
    rec_end = nl & ~((prev == 0x0A) | ((prev == 0x0D) & (prev2 == 0x0A)))
    pair2 = q & out & (prev == 0x22)
    kept = ~(delim | nl | ((a == 0x0D) & out) | (q & ~pair2))
    res = []
    for lo in range(0, len(text), T):
        s = slice(lo, lo + T)
        res.append((int(kept[s].sum()), int(delim[s].sum() + rec_end[s].sum()), int(rec_end[s].sum())))
    return res


# ------------------------------------------------------------------ the trip text
_UNIT = 'lorem, ipsum\n dolor ""sit"" amet\r\n café €9 \U0001F600 elit, '.encode('utf-8')


def _fill(n: int) -> bytes:
    """n bytes of quoted-cell body: ',', '\\n', '\\r\\n', '""' pairs and 2-, 3-, 4-byte code points, whole."""
    return _UNIT * (n // len(_UNIT)) + b'x' * (n % len(_UNIT))


def trip_text(k: int) -> bytes:
    """About 7 tiles of 7-column CSV; k filler bytes in the first cell move every later byte.  With S the bytes of
    the sweep rows and 0 <= k <= T - S:

      [0, S + k)           the sweep rows, k filler bytes in the first cell
      [.., 3T - S + k)     one record whose quoted first cell holds tile 1 whole (no cell end in that tile)
      [.., 3T + k)         the sweep rows: byte x of them lies across 3T for k = S - x
      [.., 5T + k)         '\\n' and '\\r\\n' only -- zero-length records; tile 4 has no kept byte and no record end
      [.., 7T + k)         ',,,,,,\\n' records; tile 6 has cell ends and no kept byte
      [.., 7T + S - 1 + k) the sweep rows, the last record unterminated: a partial last tile
    """
    block = _sweep_text(0) + b'\n'
    S = len(block)
    assert 0 <= k <= T - S
    tail = b'",long title,2021-03-04T05:06:07,u,s,r,q\n'
    long_rec = b'"' + _fill(3 * T - 2 * S - 1 - len(tail)) + tail
    blank = b'\n\r\n' * ((2 * T) // 3) + b'\r\n'
    empties = b',,,,,,\n' * ((2 * T) // 7) + b'\n\n'
    assert len(long_rec) == 3 * T - 2 * S and len(blank) == 2 * T and len(empties) == 2 * T
    text = _sweep_text(k) + b'\n' + long_rec + block + blank + empties + block[:-1]
    assert len(text) == 7 * T + S - 1 + k
    return text


def trip_rows() -> int:
    """The records of a trip text read as a final text."""
    return 3 * len(SWEEP_ROWS) + 1 + (2 * T) // 7


def trip_shifts():
    """Fillers that put each construct of the middle sweep rows, byte by byte, across the tile edge 3T (k = S - x - j
    for byte j >= 1 of a construct at x), and 0 and 1."""
    block = _sweep_text(0) + b'\n'
    S = len(block)
    ks = {0, 1}
    first = {}
    for name, i, length in construct_spans(block):
        first.setdefault(name, (i, length))
    assert set(first) == set(CONSTRUCTS)
    for i, length in first.values():
        ks |= {S - i - j for j in range(1, length)}
    return sorted(ks)


# ------------------------------------------------------------------ the two real-size texts
MANY_CYCLE = (b'a,b,2021-03-04 05:06:07,,,,\n',        # the layout date (the one record above 24 bytes)
              b'x,y,NA,u,s,,q\n',                      # an NA date
              b'"q,""z",,,,,,q\r\n',                   # a quoted cell with a ',' and a pair; "\r\n"
              b'nan,,,,,,N/A\n',
              b'12,3.5,d,,,6,7\n',
              b'caf\xc3\xa9,t,d,,,,q\n',
              b'e,"f\ng",d,,,,q\r\n',                  # a quoted '\n'
              b'wx,,y,,,,z1\n')
MANY_CYCLES = 65537


def many_rows_text() -> bytes:
    """Just over MAX_GRID * BLOCK rows in just over MAX_GRID tiles: the per-cell and per-row kernels make a second
    trip, the tile kernels a second trip, the scans a ninth pass.  The last record has no terminator."""
    cyc = b''.join(MANY_CYCLE)
    assert R.parse(cyc, 7, True, 100)[:4] == (R.OK, 0, len(MANY_CYCLE), len(cyc))
    assert all(12 <= len(c) <= 24 for c in MANY_CYCLE[1:]) and len(MANY_CYCLE[0]) == 28
    text = np.tile(np.frombuffer(cyc, dtype=np.uint8), MANY_CYCLES).tobytes()[:-1]
    assert many_rows_count() > MAX_GRID * BLOCK and len(text) > MAX_GRID * T
    return text


def many_rows_count() -> int:
    return len(MANY_CYCLE) * MANY_CYCLES


LONG_ROWS = 40
LONG_BODY = 230000
_LONG_TAIL = b'",Title %02d,2021-03-04 05:06:07,u,s,r,q\n'


def long_rows_edges():
    """{scan-pass edge e (the byte position e * PASS): the construct long_rows_text puts across it}."""
    n = LONG_ROWS * (1 + LONG_BODY + len(_LONG_TAIL % 0))
    edges = {e: 'pair' for e in range(1, n // PASS + 1)}
    edges[3] = 'cp4'
    edges[5] = 'crlf'
    return edges


def long_rows_text() -> bytes:
    """40 records whose quoted article cell holds 230 000 bytes (',', '\\n', '\\r\\n', '""' pairs, code points): more
    than 8 * BLOCK tiles and an arena above MAX_GRID * BLOCK * 16 bytes (the gathers' second trip).  Across every
    multiple of PASS lies a '""' pair (its first quote the byte before the edge) -- across 3 * PASS a 4-byte code
    point (two bytes a side), across 5 * PASS a quoted '\\r\\n' instead.  MAX_GRID * T is the eighth of these edges
    and the edge between a block's first and second trip.  The first cell begins 'pp': a byte less or more there
    moves every construct off its edge."""
    edges = long_rows_edges()
    what = {'pair': (b'""', 1), 'cp4': ('\U0001F600'.encode('utf-8'), 2), 'crlf': (b'\r\n', 1)}
    parts, pos, placed = [], 0, set()
    for r in range(LONG_ROWS):
        parts.append(b'"pp')
        pos += 3
        end = pos + LONG_BODY - 2
        while pos < end:
            e = pos // PASS + 1
            con, before = what[edges.get(e, 'pair')]
            at = e * PASS - before
            if pos <= at and at + len(con) <= end:
                parts += [_fill(at - pos), con]
                pos = at + len(con)
                placed.add(e)
            else:
                parts.append(_fill(end - pos))
                pos = end
        tail = _LONG_TAIL % r
        parts.append(tail)
        pos += len(tail)
    text = b''.join(parts)
    assert len(text) == pos and placed == set(edges) and MAX_GRID * T // PASS in placed
    assert len(text) > 8 * BLOCK * T and (len(text) + T - 1) // T > MAX_GRID
    return text


# ------------------------------------------------------------------ column layouts
def layouts():
    return [(6, [0, 1, 2, 3, 4, 5]), (6, [5, 4, 3, 2, 1, 0]), (7, [6, 1, 0, 3, 4, 5]), (9, [8, 0, 4, 1, 2, 3]),
            (9, [1, 2, 8, 0, 4, 5]), (64, [63, 0, 31, 32, 1, 62]), (4096, [4095, 0, 2048, 1, 4094, 7])]


_LAYOUT_NEEDED = [
    ['An article, "quoted" inside', 'Title one', '2021-03-04 05:06:07', 'http://a/1', 'src', 'http://s/1'],
    ['second café \U0001F600', 'NA', 'NA', 'u', 'say "hi"', ''],
    ['12', 'third\ntitle', '2021-02-30 00:00:00', '1,2', 'true', '-3.5e7'],
    ['', '', '2020-02-29T23:59:59', 'nan', ' 42 ', 'line\r\nbreak'],
    ['the last', 'record', '1999-12-31 23:59:59', 'has', 'no', 'terminator'],
]


def layout_text(ncols: int, cols) -> bytes:
    """3 to 5 records of R.WORDS cells with the needed cells of _LAYOUT_NEEDED at ``cols``; a needed cell is quoted
    with a '""' pair; the last record has no terminator.  With 4096 columns a record spans more than one tile."""
    rows = 3 if ncols > 64 else 5
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator='\n', quoting=csv.QUOTE_MINIMAL)
    for r in range(rows):
        row = [R.WORDS[(5 * r + 3 * c) % len(R.WORDS)] for c in range(ncols)]
        for k, c in enumerate(cols):
            row[c] = _LAYOUT_NEEDED[r][k]
        w.writerow(row)
    text = buf.getvalue().encode('utf-8')[:-1]
    assert b'""quoted""' in text and (ncols < 4096 or len(text) > rows * T)
    return text


# ------------------------------------------------------------------ NA tables
def na_table(strings):
    """(buf, off, n) in the shape of ingest._na_table()."""
    vals = [s if isinstance(s, bytes) else s.encode('utf-8') for s in strings]
    off = np.zeros(len(vals) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in vals], dtype=np.int64)
    return np.frombuffer(b''.join(vals) or b'\0', dtype=np.uint8).copy(), off, len(vals)


def na_frozenset(na):
    buf, off, n = na
    return frozenset(bytes(buf[off[k]:off[k + 1]]) for k in range(n))


NA16 = b'ABCDEFGHIJKLMNOP'                  # MAX_NA_LEN bytes
NA_EMPTY = na_table([])
NA_64 = na_table([NA16, b'-', b''] + [('na%d' % i).encode() * (1 + i % 3) for i in range(61)])   # MAX_NA entries
assert NA_64[2] == 64 and len(na_frozenset(NA_64)) == 64 and max(np.diff(NA_64[1])) == 16


def na64_text() -> bytes:
    """Cells at the table's limits: the 16-byte string, its first 15 bytes, itself and a byte; the 1-byte string and
    ''; pandas' NA strings, which this table does not hold."""
    s = NA16.decode()
    rows = [[s, s[:15], s, 'u', 's', 'r', 'q'],
            [s[:15], s, s[:15], '-', '', s + 'Q', 'q'],
            [s + 'Q', s + 'Q', s + 'Q', s, s[:15], '-', ''],
            ['-', '', '-', 'na7', 'na7na7', 'na8na8na8', 'na7na'],
            ['', '-', '', '--', ' ', 'na60', 'na61'],
            ['nan', 'NULL', 'NA', 'N/A', s.lower(), s[1:], '2021-03-04 05:06:07'],
            [s[1:] + 'A', 'P' + s[:15], '2021-03-04 05:06:07', 'x', 'y', 'z', s]]
    return '\n'.join(','.join(r) for r in rows).encode()


def empty_na_rows():
    """(article, title) of each row for the empty NA table, where '' is a cell of no bytes and not "nan": runs of
    1, 2 and 40 rows with both cells empty -- at the arena's very start, at offsets that are multiples of 16, at one
    that is not, and at its very end with a total that is a multiple of 16 -- and single empty cells."""
    rows = [('', '')]                                   # offset 0
    rows += [('a' * 10, 'b' * 6)] + [('', '')] * 2      # offset 16
    rows += [('c' * 5, 'd' * 4)] + [('', '')] * 40      # offset 25
    rows += [('e' * 20, 'f' * 3)] + [('', '')] * 40     # offset 48
    rows += [('', 'g' * 7), ('h' * 9, ''), ('', '')]    # offset 64 after them
    rows += [('i' * 16, ''), ('', 'j' * 16), ('k' * 15, 'l' * 17)]
    rows += [('', '')] * 2                              # the arena's end: 128
    return rows


def empty_na_text() -> bytes:
    return ''.join('%s,%s,2021-03-04 05:06:07,u,,r,q\n' % (a, t) for a, t in empty_na_rows()).encode()


def empty_na_offsets():
    off = [0]
    for a, t in empty_na_rows():
        off += [off[-1] + len(a), off[-1] + len(a) + len(t)]
    assert off[-1] % 16 == 0 and off[1:3] == [0, 0] and off[-5:] == [off[-1]] * 5
    return off


# ------------------------------------------------------------------ the date table
_LAYOUT = re.compile(rb'[0-9]{4}-[0-9]{2}-[0-9]{2}[ T][0-9]{2}:[0-9]{2}:[0-9]{2}')
DATE_NA = [b'NA', b'nan', b'NULL', b'', b'N/A', b'<NA>']        # (of pandas' default NA strings)
DATE_YEARS = (1000, 1582, 1600, 1899, 1900, 1969, 1970, 1972, 2000, 2038, 2100, 2400, 9999)


def date_expect(cell: bytes):
    """(kind, us) of a date cell by Python's calendar: kind 2 for an NA string; kind 1 for the intact layout
    'YYYY-MM-DD HH:MM:SS' (' ' or 'T') with year >= 1000 whose fields ``datetime`` accepts, us = its epoch
    microseconds read as UTC (negative before 1970); else kind 0."""
    if cell in DATE_NA:
        return 2, 0
    if len(cell) != 19 or not _LAYOUT.fullmatch(cell):
        return 0, 0
    f = [int(cell[a:b]) for a, b in ((0, 4), (5, 7), (8, 10), (11, 13), (14, 16), (17, 19))]
    if f[0] < 1000:
        return 0, 0
    try:
        datetime.datetime(*f)
    except ValueError:
        return 0, 0
    return 1, calendar.timegm(tuple(f)) * 10 ** 6


def date_cases():
    """[(cell bytes, kind, us)]."""
    cells = []
    for y in DATE_YEARS:
        for rest in ('01-01?00:00:00', '02-28?13:14:15', '02-29?13:14:15', '03-01?00:00:01', '12-31?23:59:59'):
            for sep in ' T':
                cells.append('%04d-%s' % (y, rest.replace('?', sep)))
    for y in (2023, 2024):
        for m in range(1, 13):
            last = calendar.monthrange(y, m)[1]
            for d in (last, last + 1):
                for sep in ' T':
                    cells.append('%04d-%02d-%02d%s12:00:00' % (y, m, d, sep))
    cells += ['2021-03-00 05:06:07', '2021-00-04 05:06:07', '2021-13-04 05:06:07', '2021-03-04 24:06:07',
              '2021-03-04 05:60:07', '2021-03-04 05:06:60', '0999-03-04 05:06:07']
    for base in ('2021-03-04 05:06:07', '1968-11-30T23:58:59'):
        for i in range(19):
            for ch in '/x ':
                cells.append(base[:i] + ch + base[i + 1:])
    cells += ['2021-03-04 05:06:0', '2021-03-04 05:06:070', ' 2021-03-04 05:06:07', '2021-03-04 05:06:07 ',
              '2021-03-04 05:06', '2021-03-04', '2021-03-04 05:06:07.5', '20210304T050607']
    cells += ['2021-03-04 05:06:0٧', '٢021-03-04 05:06:07', '2021-03-0² 05:06:07']   # 2-byte code points
    out = [c.encode('utf-8') for c in cells] + DATE_NA
    assert all(len(c) == 20 for c in out[-9:-6])
    return [(c,) + date_expect(c) for c in out]


DATE_QUOTED_ROW = 0        # date_text quotes this row's date cell (the quotes are stripped: the kind stays 1)


def date_text() -> bytes:
    """The table as the date column (2) of a 7-column text, a record a case."""
    rows = []
    for i, (cell, _k, _u) in enumerate(date_cases()):
        assert b',' not in cell and b'"' not in cell
        d = b'"' + cell + b'"' if i == DATE_QUOTED_ROW else cell
        rows.append(b'art %d,t,' % i + d + b',u,s,r,q\n')
    return b''.join(rows)


# ------------------------------------------------------------------ the witness table
WITNESS_BASES = ['true', 'false', 'inf', 'infinity', '+inf', '-Infinity', '1e5', '+', '-', '.', 'e', '+-inf',
                 'infinityx', '+infinity', '+infinityy', 'nan', 'tru', '1_0', '0x1F', '1,2']


def witness_cells():
    """About 120 cells: each base in three letter cases, bare and padded with spaces and tabs; blanks only."""
    cells = []
    for b in WITNESS_BASES:
        forms = [b.lower(), b.upper(), ''.join(c.upper() if i % 2 else c.lower() for i, c in enumerate(b))]
        for f in forms:
            cells += [f, ' \t' + f + '\t  ']
    cells += [' ', '\t', '  \t ', ' ' * 9, ' ' * 17]
    return [c.encode() for c in cells]


def witness_expect(cell: bytes, na) -> int:
    """The cell's NA / TEXT flag bits by the rule (R.text_witness; ``na`` a frozenset)."""
    return R.F_NA if cell in na else (R.F_TEXT if R.text_witness(cell) else 0)


def witness_rows(cells):
    """Column 0 the cells, column 4 the cells in reverse; columns 1, 3, 5 never a witness; column 2 always."""
    n = len(cells)
    return [[cells[r], b'12', b'2021-03-04 05:06:07', b'true', cells[n - 1 - r], b'', b'x'] for r in range(n)]


def witness_text(cells) -> bytes:
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator='\n', quoting=csv.QUOTE_MINIMAL)
    for row in witness_rows(cells):
        w.writerow([c.decode() for c in row])
    return buf.getvalue().encode()


# ------------------------------------------------------------------ the host oracle as numpy arrays
def host_np(text: bytes, ncols: int, cols, max_rows: int, na=None):
    """R.host_oracle for a text of millions of cells: the same keys as numpy arrays (cells, arena: bytes; arena with
    its 64 zero bytes), through kwcsv_parse, kwcsv_pack_mt and kwcsv_dates."""
    import ctypes
    from advanced_scrapper_amd import ingest
    na_buf, na_off, n_na = ingest._na_table() if na is None else na
    p, L = ingest._p, ingest._lib()
    buf = np.frombuffer(text + b'\0' * 16, dtype=np.uint8)
    cap_rows = min(max_rows, len(text) // ncols + 1)
    out = np.empty(len(text) + 16, dtype=np.uint8)
    coff = np.zeros(cap_rows * ncols + 1, dtype=np.int64)
    cfl = np.zeros(max(cap_rows * ncols, 1), dtype=np.uint8)
    pos = ctypes.c_int64(0)
    rows = int(L.kwcsv_parse(p(buf), len(text), 0, cap_rows, ncols, p(na_buf), p(na_off), n_na, p(out), len(text) + 16,
                             p(coff), p(cfl), ctypes.byref(pos), None))
    assert rows >= 0, rows
    nc = rows * ncols
    coff, cfl = coff[:nc + 1], cfl[:nc]
    cells = ingest.Cells(out, coff, cfl, rows, ncols)
    arena, off = ingest.NativeChunk(cells, R.names_for(ncols, cols), 0).arena()
    us = np.zeros(max(rows, 1), dtype=np.int64)
    kind = np.zeros(max(rows, 1), dtype=np.uint8)
    L.kwcsv_dates(p(out), p(coff), p(cfl), rows, ncols, cols[2], p(us), p(kind), ingest.host_threads())
    fl = cfl.reshape(rows, ncols)
    return {'n_rows': rows, 'consumed': int(pos.value), 'cells': out[:int(coff[nc])].tobytes(), 'coff': coff,
            'cfl': cfl, 'arena': arena.tobytes(), 'off': off, 'us': us[:rows], 'kind': kind[:rows],
            'witness': np.array([int((fl[:, c] & R.F_TEXT).any()) for c in cols], dtype=np.int32)}


def column_of(want, ncols: int, col: int):
    """(bytes, off, flags) of one column of an oracle result (R.host_oracle's or host_np's), dense, as numpy."""
    coff = np.asarray(want['coff'], dtype=np.int64)
    cfl = np.asarray(want['cfl'], dtype=np.uint8)
    rows = want['n_rows']
    lo, hi = coff[col:rows * ncols:ncols], coff[col + 1:rows * ncols + 1:ncols]
    off = np.zeros(rows + 1, dtype=np.int64)
    off[1:] = np.cumsum(hi - lo)
    cells = want['cells']
    return b''.join(cells[a:b] for a, b in zip(lo.tolist(), hi.tolist())), off, cfl[col::ncols][:rows]
