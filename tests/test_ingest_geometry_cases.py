"""CPU: the generators and tables of tests/ingest_geometry.py, held where no GPU is needed -- every small text is
taken by the rule (tests/ingest_rule.py) with kwcsv_parse's cells under the same NA table; the trip texts put every
construct across a tile edge that lies between two blocks and between one block's consecutive trips; the real-size
texts pass their thresholds; kwcsv_dates gives the ``datetime`` table; kwcsv_parse's TEXT flag the witness table."""
import numpy as np
import pytest

from tests import ingest_geometry as G
from tests import ingest_rule as R


def _rule_equals_host(text, ncols, na=None, rows=None):
    """R.parse takes the text, final or not, with the host tokenizer's cells, offsets and flags; the host result."""
    naset = R.na_set() if na is None else G.na_frozenset(na)
    for final in (True, False):
        v, bad, n_rows, consumed, cells = R.parse(text, ncols, final, 1 << 20, naset)
        assert v == R.OK, (R.NAMES[v], bad)
        got = R.host_parse(text if final else text[:consumed], ncols, 1 << 20, na)
        assert got[:2] == (n_rows, consumed)
        assert (got[2], got[3], got[4]) == (cells[0], cells[1], cells[2])
        if final and rows is not None:
            assert n_rows == rows
    return R.host_parse(text, ncols, 1 << 20, na)


# ------------------------------------------------------------------ the trip texts
def test_trip_texts_rule_and_special_tiles():
    shifts = G.trip_shifts()
    assert 8 <= len(shifts) <= 16
    partial = False
    for k in shifts:
        text = G.trip_text(k)
        got = _rule_equals_host(text, 7, rows=G.trip_rows())
        census = G.tile_census(text)
        assert len(census) == 8
        assert census[1][0] > G.T // 2 and census[1][1] == 0      # wholly inside one quoted cell: no cell end
        a, b = got[5][len(G.SWEEP_ROWS)]                          # (the record after the first sweep rows)
        assert a < G.T and 2 * G.T < a + got[3][7 * len(G.SWEEP_ROWS) + 1] - got[3][7 * len(G.SWEEP_ROWS)] < b
        assert census[4] == (0, 0, 0)                             # zero-length records: nothing kept, no record end
        assert census[6][0] == 0 and census[6][1] > 6 * census[6][2] > 0        # empty records: cell ends, nothing kept
        partial |= len(text) % G.T % 16 != 0
    assert partial                                                # a last tile that is no multiple of 16 bytes


def test_trip_texts_straddle_blocks_and_trips():
    seen = set()
    for k in G.trip_shifts():
        seen |= G.straddled(G.trip_text(k), G.T)
    for c in G.CONSTRUCTS:
        edges = sorted(e for name, e in seen if name == c)
        assert edges, c
        # across an edge whose two tiles two blocks own under a grid of 2, 3 and 5 blocks ...
        for g in (2, 3, 5):
            assert any(G.owner(e - 1, g)[0] != G.owner(e, g)[0] for e in edges), (c, g)
        # ... and the same block in consecutive trips under a grid of one
        assert any(G.owner(e - 1, 1)[0] == G.owner(e, 1)[0] and G.owner(e - 1, 1)[1] + 1 == G.owner(e, 1)[1]
                   for e in edges), c
    # every construct byte by byte across the edge 3T, and pairs and "\r\n" across the edges inside the quoted cell
    assert {(c, 3) for c in G.CONSTRUCTS} <= seen and {e for _c, e in seen} >= {1, 2, 3}
    # under a grid of g blocks every block has a tile of the 8, and block 0 makes more than one trip
    for g in (1, 2, 3, 5):
        assert {G.owner(t, g)[0] for t in range(8)} == set(range(g))
        assert max(G.owner(t, g)[1] for t in range(8) if G.owner(t, g)[0] == 0) >= 1


# ------------------------------------------------------------------ the real-size texts
@pytest.fixture(scope='module')
def many():
    return G.many_rows_text()


@pytest.fixture(scope='module')
def long_rows():
    return G.long_rows_text()


def test_many_rows_text(many):
    rows = G.many_rows_count()
    assert rows == 524296 > 2048 * 256 and len(many) == 8454272 > 2048 * 4096
    assert b'\0' not in many and many.decode('utf-8')
    want = G.host_np(many, 7, G.COLS7, rows + 100)
    assert want['n_rows'] == rows and want['consumed'] == len(many)
    assert sorted(set(want['kind'].tolist())) == [0, 1, 2]
    assert len(want['coff']) == 7 * rows + 1 > 2048 * 256 * 7
    # the rows that a max_rows of 1000 leaves beyond the cap
    assert (rows - 1000) * 7 > 3_600_000


def test_long_rows_text(long_rows):
    text = long_rows
    assert len(text) > 9_000_000 and (len(text) + G.T - 1) // G.T > 8 * 256
    assert b'\0' not in text and text.decode('utf-8')
    edges = G.long_rows_edges()
    assert sorted(edges) == list(range(1, 9)) and 8 * G.PASS == 2048 * 4096
    for e, what in edges.items():
        at = e * G.PASS
        if what == 'pair':
            assert text[at - 1:at + 1] == b'""' and text[at - 2:at - 1] != b'"' and text[at + 1:at + 2] != b'"'
        elif what == 'cp4':
            assert text[at - 2:at + 2] == '\U0001F600'.encode('utf-8')
        else:
            assert text[at - 1:at + 1] == b'\r\n'
    assert edges[8] == 'pair' and set(edges.values()) == {'pair', 'cp4', 'crlf'}
    assert G.straddled(text, G.PASS) >= {('pair', 8), ('cp4', 3), ('crlf', 5)}
    for t in (text, text[:1] + text[2:], text[:1] + b'p' + text[1:]):
        want = G.host_np(t, 7, G.COLS7, 1 << 20)
        assert want['n_rows'] == G.LONG_ROWS and want['consumed'] == len(t)
        assert len(want['arena']) - 64 > 2048 * 256 * 16
        lens = np.diff(want['coff'])[0::7]
        head = want['cells'][:1000]
        assert lens.min() > 220_000 and b',' in head and b'\r\n' in head and b'"sit"' in head
    # a byte less or more in the first cell: no construct across a pass edge any more / one byte further
    assert not {c for c, _e in G.straddled(text[:1] + text[2:], G.PASS)} & {'pair', 'crlf'}
    assert ('cp4', 3) in G.straddled(text[:1] + b'p' + text[1:], G.PASS)


# ------------------------------------------------------------------ column layouts
def test_layouts_rule():
    for ncols, cols in G.layouts():
        text = G.layout_text(ncols, cols)
        rows = 3 if ncols > 64 else 5
        got = _rule_equals_host(text, ncols, rows=rows)
        assert not text.endswith(b'\n')
        spans = got[5]
        if ncols == 4096:
            assert all(b - a > G.T for a, b in spans)
        want = R.host_oracle(text, ncols, cols, 1 << 20)
        assert want['kind'][:3] == [1, 2, 0] and want['off'][-1] > 0
    assert [n for n, _c in G.layouts()] == [6, 6, 7, 9, 9, 64, 4096]


# ------------------------------------------------------------------ NA tables
def test_na_tables_rule():
    got = _rule_equals_host(G.na64_text(), 7, G.NA_64, rows=7)
    fl = np.array(got[4]).reshape(7, 7)
    # the 16-byte string is NA, its first 15 bytes and itself plus a byte are not; nor are pandas' own strings
    assert fl[0, 0] & R.F_NA and not fl[0, 1] & R.F_NA and not fl[2, 0] & R.F_NA
    assert fl[3, 0] & R.F_NA and fl[3, 1] & R.F_NA and not any(fl[5, :4] & R.F_NA)
    text = G.empty_na_text()
    got = _rule_equals_host(text, 7, G.NA_EMPTY, rows=len(G.empty_na_rows()))
    assert not any(f & R.F_NA for f in got[4])
    want = R.host_oracle(text, 7, G.COLS7, 1 << 20, G.NA_EMPTY)
    assert want['off'] == G.empty_na_offsets() and b'nan' not in want['arena']
    assert len(want['arena']) == want['off'][-1] + 64 and want['arena'][-64:] == b'\0' * 64
    # the same text under pandas' table: every empty cell is "nan"
    assert R.host_oracle(text, 7, G.COLS7, 1 << 20)['arena'].startswith(b'nannan')


# ------------------------------------------------------------------ dates
def test_dates_table_against_kwcsv_dates():
    cases = G.date_cases()
    assert len(cases) > 350
    kinds = [k for _c, k, _u in cases]
    assert kinds.count(1) > 150 and kinds.count(0) > 100 and kinds.count(2) == len(G.DATE_NA)
    assert min(u for _c, _k, u in cases) < -30_000_000_000 * 10 ** 6 and max(u for _c, _k, u in cases) > 2 ** 47
    by = {c: (k, u) for c, k, u in cases}
    assert by[b'1970-01-01 00:00:00'] == (1, 0) and by[b'1969-12-31T23:59:59'] == (1, -10 ** 6)
    assert [by[b'%d-02-29 13:14:15' % y][0] for y in (1900, 2000, 2100, 2400)] == [0, 1, 0, 1]
    text = G.date_text()
    _rule_equals_host(text, 7, rows=len(cases))
    want = R.host_oracle(text, 7, G.COLS7, 1 << 20)
    bad = [(c, (k, u), (want['kind'][i], want['us'][i])) for i, (c, k, u) in enumerate(cases)
           if (k, u) != (want['kind'][i], want['us'][i])]
    assert not bad, bad[:10]
    assert want['cfl'][7 * G.DATE_QUOTED_ROW + 2] & R.F_QUOTED and want['kind'][G.DATE_QUOTED_ROW] == 1


# ------------------------------------------------------------------ witnesses
def test_witness_table_against_kwcsv_parse():
    cells = G.witness_cells()
    assert 110 <= len(cells) <= 130
    na = R.na_set()
    text = G.witness_text(cells)
    got = _rule_equals_host(text, 7, rows=len(cells))
    fl = np.array(got[4]).reshape(len(cells), 7)
    want = [G.witness_expect(c, na) for c in cells]
    assert (fl[:, 0] & (R.F_NA | R.F_TEXT)).tolist() == want
    assert (fl[:, 4] & (R.F_NA | R.F_TEXT)).tolist() == want[::-1]
    assert 0 in want and R.F_TEXT in want and R.F_NA in want
    assert R.host_oracle(text, 7, G.COLS7, 1 << 20)['witness'] == [1, 0, 1, 0, 1, 0]
    # the cells that are no witness, alone: no column witness in columns 0 and 4
    quiet = [c for c, w in zip(cells, want) if w != R.F_TEXT]
    assert len(quiet) > 30
    assert R.host_oracle(G.witness_text(quiet), 7, G.COLS7, 1 << 20)['witness'] == [0, 0, 1, 0, 0, 0]
