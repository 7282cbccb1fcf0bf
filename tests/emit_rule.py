"""The rule of the per-ticker CSV rows (tests only): what csrc/kwemit.hip renders, restated on the stdlib ``csv``
writer (QUOTE_MINIMAL, "\\n" line ends) with the flag rule in plain Python, and the cases the CPU and GPU tests
share.

A :class:`Case` holds what ``kw_rows_run`` + ``kw_rows_cells`` + ``kw_rows_emit`` take: a hand-made KB table
(tests/rows_rule.py) and records, the chunk's tokenized cells built directly as ``buf`` / ``off`` / ``flags`` (no
tokenizer: NUL, a lone "\\r" and NA cells with arbitrary bytes stand where a case wants them), the six columns,
the per-document time stamps and ``n_rows_use``.  ``rule`` and ``host_emit`` (kwcsv_emit_mt, the way
egress.render_native calls it) both return ``(bytes, line_off, flags, row_doc, row_ti, stamps)`` in output order,
or ``None`` for a NUL cell.
"""
import csv
import io

import numpy as np

from advanced_scrapper_amd import egress
from advanced_scrapper_amd.ingest import Cells, _p, host_threads
from tests import rows_rule as RR

NA = 2
OUT_COL = (0, 3, 4, 5, 6, 7)          # the output column of date_time, title, url, source, source_url, article_text
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NAMES = ['ACME', 'Quote "q"', 'Comma, Inc', 'Back\\slash', 'Café é'] + [f'Name {k}' for k in range(5, 12)]


class Case:
    def __init__(self, cells, cols, t, hits, stamps, n_use=None):
        self.cells, self.cols, self.t, self.hits = cells, np.asarray(cols, dtype=np.int32), t, hits
        self.stamps = np.asarray(stamps, dtype=np.int64)
        self.n_docs = cells.nrows
        self.date_us = np.zeros(self.n_docs, dtype=np.int64)
        self.date_ok = np.ones(self.n_docs, dtype=np.uint8)
        self.n_use = n_use            # None: every row
        self._raw = None

    def raw(self):
        """rows.assemble_json_raw's arrays of the case (libkwrows on the host)."""
        if self._raw is None:
            self._raw = RR.host_raw(self.t, self.hits, self.date_us, self.date_ok)
        return self._raw

    def use(self):
        return len(self.raw()[0]) if self.n_use is None else self.n_use


def table(names):
    """Pattern p is ticker p's only name, always in period."""
    return RR.Tables(list(names), [[(p, 0, I64_MIN, I64_MAX)] for p in range(len(names))], len(names))


def na(b=b''):
    return ('na', b)


def doc(text=b'body text', title=b'A title', date=b'2024-01-02 03:04:05', url=b'http://x.example/a',
        source=b'src', source_url=b'http://s.example'):
    """One article's six cells in the order date_time, title, url, source, source_url, article_text."""
    return [date, title, url, source, source_url, text]


_EXTRA = [b'extra,"\0', b'', b'junk\r\n']


def make_cells(docs, ncols=6):
    """(Cells, cols): ncols = 6 keeps the reference order; ncols = 9 permutes the six columns among three others."""
    cols = list(range(6)) if ncols == 6 else [7, 2, 0, 5, 8, 3]
    assert ncols in (6, 9)
    parts, lens, flags = [], [], []
    for d in docs:
        row = [(_EXTRA[k % 3], 0) for k in range(ncols)]
        for c, v in zip(cols, d):
            row[c] = (v[1], NA) if isinstance(v, tuple) else (v, 0)
        for b, f in row:
            parts.append(b)
            lens.append(len(b))
            flags.append(f)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    buf = np.frombuffer(b''.join(parts) + b'\0', dtype=np.uint8).copy()
    return Cells(buf, off, np.asarray(flags, dtype=np.uint8), len(docs), ncols), cols


def make(docs, recs, stamps=None, ncols=6, names=NAMES, n_use=None, seed=0):
    """A case of ``docs`` (lists of six cells) and records ``(doc, ticker, pos, field)``."""
    cells, cols = make_cells(docs, ncols)
    hits = RR.records([(d, p, pos, f) for d, p, pos, f in recs])
    np.random.default_rng(seed).shuffle(hits)
    if stamps is None:
        stamps = [1700000000 + 60 * d for d in range(len(docs))]
    return Case(cells, cols, table(names), hits, stamps, n_use)


# ------------------------------------------------------------------ the rule
def witness(b: bytes) -> bool:
    """kwcsv_text_witness: no number (digits, sign, '.', exponent, blanks around; inf / infinity) and no bool."""
    t = b.strip(b' \t')
    if not t:
        return True
    low = t.lower()
    if low in (b'true', b'false'):
        return False
    if (low[1:] if low[:1] in (b'+', b'-') else low) in (b'inf', b'infinity'):
        return False
    return any(c not in b'0123456789+-.eE' for c in t)


def _order(raw, n_use):
    return np.argsort(raw[1][:n_use], kind='stable')


def rule(case: Case):
    row_doc, row_ti, jbuf, joff = case.raw()
    n_use = case.use()
    order = _order((row_doc, row_ti), n_use)
    c, off, jb = case.cells, case.cells.off, jbuf.tobytes()
    buf = c.buf.tobytes()
    per_doc = {}
    for d in sorted(set(row_doc[order].tolist())):
        vals, fl = [], 0
        for k, col in enumerate(case.cols.tolist()):
            cell = d * c.ncols + col
            if c.flags[cell] & NA:
                vals.append(b'')
                fl |= 1 << (8 + OUT_COL[k])
                continue
            b = buf[off[cell]:off[cell + 1]]
            if b'\0' in b:
                return None
            if b'\r' in b:
                fl |= 1 << 16
            if witness(b):
                fl |= 1 << OUT_COL[k]
            vals.append(b)
        per_doc[d] = (vals, fl)
    lines, flags = [], []
    for r in order.tolist():
        d = int(row_doc[r])
        vals, fl = per_doc[d]
        j = [jb[joff[2 * r]:joff[2 * r + 1]], jb[joff[2 * r + 1]:joff[2 * r + 2]]]
        if any(b'\0' in x for x in j):
            return None
        fl |= 6 | ((1 << 16) if any(b'\r' in x for x in j) else 0)
        row = [str(int(case.stamps[d])).encode(), vals[0], j[0], j[1]] + vals[1:]
        s = io.StringIO(newline='')
        csv.writer(s, quoting=csv.QUOTE_MINIMAL, lineterminator='\n').writerow([x.decode('latin-1') for x in row])
        lines.append(s.getvalue().encode('latin-1'))
        flags.append(fl)
    line_off = np.zeros(len(lines) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lines], out=line_off[1:])
    rd = row_doc[order].astype(np.int32)
    return (b''.join(lines), line_off, np.asarray(flags, dtype=np.uint32), rd, row_ti[order].astype(np.int32),
            case.stamps[rd].astype(np.int64))


def host_emit(case: Case):
    """kwcsv_emit_mt on the case, called as egress.render_native calls it."""
    row_doc, row_ti, jbuf, joff = case.raw()
    n = case.use()
    order = _order((row_doc, row_ti), n)
    rd = np.ascontiguousarray(row_doc[order], dtype=np.int32)
    rs = np.ascontiguousarray(case.stamps[rd], dtype=np.int64)
    if n == 0:
        return b'', np.zeros(1, np.int64), np.zeros(0, np.uint32), rd, row_ti[order].astype(np.int32), rs
    j3 = np.empty(3 * n, dtype=np.int64)
    j3[0::3], j3[1::3], j3[2::3] = joff[2 * order], joff[2 * order + 1], joff[2 * order + 2]
    c = case.cells
    jb = jbuf if len(jbuf) else np.zeros(1, np.uint8)
    line_off = np.empty(n + 1, dtype=np.int64)
    flags = np.empty(n, dtype=np.uint32)
    L = egress._csv_lib()
    art = np.empty(int(L.kwcsv_emit_art_bytes(_p(c.off), c.ncols, _p(case.cols), _p(rd), n)), dtype=np.uint8)
    out = np.empty(64, dtype=np.uint8)
    for _ in range(2):
        rc = L.kwcsv_emit_mt(_p(c.buf), _p(c.off), _p(c.flags), c.ncols, _p(case.cols), _p(rd), _p(rs), n, _p(jb), _p(j3),
                             _p(out), len(out), _p(line_off), _p(flags), _p(art), host_threads())
        if rc != -1:
            break
        out = np.empty(int(line_off[n]), dtype=np.uint8)
    if rc == -2:
        return None
    assert rc == 0, rc
    return out[:line_off[n]].tobytes(), line_off, flags, rd, row_ti[order].astype(np.int32), rs


def same(got, want) -> bool:
    if got is None or want is None:
        return got is None and want is None
    if bytes(got[0]) != bytes(want[0]):
        return False
    return all(np.asarray(g).dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))


# ------------------------------------------------------------------ cases
def _plain(n, k=0):
    return bytes((97 + (i * 7 + k) % 26) for i in range(n))


def _quoted(n, k=0):
    """n bytes with '"', ',' and '\\n' spread through them (a quote first and last when there is room)."""
    b = bytearray(_plain(n, k))
    for i in range(0, n, 5):
        b[i] = 34
    for i in range(3, n, 11):
        b[i] = 44
    for i in range(7, n, 61):
        b[i] = 10
    if n:
        b[n - 1] = 34
    return bytes(b)


LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]


def length_case(n):
    docs = [doc(text=_plain(n)), doc(title=_plain(n, 1)), doc(text=_quoted(n)), doc(title=_quoted(n, 1)),
            doc(text=_quoted(n, 2), title=_quoted(n, 3))]
    recs = [(d, d % 3, 10 + d, d % 2) for d in range(5)] + [(2, 7, 1, 0), (4, 1, 2, 1)]
    return make(docs, recs)


def big_cell_case():
    """One cell of ~300 KB with quotes, in an article with two rows, beside a small article."""
    big = _quoted(300 * 1024 + 37)
    return make([doc(text=big), doc(), doc(title=big[:70001])], [(0, 3, 1, 0), (0, 8, 2, 1), (1, 3, 4, 0), (2, 0, 1, 1)])


def _at(n, where, c=b'"'):
    b = bytearray(_plain(n))
    for i in where:
        b[i:i + 1] = c
    return bytes(b)


GEOMETRY = {
    'quote_first': _at(40, [0]), 'quote_last': _at(40, [39]), 'quote_every': b'"' * 130, 'quote_only': b'"',
    'quote_63_64': _at(200, [63, 64]), 'quote_255_256': _at(300, [255, 256]), 'commas': b',' * 70, 'newlines': b'\n' * 66,
    'cr_only': b'\r' * 5, 'crlf_inside': b'line one\r\nline two', 'cr_in_text': b'a\rb',
    'utf8_straddle': b'x' * 62 + 'é中\U0001f600'.encode() + b'y' * 10,
    'utf8_straddle_quoted': b'"' + b'x' * 61 + '中é'.encode() + b',z',
}


def geometry_case(name):
    b = GEOMETRY[name]
    docs = [doc(text=b), doc(title=b), doc(url=b, source=b, source_url=b, date=b)]
    return make(docs, [(0, 0, 1, 0), (1, 2, 3, 1), (2, 4, 5, 0), (2, 5, 6, 1)])


def na_case():
    weird = b'x,"y"\0z\r'
    docs = [doc(title=na(b'NA'), source=na(b'null')), doc(text=na(weird), url=na(weird), date=na(weird)),
            [na(b'NaN'), na(b''), na(b'N/A'), na(weird), na(b'nan'), na(b'NULL')], doc()]
    return make(docs, [(0, 0, 1, 0), (1, 1, 2, 1), (1, 2, 2, 0), (2, 3, 3, 0), (3, 4, 4, 1)])


WITNESS = [b'12', b'-1.5e3', b' 7 ', b'TRUE', b'false', b'+inf', b'Infinity', b'1e', b'   ', b' \t ', b'1,2',
           'é'.encode(), b'', b'-Infinity', b'+true', b'inf inity', b'1 2', b'\t-INF\t', b'infinit', b'e', b'tru',
           b'0x10', b'1_000', b'.', b'--', b'nan']


def witness_case():
    docs = []
    for k, w in enumerate(WITNESS):
        cells = doc()
        cells[1 + k % 5] = w                       # title .. article_text in turn
        cells[0] = WITNESS[(k + 3) % len(WITNESS)]   # and the date_time cell
        docs.append(cells)
    return make(docs, [(d, d % 12, d, d % 2) for d in range(len(docs))])


def json_case():
    """{} in either column, keys that need quoting or escaping, a [] value, a long position list."""
    docs = [doc() for _ in range(6)]
    recs = [(0, 0, 5, 0),                                              # title {}
            (1, 0, 5, 1),                                              # text {}
            (2, 1, 1, 0), (2, 1, 9, 1), (2, 2, 3, 0), (2, 3, 4, 1), (2, 4, 7, 0),
            (3, 5, RR.NOPOS, 0), (3, 6, RR.NOPOS, 1), (3, 6, 8, 1)]   # [] and [8]
    recs += [(4, 7, 3 * k + k % 7, k % 2) for k in range(900)]        # a long position list, both fields
    recs += [(5, p, 100 + p, p % 2) for p in range(12)]               # every ticker
    return make(docs, recs)


STAMPS = [0, 7, -1, I64_MIN, I64_MAX, 1700000000, -1700000000, 9, 10, 99, 100, -10]


def stamps_case():
    docs = [doc() for _ in STAMPS]
    return make(docs, [(d, d % 3, d, 0) for d in range(len(docs))] + [(3, 9, 1, 1), (4, 9, 1, 1)], stamps=STAMPS)


def no_rows_case():
    return make([doc(), doc()], [])


def one_row_case():
    return make([doc(), doc(text=_quoted(100))], [(1, 6, 3, 0)])


def many_tickers_case(n=300):
    names = [f'T name {k}' for k in range(n)]
    docs = [doc(), doc(text=_quoted(3000), title=b'One, "two"'), doc()]
    recs = [(1, k, 10 + k, k % 2) for k in range(n)] + [(0, 5, 1, 0), (2, 299, 2, 1)]
    return make(docs, recs, names=names)


def sparse_case(n=2000):
    """2 000 articles of which every 7th has rows; the others hold NUL and quotes that nobody may look at."""
    docs = []
    for d in range(n):
        if d % 7 == 0:
            docs.append(doc(text=_quoted(40 + d % 300, d), title=_plain(5 + d % 40, d), date=b'2024-01-02' if d % 3 else na()))
        else:
            docs.append(doc(text=b'never "read"\0', title=b'\0'))
    recs = [(d, (d // 7 + k) % 12, d + k, k % 2) for d in range(0, n, 7) for k in range(1 + d % 3)]
    return make(docs, recs, ncols=9)


def gaps_case():
    docs = [doc(text=_plain(30, d)) for d in range(8)]
    return make(docs, [(d, t, d, 0) for d in range(8) for t in (1, 5, 9) if (d + t) % 2])


def prefix_case(n_use):
    """Two articles of three rows each: n_use = 0, 1, 4 (inside the second article's rows), 6."""
    docs = [doc(text=b'first'), doc(text=b'second "q"'), doc(text=b'no rows\0')]
    recs = [(0, 7, 1, 0), (0, 2, 2, 1), (0, 10, 3, 0), (1, 10, 1, 0), (1, 0, 2, 1), (1, 7, 3, 0)]
    return make(docs, recs, n_use=n_use)


def columns_case(ncols):
    docs = [doc(text=_quoted(70, d), title=_plain(9, d), url=b'u,' + _plain(d), source=na() if d % 2 else b'S') for d in range(5)]
    return make(docs, [(d, (3 * d) % 12, d, d % 2) for d in range(5)] + [(4, 0, 1, 0)], ncols=ncols)


def nul_case(with_rows: bool):
    """A NUL in the title of article 1, which has a row or has none."""
    docs = [doc(), doc(title=b'nul\0here'), doc()]
    return make(docs, [(0, 1, 1, 0), (2, 2, 2, 1)] + ([(1, 3, 3, 0)] if with_rows else []))


def nul_beyond_prefix_case():
    """The NUL article's rows lie beyond n_rows_use: it has no rendered row."""
    docs = [doc(), doc(title=b'nul\0here')]
    return make(docs, [(0, 1, 1, 0), (1, 3, 3, 0)], n_use=1)


def large_case(seed=11, n=700):
    rng = np.random.default_rng(seed)
    docs = [doc(text=_quoted(int(rng.integers(200, 4000)), d), title=_plain(int(rng.integers(0, 90)), d)) for d in range(n)]
    recs = [(d, int(t), int(rng.integers(0, 5000)), int(rng.integers(0, 2))) for d in range(n)
            for t in rng.choice(12, size=int(rng.integers(0, 4)), replace=False)]
    return make(docs, recs)


_POOL = ([_plain(n) for n in (0, 1, 5, 63, 64, 65, 200)] + [_quoted(n) for n in (1, 2, 16, 63, 64, 65, 130, 700)] +
         list(GEOMETRY.values()) + WITNESS)


def fuzz_case(seed):
    """A small chunk (<= 40 articles, <= 12 tickers) drawing from everything above."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 41))
    docs = []
    for _d in range(n):
        cells = []
        for _c in range(6):
            b = _POOL[int(rng.integers(len(_POOL)))]
            if rng.random() < 0.01:
                b = b + b'\0'
            cells.append(na(b + (b'\0"' if rng.random() < 0.3 else b'')) if rng.random() < 0.15 else b)
        docs.append(cells)
    n_rec = int(rng.integers(0, 4 * n + 1))
    recs = [(int(rng.integers(n)), int(rng.integers(12)), RR.NOPOS if rng.random() < 0.1 else int(rng.integers(10 ** int(rng.integers(1, 10)))),
             int(rng.integers(2))) for _ in range(n_rec)]
    pool = STAMPS + [int(x) for x in rng.integers(-10 ** 12, 10 ** 12, 4)]
    stamps = [pool[int(rng.integers(len(pool)))] for _ in range(n)]
    case = make(docs, recs, stamps=stamps, ncols=6 if rng.random() < 0.5 else 9, seed=seed)
    n_rows = len(case.raw()[0])
    if rng.random() < 0.5:
        case.n_use = int(rng.integers(0, n_rows + 1))
    return case


def cases():
    """name -> builder of every fixed case (the fuzz cases come from :func:`fuzz_case`)."""
    out = {f'len_{n}': (lambda n=n: length_case(n)) for n in LENGTHS}
    out['big_cell'] = big_cell_case
    out.update({f'geo_{k}': (lambda k=k: geometry_case(k)) for k in GEOMETRY})
    out.update(na_cells=na_case, witness=witness_case, json=json_case, stamps=stamps_case, no_rows=no_rows_case,
               one_row=one_row_case, many_tickers=many_tickers_case, sparse=sparse_case, gaps=gaps_case,
               large=large_case, nul_rows=lambda: nul_case(True), nul_no_rows=lambda: nul_case(False),
               nul_beyond_prefix=nul_beyond_prefix_case)
    out.update({f'prefix_{k}': (lambda k=k: prefix_case(k)) for k in (0, 1, 4, 6)})
    out.update({f'cols_{k}': (lambda k=k: columns_case(k)) for k in (6, 9)})
    return out
