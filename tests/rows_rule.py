"""The staged rule of the per-ticker match cells (tests only): what csrc/kwrows.hip computes, stage by stage, in
numpy -- order, groups, entries, rows, byte lengths, fill -- and the cases the CPU and GPU tests share.

``assemble`` takes what ``kw_rows_run`` takes (records in any order, per-document date_us / date_ok, the
occurrence CSR, invalid_rx, the json.dumps keys) and returns rows.assemble_json_raw's four arrays, or ``None``
for the verdict KW_ROWS_INVALID_REGEX.  ``host_raw`` is rows.assemble_json_raw (libkwrows) on the same inputs:
the reference every comparison uses.
"""
import json

import numpy as np

from advanced_scrapper_amd import _native
from advanced_scrapper_amd import rows as R

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NOPOS = _native.KW_NOPOS


# ------------------------------------------------------------------ inputs
class Tables:
    """A KB's occurrence tables as rows._kb_tables makes them, from plain lists: ``names[p]`` and
    ``occ[p] = [(ticker, rank, lo, hi), ...]`` in table order."""

    def __init__(self, names, occ, n_tickers, invalid=()):
        flat = [o for lst in occ for o in lst]
        self.off = np.zeros(len(occ) + 1, dtype=np.int64)
        self.off[1:] = np.cumsum([len(lst) for lst in occ])
        self.ti = np.array([o[0] for o in flat], dtype=np.int32)
        self.rank = np.array([o[1] for o in flat], dtype=np.int32)
        self.lo = np.array([o[2] for o in flat], dtype=np.int64)
        self.hi = np.array([o[3] for o in flat], dtype=np.int64)
        keys = [json.dumps(n).encode('ascii') for n in names]
        self.key_off = np.zeros(len(keys) + 1, dtype=np.int64)
        self.key_off[1:] = np.cumsum([len(k) for k in keys])
        self.key_buf = np.frombuffer(b''.join(keys) or b'\0', dtype=np.uint8).copy()
        self.invalid = np.zeros(len(names), dtype=np.uint8)
        self.invalid[list(invalid)] = 1
        self.n_tickers = n_tickers
        self.names = list(names)

    def tuple(self):
        return (self.off, self.ti, self.rank, self.lo, self.hi, self.invalid, self.key_buf, self.key_off)


class _KB:
    """What rows.assemble_json_raw reads of a CompiledKB."""

    def __init__(self, t: Tables):
        self._rows_tables = t.tuple()
        self.tickers = [f'T{i}' for i in range(t.n_tickers)]


class _Dates:
    def __init__(self, date_us, date_ok):
        self.us, self.ok = date_us, date_ok

    def __len__(self):
        return len(self.us)

    def epoch_us_arrays(self):
        return self.us, self.ok


def records(rows) -> np.ndarray:
    """[(doc, pattern, pos, field), ...] -> HIT_DTYPE records."""
    a = np.zeros(len(rows), dtype=_native.HIT_DTYPE)
    if len(rows):
        r = np.asarray(rows, dtype=np.uint64)
        a['doc'], a['pattern'], a['pos'], a['field'] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return a


def host_raw(t: Tables, hits, date_us, date_ok):
    """rows.assemble_json_raw (kwrows_assemble_mt) on these inputs."""
    return R.assemble_json_raw(_KB(t), hits, _Dates(np.asarray(date_us, np.int64), np.asarray(date_ok, np.uint8)))


def same(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def cells_equal_in_order(got, want) -> bool:
    """Per document {ticker: {'text': {...}, 'title': {...}}}: equal, with every dict in the same key order."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if g != w or list(g) != list(w):
            return False
        for tk in w:
            if list(g[tk]['text']) != list(w[tk]['text']) or list(g[tk]['title']) != list(w[tk]['title']):
                return False
    return True


def raw_cells(raw, tickers, n_docs):
    """rows.assemble_json_raw's arrays as per-document {ticker: {'text': ..., 'title': ...}} (json.loads)."""
    row_doc, row_ti, buf, off = raw
    text = buf.tobytes().decode('ascii')
    out = [{} for _ in range(n_docs)]
    for r, (d, ti) in enumerate(zip(row_doc.tolist(), row_ti.tolist())):
        out[d][tickers[ti]] = {'text': json.loads(text[off[2 * r]:off[2 * r + 1]]),
                               'title': json.loads(text[off[2 * r + 1]:off[2 * r + 2]])}
    return out


# ------------------------------------------------------------------ the stages
def stage_order(hits, date_ok, n_docs):
    """Records of documents that have a date, by (doc, field, pattern, pos)."""
    doc = hits['doc'].astype(np.int64)
    keep = doc < n_docs
    keep[keep] = date_ok[doc[keep]] != 0
    h = hits[keep]
    return h[np.lexsort((h['pos'], h['pattern'], h['field'], h['doc']))]


def stage_entries(h, date_us, t: Tables):
    """Group heads -> entries (doc, ticker, field, rank, pattern, first record, last record) in group order then
    table order, and whether an in-period match is an invalid regex."""
    n = len(h)
    if n == 0:
        return np.zeros((0, 7), dtype=np.int64), False
    key = np.stack([h['doc'], h['field'], h['pattern']], axis=1).astype(np.int64)
    head = np.ones(n, dtype=bool)
    head[1:] = (key[1:] != key[:-1]).any(axis=1)
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    ent, invalid = [], False
    for g, ge in zip(starts.tolist(), ends.tolist()):
        d, f, p = key[g].tolist()
        a = int(date_us[d])
        seen = set()
        for o in range(int(t.off[p]), int(t.off[p + 1])):
            ti = int(t.ti[o])
            if ti in seen or not (int(t.lo[o]) <= a <= int(t.hi[o])):
                continue
            seen.add(ti)
            invalid |= bool(t.invalid[p])
            ent.append((d, ti, f, int(t.rank[o]), p, g, ge))
    return np.array(ent, dtype=np.int64).reshape(-1, 7), invalid


def stage_entry_order(ent):
    """Entries by (doc, ticker, field, rank): unique keys."""
    return ent[np.lexsort((ent[:, 3], ent[:, 2], ent[:, 1], ent[:, 0]))]


def _digits(v):
    return np.searchsorted(np.array([10 ** k for k in range(1, 10)], dtype=np.uint64), v, side='right') + 1


def stage_pieces(ent, h, t: Tables):
    """Per ordered entry: row head, row end, its prefix and suffix, and its exact byte length."""
    m = len(ent)
    row = ent[:, :2]
    head = np.ones(m, dtype=bool)
    head[1:] = (row[1:] != row[:-1]).any(axis=1)
    last = np.append(head[1:], True)
    title = ent[:, 2] != 0
    prev_title = np.append(False, title[:-1]) & ~head
    prefix = np.where(head, np.where(title, '{}{', '{'), np.where(title & ~prev_title, '}{', ', '))
    suffix = np.where(last, np.where(title, '}', '}{}'), '')
    pos = h['pos']
    length = np.zeros(m, dtype=np.int64)
    for j in range(m):
        p, g, ge = ent[j, 4:7].tolist()
        q = pos[g:ge]
        q = q[q != NOPOS]
        body = int(_digits(q.astype(np.uint64)).sum()) + 2 * max(len(q) - 1, 0)
        length[j] = len(prefix[j]) + int(t.key_off[p + 1] - t.key_off[p]) + 4 + body + len(suffix[j])
    return head, last, title, prefix, suffix, length


def stage_fill(ent, h, t: Tables, pieces):
    head, last, title, prefix, suffix, length = pieces
    m = len(ent)
    start = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(length, out=start[1:])
    row_of = np.cumsum(head) - 1
    n_rows = int(head.sum())
    out = bytearray(int(start[-1]))
    off = np.zeros(2 * n_rows + 1, dtype=np.int64)
    keys = t.key_buf.tobytes()
    for j in range(m):
        p, g, ge = ent[j, 4:7].tolist()
        q = [str(int(v)) for v in h['pos'][g:ge] if v != NOPOS]
        piece = (prefix[j].encode() + keys[t.key_off[p]:t.key_off[p + 1]] + b': [' + ', '.join(q).encode() + b']' +
                 suffix[j].encode())
        assert len(piece) == length[j], (j, piece, length[j])      # the size pass is exact
        out[start[j]:start[j + 1]] = piece
        r = int(row_of[j])
        if head[j]:
            off[2 * r] = start[j]
        if title[j] and (head[j] or not title[j - 1]):
            off[2 * r + 1] = start[j] + len(prefix[j]) - 1
        if last[j] and not title[j]:
            off[2 * r + 1] = start[j + 1] - 2
    off[2 * n_rows] = start[-1]
    return (ent[head, 0].astype(np.int32), ent[head, 1].astype(np.int32), np.frombuffer(bytes(out), dtype=np.uint8),
            off)


def assemble(t: Tables, hits, date_us, date_ok):
    date_us, date_ok = np.asarray(date_us, np.int64), np.asarray(date_ok, np.uint8)
    n_docs = len(date_us)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(1, np.int64))
    if len(hits) == 0 or n_docs == 0:
        return empty
    h = stage_order(hits, date_ok, n_docs)
    ent, invalid = stage_entries(h, date_us, t)
    if invalid:
        return None
    if len(ent) == 0:
        return empty
    ent = stage_entry_order(ent)
    return stage_fill(ent, h, t, stage_pieces(ent, h, t))


# ------------------------------------------------------------------ cases
POSITIONS = [5, 12, 123, 1234, 12345, 123456, 1234567, 8388607, 12345678, 123456789, 1234567890, 4294967294]


def hand_case(seed=1):
    """The issue's hand-made records (shuffled): documents without records, without a date, beyond n_docs; dates
    on both bounds; open bounds; a first occurrence out of period and a second in; text-only and title-only
    tickers; KW_NOPOS alone and beside positions; positions of 1..10 digits; escaped and long keys."""
    long_name = ''.join(chr(0x4E00 + k) for k in range(64))           # 64 non-ASCII code points: a 386-byte key
    names = ['ACME', 'Ünï "q" \\z', 'Beta Corp', long_name, 'bad(regex', 'Text Only']
    assert len(json.dumps(long_name)) == 386
    occ = [
        [(0, 0, 100, 200)],
        [(1, 0, I64_MIN, I64_MAX)],
        [(2, 0, 1000, 2000), (0, 1, I64_MIN, 150), (2, 3, I64_MIN, I64_MAX), (2, 4, I64_MIN, I64_MAX)],
        [(3, 0, I64_MIN, 500)],
        [(4, 0, 5000, 6000)],
        [(5, 0, 0, I64_MAX)],
    ]
    t = Tables(names, occ, 6, invalid=[4])
    date_us = [100, 150, 200, 150, 150, 201]
    date_ok = [1, 1, 1, 0, 1, 1]
    rows = [(0, 0, q, 0) for q in POSITIONS]
    rows += [(0, 0, NOPOS, 1), (0, 1, NOPOS, 0), (0, 1, 7, 0), (0, 1, 3, 0)]
    rows += [(2, 0, 0, 1), (2, 2, 4, 0), (2, 3, 9, 1)]
    rows += [(3, 0, 1, 0), (3, 5, 2, 0)]
    rows += [(4, 2, 8, 0), (4, 2, 2, 1), (4, 5, 6, 0), (4, 1, 1, 1), (4, 3, NOPOS, 0), (4, 3, NOPOS, 0)]
    rows += [(5, 0, 3, 0), (5, 2, 1, 0), (5, 4, 3, 0)]
    rows += [(6, 0, 1, 0), (9, 1, 2, 1), (4294967295, 0, 1, 0)]
    hits = records(rows)
    np.random.default_rng(seed).shuffle(hits)
    return t, hits, date_us, date_ok


def invalid_case(in_period: bool):
    """One record of a name whose regex does not compile, in or out of its ticker's period."""
    t = hand_case()[0]
    return t, records([(0, 4, NOPOS, 0), (0, 0, 1, 0)]), [5500 if in_period else 150], [1]


def one_name_case(m: int):
    """A document with ``m`` records of one name (positions descending, duplicates of none) between two small
    documents."""
    t = Tables(['Solo', 'Other'], [[(0, 0, I64_MIN, I64_MAX)], [(1, 0, I64_MIN, I64_MAX), (0, 1, I64_MIN, I64_MAX)]], 2)
    rows = [(0, 1, 3, 0), (0, 0, 1, 1)] + [(1, 0, 7 * (m - k), 0) for k in range(m)] + [(2, 1, 9, 1), (2, 0, 4, 0)]
    return t, records(rows), [0, 0, 0], [1, 1, 1]


def many_tickers_case(n: int = 300):
    """One document matching ``n`` distinct tickers (more entries than a wave holds), through n names of one
    ticker each and one name that all tickers share."""
    names = [f'Name {k}' for k in range(n)] + ['Shared']
    occ = [[(k, 0, I64_MIN, I64_MAX)] for k in range(n)] + [[(k, 1, I64_MIN, I64_MAX) for k in reversed(range(n))]]
    t = Tables(names, occ, n)
    rows = [(1, k, 10 + k, k % 2) for k in range(n)] + [(1, n, 5, 1), (1, n, NOPOS, 0), (0, 3, 1, 0), (2, 4, 2, 1)]
    hits = records(rows)
    np.random.default_rng(2).shuffle(hits)
    return t, hits, [0, 0, 0], [1, 1, 1]


def random_case(seed: int, n_rec: int = 20000, n_docs: int = 2000, n_pat: int = 300, n_tick: int = 80):
    """Seeded random occurrence table (repeated tickers per name, open and closed bounds) and records (both
    fields, KW_NOPOS, repeated records, documents without a date and beyond n_docs)."""
    rng = np.random.default_rng(seed)
    next_rank = [0] * n_tick
    occ = []
    for _p in range(n_pat):
        lst = []
        for _ in range(int(rng.integers(1, 7))):
            ti = int(rng.integers(n_tick))
            lo = I64_MIN if rng.random() < 0.3 else int(rng.integers(0, 60))
            hi = I64_MAX if rng.random() < 0.3 else int(rng.integers(40, 100))
            lst.append((ti, next_rank[ti], lo, hi))
            next_rank[ti] += 1
        occ.append(lst)
    for ti in range(n_tick):                                  # ranks in no particular order inside a ticker
        perm = rng.permutation(next_rank[ti])
        for lst in occ:
            for k, o in enumerate(lst):
                if o[0] == ti:
                    lst[k] = (o[0], int(perm[o[1]]), o[2], o[3])
    names = [f'N{p} "é\\' if p % 7 == 0 else f'name {p}' for p in range(n_pat)]
    t = Tables(names, occ, n_tick)
    hits = np.zeros(n_rec, dtype=_native.HIT_DTYPE)
    hits['doc'] = rng.integers(0, n_docs + n_docs // 50 + 1, n_rec)
    hits['pattern'] = rng.integers(0, n_pat, n_rec)
    hits['field'] = rng.integers(0, 2, n_rec)
    hits['pos'] = np.where(rng.random(n_rec) < 0.15, NOPOS, rng.integers(0, 3000, n_rec) ** 3 % (1 << 32))
    date_us = rng.integers(0, 100, n_docs)
    date_ok = (rng.random(n_docs) < 0.95).astype(np.uint8)
    return t, hits, date_us, date_ok
