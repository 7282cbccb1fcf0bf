"""The byte-geometry sweep of the URL dedup (csrc/dedup.hip): generators, no GPU, no product imports.

The dedup kernels never store a normalised URL: the transform (``transform_row_lds`` from a wave's LDS stage,
``transform_row`` from global memory), the pair compare (``NormRow`` over ``GRow``), the recheck and the host's exact
pass (``RowGen``) and the dense copy (``NormRow`` over ``LRow``, two lanes a row) each regenerate the normalised
words from the raw bytes and a 16-byte plan, under their own alignments.  The families below walk what those
pieces depend on: the row start modulo 4 and 16, the cut ``j``, ``E`` and ``G`` modulo 8, the length modulo 128,
the stage limits of the transform and of the copy, the row counts around a claim and a scan tile.

Every expected value comes from ``oracle/dedup_oracle.py`` (``url_transform``, ``keep_first``, ``dedup_rows``).
``route()`` restates the kernel's route choice in plain Python; it is used for the census of
tests/test_dedup_geometry_cases.py (which holds it to the oracle), never for an expected output.

The rows are ``str`` (a lone surrogate is encoded with ``surrogatepass``, as the product's ``pack_urls`` does);
``pack`` builds the arena and the offsets itself, with exactly the 32 readable bytes past the end that
include/kwdedup.h promises, filled with bytes that would change a result if a read past a row's end leaked into it.
"""
from __future__ import annotations

import functools
import random
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import dedup_oracle as dd

# the kernels' geometry as the generators assume it: kw_dedup_geometry() in the library's order (the CPU test
# asserts the two are equal, so a retune fails there and not silently here)
GEOMETRY_NAMES = ('STAGE_BYTES', 'TCLAIM', 'SCAN_TILE', 'PAIR_LANES', 'PAIR_UNROLL', 'CPS_ROWS', 'CPS_IN', 'CPS_OUT',
                  'CP_STAGE', 'COLLIDE_CAP')
GEOMETRY = dict(zip(GEOMETRY_NAMES, (8192, 8, 1024, 4, 4, 32, 6144, 4096, 8192, 65536)))

PAD_BYTES = 32
PAD = (b"lhtml:80http:news/%'" + b'\xff' * PAD_BYTES)[:PAD_BYTES]

NO_HTML, KEPT, FILTERED, DUPLICATE = 0, 1, 2, 3   # KW_URL_* (include/kwdedup.h)


def enc(s: str) -> bytes:
    return s.encode('utf-8', 'surrogatepass')


# ------------------------------------------------------------------ packing and the oracle's side
def pack(rows: Sequence[str], pad: bytes = PAD) -> Tuple[np.ndarray, np.ndarray]:
    """(arena, offsets): the rows' UTF-8 bytes back to back, then `pad`; int64 offsets [n + 1]."""
    e = [enc(r) for r in rows]
    off = np.zeros(len(e) + 1, dtype=np.int64)
    if e:
        off[1:] = np.cumsum([len(x) for x in e])
    arena = np.frombuffer(b''.join(e) + pad, dtype=np.uint8).copy()
    assert len(arena) == int(off[-1]) + len(pad)
    return arena, off


def codes_from_keys(rows: Sequence[str], keys: Sequence[Optional[str]], kept: Sequence[int], normalize: bool = True):
    """The KW_URL_* code of every row from the oracle's keys and kept rows (uint8)."""
    ks = set(kept)
    return np.array([KEPT if i in ks else
                     (DUPLICATE if keys[i] is not None else
                      (NO_HTML if not normalize or dd._HTML.search(u) is None else FILTERED))
                     for i, u in enumerate(rows)], dtype=np.uint8)


def oracle_codes(rows: Sequence[str], normalize: bool = True) -> np.ndarray:
    keys = [dd.url_transform(u) for u in rows] if normalize else list(rows)
    return codes_from_keys(rows, keys, dd.keep_first(keys), normalize)


Expected = namedtuple('Expected', 'codes kept_rows kept_off kept_bytes counts')


def expected(rows: Sequence[str], normalize: bool = True) -> Expected:
    """What a run over `rows` must give: per-row codes, the kept rows' indices, dense offsets and bytes (all from
    the oracle), the four counts."""
    if normalize:
        keys = [dd.url_transform(u) for u in rows]
        kept, new = dd.dedup_rows(rows)
    else:
        keys = list(rows)
        kept = dd.keep_first(keys)
        new = [rows[i] for i in kept]
    codes = codes_from_keys(rows, keys, kept, normalize)
    nb = [enc(s) for s in new]
    off = np.zeros(len(nb) + 1, dtype=np.int64)
    if nb:
        off[1:] = np.cumsum([len(x) for x in nb])
    counts = [int(x) for x in np.bincount(codes, minlength=4)[:4]]
    return Expected(codes, np.asarray(kept, dtype=np.int64), off, b''.join(nb), counts)


# ------------------------------------------------------------------ the kernel's route choice, restated
Route = namedtuple('Route', 'route cut E G ec ins filtered norm')
FAST_ROUTES = ('fast', 'ins', 'gap', 'ins_gap')
ROUTES = ('no_html',) + FAST_ROUTES + ('slow',)
_INF = 1 << 62
_M64 = (1 << 64) - 1
_DOTHTML = 0x6C6D74682E


def _slow_bytes(u: bytes, j: int) -> Tuple[bytes, bool]:
    """slow_row: the byte-serial rewrite of u[0, j) (a 3-byte window drops ':80', then a 5-byte window turns
    'http:' into 'https:'), ".html", and the 6-byte filter window over what is emitted."""
    out = bytearray()
    P: List[int] = []
    Q: List[int] = []

    def h_push(c):
        Q.append(c)
        if len(Q) == 5:
            if bytes(Q) == b'http:':
                out.extend(b'https:')
                Q.clear()
            else:
                out.append(Q.pop(0))

    for c in u[:j]:
        P.append(c)
        if len(P) == 3:
            if bytes(P) == b':80':
                P.clear()
            else:
                h_push(P.pop(0))
    while P:
        h_push(P.pop(0))
    out.extend(Q)
    out.extend(b'.html')
    bad = any(bytes(out[k:k + 6]) in (b'news/%', b"news/'") for k in range(len(out) - 5))
    return bytes(out), bad


def _fast_bytes(u: bytes, j: int, ins: int, G: int, E: int) -> bytes:
    """FastWords::word for x = 0, 8, ... below E + 5, from the row's bytes followed by the hostile pad."""
    buf = u + PAD

    def ld64(p):
        return int.from_bytes(buf[p:p + 8], 'little')

    def body(x):
        if ins and x == 0:
            w = (0x7370747468 | (ld64(4) << 40)) & _M64
        else:
            w = ld64(x - ins + (3 if x >= G else 0))
        if x < G < x + 8:
            k = (G - x) * 8
            w = ((w & ((1 << k) - 1)) | (ld64(G - ins + 3) << k)) & _M64
        return w

    def splice(w, x):
        if E < x + 8:
            if E >= x:
                sh = (E - x) * 8
                w = ((w & ((1 << sh) - 1)) | (_DOTHTML << sh)) & _M64
            else:
                d = x - E
                w = _DOTHTML >> (8 * d) if d < 8 else 0
        return w

    n = E + 5
    out = b''.join(splice(body(x) if x < E else 0, x).to_bytes(8, 'little') for x in range(0, n, 8))
    assert not any(out[n:])          # zeros past the length
    return out[:n]


def route(u: bytes) -> Route:
    """transform_row (csrc/dedup.hip) on one row's bytes: the cut, the extra ':' bytes, the route, the plan."""
    L = len(u)
    j = -1
    for q in range(1, L - 3):
        if u[q:q + 4] == b'html' and u[q - 1] != 0x0A:
            s = q - 1
            if u[s] >= 0x80:
                while s > 0 and (u[s] & 0xC0) == 0x80 and q - s < 4:
                    s -= 1
            j = s
            break
    if j < 0:
        return Route('no_html', -1, None, None, None, 0, False, None)
    scheme_http, excl = False, -1
    if L >= 5 and u[:4] == b'http':
        if u[4] == 0x3A and not (L >= 7 and u[4:7] == b':80'):
            scheme_http, excl = True, 4
        if L >= 6 and u[4:6] == b's:' and not (L >= 8 and u[5:8] == b':80'):
            excl = 5
    colons = [p for p in range(L) if u[p] == 0x3A and p != excl]
    ec = colons[0] if colons else _INF
    ec2 = colons[1] if len(colons) > 1 else _INF
    kf = min((p for p in range(5, L) if u[p] in (0x25, 0x27) and u[p - 5:p] == b'news/'), default=_INF)
    gap = ec < j
    if gap and not (ec2 >= j and ec > 5 and ec + 3 <= j and u[ec:ec + 3] == b':80'):
        norm, bad = _slow_bytes(u, j)
        return Route('slow', j, None, None, ec, 0, bad, norm)
    ins = 1 if scheme_http and j > 4 else 0
    G = ec + ins if gap else _INF
    E = j + ins - (3 if gap else 0)
    norm = _fast_bytes(u, j, ins, G, E)
    jn = gap and any(norm[x:x + 6] in (b'news/%', b"news/'") for x in range(G - 5, G))
    name = ('ins_gap' if ins else 'gap') if gap else ('ins' if ins else 'fast')
    return Route(name, j, E, G if gap else None, ec if gap else None, ins, kf < j or jn, norm)


# ------------------------------------------------------------------ placing rows at chosen starts
class Builder:
    """Rows back to back, with filler rows that steer the next row's start.  A filler is itself a row with no
    cut that ends in "htm" (or the tail of it): when the next row starts with 'l' the bytes across the row
    boundary spell "html", which must not count for either row."""

    def __init__(self):
        self.rows: List[str] = []
        self.pos = 0
        self.marks: List[int] = []     # indices of the rows added through add / add_at (not the fillers)

    def filler(self, n: int) -> str:
        return ('f' * n + 'htm')[-n:] if n else ''

    def add(self, row: str, mark: bool = True) -> int:
        if mark:
            self.marks.append(len(self.rows))
        self.rows.append(row)
        self.pos += len(enc(row))
        return len(self.rows) - 1

    def add_at(self, row: str, start: int, mod: int = 16) -> int:
        """`row` at a start that is `start` modulo `mod`, behind one filler row (of 0..mod-1 bytes)."""
        self.add(self.filler((start - self.pos) % mod), mark=False)
        assert self.pos % mod == start % mod
        return self.add(row)

    def starts(self) -> List[int]:
        """The start offset of every row."""
        out, p = [], 0
        for r in self.rows:
            out.append(p)
            p += len(enc(r))
        return out


def marked(b: Builder) -> List[Tuple[str, int]]:
    """(row, start offset) of the builder's own rows (fillers left out)."""
    st = b.starts()
    return [(b.rows[i], st[i]) for i in b.marks]


# ------------------------------------------------------------------ family: align_cut
@functools.lru_cache(maxsize=None)
def align_cut() -> Builder:
    """scheme + 'x' * k + 'html' + tail at every row start modulo 16: the cut j and E at every residue modulo 8
    (E >> 3 from 0 to 3), without and with the 's' insertion.  A quarter of the scheme-less rows start with 'l'
    behind a filler that ends in "htm"."""
    b = Builder()
    for scheme in ('', 'http://', 'https://'):
        for k in range(25):
            for tail in ('', '?q'):
                for start in range(16):
                    body = 'x' * k
                    if scheme == '' and k >= 1 and start % 4 == 1:
                        body = 'l' + body[1:]
                    b.add_at(scheme + body + 'html' + tail, start)
    return b


# ------------------------------------------------------------------ family: cut_rule
@functools.lru_cache(maxsize=None)
def cut_rule() -> Builder:
    b = Builder()
    rows: List[str] = []
    rows += ['html' + 'x' * a + 'xhtml' for a in range(9)]            # "html" at q = 0, then a valid one
    rows += ['\nhtml', 'a\nhtml', '\nhtml\nhtml']                      # no valid one at all
    for o in range(8):                                                 # the pair slid through an 8-byte step
        for d in (0, 1, 2, 3, 4, 7):
            rows.append('p' * o + '\nhtml' + 'y' * d + 'xhtml')        # invalid first, valid later
            rows.append('p' * o + 'xhtml' + 'y' * d + '\nhtml')        # valid first
        rows.append('p' * o + 'ahtmlbhtml')                            # two valid candidates, 5 apart
        rows.append('p' * o + 'ahtmlhtml')                             # ... 4 apart
        rows.append('p' * o + 'chtml\nhtmldhtml')
    rows += ['x' * k + 'htm' for k in range(12)]
    for cp in ('a', 'é', '中', '😀', '\ud800'):                       # 1, 2, 3, 4 bytes and a lone surrogate
        rows.append(cp + 'html')
        rows += ['https://h/' + 'w' * p + cp + 'html?' for p in range(4)]
        rows += ['w' * p + cp + cp + 'html' for p in range(4)]
        rows.append('\n' + cp + 'html')
        rows.append(cp + '\nhtml' + cp + 'html')
    rows += ['news/%html', 'https://a/news/%html', "https://a/news/'html", 'https://a/xnews/%html.html']
    for r in rows:
        for start in (0, 5, 10, 15):                                   # every start modulo 4
            b.add_at(r, start)
    # 'x' * k + 'html' cut short at every length 0..15; what is cut off starts the next row, so the bytes across
    # the boundary spell the whole of it ("html" ending exactly at L when nothing is cut off)
    for k in range(12):
        s = 'x' * k + 'html' + 'zzzzzzzzzzzzzzzz'
        for L in range(16):
            b.add_at(s[:L], (k + 3 * L) % 16)
            b.add(s[L:L + 6])
    return b


# ------------------------------------------------------------------ family: gap
GAP_BOUNDARY = ('abcde:80/x.html', 'abcdef:80/x.html', 'https://h:8html', 'https://h:80html', 'https://h:80xhtml',
                'http://h:8html', 'http://h:80html', 'http://h:80xhtml',
                'https://h:80/x.html:', 'https://h:80/x:html', 'https://h:80/:x.html', 'https://h:80/x.html:80',
                'http://h:80/x:html', 'http://h:80/:x.html',
                'http:80/x.html', 'https:80/x.html', 'https::80/x.html', 'http::80/x.html', 'http:80html',
                'https:80html', 'http:html', 'https:html', 'http:xhtml', 'https:xhtml')


@functools.lru_cache(maxsize=None)
def gap() -> Builder:
    """One ':80' after the scheme: G at every residue modulo 8, E from G (ec + 3 == j) to the next word, with and
    without the 's' insertion, each at four starts (all residues modulo 4; all 16 starts over the family)."""
    b = Builder()
    idx = 0
    for scheme in ('https://h', 'http://h'):
        for a in range(8):
            for c in range(10):
                row = scheme + 'y' * a + ':80' + 'z' * c + '.html'
                for i in range(4):
                    b.add_at(row, (idx + 5 * i) % 16)
                idx += 1
    for row in GAP_BOUNDARY:
        for i in range(4):
            b.add_at(row, (idx + 5 * i) % 16)
        idx += 1
    return b


# ------------------------------------------------------------------ family: filter
FILTER_SPLITS = tuple('news/%'[:i] + ':80' + 'news/%'[i:] for i in range(1, 6))   # 'n:80ews/%' .. 'news/:80%'


@functools.lru_cache(maxsize=None)
def filter_rows() -> Builder:
    b = Builder()
    rows: List[str] = []
    for c in ('%', "'"):
        for o in range(8):                                             # the '%' at every position modulo 8
            rows.append('https://a/' + 'p' * o + 'news/' + c + 'q.html')
            rows.append('http://a/' + 'p' * o + 'news/' + c + 'q.html')
            rows.append('https://a/' + 'p' * o + 'news/' + c + 'html')   # ending at j: the cut code point, kept
            rows.append('https://a/' + 'p' * o + 'news/' + c + 'xhtml')  # ending at j - 1: filtered
            rows.append('https://a/' + 'p' * o + 'NEWS/' + c + 'q.html')
            rows.append('https://a/' + 'p' * o + 'news/x' + c + 'q.html')
        rows += ['news/' + c + 'a.html', 'news/' + c + 'html', 'news/' + c + 'xhtml', 'xnews/' + c + '.html',
                 'ews/' + c + 'a.html']
        for sp in FILTER_SPLITS:                                       # across the gap, with and without the insertion
            sp = sp.replace('%', c)
            rows += ['https://hh/' + sp + 'a.html', 'http://hh/' + sp + 'a.html', 'https://hh/' + sp + 'html',
                     'http://hh/' + sp + 'xhtml']
        # near the gap without spelling it: kept
        rows += ['https://hh/new:80s/x' + c + 'a.html', 'https://hh/news:80x/' + c + 'a.html',
                 'http://hh/news/:80x' + c + 'a.html']
        # on the byte-serial route
        rows += ['http://a:80/b:80/news/' + c + 'x.html', 'http://a:80/b:80/news/' + c + 'html',
                 'http://a:80/ne:80ws/' + c + 'x.html']
    for r in rows:
        for start in (0, 5, 10, 15):
            b.add_at(r, start)
    return b


# ------------------------------------------------------------------ family: slow
SLOW_BASE = ('http://x:80/a:80/b.html', 'htt:80p://x.com/a.html', 'https://h/:8:800.html', 'x:80:80.html',
             'http:http:a.html', 'http://x/http:y.html', 'ht:80tp:a.html', ':8:800.html',
             'https://x:81/a.html', 'abcde:80/x.html')


@functools.lru_cache(maxsize=None)
def slow() -> Builder:
    """The byte-serial route's strings at every start modulo 8; the normalised lengths cover every residue
    modulo 8 (Emit::finish's partial word); 'http:' * m grows by 6 bytes for 5 (the slow_words bound)."""
    b = Builder()
    rows = list(SLOW_BASE)
    rows.append('http:/:80/a.html')                    # (one ':80' right behind the scheme: not byte-serial)
    rows += ['http://x:80/a:80/' + 'z' * t + '.html' for t in range(8)]
    rows += ['http:' * m + 'y.html' for m in range(1, 13)]
    rows += ['x' + 'http:' * m + '.html' for m in (1, 2, 7, 40)]
    rows += ['http://x/' + 'a:80' * m + '.html' for m in (2, 3, 50)]
    for r in rows:
        for start in range(8):
            b.add_at(r, start, 8)
    return b


# ------------------------------------------------------------------ family: same_key
SAME_KEY_LENS = (21, 22, 23, 24, 25, 63, 64, 65, 119, 120, 121, 127, 128, 129, 135, 136, 137, 255, 256, 257)
N_SPELLINGS = 10
SPELLING_ROUTES = ('fast', 'ins', 'gap', 'ins_gap', 'slow', 'slow', 'slow', 'fast', 'fast', 'fast')


def same_key_name(length: int, r: int = 0) -> str:
    """N = 'https://h.com/<letter>/' + 'k' * m + '.html' of `length` bytes (21 is the shortest); the letter tells
    the rotations' keys apart."""
    assert length >= 21
    return 'https://h.com/' + 'abcdefghij'[r] + '/' + 'k' * (length - 21) + '.html'


def spell(N: str, s: int) -> str:
    """Spelling s of the normalised URL N (which starts 'https://h.com' and ends '.html'): four fast plan kinds,
    three byte-serial ones, three cut variants."""
    assert N.startswith('https://') and N.endswith('.html') and len(N) >= 21
    return (N,
            'http://' + N[8:],
            N[:13] + ':80' + N[13:],
            'http://' + N[8:13] + ':80' + N[13:],
            'http://' + N[8:13] + ':80:80' + N[13:],
            'htt:80ps://' + N[8:],
            'htt:80p://' + N[8:],
            N[:-5] + 'xhtml',
            N[:-5] + '€html?z',
            N + '.html')[s]


def near_miss_positions(length: int) -> List[int]:
    """Byte positions of N at which a near miss differs: the first byte after the scheme, both bytes at every
    8-byte word edge, bytes 127 and 128, the last byte before ".html"."""
    ps = {8, length - 6, 127, 128}
    for e in range(16, length, 8):
        ps |= {e - 1, e}
    return sorted(p for p in ps if 8 <= p < length - 5)


def near_misses(N: str) -> List[str]:
    return [N[:p] + 'Q' + N[p + 1:] for p in near_miss_positions(len(N))]


@functools.lru_cache(maxsize=None)
def same_key() -> Tuple[List[str], Dict[str, list]]:
    """Per length, ten keys (one a rotation), each in all ten spellings with spelling r first in rotation r:
    every spelling is the first occurrence once, and the later nine are compared with it, so every ordered pair
    (earlier, later) of plan kinds occurs.  Beside rotation 0's key its near misses, one byte off, in changing
    spellings: all kept.  Returns (rows, {'spelled': [(row index, N)], 'near': [(row index, N, N')]})."""
    rows: List[str] = []
    meta = {'spelled': [], 'near': []}
    for length in SAME_KEY_LENS:
        for r in range(N_SPELLINGS):
            N = same_key_name(length, r)
            for t in range(N_SPELLINGS):
                meta['spelled'].append((len(rows), N))
                rows.append(spell(N, (r + t) % N_SPELLINGS))
            if r == 0:
                for q, M in enumerate(near_misses(N)):
                    meta['near'].append((len(rows), N, M))
                    rows.append(spell(M, q % N_SPELLINGS))
    return rows, meta


TWIN_LENS = (137, 256, 257)
TWIN_REPEATS = 2


def tail_twins(length: int, spelled: bool = True) -> List[str]:
    """A run of its own: same_key's key of `length` bytes and keys that equal it in their first 128 bytes and differ
    in one byte behind them, then TWIN_REPEATS repeats of the key.  compare_pairs takes 128 bytes of a pair a round
    (4 lanes x 4 words x 8 bytes), and a pair is compared only when the two rows share a hash tag; under the 4-bit
    test hash a run has at most 16 first rows, so all but 16 of these rows are compared with a row of this run --
    pairs that only the second and third round tell apart."""
    N = same_key_name(length)
    ps = sorted({128, 129, 135, 136, length - 6} & set(range(128, length - 5)))
    keys = [N] + [N[:p] + c + N[p + 1:] for p in ps for c in 'QRSTUVWX'] + [N] * TWIN_REPEATS
    return [spell(k, (3 * i) % N_SPELLINGS) if spelled else k for i, k in enumerate(keys)]


# ------------------------------------------------------------------ family: groups
GROUP_ROW_COUNTS = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)
GROUP_NCH = (510, 511, 512, 513)


@functools.lru_cache(maxsize=None)
def _pool() -> Tuple[str, ...]:
    """Rows of align_cut, gap and same_key, every plan kind among them, in a seeded order."""
    rows = [r for r, _ in marked(align_cut())][::7] + [r for r, _ in marked(gap())][::3] + same_key()[0][::5]
    random.Random(11).shuffle(rows)
    return tuple(rows)


def group_count_rows(n: int) -> List[str]:
    """n rows of the pool (with repeats of it when the pool is shorter: duplicates across the claims)."""
    p = _pool()
    k = max(1, (n * 2) // 3)
    return [p[(i % k) * 5 % len(p)] for i in range(n)]


def _exact_row(tag: str, length: int) -> str:
    """A kept fast row whose raw and normalised length is `length`."""
    head = 'https://h.com/' + tag + '/'
    assert length >= len(head) + 5, (tag, length)
    return head + 'w' * (length - len(head) - 5) + '.html'


def nch_of(A0: int, A1: int) -> int:
    """dd_transform_kernel: the 16-byte chunks that cover [A0, A1 + 16) from A0 rounded down."""
    return (A1 + 16 - (A0 & ~15) + 15) >> 4


def group_nch(rows: Sequence[str]) -> List[int]:
    _, off = pack(rows)
    n = len(rows)
    return [nch_of(int(off[i]), int(off[min(i + 64, n)])) for i in range(0, n, 64)]


@functools.lru_cache(maxsize=None)
def groups_run() -> Tuple[str, ...]:
    """Groups of 64 rows side by side in one run: nch at 510, 511 (both ends of its 16 byte totals), 512 (both
    ends), 513, then 511 and 512 again; a group with one 9000-byte row; a group of 64 empty rows; a partial last
    group.  63 rows of a group come from the pool (the same rows in several groups: duplicates on both sides of a
    route change), the 64th makes the byte total exact."""
    rng = random.Random(12)
    pool = _pool()
    rows: List[str] = []
    pos = 0

    def add_group(g_rows):
        nonlocal pos
        assert len(g_rows) <= 64 and len(rows) % 64 == 0
        rows.extend(g_rows)
        pos += sum(len(enc(r)) for r in g_rows)

    plan = [(510, 0), (511, 0), (511, 15), (512, 0), (512, 15), (513, 0), (511, 7), (512, 3)]
    for gi, (nch, delta) in enumerate(plan):
        total = 16 * nch - 31 - (pos & 15) + delta        # nch = (pos % 16 + total + 31) >> 4
        g = [pool[rng.randrange(len(pool))] for _ in range(63)]
        while sum(len(enc(r)) for r in g) > total - 64:
            g[max(range(63), key=lambda i: len(enc(g[i])))] = ''
        last = _exact_row('g%d' % (gi % 3), total - sum(len(enc(r)) for r in g))
        g.insert(rng.randrange(64), last)
        A0 = pos
        add_group(g)
        assert nch_of(A0, pos) == nch
    g = [pool[rng.randrange(len(pool))] for _ in range(63)]
    g.insert(17, _exact_row('big', 9000) + '?z')
    add_group(g)
    add_group([''] * 64)
    add_group([pool[rng.randrange(len(pool))] for _ in range(40)])
    return tuple(rows)


# ------------------------------------------------------------------ family: copy
COPY_KEPT_COUNTS = (1, 31, 32, 33, 64, 65)
COPY_DENSE = (4080, 4096, 4112)      # D1 - (D0 & ~15) of a task: the last two either side of CPS_OUT
COPY_RAW = (6128, 6144, 6160)        # B1 - B0 of a task: the last two either side of CPS_IN


def copy_count_rows(n_kept: int) -> List[str]:
    """A run with exactly n_kept kept rows (the last task partial unless n_kept is a multiple of 32), dropped
    rows between them; the first kept row is 'xhtml': '.html', E = 0."""
    rows = ['xhtml']
    for i in range(1, n_kept):
        rows.append(spell(_exact_row('n%d' % i, 30 + (i * 7) % 90), i % N_SPELLINGS))
        if i % 3 == 0:
            rows.append(rows[-2])                      # a duplicate
        if i % 5 == 0:
            rows.append('no cut %d' % i)
    rows += ['yhtml', 'xhtml?']                        # '.html' again: duplicates
    return rows


@functools.lru_cache(maxsize=None)
def copy_run() -> Tuple[str, ...]:
    """Tasks of 32 kept rows, one after another in one run (every task adds exactly 32 kept rows):
    17 tasks whose dense bytes are 1 modulo 16 (D0 at every residue modulo 16); tasks with the dense range at
    COPY_DENSE; tasks with the raw span at COPY_RAW, stretched by dropped rows (duplicates, rows with no cut,
    filtered rows) between the kept ones; a task of byte-serial rows alone; the '.html' row of length 5."""
    rows: List[str] = []
    st = {'pos': 0, 'dense': 0, 'task': 0}

    def add(row, kept_len=None):
        rows.append(row)
        st['pos'] += len(enc(row))
        if kept_len is not None:
            st['dense'] += kept_len

    def kept(tag, length, s=0):
        add(spell(_exact_row(tag, length), s), length)

    def dense_task(total, spellings=(0, 1, 2, 3)):
        t = st['task']
        st['task'] += 1
        left = total
        for i in range(31):
            ln = total // 32 + (i * 5 + t) % 7 - 3          # (the 7 residues in turn: about total / 32 is left)
            kept('t%d.%d' % (t, i), ln, spellings[i % len(spellings)])
            left -= ln
        kept('t%d.31' % t, left, spellings[t % len(spellings)])

    add('xhtml', 5)                                     # '.html': E = 0; with it the first task has 32 kept rows
    t0 = st['task']
    st['task'] += 1
    left = 1601 - 5
    for i in range(30):
        kept('t%d.%d' % (t0, i), 50, i % 4)
        left -= 50
    kept('t%d.30' % t0, left)
    for _ in range(16):                                 # D0 = 1601 * k: every residue modulo 16
        dense_task(1601)
    for n, want in enumerate(COPY_DENSE + COPY_DENSE):  # (twice, a task between to move D0 off a multiple of 16)
        dense_task(1603 + 4 * n)
        dense_task(want - (st['dense'] & 15))
    for want in COPY_RAW:
        t = st['task']
        st['task'] += 1
        B0 = st['pos'] & ~15
        first = len(rows)
        for i in range(31):
            kept('r%d.%d' % (t, i), 40 + i, i % 4)
            if i % 3 == 0:
                add(rows[first])                        # a duplicate of the task's first row
            elif i % 3 == 1:
                add('https://a/news/%' + 'd' * 90 + '.html')
            else:
                add('n' * 100 + 'htm')
        last = _exact_row('r%d.31' % t, 60)
        # need of the last row = its start + 16 + its cut (60 - 5); B1 - B0 = want
        fill = B0 + want - 16 - 55 - st['pos']
        assert fill >= 0
        add('m' * fill)
        add(last, 60)
        assert st['pos'] - 60 + 16 + 55 - B0 == want
    t = st['task']
    st['task'] += 1
    for i in range(32):                                 # byte-serial rows alone (need = b + 16)
        N = _exact_row('s%d.%d' % (t, i), 30 + i)
        add(spell(N, 4 + i % 3), len(N))
    dense_task(1300)                                    # and a last whole task behind them
    for i in range(7):                                  # a partial last task
        kept('p.%d' % i, 33 + i, i % N_SPELLINGS)
    return tuple(rows)


def copy_tasks(rows: Sequence[str]) -> List[dict]:
    """dd_copy_staged_kernel's tasks over the oracle's kept rows: per task its dense range D1 - (D0 & ~15), its raw
    span B1 - B0 (B1 = the last row's start + 16 + its cut, + 0 for a byte-serial row), D0 modulo 16, its rows'
    routes."""
    R = GEOMETRY['CPS_ROWS']
    kept, new = dd.dedup_rows(rows)
    _, off = pack(rows)
    lens = [len(enc(s)) for s in new]
    d = [0]
    for x in lens:
        d.append(d[-1] + x)
    out = []
    for k0 in range(0, len(kept), R):
        k1 = min(k0 + R, len(kept))
        rts = [route(enc(rows[i])) for i in kept[k0:k1]]
        need = int(off[kept[k1 - 1]]) + 16 + (0 if rts[-1].route == 'slow' else rts[-1].cut)
        out.append({'dense': d[k1] - (d[k0] & ~15), 'raw': need - (int(off[kept[k0]]) & ~15), 'd0': d[k0] & 15,
                    'rows': k1 - k0, 'routes': {r.route for r in rts}, 'min_len': min(lens[k0:k1])})
    return out


# ------------------------------------------------------------------ family: raw (normalize = False)
@functools.lru_cache(maxsize=None)
def raw_rows() -> Builder:
    """Keep-first over the strings themselves: lengths 0..24 at every start modulo 16, once the same string at
    every start (one kept, fifteen duplicates compared at every alignment pair) and once with the start in it
    (all kept: the copy at every alignment); the empty string three times and more; same_key's keys and near
    misses (lengths around 24, 64, 120, 128, 136 and 256, one byte apart), each twice."""
    b = Builder()
    b.add('')
    b.add('')
    b.add('')
    for L in range(25):
        base = ('r%02d' % L + 'abcdefghijklmnopqrstuvwxyz')[:L]
        for start in range(16):
            b.add_at(base, start)
            b.add_at(base[:-1] + 'ABCDEFGHIJKLMNOP'[start] if L else '', (start + 7) % 16)
    keys = []
    for length in SAME_KEY_LENS:
        N = same_key_name(length)
        keys += [N] + near_misses(N)
    for i, k in enumerate(keys):
        b.add_at(k, i % 16)
    for i, k in enumerate(reversed(keys)):
        b.add_at(k, (3 * i + 1) % 16)
    return b


# ------------------------------------------------------------------ the long collision list
def collide_rows(n_distinct: int = 70000, n_repeat: int = 5000) -> List[str]:
    """n_distinct short URLs and n_repeat repeats among them: under the 4-bit test hash all of them share a tag, so
    all but the first row of each of the 16 slots are listed for the host's exact pass."""
    rows = ['https://h/%05x.html' % i for i in range(n_distinct)]
    step = n_distinct // n_repeat
    return rows + [rows[i * step] if i % 2 else 'http://h:80/%05x.html?r' % (i * step) for i in range(n_repeat)]


# ------------------------------------------------------------------ the CPU fuzz's tokens
FUZZ_TOKENS = ('http:', 'https:', ':80', ':', 'html', '.html', 'news/%', "news/'", 'news/', '%', "'", '\n', 'é', '中',
               '😀', 'a', 'b', '/', 'x.', '80', 'htt', 'p:', 's', 'tml', 'h', ':8', '0')


def fuzz_strings(n: int = 20000, seed: int = 5) -> List[str]:
    rng = random.Random(seed)
    return [''.join(rng.choice(FUZZ_TOKENS) for _ in range(rng.randint(1, 9))) for _ in range(n)]


FAMILIES = ('align_cut', 'cut_rule', 'gap', 'filter', 'slow', 'same_key', 'groups', 'copy')


def family_rows(name: str) -> List[str]:
    """The rows of a normalising family's (main) run."""
    if name == 'same_key':
        return list(same_key()[0])
    if name == 'groups':
        return list(groups_run())
    if name == 'copy':
        return list(copy_run())
    return list({'align_cut': align_cut, 'cut_rule': cut_rule, 'gap': gap, 'filter': filter_rows,
                 'slow': slow}[name]().rows)
