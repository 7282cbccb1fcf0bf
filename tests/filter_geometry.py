"""Byte-geometry cases for the fast path's filter and probe kernels (csrc/kwmatch_split.hpp): exact names planted on
tile edges, lane edges, a group's first and last bytes and across field, document and group boundaries.

Pure Python, deterministic (string-seeded ``random.Random``; no set or hash order), no GPU and no oracle.  The
builder lays documents out as ``matcher.pack_fields`` does (plain concatenation of text, title, text, ...), so it
knows every byte offset while it builds and sizes the filler in front of an occurrence to put it at a chosen
place.  ``tags()`` is the independent side: it derives what an occurrence exercises from the packed offsets (and
the arena's bytes for the neighbour kinds), not from what the builder meant; tests/test_filter_geometry_cases.py
holds the two against each other and against the CPU oracle.

The kernels' geometry restated: a filter wave takes a group of 32 documents as one flat byte range that starts at
``base = gb & ~15`` (gb = the group's first byte, g0 = gb & 15) and ends at ge (gl = ge - base), in 1 KiB tiles of
64 lanes x 16 bytes; lane 63's fifth word is the word after the tile.
"""
from __future__ import annotations

import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

FG_DOCS = 32
TILE = 1024
MAX_FIELD = 8192
MAX_DOCS = 6000

LONG = 'BERKSHIRE HATHAWAY INC'
FAMILY = ('GE', 'GEO', 'GEOS')
CLASSES = ('2', '3', '4', '5-8', '>16')
REP = {'2': 'GE', '3': 'GEO', '4': 'GEOS', '5-8': 'NVIDIA', '>16': LONG}      # the class's name on every edge
ALT = {'2': '3M', '3': 'IBM', '4': 'AT&T', '5-8': 'NVIDIA', '>16': LONG}      # a second one where there is one
SPLIT = {'2': ('GE',), '3': ('IBM', 'GEO'), '4': ('AT&T',), '5-8': ('NVIDIA',), '>16': (LONG,)}   # straddled names
NONWORD = ('C++', '.NET', 'U.S.')             # a first or last code point that is no word character
FUZZY3, FUZZY9 = 'Zq7', 'Vy-Kx~Jw8'           # fuzzy-class names: found as exact substrings only (m <= 10)
BASE_U = ['GEOS', 'AT&T', '.NET', 'U.S.', 'NVIDIA', LONG]
SHORT = {                                     # the 2-3 byte uppercase names of each KB -> fk_stage1<variant>
    0: [],
    3: ['GE', 'GEO', 'IBM', '3M', 'C++'],
    2: ['GE', 'EG', 'GEO'],
    1: ['GE', 'GEO', 'AÉ'],
}
ALL_U = BASE_U + ['GE', 'GEO', 'IBM', '3M', 'C++', 'EG', 'AÉ']
TILE_BOUNDARIES = (1, 2, 3, 4, 7)
GEND_VALUES = (0, 1, 2, 3, 4, 15, 16, 17) + tuple(range(1008, 1024))
NB_KINDS = ('word', 'sp', 'dot', 'plus', 'nl', 'eacute', 'rsquo')
NB_TEXT = {'word': 'a', 'sp': ' ', 'dot': '.', 'plus': '+', 'nl': '\n', 'eacute': 'é', 'rsquo': '’'}
EDGE_KINDS = ('letter', 'digit', 'us', 'space', 'own')
EDGE_POS = ('text_first', 'text_last', 'title_first', 'title_last')
SMALL_SIZES = (1, 31, 32, 33, 64, 65, 97)     # documents of the small corpora (their last group is the arena's last)
SMALL_CLASS = {1: '2', 31: '3', 33: '4', 65: '5-8', 97: '>16', 32: '2', 64: '3'}

_ALPHABET = 'abcdefghilmnoprstu'              # lower case, none of the fuzzy names' letters
_NOISE = ['GEa', 'aGE', 'GEOa', 'GEOSa', 'aGEOS', 'IBMa', 'aIBM', '3Ma', 'a3M', 'EGa', 'aEG', 'NVIDIB', 'NVIDIAa',
          'NVIDxa', 'AT&', 'AT&Ta', '.NE', '.NET', 'C++', 'U.S.', 'U.Sa', 'BERKSHIRE HATHAWAY INK',
          'BERKSHIRE HATHAWAX INC', 'BERKa', 'Zq8', 'Zq9', 'Vy-Kx~Jw9', 'Vy-Kx~', 'GEGa', 'GEOT']


def kb_names(variant: int, fuzzy: bool = True) -> List[str]:
    """The names of the KB that selects stage-1 gate `variant` (fuzzy=False: its uppercase names only)."""
    return SHORT[variant] + BASE_U + ([FUZZY3, FUZZY9] if fuzzy else [])


def processed(names: Sequence[str]) -> Dict:
    return {f'T{i}': {'aliases': {n: (None, None)}} for i, n in enumerate(names)}


def name_class(name: str) -> str:
    if name == FUZZY3:
        return 'f3'
    if name == FUZZY9:
        return 'f9'
    n = len(name.encode())
    return '2' if n == 2 else '3' if n == 3 else '4' if n == 4 else '5-8' if n <= 8 else '>16'


def is_word(ch: Optional[str]) -> bool:
    return ch is not None and (ch.isalnum() or ch == '_')


def expect_match(name: str, prev: Optional[str], nxt: Optional[str]) -> bool:
    """The builder's rule for an occurrence inside its field (prev / nxt: the code points next to it in the field,
    None at a field edge): a fuzzy-class name always; an uppercase name when a word / non-word change stands at
    both of its ends, a field edge counting as a non-word."""
    if name in (FUZZY3, FUZZY9):
        return True
    return is_word(name[0]) != is_word(prev) and is_word(name[-1]) != is_word(nxt)


def default_pre(name: str) -> str:
    return ' ' if is_word(name[0]) else 'a'


def default_post(name: str) -> str:
    return ' ' if is_word(name[-1]) else 'a'


# --------------------------------------------------------------------------------------------------- the corpus
class Corpus:
    """Documents as UTF-8 fields, the occurrences planted in them and the names split over a boundary."""

    def __init__(self, label: str):
        self.label = label
        self.fields: List[bytes] = []          # text, title, text, ...
        self.nbytes = 0
        self.plants: List[Tuple[int, int, int, str, str]] = []     # (doc, field, byte start, name, case label)
        self.straddles: List[Tuple[int, int, int, str, str]] = []  # (doc, field, split, name, kind): name[:split]
                                                                   # ends that field, name[split:] starts the next
        self.rng = random.Random('filter-geometry/' + label)
        self.survivors: List[Tuple[int, int, int, int]] = []       # dense runs: (doc, field, byte start, bytes)

    # -- filler
    def clean(self, n: int) -> bytes:
        out = []
        have = 0
        while have < n:
            w = ''.join(self.rng.choice(_ALPHABET) for _ in range(self.rng.randint(2, 9))) + ' '
            out.append(w)
            have += len(w)
        return ''.join(out)[:n].encode()

    def noisy(self, n: int) -> bytes:
        """Near misses between spaces (every token fails whatever stands around the filler), clean filler to n."""
        out = b''
        while True:
            t = (' ' + self.rng.choice(_NOISE) + ' ' + self.clean(self.rng.randint(0, 6)).decode()).encode()
            if len(out) + len(t) + 1 > n:
                break
            out += t
        if len(out) < n:
            out += b' ' + self.clean(n - len(out) - 1)
        return out[:n] if n else b''

    def fill(self, n: int, noisy: bool = False) -> bytes:
        return self.noisy(n) if noisy and n >= 8 else self.clean(n)

    # -- documents
    @property
    def n_docs(self) -> int:
        return len(self.fields) // 2

    def doc(self, text: bytes, title: bytes, plants=()) -> int:
        """Append one document; plants: (field, byte start, name, label)."""
        assert len(text) <= MAX_FIELD and len(title) <= MAX_FIELD
        d = self.n_docs
        self.fields += [bytes(text), bytes(title)]
        self.nbytes += len(text) + len(title)
        for f, s, name, label in plants:
            assert (title if f else text)[s:s + len(name.encode())] == name.encode(), (label, name)
            self.plants.append((d, f, s, name, label))
        return d

    def filler_doc(self, size: int, noisy: bool = False) -> int:
        """A document of `size` bytes without an occurrence."""
        t = 12 if size >= 40 else 0
        return self.doc(self.fill(size - t, noisy), self.clean(t))

    def pad_group(self):
        """Filler documents up to the next multiple of 32."""
        while self.n_docs % FG_DOCS:
            self.filler_doc(48)

    # -- results
    def strings(self) -> Tuple[List[str], List[str]]:
        s = [f.decode() for f in self.fields]
        return s[0::2], s[1::2]

    def offsets(self) -> np.ndarray:
        off = np.zeros(len(self.fields) + 1, dtype=np.int64)
        np.cumsum([len(f) for f in self.fields], out=off[1:])
        return off

    def arena(self) -> bytes:
        return b''.join(self.fields)

    def expected(self, names: Sequence[str]) -> Dict[Tuple[int, int, str], List[int]]:
        """(doc, field, name) -> sorted code-point positions of the occurrences planted as matches, names of the KB."""
        have = set(names)
        out: Dict[Tuple[int, int, str], List[int]] = {}
        for d, f, s, name, _label in self.plants:
            if name in have and self.plant_matches(d, f, s, name):
                fb = self.fields[2 * d + f]
                out.setdefault((d, f, name), []).append(len(fb[:s].decode()))
        for v in out.values():
            v.sort()
        return out

    def plant_matches(self, d: int, f: int, s: int, name: str) -> bool:
        fb = self.fields[2 * d + f]
        before, after = fb[:s].decode(), fb[s + len(name.encode()):].decode()
        return expect_match(name, before[-1] if before else None, after[0] if after else None)


def payload(name: str, pre: Optional[str] = None, post: Optional[str] = None) -> Tuple[bytes, int]:
    """(pre + name + post as bytes, the name's byte offset in them)."""
    pre = default_pre(name) if pre is None else pre
    post = default_post(name) if post is None else post
    return (pre + name + post).encode(), len(pre.encode())


# --------------------------------------------------------------------------------------------------- free cases
# Cases that need no chosen byte offset: lists of documents (text, title, plants, straddles) that ride in the
# positioned groups in place of filler documents and stay together inside one group.
def _field_with(c: Corpus, parts, lead: int = 24, tail: int = 24):
    """filler + parts joined by filler + filler; parts: (name, pre, post, label) -> (bytes, plants as (start, name, label))."""
    out = c.clean(lead)
    plants = []
    for name, pre, post, label in parts:
        pl, o = payload(name, pre, post)
        plants.append((len(out) + o, name, label))
        out += pl + c.clean(c.rng.randint(10, 20))
    return out + c.clean(tail), plants


def _edge_byte(kind: str, name: str, before: bool) -> str:
    return {'letter': 'z', 'digit': '5', 'us': '_', 'space': ' ', 'own': name[-1] if before else name[0]}[kind]


def _free_items(c: Corpus) -> List[List[Tuple[bytes, bytes, list, list]]]:
    items = []

    def one(text, title, tp=(), ip=(), st=()):
        return (text, title, [(0,) + p for p in tp] + [(1,) + p for p in ip], list(st))

    # field edges: the occurrence is the first / last bytes of a text / a title; the arena byte next to it belongs
    # to the neighbouring field or document
    for name in [REP[k] for k in CLASSES] + ['C++', '.NET']:
        nb = name.encode()
        for kind in EDGE_KINDS:
            for pos in EDGE_POS:
                label = f'fedge/{pos}/{kind}'
                inner = default_post(name) if pos.endswith('first') else default_pre(name)
                if pos == 'text_first':     # the previous document's title ends with the neighbour byte
                    prev = one(c.clean(30), c.clean(11) + _edge_byte(kind, name, True).encode())
                    text = nb + inner.encode() + c.clean(30)
                    items.append([prev, one(text, c.clean(12), tp=[(0, name, label)])])
                elif pos == 'text_last':    # the document's own title starts with it
                    text = c.clean(30) + inner.encode() + nb
                    title = _edge_byte(kind, name, False).encode() + c.clean(11)
                    items.append([one(text, title, tp=[(len(text) - len(nb), name, label)])])
                elif pos == 'title_first':  # its own text ends with it
                    text = c.clean(30) + _edge_byte(kind, name, True).encode()
                    title = nb + inner.encode() + c.clean(11)
                    items.append([one(text, title, ip=[(0, name, label)])])
                else:                       # the next document's text starts with it
                    title = c.clean(11) + inner.encode() + nb
                    nxt = one(_edge_byte(kind, name, False).encode() + c.clean(30), c.clean(12))
                    items.append([one(c.clean(30), title, ip=[(len(title) - len(nb), name, label)]), nxt])
    # straddles: a name split over text|title and over title|next text, with an unsplit control document
    for cls in CLASSES:
        for name in SPLIT[cls]:
            nb = name.encode()
            for s in range(1, len(nb)):
                left, right = nb[:s], nb[s:]
                lp = [(31, left.decode(), 'straddle/piece')] if left.decode() in ALL_U else []
                ctl_text, ctl_p = _field_with(c, [(name, None, None, 'straddle/control')])
                ctl = one(ctl_text, c.clean(12), tp=ctl_p)
                a = one(c.clean(30) + b' ' + left, right + b' ' + c.clean(11), tp=lp, st=[(0, s, name, 'text|title')])
                items.append([a, ctl])
                ip = [(13, left.decode(), 'straddle/piece')] if left.decode() in ALL_U else []
                b0 = one(c.clean(30), c.clean(12) + b' ' + left, ip=ip, st=[(1, s, name, 'title|text')])
                b1 = one(right + b' ' + c.clean(30), c.clean(12))
                ctl_text, ctl_p = _field_with(c, [(name, None, None, 'straddle/control')])
                items.append([b0, b1, one(ctl_text, c.clean(12), tp=ctl_p)])
    # neighbours inside a field: each side takes each kind; one document per (name, kind before, ASCII or not)
    for name in [REP[k] for k in CLASSES] + ['3M', 'IBM', 'AT&T', 'C++', 'U.S.', '.NET', 'EG', 'AÉ', FUZZY3, FUZZY9]:
        for kb in NB_KINDS:
            for nonascii in (False, True):
                parts = [(name, NB_TEXT[kb], NB_TEXT[ka], f'nb/{kb}/{ka}') for ka in NB_KINDS
                         if ((kb in ('eacute', 'rsquo')) or (ka in ('eacute', 'rsquo')) or not name.isascii()) == nonascii]
                if parts:
                    text, tp = _field_with(c, parts)
                    items.append([one(text, c.clean(12), tp=tp)])
    # shared keys: GEOS, GEO and GE as a whole token, as a prefix of a longer token and as a field's last bytes
    for name in FAMILY:
        text, tp = _field_with(c, [(name, ' ', ' ', 'shared/token'), (name, ' ', 'x', 'shared/prefix')])
        tail = b' ' + name.encode()
        tp.append((len(text) + 1, name, 'shared/field_end'))
        title = c.clean(9) + tail
        items.append([one(text + tail, title, tp=tp, ip=[(10, name, 'shared/field_end')])])
    return items


# --------------------------------------------------------------------------------------------------- positioned groups
def _requests() -> List[Tuple[int, str, str]]:
    """(start - base, name, label) of every occurrence that needs a chosen place in its group."""
    out = []
    for cls in CLASSES:
        name = REP[cls]
        L = len(name)
        splits = [s for s in range(1, L) if s <= 8 or s >= L - 8]
        for k in TILE_BOUNDARIES:
            out.append((TILE * k - L, name, f'tile_end/{k}'))
            out.append((TILE * k, name, f'tile_start/{k}'))
            out += [(TILE * k - s, name, f'tile_split/{k}/{s}') for s in splits]
        for r in range(16):
            out.append((TILE * 5 + 16 * 20 + r, ALT[cls], f'res/{r}'))
        for t, lane in ((2, 0), (3, 1), (5, 62), (6, 63)):
            out.append((TILE * t + 16 * lane + 3, ALT[cls], f'lane/{lane}'))
    for name in NONWORD + (FUZZY3, FUZZY9, 'IBM', '3M'):
        L = len(name)
        for k in (1, 4):
            out.append((TILE * k - L, name, f'tile_end/{k}'))
            out.append((TILE * k, name, f'tile_start/{k}'))
            out += [(TILE * k - s, name, f'tile_split/{k}/{s}') for s in range(1, L)]
        out += [(TILE * 6 + 16 * 30 + r, name, f'res/{r}') for r in (0, 13, 14, 15)]
    return out


class _Pool:
    def __init__(self, items):
        self.items = list(items)

    def take(self, docs: int, nbytes: int):
        """The first item of at most `docs` documents and `nbytes` bytes, or None."""
        for i, it in enumerate(self.items[:40]):
            if len(it) <= docs and sum(len(t) + len(ti) for t, ti, _p, _s in it) <= nbytes:
                return self.items.pop(i)
        return None


def _emit_item(c: Corpus, item):
    for text, title, plants, strad in item:
        d = c.doc(text, title, [(f, s, n, lb) for f, s, n, lb in plants])
        for f, s, name, kind in strad:
            c.straddles.append((d, f, s, name, kind))


def _fill_gap(c: Corpus, pool: _Pool, docs: int, nbytes: int, noisy: bool) -> int:
    """`docs` whole documents of at most `nbytes` bytes in all (free cases where they fit, filler else); returns
    the bytes left over for the field that follows."""
    while docs > 0:
        it = pool.take(docs, nbytes - 40 * (docs - 1)) if nbytes > 40 * docs else None
        if it is not None:
            before = c.nbytes
            _emit_item(c, it)
            nbytes -= c.nbytes - before
            docs -= len(it)
            continue
        size = min(nbytes // (docs + 1), MAX_FIELD)
        c.filler_doc(size, noisy)
        nbytes -= size
        docs -= 1
    return nbytes


def _positioned_group(c: Corpus, pool: _Pool, head, reqs, tail, gl: int, index: int):
    """One group of 32 documents whose byte range has ge - base = gl.  head: (name, lead bytes 0 / 1, label) at the
    group's first bytes or None; reqs: (start - base, name, label) ascending; tail: (name, label): the last bytes
    of the group's last non-empty field."""
    assert c.n_docs % FG_DOCS == 0
    gb = c.nbytes
    base = gb & ~15
    noisy = index % 3 == 1
    anchors = []     # (absolute start of the payload, payload, name offset, name, label, kind)
    if head is not None:
        name, lead, label = head
        pl, o = payload(name, ' ' * lead, None)
        anchors.append((gb, pl, o, name, label, 'head'))
    for rel, name, label in reqs:
        pl, o = payload(name)
        anchors.append((base + rel - o, pl, o, name, label, 'mid'))
    name, label = tail
    pl, o = payload(name, None, '')
    anchors.append((base + gl - len(pl), pl, o, name, label, 'tail'))
    spare = FG_DOCS - len(anchors)
    gaps = []
    cur = gb
    for a in anchors:
        gaps.append(max(0, a[0] - cur - 96))
        cur = a[0] + len(a[1]) + 64
    total = sum(gaps) or 1
    quota = [spare * g // total for g in gaps]
    quota[-1] += spare - sum(quota)
    for a, q in zip(anchors, quota):
        start, pl, o, name, label, kind = a
        need = start - c.nbytes
        assert need >= 0, (c.label, index, label, need)
        if kind == 'tail' and index % 2:    # the occurrence ends the title; the text takes filler
            left = _fill_gap(c, pool, q, need - 20, noisy) + 20
            text = c.fill(left // 2, noisy)
            title = c.clean(left - left // 2) + pl
            c.doc(text, title, [(1, len(title) - len(pl) + o, name, label)])
            continue
        left = _fill_gap(c, pool, q, need, noisy)
        assert left >= 0 and (kind != 'head' or left == 0)
        text = c.fill(left, noisy) + pl
        if kind == 'tail':
            c.doc(text, b'', [(0, left + o, name, label)])
        else:
            text += c.clean(c.rng.randint(16, 40))
            c.doc(text, c.clean(8) if index % 2 else b'', [(0, left + o, name, label)])
    assert c.n_docs % FG_DOCS == 0 and c.nbytes == base + gl, (c.label, index, c.n_docs, c.nbytes - base, gl)


def _plain_group(c: Corpus, pool: _Pool, first, last):
    """32 documents: `first`, 30 free-case or filler documents, `last` (each (text, title, plants, straddles))."""
    assert c.n_docs % FG_DOCS == 0
    _emit_item(c, [first])
    left = _fill_gap(c, pool, FG_DOCS - 2, 30 * 150, False)
    del left
    _emit_item(c, [last])
    assert c.n_docs % FG_DOCS == 0


def _empties_groups(c: Corpus, pool: _Pool, cls: str):
    """Layouts with empty documents for one class: slots 0 / 30 / 31 around a run of 29, an all-empty group, then
    slots 1, 3 and 6 with runs of 1 and 2."""
    name = REP[cls]

    def planted(label, in_title=False, other=True):
        body, tp = _field_with(c, [(name, None, None, label)], lead=14, tail=10)
        if in_title:
            c.doc(c.clean(20) if other else b'', body, [(1, tp[0][0], name, label)])
        else:
            c.doc(body, c.clean(9) if other else b'', [(0, tp[0][0], name, label)])

    assert c.n_docs % FG_DOCS == 0
    planted('empties/slot0', other=False)                 # its title is empty; 29 empty documents follow
    for _ in range(29):
        c.doc(b'', b'')
    planted('empties/slot30', in_title=True, other=False)   # its text is empty
    planted('empties/slot31')
    for _ in range(FG_DOCS):                              # a whole group of empty documents
        c.doc(b'', b'')
    c.filler_doc(60)
    planted('empties/slot1')
    c.doc(b'', b'')
    planted('empties/slot3')
    c.doc(b'', b'')
    c.doc(b'', b'')
    planted('empties/slot6')
    c.doc(b'', b'')
    planted('empties/slot8')
    _fill_gap(c, pool, 21, 21 * 150, False)
    planted('empties/slot30b')
    planted('empties/slot31b')
    assert c.n_docs % FG_DOCS == 0


def main_corpus() -> Corpus:
    c = Corpus('main')
    pool = _Pool(_free_items(c))
    # the positioned requests, spread over the chained groups: at least 192 bytes apart in one group
    n_groups = len(CLASSES) * len(GEND_VALUES)
    slots: List[List[Tuple[int, str, str]]] = [[] for _ in range(n_groups)]
    nxt = 0
    for req in _requests():
        for k in range(n_groups):
            g = (nxt + k) % n_groups
            if all(abs(req[0] - r[0]) >= 192 for r in slots[g]) and len(slots[g]) < 6:
                slots[g].append(req)
                nxt = g + 1
                break
        else:
            raise AssertionError(f'no group takes {req}')
    # the chain: group i ends with the class's name at (ge - base) % 1024 = v, so the next group starts at g0 = v & 15
    # with the same class's name as its first bytes (one byte in after v = 16)
    c.filler_doc(50)
    c.pad_group()
    head = None
    i = 0
    for cls in CLASSES:
        for v in GEND_VALUES:
            _positioned_group(c, pool, head, sorted(slots[i]), (REP[cls], f'gend/{v}'), 8 * TILE + v, i)
            head = (REP[cls], 1 if v == 16 else 0, 'gstart+1' if v == 16 else f'gstart/{v & 15}')
            i += 1
    # the group after the chain takes the last head; then the names split over a group boundary
    def first_doc(hd):
        name, lead, label = hd
        pl, o = payload(name, ' ' * lead, None)
        return (pl + c.clean(30), c.clean(10), [(0, o, name, label)], [])

    pending = first_doc(head)
    for cls in CLASSES:
        for name in SPLIT[cls]:
            nb = name.encode()
            for s in range(1, len(nb)):
                left, right = nb[:s], nb[s:]
                ip = [(1, 13, left.decode(), 'straddle/piece')] if left.decode() in ALL_U else []
                last = (c.clean(30), c.clean(12) + b' ' + left, ip, [(1, s, name, 'group')])
                _plain_group(c, pool, pending, last)
                ctl, tp = _field_with(c, [(name, None, None, 'straddle/control')])
                pending = (right + b' ' + ctl, c.clean(10), [(0, len(right) + 1 + p, n, lb) for p, n, lb in tp], [])
    _plain_group(c, pool, pending, (c.clean(40), c.clean(10), [], []))
    for cls in CLASSES:
        _empties_groups(c, pool, cls)
    while pool.items:      # whatever free cases are left
        _emit_item(c, pool.items.pop(0))
    assert c.n_docs <= MAX_DOCS, c.n_docs
    return c


def small_corpus(n: int) -> Corpus:
    """Exactly n documents; the class's name is the last bytes of the arena (and of a group of n % 32 documents)."""
    c = Corpus(f'small{n}')
    name = REP[SMALL_CLASS[n]]
    for d in range(n - 1):
        if d % 7 == 3:
            c.doc(b'', b'')
        else:
            text, tp = _field_with(c, [(ALT[CLASSES[d % 5]], None, None, 'small')], lead=10 + d % 17, tail=8)
            c.doc(text, c.clean(6 + d % 5), [(0,) + p for p in tp])
    pl, o = payload(name, None, '')
    if n % 2:
        text = c.clean(21 + n % 16) + pl
        c.doc(text, b'', [(0, len(text) - len(pl) + o, name, 'gend/small')])
    else:
        title = c.clean(5 + n % 16) + pl
        c.doc(c.clean(33), title, [(1, len(title) - len(pl) + o, name, 'gend/small')])
    assert c.n_docs == n
    return c


_CACHE: Dict[str, List[Corpus]] = {}


def cases(fresh: bool = False) -> List[Corpus]:
    """The main corpus and the small ones (each its own arena)."""
    if fresh or 'main' not in _CACHE:
        out = [main_corpus()] + [small_corpus(n) for n in SMALL_SIZES]
        if fresh:
            return out
        _CACHE['main'] = out
    return _CACHE['main']


def dense_cases(fresh: bool = False) -> List[Corpus]:
    """Fields of 1, 3 and 5 KiB of a 2-byte name repeated without separators (every second position a stage-1 and
    stage-2 survivor of a KB that holds it, none a match), and of noisy filler, single occurrences between them."""
    if not fresh and 'dense' in _CACHE:
        return _CACHE['dense']
    c = Corpus('dense')
    real = ['GE', 'GEOS', 'NVIDIA', 'IBM', LONG, FUZZY3, 'AT&T', 'C++', 'GEO', FUZZY9, '3M', 'U.S.']
    k = 0
    for rep in range(3):
        for size in (1024, 3072, 5120):
            for noisy in (False, True):
                parts, plants = b'', []
                for piece in range(2):
                    half = size // 2
                    if noisy:
                        parts += c.noisy(half)
                    else:
                        run = (b'EG' if rep == 2 else b'GE') * (half // 2)
                        c.survivors.append((c.n_docs, 0, len(parts) + 1, len(run)))
                        parts += b' ' + run + b' '
                    name = real[k % len(real)]
                    k += 1
                    pl, o = payload(name)
                    plants.append((0, len(parts) + o, name, f'dense/{size}/{"noisy" if noisy else "run"}'))
                    parts += pl
                title, tp = _field_with(c, [(real[k % len(real)], None, None, 'dense/title')], lead=8, tail=4)
                c.doc(parts, title, plants + [(1,) + p for p in tp])
                c.filler_doc(64)
    out = [c]
    if not fresh:
        _CACHE['dense'] = out
    return out


def dense_survivors(c: Corpus, names: Sequence[str]) -> int:
    """Positions inside the dense runs where a 2-byte name of the KB starts: each passes stage 1 and stage 2."""
    two = [n.encode() for n in names if len(n.encode()) == 2]
    total = 0
    for d, f, s, n in c.survivors:
        fb = c.fields[2 * d + f]
        total += sum(fb[p:p + 2] in two for p in range(s, s + n - 1))
    return total


# --------------------------------------------------------------------------------------------------- the classifier
def _kind_of_byte(b: int, own: int) -> str:
    ch = chr(b)
    return ('own' if b == own else 'letter' if ch.isalpha() else 'digit' if ch.isdigit() else 'us' if ch == '_'
            else 'space' if ch == ' ' else 'other')


def _nb_kind(arena: bytes, lo: int, hi: int, before: bool) -> str:
    """Kind of the code point that ends at hi (before) / starts at lo (after), inside [lo, hi)."""
    s = arena[lo:hi]
    if not s:
        return 'none'
    for kind in ('eacute', 'rsquo'):
        e = NB_TEXT[kind].encode()
        if (s.endswith(e) if before else s.startswith(e)):
            return kind
    b = s[-1] if before else s[0]
    if b >= 0x80:
        return 'other'
    ch = chr(b)
    return {' ': 'sp', '.': 'dot', '+': 'plus', '\n': 'nl'}.get(ch, 'word' if is_word(ch) else 'other')


def _group(off, doc):
    n = (len(off) - 1) // 2
    d0 = doc // FG_DOCS * FG_DOCS
    nd = min(FG_DOCS, n - d0)
    return n, d0, nd, int(off[2 * d0]), int(off[2 * (d0 + nd)])


def tags(off, doc: int, field: int, start: int, length: int, arena: Optional[bytes] = None) -> List[str]:
    """What the occurrence of `length` bytes at byte `start` of (doc, field) exercises, from the packed offsets
    (the arena only names the bytes next to it)."""
    n, d0, nd, gb, ge = _group(off, doc)
    base, g0 = gb & ~15, gb & 15
    gl = ge - base
    fb, fe = int(off[2 * doc + field]), int(off[2 * doc + field + 1])
    a = fb + start
    assert fb <= a and a + length <= fe
    rel, end = a - base, a - base + length
    out = [f'res/{rel % 16}']
    tile, last_tile = rel // TILE, (gl - 1) // TILE
    lane = rel % TILE // 16
    if 0 < tile < last_tile and lane in (0, 1, 62, 63):
        out.append(f'lane/{lane}')
    for k in TILE_BOUNDARIES:
        if end == TILE * k:
            out.append(f'tile_end/{k}')
        if rel == TILE * k:
            out.append(f'tile_start/{k}')
        if rel < TILE * k < end:
            out.append(f'tile_split/{k}/{TILE * k - rel}')
    nonempty = [i for i in range(2 * d0, 2 * (d0 + nd)) if off[i + 1] > off[i]]
    here = 2 * doc + field
    if nonempty and nonempty[0] == here:
        if start == 0:
            out.append(f'gstart/{g0}')
        if start == 1:
            out.append('gstart+1')
    if nonempty and nonempty[-1] == here and a + length == fe:
        out.append(f'gend/{gl % TILE}')
        out.append('gend_last' if ge == int(off[-1]) else 'gend_next')
        if nd < FG_DOCS:
            out.append('gend_short')
    side = 'title' if field else 'text'
    if arena is not None:
        if start == 0 and a > 0:
            out.append(f'fedge/{side}_first/{_kind_of_byte(arena[a - 1], arena[a + length - 1])}')
        if a + length == fe and fe < int(off[-1]):
            out.append(f'fedge/{side}_last/{_kind_of_byte(arena[fe], arena[a])}')
        if start > 0 and a + length < fe:
            out.append(f'nb/{_nb_kind(arena, fb, a, True)}/{_nb_kind(arena, a + length, fe, False)}')
        if start > 0 and a + length < fe and is_word(chr(arena[a + length])) and arena[a + length] < 0x80:
            out.append('shared/prefix')
        if start > 0 and a + length < fe and max(arena[a - 1], arena[a + length]) < 0x80 and \
                not is_word(chr(arena[a - 1])) and not is_word(chr(arena[a + length])):
            out.append('shared/token')
        if a + length == fe:
            out.append('shared/field_end')
    slot = doc % FG_DOCS
    if slot in (0, 1, 30, 31):
        out.append(f'slot/{slot}')

    def empty(d):
        return 0 <= d < n and off[2 * d] == off[2 * d + 2]

    for step, word in ((-1, 'before'), (1, 'after')):
        run, d = 0, doc + step
        while empty(d):
            run += 1
            d += step
        if run in (1, 2, 29):
            out.append(f'empties_{word}/{run}')
    if field == 1 and off[2 * doc] == off[2 * doc + 1]:
        out.append('empty_text')
    if field == 0 and off[2 * doc + 1] == off[2 * doc + 2]:
        out.append('empty_title')
    for step, word in ((-1, 'after'), (1, 'before')):
        e0 = d0 + step * FG_DOCS
        f0 = e0 + step * FG_DOCS
        if 0 <= e0 and e0 + FG_DOCS <= n and off[2 * e0] == off[2 * (e0 + FG_DOCS)] and 0 <= f0 < n and \
                off[2 * f0] < off[2 * min(f0 + FG_DOCS, n)]:
            out.append(f'{word}_empty_group')
    return out


def straddle_tag(off, doc: int, field: int, split: int, length: int) -> str:
    """The boundary a name of `length` bytes split after `split` bytes crosses: its head ends (doc, field)."""
    n = (len(off) - 1) // 2
    fb, fe = int(off[2 * doc + field]), int(off[2 * doc + field + 1])
    assert fe - fb >= split and 2 * doc + field + 2 <= 2 * n
    assert int(off[2 * doc + field + 2]) - fe >= length - split      # the rest starts the next field
    kind = 'text|title' if field == 0 else 'group' if (doc + 1) % FG_DOCS == 0 else 'title|text'
    return f'straddle/{kind}/{split}'


def required_cells() -> List[Tuple[str, str]]:
    """Every (tag, key-length class) the main corpora must hold."""
    out = []
    for cls in CLASSES:
        L = len(REP[cls])
        t = [f'res/{r}' for r in range(16)] + [f'lane/{x}' for x in (0, 1, 62, 63)]
        for k in TILE_BOUNDARIES:
            t += [f'tile_end/{k}', f'tile_start/{k}']
            t += [f'tile_split/{k}/{s}' for s in range(1, L) if s <= 8 or s >= L - 8]
        t += [f'gstart/{g}' for g in range(16)] + ['gstart+1']
        t += [f'gend/{v}' for v in GEND_VALUES] + ['gend_next', 'gend_last', 'gend_short']
        t += [f'fedge/{p}/{k}' for p in EDGE_POS for k in EDGE_KINDS]
        t += [f'nb/{a}/{b}' for a in NB_KINDS for b in NB_KINDS]
        t += [f'slot/{s}' for s in (0, 1, 30, 31)]
        t += [f'empties_{w}/{r}' for w in ('before', 'after') for r in (1, 2, 29)]
        t += ['empty_text', 'empty_title', 'after_empty_group', 'before_empty_group']
        for kind in ('text|title', 'title|text', 'group'):
            t += [f'straddle/{kind}/{s}' for s in range(1, L)]
        out += [(x, cls) for x in t]
    return out


def required_named() -> List[Tuple[str, str]]:
    """(tag, name) cells that belong to a name, not to a class."""
    out = [(f'shared/{k}', n) for n in FAMILY for k in ('token', 'prefix', 'field_end')]
    for name in ('C++', '.NET'):
        out += [(f'fedge/{p}/{k}', name) for p in EDGE_POS for k in EDGE_KINDS]
    for name in NONWORD + (FUZZY3, FUZZY9):
        out += [(f'tile_split/{k}/{s}', name) for k in (1, 4) for s in range(1, len(name))]
        out += [(f'res/{r}', name) for r in (13, 14, 15)]
    return out
