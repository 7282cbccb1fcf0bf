"""The byte-geometry sweep of the non-ASCII decoders: kw_tx_kernel / tx_field / tx_pos (the one-byte-per-code-point
view and its chunk table), decode_field_fast / to_cp_fast (the resolve kernel) and decode_field (the generic kernel).

Fields are concatenations of exact occurrences of KB names with no separator, so every code point of a field
belongs to an occurrence that the hit records report with its re.finditer position: a wrong chunk count or tx_pos
shifts every later position, an overlapping view corrupts another document's.  (An exact occurrence is matched on
the arena's own bytes, so a wrong byte of the view moves no position: family j's decisions see it.)  The
generator works from the packed arena offsets (fields lie back to back in matcher.pack_fields' arena, so a field's
alignment is set by everything before it) and places characters on purpose: over the 16-byte lane boundaries, over
the 1024-byte block boundaries counted from base = fb & ~15, at field ends around them, at every start alignment
and at every output alignment of the title.

Pure Python, deterministic (one string-seeded random.Random, no set or hash order).  The predicates at the end
compute, from the packed arena and its offsets (families f and i: and the names), which cells of each family a
corpus hits; tests/test_tx_geometry_cases.py asserts that every cell is hit, so the generator cannot drift, and
tests/test_gpu_tx_geometry.py sends the documents through every route.

Families (a tag names the one a document was built for and goes into every failure message):
    a  start alignment of text and title, first character ASCII / multi-byte
    b  characters of 2, 3, 4 bytes over (every split), ending on and starting on a lane boundary inside a block,
       base + 1024 and base + 2048, in a text and in a title
    c  field ends: on a block boundary, 1..4 bytes past it, a last chunk of 1 / 15 / 16 bytes, a field inside one
       chunk from its offset 13
    d  text code points mod 16 x title code points {0, 1, 15, 16, 17, 31, 32, 33, 48}; blocks emitting fewer than
       16, exactly 256 and exactly 1024 code points
    e  which fields are non-ASCII
    f  occurrences per field: <= 64, 65..512, > 512 in a text, > 64 in a title
    g  texts of 16383, 16384 and 16385 bytes (FK_CP_CAP = 16384)
    h  the wave and slab mix (document count, ASCII documents between, slabs per 64-document group)
    i  all-uppercase names with a multi-byte word / non-word neighbour over a lane boundary, first and last in a field
    j  a field that ends with a name less one letter and holds the name nowhere else: the name is decided, without
       a position, by an edge window on the decoded code points (an exact occurrence is matched on the arena's own
       bytes, so only such a decision sees a wrong byte of the view); the ending's characters over every boundary
       of family b, and one ending for each code point late in a marker probe chain
"""
import collections
import random
import re

import numpy as np

from advanced_scrapper_amd.matcher import pack_fields

TX_SLAB = 16384
FK_CP_CAP = 16384
PAD = 'zq '                                   # the ASCII documents' and pads' alphabet: in no name
LOWER = 'abcdefghijklmnoprstuvwxy'            # the names' ASCII letters (24: a distinct last letter each)
CAPS = 'ABCDEFGHIJKLMNOPRSTUVWXY'             # a distinct first capital each
UPPERS = ['QZ', 'ZQX', 'XQZQ']                # class U: decided with decode_before / decode_at on the neighbours
GENERIC_UPPER = 'ZQX'
WORD_NB = {2: ['é', 'ж'], 3: ['中'], 4: ['\U0001D400']}                  # \w neighbours by UTF-8 width
NONWORD_NB = {2: ['¡'], 3: ['—', '€', '’'], 4: ['\U0001F600']}           # not \w
FILL4 = '\U0001F601'                          # code points of no name: 0x80 in the view
FILL3 = '㐀'
FILL2 = '¿'
TITLE_CPS = (0, 1, 15, 16, 17, 31, 32, 33, 48)
MAX_OCC = 58                                  # occurrences per field outside family f: at most 64 items on the GPU
SPLITS = [(w, k) for w in (2, 3, 4) for k in range(1, w)]               # k bytes before the boundary, w - k after
TOUCH = [(w, k) for w in (2, 3, 4) for k in range(0, w + 1)]            # k = 0: starts on it, k = w: ends on it
RESERVED = set(''.join(sum(WORD_NB.values(), []) + sum(NONWORD_NB.values(), [])) + FILL4 + FILL3 + FILL2)


def slot(cp):
    return ((cp * 0x9E3779B1) & 0xFFFFFFFF) >> 24


def width(ch):
    return len(ch.encode('utf-8'))


def name_class(name):
    from oracle import kwmatch_oracle as orc
    return orc.name_class(name)


# ------------------------------------------------------------------------------------------------ marker table
def marker_table(names):
    """The library's marker table restated (csrc/kwmatch.hip): the non-ASCII code points of the fuzzy names, most
    frequent first (equal counts: smaller code point first), the first 127 get 0x81.., each into the 256-slot
    open-addressed table at slot(cp), linear probing, wrapping at 255.  Returns (key, val, order)."""
    freq = collections.Counter(ord(c) for n in names if name_class(n) == 'F' for c in n if ord(c) >= 0x80)
    order = sorted(freq, key=lambda c: (-freq[c], c))
    key, val = [None] * 256, [0x80] * 256
    for k, cp in enumerate(order[:127]):
        s = slot(cp)
        while key[s] is not None:
            s = (s + 1) & 255
        key[s], val[s] = cp, 0x81 + k
    return key, val, order


def marker_lookup(key, val, cp):
    """(marker, slots examined, whether the walk passed from slot 255 to slot 0)."""
    s = slot(cp)
    wrapped = False
    for k in range(256):
        if key[s] == cp:
            return val[s], k + 1, wrapped
        if key[s] is None:
            return 0x80, k + 1, wrapped
        wrapped |= s == 255
        s = (s + 1) & 255
    return 0x80, 256, wrapped


# ------------------------------------------------------------------------------------------------ names
_CACHE = {}


def _pool():
    two = [c for c in list(range(0xC0, 0x250)) + list(range(0x391, 0x3CA)) + list(range(0x410, 0x450))
           if c not in (0xD7, 0xF7, 0x3A2)]
    three = list(range(0x4E00, 0x4E00 + 700))
    four = list(range(0x10400, 0x10450)) + list(range(0x1D401, 0x1D454))
    return {2: [c for c in two if chr(c) not in RESERVED], 3: [c for c in three if chr(c) not in RESERVED], 4: four}


def _plan():
    """The 128 non-ASCII code points of the names, chosen by their slot: four that share one home slot (a probe chain
    of at least 4), three whose home is slot 255 (the chain wraps to slots 0 and 1), then the rest; the largest is
    kept apart as the 128th (KB `over`)."""
    if 'plan' in _CACHE:
        return _CACHE['plan']
    rng = random.Random('tx-geometry-code-points')
    pool = _pool()
    allp = sorted(pool[2] + pool[3] + pool[4])
    over_cp = max(pool[4])
    allp.remove(over_cp)
    by_slot = collections.defaultdict(list)
    for c in allp:
        by_slot[slot(c)].append(c)
    wrap = by_slot[255][:3]
    assert len(wrap) >= 2
    s_chain = next(s for s in range(16, 240) if len(by_slot[s]) >= 4)
    chain = by_slot[s_chain][:4]
    special = wrap + chain
    rest = {w: [c for c in pool[w] if c not in special and c != over_cp] for w in (2, 3, 4)}
    for w in rest:
        rng.shuffle(rest[w])
    plan = dict(special=special, wrap=wrap, chain=chain, s_chain=s_chain, rest=rest, over_cp=over_cp)
    _CACHE['plan'] = plan
    return plan


def _build_names():
    if 'names' in _CACHE:
        return _CACHE['names']
    rng = random.Random('tx-geometry-names')
    plan = _plan()
    rest = {w: list(v) for w, v in plan['rest'].items()}
    used = []                                  # the non-ASCII code points handed out so far, in order
    special = list(plan['special'])

    def fresh(w):
        c = rest[w].pop()
        used.append(c)
        return chr(c)

    def body(m_body, n_reuse, heavy):
        """m_body characters: one fresh code point of each width, n_reuse earlier ones, ASCII letters."""
        na = [fresh(2), fresh(3), fresh(4)]
        for _ in range(n_reuse):
            if special:
                c = special.pop(0)
                used.append(c)
                na.append(chr(c))
            else:
                cands = [c for c in used if (width(chr(c)) == 4) or not heavy]
                na.append(chr(rng.choice(cands)))
        chars = na + [rng.choice(LOWER) for _ in range(m_body - len(na))]
        rng.shuffle(chars)
        return ''.join(chars)

    # (code points, reused non-ASCII ones, heavy): 12 light names, 6 heavy ones (titles of few occurrences)
    # (the first names take the chain and wrap code points: long enough that the name less one code point at a field
    # edge still scores over 95, which needs 11 code points: family j)
    shapes = [(12, 1, 0), (13, 1, 0), (14, 1, 0), (18, 2, 0), (20, 2, 0), (11, 1, 0), (8, 1, 0), (9, 1, 0), (10, 1, 0),
              (15, 0, 0), (16, 0, 0), (17, 0, 0), (20, 9, 1), (20, 9, 1), (19, 8, 1), (20, 9, 1), (19, 9, 1), (20, 8, 1)]
    base = []
    for i, (m, nr, heavy) in enumerate(shapes):
        base.append(CAPS[i] + body(m - 2, nr, heavy) + LOWER[i])
    head, tail = [], []
    for j, w in enumerate((2, 3, 4)):          # names that begin / end with a multi-byte character
        i = len(shapes) + j
        lead = fresh(w)
        head.append(lead + CAPS[i] + body(7 + 2 * j, 0, 0) + LOWER[i])
    for j, w in enumerate((2, 3, 4)):
        i = len(shapes) + 3 + j
        last = fresh(w)
        tail.append(CAPS[i] + LOWER[i] + body(6 + 2 * j, 0, 0) + last)
    base_all = base + head + tail
    n_base = len(set(used))
    # `full`: further names that bring the distinct non-ASCII code points to exactly 127
    extra = []
    left = 127 - n_base
    i = 0
    while left > 0:
        take = min(6, left)
        ws = [(2, 3, 4)[(i + q) % 3] for q in range(take)]
        chars = [fresh(w) for w in ws] + [rng.choice(LOWER) for _ in range(12 - take)]
        rng.shuffle(chars)
        extra.append(CAPS[i % 24] + LOWER[(i * 7 + 3) % 24] + ''.join(chars) + LOWER[(i * 5 + 1) % 24])
        left -= take
        i += 1
    assert len(set(used)) == 127
    over = 'Ov' + chr(used[3]) + 'er' + chr(plan['over_cp']) + 'fl' + chr(used[10]) + 'w'
    names = dict(base=base_all, light=base[:12], heavy=base[12:], head=head, tail=tail, extra=extra, over=over)
    _CACHE['names'] = names
    return names


def kb_names(which):
    """The names of KB `base`, `full` or `over` (fuzzy names, then the three uppercase ones)."""
    n = _build_names()
    out = list(n['base'])
    if which in ('full', 'over'):
        out += n['extra']
    if which == 'over':
        out.append(n['over'])
    assert which in ('base', 'full', 'over')
    return out + UPPERS


def fuzzy_names(which):
    return kb_names(which)[:-len(UPPERS)]


def processed(name_list):
    return {f'T{i}': {'aliases': {n: (None, None)}} for i, n in enumerate(name_list)}


def full_fillers():
    """Code points of no name whose home slot lies inside `full`'s probe chains (one at slot 255 or 254, one in the
    shared-slot chain): their lookup walks the chain, misses and must give 0x80."""
    key, val, _order = marker_table(kb_names('full'))
    plan = _plan()
    taken = {c for c in key if c is not None} | {plan['over_cp']} | {ord(c) for c in RESERVED}
    out = []
    for homes in ((255, 254), (plan['s_chain'], plan['s_chain'] + 1)):
        for c in list(range(0x100, 0x2000)) + list(range(0x4E00, 0x9000)):
            if slot(c) in homes and c not in taken and marker_lookup(key, val, c)[1] >= 3:
                out.append(chr(c))
                break
    return out


# ------------------------------------------------------------------------------------------------ tiling
class Unreachable(Exception):
    pass


class Tiler:
    """Concatenations of names of an exact byte (or code point) length."""

    def __init__(self, names, heavy):
        self.names = list(names)
        self.heavy = set(heavy)
        self.len = {'b': [len(n.encode()) for n in names], 'c': [len(n) for n in names]}
        self.reach = {u: self._reach(self.len[u], 20000 if u == 'b' else 4000) for u in 'bc'}

    @staticmethod
    def _reach(lens, top):
        r = np.zeros(top + 1, dtype=bool)
        r[0] = True
        for n in range(1, top + 1):
            r[n] = any(l <= n and r[n - l] for l in lens)
        return r

    def ok(self, n, unit='b'):
        return 0 <= n < len(self.reach[unit]) and bool(self.reach[unit][n])

    def tile(self, n, rng, unit='b', counts=None, cap=24, heavy=False, ascii_first=False):
        """Names of n bytes (code points) in all; counts: the field's occurrences per name so far, kept up to date."""
        if not self.ok(n, unit):
            raise Unreachable(n)
        counts = counts if counts is not None else collections.Counter()
        for _ in range(20):       # (a name left out or at its cap can leave a remainder that only it fits: again)
            trial = collections.Counter(counts)
            try:
                s = self._tile(n, rng, unit, trial, cap, heavy, ascii_first)
            except Unreachable:
                continue
            counts.update(trial - counts)
            return s
        raise Unreachable(n)

    def _tile(self, n, rng, unit, counts, cap, heavy, ascii_first):
        L, reach = self.len[unit], self.reach[unit]
        out, rem = [], n
        while rem:
            cands = [i for i, l in enumerate(L) if l <= rem and reach[rem - l] and counts[i] < cap
                     and not (ascii_first and not out and ord(self.names[i][0]) >= 0x80)]
            if not cands:
                raise Unreachable(n)
            if heavy and any(self.names[i] in self.heavy for i in cands):      # few occurrences: the long names
                cands = [i for i in cands if self.names[i] in self.heavy]
            i = rng.choice(cands)
            counts[i] += 1
            out.append(self.names[i])
            rem -= L[i]
        return ''.join(out)

    def compose(self, fb, pins, fe, rng, heavy=None, cap=24, ascii_first=False, exclude=()):
        """The field at arena bytes [fb, fe): each pin (arena offset, string) at its place, names between; a field
        of more than 1000 bytes takes the long names, to stay at or below MAX_OCC occurrences."""
        heavy = fe - fb > 1000 if heavy is None else heavy
        counts = collections.Counter({self.names.index(n): cap for n in exclude})
        out, cur = [], fb
        for at, s in sorted(pins):
            out.append(self.tile(at - cur, rng, counts=counts, cap=cap, heavy=heavy, ascii_first=ascii_first and not out))
            out.append(s)
            if s in self.names:
                counts[self.names.index(s)] += 1
            cur = at + len(s.encode())
        out.append(self.tile(fe - cur, rng, counts=counts, cap=cap, heavy=heavy, ascii_first=ascii_first and not out))
        return ''.join(out)

    def pin_char(self, fb, bound, w, k, rng, names=None):
        """A name placed so that one of its characters of w bytes has k bytes before arena offset `bound`; the
        bytes from fb to the name are reachable."""
        order = list(names if names is not None else self.names)
        rng.shuffle(order)
        for name in order:
            o = 0
            for ch in name:
                if width(ch) == w:
                    at = bound - k - o
                    if at == fb or self.ok(at - fb):
                        return at, name
                o += width(ch)
        raise Unreachable((fb, bound, w, k))

    def next_ok(self, n, unit='b'):
        while not self.ok(n, unit):
            n += 1
        return n


def near_occurrence(name, keep):
    """The name less one ASCII letter (not its first or last character, not index `keep`), and where `keep` went."""
    cands = [i for i in range(1, len(name) - 1) if name[i].isascii() and i != keep]
    i = cands[len(cands) // 2]
    return name[:i] + name[i + 1:], keep - (i < keep)


def pad_text(n, rng):
    s = ''.join(rng.choice(PAD) for _ in range(n))
    return s


def filler(nbytes):
    """nbytes >= 2 of non-ASCII code points of no name (0x80 in the view)."""
    three, two = {0: (nbytes // 3, 0), 1: ((nbytes - 4) // 3, 2), 2: ((nbytes - 2) // 3, 1)}[nbytes % 3]
    assert three >= 0 and 3 * three + 2 * two == nbytes
    return FILL3 * three + FILL2 * two


# ------------------------------------------------------------------------------------------------ the corpus
class _Builder:
    def __init__(self):
        self.texts, self.titles, self.tags = [], [], []
        self.cur = 0

    def add(self, text, title, tag):
        self.texts.append(text)
        self.titles.append(title)
        self.tags.append(tag)
        self.cur += len(text.encode()) + len(title.encode())

    def pad_to(self, align, rng, least=1):
        """An all-ASCII document in front, so that the next text starts at `align` modulo 16."""
        n = (align - self.cur - least) % 16 + least
        self.add(pad_text(n, rng), '', f'ascii pad of {n} bytes')


def _bound_name(kind):
    return {'lane': 'lane boundary', 'block1': 'block boundary 1024', 'block2': 'block boundary 2048'}[kind]


def _split_name(w, k):
    if k == 0:
        return f'{w}-byte char starting on'
    if k == w:
        return f'{w}-byte char ending on'
    return f'{w}-byte char split {k}|{w - k} over'


def corpus():
    """(texts, titles, tags): the documents of the sweep, the same for the three KBs."""
    if 'corpus' in _CACHE:
        return _CACHE['corpus']
    N = _build_names()
    T = Tiler(N['base'], N['heavy'])
    rng = random.Random('tx-geometry-corpus')
    small, big = [], []          # jobs: functions of the builder, run in an order that spreads the big documents

    def small_na(n=None):
        return T.tile(T.next_ok(n if n is not None else rng.randrange(90, 200)), rng)

    # ---- a: start alignments
    def job_a(v, first):
        def run(b):
            b.pad_to(v, rng)
            fb = b.cur
            tv = (v * 5 + 3) % 16
            n = next(x for x in range(2100 + rng.randrange(400), 4000) if (fb + x) % 16 == tv)
            lead = rng.choice(N['head']) if first == 'multi' else rng.choice(N['light'])
            text = T.compose(fb, [(fb, lead)], fb + n, rng)
            lead = rng.choice(N['head']) if first == 'multi' else rng.choice(N['light'])
            t0 = fb + n
            title = T.compose(t0, [(t0, lead)], t0 + T.next_ok(150 + rng.randrange(100)) + len(lead.encode()), rng)
            b.add(text, title, f'both/start alignment text fb%16={v} title fb%16={tv}, first char {first}')
        return run
    for v in range(16):
        for first in ('ascii', 'multi'):
            big.append(job_a(v, first))

    # ---- b: characters over, on and after the boundaries
    def job_b(where, kind, w, k):
        def run(b):
            if where == 'text':
                fb = b.cur
            else:
                text = small_na() if rng.random() < 0.5 else pad_text(rng.randrange(10, 60), rng)
                fb = b.cur + len(text.encode())
            base = fb & ~15
            bound = base + {'lane': 16 * rng.randrange(12, 60), 'block1': 1024, 'block2': 2048}[kind]
            heavy = True if where == 'title' or kind == 'block2' else None
            at, name = T.pin_char(fb, bound, w, k, rng, N['heavy'] if heavy else None)
            end = at + len(name.encode())
            field = T.compose(fb, [(at, name)], end + T.next_ok(100 + rng.randrange(60)), rng, heavy=heavy)
            tag = f'{where}/{_split_name(w, k)} {_bound_name(kind)}, fb%16={fb % 16}'
            if where == 'text':
                b.add(field, pad_text(rng.randrange(0, 30), rng) if rng.random() < 0.5 else '', tag)
            else:
                b.add(text, field, tag)
        return run
    for where in ('text', 'title'):
        for kind in ('lane', 'block1', 'block2'):
            for w, k in TOUCH:
                (small if kind == 'lane' else big).append(job_b(where, kind, w, k))

    # ---- c: field ends
    def job_c_end(q, r):
        def run(b):
            fb = b.cur
            fe = (fb & ~15) + 1024 * q + r
            if r == 0:
                text = T.compose(fb, [], fe, rng)
                tag = f'text/field end on block boundary {1024 * q}, fb%16={fb % 16}'
            else:
                last = N['tail'][min(r, 3) - 1]      # r = 1, 2, 3: 2, 3, 4 bytes, one before the boundary; 4: after it
                text = T.compose(fb, [(fe - len(last.encode()), last)], fe, rng)
                tag = (f'text/field end {r} past block boundary {1024 * q}, last char {width(last[-1])} bytes '
                       f'{"split 1|" + str(r) + " over" if r < 4 else "starting on"} it, fb%16={fb % 16}')
            b.add(text, '', tag)
        return run
    for q in (1, 2):
        for r in range(5):
            big.append(job_c_end(q, r))

    def job_c_chunk(v):
        def run(b):
            fb = b.cur
            n = next(x for x in range(180, 400) if (fb + x - (fb & ~15)) % 16 == v % 16 and T.ok(x))
            b.add(T.tile(n, rng), '', f'text/last 16-byte chunk holds {v} bytes, fb%16={fb % 16}')
        return run
    for v in (1, 15, 16):
        small.append(job_c_chunk(v))

    def job_c_13(b):
        b.pad_to(13, rng)
        b.add(N['tail'][1][-1], '', 'text/field of one 3-byte char inside one chunk from offset 13')
    small.append(job_c_13)

    # ---- d: output alignment of the title
    def job_d(v, tc, j):
        def run(b):
            n0 = (48 if j % 2 else 112) + v
            def cps(n, multi_first):      # (a multi-byte first character where the count allows: the permuted order's
                head = N['head'][j % 3]   #  start alignments need many such fields)
                if multi_first and T.ok(n - len(head), 'c'):
                    return head + T.tile(n - len(head), rng, unit='c')
                return T.tile(n, rng, unit='c')
            text = cps(n0, j % 2 == 0)
            if tc == 0:
                title = ''
            elif tc == 1:
                title = N['head'][j % 3][0]
            else:
                title = cps(tc, j % 4 < 2)
            b.add(text, title, f'both/text of {n0} code points (sh={n0 % 16}), title of {tc}')
        return run
    j = 0
    for v in range(16):
        for tc in TITLE_CPS:
            small.append(job_d(v, tc, j))
            j += 1

    def job_d_block(what):
        def run(b):
            fb = b.cur
            b1 = (fb & ~15) + 1024
            mid = FILL4 * 256 if what == 256 else pad_text(1024, rng)
            text = T.tile(b1 - fb, rng, heavy=True) + mid + small_na()
            b.add(text, '', f'text/block of {what} code points out at block boundary 1024, fb%16={fb % 16}')
        return run
    big.append(job_d_block(256))
    big.append(job_d_block(1024))

    # ---- e: which fields are non-ASCII
    small.append(lambda b: b.add(small_na(300), pad_text(20, rng), 'text/non-ASCII text, ASCII title'))
    small.append(lambda b: b.add(pad_text(300, rng), small_na(120), 'title/ASCII text, non-ASCII title'))
    small.append(lambda b: b.add(small_na(300), small_na(120), 'both/non-ASCII text and title'))
    small.append(lambda b: b.add('', small_na(120), 'title/empty text, non-ASCII title'))
    small.append(lambda b: b.add(N['head'][2][0], '', 'text/text of one 4-byte char'))
    small.append(lambda b: b.add(N['head'][2][0], pad_text(9, rng), 'text/text of one 4-byte char, ASCII title'))

    # ---- f: item classes
    def job_f_text(n_occ):
        def run(b):
            counts = collections.Counter()
            out = []
            while len(out) < n_occ:
                i = rng.choice([i for i in range(len(T.names)) if counts[i] < 24])
                counts[i] += 1
                out.append(T.names[i])
            b.add(''.join(out), '', f'text/{n_occ} occurrences in the text '
                                    f'({"big document" if n_occ > 512 else "one document at a time"})')
        return run
    for n_occ in (65, 200, 500, 530):
        big.append(job_f_text(n_occ))

    def job_f_title(b):
        counts = collections.Counter()
        out = []
        while len(out) < 70:
            i = rng.choice([i for i in range(12) if counts[i] < 24])
            counts[i] += 1
            out.append(T.names[i])
        b.add(small_na(), ''.join(out), 'title/70 occurrences in the title (big document)')
    big.append(job_f_title)

    # ---- g: the size bound
    def job_g(nbytes):
        def run(b):
            while not 8 <= len(b.texts) % 64 <= 55:          # in the middle of its 64-document group
                b.add(pad_text(rng.randrange(5, 40), rng), '', 'ascii document')
            fb = b.cur
            fe = fb + nbytes
            base = fb & ~15
            parts, cur = [], fb
            parts.append(T.tile(T.next_ok(600), rng, heavy=True))
            cur += len(parts[-1].encode())
            tail_n = T.next_ok(600)
            for q in range(1, 17):
                bound = base + 1024 * q
                if bound - 60 < cur + 2 or bound + 120 > fe - tail_n:
                    continue
                w, k = SPLITS[q % len(SPLITS)]
                at = None
                for name in T.names:                          # (any gap of >= 2 bytes takes the filler)
                    o = 0
                    for ch in name:
                        if width(ch) == w and at is None and bound - k - o - cur >= 2:
                            at, pick = bound - k - o, name
                        o += width(ch)
                    if at is not None:
                        break
                parts.append(filler(at - cur))
                parts.append(pick)
                cur = at + len(pick.encode())
            parts.append(filler(fe - tail_n - cur))
            parts.append(T.tile(tail_n, rng, heavy=True))
            text = ''.join(parts)
            assert len(text.encode()) == nbytes
            b.add(text, '', f'text/text of {nbytes} bytes (FK_CP_CAP {FK_CP_CAP}), names over every block boundary, '
                            f'fb%16={fb % 16}')
        return run
    g_jobs = [job_g(n) for n in (16383, 16384, 16385)]

    # ---- i: uppercase names with multi-byte neighbours over a lane boundary
    def job_i(u, side, word, w, k):
        def run(b):
            fb = b.cur
            nb = rng.choice((WORD_NB if word else NONWORD_NB)[w])
            other = '—'
            unit = (nb + u + other) if side == 'before' else (other + u + nb)
            o = 0 if side == 'before' else width(other) + len(u)          # the neighbour's byte offset in the unit
            bound = (fb & ~15) + 16 * rng.randrange(12, 40)
            at = next(bound - 16 * s - k - o for s in range(0, 8) if T.ok(bound - 16 * s - k - o - fb))
            end = at + len(unit.encode())
            text = T.compose(fb, [(at, unit)], end + T.next_ok(80), rng)
            b.add(text, '', f'text/uppercase {u} with {"word" if word else "non-word"} neighbour U+{ord(nb):04X} {side} it, '
                            f'{w}-byte char split {k}|{w - k} over lane boundary, fb%16={fb % 16}')
        return run
    n_i = 0
    for side in ('before', 'after'):
        for word in (True, False):
            for w, k in SPLITS:
                small.append(job_i(UPPERS[n_i % 3], side, word, w, k))
                n_i += 1
    for u in UPPERS:
        small.append(lambda b, u=u: b.add(u + '—' + small_na(), '', f'text/uppercase {u} first in the field'))
        small.append(lambda b, u=u: b.add(small_na() + '’' + u, pad_text(7, rng), f'text/uppercase {u} last in the field'))

    # ---- j: a name less one ASCII letter at the field's end, the name nowhere else in the field: it is decided
    # (reported without a position) by an edge window on the decoded code points, here the view's bytes themselves
    def job_j(kind, w, k, cp):
        def run(b):
            fb = b.cur
            base = fb & ~15
            bound = base + {'lane': 16 * rng.randrange(12, 60), 'block1': 1024, 'block2': 2048, None: 0}[kind]
            order = [n for n in N['base'][:18] if len(n) >= 11 and (cp is None or cp in n)]
            rng.shuffle(order)
            for name in order:
                for idx, ch in enumerate(name):
                    if (cp is None and width(ch) != w) or (cp is not None and ch != cp):
                        continue
                    near, at_idx = near_occurrence(name, idx)
                    o = len(near[:at_idx].encode())
                    if cp is not None:
                        at = fb + T.next_ok(150 + rng.randrange(100))
                    else:
                        at = bound - k - o
                    try:
                        text = T.compose(fb, [(at, near)], at + len(near.encode()), rng, exclude=[name])
                    except Unreachable:
                        continue
                    if cp is not None:
                        tag = f'text/ends with a name less one letter that holds U+{ord(cp):04X} (marker probe chain), fb%16={fb % 16}'
                    else:
                        tag = (f'text/ends with a name less one letter, its {_split_name(w, k)} {_bound_name(kind)}, '
                               f'fb%16={fb % 16}')
                    b.add(text, '', tag)
                    return
            raise Unreachable((kind, w, k, cp))
        return run
    for kind in ('lane', 'block1', 'block2'):
        for w, k in SPLITS:
            (small if kind == 'lane' else big).append(job_j(kind, w, k, None))
    for c in _plan()['special']:
        small.append(job_j(None, 0, 0, chr(c)))

    # ---- the other KBs' names and the marker table's fillers (code points of no name in KB base)
    def job_extra(names, what, in_title):
        def run(b):
            parts = []
            for n in names:
                parts += [small_na(60), n]
            s = ''.join(parts) + small_na(60)
            b.add(small_na(100) if in_title else s, s if in_title else '', f'{"title" if in_title else "text"}/{what}')
        return run
    ex = N['extra']
    for i in range(0, len(ex), 2):
        small.append(job_extra(ex[i:i + 2], 'names of KB full only', i % 4 == 2))
    for in_title in (False, True, False):
        small.append(job_extra([N['over']], 'the name with the 128th code point (KB over)', in_title))
    fl = full_fillers()
    for i in range(4):
        def run(b, i=i):
            s = small_na(80) + fl[i % 2] + small_na(80) + fl[(i + 1) % 2] + fl[i % 2] + small_na(40)
            b.add(s if i % 2 == 0 else pad_text(12, rng), '' if i % 2 == 0 else s,
                  f'{"text" if i % 2 == 0 else "title"}/filler code points inside the marker table\'s probe chains')
        small.append(run)

    # ---- the order: the big documents spread evenly, an ASCII document after every fourth, the 16 KiB texts in
    # the middle of three different groups
    rng.shuffle(small)
    rng.shuffle(big)
    jobs = list(small)
    for i, jb in enumerate(big):
        jobs.insert(min(len(jobs), i * (len(small) + len(big)) // len(big)), jb)
    for i, jb in enumerate(g_jobs):
        jobs.insert((i + 1) * len(jobs) // 4, jb)
    b = _Builder()
    for i, jb in enumerate(jobs):
        jb(b)
        if i % 4 == 3:
            b.add(pad_text(rng.randrange(1, 48), rng), pad_text(rng.randrange(0, 12), rng), 'ascii document')
    while len(b.texts) % 64 in (0, 63) or len(b.texts) < 300:
        b.add(pad_text(rng.randrange(1, 48), rng), '', 'ascii document')
    _CACHE['corpus'] = (b.texts, b.titles, b.tags)
    return _CACHE['corpus']


def generic_corpus():
    """Every text with 65 occurrences of one uppercase name appended: the generic kernel's documents."""
    texts, titles, tags = corpus()
    many = ' ' + ' '.join([GENERIC_UPPER] * 65)
    return [t + many for t in texts], titles, tags


def permuted_corpus(seed=None):
    """The documents in a seeded permutation, an empty document after every 31st; src = the source document or -1.
    seed None: the first seed whose packing still hits every cell of families a and d."""
    texts, titles, tags = corpus()
    if seed is None:
        if 'perm_seed' not in _CACHE:
            for s in range(200):
                t2, i2, _g2, _src = permuted_corpus(s)
                arena, off = pack_fields(t2, i2)
                if not missing_a(cells_a(arena, off)) and not missing_d(cells_d(arena, off)):
                    _CACHE['perm_seed'] = s
                    break
        seed = _CACHE['perm_seed']
    order = list(range(len(texts)))
    random.Random(f'tx-geometry-permutation-{seed}').shuffle(order)
    ot, oi, og, src = [], [], [], []
    for k, d in enumerate(order):
        ot.append(texts[d])
        oi.append(titles[d])
        og.append(tags[d] + f' (source document {d})')
        src.append(d)
        if k % 31 == 30:
            ot.append('')
            oi.append('')
            og.append('empty document')
            src.append(-1)
    return ot, oi, og, src


# ------------------------------------------------------------------------------------------------ predicates
def _fields(arena, off):
    """Per field: document, field index, fb, fe, has a non-ASCII byte, its document has a non-ASCII field."""
    n = (len(off) - 1) // 2
    hi = np.concatenate([[0], np.cumsum(arena >= 0x80)])
    cnt = hi[off[1:]] - hi[off[:-1]]
    na = cnt > 0
    doc_na = na[0::2] | na[1::2]
    return [(i // 2, i % 2, int(off[i]), int(off[i + 1]), bool(na[i]), bool(doc_na[i // 2])) for i in range(2 * n)]


def _leads(arena, fb, fe):
    a = arena[fb:fe]
    return (a & 0xC0) != 0x80


def _cw(b0):
    return 1 if b0 < 0x80 else 2 if b0 < 0xE0 else 3 if b0 < 0xF0 else 4


def cells_a(arena, off):
    out = set()
    for _d, f, fb, fe, _na, dna in _fields(arena, off):
        if dna and fe > fb:
            out.add(('title' if f else 'text', fb % 16, 'multi' if arena[fb] >= 0x80 else 'ascii'))
    return out


def missing_a(cells):
    return [(w, v, c) for w in ('text', 'title') for v in range(16) for c in ('ascii', 'multi') if (w, v, c) not in cells]


def cells_b(arena, off):
    out = set()
    for _d, f, fb, fe, na, _dna in _fields(arena, off):
        if not na:
            continue
        base = fb & ~15
        a = arena[fb:fe]
        for p in (np.flatnonzero(a >= 0xC0) + fb).tolist():
            w = _cw(int(arena[p]))
            e = p + w
            hits = []
            if p % 16 == 0:
                hits.append((p, 0))
            if e % 16 == 0:
                hits.append((e, w))
            if p // 16 != (e - 1) // 16:
                bd = (e - 1) // 16 * 16
                hits.append((bd, bd - p))
            for bd, k in hits:
                rel = bd - base
                if not fb < bd < fe:
                    continue
                kind = 'block1' if rel == 1024 else 'block2' if rel == 2048 else 'lane' if rel % 1024 else None
                if kind:
                    out.add(('title' if f else 'text', kind, w, k))
    return out


def missing_b(cells):
    return [(wh, kind, w, k) for wh in ('text', 'title') for kind in ('lane', 'block1', 'block2') for w, k in TOUCH
            if (wh, kind, w, k) not in cells]


def cells_c(arena, off):
    out = set()
    for _d, _f, fb, fe, na, _dna in _fields(arena, off):
        if not na:
            continue
        base = fb & ~15
        lead = _leads(arena, fb, fe)
        last = fb + int(np.flatnonzero(lead)[-1])          # the last character's first byte
        for q in (1, 2):
            r = fe - (base + 1024 * q)
            if r == 0:
                out.add(('end_on', q))
            if 1 <= r <= 3 and last < base + 1024 * q:
                out.add(('end_past', q, r))
            if r == 4 and last == base + 1024 * q:
                out.add(('end_past', q, 4))
        if fe - base > 16:
            out.add(('last_chunk', (fe - base - 1) % 16 + 1))
        if fb % 16 == 13 and fe <= base + 16:
            out.add(('one_chunk_13',))
    return out


def missing_c(cells):
    want = [('end_on', q) for q in (1, 2)] + [('end_past', q, r) for q in (1, 2) for r in (1, 2, 3, 4)]
    want += [('last_chunk', v) for v in (1, 15, 16)] + [('one_chunk_13',)]
    return [c for c in want if c not in cells]


def cells_d(arena, off):
    out = set()
    cps = {}
    for d, f, fb, fe, na, dna in _fields(arena, off):
        if not dna:
            continue
        lead = _leads(arena, fb, fe)
        cps[(d, f)] = int(lead.sum())
        if f == 1:
            out.add((cps[(d, 0)] % 16, cps[(d, 1)]))
        if na:
            base = fb & ~15
            for blk in range(base, fe, 1024):
                lo, hi = max(blk, fb), min(blk + 1024, fe)
                n = int(lead[lo - fb:hi - fb].sum())
                if blk > base and n < 16:
                    out.add(('short_block',))
                if lo == blk and hi == blk + 1024 and n in (256, 1024):
                    out.add(('block', n))
    return out


def missing_d(cells):
    want = [(v, tc) for v in range(16) for tc in TITLE_CPS] + [('short_block',), ('block', 256), ('block', 1024)]
    return [c for c in want if c not in cells]


def cells_e(arena, off):
    out = set()
    f = _fields(arena, off)
    for (d, _0, fb0, fe0, na0, _a), (_d, _1, fb1, fe1, na1, _b) in zip(f[0::2], f[1::2]):
        if na0 and not na1 and fe1 > fb1:
            out.add('text_only')
        if na1 and not na0 and fe0 > fb0:
            out.add('title_only')
        if na0 and na1:
            out.add('both')
        if na1 and fe0 == fb0:
            out.add('empty_text')
        if na0 and fe0 - fb0 == 4 and arena[fb0] >= 0xF0:
            out.add('one_4byte_text')
    return out


def missing_e(cells):
    return [c for c in ('text_only', 'title_only', 'both', 'empty_text', 'one_4byte_text') if c not in cells]


def occurrences(s, names):
    return sum(len(re.findall(re.escape(n), s)) for n in names)


def item_classes(texts, titles, names):
    """Per document, from its occurrences of the fuzzy names (each is at least one item on the GPU): 'batch' (at most
    64 in either field), 'wave' (a text of 65..512), 'big' (a text of more than 512 or a title of more than 64)."""
    out = []
    for a, b in zip(texts, titles):
        n0, n1 = occurrences(a, names), occurrences(b, names)
        out.append('big' if n0 > 512 or n1 > 64 else 'wave' if n0 > 64 else 'batch')
    return out


def cells_f(arena, off, names):
    out = set()
    per_name = 0
    raw = arena.tobytes()
    for _d, f, fb, fe, na, _dna in _fields(arena, off):
        if not na:
            continue
        s = raw[fb:fe].decode('utf-8')
        each = [len(re.findall(re.escape(n), s)) for n in names]
        n = sum(each)
        per_name = max(per_name, max(each))
        if f == 0:
            out.add('text<=64' if n <= 64 else 'text65..512' if n <= 512 else 'text>512')
        elif n > 64:
            out.add('title>64')
    if per_name <= 30:
        out.add('name<=30')
    return out


def missing_f(cells):
    return [c for c in ('text<=64', 'text65..512', 'text>512', 'title>64', 'name<=30') if c not in cells]


def tx_need(fb0, fe0, fb1, fe1, na0, na1):
    """Bytes of tarena kw_tx_kernel takes for a document (view bytes, then the u16 chunk tables)."""
    nb = ((fe0 - fb0) + (fe1 - fb1) + 16 + 15) & ~15
    nch = lambda fb, fe: ((fe - (fb & ~15) + 15) >> 4) + 1
    nc = (nch(fb0, fe0) if na0 else 0) + (nch(fb1, fe1) if na1 else 0)
    return nb + ((2 * nc + 15) & ~15)


def cells_g(arena, off):
    out = set()
    f = _fields(arena, off)
    for (d, _0, fb0, fe0, na0, _a), (_d, _1, fb1, fe1, na1, _b) in zip(f[0::2], f[1::2]):
        n = fe0 - fb0
        if na0 and n in (16383, 16384, 16385) and 8 <= d % 64 <= 55:
            if n > FK_CP_CAP or tx_need(fb0, fe0, fb1, fe1, na0, na1) > TX_SLAB:
                out.add(n)
    return out


def missing_g(cells):
    return [n for n in (16383, 16384, 16385) if n not in cells]


def cells_h(arena, off):
    """'count', and per full 64-document group 'holes' (ASCII documents among the non-ASCII ones) and 'slabs' (the
    group's wave claims at least two slabs); the names of the cells a corpus misses come from missing_h."""
    out = set()
    f = _fields(arena, off)
    n = len(f) // 2
    if n >= 300 and n % 64:
        out.add('count')
    for g in range(n // 64):
        slab = end = claims = 0
        nna = 0
        for d in range(64 * g, 64 * g + 64):
            (_d, _0, fb0, fe0, na0, _a), (_e, _1, fb1, fe1, na1, _b) = f[2 * d], f[2 * d + 1]
            if not (na0 or na1):
                continue
            nna += 1
            if (na0 and fe0 - fb0 > FK_CP_CAP) or (na1 and fe1 - fb1 > FK_CP_CAP):
                continue
            need = tx_need(fb0, fe0, fb1, fe1, na0, na1)
            if slab + need > end:
                slab, end = 0, max(need, TX_SLAB)
                claims += 1
            slab += need
        if 0 < nna < 64:
            out.add(('holes', g))
        if claims >= 2:
            out.add(('slabs', g))
    return out


def missing_h(cells, n_docs):
    want = ['count'] + [(k, g) for g in range(n_docs // 64) for k in ('holes', 'slabs')]
    return [c for c in want if c not in cells]


def cells_i(arena, off, uppers=UPPERS):
    out = set()
    raw = arena.tobytes()
    for _d, _f, fb, fe, na, _dna in _fields(arena, off):
        if not na:
            continue
        fld = raw[fb:fe]
        for u in uppers:
            ub = u.encode()
            for m in re.finditer(re.escape(ub), fld):
                s, e = fb + m.start(), fb + m.end()
                if s == fb:
                    out.add(('first', u))
                if e == fe:
                    out.add(('last', u))
                if s > fb and arena[s - 1] >= 0x80:
                    p = s - 1
                    while (arena[p] & 0xC0) == 0x80:
                        p -= 1
                    out |= _nb_cell(raw, p, s, 'before')
                if e < fe and arena[e] >= 0x80:
                    out |= _nb_cell(raw, e, e + _cw(int(arena[e])), 'after')
    return out


def _nb_cell(raw, p, e, side):
    ch = raw[p:e].decode('utf-8')
    if p // 16 == (e - 1) // 16:
        return set()
    bd = (e - 1) // 16 * 16
    return {(side, 'word' if re.match(r'\w', ch) else 'non-word', e - p, bd - p)}


def missing_i(cells):
    want = [(side, cls, w, k) for side in ('before', 'after') for cls in ('word', 'non-word') for w, k in SPLITS]
    want += [(k, u) for k in ('first', 'last') for u in UPPERS]
    return [c for c in want if c not in cells]


def cells_j(arena, off, names):
    """Fields that end with a name less one ASCII letter and hold the name nowhere: (boundary, w, k) of the
    multi-byte characters of that ending over a boundary, and ('cp', code point) of its chain and wrap code points."""
    out = set()
    raw = arena.tobytes()
    special = {chr(c) for c in _plan()['special']}
    for _d, _f, fb, fe, na, _dna in _fields(arena, off):
        if not na or fe - fb < 40:
            continue
        s = raw[fb:fe].decode('utf-8')
        for n in names:
            if len(n) < 11 or n in s:
                continue
            for i in range(1, len(n) - 1):
                v = n[:i] + n[i + 1:]
                if not (n[i].isascii() and s.endswith(v)):
                    continue
                base = fb & ~15
                p = fe - len(v.encode())
                for ch in v:
                    w = width(ch)
                    if ch in special:
                        out.add(('cp', ord(ch)))
                    if w > 1 and p // 16 != (p + w - 1) // 16:
                        bd = (p + w - 1) // 16 * 16
                        rel = bd - base
                        kind = 'block1' if rel == 1024 else 'block2' if rel == 2048 else 'lane' if rel % 1024 else None
                        out.add((kind, w, bd - p))
                    p += w
                break
    return out


def missing_j(cells):
    want = [(kind, w, k) for kind in ('lane', 'block1', 'block2') for w, k in SPLITS]
    want += [('cp', c) for c in _plan()['special']]
    return [c for c in want if c not in cells]


def coverage(texts, titles, names):
    """family -> the cells the corpus misses (all empty: every cell is hit)."""
    arena, off = pack_fields(texts, titles)
    return {'a': missing_a(cells_a(arena, off)), 'b': missing_b(cells_b(arena, off)),
            'c': missing_c(cells_c(arena, off)), 'd': missing_d(cells_d(arena, off)),
            'e': missing_e(cells_e(arena, off)), 'f': missing_f(cells_f(arena, off, names)),
            'g': missing_g(cells_g(arena, off)), 'h': missing_h(cells_h(arena, off), len(texts)),
            'i': missing_i(cells_i(arena, off)), 'j': missing_j(cells_j(arena, off, names))}
