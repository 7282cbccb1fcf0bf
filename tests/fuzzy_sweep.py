"""The partial_ratio > 95 boundary sweep: names of every length 8..64 and, for each, fields holding the name
with every small number of deletions and insertions, at every edit placement and every field edge where the
kernels' derived bounds (kfull, dmax, the staged window of base +- 2k, the prefix / suffix window rules, the
edge table of one-deletion variants, SHORT_EXACT_MAX, the 64-code-point cap) step.

Pure Python: no GPU, no oracle.  Everything is deterministic (string-seeded random.Random, no set or hash
order).  tests/test_fuzzy_sweep_cases.py holds the oracle against its brute force on these cases and checks
that they straddle the threshold; tests/test_gpu_fuzzy_sweep.py sends them through every kernel route.

A case is one field string built from one intended name; its tags say how:

    kind    indel | subst | transp | clip | short | cap64 | na | rep_del | rep_dup
    family  a | b (the two seeds) | na (non-ASCII names) | rep (names with runs)
    m       code points of the name
    nd, ni  deletions and insertions (a substitution is one of each, a transposition too)
    edit    where the edits sit in the name: none | after_first | before_last | spread | touch_first | touch_last
    place   where the variant sits in the field: middle | start | end | whole | gap_start | gap_end
    gap     filler code points between the variant and the field edge (gap_start / gap_end)
    clip    code points dropped at the name's first (+c) or last (-c) end, 0 = none
"""
import random
from collections import namedtuple

ALPHA = 'abcdefghilmnoprstuy'            # the names' letters: none of FILL's
FILL = 'zq vj xk wq zj qx vk jz'         # no name shares a 4-gram (nor a letter) with it
FILLC = FILL + ' '
GAPC = 'zqvjxkwqzjqxvkjz'                # the filler of the 1..7-code-point gaps: no space at a field edge
INS = '#%'                               # inserted characters: in no name and not in the filler
KEY_LENGTHS = (10, 11, 20, 21, 30, 31, 40, 41, 50, 51, 60, 61, 64)   # never thinned
LENGTHS = tuple(range(8, 65))
NA_LENGTHS = (11, 20, 21, 40, 41, 60, 61, 64)
REP_LENGTHS = (11, 20, 21, 41, 64)
EDITS = ('after_first', 'before_last', 'spread', 'touch_first', 'touch_last')
MAX_DOCS = 30000
MAX_DOC_BYTES = 400

Case = namedtuple('Case', 'field name variant tags')


def kfull(m):
    """Unmatched name code points a full window may have: the largest k with 20 k < m."""
    k = 0
    while 20 * (k + 1) < m:
        k += 1
    return k


def dmax(m):
    """The indel budget of any window of the family (csrc/kwmatch.hip dmax_h)."""
    return max(2 * kfull(m), (2 * m - 2) // 20)


# ------------------------------------------------------------------------------------------------ names
def _make_name(family, m):
    """Letters and single spaces, first letter uppercase, no code point (case folded) within the six before it."""
    rng = random.Random(f'fuzzy-sweep-{family}-{m}')
    out = [rng.choice(ALPHA).upper()]
    since_space = 1
    while len(out) < m:
        i = len(out)
        recent = {c.lower() for c in out[-6:]}
        if ' ' not in recent and since_space >= 4 and i < m - 3 and rng.random() < 0.3:
            out.append(' ')
            since_space = 0
            continue
        out.append(rng.choice([c for c in ALPHA if c not in recent]))
        since_space += 1
    return ''.join(out)


def names(family):
    """length -> name, for every length 8..64."""
    return {m: _make_name(family, m) for m in LENGTHS}


def nonascii_names():
    """length -> a name with two or three of e-acute, u-umlaut, sharp s, one of them in the first four."""
    out = {}
    for m in NA_LENGTHS:
        cps = list(_make_name('na', m))
        spots = [(1, 'é'), (m // 2, 'ü')] + ([(m - 3, 'ß')] if m >= 40 else [])
        for p, c in spots:
            if cps[p] == ' ':
                p += 1
            cps[p] = c
        out[m] = ''.join(cps)
    return out


def repeat_names():
    """length -> a name made of runs (aaa, abab, ee ...): ambiguous LCS alignments, equal neighbours."""
    chunks = ['aaa', 'b', 'abab', ' ', 'cc', 'dede', 'r', ' ', 'ooo', 'stst', 'n', ' ', 'ee', 'lili', 'mmm', ' ']
    out = {}
    for m in REP_LENGTHS:
        s = 'B'
        i = m          # (a different phase of the chunk cycle for each length)
        while len(s) < m:
            s += chunks[i % len(chunks)]
            i += 1
        s = s[:m]
        if s[-1] == ' ':
            s = s[:-1] + 'u'
        out[m] = s
    return out


def kb_small():
    """The 57 names of family a: at most 64 fuzzy names are as long as any field (the short-field pretest)."""
    return [names('a')[m] for m in LENGTHS]


def kb_big():
    """Both families and the two small ones: more than 64 fuzzy names for fields of up to 32 code points."""
    a, b, na, rep = names('a'), names('b'), nonascii_names(), repeat_names()
    return ([a[m] for m in LENGTHS] + [b[m] for m in LENGTHS] + [na[m] for m in NA_LENGTHS]
            + [rep[m] for m in REP_LENGTHS])


def processed(name_list):
    return {f'T{i}': {'aliases': {n: (None, None)}} for i, n in enumerate(name_list)}


# ------------------------------------------------------------------------------------------------ variants
def _ins(n):
    return (INS * n)[:n]


def _spread_positions(m, e):
    """e distinct interior positions 1..m-2, evenly spread."""
    pos = [(j + 1) * m // (e + 1) for j in range(e)]
    pos = [min(max(p, 1), m - 2) for p in pos]
    assert len(set(pos)) == e, (m, e, pos)
    return pos


def indel_variant(name, nd, ni, edit):
    m = len(name)
    if nd + ni == 0:
        return name
    if edit == 'after_first':        # insertions directly after the first code point, deletions one further on
        return name[0] + _ins(ni) + name[1:2] + name[2 + nd:]
    if edit == 'before_last':
        return name[:m - 2 - nd] + name[m - 2:m - 1] + _ins(ni) + name[-1]
    if edit == 'touch_first':        # the first code points themselves go; insertions in front of the rest
        return _ins(ni) + name[nd:]
    if edit == 'touch_last':
        return name[:m - nd] + _ins(ni)
    assert edit == 'spread'
    ops = []                         # deletions and insertions alternate over the spread positions
    d, i = nd, ni
    while d or i:
        if d:
            ops.append('d')
            d -= 1
        if i:
            ops.append('i')
            i -= 1
    cps = list(name)
    for p, op in sorted(zip(_spread_positions(m, nd + ni), ops), reverse=True):
        if op == 'd':
            del cps[p]
        else:
            cps.insert(p, INS[p % 2])
    return ''.join(cps)


def subst_variant(name, s):
    cps = list(name)
    for j, p in enumerate(_spread_positions(len(name), s)):
        cps[p] = INS[j % 2]
    return ''.join(cps)


def transp_variant(name, t):
    cps = list(name)
    for p in _spread_positions(len(name) - 1, t):      # p and p + 1 are interior: 1 <= p, p + 1 <= m - 2
        cps[p], cps[p + 1] = cps[p + 1], cps[p]
    return ''.join(cps)


def clip_variant(name, side, c, extra):
    v = name[c:] if side == 'first' else name[:len(name) - c]
    p = len(v) // 2
    if extra == 'del':
        v = v[:p] + v[p + 1:]
    elif extra == 'ins':
        v = v[:p] + INS[0] + v[p:]
    return v


# ------------------------------------------------------------------------------------------------ fields
def _left(n):
    s = (FILLC * 4).rstrip()
    return s[len(s) - n:] if n else ''


def _right(n):
    return (FILLC * 4)[:n]


SIDE = 30      # filler code points on a side that is not an edge


def build_field(variant, place, gap=0, side=SIDE):
    if place == 'middle':
        return _left(side) + variant + _right(side)
    if place == 'start':
        return variant + _right(side)
    if place == 'end':
        return _left(side) + variant
    if place == 'whole':
        return variant
    assert 1 <= gap <= len(GAPC)
    if place == 'gap_start':
        return GAPC[len(GAPC) - gap:] + variant + _right(side)
    assert place == 'gap_end'
    return _left(side) + variant + GAPC[:gap]


def _gaps(m):
    k = kfull(m)
    return sorted({g for g in (1, 2, 2 * k, 2 * k + 1) if g >= 1})


def _places(m, full):
    out = [('middle', 0), ('start', 0), ('end', 0), ('whole', 0)]
    if full:
        out += [(p, g) for g in _gaps(m) for p in ('gap_start', 'gap_end')]
    return out


def _tags(kind, family, m, nd, ni, edit, place, gap=0, clip=0):
    return {'kind': kind, 'family': family, 'm': m, 'nd': nd, 'ni': ni, 'edit': edit, 'place': place, 'gap': gap,
            'clip': clip}


# ------------------------------------------------------------------------------------------------ the sweep
def _indel_cases(family, nm):
    out = []
    for m in LENGTHS:
        name, k = nm[m], kfull(m)
        key = m in KEY_LENGTHS
        for nd in range(k + 2):
            for ni in range(k + 2):
                if nd + ni == 0:
                    edits = ('none',)
                elif family == 'a' and key:
                    edits = EDITS
                elif family == 'a':
                    # the other lengths: the packed placement and the touched end alternate with the length; spread
                    # is thinned to the single edits and the edit counts around the threshold
                    edits = ('after_first', 'touch_last') if m % 2 else ('before_last', 'touch_first')
                    if nd + ni == 1 or (max(nd, ni) >= k and min(nd, ni) <= 1):
                        edits += ('spread',)
                else:
                    edits = ('spread',) if key or abs(nd - ni) <= 1 else ()
                for edit in edits:
                    if edit.startswith('touch') and nd == 0:
                        continue             # (only a deletion touches the end code point itself)
                    v = indel_variant(name, nd, ni, edit)
                    if family == 'a' and key:
                        places = _places(m, True)
                    elif family == 'a':
                        # the field edge on the side of the edits, the middle, and the whole field for the spread
                        far = edit in ('before_last', 'touch_last')
                        places = [('middle', 0), ('end', 0) if far else ('start', 0)]
                        if edit in ('spread', 'none'):
                            places = _places(m, False)
                        elif edit.startswith('touch') and ni <= 1:
                            places.append(('whole', 0))      # (a field shorter than the name: the roles swap)
                    else:
                        places = [('middle', 0), ('whole', 0)]
                    for place, gap in places:
                        out.append(Case(build_field(v, place, gap), name, v,
                                        _tags('indel', family, m, nd, ni, edit, place, gap)))
    return out


def _subst_transp_cases(nm):
    out = []
    for m in LENGTHS:
        name, k = nm[m], kfull(m)
        for s in range(1, k + 2):
            for kind, v in (('subst', subst_variant(name, s)), ('transp', transp_variant(name, s))):
                for place in ('middle', 'start', 'whole') if m % 2 else ('middle', 'end', 'whole'):
                    out.append(Case(build_field(v, place), name, v, _tags(kind, 'a', m, s, s, 'spread', place)))
    return out


def _clip_cases(nm):
    out = []
    for m in LENGTHS:
        name = nm[m]
        for side, place in (('first', 'start'), ('last', 'end')):
            for c in range(1, dmax(m) + 2):
                for extra in ('none', 'del', 'ins'):
                    v = clip_variant(name, side, c, extra)
                    nd, ni = (1, 0) if extra == 'del' else (0, 1) if extra == 'ins' else (0, 0)
                    clip = c if side == 'first' else -c
                    places = [place] + (['middle'] if extra == 'none' and m in KEY_LENGTHS else [])
                    for pl in places:
                        out.append(Case(build_field(v, pl), name, v, _tags('clip', 'a', m, nd, ni, extra, pl, 0, clip)))
    return out


def _cap64_cases(nm):
    """The 64-code-point name, exact and with 1..7 edits, in fields of exactly 64 and 65 code points."""
    out = []
    name = nm[64]
    for e in range(8):
        for nd, ni in sorted({(e, 0), (e - e // 2, e // 2), (0, e)}):
            v = indel_variant(name, nd, ni, 'spread')
            for n in (64, 65):
                pad = n - len(v)
                if pad < 0:
                    continue
                for place, field in (('gap_end', v + GAPC[:pad]), ('gap_start', GAPC[len(GAPC) - pad:] + v if pad else v)):
                    if pad == 0 and place == 'gap_start':
                        continue
                    assert len(field) == n
                    out.append(Case(field, name, v, _tags('cap64', 'a', 64, nd, ni, 'spread',
                                                          place if pad else 'whole', pad)))
    return out


def _short_cases(nm):
    """Fields of exactly 10 and 11 code points (SHORT_EXACT_MAX and one more): a substring of a longer name, one
    with a substitution, and a substring one longer with one code point deleted."""
    out = []
    for m in (12, 20, 21, 40, 64):
        name = nm[m]
        for L in (10, 11):
            for o in sorted({0, (m - L - 1) // 2, m - L - 1}):
                sub, sub1 = name[o:o + L], name[o:o + L + 1]
                fields = [('none', 0, 0, sub), ('subst', 1, 1, sub[:L // 2] + INS[0] + sub[L // 2 + 1:])]
                fields += [(f'del{p}', 1, 0, sub1[:p] + sub1[p + 1:]) for p in (1, L // 2, L - 1)]
                if o == 0:
                    fields.append(('none_tail', 0, 0, name[m - L:]))
                for edit, nd, ni, f in fields:
                    assert len(f) == L
                    out.append(Case(f, name, f, _tags('short', 'a', m, nd, ni, edit, 'whole', L)))
    return out


def nonascii_cases():
    """The non-ASCII names with edits that delete, replace and insert at their non-ASCII code points, alone and
    with one more deletion elsewhere (the threshold of the names of 21 and more)."""
    out = []
    for m, name in nonascii_names().items():
        marks = [p for p, c in enumerate(name) if ord(c) > 127]
        assert 2 <= len(marks) <= 3 and marks[0] < 4
        variants = [('none', 0, 0, name)]
        for p in marks:
            other = 'ü' if name[p] != 'ü' else 'é'
            variants += [(f'del@{p}', 1, 0, name[:p] + name[p + 1:]),
                         (f'rep#@{p}', 1, 1, name[:p] + '#' + name[p + 1:]),
                         (f'repΩ@{p}', 1, 1, name[:p] + 'Ω' + name[p + 1:]),
                         (f'repmark@{p}', 1, 1, name[:p] + other + name[p + 1:]),
                         (f'ins#@{p}', 0, 1, name[:p] + '#' + name[p:]),
                         (f'insmark@{p}', 0, 1, name[:p + 1] + other + name[p + 1:])]
        for edit, nd, ni, v in variants:
            q = 3 * len(v) // 4
            for extra, v2 in ((0, v), (1, v[:q] + v[q + 1:])):
                for place in ('middle', 'start', 'end', 'whole'):
                    out.append(Case(build_field(v2, place), name, v2,
                                    _tags('na', 'na', m, nd + extra, ni, edit, place)))
    return out


def repeat_cases():
    """The names with runs: every single deletion (the edge table skips the variant equal to its neighbour's) and
    every doubled code point."""
    out = []
    for m, name in repeat_names().items():
        places = ('start', 'end', 'whole', 'middle') if m <= 21 else ('middle', 'whole')
        for p in range(m):
            for kind, nd, ni, v in (('rep_del', 1, 0, name[:p] + name[p + 1:]),
                                    ('rep_dup', 0, 1, name[:p] + name[p] + name[p:])):
                if kind == 'rep_dup' and m <= 21 and p % 2:
                    continue
                for place in places:
                    out.append(Case(build_field(v, place), name, v, _tags(kind, 'rep', m, nd, ni, f'@{p}', place)))
        out.append(Case(name, name, name, _tags('rep_del', 'rep', m, 0, 0, 'none', 'whole')))
    return out


def _check_filler(all_names):
    grams = set()
    for n in all_names:
        grams.update(n[i:i + 4] for i in range(len(n) - 3))
    for filler in (FILLC * 4, GAPC, FILL + ' ' + FILL):
        shared = [filler[i:i + 4] for i in range(len(filler) - 3) if filler[i:i + 4] in grams]
        assert not shared, shared
    for n in all_names:
        assert not set(INS) & set(n)
    assert not set(INS) & set(FILLC + GAPC)


def _check_names():
    for fam in ('a', 'b'):
        for m, n in names(fam).items():
            assert len(n) == m and n[0].isupper() and n[1:] == n[1:].lower() and '  ' not in n and n == n.strip(), n
            assert set(n.lower()) <= set(ALPHA + ' ')
            assert not n.isupper() and not n.islower()          # the fuzzy class
            low = n.lower()
            for i in range(1, m):
                assert low[i] not in low[max(0, i - 6):i], (n, i)
    big = kb_big()
    assert len(set(big)) == len(big) == 2 * len(LENGTHS) + len(NA_LENGTHS) + len(REP_LENGTHS)
    assert len(kb_small()) == 57 and 2 * len(LENGTHS) == 114
    for n in big:
        assert not n.isupper() and not n.islower() and len(n) <= 64
    for m, n in list(nonascii_names().items()) + list(repeat_names().items()):
        assert len(n) == m and n == n.strip() and '  ' not in n, n
    _check_filler(big)


_CACHE = {}


def ascii_cases(family=None):
    """The all-ASCII cases (families a and b): the main sweep."""
    if 'ascii' not in _CACHE:
        _check_names()
        a, b = names('a'), names('b')
        _CACHE['ascii'] = (_indel_cases('a', a) + _subst_transp_cases(a) + _clip_cases(a) + _cap64_cases(a)
                           + _short_cases(a) + _indel_cases('b', b))
    cs = _CACHE['ascii']
    return [c for c in cs if c.tags['family'] == family] if family else list(cs)


def all_cases():
    return ascii_cases() + repeat_cases() + nonascii_cases()


def documents(cases):
    """(texts, titles, tags): every case once as the text and once as the title, the other field filler; every
    fourth case as one document with the variant in both fields.  tags[d] is the case's tags plus 'in'."""
    texts, titles, tags = [], [], []

    def add(text, title, t, where):
        assert len(text.encode()) + len(title.encode()) <= MAX_DOC_BYTES
        texts.append(text)
        titles.append(title)
        tags.append(dict(t, **{'in': where}))

    for i, c in enumerate(cases):
        if i % 4 == 0:
            add(c.field, c.field, c.tags, 'both')
        else:
            add(c.field, FILL, c.tags, 'text')
            add(FILL, c.field, c.tags, 'title')
    return texts, titles, tags


def describe(tag):
    return ' '.join(f'{k}={v}' for k, v in tag.items())
