"""Names and documents of the regex-program tests (GPU test and the reference golden share them).

Every name is a fuzzy-class KB name whose regex uses a construct beyond literals and '.'.  A field is decided
only when it holds the name nearly verbatim (partial_ratio > 95 on the name's characters), so each document
carries the literal name plus forms the regex matches (FORMS) or near misses (MISSES).
"""
from __future__ import annotations

import random

# name -> (construct class, forms re.finditer(name) matches, near misses)
NAMES = {
    '[24]7.ai': ('set', ['27.ai', '47xai', '27-ai'], ['24]7.ai', '2\n.ai', '37.ai']),
    'Ab[cd]e.f': ('set', ['Abce.f', 'Abdexf'], ['Abee.f', 'Abde\nf']),
    'Macy\\s': ('category', ['Macy s', 'Macy\xa0', 'Macy\n', 'Macy '], ['Macys', 'Macy\\s']),
    '\\d+ Capital': ('category', ['42 Capital', '٣٤ Capital', '7 Capital'], ['x Capital', ' Capital']),
    'Sun\\w\\W\\S\\Dx Ltd': ('category', ['Suné -yx Ltd', 'Sun_\n!!x Ltd', 'Sun9 中_x Ltd'], ['Sun- -yx Ltd', 'Sunaa-yx Ltd',
                                                                                            'Suna  yx Ltd', 'Suna -7x Ltd']),
    '[^a-c]xon Mobil': ('negated set', ['Exxon Mobil', 'éxon Mobil', '\nxon Mobil', '中xon Mobil'], ['axon Mobil', 'cxon Mobil']),
    'Dow[^\\d\\s]Jones': ('negated set', ['Dow-Jones', 'DowéJones', 'Dow_Jones'], ['Dow Jones', 'Dow7Jones', 'Dow\nJones', 'Dow٣Jones']),
    '^Top Shop': ('assertion ^', [], ['Top Shop']),
    '\\AZillow Group': ('assertion \\A', [], ['Zillow Group']),
    'Yum Brands$': ('assertion $', [], ['Yum Brands']),
    'Kroger Co\\Z': ('assertion \\Z', [], ['Kroger Co']),
    'Ke$ha Holdings': ('assertion $', [], ['Keha Holdings', 'Ke\nha Holdings']),
    '\\bFoo\\b Inc': ('assertion \\b', ['Foo Inc', '-Foo Inc', '中 Foo Inc'], ['XFoo Inc', 'éFoo Inc', '_Foo Inc', 'Foo_ Inc']),
    'Go\\BPro Inc': ('assertion \\B', ['GoPro Inc'], ['Go Pro Inc', 'Go-Pro Inc']),
    'x-Fab*?rik': ('lazy', ['x-Farik', 'x-Fabbbrik', 'x-Fabrik'], ['x-Fab*?rik', 'x-Fabbik']),
    'Toys.+?Us Inc': ('lazy', ['Toys R Us Inc', 'ToysXUs Inc', 'Toys Us Us Inc'], ['ToysUs Inc', 'Toys\nUs Inc']),
    'Pay.{2,4}?al Co': ('lazy', ['Pay--al Co', 'Payalalal Co', 'Pay123al Co'], ['Pay-al Co', 'Pay12345al Co']),
    'A|X Armani Exchange': ('branch', ['A', 'X Armani Exchange'], ['x armani']),
    'Toys.R.Us|Toys R Us': ('branch', ['ToysXRXUs', 'Toys R Us', 'Toys.R.Us'], ['Toys RUs', 'Toys\nR\nUs']),
    'Toy|Toys R Us': ('branch', ['Toys R Us', 'Toy'], ['To']),
    'Big(Lots|Lot.+|L)x Inc': ('branch', ['BigLotsx Inc', 'BigLot--x Inc', 'BigLx Inc', 'BigLotsxx Inc'], ['BigLotx Inc', 'Bigx Inc']),
}
# anchored names match only at a field's edge: where the form must stand
EDGE = {'^Top Shop': 'start', '\\AZillow Group': 'start', 'Yum Brands$': 'end', 'Kroger Co\\Z': 'end'}
CLASSES = sorted({v[0] for v in NAMES.values()})
HOST_NAMES = ['Joe (Jr)?', 'a?', '(Wal|K)+mart Inc', 'Acme (?=Corp)Corp', '(Tic)-\\1 Tac', 'Jim(my)? Dean Inc']
FIXED_SET_NAMES = ['[24]7.ai', 'Ab[cd]e.f']

FILL = 'lorem ipsum dolor sit amet '


def processed(names):
    return {'TK': {'name': {n: (None, None) for n in names}}}


def _fill(n: int) -> str:
    return (FILL * (n // len(FILL) + 1))[:n]


def _plain(name: str) -> str:
    """What an anchored name matches (the name without its assertion)."""
    return NAMES[name][2][0]


def variants(name: str, rng: random.Random, k: int = 6):
    """k documents for one name: the literal name (so that the field is decided) with forms and misses."""
    _cls, forms, misses = NAMES[name]
    out = []
    for i in range(k):
        parts = [name] + [rng.choice(forms) for _ in range(rng.randint(0, 3)) if forms]
        parts += [rng.choice(misses) for _ in range(rng.randint(0, 2))]
        rng.shuffle(parts)
        sep = rng.choice([' ', ', ', '; ', ' \n'])
        body = sep.join(parts)
        edge = EDGE.get(name)
        if edge == 'start' and i % 3 != 2:
            body = _plain(name) + sep + body
        elif edge == 'end' and i % 3 != 2:
            body = body + sep + _plain(name) + ('\n' if i % 3 == 1 and name.endswith('$') else '')
        elif edge is None:
            body = rng.choice(['', 'intro ', FILL]) + body + rng.choice(['', ' outro', '.'])
        out.append(body)
    out.append(name)                       # the literal alone
    out.append(name + ' ' + name[:-1])     # ... and with a truncated copy
    return out


def seam_docs(name: str):
    """Documents whose length sits at the engines' seams with a match straddling each: 63 / 64 / 65 (and 127 /
    128 / 129) code points for the 64 starts of a backtracking round, 2047 / 2048 / 2049 + L for the 2048
    starts of a shift-and round."""
    _cls, forms, _m = NAMES[name]
    form = forms[0] if forms else _plain(name)
    edge = EDGE.get(name)
    out = []
    for total in (63, 64, 65, 127, 128, 129):
        if edge == 'start':
            doc = form + ' ' + name
            doc = doc + _fill(max(0, total - len(doc)))
        else:                              # the form ends the field, so it straddles the round's edge
            doc = name + ' '
            doc = doc + _fill(max(0, total - len(doc) - len(form))) + form
        out.append(doc)
    L = len(name)
    for base in (2047, 2048, 2049):
        total = base + L
        if edge == 'start':
            doc = form + ' ' + name
            out.append(doc + _fill(total - len(doc)))
            continue
        at = 2048 - len(form) // 2         # the form straddles start 2048
        doc = name + ' '
        doc = doc + _fill(at - len(doc)) + form
        if edge == 'end':
            out.append(doc)
        else:
            out.append(doc + _fill(max(0, total - len(doc) - len(form))) + form)
    return out


def documents(names=None, seed: int = 23):
    """(texts, titles) over every name: the issue's table, seeded variants, seam lengths, short fields, and the
    same with a non-ASCII code point in front (the resolve and transcoded routes)."""
    from tests.test_regex_program import TABLE
    names = list(NAMES) if names is None else names
    rng = random.Random(seed)
    docs = [doc for n, (doc, _want) in TABLE.items() if n in names]
    docs.append('^Top Shop and Top Shop')
    for n in names:
        docs += variants(n, rng)
        docs += seam_docs(n)
        docs += [n[:-1], n[1:], n[:5]]     # fields shorter than the program
    plain = list(docs)
    docs += ['é' + d for d in plain[::2]] + ['中 ' + d for d in plain[1::2]]
    texts = docs
    titles = [d for d in reversed(docs)]
    titles = [t if len(t) < 300 else t[-200:] for t in titles]
    return texts, titles
