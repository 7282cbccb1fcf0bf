"""The byte-geometry sweep of tests/tx_geometry.py on the CPU: every cell of every family is hit (from the packed
arena and its offsets, so the generator cannot drift), the three knowledge bases fill the marker table as they
claim (against a Python restatement of its build), and the oracle's positions on these fields equal a plain
re.finditer loop, which knows nothing of bytes.  tests/test_gpu_tx_geometry.py sends the documents through every
kernel route."""
import re

import pytest

from advanced_scrapper_amd.matcher import pack_fields
from oracle import kwmatch_oracle as orc
from tests import tx_geometry as tg


@pytest.fixture(scope='module')
def docs():
    return tg.corpus()


@pytest.fixture(scope='module')
def cover(docs):
    texts, titles, _tags = docs
    return tg.coverage(texts, titles, tg.fuzzy_names('base'))


@pytest.mark.parametrize('family', list('abcdefghij'))
def test_every_cell_of_the_family_is_hit(cover, family):
    assert cover[family] == [], f'family {family}: no document for {cover[family][:20]}'


def test_corpus_shape_and_determinism(docs):
    texts, titles, tags = docs
    assert len(texts) == len(titles) == len(tags)
    assert 300 <= len(texts) <= 600 and len(texts) % 64
    sizes = sorted(len(t.encode()) for t in texts)
    assert sizes[-3:] == [16383, 16384, 16385]
    for n in (16383, 16384, 16385):
        (d,) = [i for i, t in enumerate(texts) if len(t.encode()) == n]
        assert f'text of {n} bytes' in tags[d] and 8 <= d % 64 <= 55
        assert tg.occurrences(texts[d], tg.fuzzy_names('base')) <= 512
    assert sizes[-4] < 16383 and max(len(t.encode()) for t in titles) <= 3300
    # all but the item-class and size-bound documents stay at about 3.2 KiB and, so that the batched epilogue takes
    # them (at most 64 items in a field), at few occurrences per field
    assert sum(1 for s in sizes if s > 3400) == 6
    fuzzy = tg.fuzzy_names('over')
    for a, b, t in zip(texts, titles, tags):
        if 'occurrences in the' not in t:
            assert tg.occurrences(a, fuzzy) <= tg.MAX_OCC and tg.occurrences(b, fuzzy) <= tg.MAX_OCC, t
    classes = tg.item_classes(texts, titles, fuzzy)
    assert [t for t, c in zip(tags, classes) if c != 'batch'] == [t for t in tags if 'occurrences in the' in t]
    assert classes.count('wave') == 3 and classes.count('big') == 2
    tg._CACHE.clear()
    again = tg.corpus()
    assert again == (texts, titles, tags)


def test_knowledge_bases():
    names = {w: tg.kb_names(w) for w in ('base', 'full', 'over')}
    for w, ns in names.items():
        assert len(set(ns)) == len(ns)
        fuzzy, upper = ns[:-3], ns[-3:]
        assert [orc.name_class(n) for n in upper] == ['U'] * 3 and upper == tg.UPPERS
        assert all(orc.name_class(n) == 'F' for n in fuzzy)
        assert all(re.escape(n) == n for n in fuzzy), 'a name with a regex metacharacter'
    base = tg.fuzzy_names('base')
    assert len(base) == 24
    for n in base:
        assert 8 <= len(n) <= 20
        assert {tg.width(c) for c in n} == {1, 2, 3, 4}
    assert len({n[0] for n in base}) == 24 and len({n[-1] for n in base}) == 24
    # base: fewer than 127 distinct non-ASCII code points, every one with a marker
    _key, _val, order = tg.marker_table(names['base'])
    assert 0 < len(order) < 127
    # full: exactly 127, a probe chain of at least 4, a chain that begins at slot 254 / 255 and wraps to slot 0
    key, val, order = tg.marker_table(names['full'])
    assert len(order) == 127 and sum(k is not None for k in key) == 127
    walks = {cp: tg.marker_lookup(key, val, cp) for cp in order}
    assert all(v == 0x81 + order.index(cp) for cp, (v, _n, _w) in walks.items())
    assert max(n for _v, n, _w in walks.values()) >= 4
    wrapped = [cp for cp, (_v, _n, w) in walks.items() if w]
    assert wrapped and all(tg.slot(cp) >= 254 for cp in wrapped if key.index(cp) < 4)
    assert any(tg.slot(cp) in (254, 255) and key.index(cp) < tg.slot(cp) for cp in wrapped)
    # the documents hold code points of those chains' late members, so their occurrences depend on the walk
    texts, titles, _tags = tg.corpus()
    blob = ''.join(texts) + ''.join(titles)
    assert any(chr(cp) in blob for cp in wrapped)
    assert any(chr(cp) in blob for cp, (_v, n, _w) in walks.items() if n >= 4)
    # ... and fillers of no name whose home slot lies inside them: the walk passes occupied slots and misses
    fillers = tg.full_fillers()
    assert len(fillers) == 2
    for c in fillers:
        v, n, _w = tg.marker_lookup(key, val, ord(c))
        assert ord(c) not in order and v == 0x80 and n >= 3 and c in blob
    assert tg.marker_lookup(key, val, ord(fillers[0]))[2], 'the first filler walks from slot 255 to slot 0'
    # over: a 128th code point, in one name only, the largest: it alone has no marker
    key, val, order = tg.marker_table(names['over'])
    assert len(order) == 128
    last = order[127]
    assert last == max(order) and tg.marker_lookup(key, val, last)[0] == 0x80
    assert [n for n in names['over'] if chr(last) in n] == [tg._build_names()['over']]
    assert all(tg.marker_lookup(key, val, cp)[0] != 0x80 for cp in order[:127])
    assert sum(1 for t in texts + titles if tg._build_names()['over'] in t) >= 3


def test_oracle_positions_equal_a_finditer_loop(docs):
    """Every field, every name of the largest KB with an exact occurrence: the oracle reports the name (an exact
    occurrence scores 100) with the positions of a plain loop; the same on the generic kernel's texts."""
    texts, titles, _tags = docs
    names = tg.kb_names('over')
    fuzzy = names[:-3]
    oracle = orc.Oracle(tg.processed(names))
    gtexts, _i, _g = tg.generic_corpus()
    fields = [(d, 'text', s) for d, s in enumerate(texts)] + [(d, 'title', s) for d, s in enumerate(titles)]
    fields += [(d, 'generic text', s) for d, s in enumerate(gtexts[::7])]
    n_occ = n_cp = n_cov = 0
    for d, what, s in fields:
        res = oracle.field_results(s)
        covered = bytearray(len(s))
        for n in fuzzy:
            plain = [m.start() for m in re.finditer(re.escape(n), s)]
            if plain:
                assert res.get(n) == plain, (d, what, n)
                if what != 'generic text':
                    n_occ += len(plain)
                    for p in plain:
                        covered[p:p + len(n)] = b'\1' * len(n)
        for u in tg.UPPERS:
            plain = [m.start() for m in re.finditer(r'\b' + u + r'\b', s)]
            assert res.get(u, []) == plain, (d, what, u)
        if what != 'generic text':
            n_cp += len(s)
            n_cov += sum(covered)
    print(f'{len(texts)} documents, {n_occ} exact occurrences witness {n_cov} of {n_cp} code points')
    # (the rest: the ASCII documents and pads, the 16 KiB texts' filler, the two filler blocks, the other KBs' names)
    assert n_occ > 5000 and n_cov > 0.8 * n_cp


def test_uppercase_neighbours_decide(docs):
    """Family i means something: with a word neighbour the uppercase name is not reported, with a non-word one it is."""
    texts, _titles, tags = docs
    seen = set()
    for s, t in zip(texts, tags):
        m = re.search(r'uppercase (\w+) with (word|non-word) neighbour', t)
        if m:
            u, cls = m.group(1), m.group(2)
            assert u in s and bool(orc.upper_positions(u, s)) == (cls == 'non-word'), t
            seen.add(cls)
    assert seen == {'word', 'non-word'}


def test_near_occurrences_hang_on_every_code_point(docs):
    """Family j means something: the name that the field's ending lacks a letter of is reported without a position,
    and no longer when any one multi-byte character of that ending is another code point (a wrong view byte)."""
    texts, _titles, tags = docs
    base = tg.fuzzy_names('base')
    oracle = orc.Oracle(tg.processed(tg.kb_names('base')))
    n_docs = 0
    for s, t in zip(texts, tags):
        if 'ends with a name less one letter' not in t:
            continue
        ends = [(n, n[:i] + n[i + 1:]) for n in base if n not in s for i in range(1, len(n) - 1)
                if n[i].isascii() and s.endswith(n[:i] + n[i + 1:])]
        assert ends, t
        n, v = ends[0]
        assert oracle.field_results(s).get(n) == [], t
        head = s[:len(s) - len(v)]
        for i, ch in enumerate(v):
            if ord(ch) >= 0x80:
                assert n not in oracle.field_results(head + v[:i] + tg.FILL3 + v[i + 1:]), (t, i)
        n_docs += 1
    assert n_docs == 3 * len(tg.SPLITS) + len(tg._plan()['special'])


def test_permutation_keeps_the_alignment_families():
    texts, titles, tags, src = tg.permuted_corpus()
    assert texts[31] == '' and titles[31] == '' and src[31] == -1 and tags[31] == 'empty document'
    assert sorted(s for s in src if s >= 0) == list(range(len(tg.corpus()[0])))
    arena, off = pack_fields(texts, titles)
    assert tg.missing_a(tg.cells_a(arena, off)) == [] and tg.missing_d(tg.cells_d(arena, off)) == []
    a0, o0 = pack_fields(*tg.corpus()[:2])
    moved = sum(1 for k, s in enumerate(src) if s >= 0 and off[2 * k] % 16 != o0[2 * s] % 16)
    assert moved > len(src) // 2
