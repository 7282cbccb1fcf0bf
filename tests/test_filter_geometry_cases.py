"""CPU: the case builder of tests/filter_geometry.py held to its claims, so that a later edit cannot hollow the
filter / probe sweep out: the builder is deterministic, the tags its independent classifier derives from the packed
offsets hold every required (tag, key-length class) cell, the CPU oracle returns exactly the planted intent, and no
two occurrences of a name overlap (the premise of the GPU test's item counts)."""
import re

import pytest

from tests import filter_geometry as fg


@pytest.fixture(scope='module')
def corpora():
    return fg.cases()


def test_builder_is_deterministic(corpora):
    again = fg.cases(fresh=True)
    assert [c.fields for c in again] == [c.fields for c in corpora]
    assert [c.plants for c in again] == [c.plants for c in corpora]
    assert [c.straddles for c in again] == [c.straddles for c in corpora]
    d0, d1 = fg.dense_cases(), fg.dense_cases(fresh=True)
    assert [c.fields for c in d0] == [c.fields for c in d1] and [c.plants for c in d0] == [c.plants for c in d1]


def test_sizes(corpora):
    assert [c.n_docs for c in corpora[1:]] == list(fg.SMALL_SIZES)
    assert {1, 31, 32, 33, 64, 65} <= {c.n_docs for c in corpora}
    assert corpora[0].n_docs <= fg.MAX_DOCS
    for c in corpora + fg.dense_cases():
        assert max(len(f) for f in c.fields) <= fg.MAX_FIELD and c.nbytes < 16 << 20
        from advanced_scrapper_amd.matcher import pack_fields
        _arena, off = pack_fields(*c.strings())
        assert off.tolist() == c.offsets().tolist()       # the builder's layout is pack_fields'


def test_filler_shares_nothing_with_the_names():
    """The clean filler (its alphabet and the space) holds no byte pair of a 2-3 byte name and no 4-gram of any
    name; every near miss of the noisy filler holds the first two bytes of a name and is no match between spaces."""
    names = sorted({n for v in fg.SHORT for n in fg.kb_names(v)})
    filler = set((fg._ALPHABET + ' ').encode())
    for n in names:
        b = n.encode()
        if len(b) <= 3:
            assert not any(set(b[i:i + 2]) <= filler for i in range(len(b) - 1)), n
        assert not any(set(b[i:i + 4]) <= filler for i in range(len(b) - 3)), n
    c = fg.Corpus('filler')
    assert set(c.clean(4096)) <= filler and len(c.clean(37)) == 37 and len(c.noisy(513)) == 513
    for tok in fg._NOISE:
        s = f' {tok} '
        assert any(n[:2] in tok for n in names), tok
        for n in names:
            if n in (fg.FUZZY3, fg.FUZZY9):
                assert n not in s, (tok, n)
            else:
                assert not re.search(r'\b' + re.escape(n) + r'\b', s), (tok, n)


def _cells(corpora):
    """(tag, class) and (tag, name) of every occurrence planted as a match (the edge and neighbour tags: of every
    occurrence), and of every straddle, through the classifier."""
    by_class, by_name = set(), set()
    for c in corpora:
        off, arena = c.offsets(), c.arena()
        for d, f, s, name, _label in c.plants:
            match = c.plant_matches(d, f, s, name)
            for t in fg.tags(off, d, f, s, len(name.encode()), arena):
                if match or t.startswith(('fedge/', 'nb/', 'shared/')):
                    if t == 'shared/token' and not match:
                        continue
                    by_class.add((t, fg.name_class(name)))
                    by_name.add((t, name))
        for d, f, split, name, kind in c.straddles:
            t = fg.straddle_tag(off, d, f, split, len(name.encode()))
            assert t == f'straddle/{kind}/{split}', (c.label, d, t, kind)
            by_class.add((t, fg.name_class(name)))
    return by_class, by_name


def test_every_required_cell_is_covered(corpora):
    by_class, by_name = _cells(corpora)
    missing = [cell for cell in fg.required_cells() if cell not in by_class]
    missing += [cell for cell in fg.required_named() if cell not in by_name]
    assert not missing, f'{len(missing)} cells are not covered, the first: {missing[:20]}'


def test_labels_are_what_the_classifier_sees(corpora):
    """An occurrence the builder placed for a positioned cell carries that tag by the classifier's own arithmetic."""
    n = 0
    for c in corpora:
        off, arena = c.offsets(), c.arena()
        for d, f, s, name, label in c.plants:
            if label.startswith(('tile_', 'res/', 'lane/', 'gstart', 'gend/', 'fedge/', 'nb/', 'shared/')) and \
                    label != 'gend/small':
                assert label in fg.tags(off, d, f, s, len(name.encode()), arena), (c.label, d, f, s, name, label)
                n += 1
    assert n > 1500


@pytest.mark.parametrize('variant', [0, 1, 2, 3])
def test_oracle_returns_the_planted_intent(corpora, variant):
    """tests/oracle_matcher.OracleMatcher on every corpus, per KB: every occurrence planted as a match at its
    code-point position, every one planted as a non-match (straddles, wrong \\b) absent, nothing else anywhere."""
    from tests.oracle_matcher import OracleMatcher
    names = fg.kb_names(variant)
    om = OracleMatcher(fg.processed(names))
    for c in corpora + fg.dense_cases():
        texts, titles = c.strings()
        rec = om.match_strings(texts, titles)
        got = {}
        for d, p, q, f in zip(rec['doc'].tolist(), rec['pattern'].tolist(), rec['pos'].tolist(), rec['field'].tolist()):
            got.setdefault((d, f, om.ckb.names[p]), []).append(q)
        for v in got.values():
            v.sort()
        want = c.expected(names)
        lost = sorted(k for k in want if got.get(k) != want[k])
        extra = sorted(k for k in got if k not in want)
        assert not lost and not extra, (c.label, 'planted but not found', lost[:8], 'not planted', extra[:8],
                                        [(k, got[k], c.fields[2 * k[0] + k[1]][:80]) for k in extra[:3]])
    planted_off = [(d, f, s, n) for c in corpora for d, f, s, n, _l in c.plants if not c.plant_matches(d, f, s, n)]
    assert len(planted_off) > 100 and sum(len(c.straddles) for c in corpora) > 90


def test_no_two_occurrences_overlap(corpora):
    """In every field, no two occurrences (any two names of a KB's uppercase names, overlapping search) that the
    oracle reports overlap: one verified use is then one item."""
    for variant in (0, 1, 2, 3):
        names = fg.kb_names(variant, fuzzy=False)
        rx = [(n, re.compile(r'(?=\b' + re.escape(n) + r'\b)')) for n in names]
        for c in corpora + fg.dense_cases():
            for s in c.strings()[0] + c.strings()[1]:
                spans = sorted((m.start(), m.start() + len(n)) for n, r in rx if n in s for m in r.finditer(s))
                for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                    assert a1 <= b0, (c.label, s[a0:b1])
