"""The boundary sweep of tests/fuzzy_sweep.py on the CPU: the oracle's decision equals its brute-force DP on every
case (both argument orders, no stride: the whole sweep takes a few seconds), the sweep straddles the threshold at
every length where a kernel bound steps, and its names stay apart, so that a wrong-name hit in a GPU failure
message means something."""
import collections

import pytest

from oracle import kwmatch_oracle as orc
from tests import fuzzy_sweep as fs


@pytest.fixture(scope='module')
def sweep():
    cases = fs.all_cases()
    hit = [orc.partial_ratio_gt95(c.field, c.name) for c in cases]
    return cases, hit


def test_sweep_size_and_determinism(sweep):
    cases, _hit = sweep
    texts, titles, tags = fs.documents(cases)
    assert len(texts) == len(titles) == len(tags) <= fs.MAX_DOCS
    assert max(len(a.encode()) + len(b.encode()) for a, b in zip(texts, titles)) <= fs.MAX_DOC_BYTES
    fs._CACHE.clear()
    again = fs.all_cases()
    assert [(c.field, c.name, c.tags) for c in again] == [(c.field, c.name, c.tags) for c in cases]
    # every case is in a text and in a title; one case in four is in both fields of one document
    where = collections.Counter(t['in'] for t in tags)
    assert where['text'] == where['title'] and where['both'] * 3 >= where['text'] > 0
    # the lengths that must not be thinned carry every (nd, ni) pair at every edit and field placement
    for m in fs.KEY_LENGTHS:
        k = fs.kfull(m)
        have = {(c.tags['nd'], c.tags['ni'], c.tags['edit'], c.tags['place'], c.tags['gap']) for c in cases
                if c.tags['kind'] == 'indel' and c.tags['family'] == 'a' and c.tags['m'] == m}
        for nd in range(k + 2):
            for ni in range(k + 2):
                for edit in fs.EDITS if nd + ni else ('none',):
                    if edit.startswith('touch') and nd == 0:
                        continue
                    for place, gap in fs._places(m, True):
                        assert (nd, ni, edit, place, gap) in have, (m, nd, ni, edit, place, gap)
    # the staged window and the clipped window starts hang over the field: gaps of 1, 2, 2k and 2k + 1
    assert fs._gaps(64) == [1, 2, 6, 7] and fs._gaps(41) == [1, 2, 4, 5] and fs._gaps(21) == [1, 2, 3]


def test_oracle_equals_brute_force_on_the_sweep(sweep):
    cases, hit = sweep
    bad = []
    for c, h in zip(cases, hit):
        b1 = orc.partial_ratio_score(c.field, c.name, brute=True) > 95
        b2 = orc.partial_ratio_score(c.name, c.field, brute=True) > 95
        if not (h == b1 == b2) or orc.partial_ratio_gt95(c.name, c.field) != h:
            bad.append((fs.describe(c.tags), c.field, c.name, h, b1, b2))
    n_hit = sum(hit)
    print(f'\nfuzzy sweep: {len(cases)} cases, {n_hit} hits, {len(cases) - n_hit} misses; '
          f'{len(fs.documents(cases)[0])} documents; brute force on every case, {len(bad)} disagreements')
    assert not bad, bad[:5]


def _sel(sweep, **want):
    cases, hit = sweep
    return [(c, h) for c, h in zip(cases, hit) if all(c.tags[k] == v for k, v in want.items())]


def test_sweep_straddles_the_threshold(sweep):
    # --- middle of filler, the two seeded families (only full windows see the variant)
    for fam in ('a', 'b'):
        for m in fs.LENGTHS:
            mid = _sel(sweep, family=fam, kind='indel', m=m, place='middle')
            e = lambda c: c.tags['nd'] + c.tags['ni']
            if m >= 21:
                assert any(h for c, h in mid if e(c) >= 2), (fam, m)
                assert any(not h for c, h in mid if e(c) >= 2), (fam, m)
                assert all(h for c, h in mid if e(c) <= 1) and any(e(c) == 1 for c, h in mid), (fam, m)
            else:
                assert all(not h for c, h in mid if e(c) >= 1) and any(e(c) >= 1 for c, h in mid), (fam, m)
                assert all(h for c, h in mid if e(c) == 0) and any(e(c) == 0 for c, h in mid), (fam, m)
    # --- edge windows: names of 11..20 have them at the field start and at the field end, names of 8..10 none
    cases, hit = sweep
    for m in range(8, 21):
        edge = {'start': [], 'end': []}
        for c, h in zip(cases, hit):
            t = c.tags
            if t['family'] == 'a' and t['m'] == m and t['kind'] in ('indel', 'clip') and t['place'] in edge \
                    and (t['nd'] + t['ni'] > 0 or t['clip']):
                edge[t['place']].append(h)
        for place, hs in edge.items():
            assert hs, (m, place)
            assert any(hs) if m >= 11 else not any(hs), (m, place)
    # --- clipped variants of the names of 21 and more: a miss at every length, a hit with c >= 2 at every length
    # that can have one.  A variant cut by c at its field edge scores at best through the window of m - c code
    # points: d = c, 20 c < 2 m - c, i.e. 21 c < 2 m; in the middle of filler c <= kfull(m).  At m = 21 both
    # fail for c = 2 (42 < 42; kfull = 1), so 21 has hits with c = 1 only, and that is asserted instead.
    for m in range(21, 65):
        clip = [(c, h) for c, h in _sel(sweep, kind='clip', m=m)]
        assert any(not h for c, h in clip), m
        if m >= 22:
            assert any(h for c, h in clip if abs(c.tags['clip']) >= 2), m
        else:
            assert not any(h for c, h in clip if abs(c.tags['clip']) >= 2), m
            assert any(h for c, h in clip if abs(c.tags['clip']) == 1), m
    # --- whole fields shorter than the name (the field is the needle): a hit and a miss at every field length
    # 11..63 (a field of 64 would need a name of 65: over the cap)
    by_len = collections.defaultdict(list)
    for c, h in zip(cases, hit):
        if c.tags['place'] == 'whole' and len(c.field) < len(c.name) and c.tags['family'] in ('a', 'b'):
            by_len[len(c.field)].append(h)
    for n in range(11, 64):
        assert any(by_len[n]) and not all(by_len[n]), (n, by_len[n])
    # --- whole fields of exactly m, m - 1 and m + 1 code points at every length
    for m in fs.LENGTHS:
        lens = {len(c.field) for c, _h in _sel(sweep, family='a', kind='indel', m=m, place='whole')}
        assert {m - 1, m, m + 1} <= lens, (m, lens)
    # --- fields of exactly 10 and 11 code points
    for L in (10, 11):
        sh = [h for c, h in _sel(sweep, kind='short', gap=L)]
        assert any(sh) and not all(sh), (L, sh)
        assert all(len(c.field) == L for c, _h in _sel(sweep, kind='short', gap=L))
    # --- the 64-code-point name in fields of 64 and 65 code points
    cap = _sel(sweep, kind='cap64')
    assert {len(c.field) for c, _h in cap} == {64, 65}
    assert {c.tags['nd'] + c.tags['ni'] for c, _h in cap} == set(range(8))
    assert any(h for c, h in cap if c.tags['nd'] + c.tags['ni'] >= 2) and any(not h for _c, h in cap)
    # --- the two small families have both outcomes too
    for fam in ('na', 'rep'):
        hs = [h for _c, h in _sel(sweep, family=fam)]
        assert any(hs) and not all(hs), fam


def test_names_stay_apart(sweep):
    """Every field against every name of the large KB: a case of the seeded and the non-ASCII families hits no
    name but its own.  The names with runs are built from the same chunks and may hit one another; those hits are
    the oracle's, confirmed by the brute force, and never reach into another family."""
    cases, hit = sweep
    big = fs.kb_big()
    fam_of = {}
    for fam, table in (('a', fs.names('a')), ('b', fs.names('b')), ('na', fs.nonascii_names()),
                       ('rep', fs.repeat_names())):
        for n in table.values():
            fam_of[n] = fam
    ns = orc.NameSet(big)
    seen = {}
    stray = []
    for c, h in zip(cases, hit):
        if c.field not in seen:
            seen[c.field] = ns.decide(c.field)
        dec = seen[c.field]
        assert bool(dec[big.index(c.name)]) == h, fs.describe(c.tags)
        for n, d in zip(big, dec):
            if d and n != c.name:
                stray.append((c, n))
    print(f'\n{len(stray)} hits of a name other than the intended one, all among the names with runs')
    for c, n in stray:
        assert c.tags['family'] == 'rep' and fam_of[n] == 'rep', (fs.describe(c.tags), c.field, n)
        assert orc.partial_ratio_score(c.field, n, brute=True) > 95
