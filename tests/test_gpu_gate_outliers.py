"""The stage-1 pair box chosen by selectivity (kw_compile with a background sample, csrc/kwmatch.hip choose_gate):
KBs of a dozen short uppercase names whose outliers -- a 2-byte name whose first or second byte lies far from the
others', a 3-byte name with such a byte -- would stretch the bounding box, compiled with a sample in which the
stretched box is expensive.  Each KB must report the gate worked out by hand from the cost model (fk_stage1<2..6>
through kw_filter_variant), and the scan's records must equal the CPU oracle's bit-exact wherever a name stands:
all 16 lane offsets, across 1 KiB tile edges, a group's first and last bytes, the first and last bytes of both
fields, with and without a word boundary beside it.  The same KB without a sample reports the bounding box's gate
and gives the same records.

The corpus reuses the builders of tests/filter_geometry.py (Corpus, payload) and the scan helpers of
tests/test_gpu_filter_geometry.py; where an occurrence stands is checked from the packed offsets, not from what
the builder meant (test_corpus_geometry, no GPU)."""
import random

import numpy as np
import pytest

from tests import filter_geometry as fg

TILE = fg.TILE
INLIERS = ['GE', 'GM', 'HP', 'IBM', 'GEO', 'BA', 'KO', 'MMM', 'CAT', 'DD']     # first bytes B..M, second bytes A..P
# case -> (outliers, sample, variant with the sample, variant without, names planted everywhere)
#   ext3     'A&E' would stretch the second byte's range down to '&': it goes to the 4-gram table, the box stays
#   first2   '3M' cannot go there (65 536 4-grams): '3' becomes the first byte's one more value
#   second2  'F5': '5' becomes the second byte's
#   both2    '3M' and 'F5'
#   all      the three together (the benchmark KB's shape)
#   equal    no outlier and a sample without uppercase pairs: both ranges widen to their hull, one flag word
CASES = {
    'ext3': (['A&E'], 'busy', 3, 3, ['A&E', 'GE', 'IBM']),
    'first2': (['3M'], 'busy', 4, 3, ['3M', 'GE', 'IBM']),
    'second2': (['F5'], 'busy', 5, 3, ['F5', 'GE', 'IBM']),
    'both2': (['3M', 'F5'], 'busy', 6, 3, ['3M', 'F5', 'GE', 'IBM']),
    'all': (['3M', 'F5', 'A&E'], 'busy', 6, 3, ['3M', 'F5', 'A&E', 'GE', 'IBM']),
    'equal': ([], 'plain', 2, 3, ['MMM', 'BA', 'GE', 'IBM']),
}
NEIGHBOURS = ((' ', ' '), ('a', ' '), (' ', 'a'), ('.', ','), ('a', 'a'), ('(', ')'), ('7', ' '), (' ', '_'))


def kb_names(case):
    return INLIERS + CASES[case][0] + fg.BASE_U + [fg.FUZZY3, fg.FUZZY9]


def sample(kind):
    """~64 KiB of lower-case words.  'busy': between them, in turn, a digit before an uppercase letter, an uppercase
    letter before a digit, before a full stop or a hyphen, and the words OF / ON -- each kind 2-3 % of the positions,
    so every stretched range of CASES costs the filter far more than the gate that avoids it (the model:
    1.86 VALU a survivor, 1024 positions a tile, a one-more-value gate 12-15 VALU) and so does the common hull of
    [B-M] and [A-P].  'plain': none of them, so the hull's cheaper gate (12 VALU less) wins."""
    rng = random.Random('gate-outliers/' + kind)
    tokens = ['5G', 'K9', 'OF', 'B.', '4K', 'B7', 'ON', 'C-']
    out, n, i = [], 0, 0
    while n < 65536:
        w = ''.join(rng.choice('abcdefghilmnoprstu') for _ in range(rng.randint(3, 8)))
        if kind == 'busy':
            w += ' ' + tokens[i % len(tokens)]
        out.append(w)
        n += len(w) + 1
        i += 1
    return ' '.join(out).encode()


class _Builder:
    """Documents whose text is laid out byte by byte: place() puts a name at a chosen arena offset."""

    def __init__(self, label):
        self.c = fg.Corpus('gate-outliers/' + label)
        self.text = b''
        self.plants = []
        self.k = 0

    @property
    def cur(self):
        return self.c.nbytes + len(self.text)

    def neighbours(self):
        self.k += 1
        return NEIGHBOURS[self.k % len(NEIGHBOURS)]

    def place(self, at, name, label):
        pre, post = self.neighbours()
        pl, o = fg.payload(name, pre, post)
        need = at - o - self.cur
        assert need >= 0, (label, name, at, self.cur)
        if len(self.text) + need + len(pl) > 6000:     # the field is full: the filler goes to fresh documents
            self.close()
            need = at - o - self.cur
            while need > 6000:
                self.c.filler_doc(4000)
                need = at - o - self.cur
        self.text += self.c.clean(need)
        self.plants.append((0, len(self.text) + o, name, label))
        self.text += pl

    def close(self, title=b'', title_plants=()):
        if self.text or title:
            self.c.doc(self.text + (self.c.clean(7) if self.text else b''), title, self.plants + list(title_plants))
        self.text, self.plants = b'', []


def corpus(case):
    """At most 64 documents (two groups) of a few KiB; group 0 starts at arena byte 0, so a tile edge is a multiple
    of 1024 there."""
    names = CASES[case][4]
    b = _Builder(case)
    c = b.c
    # the group's first bytes; then every name at every lane offset
    first = names[0].encode()
    b.text = first + b' '
    b.plants.append((0, 0, names[0], 'gstart'))
    for name in names:
        for r in range(16):
            at = (b.cur + 40 + 15) // 16 * 16 + r
            b.place(at, name, f'res/{r}')
    # across the tile edges: the name's first s bytes end a tile (s = 0: it starts the next one)
    edge = (b.cur + 200) // TILE + 1
    for name in names:
        for s in range(len(name) + 1):
            b.place(TILE * edge - s, name, f'tile/{s}')
            edge += 1
    b.close()
    assert c.n_docs < 20 and c.nbytes < 30 * TILE, (c.n_docs, c.nbytes)
    # the first and last bytes of both fields (the neighbour across the edge is the other field's name)
    for name in names:
        nb = name.encode()
        text = nb + b' ' + c.clean(30) + b' ' + nb
        title = nb + b' ' + c.clean(12) + b' ' + nb
        c.doc(text, title, [(0, 0, name, 'text_first'), (0, len(text) - len(nb), name, 'text_last'),
                            (1, 0, name, 'title_first'), (1, len(title) - len(nb), name, 'title_last')])
    # the last bytes of group 0, the first of group 1, the arena's last bytes
    for g, name in ((0, names[0]), (1, names[-1])):
        while c.n_docs % fg.FG_DOCS != fg.FG_DOCS - 1:
            c.filler_doc(300)
        nb = name.encode()
        title = c.clean(9) + b' ' + nb
        c.doc(c.clean(40), title, [(1, len(title) - len(nb), name, 'gend')])
        if g == 0:
            nxt = names[1].encode()
            c.doc(nxt + b' ' + c.clean(500), c.clean(8), [(0, 0, names[1], 'gstart')])
            for name2 in names:     # group 1 starts at an odd byte: the lane offsets once more, two each
                text, plants = c.clean(20), []
                for _ in range(2):
                    pl, o = fg.payload(name2)
                    plants.append((0, len(text) + o, name2, 'group1'))
                    text += pl + c.clean(c.rng.randint(17, 31))
                c.doc(text, c.clean(6), plants)
    assert c.n_docs == 64
    return c


_CORPORA = {}


def cached_corpus(case):
    if case not in _CORPORA:
        _CORPORA[case] = corpus(case)
    return _CORPORA[case]


@pytest.mark.parametrize('case', sorted(CASES))
def test_corpus_geometry(case):
    """No GPU: from the packed offsets, every planted name stands at all 16 lane offsets, over a tile edge with each
    split, at a group's first and last bytes and at the first and last bytes of both fields; at least one occurrence
    of each has a word character beside it and one has none; the oracle finds exactly the planted matches."""
    from tests.oracle_matcher import OracleMatcher
    c = cached_corpus(case)
    off, arena = c.offsets(), c.arena()
    assert c.n_docs <= 64 and max(len(f) for f in c.fields) <= 8192
    g1 = int(off[2 * fg.FG_DOCS])
    seen = {}
    for d, f, s, name, _label in c.plants:
        L = len(name.encode())
        a = int(off[2 * d + f]) + s
        assert arena[a:a + L] == name.encode()
        base = 0 if d < fg.FG_DOCS else g1 & ~15
        t = seen.setdefault(name, set())
        t.add(('res', (a - base) % 16))
        if (a - base) // TILE != (a - base + L - 1) // TILE:
            t.add(('split', TILE - (a - base) % TILE))
        if (a - base) % TILE == 0:
            t.add(('split', 0))
        if (a - base + L) % TILE == 0:
            t.add(('split', L))
        for tag in fg.tags(off, d, f, s, L, arena):
            if tag.startswith(('gstart/', 'gend/', 'fedge/')):
                t.add(tag.split('/')[0] + ('/' + tag.split('/')[1] if tag.startswith('fedge') else ''))
        before = arena[a - 1:a].decode() if s > 0 else None
        after = arena[a + L:a + L + 1].decode() if a + L < int(off[2 * d + f + 1]) else None
        t.add(('boundary', fg.expect_match(name, before, after)))
    for name in CASES[case][4]:
        t = seen[name]
        L = len(name.encode())
        want = {('res', r) for r in range(16)} | {('split', s) for s in range(L + 1)} | \
            {f'fedge/{p}' for p in fg.EDGE_POS} | {('boundary', True), ('boundary', False)}
        assert want <= t, (name, sorted(map(str, want - t)))
    assert 'gstart' in seen[CASES[case][4][0]] and 'gstart' in seen[CASES[case][4][1]]
    assert 'gend' in seen[CASES[case][4][0]] and 'gend' in seen[CASES[case][4][-1]]
    om = OracleMatcher(fg.processed(kb_names(case)))
    rec = om.match_strings(*c.strings())
    got = {}
    for d, f, p, pos in zip(rec['doc'].tolist(), rec['field'].tolist(), rec['pattern'].tolist(), rec['pos'].tolist()):
        got.setdefault((d, f, om.ckb.names[p]), []).append(pos)
    want = c.expected(kb_names(case))
    assert {k: sorted(v) for k, v in got.items()} == want


# ---------------------------------------------------------------------------------------------------- the GPU side
@pytest.fixture(scope='module')
def oracle_records():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests.oracle_matcher import OracleMatcher
    from tests.test_gpu_filter_geometry import _as_set
    seen = {}

    def records(case):
        if case not in seen:
            om = OracleMatcher(fg.processed(kb_names(case)))
            seen[case] = _as_set(om.match_strings(*cached_corpus(case).strings()), om.ckb.names)
        return seen[case]
    return records


def _matcher(case, with_sample):
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    _outliers, kind, chosen, bounding, _planted = CASES[case]
    m = GpuMatcher(compile_kb(fg.processed(kb_names(case))), None, sample(kind) if with_sample else None)
    want = chosen if with_sample else bounding
    assert m.filter_variant() == want, (case, with_sample, m.filter_variant(), want)
    return m


def _check(m, case, want, entry):
    """Two scans on the handle: the oracle's records, every document on the fast path, nothing deferred, no rescan."""
    from advanced_scrapper_amd import _native
    from tests.test_gpu_filter_geometry import _as_set, _describe, _scan
    c = cached_corpus(case)
    for rep in (0, 1):
        got = _as_set(_scan(m, c, entry), m.ckb.names)
        st = m.stats()
        lost, extra = want - got, got - want
        assert not lost and not extra, (
            f'{case}, {entry}, scan {rep}: {len(lost)} records lost, {len(extra)} not the oracle\'s; lost: '
            f'{_describe(c, lost)}; extra: {_describe(c, extra)}; stats {st}')
        routes = m.doc_routes(c.n_docs)
        assert (routes == _native.KW_ROUTE_SCAN).all(), (case, entry, rep, np.bincount(routes, minlength=4).tolist())
        assert st['deferred_docs'] == 0 and st['rescans'] == 0, (case, entry, rep, st)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['scan', 'host'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_chosen_gate(oracle_records, case, entry):
    """With the sample: the gate the model must choose, and the oracle's records through kw_scan and kw_scan_host."""
    m = _matcher(case, True)
    try:
        st = _check(m, case, oracle_records(case), entry)
        print(f'{case}, {entry}: variant {m.filter_variant()}, stats {st}')
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_without_a_sample_the_bounding_box(oracle_records, case):
    """The same KB without a sample: the bounding box's gate (today's variant), the same records; and no more
    stage-2 survivors with the sample's gate than with the bounding box's on this corpus."""
    m = _matcher(case, False)
    try:
        st0 = _check(m, case, oracle_records(case), 'host')
    finally:
        m.close()
    m = _matcher(case, True)
    try:
        st1 = _check(m, case, oracle_records(case), 'host')
    finally:
        m.close()
    print(f'{case}: stage-1 survivors {st0["candidates"]} -> {st1["candidates"]}, stage 2 {st0["candidates_stage2"]} '
          f'-> {st1["candidates_stage2"]}')
    if case != 'equal':     # (the hull is wider than the bounding box: there the gain is the gate's own instructions)
        assert st1['candidates_stage2'] <= st0['candidates_stage2'], (st0, st1)
