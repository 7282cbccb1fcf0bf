"""The partial_ratio > 95 boundary sweep (tests/fuzzy_sweep.py) through every kernel route of the scan: document by
document, all names of the KB, both fields and the positions of GpuMatcher.match_strings against the CPU oracle
(tests/oracle_matcher.OracleMatcher) on the same strings, bit-exact.  Every route asserts that it was taken.

The oracle's side is computed once per KB and distinct field string (a module fixture) and shared by the routes
that scan the same strings.  tests/test_fuzzy_sweep_cases.py holds the oracle itself against its brute-force DP
on these cases and checks that they straddle the threshold."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import fuzzy_sweep as fs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPPER = 'IBM'                 # an all-uppercase name: 65 occurrences send a document to the generic kernel
KBS = {'small': fs.kb_small, 'big': fs.kb_big}


def kb_names(which):
    return KBS[which]() + [UPPER]


class _Oracle:
    """OracleMatcher's result of one field string, computed once: pattern id -> positions."""

    def __init__(self, which):
        from tests.oracle_matcher import OracleMatcher
        self.o = OracleMatcher(fs.processed(kb_names(which)))
        self.seen = {}

    def field(self, s):
        r = self.seen.get(s)
        if r is None:
            r = self.seen[s] = {self.o.pid[n]: list(pos) for n, pos in self.o._field(s).items()}
        return r

    def grouped(self, texts, titles):
        """What group_hits gives for OracleMatcher.match_strings(texts, titles)."""
        out = {}
        for d, pair in enumerate(zip(texts, titles)):
            for f, s in enumerate(pair):
                r = self.field(s)
                if r:
                    out.setdefault(d, {})[f] = r
        return out


@pytest.fixture(scope='module')
def oracles():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return {which: _Oracle(which) for which in KBS}


def _matcher(which):
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    return GpuMatcher(compile_kb(fs.processed(kb_names(which))))


def _scan(m, texts, titles):
    from advanced_scrapper_amd.matcher import group_hits
    assert len(texts) <= fs.MAX_DOCS
    return group_hits(m.match_strings(texts, titles))


def _equal(got, want, m, texts, titles, tags, what):
    names = m.ckb.names
    bad = [d for d in range(len(texts)) if got.get(d) != want.get(d)]
    for d in bad[:8]:
        show = lambda r: {f: {names[p]: v for p, v in byp.items()} for f, byp in (r or {}).items()}
        print(f'{what} doc {d} [{fs.describe(tags[d])}] text {texts[d]!r} title {titles[d]!r}: '
              f'got {show(got.get(d))} want {show(want.get(d))}')
    assert not bad, f'{what}: GPU differs from the oracle on {len(bad)} documents, first {bad[:20]}'


def _routes(m, n):
    from advanced_scrapper_amd import _native
    r = m.doc_routes(n)
    return r, {k: int((r == getattr(_native, 'KW_ROUTE_' + k)).sum()) for k in ('SCAN', 'TRANSCODE', 'RESOLVE', 'GENERIC')}


# ------------------------------------------------------------------------------------------------ documents
def default_docs(which):
    """small: the cases of family a (its KB); big: every all-ASCII case and the names with runs."""
    cases = fs.ascii_cases('a') if which == 'small' else fs.ascii_cases() + fs.repeat_cases()
    return fs.documents(cases)


def _alternate(fields):
    """(field, tags) pairs as documents: the field as the text and as the title by turns, the other filler."""
    texts, titles, tags = [], [], []
    for i, (s, t) in enumerate(fields):
        texts.append(fs.FILL if i % 2 else s)
        titles.append(s if i % 2 else fs.FILL)
        tags.append(dict(t, **{'in': 'title' if i % 2 else 'text'}))
        assert len(texts[-1].encode()) + len(titles[-1].encode()) <= fs.MAX_DOC_BYTES
    return texts, titles, tags


def _route_cases(places):
    return [c for c in fs.ascii_cases('a') if c.tags['m'] in fs.KEY_LENGTHS and c.tags['kind'] in ('indel', 'clip')
            and c.tags['place'] in places]


def nonascii_docs():
    """The never-thinned lengths' cases with one non-ASCII code point in the field (e-acute, a code point of the
    KB's non-ASCII names, and a CJK one of no name, by turns): far from the variant, directly before it, directly
    after it and, for one case in four, inside it; then the non-ASCII names' own cases."""
    fields = []
    for i, c in enumerate(_route_cases(('middle', 'start', 'end', 'whole'))):
        cp = 'é中'[i % 2]
        v, place = c.variant, c.tags['place']
        plain = fs.build_field(v, place)
        made = [('before', fs.build_field(cp + v, place)), ('after', fs.build_field(v + cp, place))]
        if place != 'whole':
            made.append(('far', plain + cp if place == 'start' else cp + plain))
        if i % 4 == 0:
            j = len(v) // 3
            made.append(('inside', fs.build_field(v[:j] + cp + v[j:], place)))
        fields += [(s, dict(c.tags, na=where, cp=cp)) for where, s in made]
    texts, titles, tags = _alternate(fields)
    t2, i2, g2 = fs.documents(fs.nonascii_cases())
    return texts + t2, titles + i2, tags + g2


def generic_docs():
    """Middle, start and end placements with 65 occurrences of the uppercase name in the field, away from the
    variant: after the filler (middle, start) or before it (end)."""
    many = ' '.join([UPPER] * 65)
    fields = []
    for c in _route_cases(('middle', 'start', 'end')):
        plain = fs.build_field(c.variant, c.tags['place'], side=12)      # (a document has at most 400 bytes)
        s = many + ' ' + plain if c.tags['place'] == 'end' else plain + ' ' + many
        fields.append((s, dict(c.tags, many=65)))
    return _alternate(fields)


def geometry_docs(permute):
    """The small KB's documents in generator order or in a fixed permutation, an empty document after every 31st:
    the cases fall on other lanes and group edges."""
    texts, titles, tags = default_docs('small')
    order = list(range(len(texts)))
    if permute:
        random.Random('fuzzy-sweep-geometry').shuffle(order)
    ot, oi, og = [], [], []
    for k, d in enumerate(order):
        ot.append(texts[d])
        oi.append(titles[d])
        og.append(dict(tags[d], src=d))
        if k % 31 == 30:
            ot.append('')
            oi.append('')
            og.append({'kind': 'empty', 'src': -1})
    return ot, oi, og


# ------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize('which', ['small', 'big'])
def test_default_path(oracles, which):
    """The group epilogue, kw_verify_kernel and kw_short_kernel; 57 fuzzy names (every short field takes the
    epilogue's signature pretest) and 127 (fields of up to 32 code points do not)."""
    texts, titles, tags = default_docs(which)
    m = _matcher(which)
    try:
        n_fuzzy = sum(1 for c in m.ckb.classes if c == 'F')
        assert n_fuzzy == (57 if which == 'small' else 127)
        got = _scan(m, texts, titles)
        routes, count = _routes(m, len(texts))
        st = m.stats()
        _equal(got, oracles[which].grouped(texts, titles), m, texts, titles, tags, f'default/{which}')
    finally:
        m.close()
    assert count['SCAN'] == len(texts), count
    assert st['lcs_windows'] > 0 and st['verifications'] > 0 and st['edge_items'] > 0, st


def test_per_document_epilogue(oracles, tmp_path):
    """kw_epi_kernel (KW_DEV=1, KW_EPI_FLAT=0).  The library reads KW_EPI_FLAT once per process, at its first scan,
    so setting it in a process that has scanned before changes nothing: the scan runs in a fresh process
    (tests/fuzzy_sweep_worker.py), which checks that the knobs were in place before its first scan, and its
    records are compared here with the default path's and the oracle's."""
    from advanced_scrapper_amd import _native
    from advanced_scrapper_amd.matcher import group_hits
    texts, titles, tags = default_docs('small')
    out = str(tmp_path / 'hits.npy')
    env = dict(os.environ, KW_DEV='1', KW_EPI_FLAT='0')
    r = subprocess.run([sys.executable, '-m', 'tests.fuzzy_sweep_worker', out], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info['epi_flat'] == '0' and info['dev'] == '1' and info['first_scan'] and info['docs'] == len(texts)
    per_doc = group_hits(np.load(out).view(_native.HIT_DTYPE).reshape(-1))
    m = _matcher('small')
    try:
        default = _scan(m, texts, titles)
        if m.stats()['rescans']:
            default = _scan(m, texts, titles)      # (the grown task queues: the statistics of one pass)
        st = m.stats()
        print(f'default path stats {st}')
        _equal(per_doc, oracles['small'].grouped(texts, titles), m, texts, titles, tags, 'per-document epilogue')
    finally:
        m.close()
    assert per_doc == default
    print(f'per-document epilogue stats {info["stats"]}')
    # The other epilogue really ran.  Filter and probe are the same (equal candidates, anchor hits, edge items), but
    # the two epilogues queue their verify tasks differently (the group epilogue works name groups across a batch of
    # documents, the per-document one a document's items), so for one pass over this fixed corpus the task kernels
    # count different work for the same hits: 227 426 LCS windows / 48 779 verifications after the group epilogue,
    # 228 598 / 48 958 after the per-document one (MI355X; the counts are sums over decisions, not timing).  Equal
    # counters would mean the same epilogue ran twice: look for another witness before relaxing this.
    assert st['rescans'] == 0 and info['stats']['rescans'] == 0
    for k in ('candidates', 'anchor_hits', 'edge_items'):
        assert info['stats'][k] == st[k], k
    assert (info['stats']['lcs_windows'], info['stats']['verifications']) != (st['lcs_windows'], st['verifications']), st


def test_transcoded_view(oracles):
    from advanced_scrapper_amd import _native
    texts, titles, tags = nonascii_docs()
    m = _matcher('big')
    try:
        got = _scan(m, texts, titles)
        routes, count = _routes(m, len(texts))
        _equal(got, oracles['big'].grouped(texts, titles), m, texts, titles, tags, 'transcoded view')
    finally:
        m.close()
    assert count['TRANSCODE'] > len(texts) * 3 // 4, count
    # the non-ASCII names' own cases too
    own = [d for d, t in enumerate(tags) if t['family'] == 'na']
    assert own and int((routes[own] == _native.KW_ROUTE_TRANSCODE).sum()) > len(own) // 2, count


@pytest.mark.parametrize('mode', ['no_markers', 'no_room'])
def test_resolve_kernel(oracles, monkeypatch, mode):
    """The same non-ASCII documents when the view cannot take them: every non-ASCII name without markers
    (KW_TEST_TX_MARKERS=0) or no room in the view (KW_TEST_TX_CAP=16), on a fresh handle."""
    if mode == 'no_markers':
        monkeypatch.setenv('KW_TEST_TX_MARKERS', '0')
    else:
        monkeypatch.setenv('KW_TEST_TX_CAP', '16')
    texts, titles, tags = nonascii_docs()
    m = _matcher('big')
    try:
        got = _scan(m, texts, titles)
        _routes_of, count = _routes(m, len(texts))
        _equal(got, oracles['big'].grouped(texts, titles), m, texts, titles, tags, f'resolve/{mode}')
    finally:
        m.close()
    assert count['RESOLVE'] > 0, count
    if mode == 'no_room':
        assert count['TRANSCODE'] == 0 and count['RESOLVE'] > len(texts) * 3 // 4, count


def test_generic_kernel(oracles):
    from advanced_scrapper_amd import _native
    texts, titles, tags = generic_docs()
    m = _matcher('small')
    try:
        got = _scan(m, texts, titles)
        routes, count = _routes(m, len(texts))
        st = m.stats()
        _equal(got, oracles['small'].grouped(texts, titles), m, texts, titles, tags, 'generic kernel')
    finally:
        m.close()
    # more than 64 items of one name in a text: the generic kernel.  In a title they are also more items than the
    # epilogue holds for a title (64): the big-document queue of its workgroup and then the generic kernel, or,
    # when that queue is full, the resolve kernel's big documents (which decide on code points too)
    in_text = np.array([t['in'] == 'text' for t in tags])
    assert int((routes[in_text] == _native.KW_ROUTE_GENERIC).sum()) == int(in_text.sum()) > 1000, count
    assert count['GENERIC'] + count['RESOLVE'] == len(texts), count
    assert st['deferred_docs'] >= int(in_text.sum()), st


_PER_SOURCE = {}      # test_group_geometry's results by source document, one entry per pass


@pytest.mark.parametrize('permute', [False, True], ids=['in_order', 'permuted'])
def test_group_geometry(oracles, permute):
    """One pass in generator order, one in a fixed permutation, an empty document after every 31st: per document
    the results are the oracle's, and the same in both passes."""
    texts, titles, tags = geometry_docs(permute)
    assert texts[31] == '' and titles[31] == '' and texts[30] != '' and len(texts) % 32 != 0
    m = _matcher('small')
    try:
        got = _scan(m, texts, titles)
        _routes_of, count = _routes(m, len(texts))
        _equal(got, oracles['small'].grouped(texts, titles), m, texts, titles, tags,
               f'geometry/{"permuted" if permute else "in order"}')
    finally:
        m.close()
    assert count['SCAN'] == len(texts), count
    assert not any(got.get(d) for d, t in enumerate(tags) if t['src'] < 0)
    _PER_SOURCE[permute] = {t['src']: got.get(d) for d, t in enumerate(tags) if t['src'] >= 0}
    if len(_PER_SOURCE) == 2:
        assert _PER_SOURCE[False] == _PER_SOURCE[True]
