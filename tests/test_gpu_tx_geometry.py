"""The byte-geometry sweep (tests/tx_geometry.py) through every route that decodes non-ASCII bytes: the transcoded
view (kw_tx_kernel / tx_field / tx_pos) under the batched, the one-at-a-time and the per-document epilogue, the
resolve kernel (decode_field_fast / to_cp_fast) and the generic kernel (decode_field).  Every test compares every
document's hits (all names, both fields, all positions) with the CPU oracle on the same strings, bit-exact, names
the geometry a differing document was built for, and asserts the route it claims to exercise.

The fields are concatenations of exact occurrences of KB names, so a wrong chunk count or tx_pos shifts every later
reported position and an overlapping view corrupts another document's; a wrong view byte changes the decision of
family j's fields, which end with a name less one letter.  The oracle's side
is computed once per KB and document list (a module fixture); tests/test_tx_geometry_cases.py holds the oracle
against a plain re.finditer loop on these fields and checks that every cell of every family is hit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tx_geometry as tg

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _docs(which):
    if which == 'generic':
        return tg.generic_corpus()
    if which == 'permuted':
        return tg.permuted_corpus()[:3]
    return tg.corpus()


class _Oracles:
    """oracle_pool.field_results per (KB, document list), computed once: what group_hits gives for the scan."""

    def __init__(self):
        self.seen = {}
        self.by_string = {}

    def grouped(self, kb, which):
        if (kb, which) not in self.seen:
            from advanced_scrapper_amd.kb import compile_kb
            from tests import oracle_pool
            names = tg.kb_names(kb)
            proc = tg.processed(names)
            pid = {n: i for i, n in enumerate(compile_kb(proc).names)}
            texts, titles, _tags = _docs(which)
            known = self.by_string.setdefault(kb, {})
            new = sorted({s for s in texts + titles if s not in known})
            if new:
                known.update(zip(new, oracle_pool.field_results(proc, new)))
            out = {}
            for d, pair in enumerate(zip(texts, titles)):
                for f, s in enumerate(pair):
                    r = {pid[n]: list(pos) for n, pos in known[s].items()}
                    if r:
                        out.setdefault(d, {})[f] = r
            self.seen[(kb, which)] = out
        return self.seen[(kb, which)]


@pytest.fixture(scope='module')
def oracles():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return _Oracles()


def _matcher(kb):
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    return GpuMatcher(compile_kb(tg.processed(tg.kb_names(kb))))


def _scan(kb, which):
    """(grouped hits, routes, statistics, the KB's names) of one scan on a fresh handle."""
    from advanced_scrapper_amd.matcher import group_hits
    texts, titles, _tags = _docs(which)
    m = _matcher(kb)
    try:
        got = group_hits(m.match_strings(texts, titles))
        routes = m.doc_routes(len(texts))
        st = m.stats()
        names = list(m.ckb.names)
    finally:
        m.close()
    return got, routes, st, names


def _equal(got, want, names, which, what):
    texts, titles, tags = _docs(which)
    bad = [d for d in range(len(texts)) if got.get(d) != want.get(d)]
    for d in bad[:6]:
        for f in (0, 1):
            g, w = (got.get(d) or {}).get(f, {}), (want.get(d) or {}).get(f, {})
            diff = {names[p]: (g.get(p), w.get(p)) for p in sorted(set(g) | set(w)) if g.get(p) != w.get(p)}
            if diff:
                some = dict(list(diff.items())[:3])
                print(f'{what} doc {d} [{tags[d]}] field {f}: {len(diff)} names differ, (got, want) {some}')
    assert not bad, (f'{what}: GPU differs from the oracle on {len(bad)} of {len(texts)} documents; the first: '
                     + '; '.join(f'{d} [{tags[d]}]' for d in bad[:8]))


def _nonascii(which):
    texts, titles, _tags = _docs(which)
    return np.array([not (a + b).isascii() for a, b in zip(texts, titles)])


def _over_cap(which):
    texts, _titles, _tags = _docs(which)
    return np.array([not t.isascii() and len(t.encode()) > tg.FK_CP_CAP for t in texts])


def _route(name):
    from advanced_scrapper_amd import _native
    return getattr(_native, 'KW_ROUTE_' + name)


def _assert_routes(routes, mask, name, which, what):
    _texts, _titles, tags = _docs(which)
    off = np.flatnonzero(mask & (routes != _route(name)))
    back = {_route(k): k for k in ('SCAN', 'TRANSCODE', 'RESOLVE', 'GENERIC')}
    assert not len(off), (f'{what}: {len(off)} of {int(mask.sum())} documents did not report {name}; the first: '
                          + '; '.join(f'{d} {back[int(routes[d])]} [{tags[d]}]' for d in off[:8]))


def _classes(which):
    texts, titles, _tags = _docs(which)
    return np.array(tg.item_classes(texts, titles, tg.fuzzy_names('over')))


def _view_routes(routes, st, which, what, resolve=()):
    """Every document with a non-ASCII field on the transcoded view, but the text over FK_CP_CAP bytes and the
    item classes (tx_geometry.item_classes) in `resolve`, which report the resolve kernel."""
    na, over = _nonascii(which), _over_cap(which)
    cls = _classes(which)
    assert int(over.sum()) == 1 and {'batch', 'wave', 'big'} == set(cls[na].tolist())
    left = na & (over | np.isin(cls, list(resolve)))
    print(f'{what}: routes {np.bincount(routes, minlength=4).tolist()} (scan, resolve, generic, transcode), '
          f'non-ASCII documents {int(na.sum())}, stats {st}')
    _assert_routes(routes, left, 'RESOLVE', which, what)
    _assert_routes(routes, na & ~left, 'TRANSCODE', which, what)
    assert st['big_docs'] > 0, st


# ------------------------------------------------------------------------------------------------ the view
def test_view_batched(oracles):
    """a. KB base, default settings: no name is PI_TXUNSAFE, kw_epi_flat_kernel<true> batches the transcoded
    documents (tx_pos lane by lane).  Its batches hold 64 items a field: every document outside family f stays
    below that and reports the view; family f's five documents, built to pass it, are the resolve kernel's by
    design and take the view in the next test."""
    got, routes, st, names = _scan('base', 'corpus')
    _equal(got, oracles.grouped('base', 'corpus'), names, 'corpus', 'view, batched')
    _view_routes(routes, st, 'corpus', 'view, batched', resolve=('wave', 'big'))


def test_view_one_document_at_a_time(oracles, monkeypatch):
    """b. KW_TEST_EPI_TXB=0 (read per scan): epi_tx_doc's own tx_pos use, and epi_big_doc's for the big documents."""
    monkeypatch.setenv('KW_TEST_EPI_TXB', '0')
    got, routes, st, names = _scan('base', 'corpus')
    _equal(got, oracles.grouped('base', 'corpus'), names, 'corpus', 'view, one document at a time')
    _view_routes(routes, st, 'corpus', 'view, one document at a time')


def test_per_document_epilogue(oracles, tmp_path):
    """c. kw_epi_kernel (KW_DEV=1, KW_EPI_FLAT=0, read once per process): a fresh process scans
    (tests/tx_geometry_worker.py) and checks that the knobs were in place before its first scan."""
    from advanced_scrapper_amd import _native
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import group_hits
    texts, _titles, _tags = tg.corpus()
    out = str(tmp_path / 'hits.npy')
    env = dict(os.environ, KW_DEV='1', KW_EPI_FLAT='0')
    r = subprocess.run([sys.executable, '-m', 'tests.tx_geometry_worker', out], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info['epi_flat'] == '0' and info['dev'] == '1' and info['first_scan'] and info['docs'] == len(texts)
    got = group_hits(np.load(out).view(_native.HIT_DTYPE).reshape(-1))
    names = list(compile_kb(tg.processed(tg.kb_names('base'))).names)
    _equal(got, oracles.grouped('base', 'corpus'), names, 'corpus', 'per-document epilogue')
    # (kw_epi_kernel has one wave's item buffers and no big-document queue for the view: past them, the resolve kernel)
    _view_routes(np.load(out + '.routes.npy'), info['stats'], 'corpus', 'per-document epilogue', resolve=('big',))


# ------------------------------------------------------------------------------------------------ resolve, generic
@pytest.mark.parametrize('mode', ['no_markers', 'no_room'])
def test_resolve_kernel(oracles, monkeypatch, mode):
    """d, e. decode_field_fast / to_cp_fast over the same geometry: no name has a marker (KW_TEST_TX_MARKERS=0,
    every non-ASCII name PI_TXUNSAFE) or the view has no room (KW_TEST_TX_CAP=16), on a fresh handle."""
    monkeypatch.setenv('KW_TEST_TX_MARKERS' if mode == 'no_markers' else 'KW_TEST_TX_CAP', '0' if mode == 'no_markers' else '16')
    got, routes, st, names = _scan('base', 'corpus')
    _equal(got, oracles.grouped('base', 'corpus'), names, 'corpus', f'resolve/{mode}')
    na = _nonascii('corpus')
    print(f'resolve/{mode}: routes {np.bincount(routes, minlength=4).tolist()}, stats {st}')
    assert int((routes == _route('TRANSCODE')).sum()) == 0
    _assert_routes(routes, na, 'RESOLVE', 'corpus', f'resolve/{mode}')


def test_generic_kernel(oracles):
    """f. 65 occurrences of one uppercase name after every text: more than 64 items of one name, decode_field.
    Every document is deferred to the generic kernel (the statistics).  kw_doc_routes reports GENERIC for those the
    epilogue defers, the all-ASCII ones; a document with a non-ASCII field is first the resolve kernel's (more than
    64 items in a field), which defers it in turn and leaves its route at RESOLVE."""
    got, routes, st, names = _scan('base', 'generic')
    _equal(got, oracles.grouped('base', 'generic'), names, 'generic', 'generic kernel')
    print(f'generic: routes {np.bincount(routes, minlength=4).tolist()}, stats {st}')
    na = _nonascii('generic')
    assert st['deferred_docs'] == len(routes), st
    _assert_routes(routes, ~na, 'GENERIC', 'generic', 'generic kernel')
    _assert_routes(routes, na, 'RESOLVE', 'generic', 'generic kernel')
    assert st['resolved_docs'] == int(na.sum()), st


# ------------------------------------------------------------------------------------------------ the marker table
def test_full_marker_table(oracles):
    """g. KB full: 127 distinct non-ASCII code points, probe chains of 4 and over the wrap at slot 255."""
    got, routes, st, names = _scan('full', 'corpus')
    _equal(got, oracles.grouped('full', 'corpus'), names, 'corpus', 'full marker table')
    _view_routes(routes, st, 'corpus', 'full marker table', resolve=('wave', 'big'))      # (batched, as in a)


def test_marker_overflow(oracles):
    """h. KB over: the name with the 128th code point is PI_TXUNSAFE; its documents leave the view."""
    got, routes, st, names = _scan('over', 'corpus')
    _equal(got, oracles.grouped('over', 'corpus'), names, 'corpus', 'marker overflow')
    texts, titles, _tags = tg.corpus()
    name = tg.kb_names('over')[-4]
    holds = np.array([name in a or name in b for a, b in zip(texts, titles)])
    print(f'marker overflow: routes {np.bincount(routes, minlength=4).tolist()}, stats {st}')
    assert int(holds.sum()) >= 3
    _assert_routes(routes, holds, 'RESOLVE', 'corpus', 'marker overflow')
    assert int((routes[_nonascii('corpus')] == _route('TRANSCODE')).sum()) > 0


# ------------------------------------------------------------------------------------------------ permutation
def test_permuted(oracles):
    """i. A seeded permutation with an empty document after every 31st: every alignment and every wave's
    membership changes; families a and d are still fully hit on the permuted packing."""
    from advanced_scrapper_amd.matcher import pack_fields
    texts, titles, tags, src = tg.permuted_corpus()
    arena, off = pack_fields(texts, titles)
    assert tg.missing_a(tg.cells_a(arena, off)) == [] and tg.missing_d(tg.cells_d(arena, off)) == []
    got, routes, st, names = _scan('base', 'permuted')
    want = oracles.grouped('base', 'permuted')
    _equal(got, want, names, 'permuted', 'permuted')
    plain = oracles.grouped('base', 'corpus')
    assert all(want.get(k) == plain.get(s) for k, s in enumerate(src) if s >= 0)
    assert not any(got.get(k) for k, s in enumerate(src) if s < 0)
    print(f'permuted: routes {np.bincount(routes, minlength=4).tolist()}, stats {st}')
    assert int((routes[_nonascii('permuted')] == _route('TRANSCODE')).sum()) > 0
