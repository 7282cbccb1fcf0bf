"""The byte-geometry sweep of tests/filter_geometry.py through kw_filter_kernel and kw_probe_kernel
(csrc/kwmatch_split.hpp): exact names on tile edges, lane edges, a group's first and last bytes and across field,
document and group boundaries, under four KBs that differ only in their 2-3 byte uppercase names and so compile the
four stage-1 gates fk_stage1<0..3> (asserted through kw_filter_variant).

Every test compares the scan's records (document, field, name, code-point position) with the CPU oracle
(tests/oracle_matcher.OracleMatcher) on the same strings, bit-exact, and names the case label and the classifier's
tags of an occurrence that differs.  All-ASCII documents must stay on the fast path (KW_ROUTE_SCAN, nothing
deferred, no rescan on the second scan of a corpus): the generic kernel would hide the errors this sweep is for.
tests/test_filter_geometry_cases.py holds the builder to its tag table and the oracle to the planted intent."""
import numpy as np
import pytest

from tests import filter_geometry as fg

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, 2, 3)


class _Oracles:
    """The oracle's record set per (KB, corpus), computed once."""

    def __init__(self):
        self.seen = {}

    def records(self, variant, fuzzy, c):
        key = (variant, fuzzy, c.label)
        if key not in self.seen:
            om = self.seen.get((variant, fuzzy))
            if om is None:
                from tests.oracle_matcher import OracleMatcher
                om = self.seen[(variant, fuzzy)] = OracleMatcher(fg.processed(fg.kb_names(variant, fuzzy)))
            rec = om.match_strings(*c.strings())
            self.seen[key] = _as_set(rec, om.ckb.names)
        return self.seen[key]


def _as_set(rec, names):
    out = set(zip(rec['doc'].tolist(), rec['field'].tolist(), (names[p] for p in rec['pattern'].tolist()),
                  rec['pos'].tolist()))
    assert len(out) == len(rec), 'a record twice'
    return out


@pytest.fixture(scope='module')
def oracles():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return _Oracles()


def _matcher(variant, fuzzy=True):
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    m = GpuMatcher(compile_kb(fg.processed(fg.kb_names(variant, fuzzy))))
    # the expectation was worked out from kw_compile's box arithmetic: a KB that lands elsewhere is the KB's fault
    assert m.filter_variant() == variant, (variant, m.filter_variant())
    return m


def _scan(m, c, entry):
    from advanced_scrapper_amd.matcher import pack_fields
    texts, titles = c.strings()
    if entry == 'host':
        return m.match_strings(texts, titles)
    arena, off = pack_fields(texts, titles)
    d_arena, d_off = m.upload(arena, off)
    m.scan(d_arena, d_off, len(texts))
    return m.fetch()


def _describe(c, recs):
    """Case labels and classifier tags of the planted occurrences behind some (doc, field, name, position) records."""
    off, arena = c.offsets(), c.arena()
    out = []
    for d, f, name, pos in sorted(recs)[:6]:
        fb = c.fields[2 * d + f]
        hit = [(s, lb) for dd, ff, s, n, lb in c.plants if (dd, ff, n) == (d, f, name) and len(fb[:s].decode()) == pos]
        if hit:
            s, lb = hit[0]
            out.append(f'{name!r} doc {d} field {f} pos {pos} [{lb}] tags {fg.tags(off, d, f, s, len(name.encode()), arena)}')
        else:
            out.append(f'{name!r} doc {d} field {f} pos {pos} [not planted] {fb[max(0, pos - 8):pos + 24]!r}')
    return out


def _check(m, oracles, variant, c, entry, what, fuzzy=True, strict=True):
    """One corpus, scanned twice on the handle: records equal to the oracle's; all-ASCII documents on the fast path."""
    from advanced_scrapper_amd import _native
    want = oracles.records(variant, fuzzy, c)
    texts, titles = c.strings()
    for rep in (0, 1):
        got = _as_set(_scan(m, c, entry), m.ckb.names)
        st = m.stats()
        lost, extra = want - got, got - want
        assert not lost and not extra, (
            f'{what}, corpus {c.label}, scan {rep}: {len(lost)} records lost, {len(extra)} not the oracle\'s; lost: '
            f'{_describe(c, lost)}; extra: {_describe(c, extra)}; stats {st}')
    routes = m.doc_routes(len(texts))
    ascii_doc = np.array([(a + b).isascii() for a, b in zip(texts, titles)])
    print(f'{what}, corpus {c.label}: routes (scan, resolve, generic, transcode) '
          f'{np.bincount(routes, minlength=4).tolist()}, non-ASCII documents {int((~ascii_doc).sum())} with routes '
          f'{np.bincount(routes[~ascii_doc], minlength=4).tolist()}, rescans {st["rescans"]} causes '
          f'{st["rescan_causes"]}, stage-2 candidates {st["candidates_stage2"]}')
    if strict:
        off_path = np.flatnonzero(ascii_doc & (routes != _native.KW_ROUTE_SCAN))
        assert not len(off_path), (what, c.label, 'all-ASCII documents off the fast path', off_path[:8].tolist(),
                                   routes[off_path[:8]].tolist())
        assert st['deferred_docs'] == 0, (what, c.label, st)
        assert st['rescans'] == 0, (what, c.label, 'the second scan of the corpus rescanned', st)
    return st


# ------------------------------------------------------------------------------------------------ the main corpora
@pytest.mark.parametrize('entry', ['scan', 'host'])
@pytest.mark.parametrize('variant', VARIANTS)
def test_main_corpora(oracles, variant, entry):
    """Device tensors through kw_scan, and match_strings through kw_scan_host: every corpus, each gate."""
    m = _matcher(variant)
    try:
        for c in fg.cases():
            _check(m, oracles, variant, c, entry, f'gate {variant}, {entry}')
    finally:
        m.close()


@pytest.mark.parametrize('setting', ['chunk3', 'chunk64', 'static'])
@pytest.mark.parametrize('variant', VARIANTS)
def test_several_groups_in_one_region(oracles, monkeypatch, variant, setting):
    """KW_CHUNK_GROUPS=3 / 64 (several groups, then all of a small corpus's, in one candidate region: the group
    header records, the probe's cur_group carried over its batches of 64) and the grid-stride filter
    (KW_STATIC_GROUPS=1); read per scan under KW_DEV=1."""
    monkeypatch.setenv('KW_DEV', '1')
    if setting == 'static':
        monkeypatch.setenv('KW_STATIC_GROUPS', '1')
    else:
        monkeypatch.setenv('KW_CHUNK_GROUPS', setting[5:])
    m = _matcher(variant)
    try:
        for c in fg.cases():
            _check(m, oracles, variant, c, 'host', f'gate {variant}, {setting}')
    finally:
        m.close()


@pytest.mark.parametrize('variant', [0, 3])
def test_one_item_per_verified_use(oracles, variant):
    """KBs of uppercase names only: the probe's items of every field are the oracle's positions in it, one verified
    use an item (no two occurrences overlap: tests/test_filter_geometry_cases.py)."""
    m = _matcher(variant, fuzzy=False)
    try:
        for c in fg.cases():
            _check(m, oracles, variant, c, 'host', f'gate {variant}, uppercase only', fuzzy=False)
            want = np.zeros((c.n_docs, 2), dtype=np.int64)
            for d, f, _name, _pos in oracles.records(variant, False, c):
                want[d, f] += 1
            items = m.doc_items(c.n_docs).astype(np.int64)
            bad = np.argwhere(items != want)
            assert not len(bad), (variant, c.label, [(int(d), int(f), int(items[d, f]), int(want[d, f])) for d, f in bad[:8]])
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ the dense corpus
@pytest.mark.parametrize('variant', VARIANTS)
def test_dense_runs_keep_the_ring_full(oracles, variant):
    """Runs of a 2-byte name without separators: every position or every second one survives stage 1 and stage 2,
    none matches; the entry ring stays full and rounds take fewer than 64 entries.  Rescans are a legitimate route."""
    m = _matcher(variant)
    try:
        for c in fg.dense_cases():
            st = _check(m, oracles, variant, c, 'host', f'gate {variant}, dense', strict=False)
            planted = fg.dense_survivors(c, fg.kb_names(variant))
            print(f'gate {variant}, dense: planted survivors {planted}, stats {st}')
            assert st['candidates_stage2'] >= planted, (planted, st)
    finally:
        m.close()
