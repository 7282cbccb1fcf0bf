"""CPU: the generators of tests/dedup_geometry.py held to their claims, where no GPU is needed, so that a later edit
cannot hollow the sweep out: a census of every family through ``route()`` (the kernel's route choice restated),
``route()`` itself against the oracle on every family row and a seeded token fuzz, and the stage and claim edges
computed from the library's own constants (``kw_dedup_geometry``)."""
import collections
import ctypes

import numpy as np
import pytest

from oracle import dedup_oracle as dd
from tests import dedup_geometry as G


@pytest.fixture(scope='module')
def geometry():
    """kw_dedup_geometry() by name: host code, no device."""
    from advanced_scrapper_amd import _native
    v = (ctypes.c_int32 * len(G.GEOMETRY_NAMES))()
    assert _native.lib().kw_dedup_geometry(v, len(v)) == 0
    return dict(zip(G.GEOMETRY_NAMES, (int(x) for x in v)))


def test_generators_constants_are_the_librarys(geometry):
    assert geometry == G.GEOMETRY
    from advanced_scrapper_amd import _native
    assert 'kw_dedup_geometry' in _native.EXPORTS and 'kw_dedup_route_counts' in _native.EXPORTS
    v = (ctypes.c_int32 * 3)(-1, -1, -1)
    assert _native.lib().kw_dedup_geometry(v, 2) == 0 and list(v) == [G.GEOMETRY['STAGE_BYTES'], G.GEOMETRY['TCLAIM'], -1]
    assert _native.lib().kw_dedup_geometry(None, 2) == _native.KW_EINVAL


def test_pack_is_exact_and_hostile():
    rows = ['ab', '', 'é', '\ud800']
    arena, off = G.pack(rows)
    assert off.tolist() == [0, 2, 2, 4, 7] and arena.dtype == np.uint8 and off.dtype == np.int64
    assert len(arena) == 7 + 32 and bytes(arena[7:]) == G.PAD
    assert G.PAD.startswith(b"lhtml:80http:news/%'") and set(G.PAD[20:]) == {0xFF} and len(G.PAD) == 32


# ------------------------------------------------------------------ route() against the oracle
def test_route_equals_oracle_on_families_and_fuzz():
    """no_html <=> the regex finds nothing; filtered <=> the oracle drops a row the regex matched; the Python
    FastWords bytes (and the byte-serial rewrite's) equal the oracle's normalised URL."""
    rows = sum((G.family_rows(f) for f in G.FAMILIES), []) + G.fuzz_strings(20000)
    assert len(G.fuzz_strings(20000)) == 20000 and len(set(G.fuzz_strings(20000))) > 15000
    seen = collections.Counter()
    for u in rows:
        b = G.enc(u)
        r = G.route(b)
        want = dd.url_transform_bytes(b)
        matched = dd._HTML.search(u) is not None
        assert (r.route == 'no_html') == (not matched), u
        if not matched:
            continue
        assert r.filtered == (want is None), u
        if want is not None:
            assert r.norm == want, u
        if r.route in G.FAST_ROUTES:
            assert len(r.norm) == r.E + 5
        seen[r.route, r.filtered] += 1
    for name in G.ROUTES[1:]:
        assert seen[name, False] > 100 and seen[name, True] > 10, name


def test_codes_helper():
    rows = ['a.html', 'a.html?x', 'nothing', 'https://x/news/%a.html', 'b.html']
    assert G.oracle_codes(rows).tolist() == [1, 3, 0, 2, 1]
    assert G.oracle_codes(rows, normalize=False).tolist() == [1, 1, 1, 1, 1]
    e = G.expected(rows)
    assert e.kept_rows.tolist() == [0, 4] and e.kept_bytes == b'a.htmlb.html' and e.kept_off.tolist() == [0, 6, 12]
    assert e.counts == [1, 2, 1, 1]


# ------------------------------------------------------------------ the census, family by family
def test_census_align_cut():
    b = G.align_cut()
    rs = [(G.route(G.enc(r)), s) for r, s in G.marked(b)]
    for name in ('fast', 'ins', 'no_html'):
        assert {s % 16 for r, s in rs if r.route == name} == set(range(16)), name
    for name in ('fast', 'ins'):
        assert {r.E % 8 for r, _ in rs if r.route == name} == set(range(8))
        assert {r.cut % 8 for r, _ in rs if r.route == name} == set(range(8))
        # (E, start modulo 16) jointly, for E >> 3 from 0 to 2 (3 with the scheme)
        assert {(r.E, s % 16) for r, s in rs if r.route == name} >= {(e, s) for e in range(7, 24) for s in range(16)}
    assert {r.E >> 3 for r, _ in rs if r.route != 'no_html'} == {0, 1, 2, 3}
    assert any(r.E == 0 for r, _ in rs if r.route == 'fast')
    # a filler that ends in "htm" right before a row that starts with 'l', at several starts
    rows = b.rows
    cross = [i for i in b.marks if rows[i].startswith('l') and rows[i - 1].endswith('htm')]
    starts = b.starts()
    assert len(cross) > 50 and len({starts[i] % 16 for i in cross}) >= 3
    assert all(G.route(G.enc(rows[i - 1])).route == 'no_html' for i in b.marks)
    n_l = sum(rows[i].startswith('l') for i in b.marks)
    n_plain = sum(not rows[i].startswith('http') for i in b.marks)
    assert 0.2 < n_l / n_plain <= 0.25


def test_census_cut_rule():
    b = G.cut_rule()
    rows = [r for r, _ in G.marked(b)]
    st = collections.defaultdict(set)
    for r, s in G.marked(b):
        st[r].add(s % 4)
    assert all(v == {0, 1, 2, 3} for r, v in st.items() if r in ('\nhtml', 'news/%html', '😀html', 'xxxhtm'))
    assert dd.url_transform('\nhtml') is None and dd.url_transform('htmlxhtml') == 'html.html'
    assert dd.url_transform('news/%html') == 'news/.html' and dd.url_transform('https://a/news/%html') == 'https://a/news/.html'
    # the '\nhtml' + 'xhtml' pair: the invalid candidate in either half of an 8-byte step and the valid one behind
    # it in the same step, the next half, the next step
    cells = set()
    for r in rows:
        k = r.find('\nhtml')
        v = G.route(G.enc(r))
        if k >= 0 and v.route == 'fast' and r.isascii() and v.cut > k:
            qi, qv = k + 1, v.cut + 1                    # (half of the invalid one, half of the valid one, steps apart)
            cells.add(((qi % 8) // 4, (qv % 8) // 4, qv // 8 - qi // 8))
    assert cells >= {(0, 1, 0), (1, 0, 1), (0, 0, 1), (0, 1, 1), (1, 1, 1)}
    # two valid candidates in one 8-byte step: the first wins
    assert any(r.endswith('ahtmlbhtml') and G.route(G.enc(r)).cut % 8 <= 2 for r in rows)
    # the code point before "html": 1 to 4 bytes and the lone surrogate, the cut at every residue modulo 4
    for cp in ('a', 'é', '中', '😀', '\ud800'):
        cuts = {G.route(G.enc(r)).cut % 4 for r in rows if r.endswith(cp + 'html?')}
        assert cuts == {0, 1, 2, 3}, cp
        assert dd.url_transform(cp + 'html') == '.html'
    assert len(G.enc('\ud800')) == 3
    # 'x' * k + 'html' at every length 0..15: "html" ending exactly at L, one to three bytes short, and long
    ends = collections.Counter()
    for k in range(12):
        for L in range(16):
            r = ('x' * k + 'html' + 'z' * 16)[:L]
            assert r in st
            ends[min(L - (k + 4), 1)] += G.route(G.enc(r)).route != 'no_html'
    assert ends[0] == 11 and ends[1] > 30 and ends[-1] == ends[-2] == ends[-3] == 0
    assert {len(r) for r in rows if set(r) <= {'x', 'h', 't', 'm'} and r.endswith('htm')} >= set(range(3, 15))


def test_census_gap():
    b = G.gap()
    rs = [(G.route(G.enc(r)), s, r) for r, s in G.marked(b)]
    for name in ('gap', 'ins_gap'):
        mine = [(r, s) for r, s, _ in rs if r.route == name]
        assert {s % 16 for _, s in mine} == set(range(16)), name
        assert {r.G % 8 for r, _ in mine} == set(range(8)) and {r.E % 8 for r, _ in mine} == set(range(8))
        for g in range(8):
            # ".html" right at the gap (ec + 3 == j), in the gap's word, in the next word; all starts modulo 4
            d = {(r.E - r.G, s % 4) for r, s in mine if r.G % 8 == g}
            assert {x for x, _ in d} >= set(range(10)), (name, g)
            assert d >= {(x, m) for x in range(10) for m in range(4)}
            assert any(r.E == r.G and r.ec + 3 == r.cut for r, _ in mine if r.G % 8 == g)
            assert any(r.E >> 3 == r.G >> 3 and r.E > r.G for r, _ in mine if r.G % 8 == g) or g == 7
            assert any(r.E >> 3 == (r.G >> 3) + 1 for r, _ in mine if r.G % 8 == g)
    want = {'abcde:80/x.html': 'slow', 'abcdef:80/x.html': 'gap', 'https://h:8html': 'slow', 'https://h:80html': 'slow',
            'https://h:80xhtml': 'gap', 'http://h:80xhtml': 'ins_gap', 'https://h:80/x.html:': 'gap',
            'https://h:80/x:html': 'gap', 'https://h:80/:x.html': 'slow', 'http:80/x.html': 'slow',
            'https:80/x.html': 'slow', 'https::80/x.html': 'gap', 'http::80/x.html': 'slow', 'http:html': 'fast', 'http:xhtml': 'ins'}
    got = {r: v.route for v, _, r in rs}
    assert {k: got[k] for k in want} == want
    assert set(G.GAP_BOUNDARY) <= set(got)
    for k in G.GAP_BOUNDARY:
        assert {s % 4 for _, s, r in rs if r == k} == {0, 1, 2, 3}
    assert dd.url_transform('https://h:80html') == 'https://h:8.html' and dd.url_transform('http:80/x.html') == 'http/x.html'


def test_census_filter():
    b = G.filter_rows()
    rows = [r for r, _ in G.marked(b)]
    rs = {r: G.route(G.enc(r)) for r in rows}
    for c in ('%', "'"):
        assert {r.find('news/' + c) % 8 for r in rows if r.endswith('news/' + c + 'q.html') and dd.url_transform(r) is None} \
            == set(range(8))
        for sp in G.FILTER_SPLITS:                       # across the gap: the reference filters after the rewrite
            sp = sp.replace('%', c)
            for r, kind in (('https://hh/' + sp + 'a.html', 'gap'), ('http://hh/' + sp + 'a.html', 'ins_gap'),
                            ('http://hh/' + sp + 'xhtml', 'ins_gap')):
                assert rs[r].route == kind and rs[r].filtered and dd.url_transform(r) is None, r
            assert dd.url_transform('https://hh/' + sp + 'html') is not None or sp.endswith(':80' + c) is False
        assert dd.url_transform('https://a/news/' + c + 'html') == 'https://a/news/.html'        # ending at j: kept
        assert dd.url_transform('https://a/news/' + c + 'xhtml') is None                         # at j - 1: filtered
        assert dd.url_transform('https://a/NEWS/' + c + 'q.html') is not None
        assert dd.url_transform('news/' + c + 'a.html') is None and rs['news/' + c + 'a.html'].route == 'fast'
        assert dd.url_transform('https://hh/new:80s/x' + c + 'a.html') is not None
        assert rs['http://a:80/b:80/news/' + c + 'x.html'].route == 'slow' and rs['http://a:80/b:80/news/' + c + 'x.html'].filtered
    assert len(G.FILTER_SPLITS) == 5 and G.FILTER_SPLITS[0] == 'n:80ews/%' and G.FILTER_SPLITS[-1] == 'news/:80%'
    st = collections.defaultdict(set)
    for r, s in G.marked(b):
        st[r].add(s % 4)
    assert all(v == {0, 1, 2, 3} for v in st.values())
    by = collections.Counter((v.route, v.filtered) for v in rs.values())
    for name in ('fast', 'gap', 'ins_gap', 'slow'):
        assert by[name, True] and by[name, False], name


def test_census_slow():
    b = G.slow()
    rs = [(G.route(G.enc(r)), s, r) for r, s in G.marked(b)]
    for base in G.SLOW_BASE:
        assert {s % 8 for v, s, r in rs if r == base and v.route == 'slow'} == set(range(8)), base
    assert {len(v.norm) % 8 for v, _, _ in rs if v.route == 'slow'} == set(range(8))
    # 'http:' * m: six bytes out for five in, the growth slow_words() allows for
    v = G.route(G.enc('http:' * 12 + 'y.html'))
    assert v.route == 'slow' and len(v.norm) == 6 * 12 + 6 and v.norm == G.enc(dd.url_transform('http:' * 12 + 'y.html'))
    assert sum(v.route == 'slow' for v, _, _ in rs) > 250


def test_census_same_key():
    rows, meta = G.same_key()
    assert {len(N) for _, N in meta['spelled']} == set(G.SAME_KEY_LENS)
    for edge in (24, 64, 120, 128, 136, 256):
        assert {edge - 1, edge, edge + 1} <= set(G.SAME_KEY_LENS)
    first = {}
    pairs = set()
    for i, N in meta['spelled']:
        assert dd.url_transform(rows[i]) == N, rows[i]
        kind = [s for s in range(G.N_SPELLINGS) if G.spell(N, s) == rows[i]][0]
        assert G.route(G.enc(rows[i])).route == G.SPELLING_ROUTES[kind]
        if N not in first:
            first[N] = kind
        else:
            pairs.add((len(N), first[N], kind))
    # every spelling is the first occurrence once per length, and every ordered pair of spellings occurs
    for length in G.SAME_KEY_LENS:
        assert {(a, c) for n, a, c in pairs if n == length} == \
            {(a, c) for a in range(G.N_SPELLINGS) for c in range(G.N_SPELLINGS) if a != c}
    keys = set(first)
    kept = set(dd.dedup_rows(rows)[0])
    seen_near = set()
    for i, N, M in meta['near']:
        assert dd.url_transform(rows[i]) == M and M != N and len(M) == len(N)
        assert sum(x != y for x, y in zip(M, N)) == 1
        assert M not in keys and M not in seen_near and i in kept
        seen_near.add(M)
    for length in G.SAME_KEY_LENS:
        ps = G.near_miss_positions(length)
        assert 8 in ps and length - 6 in ps
        assert {p for p in range(15, length - 5) if p % 8 in (0, 7)} <= set(ps)
        if length > 134:
            assert 127 in ps and 128 in ps
    assert len({G.route(G.enc(rows[i])).route for i, _, _ in meta['near']}) == 5


def test_census_tail_twins(geometry):
    round_bytes = geometry['PAIR_LANES'] * geometry['PAIR_UNROLL'] * 8
    assert round_bytes == 128
    for length in G.TWIN_LENS:
        for spelled in (True, False):
            rows = G.tail_twins(length, spelled)
            keys = [dd.url_transform(r) for r in rows] if spelled else rows
            N = G.same_key_name(length)
            assert keys[0] == N and keys[-G.TWIN_REPEATS:] == [N] * G.TWIN_REPEATS
            assert all(len(k) == length and k[:round_bytes] == N[:round_bytes] for k in keys)
            assert len(set(keys)) == len(keys) - G.TWIN_REPEATS > 16 + 4
            assert {min(p for p in range(length) if k[p] != N[p]) for k in keys[1:-G.TWIN_REPEATS]} >= {128, 129, length - 6}
            if spelled:
                assert len({G.route(G.enc(r)).route for r in rows}) == 5
    assert any(n > 2 * round_bytes for n in G.TWIN_LENS)                 # a third round


def test_census_groups(geometry):
    S, T = geometry['STAGE_BYTES'], geometry['TCLAIM']
    assert {T * 64 - 1, T * 64, T * 64 + 1, geometry['SCAN_TILE'] - 1, geometry['SCAN_TILE'], geometry['SCAN_TILE'] + 1,
            1, 63, 64, 65} == set(G.GROUP_ROW_COUNTS)
    rows = G.groups_run()
    nch = G.group_nch(rows)
    assert set(G.GROUP_NCH) <= set(nch)
    staged = [n for n in nch if n * 16 + 16 <= S]
    assert max(staged) == 511 and min(n for n in nch if n not in staged) == 512
    assert max(staged) * 16 + 32 > S                                  # 511 is the last staged value
    # side by side: a staged group next to a global one, both ways
    flips = {(a * 16 + 16 <= S, b * 16 + 16 <= S) for a, b in zip(nch, nch[1:])}
    assert {(True, False), (False, True)} <= flips
    assert any(n > 9000 // 16 for n in nch) and 2 in nch               # the 9000-byte row's group; 64 empty rows
    assert len(rows) % 64 != 0
    # both transform routes see every plan kind, and duplicates fall on both sides of a route change
    by = {True: set(), False: set()}
    where = collections.defaultdict(set)
    keys = [dd.url_transform(r) for r in rows]
    for i, r in enumerate(rows):
        st = nch[i // 64] * 16 + 16 <= S
        by[st].add(G.route(G.enc(r)).route)
        if keys[i] is not None:
            where[keys[i]].add(st)
    assert by[True] == set(G.ROUTES) and by[False] == set(G.ROUTES)
    assert sum(len(v) == 2 for v in where.values()) > 50
    for n in G.GROUP_ROW_COUNTS:
        r = G.group_count_rows(n)
        assert len(r) == n and (n < 3 or len(set(r)) < n)


def test_census_copy(geometry):
    R, CIN, COUT = geometry['CPS_ROWS'], geometry['CPS_IN'], geometry['CPS_OUT']
    assert set(G.COPY_DENSE) == {COUT - 16, COUT, COUT + 16} and set(G.COPY_RAW) == {CIN - 16, CIN, CIN + 16}
    assert set(G.COPY_KEPT_COUNTS) == {1, R - 1, R, R + 1, 2 * R, 2 * R + 1}
    tasks = G.copy_tasks(G.copy_run())
    assert all(t['rows'] == R for t in tasks[:-1]) and 0 < tasks[-1]['rows'] < R
    for want in G.COPY_DENSE:
        hit = [t for t in tasks if t['dense'] == want]
        assert len(hit) == 2 and all(t['raw'] <= CIN for t in hit) and len({t['d0'] for t in hit}) == 2
    for want in G.COPY_RAW:
        hit = [t for t in tasks if t['raw'] == want]
        assert len(hit) == 1 and hit[0]['dense'] <= COUT
    # nothing else takes the fallback: the six aimed tasks are the edges
    assert sum(t['dense'] > COUT or t['raw'] > CIN for t in tasks) == 3
    assert {t['d0'] for t in tasks} == set(range(16))
    assert any(t['routes'] == {'slow'} and t['rows'] == R for t in tasks)
    assert any(t['min_len'] == 5 for t in tasks)
    assert all(t['routes'] >= set(G.FAST_ROUTES) for t in tasks if t['dense'] in G.COPY_DENSE)
    for n in G.COPY_KEPT_COUNTS:
        rows = G.copy_count_rows(n)
        e = G.expected(rows)
        assert e.counts[G.KEPT] == n and e.kept_bytes.startswith(b'.html') and (n < 4 or e.counts[G.DUPLICATE] > 2)


def test_census_raw():
    b = G.raw_rows()
    rows = b.rows
    assert rows[:3] == ['', '', ''] and G.oracle_codes(rows, False)[:3].tolist() == [1, 3, 3]
    cells = {(len(r), s % 16) for r, s in G.marked(b)}
    assert cells >= {(L, s) for L in range(25) for s in range(16)}
    assert {127, 128, 129} <= {len(r) for r in rows}
    e = G.expected(rows, normalize=False)
    assert e.counts[G.NO_HTML] == e.counts[G.FILTERED] == 0 and e.counts[G.KEPT] > 900 and e.counts[G.DUPLICATE] > 900
    N = G.same_key_name(128)
    assert rows.count(N) == 2 and all(rows.count(m) == 2 for m in G.near_misses(N))


def test_collide_rows_pass_the_cap(geometry):
    rows = G.collide_rows()
    e = G.expected(rows)
    assert e.counts == [0, 70000, 0, 5000]
    assert len(rows) - 16 > geometry['COLLIDE_CAP']                    # (the 4-bit hash: at most 16 rows hold a slot)
    assert len({G.route(G.enc(r)).route for r in rows}) == 2


def test_every_family_is_needed():
    """Each family's own census cell is hit by no other family (so deleting one fails its census test, and merging
    two would lose cells)."""
    fam = {f: [G.route(G.enc(r)) for r in G.family_rows(f)] for f in G.FAMILIES}
    assert not any(v.route in ('gap', 'ins_gap') for v in fam['align_cut'])
    assert not any(v.route == 'slow' for v in fam['align_cut'] + fam['cut_rule'])
    assert sum(v.filtered for f in G.FAMILIES if f != 'filter' for v in fam[f]) < sum(v.filtered for v in fam['filter'])
    assert max(len(v.norm) for v in fam['same_key'] if v.norm) >= 257
    assert all(G.family_rows(f) for f in G.FAMILIES)
