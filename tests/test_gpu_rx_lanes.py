"""The regex task kernel's three routes against the CPU oracle: a decided regex-class name with an RXM use in an
ASCII field is a task one lane decides (it walks the field's items: no match of the name's program, or one), a
task the whole wave takes in the same round (two or more items of the name, or a field of more than
RX_LANE_ITEMS items: sort and leftmost non-overlapping selection), or a field search (a non-ASCII field, more
than 64 items of the name).

The names, the background sample and the matcher are those of tests/test_gpu_rxm_fallback.py: raw names with a
'.', whose programs get an RXM use at a fallback window priced by a 1 MiB sample, so an ASCII field of theirs needs
no search.  A name that occurs literally in a longer field is decided, positions and all, by the scan's epilogue;
the regex tasks are the names decided otherwise: a field no longer than the name (the short kernel decides it),
or an edge window ('.R. Horton' decides 'D.R. Horton') with the program's matches elsewhere ('DxR. Horton').
"""
import numpy as np
import pytest

from advanced_scrapper_amd import _native

from tests.test_gpu_parity import _compare, _gpu_maps

pytestmark = pytest.mark.gpu

RX_LANE_ITEMS = 64   # csrc/kwmatch_fast_kernel.hpp

_NAMES = ['D.R. Horton', 'Jon A. Olson', 'Hotels.com', 'x.yz.free', 'abcd.abcd.abcd', 'pq.rstu', 'Vexo.Grid (VXG)']
_OTHER = ['Globex Corporation', 'IBM']
_PROCESSED = {'TK': {'name': {n: (None, None) for n in _NAMES + _OTHER}}}


def _sample() -> bytes:
    """Every name once and the names' literal runs once more (so every raw name's rarest window is one with the
    '.'), digits up to 1 MiB."""
    head = ' , '.join(_NAMES) + ' Horton Jon Olson Hotels com free abcd rstu Vexo Grid VXG '
    fill = '0123456789 '
    s = head + fill * (((1 << 20) - len(head)) // len(fill))
    return s.encode()


@pytest.fixture(scope='module')
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    return GpuMatcher(compile_kb(_PROCESSED), background=_sample())


def _run(m, texts, titles):
    """(maps, statistics, task counts) of one scan, the maps checked against the oracle."""
    got = _gpu_maps(m, texts, titles)
    st, tc = m.stats(), m.task_counts()
    bad = _compare(_PROCESSED, texts, titles, got)
    assert not bad, f"GPU differs from the oracle on docs {bad[:20]}"
    return got, st, tc


# ------------------------------------------------------------------ case 1: every k and every route
_K0 = 'Vexo.Grid (VXG)'                       # decided, the program unmatched: `name: []`
_K1 = ['D.R. Horton', 'see Hotels.com', 'x.yz.free and then pq.rstu', 'pq.rstu', 'Hotels.com']
_K2 = 'pq.rstupq.rstu'                        # two matches, adjacent
_KOV = 'abcd.abcd.abcd.abcd.abcd'             # three items, overlapping: the leftmost, then none
_K64 = 'pq.rstu ' * 64
_K65 = 'pq.rstu ' * 65                        # more items of one name than the item path takes: searched
# the same counts for names an edge window decides
_EDGE = ['.R. Horton',                                                  # no match of the program
         '.R. Horton is DxR. Horton',                                   # one
         '.R. Horton DxR. Horton DyR. Horton on A. Olson',              # two, and none of another name
         'on A. Olson Jon Ax OlsonJon Ay Olson',                        # two, adjacent
         'bcd.abcd.abcd abcdXabcdXabcdXabcdXabcd',                      # four, overlapping
         'exo.Grid (VXG) and VexoxGrid VXG, Vexo\nGrid VXG']                 # one ('\n' at the wildcard: none)
_EDGE64 = '.R. Horton ' + 'DxR. Horton ' * 64
_EDGE65 = '.R. Horton ' + 'DxR. Horton ' * 65
_ASCII_FIELDS = [_K0] + _K1 + [_K2, _KOV, _K64] + _EDGE


def _pairs(fields):
    """Each field as a text beside another of the list as its title."""
    return list(fields), list(fields[1:]) + list(fields[:1])


def test_every_count_and_route_equals_the_oracle(m):
    fields = _ASCII_FIELDS + [_K65, _EDGE64, _EDGE65]
    na = ['é ' + f for f in fields]
    t0, i0 = _pairs(fields)
    t1, i1 = _pairs(na)
    # one field ASCII and the other not, both ways
    texts, titles = t0 + t1 + fields + na, i0 + i1 + na + fields
    got, st, tc = _run(m, texts, titles)
    print(f"regex_searches {st['regex_searches']}, tasks {tc}")
    assert tc['regex'] > 0
    at = {f: got[d][0] for d, f in enumerate(fields)}
    assert at[_K0] == {_K0: []} and at['.R. Horton'] == {'D.R. Horton': []}
    assert at[_K2] == {'pq.rstu': [0, 7]} and at[_KOV] == {'abcd.abcd.abcd': [0]}
    assert at[_EDGE[1]] == {'D.R. Horton': [14]}
    assert at[_EDGE[2]] == {'D.R. Horton': [11, 23], 'Jon A. Olson': []}
    assert at[_EDGE[3]] == {'Jon A. Olson': [12, 24]}
    assert at[_EDGE[4]] == {'abcd.abcd.abcd': [4, 19]}
    assert at[_EDGE[5]] == {'Vexo.Grid (VXG)': [19]}
    assert len(at[_K64]['pq.rstu']) == 64 and len(at[_K65]['pq.rstu']) == 65
    assert len(at[_EDGE64]['D.R. Horton']) == 64 and len(at[_EDGE65]['D.R. Horton']) == 65
    assert got[len(fields) + fields.index(_K2)][0] == {'pq.rstu': [2, 9]}


def test_ascii_fields_up_to_64_items_of_a_name_need_no_search(m):
    texts, titles = _pairs(_ASCII_FIELDS)
    _, st, tc = _run(m, texts, titles)
    print(f"tasks {tc}")
    assert tc['regex'] >= 2 * (len(_EDGE) + 1)   # at least the edge-decided names, in the texts and the titles
    assert st['regex_searches'] == 0


def test_65_items_of_a_name_and_non_ascii_fields_are_searched(m):
    na = ['é ' + f for f in _ASCII_FIELDS]
    _, s65, _ = _run(m, [_K65, 'D.R. Horton', _EDGE65], ['pq.rstu', _K65, _EDGE65])
    _, sna, _ = _run(m, na, [''] * len(na))
    _, sall, _ = _run(m, [_K65, _EDGE65] + na, [_EDGE65, _K65] + [''] * len(na))
    # an ASCII field beside a non-ASCII one adds no search
    _, smix, _ = _run(m, na, list(_ASCII_FIELDS))
    print(f"regex_searches: 65 items {s65['regex_searches']}, non-ASCII {sna['regex_searches']}, both "
          f"{sall['regex_searches']}, non-ASCII with ASCII titles {smix['regex_searches']}")
    assert sall['regex_searches'] > 0 and sna['regex_searches'] > 0
    assert smix['regex_searches'] == sna['regex_searches']


# ------------------------------------------------------------------ case 2: the item-walk bound
_PAD = 'IBM '


def _bound_field(kind, reps, where):
    pad = _PAD * reps
    if kind == 'literal':   # the name itself: the epilogue's own positions
        return {'first': 'pq.rstu ' + pad, 'last': pad + 'pq.rstu', 'absent': pad + 'pq.rst'}[where]
    # an edge window decides the name: a regex task, its answer the field's RXM items
    return '.R. Horton ' + {'first': 'DxR. Horton ' + pad, 'last': pad + 'DxR. Horton', 'absent': pad}[where]


def _items(m, field):
    m.match_strings([field], [''])
    return int(m.doc_items(1)[0, 0])


@pytest.mark.parametrize('where', ['first', 'last', 'absent'])
@pytest.mark.parametrize('kind', ['literal', 'edge'])
def test_item_walk_bound(m, kind, where):
    """Fields of RX_LANE_ITEMS - 1, RX_LANE_ITEMS, RX_LANE_ITEMS + 1 and 4 RX_LANE_ITEMS items (the counts read
    back from the scan; the padding sized from two measured fields), with one match of the name first, last or
    absent."""
    a, b = _items(m, _bound_field(kind, 8, where)), _items(m, _bound_field(kind, 16, where))
    assert b > a and (b - a) % 8 == 0, f"items of 8 / 16 pads: {a} / {b}"
    per = (b - a) // 8
    base = a - 8 * per
    print(f"{kind} {where}: {per} items per pad, {base} beside them")
    targets = [RX_LANE_ITEMS - 1, RX_LANE_ITEMS, RX_LANE_ITEMS + 1, 4 * RX_LANE_ITEMS]
    assert all((t - base) % per == 0 for t in targets), f"{targets} items: not reachable, {per} per pad over {base}"
    texts = [_bound_field(kind, (t - base) // per, where) for t in targets]
    got, st, tc = _run(m, texts, ['pq.rstu'] * len(texts))
    counts = m.doc_items(len(texts))[:, 0].tolist()
    print(f"{kind} {where}: items {counts}, regex_searches {st['regex_searches']}, tasks {tc}")
    assert counts == targets
    assert st['regex_searches'] == 0
    if kind == 'edge' and where != 'absent':
        assert tc['regex'] > len(texts)   # more than the titles': edge-decided names with their items
    name = 'pq.rstu' if kind == 'literal' else 'D.R. Horton'
    for d, t in enumerate(texts):
        hit = t.find('pq.rstu' if kind == 'literal' else 'DxR. Horton')
        want = None if kind == 'literal' and where == 'absent' else [hit] if hit >= 0 else []
        assert got[d][0].get(name) == want, (d, got[d][0])
        assert got[d][0].get('IBM') and got[d][1] == {'pq.rstu': [0]}


# ------------------------------------------------------------------ cases 3 and 4: whole prefetch rounds
def _sorted_records(hits):
    r = np.stack([hits['doc'], hits['field'], hits['pattern'], hits['pos']], axis=1).astype(np.int64)
    return r[np.lexsort((r[:, 3], r[:, 2], r[:, 1], r[:, 0]))]


def _periodic(m, docs, n):
    """n documents cycling through docs (n a multiple of their number), scanned at the defaults and checked
    against the oracle: the first period through the maps, the rest as the first period's records repeated."""
    period = len(docs)
    assert n % period == 0
    texts = [docs[d % period][0] for d in range(n)]
    titles = [docs[d % period][1] for d in range(n)]
    hits = m.match_strings(texts, titles)
    st, tc = m.stats(), m.task_counts()
    routes = m.doc_routes(n)
    rec = _sorted_records(hits)
    first = rec[rec[:, 0] < period]
    reps = n // period
    tiled = np.tile(first, (reps, 1))
    tiled[:, 0] += np.repeat(np.arange(reps, dtype=np.int64) * period, len(first))
    assert np.array_equal(tiled, rec), 'the records do not repeat with the documents'
    _, st1, _ = _run(m, texts[:period], titles[:period])
    assert st['regex_searches'] == reps * st1['regex_searches']
    return {'texts': texts, 'titles': titles, 'rec': rec, 'stats': st, 'tasks': tc, 'routes': routes}


# (an edge window decides a name at the field's first or last byte: two regex tasks an ASCII field)
_T_EDGE = '.R. Horton is here, VexoxGrid VXG and exo.Grid (VXG)'                       # no match, and one
_T_EDGE_K = '.R. Horton DxR. Horton DyR. Horton abcdXabcdXabcdXabcdXabcd Jon Ax Olson on A. Olson'   # two, and one
_T_EDGE_OV = 'bcd.abcd.abcd abcdXabcdXabcdXabcdXabcd exo.Grid (VXG)'                   # four overlapping, and none
_T_NA = 'é D.R. Horton Jon A. Olson Hotels.com x.yz.free abcd.abcd.abcd pq.rstu ' + _K0   # seven searches
_T_NA_K = 'é ' + _K2 + ' ' + _KOV + ' Hotels.com D.R. Horton x.yz.free Jon A. Olson ' + _K0
_ROUND_DOCS = [(_T_EDGE_K, _T_NA), (_T_NA_K, _T_EDGE), (_T_NA, _T_NA_K), (_T_NA_K, _T_NA),
               (_T_EDGE_OV, _T_NA_K), (_T_NA, _T_EDGE_K), (_T_NA_K, _T_NA_K), (_T_NA, _T_NA),
               (_T_EDGE, _T_NA), (_T_NA_K, _T_EDGE_OV), (_T_NA, _T_NA_K), (_T_NA_K, _T_NA),
               (_T_EDGE_K, _T_EDGE_OV)]


@pytest.fixture(scope='module')
def rounds(m):
    """48k documents of at most 120 bytes a field that cycle through _ROUND_DOCS: 9 regex tasks a document (an
    ASCII field's two edge-decided names, a non-ASCII field's seven names), 14 (both non-ASCII) or 4: 142 in 13
    documents, 131 in a region of 12."""
    assert all(len(t.encode()) <= 120 and len(i.encode()) <= 120 for t, i in _ROUND_DOCS)
    period = len(_ROUND_DOCS)
    return _periodic(m, _ROUND_DOCS, period * -(-48 * 1024 // period))


def test_regions_hold_more_than_one_round(rounds):
    """More regex tasks per region than one prefetch round of the early kernel's two waves a region takes (the
    mean over the regions, so the largest too), the largest region's last round partly filled."""
    tc = rounds['tasks']
    print(f"task counts: {tc}, regex_searches {rounds['stats']['regex_searches']}")
    assert tc['regex_early'] > 64 * 2 * tc['regions']
    assert tc['regex_early_max'] % (64 * 2) != 0
    assert rounds['stats']['regex_searches'] > 0


@pytest.mark.parametrize('env', [{'KW_RX_EARLY_G': 1}, {'KW_RX_EARLY_G': 4}, {'KW_RX_SPLIT': 0}, {'KW_RX_SPLIT': 1},
                                 {'KW_TASK_G': '1,4,4,1'}])
def test_rounds_at_every_wave_count(m, rounds, monkeypatch, env):
    """The same records and the same searches at 1 and 4 waves a region, with the regex tasks beside the verify /
    short kernels or after them."""
    monkeypatch.setenv('KW_DEV', '1')
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    hits = m.match_strings(rounds['texts'], rounds['titles'])
    st = m.stats()
    assert np.array_equal(_sorted_records(hits), rounds['rec'])
    assert st['regex_searches'] == rounds['stats']['regex_searches']


def test_lanes_queue_and_search_in_every_round(m):
    """Every document queues a task the wave takes (two matches of 'D.R. Horton'), one a lane decides (one of
    'Jon A. Olson', which an edge window at the field's end decides) and a field search (the other field, non-ASCII, on the transcoded view), the fields swapped in
    every other document: however a region orders its tasks, a prefetch round of 64 leaves lanes to each route.
    The ASCII fields add no search to the other fields' own."""
    asc, na = '.R. Horton DxR. Horton DyR. Horton Jon Ax Olson on A. Olson', 'é Hotels.com'
    n = 6000
    r = _periodic(m, [(asc, na), (na, asc)], n)
    print(f"regex_searches {r['stats']['regex_searches']}, task counts {r['tasks']}")
    assert (r['routes'] == _native.KW_ROUTE_TRANSCODE).all()
    assert r['tasks']['regex'] == 3 * n and r['tasks']['regex_max'] > 64
    assert r['stats']['regex_searches'] == n
