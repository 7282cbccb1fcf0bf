"""GPU tests of the edge prefilter the filter kernel computes (DH_EDGE0 / DH_EDGE1 in the documents' flags) and of
the group epilogue's short-field signature pretest (fields of SHORT_EXACT_MAX + 1 .. 64 code points with at most
64 fuzzy names at least as long): every document's hits against the CPU oracle (tests/oracle_matcher.py)."""
import pytest

pytestmark = pytest.mark.gpu

EDGE_MIN_M = 11          # kwmatch_fast.hpp: names of EDGE_MIN_M..EDGE_MAX_M code points have edge-only windows
SHORT_EXACT_MAX = 10     # kwmatch_device.hpp: fields this short only match exactly
FILL = 'zq vj xk wq zj qx vk jz'    # no name shares a 4-gram with it

# fuzzy names (mixed case) of 11..20 code points, one with non-ASCII code points; an all-uppercase name for the
# documents with many items
EDGE_NAMES = ['Acme Widget', 'Borealis Ltd', 'Cobalt Works', 'Dunmore Hldgs', 'Everest Partner', 'Fjord Shipping Co',
              'Granite Peak Mining', 'Harbor Light Brewing', 'Société Générale']
assert sorted({len(n) for n in EDGE_NAMES}) == [11, 12, 13, 15, 16, 17, 19, 20]


def _processed(names):
    return {f'T{i}': {'aliases': {n: (None, None)}} for i, n in enumerate(names)}


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _check(m, o, texts, titles):
    """The GPU's hits of every document equal the oracle's; returns the oracle's grouped hits."""
    from advanced_scrapper_amd.matcher import group_hits
    got = group_hits(m.match_strings(texts, titles))
    want = group_hits(o.match_strings(texts, titles))
    bad = [d for d in range(len(texts)) if got.get(d) != want.get(d)]
    for d in bad[:4]:
        print(f'doc {d} text {texts[d][:60]!r} title {titles[d][:60]!r}: got {got.get(d)} want {want.get(d)}')
    assert not bad, f'GPU differs from the oracle on docs {bad[:20]}'
    return want


def _windows(name):
    """The name with one code point deleted: the first, a middle one, the last."""
    return [name[1:], name[:len(name) // 2] + name[len(name) // 2 + 1:], name[:-1]]


def _edge_docs():
    texts, titles = [], []

    def add(text, title):
        texts.append(text)
        titles.append(title)

    # every name, every deletion, at the four field edges (the documents fall on lanes 0, 31 and 32 of their
    # groups among the others: 9 names x 3 windows x 4 places = 108 documents, then the special ones)
    for n in EDGE_NAMES:
        for w in _windows(n):
            add(f'{w} {FILL} {FILL}', f'{FILL}')
            add(f'{FILL} {FILL} {w}', f'{FILL}')
            add(f'{FILL}', f'{w} {FILL}')
            add(f'{FILL}', f'{FILL} {w}')
    # fields of exactly EDGE_MIN_M bytes (no prefilter test: the short-field path) and EDGE_MIN_M + 1 bytes
    w11, w12 = 'Borealis Ltd'[1:], 'Dunmore Hldgs'[:-1]
    assert len(w11) == EDGE_MIN_M and len(w12) == EDGE_MIN_M + 1
    for w in (w11, w12, 'Acme Widget'[1:] + 'z', 'z' + 'Acme Widget'[:-1]):
        add(w, FILL)
        add(FILL, w)
        add(w, w)
    # empty text / empty title / both
    add('', f'Cobalt Work {FILL}')
    add(f'{FILL} obalt Works', '')
    add('', '')
    # a non-ASCII field with an edge window (a transcoded document), the non-ASCII bytes in and off the window
    add(f'verest Partner {FILL} é {FILL}', f'{FILL} ü Fjord Shipping C')
    add(f'ociété Générale {FILL}', f'{FILL} Société Général')
    add(f'é {FILL} Granite Peak Minin', f'ranite Peak Mining 中 {FILL}')
    # more than 64 items in a field (the per-document epilogue paths read the flag too), ASCII and non-ASCII
    many = ' '.join(['IBM'] * 70)
    add(f'cme Widget {many} Harbor Light Brewin', f'orealis Ltd {FILL}')
    add(f'cme Widget {many} é Harbor Light Brewin', f'{FILL} Borealis Lt')
    # the arena's last document: its title's last eight bytes are the arena's
    add(f'{FILL}', f'{FILL} Everest Partne')
    return texts, titles


@pytest.fixture(scope='module')
def edge_kb():
    _gpu()
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    from tests.oracle_matcher import OracleMatcher
    processed = _processed(EDGE_NAMES + ['IBM'])
    m = GpuMatcher(compile_kb(processed))
    yield m, OracleMatcher(processed)
    m.close()


def test_edge_windows_at_every_field_edge(edge_kb):
    m, o = edge_kb
    texts, titles = _edge_docs()
    assert len(texts) > 2 * 32 + 31       # lanes 0, 31 and 32 of full groups and a last group of fewer than 32
    want = _check(m, o, texts, titles)
    assert m.stats()['edge_items'] > 0
    # the cases are not vacuous: each of the 108 window documents is a hit of its name at its place
    for d in range(108):
        assert want.get(d), (d, texts[d], titles[d])
    assert want.get(len(texts) - 1, {}).get(1), 'the last title ends with a window'


def test_every_lane_flags_its_document(edge_kb):
    """70 documents that all hit, text and title alternating: two full groups and one of six documents."""
    m, o = edge_kb
    texts, titles = [], []
    for d in range(70):
        n = EDGE_NAMES[d % 8]
        w = _windows(n)[d % 3]
        texts.append(f'{w} {FILL}' if d % 2 else f'{FILL} {FILL}')
        titles.append(f'{FILL}' if d % 2 else f'{FILL} {w}')
    want = _check(m, o, texts, titles)
    assert all(want.get(d) for d in range(70))


@pytest.mark.parametrize('field', [0, 1])
def test_corpus_of_one_document(edge_kb, field):
    m, o = edge_kb
    w = f'{FILL} Granite Peak Minin'
    want = _check(m, o, [w if field == 0 else FILL], [w if field == 1 else FILL])
    assert want.get(0, {}).get(field)


def _long_names(k, lo, hi):
    """k distinct fuzzy names of lo..hi code points, made of words that differ in every name."""
    out = []
    for i in range(k):
        ln = lo + (i * 7) % (hi - lo + 1)
        words = []
        j = 0
        while len(' '.join(words)) < ln:
            a, b = (i * 5 + j * 3) % 26, (i * 11 + j * 7 + 1) % 26
            words.append(chr(65 + a) + chr(97 + b) * 2 + chr(97 + (a + b) % 26) + chr(97 + (i + j) % 26))
            j += 1
        out.append(' '.join(words)[:ln].rstrip() + 'x' * (ln - len(' '.join(words)[:ln].rstrip())))
    assert len(set(out)) == k and all(lo <= len(n) <= hi for n in out)
    return out


def _short_titles(names, n_docs=300):
    """Titles of SHORT_EXACT_MAX + 1 .. 64 code points: a long name cut to the title's length with zero, one or
    a few edits, and titles unlike any name."""
    texts, titles = [], []
    for d in range(n_docs):
        n = names[d % len(names)]
        ln = SHORT_EXACT_MAX + 1 + (d * 13) % (64 - SHORT_EXACT_MAX)
        s = d % len(n)
        t = (n[s:] + n[:s])[:ln] if d % 5 == 4 else n[:ln]
        kind = d % 4
        if kind == 1 and len(t) > 4:                       # one substitution
            t = t[:3] + '#' + t[4:]
        elif kind == 2 and len(t) > 12:                    # edits spread over the title
            t = t[:2] + t[3:9] + '%%' + t[9:]
        elif kind == 3:                                    # unlike any name
            t = (FILL + ' ' + FILL + ' ' + FILL)[:max(len(t), SHORT_EXACT_MAX + 1)]
        t = (t + ' ' + FILL + ' ' + FILL + ' ' + FILL)[:ln]      # (a name shorter than the title: the name, then filler)
        if t.endswith(' '):
            t = t[:-1] + 'q'
        texts.append(f'{FILL} {d}')
        titles.append(t)
    assert min(len(t) for t in titles) == SHORT_EXACT_MAX + 1 and max(len(t) for t in titles) == 64
    return texts, titles


@pytest.mark.parametrize('n_names, lo', [(20, 11), (80, 40)])
def test_short_titles_signature_pretest(n_names, lo):
    """(20, 11): fewer than 64 fuzzy names, every title takes the pretest; (80, 40): more than 64 names at least
    as long as the titles of up to 40 code points (no pretest for them), at most 64 above."""
    _gpu()
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    from tests.oracle_matcher import OracleMatcher
    names = _long_names(n_names, lo, 64)
    processed = _processed(names)
    texts, titles = _short_titles(names)
    m = GpuMatcher(compile_kb(processed))
    try:
        want = _check(m, OracleMatcher(processed), texts, titles)
    finally:
        m.close()
    hit = sum(1 for d in range(len(texts)) if want.get(d, {}).get(1))
    assert 20 <= hit <= len(texts) - 20, hit          # titles that match a name and titles that match none
