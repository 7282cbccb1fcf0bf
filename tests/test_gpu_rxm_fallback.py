"""Regex names whose program shares no literal window with an anchor: the fallback window (an RXM use at the
program's rarest window of four literals, priced by the background sample) against the CPU oracle.

The raw names' anchors hold the '.', so no literal window of their programs keys an anchor: without the
fallback every decided field of such a name is searched (``regex_searches``), with it none is.  Every matcher
here is built with a background sample made in the test (1 MiB: outside the name's own occurrences a window may
occur 4 times, the ceiling being 16 per 4 MiB, and 4 times per occurrence of the name); ``KW_RXM_FALLBACK_MAX=0``
(with ``KW_DEV=1``, read when the matcher is compiled) gives the matcher without fallback windows that proves the
construction.
"""
import pytest

from tests.test_gpu_parity import _compare, _gpu_maps

pytestmark = pytest.mark.gpu

# the names of the fallback; 'Vexo.Grid (VXG)': the group's parentheses are no part of the program, so the raw
# name never matches it (decided, no position: `name: []`)
_NAMES = ['D.R. Horton', 'Jon A. Olson', 'Hotels.com', 'x.yz.free', 'abcd.abcd.abcd', 'pq.rstu', 'Vexo.Grid (VXG)']
_CEILING_NAME = 'K.L. Wexford'          # every literal window of its program is frequent in the sample
_ABSENT_NAME = 'M.N. Quibble'          # the sample holds its word twice and the name never
_OTHER = ['Globex Corporation', 'IBM']  # start with none of the literal windows above
_PROCESSED = {'TK': {'name': {n: (None, None) for n in _NAMES + [_CEILING_NAME, _ABSENT_NAME] + _OTHER}}}


def _sample() -> bytes:
    """Every name once (a window is priced against the name's own occurrences) and the names' literal runs once
    more (so every raw name's rarest window is one with the '.'), the ceiling name's word 2000 times, the absent
    name's word twice, digits up to 1 MiB."""
    head = ' , '.join(_NAMES + [_CEILING_NAME]) + ' Horton Jon Olson Hotels com free abcd rstu Vexo Grid VXG '
    head += 'Quibble Quibble '
    head += 'Wexford ' * 2000
    fill = '0123456789 '
    s = head + fill * (((1 << 20) - len(head)) // len(fill))
    return s.encode()


def _matcher(monkeypatch, fallback=True, sample=True):
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.kb import compile_kb
    from advanced_scrapper_amd.matcher import GpuMatcher
    if not fallback:
        monkeypatch.setenv('KW_DEV', '1')
        monkeypatch.setenv('KW_RXM_FALLBACK_MAX', '0')
    m = GpuMatcher(compile_kb(_PROCESSED), background=_sample() if sample else None)
    if not fallback:
        monkeypatch.delenv('KW_RXM_FALLBACK_MAX')
        monkeypatch.delenv('KW_DEV')
    return m


def _ascii_docs():
    """ASCII fields that need no search with the fallback windows (each is a text and another's title)."""
    docs = [
        'D.R. Horton',                                              # byte 0 and the field's last byte
        'see Hotels.com',
        'x.yz.free and then pq.rstu',
        'Jon A. Olson met JonXA. Olson, Jon A- Olson and Jon A.Olson',
        'pq.rstupq.rstupqXrstu',                                    # adjacent
        'Hotels.comHotelsxcom Hotels.coHotels.com',
        'abcd.abcd.abcd abcdXabcdXabcdXabcdXabcdXabcd',             # overlapping: leftmost, non-overlapping
        'abcd.abcd.abcd.abcd.abcd',
        'D.R. Horton D\nR. Horton D.R\nHorton DxRy Horton',         # '\n' at a wildcard: no match
        'pq\nrstu pq.rstu',
        'x\nyz.free x.yz\nfree x.yz.free',
        'Vexo.Grid (VXG)',                                          # the raw name, the program unmatched
        'a Vexo.Grid (VXG) and VexoxGrid VXG',
        '.R. Horton is DxR. Horton',                                # decided by an edge window only
        'DxR. Horton, D.R. Horto',
        'on A. Olson or JonxAx Olson',
        'IBM and Globex Corporation, D.R. Horton, Hotels.com, x.yz.free',
        'Hort Hote free abcd rstu Jon  Vexo',                       # the windows alone
        '',
    ]
    return docs, docs[3:] + docs[:3]


def test_fallback_windows_need_no_search(monkeypatch):
    """Positions in text and title equal the oracle and no field is searched; the same matcher without the
    fallback windows searches (so these names do have no shared window)."""
    texts, titles = _ascii_docs()
    m = _matcher(monkeypatch)
    got = _gpu_maps(m, texts, titles)
    searches = m.stats()['regex_searches']
    bad = _compare(_PROCESSED, texts, titles, got)
    assert not bad, f"GPU differs from the oracle on docs {bad[:20]}"
    off = _matcher(monkeypatch, fallback=False)
    got_off = _gpu_maps(off, texts, titles)
    searches_off = off.stats()['regex_searches']
    print(f"regex_searches: fallback {searches}, off {searches_off}")
    assert got_off == got
    assert searches_off > 0
    assert searches == 0
    # every listed name is reported somewhere with a position, and the unmatched program with none
    seen = {}
    for t, i in got:
        for f in (t, i):
            for n, v in f.items():
                seen.setdefault(n, []).extend(v)
    for n in _NAMES[:-1]:
        assert seen.get(n), n
    assert got[11][0] == {'Vexo.Grid (VXG)': []}


def test_more_than_64_items_of_one_name(monkeypatch):
    """70 matches of one name in a field, more RXM items than the regex tasks' item path takes (64), with the
    name decided exactly or by an edge window only: whichever path takes such a field (these documents hold more
    items than the batched epilogue takes), the positions equal the oracle's."""
    texts = ['pq.rstu ' * 70, 'x ' + 'Hotels.com' * 70, 'D.R. Horton', '.R. Horton ' + 'DxR. Horton ' * 70]
    titles = ['pqxrstu' * 70, 'pq.rstu', 'abcd.abcd.abcd ' * 70, 'Jon Ax Olson' * 70 + ' Jon A. Olso']
    m = _matcher(monkeypatch)
    got = _gpu_maps(m, texts, titles)
    print(f"regex_searches: {m.stats()['regex_searches']}")
    bad = _compare(_PROCESSED, texts, titles, got)
    assert not bad, f"GPU differs from the oracle on docs {bad[:20]}"
    assert len(got[0][0]['pq.rstu']) == 70 and len(got[2][1]['abcd.abcd.abcd']) == 70
    assert len(got[3][0]['D.R. Horton']) == 70 and len(got[3][1]['Jon A. Olson']) == 70


def test_non_ascii_fields_are_searched(monkeypatch):
    texts = ['é D.R. Horton', 'D.R. Horton DéR. Horton D中R. Horton', 'Hotels.com 中 Hotels中com Hotelsécom',
             'pq.rstu pqérstu é', 'x.yz.free x中yzéfree', 'abcd.abcd.abcdé abcd中abcdéabcd', 'Jon A. Olson Jon A中 Olson']
    titles = texts[2:] + texts[:2]
    m = _matcher(monkeypatch)
    got = _gpu_maps(m, texts, titles)
    searches = m.stats()['regex_searches']
    bad = _compare(_PROCESSED, texts, titles, got)
    assert not bad, f"GPU differs from the oracle on docs {bad[:20]}"
    assert searches > 0


def test_common_windows_keep_the_search(monkeypatch):
    """The ceiling: a name whose every literal window is frequent in the sample gets no fallback window."""
    texts = ['K.L. Wexford and KxLy Wexford', 'Wexford K.L. Wexford']
    titles = ['K.L. Wexford', 'K\nL. Wexford K.L. Wexford']
    m = _matcher(monkeypatch)
    got = _gpu_maps(m, texts, titles)
    searches = m.stats()['regex_searches']
    bad = _compare(_PROCESSED, texts, titles, got)
    assert not bad, f"GPU differs from the oracle on docs {bad[:20]}"
    assert searches > 0


def test_windows_commoner_than_the_name_keep_the_search(monkeypatch):
    """The price per occurrence of the name: windows below the ceiling, but the sample never holds the name."""
    texts = ['M.N. Quibble and MxNy Quibble', 'Quibble']
    titles = ['M\nN. Quibble M.N. Quibble', 'M.N. Quibble']
    m = _matcher(monkeypatch)
    got = _gpu_maps(m, texts, titles)
    searches = m.stats()['regex_searches']
    bad = _compare(_PROCESSED, texts, titles, got)
    assert not bad, f"GPU differs from the oracle on docs {bad[:20]}"
    assert searches > 0


def test_no_sample_no_fallback(monkeypatch):
    """A matcher built without a sample cannot price a window: it searches, as before."""
    texts, titles = _ascii_docs()
    m = _matcher(monkeypatch, sample=False)
    got = _gpu_maps(m, texts, titles)
    searches = m.stats()['regex_searches']
    bad = _compare(_PROCESSED, texts, titles, got)
    assert not bad, f"GPU differs from the oracle on docs {bad[:20]}"
    assert searches > 0
