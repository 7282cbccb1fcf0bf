"""CPU: the windowed CSV append's rule (tests/csv_window_rule.py) against ``resume_rule.parse`` over the whole text.

Every text the GPU tests stream is shown here, without a GPU, to be taken or refused for the reason intended: for a
clean text the cells are the whole-text parse's at every window size, for a text with one violation the verdict and
the file position are, and every window's ``consumed`` lies after a line end outside quotes.
"""
import pytest

from tests import csv_window_rule as W
from tests import resume_rule as R

KINDS = ['success', 'failed', 'links']
SIZES = [1, 7, 16, 33, 100, 257, 1000, 4096, 4096 + 16, 3 * 4096 - 1, 1 << 20]


def _check(text, kind, sizes):
    header, col = R.FILES[kind]
    want = R.parse(text, header, col)
    for size in sizes:
        verdict, pos, cells, consumed = W.stream(text, header, col, size)
        assert (verdict, pos, cells) == want, (kind, size, R.NAMES[want[0]])
        at = 0
        for used in consumed:
            at += used
            assert used == 0 or at == len(text) or text[at - 1:at] == b'\n'
        if verdict == R.OK:
            assert at == len(text)
    return want


@pytest.mark.parametrize('kind', KINDS)
def test_clean_texts_any_window(kind):
    for seed in range(40):
        assert _check(R.fuzz_clean(seed, kind), kind, SIZES)[0] == R.OK


@pytest.mark.parametrize('kind', KINDS)
def test_every_violation_any_window(kind):
    seen = set()
    for seed in range(8 * len(R.VIOLATIONS)):
        what, text = R.fuzz_dirty(seed, kind)
        verdict = _check(text, kind, SIZES + list(range(40, 72)))[0]
        assert verdict == R.EXPECT[what], (what, seed)
        seen.add(what)
    assert seen == set(R.VIOLATIONS)


@pytest.mark.parametrize('place', sorted(W.EDGE_PLACES))
def test_edge_text_cut_sweep(place):
    text, at = W.edge_text(W.EDGE_PLACES[place])
    header, col = R.FILES['success']
    verdict, _, cells = R.parse(text, header, col)
    assert verdict == R.OK and 35 <= len(cells) <= 50
    k = cells.index(W.REGION_CELLS[0])
    assert cells[k:k + 4] == W.REGION_CELLS
    sizes = W.sweep_windows(at)
    assert len(sizes) == 96 and sizes[0] == at + 1 and sizes[-1] > at + len(W.REGION)
    _check(text, 'success', sizes)
    # the cuts fall inside the quoted cell's line breaks, the "" pair, the UTF-8 characters and between '\r' and '\n'
    firsts = {W.stream(text, header, col, size)[3][0] for size in sizes}
    assert len(firsts) >= 5


def test_edge_places_cross_the_edges():
    assert W.EDGE_PLACES['tile'] < 4096 < W.EDGE_PLACES['tile'] + len(W.REGION)
    assert W.EDGE_PLACES['lane'] % 16 == 8


def test_record_refusal_and_header_cut():
    header, col = R.FILES['failed']
    long = b'url,error\r\nhttp://a/1,"' + b'x\n' * 450 + b'"\r\nhttp://a/2,e\r\n'
    assert R.parse(long, header, col)[0] == R.OK
    verdict, _, cells, consumed = W.stream(long, header, col, 256)
    assert verdict == R.OK and cells == [b'http://a/1', b'http://a/2'] and consumed[:3] == [11, 0, 0] and consumed[3] > 900
    assert W.stream(long, header, col, 256, max_record_bytes=400)[0] == W.RECORD
    # a first window that ends inside the header line
    verdict, _, cells, consumed = W.stream(b'url,error\nhttp://a/1,e\n', header, col, 4)
    assert verdict == R.OK and cells == [b'http://a/1'] and consumed[:2] == [0, 0]
    # the header alone, blank lines, nothing
    assert W.stream(b'url,error\n\n\n', header, col, 5)[:2] == (R.ROWS, 12)
    assert W.stream(b'', header, col, 5)[:2] == (R.HEADER, 0)


@pytest.mark.parametrize('what', R.VIOLATIONS)
def test_violation_texts_of_the_gpu_test(what):
    header, col = R.FILES['failed']
    texts = W.violation_texts(what, 4096)
    assert set(texts) == ({'first'} if what in ('header', 'norows') else {'first', 'middle', 'last'})
    for place, text in texts.items():
        want = R.parse(text, header, col)
        assert want[0] == R.EXPECT[what], (what, place)
        for size in (4096, 4096 + 16, 1000):
            assert W.stream(text, header, col, size)[:3] == want, (what, place, size)
