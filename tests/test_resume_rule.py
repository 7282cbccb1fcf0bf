"""CPU: the resume filter's CSV rule (tests/resume_rule.py, which the GPU tests pin kw_csv_append against) holds
against pandas: whenever the rule takes a text, its cells are ``pd.read_csv(text)[column].astype(str).tolist()``."""
import pytest

from tests import resume_rule as R

KINDS = ['success', 'failed', 'links']


@pytest.mark.parametrize('kind', KINDS)
def test_every_clean_text_is_taken_and_equals_pandas(kind):
    header, col = R.FILES[kind]
    for seed in range(150):
        text = R.fuzz_clean(seed, kind)
        v, pos, cells = R.parse(text, header, col)
        assert (v, pos) == (R.OK, -1), (seed, R.NAMES[v], pos, text[:300])
        assert [c.decode('utf-8') for c in cells] == R.pandas_urls(text, header, col), (seed, text[:300])


@pytest.mark.parametrize('kind', KINDS)
def test_dirty_texts(kind):
    header, col = R.FILES[kind]
    seen, taken = set(), 0
    for seed in range(390):
        what, text = R.fuzz_dirty(seed, kind)
        v, pos, cells = R.parse(text, header, col)
        assert v == R.EXPECT[what], (seed, what, R.NAMES[v], pos, text[:300])
        if v == R.OK:
            taken += 1
            assert [c.decode('utf-8') for c in cells] == R.pandas_urls(text, header, col), (seed, text[:300])
        else:
            assert cells is None and 0 <= pos <= len(text)
            seen.add(R.CONDITION[v])
    assert seen == {1, 2, 3, 4, 5, 6, 7} and taken >= 20


def test_verdict_order_and_positions():
    h, col = R.FILES['failed']
    p = lambda body: R.parse(h + b'\n' + body, h, col)[:2]   # noqa: E731
    o = len(h) + 1
    assert p(b'http://a,e\n') == (R.OK, -1)
    assert p(b'http://a,e') == (R.OK, -1)
    assert p(b'a\xff,"\0\n') == (R.NUL, o + 4)                      # NUL ahead of UTF-8, whatever their order
    assert p(b'a\xe2\x82,x"\n') == (R.UTF8, o + 1)
    assert R.parse(b'url,error \nhttp://a,"\n', h, col)[:2] == (R.HEADER, 0)
    assert p(b'x\r,e\nhttp://a,b"c\n') == (R.QUOTE, o + 15)          # QUOTE ahead of CR
    assert p(b'http://a,"e\n') == (R.QUOTE, o + 12)                  # ends inside quotes: the text's length
    assert p(b'http://a,"e"x\n') == (R.QUOTE, o + 11)                # the closing quote
    assert p(b'nocolon,e\nx\r,e\n') == (R.CR, o + 11)                # CR ahead of the records' conditions
    assert p(b'nocolon,e\nhttp://a\n') == (R.FIELDS, o + 10)         # FIELDS ahead of URL, whatever their order
    assert p(b'http://a,e\nnocolon,e\n"b:,c",e\n') == (R.URL, o + 11)
    assert p(b'') == (R.ROWS, o) and p(b'\n\r\n\n') == (R.ROWS, o + 4)
    # cells: quotes removed, "\r\n" and blank lines dropped, quoted line breaks in other cells
    v, _, cells = R.parse(h + b'\r\n"http://a,b","x\r\ny""z"\r\n\r\n\nc:d,\n', h, col)
    assert v == R.OK and cells == [b'http://a,b', b'c:d']
