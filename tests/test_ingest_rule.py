"""CPU: the device ingest's take rule (tests/ingest_rule.py, which the GPU tests pin kw_ingest_parse against) holds
against the host tokenizer: whenever the rule takes a text, the model of the device output -- kept bytes, offsets,
flags, n_rows, consumed -- is kwcsv_parse's (csrc/kwcsv.c) for the same records."""
import re
import subprocess

import pytest

from tests import ingest_rule as R


def _same_as_host(text, ncols, final, max_rows, got):
    v, _pos, n_rows, consumed, cells = got
    assert v == R.OK
    # the host tokenizer on the bytes the device took (a window that is not final ends at `consumed`)
    rows, pos, out, off, fl, _ = R.host_parse(text if final else text[:consumed], ncols, max_rows)
    assert (rows, pos) == (n_rows, consumed), (rows, pos, n_rows, consumed, text)
    assert (out, off, fl) == (cells[0], cells[1], cells[2]), text


def test_fuzz_taken_texts_equal_the_host_tokenizer():
    na = R.na_set()
    taken, verdicts = 0, set()
    for seed in range(400):
        text, ncols = R.fuzz_text(seed)
        assert len(text) <= 2048
        for final, max_rows in ((True, 1 << 20), (False, 1 << 20), (True, 2), (False, 3)):
            got = R.parse(text, ncols, final, max_rows, na)
            verdicts.add(got[0])
            if got[0] == R.OK:
                taken += 1
                _same_as_host(text, ncols, final, max_rows, got)
            else:
                assert got[2:] == (0, 0, None) and 0 <= got[1] <= len(text)
    assert taken >= 400 and verdicts >= {R.OK, R.NUL, R.UTF8, R.QUOTE, R.CR, R.BLANK, R.FIELDS}


def test_clean_texts_are_always_taken():
    """The cap on fallback: csv.writer output (QUOTE_MINIMAL, 6-9 columns, either terminator) is taken, every time."""
    na = R.na_set()
    for seed in range(300):
        text, ncols = R.clean_text(seed)
        for final in (True, False):
            got = R.parse(text, ncols, final, 1 << 20, na)
            assert got[0] == R.OK, (seed, R.NAMES[got[0]], got[1], text[:200])
            _same_as_host(text, ncols, final, 1 << 20, got)
        n = R.parse(text, ncols, True, 1 << 20, na)[2]
        assert n >= 1
        # a window that is not final holds the records whose terminator it holds
        assert R.parse(text, ncols, False, 1 << 20, na)[2] == n - (0 if text.endswith(b'\n') else 1)


BASE = b'a,b,c,d,e,f\n1,"x,y",3,4,5,6\r\nu,v,w,x,y,"z""q"\n'


def test_injected_violations_verdict_and_position():
    p = lambda text, final=True, max_rows=1 << 20: R.parse(text, 6, final, max_rows)[:4]   # noqa: E731
    n = len(BASE)
    assert p(BASE) == (R.OK, 0, 3, n)
    assert p(BASE[:-1]) == (R.OK, 0, 3, n - 1)                    # the text's end ends the last record
    assert p(BASE[:-1], final=False) == (R.OK, 0, 2, 29)          # ... unless more may follow
    assert p(BASE[:12] + b'\0' + BASE[12:]) == (R.NUL, 12, 0, 0)
    assert p(BASE[:12] + b'\xe2\x82' + BASE[12:]) == (R.UTF8, 12, 0, 0)
    assert p(b'a\xff,"\0\n') == (R.NUL, 4, 0, 0)                  # NUL ahead of UTF-8, whatever their order
    assert p(BASE[:13] + b'"' + BASE[13:]) == (R.QUOTE, 13, 0, 0)   # a '"' mid-field
    assert p(BASE[:19] + b'z' + BASE[19:]) == (R.QUOTE, 18, 0, 0)   # bytes after a closing quote
    assert p(b'x\r,e\n' + BASE[:13] + b'"' + BASE[13:]) == (R.QUOTE, 18, 0, 0)   # QUOTE ahead of CR
    assert p(BASE[:13] + b'\r' + BASE[13:]) == (R.CR, 13, 0, 0)     # a lone '\r'
    assert p(BASE[:12] + b' \t \n' + BASE[12:]) == (R.BLANK, 12, 0, 0)   # a blanks-only line
    assert p(BASE[:12] + b' \t \r\n' + BASE[12:]) == (R.BLANK, 12, 0, 0)
    assert p(BASE + b'  ') == (R.BLANK, n, 0, 0)
    assert p(BASE[:12] + b'1,2,3,4,5\n' + BASE[12:]) == (R.FIELDS, 21, 0, 0)       # a short record: its '\n'
    assert p(BASE[:12] + b'1,2,3,4,5,6,7\n' + BASE[12:]) == (R.FIELDS, 25, 0, 0)   # a long record
    assert p(BASE + b'1,2,3') == (R.FIELDS, n + 5, 0, 0)                           # the final record: the text's length
    assert p(BASE[:12] + b' \n' + BASE[12:20] + b'\n' + BASE[20:]) == (R.BLANK, 12, 0, 0)   # BLANK ahead of FIELDS
    assert p(BASE + b'1,2,3,4,5,"6') == (R.QUOTE, n + 12, 0, 0)    # an unterminated quote in a final text
    assert p(BASE + b'1,2,3,4,5,"6', final=False) == (R.OK, 0, 3, n)   # ... is an incomplete record in a window
    # an offender after the taken records is not this parse's business
    assert p(BASE + b'x"y\0\n', max_rows=3) == (R.OK, 0, 3, n)
    assert p(BASE + b'x"y\0\n', max_rows=4)[0] == R.NUL
    # zero-length records are skipped, "\r\n" included; a window that is not final may end in '\r' or a quote
    assert p(b'\n\r\n' + BASE[:12] + b'\n\r\n\n' + BASE[12:]) == (R.OK, 0, 3, n + 7)
    assert p(BASE + b'1,2,3,4,5,6\r', final=False) == (R.OK, 0, 3, n)
    assert p(BASE + b'1,2,3,4,5,"6"', final=False) == (R.OK, 0, 3, n)
    assert p(BASE + b'1,2,3,4,5,6\r') == (R.CR, n + 11, 0, 0)
    assert p(b'', final=False) == (R.OK, 0, 0, 0) and p(b'') == (R.OK, 0, 0, 0)
    assert p(b'a,b,c', final=False) == (R.OK, 0, 0, 0)


def test_sweep_shifts_put_every_construct_across_every_edge():
    """The GPU byte-geometry sweep's shifts (tests/test_gpu_ingest.py), checked where no GPU is needed: a "" pair, a
    "\\r\\n", a closing quote + ',' and a 2-, 3- and 4-byte code point each lie across a lane, a wave and a tile edge."""
    from advanced_scrapper_amd import _native
    from tests import test_gpu_ingest as G
    T = _native.lib().kw_ingest_tile_bytes()
    seen = set()
    for k in G.sweep_shifts(T):
        seen |= G._straddled(G._sweep_text(k), T)
    assert seen == {(c, e) for c in G.CONSTRUCTS for e in ('lane', 'wave', 'tile')}


def test_header_only_file_touches_no_device(tmp_path):
    """A file that holds its header alone yields nothing on the device route, and creates no device handle."""
    from advanced_scrapper_amd import ingest
    path = tmp_path / 'articles.csv'
    for tail in (b'', b'\n', b'\r\n'):
        path.write_bytes(b'article_text,title,date_time,url,source,source_url' + tail)
        assert list(ingest.read_chunks_device(str(path), 10, 0)) == list(ingest.read_chunks(str(path), 10)) == []


def test_library_exports_the_ingest_symbols():
    from advanced_scrapper_amd import _native
    want = ['kw_ingest_create', 'kw_ingest_destroy', 'kw_ingest_last_error', 'kw_ingest_last_ms', 'kw_ingest_tile_bytes',
            'kw_ingest_parse', 'kw_ingest_cells', 'kw_ingest_arena', 'kw_ingest_dates', 'kw_ingest_column_flags',
            'kw_ingest_copy_cells', 'kw_ingest_copy_column', 'kw_rows_cells_device']
    L = _native.lib()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True).stdout
    for f in want:
        assert f in _native.EXPORTS and hasattr(L, f), f
        assert re.search(rf'\bT {f}\b', out), f
    assert L.kw_ingest_tile_bytes() > 0 and L.kw_ingest_tile_bytes() % 16 == 0
