"""Pure-Python restatement of the resume filter's CSV rule and parse (csrc/cdx.hip kw_csv_append, include/kwdedup.h).

``parse(text, header, url_col)`` is what ``kw_csv_append`` computes: a verdict, the byte position of the first
offender, and (when OK) the cells of the column as bytes.  ``fuzz_clean`` / ``fuzz_dirty`` are the seeded generators
shared by the CPU rule tests (against pandas) and the GPU tests (the kernels against this module).

The rule ("Resume filter"): a text is taken natively only where the parse provably equals
``pd.read_csv(text)[column].astype(str).tolist()``.  Quote state is the parity of the '"' bytes before a byte.
Conditions are tested in this order, each over the whole text, the position being its first offender's:

  1. NUL    no NUL byte (its position);
     UTF8   the text is valid UTF-8 (the byte a strict decoder stops at);
  2. HEADER the text starts with the header line, ended by '\\n' or '\\r\\n' (position 0);
  3. QUOTE  every opening '"' is a field's first byte or follows a '"'; every closing '"' is followed by ',', '\\n',
            '\\r', '"' or the end of the text (the quote's position); the text ends outside quotes (position: its length);
  4. CR     outside quotes '\\r' is followed by '\\n' (its position);
  5. ROWS   there is a record after the header (position: the text's length);
  6. FIELDS every record that is not zero-length has exactly the header's number of fields (its first byte);
  7. URL    the column's cell, outer quotes removed, holds a ':' and no '"', '\\n' or '\\r' (its record's first byte).

Outside quotes '\\n' ends a record and ',' a field; a record's '\\r' before the '\\n' is not part of it; records of
zero length are skipped.
"""
import csv
import io
import random
import re

OK, NUL, UTF8, HEADER, QUOTE, CR, ROWS, FIELDS, URL = range(9)   # (in the order they are tested)
NAMES = ['OK', 'NUL', 'UTF8', 'HEADER', 'QUOTE', 'CR', 'ROWS', 'FIELDS', 'URL']
# the condition of the list above a verdict names
CONDITION = {NUL: 1, UTF8: 1, HEADER: 2, QUOTE: 3, CR: 4, ROWS: 5, FIELDS: 6, URL: 7}

SUCCESS_HEADER = b'url,datetime,ticker_symbols,author,source,source_url,title,article'
FAILED_HEADER = b'url,error'
LINKS_HEADER = b'date_time,url'
# (header line, the 'url' column)
FILES = {'success': (SUCCESS_HEADER, 0), 'failed': (FAILED_HEADER, 0), 'links': (LINKS_HEADER, 1)}

_EVENTS = re.compile(rb'["\r\n,]')


def parse(text: bytes, header: bytes, url_col: int):
    """(verdict, bad_pos, cells): cells is the list of the column's cells (bytes) when the verdict is OK, else None;
    bad_pos is -1 when OK."""
    n = len(text)
    n_fields = header.count(b',') + 1
    p = text.find(b'\0')
    if p >= 0:
        return NUL, p, None
    try:
        text.decode('utf-8')
    except UnicodeDecodeError as e:
        return UTF8, e.start, None
    if not (text.startswith(header + b'\n') or text.startswith(header + b'\r\n')):
        return HEADER, 0, None
    inq, bad_q, bad_cr = False, None, None
    recs, start, delims = [], 0, []
    for m in _EVENTS.finditer(text):
        i = m.start()
        c = text[i]
        if c == 0x22:
            if not inq:
                prev = text[i - 1] if i else 0x0A
                if prev not in (0x2C, 0x0A, 0x22) and bad_q is None:
                    bad_q = i
            else:
                nxt = text[i + 1] if i + 1 < n else None
                if nxt not in (None, 0x2C, 0x0A, 0x0D, 0x22) and bad_q is None:
                    bad_q = i
            inq = not inq
        elif inq:
            continue
        elif c == 0x0D:
            if not (i + 1 < n and text[i + 1] == 0x0A) and bad_cr is None:
                bad_cr = i
        elif c == 0x2C:
            delims.append(i)
        else:
            end = i - 1 if i > start and text[i - 1] == 0x0D else i
            if end > start:
                recs.append((start, end, delims))
            start, delims = i + 1, []
    if bad_q is None and inq:
        bad_q = n
    if bad_q is not None:
        return QUOTE, bad_q, None
    if bad_cr is not None:
        return CR, bad_cr, None
    if start < n:
        recs.append((start, n, delims))
    recs = recs[1:]   # (the header)
    if not recs:
        return ROWS, n, None
    for s, e, d in recs:
        if len(d) + 1 != n_fields:
            return FIELDS, s, None
    cells = []
    for s, e, d in recs:
        b = s if url_col == 0 else d[url_col - 1] + 1
        c = e if url_col == n_fields - 1 else d[url_col]
        if c - b >= 2 and text[b] == 0x22:
            b, c = b + 1, c - 1
        cell = text[b:c]
        if b':' not in cell or b'"' in cell or b'\n' in cell or b'\r' in cell:
            return URL, s, None
        cells.append(cell)
    return OK, -1, cells


def pandas_urls(text: bytes, header: bytes, url_col: int):
    """The reference's read: ``pd.read_csv(file)[column].astype(str).tolist()``."""
    import pandas as pd
    name = header.decode().split(',')[url_col]
    return pd.read_csv(io.BytesIO(text))[name].astype(str).tolist()


# ------------------------------------------------------------------ the seeded fuzz
_URLS = ['https://finance.yahoo.com/news/a-%d.html', 'http://finance.yahoo.com:80/news/b-%d.html?x=1',
         'https://finance.yahoo.com/news/d,%d,e.html', 'https://finance.yahoo.com/news/é-%d.html',
         'https://finance.yahoo.com/news/€\U0001F600-%d.html', ' http://x.com/news/%d.html ', 'a:%d', ':%d',
         "https://x.com/it's-%d.html"]
_CELLS = ['', 'nan', 'NA', '123', '1.5', 'True', 'plain text', 'with, comma', 'say "hi"', '"', '""', 'two\nlines',
          'cr\r\nlf', 'lone\rcr', 'é€\U0001F600', 'a,"b"\n"c",d', ' lead', 'trail ', '2024-01-02 03:04:05',
          'Line one.\n\n"Quoted," she said.\nLine, three.', "it's", ';', '\t', 'x' * 300]
# cells of the column that pandas would not keep as the str of its bytes, and other ineligible ones
_ODD_URLS = ['nan', 'NA', '', '123', '1.5', 'True', 'nocolon', 'null', 'N/A', '-', 'http', 'q"uote:x', 'nl\n:x', 'cr\r:x',
             '"']
_BAD_UTF8 = [b'\xff', b'\xc0\xaf', b'\xed\xa0\x80', b'\xf4\x90\x80\x80', b'\xe2\x82', b'\x80', b'\xc3',
             b'\xe0\x9f\xbf', b'\xf0\x8f\xbf\xbf', b'\xf0\x90\x80\x80\x80', b'\x80\x80\x80\x80\x80']


def _rows(rng, n_fields, url_col, n, terminator='\r\n'):
    # (csv.writer quotes the characters of its line terminator: under '\n' a '\r' would go out unquoted)
    pool = _CELLS if '\r' in terminator else [c for c in _CELLS if '\r' not in c]
    out = []
    for _ in range(n):
        row = [rng.choice(pool) for _ in range(n_fields)]
        row[url_col] = rng.choice(_URLS) % rng.randrange(40)
        out.append(row)
    return out


def _write(header: bytes, rows, terminator='\r\n', final=True) -> bytes:
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator=terminator)
    w.writerow(header.decode().split(','))
    w.writerows(rows)
    text = buf.getvalue().encode('utf-8')
    return text if final else text[:-len(terminator)]


def fuzz_clean(seed: int, kind: str = 'success') -> bytes:
    """``csv.writer`` output under the file's header (at least one row, every cell of the column holds ':' and no
    '"' or line break): eligible by construction."""
    header, url_col = FILES[kind]
    rng = random.Random(seed * 7919 + len(header))
    n = rng.choice([1, 2, 3, 17, 64, 65]) if rng.random() < 0.7 else 1 + rng.randrange(80)
    term = rng.choice(['\r\n', '\r\n', '\n'])
    rows = _rows(rng, header.count(b',') + 1, url_col, n, term)
    return _write(header, rows, term, rng.random() < 0.8)


# the violations a dirty text is made with, and the verdict each must get (blank-line runs leave a text eligible)
VIOLATIONS = ['nul', 'utf8', 'header', 'midquote', 'afterquote', 'openquote', 'lonecr', 'fewer', 'more', 'oddurl',
              'norows', 'blanks', 'quotedurl']
EXPECT = {'nul': NUL, 'utf8': UTF8, 'header': HEADER, 'midquote': QUOTE, 'afterquote': QUOTE, 'openquote': QUOTE,
          'lonecr': CR, 'fewer': FIELDS, 'more': FIELDS, 'oddurl': URL, 'norows': ROWS, 'blanks': OK, 'quotedurl': URL}


def fuzz_dirty(seed: int, kind: str = 'success'):
    """(violation, text): a clean text with one violation injected as a record of its own (or into the header)."""
    header, url_col = FILES[kind]
    nf = header.count(b',') + 1
    rng = random.Random(seed * 104729 + len(header))
    what = VIOLATIONS[seed % len(VIOLATIONS)]
    term = rng.choice(['\r\n', '\n'])
    t = term.encode()
    rows = _rows(rng, nf, url_col, rng.choice([1, 2, 5, 30]), term)
    lines = [_write(header, [r], term)[len(header) + len(t):] for r in rows]   # one encoded record each
    good = ['c%d' % k for k in range(nf)]
    good[url_col] = 'http://ok/%d' % seed

    def rec(cells):
        return ','.join(cells).encode('utf-8') + t
    head = header + t
    at = rng.randrange(len(lines) + 1)
    if what == 'nul':
        new = rec(good).replace(b'ok', b'o\0k')
    elif what == 'utf8':
        b = rec(good)
        k = rng.randrange(len(b) - len(t) + 1)
        new = b[:k] + rng.choice(_BAD_UTF8) + b[k:]
    elif what == 'header':
        head = rng.choice([header + b' ' + t, header[:-1] + t, header.upper() + t, b'"' + header + b'"' + t, header,
                           t + header + t])
        new = rec(good)
    elif what == 'midquote':
        cells = list(good)
        cells[rng.randrange(nf)] += 'ab"c'
        new = rec(cells)
    elif what == 'afterquote':
        cells = list(good)
        k = rng.randrange(nf)
        cells[k] = '"%s"y' % cells[k]
        new = rec(cells)
    elif what == 'openquote':
        cells = list(good)
        cells[-1] = '"never closed'
        new = rec(cells)
        at = len(lines)
    elif what == 'lonecr':
        cells = list(good)
        cells[rng.randrange(nf)] += rng.choice(['\rx', '\r '])
        new = rec(cells) if rng.random() < 0.7 else b'\r' + rec(good)
    elif what == 'fewer':
        new = rec(good[:-1]) if nf > 2 or rng.random() < 0.5 else rng.choice([b' ', b'x', b'\t', b'""']) + t
    elif what == 'more':
        new = rec(good + ['extra'])
    elif what == 'oddurl':
        cells = list(good)
        cells[url_col] = rng.choice(_ODD_URLS[:11])
        new = rec(cells)
    elif what == 'quotedurl':
        cells = list(good)
        cells[url_col] = rng.choice(['"http://a""b"', '"http://a\nb"', '"http://a\rb"', '""', '"nocolon,x"'])
        new = rec(cells)
    elif what == 'norows':
        lines, new = [], rng.choice([b'', t, t + t])
    else:   # blank-line runs: still eligible
        new = t * rng.choice([1, 2, 5])
    lines.insert(at, new)
    text = head + b''.join(lines)
    if what in ('nul', 'utf8', 'midquote', 'fewer', 'more', 'oddurl') and rng.random() < 0.3 and text.endswith(t):
        text = text[:-len(t)]   # a final record without a terminator
    return what, text
