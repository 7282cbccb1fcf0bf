"""Pure-Python restatement of the CDX ingest rule, its parse and the CSV rendering (csrc/cdx.hip, include/kwdedup.h).

``parse(text, dialect)`` is what ``kw_cdx_append`` computes: a verdict, the offending line, and (when OK) the
``(timestamp, url bytes)`` rows.  ``render_csv(rows)`` is what ``kw_cdx_csv_*`` writes.  ``fuzz_listings()`` is the
seeded generator shared by the CPU rule tests (against pandas) and the GPU tests (the kernel against this module).

The rule: a text is taken natively only where its parse provably equals
``pd.read_csv(delimiter=' ', header=None, usecols=[1, 2], names=['date_time', 'url'])`` (listing dialect) or
``pd.read_csv(part)`` (part-CSV dialect).  Conditions are tested in this order:

  1. no '"' byte, no '\\r' byte, no NUL byte in the whole text (bad_line: the line of the first such byte);
  2. part-CSV dialect: the text starts with the line ``date_time,url`` (bad_line 0);
  3. per non-blank line, the first offending line in order; within a line: valid UTF-8, the field count, the
     timestamp cell 1-18 ASCII digits, the URL cell contains ':'.

Blank lines (zero bytes between two '\\n') are dropped.  Lines are numbered from 0 by the '\\n' bytes before them.
"""
import random

OK, QUOTE, CR, NUL, FIELDS, TS, URL, UTF8, HEADER = range(9)
NAMES = ['OK', 'QUOTE', 'CR', 'NUL', 'FIELDS', 'TS', 'URL', 'UTF8', 'HEADER']

# (delimiter, ts_col, url_col, skip_lines, exact_fields)
LISTING = (b' ', 1, 2, 0, 0)
PART = (b',', 0, 1, 1, 2)
HEADER_LINE = b'date_time,url'


def parse(text: bytes, dialect=LISTING):
    """(verdict, bad_line, rows): rows is a list of (int timestamp, url bytes) when the verdict is OK, else None;
    bad_line is -1 when OK."""
    delim, ts_col, url_col, skip, exact = dialect
    for code, byte in ((QUOTE, b'"'), (CR, b'\r'), (NUL, b'\0')):
        p = text.find(byte)
        if p >= 0:
            return code, text.count(b'\n', 0, p), None
    lines = [(i, ln) for i, ln in enumerate(text.split(b'\n')) if ln]
    if skip:
        if not lines or lines[0] != (0, HEADER_LINE):
            return HEADER, 0, None
        lines = lines[1:]
    rows = []
    for i, ln in lines:
        try:
            ln.decode('utf-8')
        except UnicodeDecodeError:
            return UTF8, i, None
        cells = ln.split(delim)
        if (len(cells) != exact) if exact else (len(cells) < max(ts_col, url_col) + 1):
            return FIELDS, i, None
        ts, url = cells[ts_col], cells[url_col]
        if not (1 <= len(ts) <= 18 and all(0x30 <= c <= 0x39 for c in ts)):
            return TS, i, None
        if b':' not in url:
            return URL, i, None
        rows.append((int(ts), url))
    return OK, -1, rows


def render_csv(rows) -> bytes:
    """``DataFrame(rows, columns=['date_time', 'url']).to_csv(index=False)``: QUOTE_MINIMAL, where only ',' can
    ask for quotes (the rule keeps '"', '\\r' and '\\n' out of a URL)."""
    out = [b'date_time,url\n']
    for ts, url in rows:
        u = url if isinstance(url, bytes) else url.encode('utf-8')
        if b',' in u:
            u = b'"' + u + b'"'
        out.append(b'%d,' % ts + u + b'\n')
    return b''.join(out)


# ------------------------------------------------------------------ the seeded fuzz
_GOOD_URLS = ['https://finance.yahoo.com/news/a-%d.html', 'http://finance.yahoo.com:80/news/b-%d.html?x=1',
              'https://finance.yahoo.com/news/c-%d.htm', 'http://finance.yahoo.com/news/d,%d,e.html',
              'https://finance.yahoo.com/news/é-%d.html', 'https://finance.yahoo.com/news/€\U0001F600-%d.html',
              'http://x.com/news/%%20a-%d.html', 'https://finance.yahoo.com/video/q-%d.html&a=1,2']
# cells pandas would not keep as str, and other ineligible URL cells
_ODD_URLS = ['nan', 'NA', 'null', 'None', 'N/A', '123', '1.5', 'True', 'false', '-', 'inf', '1e5', 'NaN', '#N/A', '']
_ODD_TS = ['1' * 19, '-20200101000000', '+5', '2020.5', '1e5', 'abc', '', '12 ', 'nan', '0x10', '１２']
_BAD_UTF8 = [b'\xff', b'\xc0\xaf', b'\xed\xa0\x80', b'\xf4\x90\x80\x80', b'\xe2\x82', b'\x80', b'\xc3', b'\xe0\x9f\xbf',
             b'\xf0\x8f\xbf\xbf']


def _good_line(rng, k, delim=' '):
    ts = rng.choice(['20200102030405', '0', '7', '00020200102030', '123456789012345678', '000000000000000001',
                     '%014d' % rng.randrange(10 ** 14)])
    url = rng.choice(_GOOD_URLS) % rng.randrange(40)
    if delim == ' ':
        cells = ['com,yahoo)/k%d' % k, ts, url] + ['text/html', '200', 'DIGEST', '977'][:rng.choice([0, 0, 1, 4, 4, 4])]
        if rng.random() < 0.05:
            cells[0] = ''            # a line that starts with the delimiter
        return ' '.join(cells)
    if ',' in url:
        url = url.replace(',', ';')
    return ts + ',' + url


def fuzz_listing(seed: int, dialect=LISTING) -> bytes:
    """One small text (at most 200 lines) of the dialect; about half of them are eligible."""
    rng = random.Random(seed * 7919 + (1 if dialect is PART else 0))
    delim = dialect[0].decode()
    n = rng.choice([0, 1, 2, 3, 5, 17, 64, 65, 130, 200]) if rng.random() < 0.7 else rng.randrange(200)
    lines = [_good_line(rng, k, delim).encode('utf-8') for k in range(n)]
    # blank-line runs
    for _ in range(rng.choice([0, 0, 1, 3])):
        at = rng.randrange(len(lines) + 1)
        lines[at:at] = [b''] * rng.choice([1, 2, 5])
    lines = lines[:198]   # (the header line and one inserted offender still leave at most 200)
    if dialect is PART:
        lines.insert(0, HEADER_LINE)
    kind = rng.random()
    if kind < 0.5 and lines:
        at = rng.randrange(len(lines))
        what = rng.randrange(12)
        good = _good_line(rng, 999, delim)
        ts0, url0 = (good.split(' ')[1:3] if delim == ' ' else good.split(',', 1))
        mk = (lambda t, u: ('k %s %s m 200' % (t, u))) if delim == ' ' else (lambda t, u: '%s,%s' % (t, u))
        if what == 0:
            new = (good[:5] + '"' + good[5:]).encode()
        elif what == 1:
            new = good.encode() + b'\r'
        elif what == 2:
            new = (good[:7] + '\0' + good[7:]).encode()
        elif what == 3:   # too few fields / too many (exact)
            new = (rng.choice(['k', 'k 20200101000000', ' ', '  ', '\t', 'x']) if delim == ' ' else
                   rng.choice(['20200101000000', ts0 + ',' + url0 + ',extra', ' ', 'x'])).encode()
        elif what == 4:
            new = mk(rng.choice(_ODD_TS), url0).encode('utf-8')
        elif what == 5:
            new = mk(ts0, rng.choice(_ODD_URLS)).encode()
        elif what == 6:
            b = good.encode('utf-8')
            k = rng.randrange(len(b) + 1)
            new = b[:k] + rng.choice(_BAD_UTF8) + b[k:]
        elif what == 7 and dialect is PART:
            at = 0
            new = rng.choice([b'date_time,url ', b'date_time,ur', b'url,date_time', b'', b'Date_time,url'])
        elif what == 8:   # several offenders: the first one decides
            new = mk('x', url0).encode()
            lines.insert(min(len(lines), at + 1), mk(ts0, 'nocolon').encode())
        elif what == 9:
            new = mk(ts0, url0).encode() + b' ' * rng.choice([1, 2])   # trailing delimiters / spaces
        elif what == 10:
            new = b'\t' + good.encode('utf-8')
        else:
            new = mk(ts0, 'a' + url0[:3]).encode()   # 'ahtt': no colon
        lines[at] = new
    text = b'\n'.join(lines)
    if lines and rng.random() < 0.7:
        text += b'\n'
    return text


def fuzz_listings(count: int = 300, dialect=LISTING):
    return [fuzz_listing(s, dialect) for s in range(count)]
