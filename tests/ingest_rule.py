"""Pure-Python restatement of the device ingest's take rule and of what it produces (csrc/kwingest.hip,
include/kwingest.h; DESIGN.md §7, "Article ingest").

``parse(text, ncols, final, max_rows, na)`` is what ``kw_ingest_parse`` computes: a verdict, the byte position of the
first offender, ``n_rows``, ``consumed`` and (when OK) the cells as ``kwcsv_parse`` lays them out.  The CPU tests pin
it against ``kwcsv_parse`` (csrc/kwcsv.c); the GPU tests use its generators and its verdicts.

The quote state of a byte is the parity of the '"' bytes before it.  Outside quotes ',' ends a field and '\\n' ends
a record ("\\r\\n": the '\\r' belongs to the terminator); a record of no bytes but its terminator is skipped.  With
``final`` false the records are those whose '\\n' lies in the text; with ``final`` the text's end also ends a record
that has bytes.  The first ``max_rows`` records are taken; ``consumed`` is the position after the last taken
record's '\\n' (the text's length when ``final`` and the text has fewer than ``max_rows`` records).  The conditions
are tested over the bytes before a limit -- ``consumed``, or the text's length when ``final`` and the text has
fewer than ``max_rows`` records -- in this order, the position being the condition's first offender's:

  1. NUL     no NUL byte (its position);
     UTF8    valid UTF-8, strictly (the byte a strict decoder stops at);
  2. QUOTE   a '"' outside quotes follows ',', '\\n' or '"' (the text starts after a virtual '\\n'); a '"' inside
             quotes is followed by ',', '\\n', '\\r' or '"' (the text's last byte passes) (the quote's position);
             a final text ends outside quotes (position: its length);
  3. CR      outside quotes '\\r' is followed by '\\n' (its position; the last byte of a text that is not final passes);
  4. BLANK   no taken record is spaces and tabs only (the record's first byte);
  5. FIELDS  every taken record has exactly ncols fields (the position of its '\\n', or the text's length);
  6. ROWS    n_rows and the cell count stay below 2^31.

A cell's bytes are its record's without the separators, the opening and closing quote and the first '"' of a pair.
"""
import csv
import io
import random

OK, NUL, UTF8, QUOTE, CR, BLANK, FIELDS, ROWS = range(8)   # (in the order they are tested)
NAMES = ['OK', 'NUL', 'UTF8', 'QUOTE', 'CR', 'BLANK', 'FIELDS', 'ROWS']
F_QUOTED, F_NA, F_TEXT, F_CANON = 1, 2, 4, 8                # KWCSV_* (csrc/kwcsv.c)


def text_witness(s: bytes) -> bool:
    """kwcsv_text_witness: a non-NA cell that no number and no bool literal can be."""
    t = s.strip(b' \t')
    if not t:
        return True
    low = t.lower()
    if low in (b'true', b'false'):
        return False
    if (low[1:] if low[:1] in (b'+', b'-') else low) in (b'inf', b'infinity'):
        return False
    return any(c not in b'0123456789+-.eE' for c in t)


def parse(text: bytes, ncols: int, final: bool, max_rows: int, na=frozenset()):
    """(verdict, bad_pos, n_rows, consumed, cells): cells = (bytes, offsets, flags) of the taken rows when the
    verdict is OK, else None with n_rows = consumed = 0; bad_pos is 0 when OK."""
    n = len(text)
    byte = lambda i: text[i] if 0 <= i < n else (0x0A if i < 0 else 0x100)   # noqa: E731
    par, inside = 0, []
    for b in text:
        inside.append(par)
        par ^= b == 0x22
    ends, delim, kept, opening, need = [], set(), [], set(), set()
    bad_q, bad_cr = [], []
    for i, b in enumerate(text):
        sb, keep = inside[i], True
        if b == 0x22:
            if not sb:
                if byte(i - 1) not in (0x2C, 0x0A, 0x22):
                    bad_q.append(i)
                if byte(i - 1) == 0x22:
                    need.add(i)            # the second '"' of a pair: kept
                else:
                    opening.add(i)
                    keep = False
            else:
                if byte(i + 1) not in (0x2C, 0x0A, 0x0D, 0x22, 0x100):
                    bad_q.append(i)
                keep = False               # a closing quote or the first '"' of a pair
        elif b == 0x2C:
            if sb:
                need.add(i)
            else:
                delim.add(i)
                keep = False
        elif b == 0x0A:
            if sb:
                need.add(i)
            else:
                keep = False
                if not (byte(i - 1) == 0x0A or (byte(i - 1) == 0x0D and byte(i - 2) == 0x0A)):
                    ends.append(i)
        elif b == 0x0D and not sb:
            keep = False
            if byte(i + 1) != 0x0A and (final or i + 1 < n):
                bad_cr.append(i)
        if keep:
            kept.append(i)
    if final and n and not par and not (text[-1] == 0x0A and not inside[-1]):
        ends.append(n)                     # the text's end ends the last record
    found = len(ends)
    n_rows = min(found, max_rows)
    to_end = final and found < max_rows
    consumed = n if to_end else (min(ends[n_rows - 1] + 1, n) if n_rows else 0)
    limit = consumed

    def refuse(v, pos):
        return v, pos, 0, 0, None

    p = text.find(b'\0', 0, limit)
    if p >= 0:
        return refuse(NUL, p)
    try:
        text.decode('utf-8')
    except UnicodeDecodeError as e:
        if e.start < limit:
            return refuse(UTF8, e.start)
    q = [i for i in bad_q if i < limit]
    if q:
        return refuse(QUOTE, q[0])
    if to_end and par:
        return refuse(QUOTE, n)
    c = [i for i in bad_cr if i < limit]
    if c:
        return refuse(CR, c[0])
    # the taken records: [start, end) without the terminator
    spans, start = [], 0
    blank, fields = None, None
    for e in ends[:n_rows]:
        while start < e and not inside[start] and (text[start] == 0x0A or text[start:start + 2] == b'\r\n'):
            start += 1 if text[start] == 0x0A else 2      # zero-length records before it
        stop = e - 1 if (e > start and e <= n and byte(e - 1) == 0x0D and not inside[e - 1]) else e
        spans.append((start, stop, e))
        start = e + 1
    for a, b, e in spans:
        if blank is None and not text[a:b].strip(b' \t'):
            blank = a
        if fields is None and sum(1 for i in range(a, b) if i in delim) + 1 != ncols:
            fields = e
    if blank is not None:
        return refuse(BLANK, blank)
    if fields is not None:
        return refuse(FIELDS, fields)
    if n_rows >= 2 ** 31 or n_rows * ncols >= 2 ** 31:
        return refuse(ROWS, 0)
    out, off, fl = bytearray(), [0], []
    keptset = set(kept)
    for a, b, e in spans:
        cell0, quoted, needq = len(out), False, False
        for i in range(a, b + 1):
            if i == b or i in delim:
                s = bytes(out[cell0:])
                f = (F_QUOTED if quoted else 0) | (F_CANON if quoted == needq else 0)
                f |= F_NA if s in na else (F_TEXT if text_witness(s) else 0)
                fl.append(f)
                off.append(len(out))
                cell0, quoted, needq = len(out), False, False
                continue
            if i in keptset:
                out.append(text[i])
            quoted |= i in opening
            needq |= i in need
    return OK, 0, n_rows, consumed, (bytes(out), off, fl)


# ---- generators

WORDS = ['alpha', 'Beta corp', 'nan', 'NA', 'N/A', 'null', 'NULL', 'n/a ', 'NaN', '<NA>', '#N/A', 'None', 'nul',
         '12', '-3.5e7', '+inf', 'Infinity', 'true', 'FALSE', ' 42 ', 'tru', '1,2', 'say ""hi""', 'q"x', 'line\nbreak',
         'cr\r\nlf', 'café', '€ 9', '\U0001F600 ok', '', ' ', '\t', 'http://a.b/c?d=e', '2021-03-04 05:06:07',
         '2021-02-30 00:00:00', '0999-01-01T00:00:00', '2020-02-29T23:59:59', 'a b c d e f g h i j k l m n o p']


def clean_text(seed: int):
    """(text, ncols): csv.writer output, 6-9 columns, QUOTE_MINIMAL, either line terminator; no NUL, no lone '\\r'."""
    rng = random.Random(seed)
    ncols = rng.randint(6, 9)
    term = rng.choice(['\n', '\r\n'])
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator=term, quoting=csv.QUOTE_MINIMAL)
    for _ in range(rng.randint(1, 12)):
        row = []
        for _c in range(ncols):
            k = rng.random()
            if k < 0.75:
                row.append(rng.choice(WORDS))
            else:
                row.append(' '.join(rng.choice(WORDS) for _j in range(rng.randint(2, 5))))
        w.writerow(row)
    text = buf.getvalue().encode('utf-8')
    if rng.random() < 0.3 and text.endswith(term.encode()):
        text = text[:-len(term)]            # the last record without its terminator
    return text, ncols


def fuzz_text(seed: int):
    """(text, ncols): a clean text with up to three random byte edits -- most stay parseable, many do not."""
    text, ncols = clean_text(seed)
    rng = random.Random(seed * 7919 + 1)
    b = bytearray(text)
    for _ in range(rng.randint(0, 3)):
        i = rng.randrange(len(b) + 1)
        if rng.random() < 0.3:
            i = bytes(b).rfind(b'\n', 0, i) + 1     # at a line's start
        ins = rng.choice([b'"', b',', b'\n', b'\r', b'\r\n', b' ', b'""', b'\0', b'\xff', b'\xe2\x82', b'x', b'\n\n',
                          b'  \n', b'\t'])
        if rng.random() < 0.5:
            b[i:i] = ins
        else:
            b[i:i + 1] = ins
    return bytes(b), ncols


# ---- the oracle: the project's host tokenizer (csrc/kwcsv.c through advanced_scrapper_amd.ingest)

def na_set():
    from advanced_scrapper_amd import ingest
    buf, off, n = ingest._na_table()
    return frozenset(bytes(buf[off[k]:off[k + 1]]) for k in range(n))


def host_parse(text: bytes, ncols: int, max_rows: int, na=None):
    """kwcsv_parse of text from position 0: (rows or a negative code, pos_out, cell bytes, offsets, flags, spans).
    ``na``: a (buf, off, n) triple in the shape of ingest._na_table() (pandas' own table by default)."""
    import ctypes
    import numpy as np
    from advanced_scrapper_amd import ingest
    na_buf, na_off, n_na = ingest._na_table() if na is None else na
    buf = np.frombuffer(text + b'\0' * 16, dtype=np.uint8)
    cap_rows = min(max_rows, len(text) + 1)
    out = np.zeros(len(text) + 16, dtype=np.uint8)
    coff = np.zeros(cap_rows * ncols + 1, dtype=np.int64)
    cfl = np.zeros(max(cap_rows * ncols, 1), dtype=np.uint8)
    span = np.zeros(2 * cap_rows + 2, dtype=np.int64)
    pos = ctypes.c_int64(0)
    p = ingest._p
    rows = ingest._lib().kwcsv_parse(p(buf), len(text), 0, cap_rows, ncols, p(na_buf), p(na_off), n_na, p(out),
                                     len(text) + 16, p(coff), p(cfl), ctypes.byref(pos), p(span))
    if rows < 0:
        return int(rows), 0, b'', [0], [], []
    nc = int(rows) * ncols
    return (int(rows), int(pos.value), out[:int(coff[nc])].tobytes(), coff[:nc + 1].tolist(), cfl[:nc].tolist(),
            span[:2 * int(rows)].reshape(-1, 2).tolist())


def names_for(ncols: int, cols):
    """Column names with the six needed ones (ingest.NEEDED order) at ``cols``."""
    from advanced_scrapper_amd import ingest
    names = [f'c{i}' for i in range(ncols)]
    for k, c in enumerate(cols):
        names[c] = ingest.NEEDED[k]
    return names


def host_oracle(text: bytes, ncols: int, cols, max_rows: int, na=None):
    """What the host route computes for the first max_rows records of text (read as a final text): a dict of
    n_rows, consumed, cells, coff, cfl, arena, off, us, kind, witness -- through kwcsv_parse (with the NA table
    ``na``, pandas' own by default), kwcsv_pack_mt and kwcsv_dates (advanced_scrapper_amd.ingest)."""
    import numpy as np
    from advanced_scrapper_amd import ingest
    rows, pos, out, coff, cfl, spans = host_parse(text, ncols, max_rows, na)
    assert rows >= 0, rows
    cells = ingest.Cells(np.frombuffer(out + b'\0' * 16, dtype=np.uint8), np.asarray(coff, dtype=np.int64),
                         np.asarray(cfl, dtype=np.uint8), rows, ncols)
    chunk = ingest.NativeChunk(cells, names_for(ncols, cols), 0)
    arena, off = chunk.arena()
    us = np.zeros(max(rows, 1), dtype=np.int64)
    kind = np.zeros(max(rows, 1), dtype=np.uint8)
    p = ingest._p
    ingest._lib().kwcsv_dates(p(cells.buf), p(cells.off), p(cells.flags), rows, ncols, cols[2], p(us), p(kind), 1)
    fl = np.asarray(cfl, dtype=np.uint8).reshape(rows, ncols) if rows else np.zeros((0, ncols), np.uint8)
    return {'n_rows': rows, 'consumed': pos, 'cells': out, 'coff': list(coff), 'cfl': list(cfl),
            'arena': arena.tobytes(), 'off': off.tolist(), 'us': us[:rows].tolist(), 'kind': kind[:rows].tolist(),
            'witness': [int(bool((fl[:, c] & F_TEXT).any())) for c in cols], 'spans': spans}
