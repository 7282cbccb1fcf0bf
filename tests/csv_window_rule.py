"""Pure-Python restatement of the windowed CSV append (csrc/cdx.hip kw_csv_stream_*, include/kwdedup.h) on top of
``tests/resume_rule.parse``, and the inputs its CPU and GPU tests share.

``stream(text, header, url_col, window_bytes)`` cuts a text the way ``GpuUrlDedup.csv_append_file`` does: the file's
ranges ``[k * window_bytes, (k + 1) * window_bytes)``, each behind the unconsumed tail of the window before it.
``judge`` is one window: ``consumed`` is the position after the last '\\n' outside quotes (the window's length when
final); only the bytes before it are judged, by ``resume_rule.parse`` (a later window under a header line put in front
of it, since it starts at a record start outside quotes exactly as a text does after its header).  "No record after the
header" is the stream's end, not a window's.

The rule ("Windowed CSV append"): every verdict is OK iff ``parse`` over the whole text says OK, the
cells are then the same, and a text with one offender gets the whole-text verdict and position.
"""
from tests import resume_rule as R

RECORD = 'record'   # the refusal of a tail that outgrew max_record_bytes


def consumed_of(w: bytes, first: bool, final: bool, header: bytes) -> int:
    if not w:
        return 0
    if final:
        return len(w)
    if first and len(w) < len(header) + 1:
        return 0
    inq, last = False, 0
    for i, c in enumerate(w):
        if c == 0x22:
            inq = not inq
        elif c == 0x0A and not inq:
            last = i + 1
    return last


def judge(w: bytes, header: bytes, url_col: int, first: bool, final: bool):
    """(verdict, the offender's position in the window or -1, the column's cells, consumed)."""
    if not w:
        return (R.HEADER, 0, None, 0) if first and final else (R.OK, -1, [], 0)
    used = consumed_of(w, first, final, header)
    if used == 0:
        return R.OK, -1, [], 0
    pre = b'' if first else header + b'\n'
    verdict, pos, cells = R.parse(pre + w[:used], header, url_col)
    if verdict == R.ROWS:   # (blank lines, or the header alone)
        return R.OK, -1, [], used
    if verdict != R.OK:
        return verdict, pos - len(pre), None, 0
    return R.OK, -1, cells, used


def stream(text: bytes, header: bytes, url_col: int, window_bytes: int, max_record_bytes=None, judge_window=None):
    """(verdict, file position of the offender or -1, cells or None, the windows' consumed values).  ``judge_window(w,
    first, final)`` stands in for ``judge`` (the GPU tests pass kw_csv_stream_window)."""
    if judge_window is None:
        def judge_window(w, first, final):
            return judge(w, header, url_col, first, final)
    n_win = max(1, -(-len(text) // window_bytes))
    tail, pos, first, cells, consumed = b'', 0, True, [], []
    for k in range(n_win):
        w = tail + text[k * window_bytes:(k + 1) * window_bytes]
        final = k == n_win - 1
        verdict, bad, got, used = judge_window(w, first, final)
        if verdict != R.OK:
            return verdict, pos + bad, None, consumed
        consumed.append(used)
        cells += got
        first = first and used == 0
        pos += used
        tail = w[used:]
        if not final and max_record_bytes is not None and len(tail) > max_record_bytes:
            return RECORD, -1, None, consumed
    if not cells:
        return R.ROWS, len(text), None, consumed
    return R.OK, -1, cells, consumed


# ------------------------------------------------------------------ the designed edge text
# One region that holds every feature a cut can fall into: a quoted cell with '\n' and '\r\n' inside, a "" pair, a ','
# inside quotes, a two-, three- and four-byte UTF-8 character, a record ended '\r\n' next to one ended '\n', an empty
# line, and a closing quote as the last byte before the terminator.
def _record(k: int, article: str, term: str) -> str:
    return 'https://x.com/news/%d.html,2024-01-02,T%d,au,src,http://s/%d,title %d,%s%s' % (k, k, k, k, article, term)


SWEEP = 96
REGION = ('a:1,,,,,,,"x\ny\r\n""q"",é€\U0001F600"\r\n'   # (short cells: the whole region lies inside one sweep)
          'b:2,,,,,,,p\n'
          '\n'
          'c:3,,,,,,,"z"\r\n'
          '"d:4",,,,,,,w\n').encode('utf-8')
REGION_CELLS = [b'a:1', b'b:2', b'c:3', b'd:4']
assert len(REGION) < SWEEP


def edge_text(region_at: int):
    """(text, where the region starts): a success-file header, about 40 records, the region at ``region_at``."""
    head = R.SUCCESS_HEADER + b'\r\n'
    before, k = b'', 0
    while True:
        rec = _record(k, 'body %d %s' % (k, 'w' * 50), '\r\n' if k % 3 else '\n').encode()
        if len(head) + len(before) + len(rec) > region_at - 60:
            break
        before += rec
        k += 1
    fill = region_at - len(head) - len(before)
    pad = ('https://x.com/news/pad.html,d,t,a,s,u,t,' + 'p' * 400)[:fill - 1].encode() + b'\n'
    assert len(pad) == fill and pad.count(b',') == 7
    after = b''.join(_record(k + 1 + j, 'tail %d' % j, '\n' if j % 2 else '\r\n').encode() for j in range(max(8, 36 - k)))
    text = head + before + pad + REGION + after
    assert text[region_at:region_at + len(REGION)] == REGION
    return text, region_at


# the region at its natural place, across a 4096-byte tile edge, and across a 16-byte lane edge (start = 8 mod 16)
EDGE_PLACES = {'plain': 1500, 'tile': 4096 - 50, 'lane': 2048 + 8}


def sweep_windows(region_at: int):
    """The 96 window sizes whose first cut moves byte by byte through the region."""
    return list(range(region_at + 1, region_at + 1 + SWEEP))


# ------------------------------------------------------------------ one violation, in the first, a middle and the last window
def filler(size: int, k0: int) -> bytes:
    """Clean records of the failed file with a quoted multi-line cell each, at least ``size`` bytes."""
    out, k = b'', k0
    while len(out) < size:
        out += ('http://fill/%d,"say ""%d"",\nmore"\r\n' % (k, k)).encode()
        k += 1
    return out


def violation_texts(what: str, tile: int):
    """{place: text} for windows of one tile: a ``fuzz_dirty`` text of the failed file (shorter than half a tile) with
    clean records around it, so that its violation falls into the first, a middle or the last window.  A wrong
    header is the first window's alone; a text without rows has one window."""
    header, _ = R.FILES['failed']
    seed = next(s for s in range(R.VIOLATIONS.index(what), 4000, len(R.VIOLATIONS))
                if len(R.fuzz_dirty(s, 'failed')[1]) < tile // 2)
    _, dirty = R.fuzz_dirty(seed, 'failed')
    if what == 'norows':
        return {'first': dirty}
    if what == 'header':
        return {'first': dirty + filler(3 * tile, 9000)}
    t = 2 if dirty[len(header):len(header) + 2] == b'\r\n' else 1
    head, body = dirty[:len(header) + t], dirty[len(header) + t:]
    inner = body if body.endswith(b'\n') else body + b'\n'
    return {'first': head + inner + filler(3 * tile, 9000),
            'middle': head + filler(tile + tile // 2, 0) + inner + filler(tile + tile // 2, 9000),
            'last': head + filler(3 * tile, 0) + body}
