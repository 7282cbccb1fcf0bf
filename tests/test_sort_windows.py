"""The window reader of the output sort's large-file route (``sortfiles.read_windows``) in isolation -- two byte
arrays for the staging slots, a fake parse built on the host tokenizer's record spans -- and the new kwsort.h
symbols against the built library's exports.  No GPU."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HEAD = b'time_unix,article_text,title,date_time,url,source_url,source\n'


def _body(seed: int, rows: int, final_newline: bool) -> bytes:
    """Records of 7 cells and 12 to a few thousand bytes, some with quoted line breaks, some ended by "\\r\\n",
    some followed by empty lines."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(rows):
        kind = int(rng.integers(0, 10))
        if kind == 0:
            text = b'"' + b'quoted, ""x""\nline\r\n' * int(rng.integers(1, 40)) + b'"'
        elif kind == 1:
            text = b'y' * int(rng.integers(300, 3000))
        else:
            text = b'w' * int(rng.integers(0, 60))
        out.append(b'%d,%s,t,d,u,v,s' % (int(rng.integers(0, 1000)), text))
        out.append((b'\n', b'\n', b'\n', b'\r\n', b'\n\n', b'\n\r\n\n')[int(rng.integers(0, 6))])
    body = b''.join(out)
    return body if final_newline else body.rstrip(b'\r\n')


def _record_ends(body: bytes):
    """(start, the position after the terminator) of every record, from the host tokenizer's spans."""
    from advanced_scrapper_amd import ingest
    span = (ingest.parse_all(HEAD + body)[2] - len(HEAD)).tolist()
    ends = []
    for a, b in span:
        t = b + 2 if body[b:b + 2] == b'\r\n' else b + 1 if body[b:b + 1] == b'\n' else b
        ends.append((a, t))
    return ends


class _Fake:
    """The callbacks of read_windows over byte arrays; ``parse`` takes the records whose line end lies in the
    window (the ingest's rule for a window that is not final) and checks what the window holds."""

    def __init__(self, body):
        self.body = body
        self.ends = _record_ends(body)
        self.slots = [bytearray(), bytearray()]
        self.seen = []             # (start, consumed, n_rows) of every window that gave rows
        self.sizes = []            # every parsed window's bytes
        self.next_row = 0

    def fill(self, slot, at, lo, n):
        buf = self.slots[slot]
        if len(buf) < at + n:
            buf.extend(bytes(at + n - len(buf)))
        buf[at:at + n] = self.body[lo:lo + n]

    def move(self, src, src_at, dst, dst_at, n):
        assert len(self.slots[dst]) >= dst_at + n
        self.slots[dst][dst_at:dst_at + n] = self.slots[src][src_at:src_at + n]

    def parse(self, slot, at, n, final, start):
        body = self.body
        assert bytes(self.slots[slot][at:at + n]) == body[start:start + n], 'the window is not the body at its start'
        assert final == (start + n == len(body))
        self.sizes.append(n)
        # a record start: the body's start, or the byte after a record's terminator
        assert start == 0 or start == self.ends[self.next_row - 1][1], start
        taken, r = 0, self.next_row
        while r < len(self.ends) and self.ends[r][1] <= start + n:
            if not final and body[self.ends[r][1] - 1:self.ends[r][1]] != b'\n':
                break              # (the body's last record without its line end: only a final window takes it)
            taken, r = taken + 1, r + 1
        consumed = n if final else (self.ends[r - 1][1] - start if taken else 0)
        self.next_row = r
        if taken:
            self.seen.append((start, consumed, taken))
        return taken, consumed


@pytest.mark.parametrize('threaded', (False, True))
@pytest.mark.parametrize('seed,rows,final_newline', ((1, 200, True), (2, 300, False), (3, 40, True), (4, 1, False)))
def test_windows_cover_the_body_once(seed, rows, final_newline, threaded):
    from advanced_scrapper_amd import sortfiles
    body = _body(seed, rows, final_newline)
    pool = ThreadPoolExecutor(max_workers=1) if threaded else None
    try:
        for window in (1, 7, 64, 100, 256, 1000, 4096, 1 << 16, len(body), len(body) + 5):
            f = _Fake(body)
            got = sortfiles.read_windows(len(body), window, f.fill, f.move, f.parse, pool.submit if pool else None)
            assert got == len(f.seen)
            assert f.next_row == len(f.ends) == rows, (window, f.next_row)
            pos = 0
            for start, consumed, _n in f.seen:
                assert start == pos and consumed > 0
                pos += consumed
            assert pos == len(body), (window, pos)
            assert sum(n for _s, _c, n in f.seen) == rows
            if window >= len(body):
                assert f.sizes == [len(body)]
            if window <= 64:
                assert max(f.sizes) > window, 'no window grew'
    finally:
        if pool:
            pool.shutdown()


def test_headroom_carry_and_reread(monkeypatch):
    """A tail within the headroom is moved in front of the bytes read ahead; a longer one reads the window again."""
    from advanced_scrapper_amd import sortfiles
    body = _body(9, 400, True)
    monkeypatch.setattr(sortfiles, 'HEADROOM', 128)
    for window in (512, 2048, 5000):
        f = _Fake(body)
        moves = []
        move = lambda *a: (moves.append(a[4]), f.move(*a))   # noqa: E731
        sortfiles.read_windows(len(body), window, f.fill, move, f.parse)
        assert f.next_row == len(f.ends) and sum(c for _s, c, _n in f.seen) == len(body)
        assert moves and max(moves) <= 128


def test_growth_stops_at_the_largest_window():
    from advanced_scrapper_amd import ingest, sortfiles
    sizes = []

    def parse(slot, at, n, final, start):
        assert start == 0 and not final
        sizes.append(n)
        return 0, 0

    nothing = lambda *a: None   # noqa: E731
    with pytest.raises(sortfiles.Refusal) as err:
        sortfiles.read_windows(1 << 33, 1 << 20, nothing, nothing, parse)
    assert err.value.reason == 'size'
    assert sizes[0] == 1 << 20 and sizes[-1] == ingest.MAX_WINDOW
    assert all(b == min(2 * a, ingest.MAX_WINDOW) for a, b in zip(sizes, sizes[1:]))
    # a record that the doubled window holds is taken, and the reader goes on
    sizes.clear()

    def parse2(slot, at, n, final, start):
        sizes.append((start, n))
        if final:
            return 1, n
        if start == 0 and n < (1 << 24):
            return 0, 0
        return 1, n - 10

    assert sortfiles.read_windows((1 << 26) + 3, 1 << 20, nothing, nothing, parse2) >= 3
    assert sizes[:5] == [(0, 1 << 20), (0, 1 << 21), (0, 1 << 22), (0, 1 << 23), (0, 1 << 24)]
    assert sizes[5][0] == (1 << 24) - 10 and sizes[-1][0] + sizes[-1][1] == (1 << 26) + 3


def test_sorter_arguments():
    import inspect
    from advanced_scrapper_amd import ingest, sortfiles
    sig = inspect.signature(sortfiles.DeviceSorter.__init__).parameters
    assert sig['large_from'].default == ingest.MAX_WINDOW
    assert sig['window_bytes'].default == sortfiles.WINDOW_BYTES and sig['slab_bytes'].default == sortfiles.SLAB_BYTES
    assert sortfiles.SLAB_BYTES % 1024 == 0 and sortfiles.WINDOW_BYTES < ingest.MAX_WINDOW
    st = sortfiles.reset_stats()
    assert st['windows'] == 0 and st['slabs'] == 0


def test_library_exports_the_windowed_sort():
    from advanced_scrapper_amd import _native
    new = ('kw_sort_begin', 'kw_sort_window', 'kw_sort_finish', 'kw_sort_gather_begin', 'kw_sort_gather_slab')
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'kwsort.h')).read()
    L = _native.lib()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True).stdout
    for f in new:
        assert re.search(rf'^int {f}\(', hdr, re.M), f
        assert f in _native.EXPORTS and hasattr(L, f), f
        assert re.search(rf'\bT {f}\b', out), f
