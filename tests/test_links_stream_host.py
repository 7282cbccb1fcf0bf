"""CPU: the host side of the streamed link, resume and new-links routes (cdx_dedup._stream_file, links.py,
resume.py): the part dialect's host cut, the 'record' refusal, the routing by ``stream_from``, and
``links.find_new_urls``' pandas route against the reference's own run (tests/golden/new_links_golden.json).
"""
import ctypes
import json
import os

import numpy as np
import pytest

from advanced_scrapper_amd import _native, cdx_dedup, links, resume

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'new_links_golden.json')


class HostDedup(cdx_dedup.GpuUrlDedup):
    """The stream reader with host tensors in place of pinned and device memory, and no device calls."""

    def __init__(self):
        import torch
        self.torch, self.device, self.h = torch, 0, None

    def _stream_buffers(self, window_bytes, max_record_bytes):
        t = self.torch
        return ([t.empty(window_bytes, dtype=t.uint8) for _ in range(2)],
                [t.empty(window_bytes + max_record_bytes + 64, dtype=t.uint8) for _ in range(2)])

    def _stream_mark(self):
        return None

    def _stream_sync(self):
        pass

    def _stream_ptr(self):
        return ctypes.c_void_p(0)


class FakeLib:
    """kw_cdx_append that records what it was given and takes every line of two fields."""

    def __init__(self, refuse_at=None):
        self.calls, self.refuse_at = [], refuse_at

    def kw_cdx_append(self, h, d_text, n, dia, rows, verdict, bad, stream):
        text = ctypes.string_at(d_text.value, n) if n else b''
        skip = dia._obj.skip_lines
        self.calls.append((text, skip))
        lines = [ln for ln in text.split(b'\n') if ln][skip:]
        ok = self.refuse_at is None or len(self.calls) - 1 != self.refuse_at
        verdict._obj.value = _native.KW_CDX_OK if ok else _native.KW_CDX_FIELDS
        rows._obj.value = len(lines) if ok else 0
        bad._obj.value = -1
        return 0


def _links_text(n):
    return 'date_time,url\n' + ''.join('%d,http://h/%s\n' % (20240101000000 + k, 'p' * (k % 37)) for k in range(n))


@pytest.mark.parametrize('window', [16, 64, 100, 257, 4096, 1 << 20])
@pytest.mark.parametrize('final_newline', [True, False])
def test_part_dialect_host_cut(tmp_path, monkeypatch, window, final_newline):
    text = _links_text(120).encode()
    if not final_newline:
        text = text[:-1]
    path = tmp_path / 'links.csv'
    path.write_bytes(text)
    fake = FakeLib()
    monkeypatch.setattr(_native, 'lib', lambda: fake)
    verdict, rows, stats = HostDedup().cdx_append_file(str(path), 'part', window, 1 << 12)
    assert (verdict, rows, stats['refusal']) == (_native.KW_CDX_OK, 120, None)
    assert stats['windows'] == max(1, -(-len(text) // window)) and sum(stats['consumed']) == len(text)
    # the windows handed over end at a '\n' (the last at the file's end), follow each other, skip the header once
    assert b''.join(t for t, _ in fake.calls) == text
    assert all(t.endswith(b'\n') for t, _ in fake.calls[:-1]) and all(t for t, _ in fake.calls)
    assert [s for _, s in fake.calls] == [1] + [0] * (len(fake.calls) - 1)
    # no window is cut before its last '\n': what is carried holds no line end
    at = 0
    for k, used in enumerate(stats['consumed'][:-1]):
        at += used
        assert b'\n' not in text[at:(k + 1) * window]


def test_part_dialect_record_refusal_and_verdict(tmp_path, monkeypatch):
    long = ('date_time,url\n1,http://h/a\n2,http://h/' + 'x' * 5000 + '\n3,http://h/b\n').encode()
    path = tmp_path / 'links.csv'
    path.write_bytes(long)
    fake = FakeLib()
    monkeypatch.setattr(_native, 'lib', lambda: fake)
    verdict, rows, stats = HostDedup().cdx_append_file(str(path), 'part', 512, 2048)
    assert (verdict, rows, stats['refusal']) == (None, 0, 'record') and stats['tail_max'] > 2048
    assert len(fake.calls) == 1 and stats['windows'] < -(-len(long) // 512)
    # with room for the line the file is taken, the tail growing over the windows in between
    fake.calls.clear()
    verdict, rows, stats = HostDedup().cdx_append_file(str(path), 'part', 512, 8192)
    assert (verdict, rows) == (_native.KW_CDX_OK, 3) and 0 in stats['consumed'] and stats['tail_max'] > 4096
    # a window the parser refuses ends the stream with its verdict
    fake = FakeLib(refuse_at=1)
    monkeypatch.setattr(_native, 'lib', lambda: fake)
    path.write_bytes(_links_text(60).encode())
    verdict, rows, stats = HostDedup().cdx_append_file(str(path), 'part', 256, 1024)
    assert (verdict, rows, stats['windows']) == (_native.KW_CDX_FIELDS, 0, 2)


def test_reader_error_is_raised_after_the_join(tmp_path, monkeypatch):
    path = tmp_path / 'links.csv'
    path.write_bytes(_links_text(200).encode())
    fake = FakeLib()
    monkeypatch.setattr(_native, 'lib', lambda: fake)
    real = os.preadv
    seen = []

    def shrunk(fd, bufs, offset):
        seen.append(offset)
        return 0 if offset >= 1024 else real(fd, bufs, offset)
    monkeypatch.setattr(os, 'preadv', shrunk)
    import threading
    before = threading.active_count()
    with pytest.raises(OSError, match='shrank'):
        HostDedup().cdx_append_file(str(path), 'part', 512, 1024)
    assert threading.active_count() == before and max(seen) >= 1024


# ------------------------------------------------------------------ the routing by stream_from
class Router:
    """Stands in for the dedup handle: notes which call each file took."""

    def __init__(self):
        self.calls = []

    def cdx_begin(self):
        self.calls.append('begin')

    def csv_append(self, data, header, col):
        self.calls.append(('csv', len(data), header, col))
        return _native.KW_CSV_OK, -1, 3

    def cdx_append(self, data, dialect):
        self.calls.append(('cdx', len(data), dialect))
        return _native.KW_CDX_OK, -1, 2

    def csv_append_file(self, path, header, col, window, max_record):
        self.calls.append(('csv_file', os.path.basename(path), header, col, window, max_record))
        return _native.KW_CSV_OK, 3, {'windows': 4}

    def cdx_append_file(self, path, dialect, window, max_record):
        self.calls.append(('cdx_file', os.path.basename(path), dialect, window, max_record))
        return _native.KW_CDX_OK, 2, {'windows': 5}

    def run_exclude(self, n):
        return 2, 1, 1

    def remaining(self):
        return np.frombuffer(b'a:b', dtype=np.uint8), np.array([0, 3]), np.array([0])


def test_links_load_routes_by_size(tmp_path, monkeypatch):
    ex, ln = tmp_path / 'ex.csv', tmp_path / 'ln.csv'
    ex.write_bytes(b'x,url\r\n1,http://a\r\n' * 1 + b'2,http://b\r\n' * 10)
    ln.write_bytes(_links_text(3).encode())
    r = Router()
    monkeypatch.setattr(cdx_dedup, '_dedup', lambda: r)
    n_ex, n_ln = os.path.getsize(ex), os.path.getsize(ln)
    assert links.STREAM_FROM >= 2 * links.WINDOW_BYTES and links.WINDOW_BYTES == 256 << 20
    assert links._load(str(ex), str(ln))[1:] == (3, 2, (0, 0))                # the defaults: one piece
    assert r.calls == ['begin', ('csv', n_ex, 'x,url', 1), ('cdx', n_ln, 'part')]
    r.calls.clear()
    assert links._load(str(ex), str(ln), stream_from=0, window_bytes=64, max_record_bytes=32)[1:] == (3, 2, (4, 5))
    assert r.calls == ['begin', ('csv_file', 'ex.csv', 'x,url', 1, 64, 32), ('cdx_file', 'ln.csv', 'part', 64, 32)]
    r.calls.clear()
    # the threshold is the file's size: at it streamed, one byte above it not
    assert links._load(str(ex), str(ln), stream_from=n_ex, window_bytes=64, max_record_bytes=32)[3] == (4, 0)
    assert links._load(str(ex), str(ln), stream_from=n_ex + 1, window_bytes=64, max_record_bytes=32)[3] == (0, 0)
    # an empty or missing file, a header without one url column: not eligible on either route
    assert links._load(str(tmp_path / 'none.csv'), str(ln), stream_from=0) is None
    (tmp_path / 'empty.csv').write_bytes(b'')
    assert links._load(str(tmp_path / 'empty.csv'), str(ln), stream_from=0) is None
    (tmp_path / 'nourl.csv').write_bytes(b'a,b\n1,2\n')
    assert links._load(str(tmp_path / 'nourl.csv'), str(ln), stream_from=0) is None


def test_resume_routes_by_size(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'yfin_urls.csv').write_bytes(_links_text(3).encode())
    (tmp_path / 'success_articles_yfin.csv').write_bytes(b','.join(f.encode() for f in resume.SUCCESS_FIELDS) + b'\n')
    r = Router()
    monkeypatch.setattr(cdx_dedup, '_dedup', lambda: r)
    res = resume.remaining_urls()
    assert res.route == 'device' and res.windows == (0, 0, 0) and [c[0] for c in r.calls[1:]] == ['csv', 'csv']
    r.calls.clear()
    res = resume.remaining_urls(stream_from=0, window_bytes=128, max_record_bytes=64)
    assert res.route == 'device' and res.windows == (4, 0, 4)
    assert r.calls[1:] == [('csv_file', 'success_articles_yfin.csv', ','.join(resume.SUCCESS_FIELDS), 0, 128, 64),
                           ('csv_file', 'yfin_urls.csv', 'date_time,url', 1, 128, 64)]
    monkeypatch.setenv('KW_RESUME_NATIVE', '0')
    (tmp_path / 'success_articles_yfin.csv').write_bytes(
        b','.join(f.encode() for f in resume.SUCCESS_FIELDS) + b'\nhttp://h/,,,,,,,\n')
    res = resume.remaining_urls(stream_from=0)
    assert res.route == 'pandas' and res.windows == (0, 0, 0) and res.remaining == 2


# ------------------------------------------------------------------ find_new_urls, the pandas route against the reference
@pytest.mark.parametrize('case', ['plain', 'articles', 'missing_column', 'unreadable'])
def test_find_new_urls_pandas_route_against_the_golden(tmp_path, monkeypatch, capsys, case):
    with open(GOLDEN, encoding='utf-8') as fh:
        g = json.load(fh)
    new, old, out = g['names']
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('KW_LINKS_NATIVE', '0')
    for name, text in g['cases'][case]['inputs'].items():
        if text is not None:
            with open(name, 'w', encoding='utf-8', newline='') as fh:
                fh.write(text)
    res = links.find_new_urls(new, old, out)
    assert capsys.readouterr().out == g['cases'][case]['stdout']
    want = g['cases'][case]['output']
    if want is None:
        assert res is None and not os.path.exists(out)
        return
    with open(out, encoding='utf-8', newline='') as fh:
        assert fh.read() == want
    lines = g['cases'][case]['stdout'].splitlines()
    assert (res.route, res.windows) == ('pandas', (0, 0))
    assert [res.unique_new, res.unique_old, res.unique_only_new] == [int(ln.rsplit(' ', 1)[1]) for ln in lines[1:4]]
    assert res.written == len(want.splitlines()) - 1 and len({res.unique_new, res.unique_old, res.n_links}) == 3
