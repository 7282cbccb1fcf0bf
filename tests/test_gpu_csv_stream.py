"""GPU: the windowed CSV append (kw_csv_stream_* in csrc/cdx.hip, GpuUrlDedup.csv_append_file).

Bar: bit-exact.  A text cut into windows at any sizes gives the rows of ``kw_csv_append`` over the whole text (arena
bytes, offsets, timestamps), every window's ``consumed`` is the rule's (tests/csv_window_rule.py, which
tests/test_csv_window_rule.py holds against the whole-text rule on the CPU), a text with one violation gets the
whole-text call's code and file position whichever window it falls into, and a refused or abandoned stream leaves the
store as ``begin`` found it.
"""
import numpy as np
import pytest

from tests import csv_window_rule as W
from tests import resume_rule as R

pytestmark = pytest.mark.gpu
FH, FC = R.FILES['failed']
SH, SC = R.FILES['success']


@pytest.fixture(scope='module')
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.cdx_dedup import GpuUrlDedup
    return GpuUrlDedup()


@pytest.fixture(scope='module')
def T(gpu):
    return gpu.cdx_tile_bytes()


def _rows(gpu):
    arena, off, ts = gpu.cdx_rows()
    return arena, off.tolist(), ts.tolist()


def _whole(gpu, texts):
    """The store after the one-piece call over each (text, header, column)."""
    gpu.cdx_begin()
    for text, header, col in texts:
        v, pos, cells = R.parse(text, header, col)
        assert gpu.csv_append(text, header.decode(), col) == (v, pos, len(cells) if v == R.OK else 0)
    return _rows(gpu)


def _file(tmp_path, text, name='f.csv'):
    path = tmp_path / name
    path.write_bytes(text)
    return str(path)


def _stream_file(gpu, tmp_path, text, header, col, window, max_record=1 << 20):
    """One file through csv_append_file: the verdict, position and rows are the whole-text rule's, every consumed
    the window rule's, the device times finite."""
    want = W.stream(text, header, col, window, max_record)
    verdict, rows, stats = gpu.csv_append_file(_file(tmp_path, text), header.decode(), col, window, max_record)
    if want[0] == W.RECORD:
        assert (verdict, rows, stats['refusal']) == (None, 0, 'record')
        return stats
    assert (verdict, stats['bad_pos'], rows) == (want[0], want[1], len(want[2]) if want[0] == R.OK else 0), (window, stats)
    assert stats['consumed'] == want[3][:len(stats['consumed'])] and stats['refusal'] is None
    if verdict == R.OK:
        assert stats['consumed'] == want[3] and stats['windows'] == max(1, -(-len(text) // window))
    assert stats['device_text_bytes'] <= 2 * (window + max_record + 256)
    assert np.isfinite(gpu.cdx_last_ms()).all()
    return stats


# ------------------------------------------------------------------ 1. the cut sweep
@pytest.mark.parametrize('place', sorted(W.EDGE_PLACES))
def test_cut_sweep(gpu, tmp_path, place):
    text, at = W.edge_text(W.EDGE_PLACES[place])
    want = _whole(gpu, [(text, SH, SC)])
    for window in W.sweep_windows(at):
        gpu.cdx_begin()
        _stream_file(gpu, tmp_path, text, SH, SC, window)
        assert _rows(gpu) == want, (place, window)


# ------------------------------------------------------------------ 2. sizes
@pytest.mark.parametrize('grid', [None, 1, 2])
@pytest.mark.parametrize('kind', ['success', 'failed', 'links'])
def test_window_sizes_over_clean_texts(gpu, T, tmp_path, monkeypatch, kind, grid):
    """Windows of 1 tile, 1 tile + 16 and 3 tiles - 1; with the launch grids capped (KW_TEST_CSV_GRID) every tile
    kernel's loop takes several trips."""
    if grid is not None:
        monkeypatch.setenv('KW_TEST_HOOKS', '1')
        monkeypatch.setenv('KW_TEST_CSV_GRID', str(grid))
    header, col = R.FILES[kind]
    for seed in range(6 if grid is None else 3):
        text = R.fuzz_clean(seed, kind)
        want = _whole(gpu, [(text, header, col)])
        for window in (T, T + 16, 3 * T - 1):
            gpu.cdx_begin()
            _stream_file(gpu, tmp_path, text, header, col, window)
            assert _rows(gpu) == want, (kind, seed, window)


def _long_record(T):
    """A record of more than three tiles between two short ones."""
    return b'url,error\r\nhttp://a/1,e\r\nhttp://a/2,"' + b'x,\n' * (T + 100) + b'"\r\nhttp://a/3,e\r\n'


def test_special_shapes(gpu, T, tmp_path):
    cases = [(b'url,error\nhttp://a/1,e\nhttp://a/2,e\n', 1 << 16),      # one window, final at once
             (b'url,error\nhttp://a/1,e\nhttp://a/2,e', T),              # the last record has no terminator
             (b'url,error\r\n' + b'http://a/1,e\r\n' * 700 + b'http://a/2,"no end\n"', T),
             (b'url,error\nhttp://a/1,e\n', 4),                           # the first window ends inside the header line
             (b'url,error\r\nhttp://a/1,e\n', 10),                        # ... between the header's '\r' and '\n'
             (_long_record(T), T)]                                        # a record no single window holds
    for text, window in cases:
        want = _whole(gpu, [(text, FH, FC)])
        gpu.cdx_begin()
        stats = _stream_file(gpu, tmp_path, text, FH, FC, window, 4 * T)
        assert _rows(gpu) == want
    # the long record's tail grows over three windows, then is taken
    assert stats['consumed'][:3] == [25, 0, 0] and stats['consumed'][3] > 3 * T and stats['tail_max'] > 2 * T


def test_record_refusal_puts_the_store_back(gpu, T, tmp_path):
    before = _whole(gpu, [(R.fuzz_clean(1, 'failed'), FH, FC)])
    stats = _stream_file(gpu, tmp_path, _long_record(T), FH, FC, T, 2 * T)
    assert stats['refusal'] == 'record' and stats['windows'] == 3
    assert _rows(gpu) == before
    # an empty stream, and a file without rows
    assert _stream_file(gpu, tmp_path, b'url,error\n\n', FH, FC, 4)['refusal'] is None
    assert _rows(gpu) == before


# ------------------------------------------------------------------ 3. violations
def _raw_stream(gpu, text, header, col, window):
    """The text through kw_csv_stream_window itself, cut as the rule cuts it: the rule's result with the kernels as
    the judge, the window that refused, and what ``end`` answered."""
    state = {'pos': 0, 'k': -1}

    def judge(w, first, final):
        state['k'] += 1
        verdict, bad, rows, used = gpu.csv_stream_window(w, final)
        state['pos'] += used
        return verdict, (bad - (state['pos'] - used) if verdict != R.OK else -1), [None] * rows, used
    gpu.csv_stream_begin(header.decode(), col)
    got = W.stream(text, header, col, window, judge_window=judge)
    return got, state['k'], gpu.csv_stream_end(True)


@pytest.mark.parametrize('what', R.VIOLATIONS)
def test_violation_in_each_window(gpu, T, what):
    earlier = R.fuzz_clean(3, 'success')
    clean = b'url,error\n' + W.filler(2 * T, 5000)
    texts = W.violation_texts(what, T)
    for place, text in texts.items():
        want = R.parse(text, FH, FC)
        assert want[0] == R.EXPECT[what] and W.stream(text, FH, FC, T)[:3] == want, (what, place)
        before = _whole(gpu, [(earlier, SH, SC)])
        # the whole-text call's answer (nothing appended unless OK), then the stream's
        assert gpu.csv_append(text, FH.decode(), FC)[:2] == want[:2]
        gpu.cdx_begin()
        assert gpu.csv_append(earlier, SH.decode(), SC)[0] == R.OK
        got, k, end = _raw_stream(gpu, text, FH, FC, T)
        n_win = max(1, -(-len(text) // T))
        if want[0] == R.OK:
            assert got[0] == R.OK and end == (R.OK, len(want[2]))
            assert _rows(gpu) == _whole(gpu, [(earlier, SH, SC), (text, FH, FC)])
            continue
        assert got[:2] == want[:2], (what, place, R.NAMES[want[0]])
        assert end == ((R.ROWS, 0) if want[0] == R.ROWS else (R.OK, 0))
        if what in ('nul', 'utf8', 'lonecr', 'fewer', 'more', 'oddurl', 'quotedurl'):
            # (a quote violation shifts the parity behind it: the window that sees it complete may be a later one)
            assert n_win >= 4
            assert {'first': k == 0, 'middle': 0 < k < n_win - 1, 'last': k == n_win - 1}[place], (what, place, k)
        assert _rows(gpu) == before
        # a second stream on the same handle
        got, _, end = _raw_stream(gpu, clean, FH, FC, T)
        assert got[0] == R.OK and end[0] == R.OK
        assert _rows(gpu) == _whole(gpu, [(earlier, SH, SC), (clean, FH, FC)])


def test_stream_states(gpu):
    from advanced_scrapper_amd import _native
    gpu.cdx_begin()
    gpu.csv_stream_begin('url,error', 0)
    with pytest.raises(_native.KwError):
        gpu.csv_stream_begin('url,error', 0)
    with pytest.raises(_native.KwError):
        gpu.csv_append(b'url,error\na:b,c\n', 'url,error', 0)
    assert gpu.csv_stream_window(b'url,error\na:b,c\nd:e', False) == (R.OK, -1, 1, 16)
    assert gpu.csv_stream_end(False) == (R.OK, 0)          # abandoned: nothing stays
    assert _rows(gpu)[1:] == ([0], [])
    with pytest.raises(_native.KwError):
        gpu.csv_stream_window(b'url,error\n', True)        # no open stream
    gpu.csv_stream_begin('url,error', 0)
    assert gpu.csv_stream_window(b'url,error\na:b,c\n', False)[0] == R.OK
    with pytest.raises(_native.KwError):
        gpu.csv_stream_end(True)                           # commit before a final window
    assert _rows(gpu)[1:] == ([0], [])


# ------------------------------------------------------------------ 4. reuse
def test_two_streamed_files_then_exclude(gpu, T, tmp_path):
    success = R.fuzz_clean(5, 'success')
    failed = b'url,error\r\n' + W.filler(2 * T + 100, 0)
    links = 'date_time,url\n' + ''.join('%d,%s\n' % (20240101000000 + k, u) for k, u in enumerate(
        ['http://fill/%d' % k for k in range(0, 120, 3)] + ['https://finance.yahoo.com/news/a-1.html', 'http://new/1'] * 2))
    gpu.cdx_begin()
    n_s = gpu.csv_append(success, SH.decode(), SC)[2]
    n_f = gpu.csv_append(failed, FH.decode(), FC)[2]
    assert gpu.cdx_append(links.encode(), 'part')[0] == 0
    want_counts, want_codes, want_rows = gpu.run_exclude(n_s + n_f), gpu.exclude_codes().tolist(), _rows(gpu)
    gpu.cdx_begin()
    v1, r1, _ = gpu.csv_append_file(_file(tmp_path, success, 's.csv'), SH.decode(), SC, T + 16, 4 * T)
    v2, r2, s2 = gpu.csv_append_file(_file(tmp_path, failed, 'f.csv'), FH.decode(), FC, T, 4 * T)
    v3, r3, s3 = gpu.cdx_append_file(_file(tmp_path, links.encode(), 'l.csv'), 'part', 512, 4 * T)
    assert (v1, r1, v2, r2, v3) == (R.OK, n_s, R.OK, n_f, 0) and s2['windows'] >= 3 and s3['windows'] >= 3
    assert _rows(gpu) == want_rows
    assert gpu.run_exclude(n_s + n_f) == want_counts and gpu.exclude_codes().tolist() == want_codes
    assert 0 < want_counts[1] < want_counts[0]
