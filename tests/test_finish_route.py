"""Host: egress.RunFiles.finish keeps its host branch -- the rewrite of a file this run wrote, from the write index
alone -- when the device route (sortfiles.DeviceSorter.sort_indexed) is switched off, and when no device answers:
the bytes are the written records in ``np.argsort(time_unix, kind='quicksort')`` order behind the file's own
header, built here in numpy; the native library is not loaded for it; the signature and the return values stand."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS_OK = 0xFF            # a text witness in every column: the block rule passes


def build(tmp_path, stamps, name='T_match.csv', seed=1):
    """A hand-built owned file: one line a stamp, of varying length, some with a quoted line end inside; the
    RunFiles that indexed it in two appends, the file's bytes and the lines."""
    from advanced_scrapper_amd import egress
    rng = np.random.default_rng(seed)
    header = egress.header_bytes()
    lines = []
    for i, t in enumerate(stamps):
        pad = 'x' * int(rng.integers(0, 40))
        cell = f'"a {i}\nb {pad}"' if i % 3 == 0 else f'a {i} {pad}'
        lines.append(f'{int(t)},2020-01-01,{{}},{{}},t{i},u,s,su,{cell}\n'.encode())
    run = egress.RunFiles(str(tmp_path))
    (tmp_path / name).write_bytes(header + b''.join(lines))
    cut = len(lines) // 2
    for a, b in ((0, cut), (cut, len(lines))):
        if b > a:
            run.add(name, np.asarray(stamps[a:b], dtype=np.int64), np.asarray([len(x) for x in lines[a:b]], dtype=np.int64),
                    np.full(b - a, FLAGS_OK, dtype=np.uint32), header)
    return run, header, lines


def expected(header, lines, stamps):
    order = np.argsort(np.asarray(stamps, dtype=np.int64), kind='quicksort')
    body = np.frombuffer(b''.join(lines), dtype=np.uint8)
    ends = np.cumsum([len(x) for x in lines])
    starts = ends - [len(x) for x in lines]
    return header + b''.join(body[starts[r]:ends[r]].tobytes() for r in order.tolist())


def shuffled(n, seed=7):
    rng = np.random.default_rng(seed)
    stamps = 1_600_000_000 + rng.permutation(n) * 60
    stamps[::5] = stamps[0]          # ties: numpy's order among them
    return stamps.astype(np.int64)


@pytest.mark.parametrize('how', ('switch', 'no-device'))
def test_host_branch_rewrites_as_before(tmp_path, monkeypatch, how):
    from advanced_scrapper_amd import sortfiles
    if how == 'switch':
        monkeypatch.setenv('KW_FINISH_DEVICE', '0')
        monkeypatch.setattr(sortfiles, 'available', lambda: pytest.fail('the device was asked for'))
    else:
        monkeypatch.delenv('KW_FINISH_DEVICE', raising=False)
        monkeypatch.setattr(sortfiles, '_SORTER', None)
        monkeypatch.setattr(sortfiles, 'available', lambda: False)
    stamps = shuffled(257)
    run, header, lines = build(tmp_path, stamps)
    sortfiles.reset_stats()
    assert run.finish('T_match.csv') is True
    assert (tmp_path / 'T_match.csv').read_bytes() == expected(header, lines, stamps)
    assert sortfiles.LAST_STATS['index_host'] == 1 and sortfiles.LAST_STATS['indexed'] == 0
    assert os.listdir(tmp_path) == ['T_match.csv']


def test_signature_and_return_values(tmp_path, monkeypatch):
    from advanced_scrapper_amd import egress
    monkeypatch.setenv('KW_FINISH_DEVICE', '0')
    assert list(inspect.signature(egress.RunFiles.finish).parameters) == ['self', 'name']
    # in order: True, and the file is not opened
    stamps = np.arange(10, dtype=np.int64) * 3
    run, header, lines = build(tmp_path, stamps)
    path = tmp_path / 'T_match.csv'
    old = 1_500_000_000_000_000_000
    os.utime(path, ns=(old, old))
    before = os.stat(path)
    with monkeypatch.context() as m:
        m.setattr(egress, 'open', lambda *a, **k: pytest.fail('the file was opened'), raising=False)
        assert run.finish('T_match.csv') is True
    after = os.stat(path)
    assert (after.st_mtime_ns, after.st_ino) == (old, before.st_ino)
    # a name the run does not own, one it never indexed, a size the index does not describe, a lone '\r'
    assert run.finish('other.csv') is False
    run.note_other('T_match.csv')
    assert run.finish('T_match.csv') is False
    run, header, lines = build(tmp_path, shuffled(20), name='S_match.csv')
    with open(tmp_path / 'S_match.csv', 'ab') as fh:
        fh.write(b'x')
    data = (tmp_path / 'S_match.csv').read_bytes()
    assert run.finish('S_match.csv') is False and (tmp_path / 'S_match.csv').read_bytes() == data
    run, header, lines = build(tmp_path, shuffled(20), name='C_match.csv')
    run.files['C_match.csv'][0][0][3][1] |= egress._F_CR
    assert run.finish('C_match.csv') is False
    # a plan changes nothing on the host branch
    stamps = shuffled(33)
    run, header, lines = build(tmp_path, stamps, name='P_match.csv')
    run.plan(['P_match.csv', 'nothing.csv'])
    assert run.finish('P_match.csv') is True and run.finish('nothing.csv') is False
    assert (tmp_path / 'P_match.csv').read_bytes() == expected(header, lines, stamps)


def test_host_branch_loads_no_native_library(tmp_path):
    """In a fresh process: the switched-off route rewrites the file without libkwmatch being loaded."""
    code = (
        "import os, sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from tests.test_finish_route import build, expected, shuffled\n"
        "import pathlib\n"
        "tmp = pathlib.Path(%r)\n"
        "stamps = shuffled(64)\n"
        "run, header, lines = build(tmp, stamps)\n"
        "assert run.finish('T_match.csv') is True\n"
        "assert (tmp / 'T_match.csv').read_bytes() == expected(header, lines, stamps)\n"
        "from advanced_scrapper_amd import _native\n"
        "assert _native._LIB is None, 'libkwmatch was loaded'\n"
        "assert not any('libkwmatch' in line for line in open('/proc/self/maps'))\n"
        "print('ok')\n" % (REPO, str(tmp_path)))
    env = dict(os.environ, KW_FINISH_DEVICE='0')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=REPO)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr
