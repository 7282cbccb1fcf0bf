"""CPU tests of the extended regex programs: the host walk (kb.regex_program), the stream's validation in
kw_compile, and the host position fallback (matcher.resolve_host_positions)."""
import ctypes
import random
import re

import numpy as np
import pytest

from advanced_scrapper_amd import _native, kb
from advanced_scrapper_amd.kb import compile_kb
from advanced_scrapper_amd.matcher import resolve_host_positions

# name -> (document, positions the CPU oracle reports for the decided name)
TABLE = {
    '[24]7.ai': ('call [24]7.ai now: 27.ai, 47xai and 24]7.ai; 2\n.ai no', [19, 26]),
    'A|X Armani Exchange': ('A|X Armani Exchange opened; A was here, X Armani too', [0, 2, 28, 42]),
    'Ke$ha Holdings': ('Ke$ha Holdings fell', []),
    '^Top Shop': ('Top Shop ^Top Shop', [0]),
    'Macy\\s': ('Macy\\s sale at Macy s and Macy\xa0x, Macy\n', [15, 26, 34]),
    'x-Fab*?rik': ('x-Fab*?rik x-Farik x-Fabbbrik x-Fabrik', [11, 19, 30]),
    '\\bFoo\\b Inc': ('\\bFoo\\b Inc vs Foo Inc vs XFoo Inc', [15]),
    '[^a-c]xon Mobil': ('[^a-c]xon Mobil Exxon Mobil axon Mobil éxon Mobil', [5, 17, 39]),
    '\\d+ Capital': ('\\d+ Capital 42 Capital ٣٤ Capital x Capital', [12, 23]),
    'Toys.R.Us|Toys R Us': ('Toys.R.Us|Toys R Us: ToysXRXUs, Toys R Us', [0, 10, 21, 32]),
    'Joe (Jr)?': ('Joe (Jr)? Joe Jr Joe ', [0, 10, 17]),
    'a?': ('a? banana', list(range(10))),
}
HOST_NAMES = {'Joe (Jr)?', 'a?'}
# names where the arm order or laziness moves the match END (and so the later positions)
ORDER_NAMES = ['Toy|Toys R Us', 'Toys R Us|Toy', 'ab*?b', 'ab*b', 'a.+?b|a.+c', 'x[ab]{1,3}?a', 'x[ab]{1,3}a', '(ab|a)b?c',
               'a+(b|ab)c', 'b.*(cd|c)d', '\\w+?\\W\\S', 'a\\Bb|a\\b', 'q$|q\\Z|^q.', '[^\\d\\s]+1', 'ab??b']


def _processed(names):
    return {'TK': {'name': {n: (None, None) for n in names}}}


def test_compile_kb_takes_every_reference_regex():
    """The test that fails without the feature: compile_kb raised UnsupportedPattern for these names."""
    ckb = compile_kb(_processed(TABLE))
    assert sorted(ckb.names) == sorted(TABLE)
    assert {n for n, h in zip(ckb.names, ckb.host_regex) if h} == HOST_NAMES
    assert not any(ckb.invalid_regex)
    for i, n in enumerate(ckb.names):
        rows = ckb.rx_atoms[ckb.rx_off[i]:ckb.rx_off[i + 1]].tolist()
        if n in HOST_NAMES:
            assert rows == [[kb.RX_NOPOS, 0, 0, 0]]
        else:
            assert [tuple(r) for r in rows] == kb.regex_program(n)
    # the old contract stays (tests/test_host.py pins it too)
    with pytest.raises(kb.UnsupportedPattern):
        kb.regex_atoms('[24]7.ai')


def test_program_shapes():
    P = kb.regex_program
    assert P('[24]7.ai')[:3] == [(kb.RX_SET, 2, 1, 1), (kb.RX_RANGE, 50, 50, 0), (kb.RX_RANGE, 52, 52, 0)]
    assert P('Ke$ha')[2] == (kb.RX_AT, kb.AT_EOL, 0, 0)
    assert P('x*?y')[0] == (kb.RX_LIT | kb.RX_LAZY, ord('x'), 0, -1)
    assert P('x{2}?y')[0] == (kb.RX_LIT, ord('x'), 2, 2)            # nothing lazy about a fixed count
    assert P('Toy|Toys') == [(0, 84, 1, 1), (0, 111, 1, 1), (0, 121, 1, 1), (kb.RX_ALT, 2, 3, 0),
                             (kb.RX_ARM, 0, 3, 0), (kb.RX_ARM, 1, 2, 0), (0, 115, 1, 1)]
    assert P('[^a]b')[0][:2] == (kb.RX_SET, 2) and P('[^a]b')[1:3] == [(kb.RX_RANGE, 0, 96, 0), (kb.RX_RANGE, 98, 0x10FFFF, 0)]
    assert P('C++') == 'invalid' and P('(?<=a+)b') == 'invalid'
    wide = '[' + ''.join(chr(0x4E00 + 2 * i) for i in range(kb.RX_MAX_RANGES + 1)) + ']x'   # too many ranges
    for host in ('Joe (Jr)?', 'a?', '(a|(bx|cy)d)e', '(a)\\1', 'a(?=b)', '(?i)abc', 'a|', wide, 'a?' * 17 + 'b',
                 '(ab|b)+c'):
        assert P(host) == kb.RX_HOST, host
    d = P('\\d7')
    assert d[0] == (kb.RX_SET, len(d) - 2, 1, 1) and (kb.RX_RANGE, 48, 57, 0) in d and (kb.RX_RANGE, 0x663, 0x669, 0) not in d
    assert any(lo <= 0x663 <= hi for _o, lo, hi, _z in d[1:-1])


# ------------------------------------------------------------------ the engine's mirror
def _cp_ok(rows, a, c):
    op, val = rows[a][0] & 0xFF, rows[a][1]
    if op == kb.RX_LIT:
        return ord(c) == val
    if op == kb.RX_ANY:
        return c != '\n'
    return any(lo <= ord(c) <= hi for _o, lo, hi, _z in rows[a + 1:a + 1 + val])


def _nrows(row):
    return 1 + row[1] if row[0] & 0xFF == kb.RX_SET else 1


def _is_word(c):
    return c.isalnum() or c == '_'


def _at_ok(kind, s, pos):
    n = len(s)
    if kind == kb.AT_BOS:
        return pos == 0
    if kind == kb.AT_EOS:
        return pos == n
    if kind == kb.AT_EOL:
        return pos == n or (pos == n - 1 and s[pos] == '\n')
    before = pos > 0 and _is_word(s[pos - 1])
    after = pos < n and _is_word(s[pos])
    return (before != after) == (kind == kb.AT_WORD)


def _program_finditer(rows, s):
    """Python mirror of the device engine (kwmatch_kernels.hpp rx_match + rx_positions): one stack of frames,
    (row, start, count) for a repeat and (ARM row, start, -) for a branch."""
    n = len(s)

    def match_at(st):
        stack = []
        a, pos = 0, st
        while True:
            if a == len(rows):
                return pos
            op, val, lo, hi = rows[a]
            lazy, op = op & kb.RX_LAZY, op & 0xFF
            if op <= kb.RX_SET and lo == 1 and hi == 1:
                if pos < n and _cp_ok(rows, a, s[pos]):
                    pos += 1
                    a += _nrows(rows[a])
                    continue
            elif op <= kb.RX_SET:
                want = lo if lazy else hi
                k = 0
                while (want < 0 or k < want) and pos + k < n and _cp_ok(rows, a, s[pos + k]):
                    k += 1
                if k >= lo:
                    assert len(stack) < kb.RX_MAX_FRAMES
                    stack.append([a, pos, k])
                    pos += k
                    a += _nrows(rows[a])
                    continue
            elif op == kb.RX_AT:
                if _at_ok(val, s, pos):
                    a += 1
                    continue
            elif op == kb.RX_ALT:
                assert len(stack) < kb.RX_MAX_FRAMES
                stack.append([a + 1, pos, 0])
                a += 2
                continue
            elif op == kb.RX_ARM:
                a += lo
                continue
            else:
                return -1
            while stack:                      # backtrack
                t = stack[-1]
                q = rows[t[0]]
                if q[0] & 0xFF == kb.RX_ARM:
                    nxt = t[0] + 1 + q[1]
                    if nxt != t[0] + q[2]:
                        t[0] = nxt
                        a, pos = nxt + 1, t[1]
                        break
                elif q[0] & kb.RX_LAZY:
                    p = t[1] + t[2]
                    if (q[3] < 0 or t[2] < q[3]) and p < n and _cp_ok(rows, t[0], s[p]):
                        t[2] += 1
                        a, pos = t[0] + _nrows(q), p + 1
                        break
                elif t[2] > q[2]:
                    t[2] -= 1
                    a, pos = t[0] + _nrows(q), t[1] + t[2]
                    break
                stack.pop()
            else:
                return -1

    out, last = [], 0
    for st in range(n):
        e = match_at(st)
        if e >= 0 and st >= last:
            out.append(st)
            last = e if e > st else st + 1
    return out


def test_table_documents():
    for name, (doc, want) in TABLE.items():
        assert [m.start() for m in re.finditer(name, doc)] == want, name
        if name not in HOST_NAMES:
            assert _program_finditer(kb.regex_program(name), doc) == want, name
    rows = kb.regex_program('^Top Shop')
    assert _program_finditer(rows, '^Top Shop and Top Shop') == []
    assert _program_finditer(kb.regex_program('Toy|Toys R Us'), 'Toys R Us Toys R Us') == [0, 10]
    assert _program_finditer(kb.regex_program('Toys R Us|Toy'), 'Toys R Us Toys R Us') == [0, 10]
    assert _program_finditer(kb.regex_program('ab*?b'), 'abbb abbb') == [0, 5]
    assert _program_finditer(kb.regex_program('ab*?b'), 'abbab') == [0, 3]


def test_engine_mirror_equals_re():
    rng = random.Random(5)
    names = [n for n in TABLE if n not in HOST_NAMES] + ORDER_NAMES
    for name in names:
        rows = kb.regex_program(name)
        assert isinstance(rows, list), name
        alphabet = sorted(set(re.sub(r'\\[a-zA-Z]', '', name))) + ['\n', 'é', '7', ' ', 'a', 'b']
        plain = re.sub(r'[\\^$()|?*+\[\]{}]', '', name)
        for _ in range(40):
            s = ''.join(rng.choice(alphabet) for _ in range(rng.randint(0, 30)))
            if rng.random() < 0.5:
                s = s[:5] + plain + s[5:]
            want = [m.start() for m in re.finditer(name, s)]
            assert _program_finditer(rows, s) == want, (name, s)


def test_old_subset_is_unchanged(golden):
    from advanced_scrapper_amd.synth_kb import synthetic_kb
    for processed in (golden.kb_processed(), synthetic_kb(600, 11)):
        ckb = compile_kb(processed, workers=1)
        assert not any(ckb.host_regex)
        for n, c in zip(ckb.names, ckb.classes):
            if c == 'F':
                assert kb.regex_program(n) == kb.regex_atoms(n), n


# ------------------------------------------------------------------ kw_compile's validation
def _kw_compile_rc(rows):
    L = _native.lib()
    name = b'Some Name'
    b = np.frombuffer(name, dtype=np.uint8).copy()
    off = np.array([0, len(b)], dtype=np.int64)
    cls = np.array([ord('F')], dtype=np.uint8)
    rx = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
    rxo = np.array([0, len(rx)], dtype=np.int64)
    h = ctypes.c_void_p()
    rc = L.kw_compile(_native.ptr(b), _native.ptr(off), _native.ptr(cls), 1, _native.ptr(rx), _native.ptr(rxo),
                      _native.ptr(kb.word_bitmap()), None, 0, 0, ctypes.byref(h))
    msg = L.kw_last_error(h) or b''
    if h.value:
        L.kw_destroy(h)
    return rc, msg


LIT = (kb.RX_LIT, 97, 1, 1)
MALFORMED = {
    'range without its set': [LIT, (kb.RX_RANGE, 48, 57, 0)],
    'set short of its rows': [(kb.RX_SET, 2, 1, 1), (kb.RX_RANGE, 48, 57, 0)],
    'lo > hi': [(kb.RX_SET, 1, 1, 1), (kb.RX_RANGE, 57, 48, 0)],
    'unsorted rows': [(kb.RX_SET, 2, 1, 1), (kb.RX_RANGE, 60, 70, 0), (kb.RX_RANGE, 48, 57, 0)],
    'overlapping rows': [(kb.RX_SET, 2, 1, 1), (kb.RX_RANGE, 48, 57, 0), (kb.RX_RANGE, 57, 60, 0)],
    'range past 0x10FFFF': [(kb.RX_SET, 1, 1, 1), (kb.RX_RANGE, 48, 0x110000, 0)],
    'arm count too large': [LIT, (kb.RX_ALT, 3, 4, 0), (kb.RX_ARM, 1, 4, 0), LIT, (kb.RX_ARM, 1, 2, 0), LIT],
    'arm rows past the branch': [LIT, (kb.RX_ALT, 2, 4, 0), (kb.RX_ARM, 1, 4, 0), LIT, (kb.RX_ARM, 2, 2, 0), LIT],
    'arm distance wrong': [LIT, (kb.RX_ALT, 2, 4, 0), (kb.RX_ARM, 1, 3, 0), LIT, (kb.RX_ARM, 1, 2, 0), LIT],
    'branch rows wrong': [LIT, (kb.RX_ALT, 2, 5, 0), (kb.RX_ARM, 1, 4, 0), LIT, (kb.RX_ARM, 1, 2, 0), LIT],
    'one arm': [LIT, (kb.RX_ALT, 1, 2, 0), (kb.RX_ARM, 1, 2, 0), LIT],
    'arm without its branch': [LIT, (kb.RX_ARM, 1, 2, 0), LIT],
    'nested branch': [LIT, (kb.RX_ALT, 2, 7, 0), (kb.RX_ARM, 4, 7, 0), (kb.RX_ALT, 2, 2, 0), (kb.RX_ARM, 0, 2, 0),
                      (kb.RX_ARM, 0, 1, 0), (kb.RX_ARM, 1, 2, 0), LIT],
    'unknown assertion': [LIT, (kb.RX_AT, 5, 0, 0)],
    'negative assertion': [LIT, (kb.RX_AT, -1, 0, 0)],
    'nopos with other atoms': [LIT, (kb.RX_NOPOS, 0, 0, 0)],
    'two nopos': [(kb.RX_NOPOS, 0, 0, 0), (kb.RX_NOPOS, 0, 0, 0)],
    'unknown op': [LIT, (8, 0, 1, 1)],
    'lazy fixed count': [(kb.RX_LIT | kb.RX_LAZY, 97, 2, 2), LIT],
    'lazy assertion': [LIT, (kb.RX_AT | kb.RX_LAZY, 0, 0, 0)],
    'too many frames': [(kb.RX_LIT, 97, 0, 1)] * 15 + [LIT, (kb.RX_ALT, 2, 4, 0), (kb.RX_ARM, 1, 4, 0), (kb.RX_LIT, 98, 1, -1),
                                                       (kb.RX_ARM, 1, 2, 0), LIT],
    'empty shortest match': [(kb.RX_LIT, 97, 0, 1), (kb.RX_ALT, 2, 3, 0), (kb.RX_ARM, 0, 3, 0), (kb.RX_ARM, 1, 2, 0), LIT],
    'only assertions': [(kb.RX_AT, kb.AT_BOS, 0, 0), (kb.RX_AT, kb.AT_EOS, 0, 0)],
}


@pytest.mark.parametrize('case', sorted(MALFORMED))
def test_kw_compile_rejects_malformed_streams_without_gpu(case):
    rc, msg = _kw_compile_rc(MALFORMED[case])
    assert rc == _native.KW_EUNSUPPORTED, (case, rc, msg)
    assert b'pattern 0' in msg, msg


def test_python_programs_pass_the_c_check():
    """What regex_program emits is what kw_compile's check takes: every program of this file passes the
    validation (without a GPU kw_compile then fails at the device, or succeeds with one: never EUNSUPPORTED)."""
    for name in [n for n in TABLE if n not in HOST_NAMES] + ORDER_NAMES:
        rc, msg = _kw_compile_rc(kb.regex_program(name))
        assert rc != _native.KW_EUNSUPPORTED, (name, msg)
    rc, msg = _kw_compile_rc(kb.NOPOS_PROGRAM)
    assert rc != _native.KW_EUNSUPPORTED, msg


# ------------------------------------------------------------------ the host position fallback
def test_resolve_host_positions():
    names = ['Joe (Jr)?', 'a?', 'Plain Name Inc', 'C++ Partners', '[24]7.ai']
    ckb = compile_kb(_processed(names))
    pid = {n: i for i, n in enumerate(ckb.names)}
    assert [ckb.host_regex[pid[n]] for n in names] == [True, True, False, False, False]
    assert ckb.invalid_regex[pid['C++ Partners']]
    fields = {(0, 0): 'Joe (Jr)? Joe Jr Joe ', (0, 1): 'é中 Joe (Jr)? and Joe Jr', (1, 0): 'a? banana',
              (1, 1): 'Joe (Jr)', (2, 0): 'x', (2, 1): 'Jo (Jr)?'}
    NOPOS = _native.KW_NOPOS
    recs = [(0, pid['Plain Name Inc'], NOPOS, 0), (0, pid['Joe (Jr)?'], NOPOS, 0), (0, pid['[24]7.ai'], 7, 0),
            (0, pid['Joe (Jr)?'], NOPOS, 1), (0, pid['C++ Partners'], NOPOS, 1), (1, pid['a?'], NOPOS, 0),
            (1, pid['Joe (Jr)?'], NOPOS, 1), (2, pid['[24]7.ai'], NOPOS, 0), (2, pid['Joe (Jr)?'], NOPOS, 1)]
    hits = np.array(recs, dtype=_native.HIT_DTYPE)
    asked = []

    def text(doc, field):
        asked.append((doc, field))
        return fields[(doc, field)]

    got = resolve_host_positions(ckb, hits, text)
    want = []
    for d, p, q, f in recs:
        pos = [m.start() for m in re.finditer(ckb.names[p], fields[(d, f)])] if ckb.host_regex[p] and q == NOPOS else []
        want += [(d, p, x, f) for x in pos] or [(d, p, q, f)]
    assert got.dtype == hits.dtype and [tuple(int(x) for x in r) for r in got.tolist()] == want
    # code-point positions in the non-ASCII title, the kept KW_NOPOS of a decided field without a position
    assert (0, pid['Joe (Jr)?'], 3, 1) in want and (0, pid['Joe (Jr)?'], 17, 1) in want
    assert (2, pid['Joe (Jr)?'], NOPOS, 1) in want and (0, pid['C++ Partners'], NOPOS, 1) in want
    assert sorted(asked) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)]      # only decided fields of host names
    # nothing to do: the very same array comes back
    plain = compile_kb(_processed(['Plain Name Inc']))
    one = hits[:1]
    assert resolve_host_positions(plain, one, text) is one and resolve_host_positions(ckb, one, text) is one
    assert resolve_host_positions(ckb, None, text) is None
