"""tests/sort_rule.py against pandas: for every case of the table the rule takes, the rule's bytes are the bytes of
the reference's read_csv -> sort_values('time_unix') -> astype(int) -> to_csv(index=False); the rule takes at
least half of the table (so the device tests cannot pass by refusing everything); the case table names every
outcome the device route has; libkwmatch.so exports the sort's entry points."""
import re
import subprocess

import pytest

from tests import sort_rule as S

_DECIDED = {}


def decided(name, data):
    if name not in _DECIDED:
        _DECIDED[name] = S.decide(data)
    return _DECIDED[name]


@pytest.mark.parametrize('name,data', S.CASES, ids=[n for n, _ in S.CASES])
def test_taken_case_equals_pandas(name, data):
    outcome, _row, expected = decided(name, data)
    if outcome != 'OK':
        assert expected is None
        return
    assert expected == S.pandas_bytes(data), name


def test_rule_takes_at_least_half_of_the_table():
    taken = sum(decided(n, d)[0] == 'OK' for n, d in S.CASES)
    assert 2 * taken >= len(S.CASES), (taken, len(S.CASES))


def test_table_reaches_every_outcome():
    want = {'one-row': 'OK', 'ties-40x3': 'OK', 'key-int64-extremes': 'OK', 'key-negative': 'OK',
            'empty-source_url': 'OK', 'empty-title': 'OK', 'quoted-cells': 'OK', 'crlf': 'OK', 'ascending': 'OK',
            'descending': 'OK', 'header-quoted-name': 'OK', 'block-dtype-taken': 'OK', 'all-na-column': 'OK',
            'header-duplicate': 'header-duplicate', 'header-no-time_unix': 'header-no-time_unix',
            'header-5-columns': 'header-columns', 'header-missing-column': 'header-columns',
            'header-only': 'header-only', 'lone-cr': 'ingest-CR', 'blank-record': 'ingest-BLANK',
            'block-dtype-refused': 'sort-DTYPE', 'numeric-title-column': 'sort-DTYPE',
            'block-quoted-braces-bad': 'sort-FORM', 'block-quoted-braces-good': 'sort-FORM'}
    for name, data in S.CASES:
        outcome, row, _ = decided(name, data)
        if name.startswith('key-') and name not in ('key-int64-extremes', 'key-negative'):
            assert (outcome, row) == ('sort-KEY', 1), name
        elif name.startswith('form-'):
            assert (outcome, row) == ('sort-FORM', 1), name
        elif name in want:
            assert outcome == want[name], (name, outcome)
    assert decided('block-dtype-refused', dict(S.CASES)['block-dtype-refused'])[1] == 0


def test_key_form():
    ok = {b'0': 0, b'7': 7, b'-7': -7, b'10': 10, b'9223372036854775807': (1 << 63) - 1,
          b'-9223372036854775808': -(1 << 63)}
    for cell, v in ok.items():
        assert S.canonical_key(cell) == v
    for cell in (b'', b'-', b'-0', b'+1', b'01', b'00', b' 1', b'1 ', b'1.0', b'1e3', b'1_0', b'9223372036854775808',
                 b'-9223372036854775809', b'--1', b'0x1', '١'.encode()):
        assert S.canonical_key(cell) is None, cell


def test_library_exports_the_sort():
    from advanced_scrapper_amd import _native
    L = _native.lib()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True).stdout
    for f in ('kw_sort_create', 'kw_sort_keys', 'kw_sort_gather', 'kw_sort_last_ms', 'kw_sort_last_error',
              'kw_sort_destroy', 'kw_ingest_spans', 'kw_ingest_copy_spans'):
        assert f in _native.EXPORTS and hasattr(L, f), f
        assert re.search(rf'\bT {f}\b', out), f
