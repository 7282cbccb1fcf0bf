"""GPU: the byte-geometry sweep of the URL dedup (csrc/dedup.hip) -- the families of tests/dedup_geometry.py (held
to their claims on the CPU by tests/test_dedup_geometry_cases.py) through ``GpuUrlDedup.upload`` / ``run`` /
``counts`` / ``kept_device`` on a hand-packed arena whose 32 bytes past the end are hostile.

Bar: bit-exact.  Every run's per-row codes, kept row indices, dense offsets and kept bytes equal the oracle's
(``oracle/dedup_oracle.py``), the four counts add up, and a second run on the same handle gives the same codes.
"""
import functools

import numpy as np
import pytest

from tests import dedup_geometry as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.cdx_dedup import GpuUrlDedup
    return GpuUrlDedup()


@functools.lru_cache(maxsize=None)
def _family(name):
    """(rows, the oracle's expectation) of a family's main run, computed once."""
    rows = G.raw_rows().rows if name == 'raw' else G.family_rows(name)
    return rows, G.expected(rows, normalize=name != 'raw')


def _route_counts(g):
    """kw_dedup_route_counts of the last run."""
    from advanced_scrapper_amd import _native
    v = np.zeros(4, dtype=np.int64)
    g._check(_native.lib().kw_dedup_route_counts(g.h, _native.ptr(v), 4))
    return dict(zip(('slow', 'differing', 'collide', 'listed'), (int(x) for x in v)))


def _n_slow(rows):
    return sum(G.route(G.enc(r)).route == 'slow' for r in rows)


def _run(g, rows, exp=None, normalize=True):
    """One run over the hand-packed rows against the oracle, and a second run; the first run's route counters."""
    if exp is None:
        exp = G.expected(rows, normalize)
    arena, off = G.pack(rows)
    assert len(arena) == int(off[-1]) + G.PAD_BYTES
    d_a, d_o = g.upload(arena, off)
    c1 = g.run(d_a, d_o, len(rows), normalize).cpu().numpy()
    rc = _route_counts(g)
    bad = np.nonzero(c1 != exp.codes)[0]
    assert len(bad) == 0, [(int(i), rows[i], int(c1[i]), int(exp.codes[i])) for i in bad[:8]]
    assert g.counts() == exp.counts
    b, o, r = g.kept_device()
    assert np.array_equal(r.cpu().numpy(), exp.kept_rows)
    assert np.array_equal(o.cpu().numpy(), exp.kept_off)
    got = b.cpu().numpy().tobytes()
    if got != exp.kept_bytes:
        ko = exp.kept_off
        k = next(k for k in range(len(exp.kept_rows)) if got[ko[k]:ko[k + 1]] != exp.kept_bytes[ko[k]:ko[k + 1]])
        i = int(exp.kept_rows[k])
        raise AssertionError(f'kept row {k} (row {i}, dense offset {int(ko[k])}): {rows[i]!r} -> '
                             f'{got[ko[k]:ko[k + 1]]!r}, want {exp.kept_bytes[ko[k]:ko[k + 1]]!r}')
    c2 = g.run(d_a, d_o, len(rows), normalize).cpu().numpy()
    assert np.array_equal(c1, c2)
    return rc


def _lane_row_copy(monkeypatch):
    """The lane-per-row dd_copy_kernel (stage CP_STAGE) in place of the staged copy."""
    monkeypatch.setenv('KW_DEV', '1')
    monkeypatch.setenv('KW_DEDUP_COPY_LANE_ROW', '1')


@pytest.mark.parametrize('name', ['align_cut', 'cut_rule', 'gap', 'filter'])
def test_family(gpu, name):
    rows, exp = _family(name)
    rc = _run(gpu, rows, exp)
    assert rc['slow'] == _n_slow(rows)


def test_slow(gpu):
    rows, exp = _family('slow')
    rc = _run(gpu, rows, exp)
    assert rc['slow'] == _n_slow(rows) > 250


def test_same_key(gpu, monkeypatch):
    rows, exp = _family('same_key')
    rc = _run(gpu, rows, exp)
    assert rc['slow'] == _n_slow(rows)
    assert rc['differing'] == 0 and rc['collide'] == 0 and rc['listed'] == 0
    # the 4-bit hash: nearly every pair differs and goes pairs -> recheck -> the host's exact pass
    monkeypatch.setenv('KW_TEST_DEDUP_WEAK_HASH', '1')
    rc = _run(gpu, rows, exp)
    assert rc['differing'] > len(rows) // 2 and rc['collide'] > 0 and rc['listed'] == rc['collide']
    # keys equal in their first 128 bytes, a run of their own: pairs that compare_pairs' later rounds tell apart
    for length in G.TWIN_LENS:
        rows = G.tail_twins(length)
        rc = _run(gpu, rows)
        assert rc['differing'] >= len(rows) - 16 - G.TWIN_REPEATS > 0


def test_raw(gpu, monkeypatch):
    rows, exp = _family('raw')
    rc = _run(gpu, rows, exp, normalize=False)
    assert rc['slow'] == 0
    monkeypatch.setenv('KW_TEST_DEDUP_WEAK_HASH', '1')
    rc = _run(gpu, rows, exp, normalize=False)
    assert rc['differing'] > len(rows) // 2 and rc['collide'] > 0
    for length in G.TWIN_LENS:
        rows = G.tail_twins(length, spelled=False)
        rc = _run(gpu, rows, normalize=False)
        assert rc['differing'] >= len(rows) - 16 - G.TWIN_REPEATS > 0


def test_groups(gpu, monkeypatch):
    """(Which groups are staged and which read global memory: tests/test_dedup_geometry_cases.py; the kernel has
    no counter for it.)"""
    rows, exp = _family('groups')
    _run(gpu, rows, exp)
    for n in G.GROUP_ROW_COUNTS:
        _run(gpu, G.group_count_rows(n))
    _lane_row_copy(monkeypatch)
    _run(gpu, rows, exp)


def test_copy(gpu, monkeypatch):
    rows, exp = _family('copy')
    _run(gpu, rows, exp)
    for n in G.COPY_KEPT_COUNTS:
        _run(gpu, G.copy_count_rows(n))
    _lane_row_copy(monkeypatch)
    _run(gpu, rows, exp)
    for n in G.COPY_KEPT_COUNTS:
        _run(gpu, G.copy_count_rows(n))


def test_collision_list_longer_than_its_cap(gpu, monkeypatch):
    """More rows share a tag with another URL than the device list holds: dd_collect_kernel counts them again and
    the host finds them by a scan of the codes."""
    monkeypatch.setenv('KW_TEST_DEDUP_WEAK_HASH', '1')
    rows = G.collide_rows()
    rc = _run(gpu, rows)
    print('listed rows:', rc['listed'])
    assert rc['listed'] > G.GEOMETRY['COLLIDE_CAP'] and rc['collide'] == rc['listed']
