"""GPU: the one device scan (csrc/kwscan.hip, scan_launch of csrc/kwhandle.hpp) at the sizes where its shape changes.

scan_launch cuts m values into min(SCAN_CHUNKS, ceil(m / (4 * BLOCK))) chunks: one chunk up to 1024 values, one more
for every 1024 after that, and from 4 * BLOCK * SCAN_CHUNKS = 524 288 values on the chunk count stands still and the
chunks grow instead.  No other test of the suite passes that size.  A CDX listing of n one-URL lines drives it:
in kw_cdx_append the rows' arena offsets are the scan over the n URL lengths, and the row count is the scan over the
tiles' row counts.

Bar: exact.  The verdict is KW_CDX_OK, and the row count, the offsets, the timestamps and the arena bytes equal what
numpy.cumsum gives over the same generated lengths.
"""
import numpy as np
import pytest

from tests import cdx_rule as R

pytestmark = pytest.mark.gpu

BLOCK, SCAN_CHUNKS = 256, 512            # csrc/kwdev.hpp, csrc/kwhandle.hpp
EDGE = 4 * BLOCK * SCAN_CHUNKS           # 524 288
SIZES = [1, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK, 4 * BLOCK + 1, EDGE - 1, EDGE, EDGE + 1, 1_100_000]
T0 = 20200101000000


@pytest.fixture(scope='module')
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advanced_scrapper_amd.cdx_dedup import GpuUrlDedup
    return GpuUrlDedup()


@pytest.fixture(scope='module')
def listing():
    """max(SIZES) good lines `k <timestamp> <url>`, built once: the URLs are distinct (the row index is in them) and
    their lengths vary with the row index.  (text, line ends [n + 1], URL arena, URL offsets [n + 1]); a case of n
    rows takes the first n lines."""
    n = max(SIZES)
    pad = [b'x' * k for k in range(13)]
    urls = [b'http://h/%d%s' % (i, pad[i % 13]) for i in range(n)]
    lines = [b'k %d %s\n' % (T0 + i, u) for i, u in enumerate(urls)]
    line_end = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, lines), dtype=np.int64, count=n), out=line_end[1:])
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, urls), dtype=np.int64, count=n), out=off[1:])
    return b''.join(lines), line_end, b''.join(urls), off


@pytest.mark.parametrize('n', SIZES)
def test_scan_edges_through_a_listing(gpu, listing, n):
    text, line_end, arena, off = listing
    gpu.cdx_begin()
    assert gpu.cdx_append(memoryview(text)[:int(line_end[n])], 'listing') == (R.OK, -1, n)
    got_arena, got_off, got_ts = gpu.cdx_rows()
    assert len(got_ts) == n and len(got_off) == n + 1
    assert np.array_equal(got_off, off[:n + 1])
    assert np.array_equal(got_ts, T0 + np.arange(n, dtype=np.int64))
    assert got_arena == arena[:int(off[n])]
