"""One scan of the boundary sweep's small-KB documents in a process of its own (tests/test_gpu_fuzzy_sweep.py).

libkwmatch reads KW_EPI_FLAT once per process, at its first scan; the per-document epilogue (KW_DEV=1,
KW_EPI_FLAT=0) can therefore only be chosen by a process that has not scanned yet.  Usage:

    KW_DEV=1 KW_EPI_FLAT=0 python -m tests.fuzzy_sweep_worker OUT.npy

writes the scan's records ([n, 4] uint32: doc, pattern, pos, field) to OUT.npy and prints one JSON line."""
import json
import os
import sys

import numpy as np


def main(out):
    knobs = {'dev': os.environ.get('KW_DEV'), 'epi_flat': os.environ.get('KW_EPI_FLAT')}   # before the library loads
    from advanced_scrapper_amd import _native
    from tests.test_gpu_fuzzy_sweep import _matcher, default_docs
    texts, titles, _tags = default_docs('small')
    m = _matcher('small')
    try:
        try:                      # the handle, the only one of this process, has not scanned yet: no statistics
            m.stats()
            first_scan = False
        except _native.KwError:
            first_scan = True
        hits = m.match_strings(texts, titles)
        stats = m.stats()
    finally:
        m.close()
    np.save(out, np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4))
    print(json.dumps(dict(knobs, first_scan=bool(first_scan), docs=len(texts), hits=int(len(hits)), stats=stats)))


if __name__ == '__main__':
    main(sys.argv[1])
