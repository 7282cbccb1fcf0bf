"""One scan of the byte-geometry sweep's documents (KB base) in a process of its own (tests/test_gpu_tx_geometry.py).

libkwmatch reads KW_EPI_FLAT once per process, at its first scan; the per-document epilogue (KW_DEV=1,
KW_EPI_FLAT=0) can therefore only be chosen by a process that has not scanned yet.  Usage:

    KW_DEV=1 KW_EPI_FLAT=0 python -m tests.tx_geometry_worker OUT.npy

writes the scan's records ([n, 4] uint32: doc, pattern, pos, field) to OUT.npy and the documents' routes to
OUT.npy.routes.npy, and prints one JSON line."""
import json
import os
import sys

import numpy as np


def main(out):
    knobs = {'dev': os.environ.get('KW_DEV'), 'epi_flat': os.environ.get('KW_EPI_FLAT')}   # before the library loads
    from advanced_scrapper_amd import _native
    from tests import tx_geometry as tg
    from tests.test_gpu_tx_geometry import _matcher
    texts, titles, _tags = tg.corpus()
    m = _matcher('base')
    try:
        try:                      # the handle, the only one of this process, has not scanned yet: no statistics
            m.stats()
            first_scan = False
        except _native.KwError:
            first_scan = True
        hits = m.match_strings(texts, titles)
        routes = m.doc_routes(len(texts))
        stats = m.stats()
    finally:
        m.close()
    np.save(out, np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4))
    np.save(out + '.routes.npy', routes)
    print(json.dumps(dict(knobs, first_scan=bool(first_scan), docs=len(texts), hits=int(len(hits)), stats=stats)))


if __name__ == '__main__':
    main(sys.argv[1])
