"""One large per-ticker file through sortfiles.sort_file, three times: the device times and rates of the output sort
at a size that fills the grid (200k rows of 2.5 KB, 2M rows of 90 bytes).

    python scripts/sort_rate.py OUT.json        # profiles/sort_large_file.json
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
from advanced_scrapper_amd import sortfiles   # noqa: E402

HEAD = b'time_unix,date_time,text_matches,title_matches,title,url,source,source_url,article_text\n'
rng = np.random.default_rng(3)
out = {}
for label, n, tlen in (('rows_2500B_x_200k', 200000, 2400), ('rows_90B_x_2M', 2000000, 8)):
    keys = rng.integers(1_400_000_000, 1_700_000_000, n)
    pad = b'lorem ipsum dolor sit amet ' * (tlen // 27 + 1)
    rows = [b'%d,2020-01-02 03:04:05,{},{},Title %d,http://a.b/%d,yahoo,,%s\n' % (k, i, i, pad[:tlen + i % 97])
            for i, k in enumerate(keys.tolist())]
    data = HEAD + b''.join(rows)
    del rows
    work = tempfile.mkdtemp()
    path = os.path.join(work, 'X_match.csv')
    res = []
    for rep in range(3):
        with open(path, 'wb') as fh:
            fh.write(data)
        sortfiles.reset_stats()
        t0 = time.perf_counter()
        ok = sortfiles.sort_file(path)
        wall = time.perf_counter() - t0
        st = sortfiles.LAST_STATS
        assert ok, st
        b = st['gather_bytes']
        res.append({'wall_s': round(wall, 4), 'ms': {k: round(v, 3) for k, v in st['ms'].items()},
                    'wall_split_s': {k: round(v, 4) for k, v in st['wall_s'].items()},
                    'bytes': b, 'parse_GBps': round(st['bytes'] / st['ms']['parse'] / 1e6, 1),
                    'gather_GBps_out': round(b / st['ms']['gather'] / 1e6, 1),
                    'gather_share_of_8TBps': round(2 * b / (st['ms']['gather'] * 1e-3) / 8e12, 4)})
    # the result is sorted
    with open(path, 'rb') as fh:
        got = fh.read()
    ks = np.array([int(l.split(b',', 1)[0]) for l in got[len(HEAD):].split(b'\n')[:-1]])
    assert len(ks) == n and (np.diff(ks) >= 0).all() and len(got) == len(data)
    os.remove(path)
    os.rmdir(work)
    out[label] = res
sortfiles.close()
if OUT:
    with open(OUT, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
print(json.dumps(out))
