"""One per-ticker file above ingest.MAX_WINDOW -- about 1M rows of about 2.5 KB in random key order, 2.5 GB --
through sort_matched_csv on one route, in this process: one warm-up, then three timed sorts of a fresh copy.

    python scripts/sort_huge.py make FILE                        # write the synthetic file
    python scripts/sort_huge.py run FILE OUT.json LABEL [--host] [--tree DIR] [--window BYTES] [--slab BYTES]
                                [--reps N]                       # sort copies of FILE, write LABEL's result
    python scripts/sort_huge.py report OUT.json PART.json ...    # merge the parts: profiles/sort_huge_file.json

``run`` is started once per route, each in a fresh process: the device route of this tree, ``--host`` (this tree
with KW_SORT_DEVICE=0), and ``--tree DIR`` (a built checkout of the parent commit, where the file is refused with
'size' and match_keywords._sort_native runs).  ``--window`` / ``--slab`` install a DeviceSorter of that geometry.
``report`` checks that every part wrote the same bytes (sha256) and names the fastest geometry."""
import hashlib
import json
import os
import shutil
import sys
import time

HEAD = b'time_unix,date_time,text_matches,title_matches,title,url,source,source_url,article_text\n'
ROWS, TEXT = 1_000_000, 2400


def make(path):
    import numpy as np
    rng = np.random.default_rng(7)
    keys = rng.integers(1_400_000_000, 1_700_000_000, ROWS).tolist()
    pad = b'lorem ipsum dolor sit amet ' * (TEXT // 27 + 5)
    with open(path, 'wb') as fh:
        fh.write(HEAD)
        for lo in range(0, ROWS, 10000):
            fh.write(b''.join(b'%d,2020-01-02 03:04:05,{},{},Title %d,http://a.b/%d,yahoo,,%s\n'
                              % (keys[i], i, i, pad[:TEXT + i % 97]) for i in range(lo, lo + 10000)))
    print(json.dumps({'file': path, 'bytes': os.path.getsize(path), 'rows': ROWS}))


def sha256(path):
    h = hashlib.sha256()
    with open(path, 'rb') as fh:
        for block in iter(lambda: fh.read(1 << 24), b''):
            h.update(block)
    return h.hexdigest()


def run(src, out, label, host, tree, window, slab, reps):
    if host:
        os.environ['KW_SORT_DEVICE'] = '0'
    sys.path.insert(0, tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from advanced_scrapper_amd import ingest, match_keywords, sortfiles
    if window or slab:
        sortfiles._SORTER = sortfiles.DeviceSorter(0, window_bytes=window or sortfiles.WINDOW_BYTES,
                                                   slab_bytes=slab or sortfiles.SLAB_BYTES)
    work = src + '.' + label + '.csv'
    walls, stats = [], None
    for rep in range(reps + 1):                  # (the first one warms the process up)
        shutil.copyfile(src, work)
        sortfiles.reset_stats()
        t0 = time.perf_counter()
        match_keywords.sort_matched_csv(work)
        walls.append(round(time.perf_counter() - t0, 4))
        stats = sortfiles.LAST_STATS
    timed = sorted(walls[1:])
    res = {'label': label, 'route': 'host' if host else 'parent' if tree else 'device', 'bytes': os.path.getsize(src),
           'warmup_s': walls[0], 'wall_s': walls[1:], 'median_s': timed[len(timed) // 2], 'range_s': [timed[0], timed[-1]],
           'sha256': sha256(work), 'max_window': ingest.MAX_WINDOW,
           'counts': {k: stats[k] for k in ('device', 'unchanged', 'native', 'pandas', 'refused')}}
    if stats['device']:
        s = sortfiles._SORTER
        b, ms = stats['gather_bytes'], stats['ms']
        pinned = sum(len(a) for d in s._ingests.values() for a in d._stage if a is not None)
        slab_cap = s.slab_bytes + s.slab_bytes // 4 + 4096          # (kwsort.hip's pinned buffers: a quarter's slack)
        keys_cap = 8 * ROWS + 2 * ROWS + 4096
        res.update({'window_bytes': s.window_bytes, 'slab_bytes': s.slab_bytes, 'windows': stats['windows'],
                    'slabs': stats['slabs'], 'ms': {k: round(v, 3) for k, v in ms.items()},
                    'wall_split_s': {k: round(v, 4) for k, v in stats['wall_s'].items()},
                    'parse_GBps': round(stats['bytes'] / ms['parse'] / 1e6, 1),
                    'gather_GBps_out': round(b / ms['gather'] / 1e6, 1),
                    'gather_share_of_8TBps': round(2 * b / (ms['gather'] * 1e-3) / 8e12, 4),
                    'store_bytes': stats['bytes'] + 64,
                    'pinned_host_bytes': {'windows': pinned, 'slabs': 2 * slab_cap, 'keys': keys_cap,
                                          'all': pinned + 2 * slab_cap + keys_cap}})
    sortfiles.close()
    os.remove(work)
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


def report(out, parts):
    res = [json.load(open(p)) for p in parts]
    digests = {r['sha256'] for r in res}
    assert len(digests) == 1, 'the routes wrote different bytes: ' + repr([(r['label'], r['sha256']) for r in res])
    sweep = [r for r in res if r['label'].startswith('sweep')]
    doc = {'file': {'rows': ROWS, 'bytes': res[0]['bytes'], 'sha256_sorted': digests.pop()},
           'routes': {r['label']: r for r in res if not r['label'].startswith('sweep')},
           'sweep_once_each': [{k: r[k] for k in ('window_bytes', 'slab_bytes', 'wall_s', 'ms')} for r in sweep]}
    if sweep:
        # (one run each: a difference counts only where it exceeds the spread between two runs of one geometry,
        # the defaults' own sweep run against their three timed runs in routes.device)
        walls = [r['wall_s'][0] for r in sweep]
        best = sweep[walls.index(min(walls))]
        doc['sweep_range_s'] = [min(walls), max(walls)]
        doc['sweep_fastest'] = {'window_bytes': best['window_bytes'], 'slab_bytes': best['slab_bytes']}
    dev, host = doc['routes'].get('device'), doc['routes'].get('host')
    if dev and host:
        doc['defaults'] = {'window_bytes': dev['window_bytes'], 'slab_bytes': dev['slab_bytes']}
        doc['device_faster'] = dev['median_s'] < host['median_s']
        doc['gather_TBps_read_plus_write'] = round(2 * (dev['store_bytes'] - 64) / (dev['ms']['gather'] * 1e-3) / 1e12, 2)
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    argv = sys.argv[1:]
    if argv[:1] == ['make']:
        make(argv[1])
    elif argv[:1] == ['report']:
        report(argv[1], argv[2:])
    elif argv[:1] == ['run']:
        opt = {'--tree': None, '--window': 0, '--slab': 0, '--reps': 3}
        rest = argv[4:]
        for k in list(opt):
            if k in rest:
                v = rest[rest.index(k) + 1]
                opt[k] = v if k == '--tree' else int(v)
        run(argv[1], argv[2], argv[3], '--host' in rest, opt['--tree'], opt['--window'], opt['--slab'], opt['--reps'])
    else:
        sys.exit(__doc__)
