"""One large file a run wrote itself -- scripts/sort_huge.py's shape, about 1M rows of about 2.5 KB in random key
order, 2.5 GB -- finished by egress.RunFiles.finish on one route, in this process: the lines and the write index
are made by hand, then one warm-up and three timed finishes of a fresh copy.

    python scripts/finish_large.py run DIR OUT.json LABEL [--host] [--rows N] [--reps N]
    python scripts/finish_large.py report OUT.json PART.json ...      # merge: profiles/finish_large_file.json

``run`` is started once per route, each in a fresh process: the device route (the body in windows from the write
index, out in slabs) and ``--host`` (KW_FINISH_DEVICE=0: the whole file read, sliced per row and joined).  Each part
holds the wall times, the process's peak resident size and the sha256 of the result; ``report`` checks that the
routes wrote the same bytes.  The body spans several windows, so the spans lie beyond 2^31 here."""
import json
import os
import resource
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sort_huge import HEAD, TEXT, sha256  # noqa: E402


def make(path, rows):
    """The file, and its index as the run's appends would have built it: (stamps, lens)."""
    import numpy as np
    rng = np.random.default_rng(7)
    keys = rng.integers(1_400_000_000, 1_700_000_000, rows)
    pad = b'lorem ipsum dolor sit amet ' * (TEXT // 27 + 5)
    lens = np.empty(rows, dtype=np.int64)
    kl = keys.tolist()
    with open(path, 'wb') as fh:
        fh.write(HEAD)
        for lo in range(0, rows, 10000):
            lines = [b'%d,2020-01-02 03:04:05,{},{},Title %d,http://a.b/%d,yahoo,,%s\n' % (kl[i], i, i, pad[:TEXT + i % 97])
                     for i in range(lo, min(lo + 10000, rows))]
            lens[lo:lo + len(lines)] = [len(x) for x in lines]
            fh.write(b''.join(lines))
    return keys.astype(np.int64), lens


def run(work, out, label, host, rows, reps):
    import numpy as np
    os.environ['KW_FINISH_DEVICE'] = '0' if host else '1'
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from advanced_scrapper_amd import egress, sortfiles
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, 'large.src')
    stamps, lens = make(src, rows)
    out_dir = os.path.join(work, 'out_' + label)
    name = 'L_match.csv'
    walls, stats = [], None
    for _rep in range(reps + 1):                 # (the first one warms the process up)
        shutil.rmtree(out_dir, ignore_errors=True)
        os.makedirs(out_dir)
        files = egress.RunFiles(out_dir)
        shutil.copyfile(src, os.path.join(out_dir, name))
        for lo in range(0, rows, 20000):         # (appends of a chunk's rows each)
            files.add(name, stamps[lo:lo + 20000], lens[lo:lo + 20000], np.full(len(lens[lo:lo + 20000]), 0xFF, np.uint32),
                      HEAD)
        sortfiles.reset_stats()
        t0 = time.perf_counter()
        assert files.finish(name) is True
        walls.append(round(time.perf_counter() - t0, 4))
        stats = sortfiles.LAST_STATS
    timed = sorted(walls[1:])
    res = {'label': label, 'route': 'host' if host else 'device', 'rows': rows, 'bytes': os.path.getsize(src),
           'warmup_s': walls[0], 'wall_s': walls[1:], 'median_s': timed[len(timed) // 2], 'range_s': [timed[0], timed[-1]],
           'maxrss_kib': resource.getrusage(resource.RUSAGE_SELF).ru_maxrss,
           'sha256': sha256(os.path.join(out_dir, name)),
           'counts': {k: stats[k] for k in ('indexed', 'index_host', 'refused', 'windows', 'slabs')},
           'ms': {k: round(v, 3) for k, v in stats['ms'].items()},
           'wall_split_s': {k: round(v, 4) for k, v in stats['wall_s'].items()}}
    sortfiles.close()
    shutil.rmtree(out_dir, ignore_errors=True)
    os.remove(src)
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


def report(out, parts):
    res = [json.load(open(p)) for p in parts]
    assert len({r['sha256'] for r in res}) == 1, 'the routes wrote different bytes'
    doc = {'file': {'rows': res[0]['rows'], 'bytes': res[0]['bytes'], 'sha256_sorted': res[0]['sha256']},
           'routes': {r['label']: r for r in res}}
    dev, host = doc['routes'].get('device'), doc['routes'].get('host')
    if dev and host:
        doc['device_faster'] = dev['median_s'] < host['median_s']
        doc['peak_resident_MiB'] = {'device': dev['maxrss_kib'] // 1024, 'host': host['maxrss_kib'] // 1024}
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    argv = sys.argv[1:]
    if argv[:1] == ['report']:
        report(argv[1], argv[2:])
    elif argv[:1] == ['run']:
        opt = {'--rows': 1_000_000, '--reps': 3}
        rest = argv[4:]
        for k in list(opt):
            if k in rest:
                opt[k] = int(rest[rest.index(k) + 1])
        run(argv[1], argv[2], argv[3], '--host' in rest, opt['--rows'], opt['--reps'])
    else:
        sys.exit(__doc__)
