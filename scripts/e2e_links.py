"""End-to-end timing of ``links.refresh_links`` and ``links.split_links``: the device route against the pandas route.

Writes one synthetic ``yahoo_links_1.csv`` (--rows links, a tenth of them repeated), an article dataset
``yahoo_articles_all.csv`` with full article rows (multi-line cells, written with the csv module as the scraper does)
for about 45 % of the links, and a success file for a fifth of the rest (the shape of profiles/e2e_resume.json), then
times ``refresh_links()`` and, over the file it wrote, ``split_links(..., num_parts=4)`` in a fresh child process per
run (one warm-up, then the median of 5 with the range; a child initialises the GPU and creates the dedup handle before
its clocks start, and nothing is exec'd after that).  Two configurations of this tree:

    native   the device route (the default)
    pandas   KW_LINKS_NATIVE=0: the reference's lines (experiental/drop.py, split.py), the baseline, as the steps have
             no counterpart at the parent commit

Both must write the same bytes (one sha256 over the refreshed list and the four parts).  The result goes to --out
(profiles/e2e_links.json) and, as one JSON line, to stdout: per configuration and call the median, min and max seconds;
for the device route the device spans of the median run (kw_cdx_last_ms, the exclude spans, the select spans), the
host argsort time on its own line, and the select copy's bytes in + out over its time beside the row-order renderer's
(kw_cdx_csv_copy over the same links file, after the clocks stopped).

    python scripts/e2e_links.py [--rows 1000000] [--out profiles/e2e_links.json]

``--stream`` measures the streamed route instead ("Windowed CSV append") and writes
profiles/e2e_links_stream.json: over the same workload, one after the other in one call, the one-piece route
(``stream_from`` above any size), the streamed route with ``stream_from=0`` at the default window and at a
64 MiB window, and, with ``--parent-tree DIR`` (a built checkout of the parent commit), that tree's route.  With
``--pandas`` the pandas route runs too (the large-input comparison: ``--rows 10000000 --runs 1``).  Every
configuration must write the same bytes; each child reports its peak resident memory (``ru_maxrss``).
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = 4

CHILD = r'''
import hashlib, json, os, resource, sys, time
tree, folder = sys.argv[1:3]
sys.path.insert(0, tree)
os.chdir(folder)
import numpy as np
import torch
from advanced_scrapper_amd import cdx_dedup, links
torch.cuda.init()
g = cdx_dedup._dedup()
torch.cuda.synchronize()
argsort_s = []
inner = links.descending_order
def timed_order(keys):
    t = time.perf_counter()
    r = inner(keys)
    argsort_s.append(time.perf_counter() - t)
    return r
links.descending_order = timed_order
sys.stdout = open(os.devnull, 'w')
kw = {k: int(os.environ[e]) for k, e in (('stream_from', 'E2E_STREAM_FROM'), ('window_bytes', 'E2E_WINDOW_BYTES'))
      if e in os.environ}
t0 = time.perf_counter()
a = links.refresh_links(**kw)
t1 = time.perf_counter()
spans_a = None
if a.route == 'device':
    spans_a = {'cdx_last_ms': g.cdx_last_ms(), 'exclude_last_ms': g.exclude_last_ms(), 'select_last_ms': g.select_last_ms()}
t2 = time.perf_counter()
b = links.split_links('yahoo_links_new.csv', 'part', %d, 'success_articles_yfin.csv', **kw)
t3 = time.perf_counter()
sys.stdout = sys.__stdout__
spans_b = None
if b.route == 'device':
    spans_b = {'cdx_last_ms': g.cdx_last_ms(), 'exclude_last_ms': g.exclude_last_ms(), 'select_last_ms': g.select_last_ms()}
sha = hashlib.sha256()
sizes = []
for name in ['yahoo_links_new.csv'] + ['part_%%d.csv' %% i for i in range(%d)]:
    with open(name, 'rb') as fh:
        data = fh.read()
    sha.update(data)
    sizes.append(len(data))
res = {'refresh_s': t1 - t0, 'split_s': t3 - t2, 'routes': [a.route, b.route], 'refresh_counts': list(a.counts()),
       'split_counts': list(b.counts()), 'split_parts': b.parts, 'sha256': sha.hexdigest(), 'out_bytes': sizes,
       'windows': [list(getattr(a, 'windows', ())), list(getattr(b, 'windows', ()))],
       'maxrss_kb': resource.getrusage(resource.RUSAGE_SELF).ru_maxrss}
if spans_a and spans_b:
    res['refresh_spans'], res['split_spans'] = spans_a, spans_b
    res['argsort_s'] = argsort_s[0]
    # the row-order renderer over the same links file, for comparison (not timed above)
    g.cdx_begin()
    g.cdx_append(np.fromfile('yahoo_links_1.csv', dtype=np.uint8), 'part')
    g.cdx_run(normalize=False)
    csv_bytes = len(g.cdx_csv())
    res['row_order'] = {'render_ms': g.cdx_last_ms()[2], 'out_bytes': csv_bytes, 'rows': g.counts()[1]}
    # and the select renderer over the same rows in a random order, one file
    order = np.random.RandomState(1).permutation(g.counts()[1]).astype(np.int64)
    sel_bytes = len(g.csv_select(order)[0])
    res['select_same_rows'] = {'select_last_ms': g.select_last_ms(), 'out_bytes': sel_bytes, 'rows': len(order)}
print('E2E_LINKS ' + json.dumps(res))
''' % (PARTS, PARTS)

ARTICLE = ('{k} Shares of the company rose, then fell.\n"We expect a better quarter," the chief executive said, '
           '"and a calmer one."\r\n\r\nAnalysts, on average, had expected {k} cents a share.\n') * 3
FIELDS = ["url", "datetime", "ticker_symbols", "author", "source", "source_url", "title", "article"]


def write_workload(folder, rows, seed):
    import random
    rng = random.Random(seed)
    # (no ',' in a link: to_csv would quote it, and a links file with '"' bytes takes the pandas route)
    urls = ['https://finance.yahoo.com/news/%s-%d.html' % (rng.choice(['earnings', 'markets', 'why-shares-fell', 'é']), k)
            for k in range(rows - rows // 10)]
    links = urls + [rng.choice(urls) for _ in range(rows // 10)]
    rng.shuffle(links)
    with open(os.path.join(folder, 'yahoo_links_1.csv'), 'w', newline='', encoding='utf-8') as fh:
        w = csv.writer(fh, lineterminator='\n')   # (what DataFrame.to_csv wrote)
        w.writerow(['date_time', 'url'])
        # timestamps to the minute over a few years: ties are common, as in a CDX harvest
        w.writerows((20200101000000 + rng.randrange(0, 2_000_000) * 100, u) for u in links)
    rng.shuffle(urls)
    n_prev = len(urls) // 2
    for name, part in (('yahoo_articles_all.csv', urls[:n_prev]),
                       ('success_articles_yfin.csv', urls[n_prev:n_prev + (len(urls) - n_prev) // 5])):
        with open(os.path.join(folder, name), 'w', newline='', encoding='utf-8') as fh:
            w = csv.writer(fh)
            w.writerow(FIELDS)
            w.writerows((u, '2024-01-02 03:04:05', 'AAPL, MSFT', 'A. Writer', 'Wire', 'https://wire/',
                         'A "title", quoted', ARTICLE.format(k=k)) for k, u in enumerate(part))
    return {f: os.path.getsize(os.path.join(folder, f)) for f in sorted(os.listdir(folder))}


def run_config(folder, env_extra, runs, tree=REPO):
    env = dict(os.environ)
    for k in ('KW_LINKS_NATIVE', 'E2E_STREAM_FROM', 'E2E_WINDOW_BYTES'):
        env.pop(k, None)
    env.update(env_extra)
    got = []
    for _ in range(runs + 1):   # the first is the warm-up
        p = subprocess.run([sys.executable, '-c', CHILD, tree, folder], env=env, cwd=tree, capture_output=True,
                           text=True, timeout=1500)
        if p.returncode != 0:
            raise RuntimeError(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('E2E_LINKS ')][-1]
        got.append(json.loads(line[len('E2E_LINKS '):]))
        print('%s run %d: refresh %.3f s, split %.3f s' % (env_extra or 'native', len(got) - 1, got[-1]['refresh_s'],
                                                          got[-1]['split_s']), file=sys.stderr, flush=True)
    timed = got[1:]
    assert len({r['sha256'] for r in got}) == 1, 'runs of one configuration wrote different bytes'
    last = timed[-1]
    res = {'env': env_extra, 'routes': last['routes'], 'refresh_counts': last['refresh_counts'],
           'split_counts': last['split_counts'], 'split_parts': last['split_parts'], 'sha256': last['sha256'],
           'out_bytes': last['out_bytes'], 'windows': last['windows'],
           'peak_rss_MB': max(r['maxrss_kb'] for r in timed) / 1024.0}
    for key in ('refresh_s', 'split_s'):
        v = [r[key] for r in timed]
        res[key] = {'runs': v, 'median_s': statistics.median(v), 'min_s': min(v), 'max_s': max(v)}
    if 'refresh_spans' in last:
        mid = sorted(timed, key=lambda r: r['refresh_s'])[len(timed) // 2]   # the median run's device times
        for call in ('refresh', 'split'):
            s = mid[call + '_spans']
            res[call + '_device_ms'] = dict(zip(('parse', 'parse_compaction'), s['cdx_last_ms'][:2]))
            res[call + '_device_ms'].update(zip(('keep_first_run', 'set_difference_pass', 'remaining_compaction'),
                                                s['exclude_last_ms']))
            res[call + '_device_ms'].update(zip(('select_size', 'select_copy'), s['select_last_ms']))
        v = [r['argsort_s'] for r in timed]
        res['host_argsort_s'] = {'runs': v, 'median_s': statistics.median(v), 'min_s': min(v), 'max_s': max(v)}
        res['row_order'] = mid['row_order']
        res['select_same_rows'] = mid['select_same_rows']
    return res


def stream_main(args):
    """--stream: the streamed route against the one-piece route (and the parent's, and pandas)."""
    out = args.out or os.path.join(REPO, 'profiles', 'e2e_links_stream.json')
    with tempfile.TemporaryDirectory(prefix='e2e_links_', dir=args.tmp) as tmp:
        sizes = write_workload(tmp, args.rows, args.seed)
        res = {'rows': args.rows, 'seed': args.seed, 'num_parts': PARTS, 'input_bytes': sizes,
               'runs_per_config': args.runs,
               'timed': 'links.refresh_links() and links.split_links() in a fresh child per run, GPU initialised and '
                        'handle created before the clocks; 1 warm-up + the median of the runs; the configurations one '
                        'after the other in one call'}
        configs = [('one_piece', {'E2E_STREAM_FROM': str(1 << 62)}, REPO), ('streamed', {'E2E_STREAM_FROM': '0'}, REPO),
                   ('streamed_64MiB', {'E2E_STREAM_FROM': '0', 'E2E_WINDOW_BYTES': str(64 << 20)}, REPO)]
        if args.parent_tree:
            configs.append(('parent', {}, os.path.abspath(args.parent_tree)))
        if args.pandas:
            configs.append(('pandas', {'KW_LINKS_NATIVE': '0'}, REPO))
        for name, env, tree in configs:
            res[name] = run_config(tmp, env, args.runs, tree)
    res['same_result'] = len({res[name]['sha256'] for name, _, _ in configs}) == 1
    for call in ('refresh', 'split'):
        res['streamed_over_one_piece_' + call] = (res['streamed'][call + '_s']['median_s'] /
                                                  res['one_piece'][call + '_s']['median_s'])
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))
    if not res['same_result']:
        sys.exit('the configurations wrote different bytes')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--seed', type=int, default=20240229)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--stream', action='store_true', help='measure the streamed route (see above)')
    ap.add_argument('--parent-tree', default=None, help='--stream: a built checkout of the parent commit')
    ap.add_argument('--pandas', action='store_true', help='--stream: the pandas route too')
    ap.add_argument('--tmp', default=None, help='--stream: where the workload is written')
    args = ap.parse_args()
    if args.stream:
        return stream_main(args)
    args.out = args.out or os.path.join(REPO, 'profiles', 'e2e_links.json')
    with tempfile.TemporaryDirectory(prefix='e2e_links_') as tmp:
        sizes = write_workload(tmp, args.rows, args.seed)
        res = {'rows': args.rows, 'seed': args.seed, 'num_parts': PARTS, 'input_bytes': sizes,
               'runs_per_config': args.runs,
               'timed': 'links.refresh_links() and links.split_links() in a fresh child per run, GPU initialised and '
                        'handle created before the clocks; 1 warm-up + the median of the runs'}
        res['native'] = run_config(tmp, {}, args.runs)
        res['pandas'] = run_config(tmp, {'KW_LINKS_NATIVE': '0'}, args.runs)
    assert res['native']['routes'] == ['device', 'device'], 'the device route did not run'
    res['same_result'] = (res['native']['sha256'] == res['pandas']['sha256'] and
                          res['native']['refresh_counts'] == res['pandas']['refresh_counts'] and
                          res['native']['split_counts'] == res['pandas']['split_counts'])
    res['baseline'] = 'pandas'
    for call in ('refresh', 'split'):
        res['speedup_' + call] = res['pandas'][call + '_s']['median_s'] / res['native'][call + '_s']['median_s']
    # bytes in + out of a render over its copy time: every output byte is read once from the kept rows (the URL, or
    # the 8-byte timestamp behind the digits) and written once, plus 24 bytes a line of offsets and sources
    peak = 8e12
    # (both over the size pass + the copy pass: kw_cdx_last_ms [2] is their sum)
    for key, ms_of in (('select_same_rows', lambda r: sum(r['select_last_ms'])), ('row_order', lambda r: r['render_ms'])):
        r = res['native'][key]
        moved = 2 * r['out_bytes'] + 24 * r['rows']
        r['bytes_in_out'] = moved
        r['GBps'] = moved / (ms_of(r) / 1e3) / 1e9
        r['of_8TBps_peak'] = moved / (ms_of(r) / 1e3) / peak
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))
    if not res['same_result']:
        sys.exit('the two routes wrote different bytes')


if __name__ == '__main__':
    main()
