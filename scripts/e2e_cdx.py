"""End-to-end timing of the CDX drop-in's ``process_part``: this tree against a checkout of its parent commit.

Writes one synthetic CDX listing (csrc/synth.c rows as ``UrlRows.cdx_text``) and times
``cdx_dedup.process_part(listing, csv)`` on it, in a fresh child process per run (one warm-up, then the median
of 5; a child initialises the GPU and creates the dedup handle before its clock starts, and nothing is exec'd
after that).  Three configurations:

    native   this tree, the device parse + render route (the default)
    pandas   this tree with KW_CDX_NATIVE=0 (pandas parse, per-row pack, pandas to_csv)
    parent   --parent-tree: a built checkout of the parent commit, e.g.
                 git worktree add /tmp/parent HEAD~1 && (cd /tmp/parent && python -m advanced_scrapper_amd.build)

All of them must write the same bytes.  The result goes to --out (profiles/e2e_cdx.json) and, as one JSON line,
to stdout: per configuration the median, min and max seconds; for the native route kw_cdx_last_ms and the
listing's bytes over the parse + compaction time.

    python scripts/e2e_cdx.py --parent-tree /tmp/parent [--rows 1000000] [--out profiles/e2e_cdx.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import hashlib, json, sys, time
tree, txt, out = sys.argv[1:4]
sys.path.insert(0, tree)
import torch
from advanced_scrapper_amd import cdx_dedup
torch.cuda.init()
g = cdx_dedup._dedup()
torch.cuda.synchronize()
t0 = time.perf_counter()
cdx_dedup.process_part(txt, out)
t1 = time.perf_counter()
res = {'seconds': t1 - t0, 'sha256': hashlib.sha256(open(out, 'rb').read()).hexdigest(),
       'module': cdx_dedup.__file__}
if hasattr(g, 'cdx_last_ms'):
    res['cdx_last_ms'] = g.cdx_last_ms()
    res['dedup_last_ms'] = g.last_ms()
print('E2E_CDX ' + json.dumps(res))
'''


def run_config(tree, txt, out, env_extra, runs):
    env = dict(os.environ)
    env.pop('KW_CDX_NATIVE', None)
    env.update(env_extra)
    got = []
    for _ in range(runs + 1):   # the first is the warm-up
        p = subprocess.run([sys.executable, '-c', CHILD, tree, txt, out], env=env, cwd=tree, capture_output=True,
                           text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"child failed ({p.returncode}) in {tree}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('E2E_CDX ')][-1]
        got.append(json.loads(line[len('E2E_CDX '):]))
    timed = got[1:]
    secs = [r['seconds'] for r in timed]
    res = {'tree': os.path.abspath(tree), 'env': env_extra, 'runs': secs, 'median_s': statistics.median(secs),
           'min_s': min(secs), 'max_s': max(secs), 'sha256': timed[-1]['sha256']}
    assert len({r['sha256'] for r in got}) == 1, 'runs of one configuration wrote different bytes'
    if 'cdx_last_ms' in timed[-1]:
        by_run = sorted(timed, key=lambda r: r['seconds'])[len(timed) // 2]   # the median run's device times
        res['cdx_last_ms'] = dict(zip(('parse', 'compaction', 'render'), by_run['cdx_last_ms']))
        res['dedup_last_ms_total'] = by_run['dedup_last_ms'][4]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--seed', type=int, default=20240229)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'e2e_cdx.json'))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from advanced_scrapper_amd import synth
    with tempfile.TemporaryDirectory(prefix='e2e_cdx_') as tmp:
        txt = os.path.join(tmp, 'yahoo_AA.txt')
        rows = synth.generate_urls(args.rows, seed=args.seed)
        step = 100_000
        with open(txt, 'w', encoding='utf-8') as fh:
            for lo in range(0, args.rows, step):
                fh.write(rows.cdx_text(lo, min(args.rows, lo + step)))
        del rows
        n_bytes = os.path.getsize(txt)
        res = {'rows': args.rows, 'seed': args.seed, 'listing_bytes': n_bytes, 'runs_per_config': args.runs,
               'timed': 'process_part(listing, csv) in a fresh child per run, GPU initialised and handle created '
                        'before the clock; 1 warm-up + the median of the runs'}
        res['native'] = run_config(REPO, txt, os.path.join(tmp, 'native.csv'), {}, args.runs)
        res['pandas'] = run_config(REPO, txt, os.path.join(tmp, 'pandas.csv'), {'KW_CDX_NATIVE': '0'}, args.runs)
        if args.parent_tree:
            res['parent'] = run_config(args.parent_tree, txt, os.path.join(tmp, 'parent.csv'), {}, args.runs)
            res['parent']['tree'] = 'the parent commit (--parent-tree)'
        res['native']['tree'] = res['pandas']['tree'] = 'this tree'
    ms = res['native'].get('cdx_last_ms')
    assert ms, 'the native route did not run (no kw_cdx_last_ms)'
    res['parse_compaction_GBps'] = n_bytes / ((ms['parse'] + ms['compaction']) / 1e3) / 1e9
    shas = {res[k]['sha256'] for k in ('native', 'pandas', 'parent') if k in res}
    res['same_bytes'] = len(shas) == 1
    base = res.get('parent', res['pandas'])
    spread = max(res['native']['max_s'] - res['native']['min_s'], base['max_s'] - base['min_s'])
    res['baseline'] = 'parent' if 'parent' in res else 'pandas'
    res['native_no_slower'] = res['native']['median_s'] <= base['median_s'] + spread
    res['speedup_vs_baseline'] = base['median_s'] / res['native']['median_s']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))
    if not res['same_bytes']:
        sys.exit('the configurations wrote different bytes')


if __name__ == '__main__':
    main()
