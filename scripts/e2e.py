"""End-to-end drop-in timing: ``match_keywords.main`` itself over N synthetic articles, then a per-phase split.

Generates N articles of the config-2 corpus (csrc/synth.c, bench seed), writes them as the reference's article
CSV and the reference's KB JSON files (tests/golden/kb_bundle.json.gz, the reference's info/ticker) into a
scratch directory, and times ``python -m advanced_scrapper_amd.match_keywords --info-dir ... --articles ...``'s
``main()`` in-process from its first line to its return: KB load (read_and_process_json_files, prints
included), KB compile + kw_compile, native CSV ingest, GPU matching, JSON cells, row rendering, the appends
and the final sort (match_keywords.py:220-246).  A second pass over the same CSV runs main's per-chunk phases
one by one (read, dates, arena, GPU, render, write, sort) for the split; both passes must write the same
bytes.  One JSON line: end-to-end articles/s of main(), the split, the host threads.

    python scripts/e2e.py [--docs 200000] [--chunksize 20000]

``--rows-ab OUT.json`` compares the routes of the JSON cells (step a10) instead: ``main()`` over the same CSV in a
fresh child process per run (one warm-up, then the median of 5), on this tree with the device route
(csrc/kwrows.hip), on this tree with ``KW_ROWS_DEVICE=0`` (the lexsort + libkwrows on the host) and, with
``--parent-tree DIR`` (a built checkout of the parent commit), on that tree.  Every configuration must write the
same bytes.  OUT.json gets the three medians, the device route's ``kw_rows_last_ms`` split summed over the
chunks (order, expand, render) and the wall time either route spent building the cells.

``--emit-ab OUT.json`` compares the routes of the CSV rows the same way: this tree with ``KW_EMIT_DEVICE=1`` (the
lines rendered on the device, csrc/kwemit.hip), this tree with ``KW_EMIT_DEVICE=0`` (kwcsv_emit_mt on the host) and,
with ``--parent-tree DIR``, that tree.  OUT.json gets the medians, the wall time inside either renderer, and the
device route's per-chunk ``kw_rows_emit_last_ms`` (order, measure, fill, copy).

``--ingest-ab OUT.json`` compares the routes of the article ingest the same way: this tree with ``KW_INGEST_DEVICE=1``
(the CSV tokenized on the device, csrc/kwingest.hip), this tree with ``KW_INGEST_DEVICE=0`` (csrc/kwcsv.c on the
host threads) and, with ``--parent-tree DIR``, that tree.  OUT.json gets the medians and ranges, the wall time of the
ingest span per chunk (device: staging, upload and kw_ingest_parse on the main thread; host: the tokenizer on its
prefetch thread, overlapped with the matching), the ``kw_ingest_last_ms`` sums, the parse rate, and which route the
standing rule makes the default.

``--dates-ab OUT.json`` compares the routes of the article dates the same way on N articles whose dates are written
``YYYY-MM-DDTHH:MM:SS.000Z`` (synth.to_dataframe's ``'z_ms'``): this tree (the ISO rule on the device), this tree with
``KW_DATES_ISO=0`` (every such row through dateutil) and, with ``--parent-tree DIR``, that tree; then the ``'naive'``
layout on this tree against the parent, which guards the 19-byte path.  OUT.json gets the medians and ranges, the
wall time inside ``chunk.dates()``, ``dates_slow`` and the ``kw_ingest_last_ms`` sums, the ``dates`` and ``arena``
spans also per timed run (their own run-to-run spread).

``--tz-ab OUT.json`` compares the routes of ``time_unix`` the same way on N articles in the 19-byte naive layout, in
children that run under ``TZ=EST5EDT,M3.2.0,M11.1.0``: this tree (the stamps from the zone table, on the device),
this tree with ``KW_STAMPS_NATIVE=0`` (one ``timestamp()`` per rendered document) and, with ``--parent-tree DIR``, that
tree; then under ``TZ=UTC`` this tree against the parent.  OUT.json gets the medians and ranges, the sha256 of the
output, the wall time of the stamp step, ``stamps_slow``, the stamps kernel's time and the table's build time.

``--sort-ab OUT.json`` compares the routes of the final sort on a re-run: an untimed first ``main()`` over N articles
fills an output directory; the timed part is a second ``main()`` over another N articles into a copy of that
directory, so every file the first run left takes sort_matched_csv's re-read, sort and rewrite.  A fresh child per
run, the configurations in turn (one warm-up each, then the median and range of 5): this tree with
``KW_SORT_DEVICE=1`` (csrc/kwsort.hip), this tree with ``KW_SORT_DEVICE=0`` (match_keywords._sort_native and pandas)
and, with ``--parent-tree DIR``, that tree.  OUT.json gets the medians and ranges, the wall time of the final sort
loop on each route, the ``kw_sort_last_ms`` sums, the parse and gather rates, the gather kernel's share of the HBM
peak, the route counts, and which route the standing rule makes the default.

``--finish-ab OUT.json`` compares the routes by which a first ``main()`` finishes the files it wrote itself
(egress.RunFiles.finish) when the articles' dates do not follow the articles: N articles written newest first, and
the same N with ``date_perm`` dates.  A fresh child per run, the configurations in turn (one warm-up each, then the
median and range of 5): this tree (the rewrite on the device from the write index), this tree with
``KW_FINISH_DEVICE=0`` (the host branch) and, with ``--parent-tree DIR``, that tree.  OUT.json gets the whole run's
wall time and the wall time inside ``RunFiles.finish``, the files by route, the ``kw_sort_last_ms`` sums, the
process's peak resident size, and which route the standing rule makes the default; then the ascending corpus on this
tree and the parent, where the finish loop must make no device call.
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _digest(out_dir):
    h = hashlib.sha256()
    for fn in sorted(os.listdir(out_dir)):
        h.update(fn.encode())
        with open(os.path.join(out_dir, fn), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def phases(args, csv_path, processed):
    """main()'s per-chunk steps timed one by one (the split; same writes as main)."""
    from advanced_scrapper_amd import egress, ingest, match_keywords as mk
    t = dict(read=0.0, dates=0.0, arena=0.0, gpu_match=0.0, render=0.0, write=0.0, sort=0.0)
    os.makedirs('yahoo_ticker_matched_articles')
    mk._RUN = egress.RunFiles('yahoo_ticker_matched_articles')
    matcher = None
    c0 = time.perf_counter()
    for chunk in ingest.read_chunks(csv_path, args.chunksize):
        c1 = time.perf_counter(); t['read'] += c1 - c0
        if not isinstance(chunk, ingest.NativeChunk):
            matcher = mk._write_chunk('yahoo', chunk, processed, matcher)
            c0 = time.perf_counter(); t['write'] += c0 - c1
            continue
        dates, error = chunk.dates()
        c2 = time.perf_counter(); t['dates'] += c2 - c1
        if matcher is None:
            matcher = mk.get_matcher(processed, 0, mk._native_sample(chunk))
        c2 = time.perf_counter()
        arena, off = chunk.arena()
        off = off[:2 * len(dates) + 1]
        c3 = time.perf_counter(); t['arena'] += c3 - c2
        matcher.scan_host(arena, off, len(dates))
        hits = matcher.fetch_host()
        c4 = time.perf_counter(); t['gpu_match'] += c4 - c3
        rendered, exc, _row = mk._native_rows(chunk, matcher, hits, dates, error)
        c5 = time.perf_counter(); t['render'] += c5 - c4
        egress.append_rendered('yahoo_ticker_matched_articles', rendered, mk._RUN)
        c0 = time.perf_counter(); t['write'] += c0 - c5
    c7 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for name in os.listdir('yahoo_ticker_matched_articles'):
            if not mk._RUN.finish(name):
                mk.sort_matched_csv(f'yahoo_ticker_matched_articles/{name}')
    t['sort'] = time.perf_counter() - c7
    mk._RUN = None
    return {k: round(v, 3) for k, v in t.items()}


ROWS_CHILD = r'''
import contextlib, hashlib, io, json, os, sys, tempfile, time
tree, info_dir, csv_path, chunksize = sys.argv[1:5]
sys.path.insert(0, tree)
os.environ.setdefault('TZ', 'UTC')
time.tzset()
from advanced_scrapper_amd import match_keywords as mk
span = {'device_s': 0.0, 'host_s': 0.0, 'device_calls': 0, 'host_calls': 0, 'order': 0.0, 'expand': 0.0, 'render': 0.0}
host = mk.assemble_json_raw
def timed_host(ckb, hits, dates):
    t = time.perf_counter()
    out = host(ckb, hits, dates)
    span['host_s'] += time.perf_counter() - t
    span['host_calls'] += 1
    return out
mk.assemble_json_raw = timed_host
device = getattr(mk, 'assemble_json_device', None)      # (the parent tree has none)
if device is not None:
    def timed_device(matcher, dates):
        t = time.perf_counter()
        out = device(matcher, dates)
        span['device_s'] += time.perf_counter() - t
        span['device_calls'] += 1
        for k, v in matcher.rows_handle().last_ms().items():
            if k in span:
                span[k] += v
        return out
    mk.assemble_json_device = timed_device
work = tempfile.mkdtemp(prefix='e2e_rows_')
os.chdir(work)
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()):
    rc = mk.main(['--info-dir', info_dir, '--articles', csv_path, '--chunksize', chunksize, '--device', '0'])
total = time.perf_counter() - t0
assert rc == 0
h = hashlib.sha256()
out = os.path.join(work, 'yahoo_ticker_matched_articles')
for fn in sorted(os.listdir(out)):
    h.update(fn.encode())
    with open(os.path.join(out, fn), 'rb') as fh:
        h.update(fh.read())
import shutil
os.chdir(tree)
shutil.rmtree(work, ignore_errors=True)
print('E2E_ROWS ' + json.dumps({'seconds': total, 'sha256': h.hexdigest(), 'span': span}))
'''


EMIT_CHILD = r'''
import contextlib, hashlib, io, json, os, sys, tempfile, time
tree, info_dir, csv_path, chunksize = sys.argv[1:5]
sys.path.insert(0, tree)
os.environ.setdefault('TZ', 'UTC')
time.tzset()
from advanced_scrapper_amd import egress, match_keywords as mk
span = {'device_s': 0.0, 'host_s': 0.0, 'device_calls': 0, 'host_calls': 0, 'emit_ms': [], 'bytes': 0}
host = egress.render_native
def timed_host(*a):
    t = time.perf_counter()
    out = host(*a)
    span['host_s'] += time.perf_counter() - t
    span['host_calls'] += 1
    return out
egress.render_native = timed_host
device = getattr(egress, 'render_device', None)      # (the parent tree has none)
if device is not None:
    def timed_device(chunk, matcher, stamps, k, *more):
        t = time.perf_counter()
        out = device(chunk, matcher, stamps, k, *more)
        span['device_s'] += time.perf_counter() - t
        span['device_calls'] += 1
        if k and out is not None:
            span['emit_ms'].append({n: round(v, 3) for n, v in matcher.rows_handle().emit_last_ms().items()})
            span['bytes'] += sum(len(r[1]) for r in out)
        return out
    egress.render_device = timed_device
work = tempfile.mkdtemp(prefix='e2e_emit_')
os.chdir(work)
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()):
    rc = mk.main(['--info-dir', info_dir, '--articles', csv_path, '--chunksize', chunksize, '--device', '0'])
total = time.perf_counter() - t0
assert rc == 0
h = hashlib.sha256()
out = os.path.join(work, 'yahoo_ticker_matched_articles')
for fn in sorted(os.listdir(out)):
    h.update(fn.encode())
    with open(os.path.join(out, fn), 'rb') as fh:
        h.update(fh.read())
import shutil
os.chdir(tree)
shutil.rmtree(work, ignore_errors=True)
print('E2E_ROWS ' + json.dumps({'seconds': total, 'sha256': h.hexdigest(), 'span': span}))
'''


INGEST_CHILD = r'''
import contextlib, hashlib, io, json, os, sys, tempfile, time
tree, info_dir, csv_path, chunksize = sys.argv[1:5]
sys.path.insert(0, tree)
os.environ.setdefault('TZ', 'UTC')
time.tzset()
from advanced_scrapper_amd import ingest, match_keywords as mk
span = {'device_calls': 0, 'host_calls': 0, 'host_s': 0.0, 'device_s': 0.0, 'chunks': 0, 'bytes': 0,
        'classify': 0.0, 'cells': 0.0, 'arena': 0.0, 'all': 0.0, 'routes': {}}
host = ingest.read_chunks
def timed_host(path, chunksize):
    span['host_calls'] += 1
    it = host(path, chunksize)
    while True:
        t = time.perf_counter()
        try:
            chunk = next(it)
        except StopIteration:
            return
        span['host_s'] += time.perf_counter() - t
        span['chunks'] += 1
        yield chunk
ingest.read_chunks = timed_host
device = getattr(ingest, 'read_chunks_device', None)      # (the parent tree has none)
if device is not None:
    def counted_device(*a, **kw):
        span['device_calls'] += 1
        return device(*a, **kw)
    ingest.read_chunks_device = counted_device
work = tempfile.mkdtemp(prefix='e2e_ingest_')
os.chdir(work)
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()):
    rc = mk.main(['--info-dir', info_dir, '--articles', csv_path, '--chunksize', chunksize, '--device', '0'])
total = time.perf_counter() - t0
assert rc == 0
st = getattr(ingest, 'LAST_STATS', None)
if st is not None:
    span['device_s'] = st['wall_s']
    span['chunks'] = st['device'] + st['host'] + st['pandas']
    span['bytes'] = st['bytes']
    span['routes'] = {k: st[k] for k in ('device', 'host', 'pandas', 'grown', 'reused')}
    span['wall_ms'] = st['wall_ms']
    for m in st['ms']:
        for k in ('classify', 'cells', 'arena', 'all'):
            span[k] += m[k]
h = hashlib.sha256()
out = os.path.join(work, 'yahoo_ticker_matched_articles')
for fn in sorted(os.listdir(out)):
    h.update(fn.encode())
    with open(os.path.join(out, fn), 'rb') as fh:
        h.update(fh.read())
import shutil
os.chdir(tree)
shutil.rmtree(work, ignore_errors=True)
print('E2E_ROWS ' + json.dumps({'seconds': total, 'sha256': h.hexdigest(), 'span': span}))
'''


DATES_CHILD = r'''
import contextlib, hashlib, io, json, os, sys, tempfile, time
tree, info_dir, csv_path, chunksize = sys.argv[1:5]
sys.path.insert(0, tree)
os.environ.setdefault('TZ', 'UTC')
time.tzset()
from advanced_scrapper_amd import ingest, match_keywords as mk
span = {'dates_s': 0.0, 'dates_calls': 0, 'dates_slow': None, 'arena': 0.0, 'all': 0.0, 'chunks': 0}
def timed(cls):
    inner = cls.dates
    def dates(self):
        t = time.perf_counter()
        out = inner(self)
        span['dates_s'] += time.perf_counter() - t
        span['dates_calls'] += 1
        return out
    cls.dates = dates
timed(ingest.NativeChunk)
timed(ingest.DeviceChunk)
work = tempfile.mkdtemp(prefix='e2e_dates_')
os.chdir(work)
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()):
    rc = mk.main(['--info-dir', info_dir, '--articles', csv_path, '--chunksize', chunksize, '--device', '0'])
total = time.perf_counter() - t0
assert rc == 0
st = ingest.LAST_STATS
span['dates_slow'] = st.get('dates_slow')      # (the parent tree does not count them)
span['chunks'] = st['device'] + st['host'] + st['pandas']
assert st['device'] == span['chunks'] > 0
for m in st['ms']:
    for k in ('arena', 'all'):
        span[k] += m[k]
h = hashlib.sha256()
out = os.path.join(work, 'yahoo_ticker_matched_articles')
for fn in sorted(os.listdir(out)):
    h.update(fn.encode())
    with open(os.path.join(out, fn), 'rb') as fh:
        h.update(fh.read())
import shutil
os.chdir(tree)
shutil.rmtree(work, ignore_errors=True)
print('E2E_ROWS ' + json.dumps({'seconds': total, 'sha256': h.hexdigest(), 'span': span}))
'''


TZ_CHILD = r'''
import contextlib, hashlib, io, json, os, sys, tempfile, time
tree, info_dir, csv_path, chunksize = sys.argv[1:5]
sys.path.insert(0, tree)
os.environ.setdefault('TZ', 'UTC')
time.tzset()
from advanced_scrapper_amd import egress, ingest, match_keywords as mk
span = {'rows_s': 0.0, 'inner_s': 0.0, 'calls': 0}
def timed(mod, name, key):
    inner = getattr(mod, name)
    def fn(*a, **kw):
        t = time.perf_counter()
        try:
            return inner(*a, **kw)
        finally:
            span[key] += time.perf_counter() - t
    setattr(mod, name, fn)
# the stamp step = _native_rows without the calls that build the JSON cells and render the rows
timed(mk, '_native_rows', 'rows_s')
for mod, name in ((mk, 'assemble_json_device'), (mk, '_json_raw'), (egress, 'render_device'), (egress, 'render_native')):
    timed(mod, name, 'inner_s')
work = tempfile.mkdtemp(prefix='e2e_tz_')
os.chdir(work)
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()):
    rc = mk.main(['--info-dir', info_dir, '--articles', csv_path, '--chunksize', chunksize, '--device', '0'])
total = time.perf_counter() - t0
assert rc == 0
st = ingest.LAST_STATS
span['chunks'] = st['device'] + st['host'] + st['pandas']
assert st['device'] == span['chunks'] > 0
span['stamp_step_s'] = span['rows_s'] - span['inner_s']
span['stamps_slow'] = st.get('stamps_slow')          # (the parent tree does not count them)
span['stamps_kernel_ms'] = sum(st['stamps_ms']) if 'stamps_ms' in st else None      # kw_ingest_last_ms[4] over the chunks
span['arena_ms'] = sum(m['arena'] for m in st['ms'])
zone = sys.modules.get('advanced_scrapper_amd.zone')      # (the parent tree has none)
span['zone_build_ms'] = zone.LAST_BUILD_MS if zone is not None else None
span['zone_entries'] = (len(zone.table()[1]) if zone.table() is not None else 0) if zone is not None else None
span['tz'] = os.environ['TZ']
h = hashlib.sha256()
out = os.path.join(work, 'yahoo_ticker_matched_articles')
for fn in sorted(os.listdir(out)):
    h.update(fn.encode())
    with open(os.path.join(out, fn), 'rb') as fh:
        h.update(fh.read())
import shutil
os.chdir(tree)
shutil.rmtree(work, ignore_errors=True)
print('E2E_ROWS ' + json.dumps({'seconds': total, 'sha256': h.hexdigest(), 'span': span}))
'''


SORT_CHILD = r'''
import contextlib, hashlib, io, json, os, shutil, sys, tempfile, time
tree, info_dir, csv_path, chunksize, seed_dir = sys.argv[1:6]
sys.path.insert(0, tree)
os.environ.setdefault('TZ', 'UTC')
time.tzset()
from advanced_scrapper_amd import match_keywords as mk
span = {'sort_calls': 0, 'sort_s': 0.0}
inner = mk.sort_matched_csv
def timed_sort(*a, **kw):
    t = time.perf_counter()
    out = inner(*a, **kw)
    span['sort_s'] += time.perf_counter() - t
    span['sort_calls'] += 1
    return out
mk.sort_matched_csv = timed_sort
work = tempfile.mkdtemp(prefix='e2e_sort_')
out = os.path.join(work, 'yahoo_ticker_matched_articles')
shutil.copytree(seed_dir, out)                       # (the first run's files: not timed)
os.chdir(work)
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()) as log:
    rc = mk.main(['--info-dir', info_dir, '--articles', csv_path, '--chunksize', chunksize, '--device', '0'])
total = time.perf_counter() - t0
assert rc == 0 and 'Error processing' not in log.getvalue()
sf = sys.modules.get('advanced_scrapper_amd.sortfiles')      # (the parent tree has none)
if sf is not None:
    st = sf.LAST_STATS
    span['stats'] = {k: st[k] for k in ('device', 'unchanged', 'native', 'pandas', 'refused', 'bytes', 'gather_bytes',
                                        'prefetched', 'ms', 'wall_s')}
    span['loop_s'] = st.get('loop_s')
h = hashlib.sha256()
for fn in sorted(os.listdir(out)):
    h.update(fn.encode())
    with open(os.path.join(out, fn), 'rb') as fh:
        h.update(fh.read())
os.chdir(tree)
shutil.rmtree(work, ignore_errors=True)
print('E2E_ROWS ' + json.dumps({'seconds': total, 'sha256': h.hexdigest(), 'span': span}))
'''


FINISH_CHILD = r'''
import contextlib, hashlib, io, json, os, resource, shutil, sys, tempfile, time
tree, info_dir, csv_path, chunksize = sys.argv[1:5]
sys.path.insert(0, tree)
os.environ.setdefault('TZ', 'UTC')
time.tzset()
from advanced_scrapper_amd import egress, match_keywords as mk
span = {'finish_calls': 0, 'finish_s': 0.0}
inner = egress.RunFiles.finish
def timed_finish(self, name):
    t = time.perf_counter()
    out = inner(self, name)
    span['finish_s'] += time.perf_counter() - t
    span['finish_calls'] += 1
    return out
egress.RunFiles.finish = timed_finish
work = tempfile.mkdtemp(prefix='e2e_finish_')
os.chdir(work)
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()) as log:
    rc = mk.main(['--info-dir', info_dir, '--articles', csv_path, '--chunksize', chunksize, '--device', '0'])
total = time.perf_counter() - t0
assert rc == 0 and 'Error processing' not in log.getvalue()
span['maxrss_kib'] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
st = sys.modules['advanced_scrapper_amd.sortfiles'].LAST_STATS
span['stats'] = {k: st[k] for k in ('device', 'unchanged', 'native', 'pandas', 'indexed', 'index_host', 'refused', 'bytes',
                                    'gather_bytes', 'prefetched', 'windows', 'slabs', 'ms', 'wall_s') if k in st}
out = os.path.join(work, 'yahoo_ticker_matched_articles')
span['files'] = len(os.listdir(out))
span['out_bytes'] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
h = hashlib.sha256()
for fn in sorted(os.listdir(out)):
    h.update(fn.encode())
    with open(os.path.join(out, fn), 'rb') as fh:
        h.update(fh.read())
os.chdir(tree)
shutil.rmtree(work, ignore_errors=True)
print('E2E_ROWS ' + json.dumps({'seconds': total, 'sha256': h.hexdigest(), 'span': span}))
'''


def rows_config(tree, env_extra, info_dir, csv_path, chunksize, runs, child=ROWS_CHILD, span_runs=()):
    """main() in a fresh child per run on ``tree``: one warm-up, then ``runs`` timed runs."""
    import statistics
    import subprocess
    env = dict(os.environ)
    env.pop('KW_ROWS_DEVICE', None)
    env.pop('KW_EMIT_DEVICE', None)
    env.pop('KW_INGEST_DEVICE', None)
    env.pop('KW_INGEST_WINDOW', None)
    env.update(env_extra)
    got = []
    for _ in range(runs + 1):
        p = subprocess.run([sys.executable, '-c', child, tree, info_dir, csv_path, str(chunksize)], env=env,
                           cwd=tree, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError(f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('E2E_ROWS ')][-1]
        got.append(json.loads(line[len('E2E_ROWS '):]))
    timed = got[1:]
    assert len({r['sha256'] for r in got}) == 1, 'runs of one configuration wrote different bytes'
    v = [r['seconds'] for r in timed]
    mid = sorted(timed, key=lambda r: r['seconds'])[len(timed) // 2]      # the median run's spans
    out = {'env': env_extra, 'sha256': mid['sha256'], 'runs': v, 'median_s': statistics.median(v), 'min_s': min(v),
           'max_s': max(v), 'cells': mid['span']}
    for k in span_runs:                # these spans of every timed run, for their own run-to-run spread
        out[k + '_runs'] = [r['span'][k] for r in timed]
    return out


def rows_ab(args):
    import bench
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    info_dir = os.path.join(work, 'ticker')
    processed = bench.load_kb(info_dir)
    names, kinds = synth.injectable_names(compile_kb(processed))
    corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=0)
    csv_path = os.path.join(work, 'articles.csv')
    synth.to_dataframe(corpus).to_csv(csv_path, index=False)
    del corpus
    res = {'docs': args.docs, 'chunksize': args.chunksize, 'csv_bytes': os.path.getsize(csv_path),
           'runs_per_config': args.runs,
           'timed': 'match_keywords.main() wall time in a fresh child per run; 1 warm-up + the median of the runs; '
                    'cells: the median run\'s wall time inside the route that built the JSON cells (host: the '
                    'lexsort + kwrows_assemble_mt; device: kw_rows_run + kw_rows_copy) and the device times (ms) '
                    'of kw_rows_last_ms summed over the chunks'}
    try:
        res['device'] = rows_config(REPO, {'KW_ROWS_DEVICE': '1'}, info_dir, csv_path, args.chunksize, args.runs)
        res['host'] = rows_config(REPO, {'KW_ROWS_DEVICE': '0'}, info_dir, csv_path, args.chunksize, args.runs)
        if args.parent_tree:
            res['parent'] = rows_config(os.path.abspath(args.parent_tree), {}, info_dir, csv_path, args.chunksize,
                                        args.runs)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert res['device']['cells']['device_calls'] > 0 and res['device']['cells']['host_calls'] == 0
    assert res['host']['cells']['device_calls'] == 0 and res['host']['cells']['host_calls'] > 0
    res['same_bytes'] = len({res[k]['sha256'] for k in ('device', 'host', 'parent') if k in res}) == 1
    res['device_not_slower'] = res['device']['median_s'] <= res['host']['median_s']
    with open(args.rows_ab, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res), flush=True)
    assert res['same_bytes'], 'the configurations wrote different bytes'


def emit_ab(args):
    import bench
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    info_dir = os.path.join(work, 'ticker')
    processed = bench.load_kb(info_dir)
    names, kinds = synth.injectable_names(compile_kb(processed))
    corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=0)
    csv_path = os.path.join(work, 'articles.csv')
    synth.to_dataframe(corpus).to_csv(csv_path, index=False)
    del corpus
    res = {'docs': args.docs, 'chunksize': args.chunksize, 'csv_bytes': os.path.getsize(csv_path),
           'runs_per_config': args.runs,
           'timed': 'match_keywords.main() wall time in a fresh child per run; 1 warm-up + the median of the runs; '
                    'cells: the median run\'s wall time inside the renderer of the CSV rows (host: egress.render_native '
                    '= kwcsv_emit_mt; device: egress.render_device = kw_rows_cells + kw_rows_emit), the bytes the '
                    'device route rendered and its per-chunk kw_rows_emit_last_ms (ms)'}
    try:
        res['device'] = rows_config(REPO, {'KW_EMIT_DEVICE': '1'}, info_dir, csv_path, args.chunksize, args.runs, EMIT_CHILD)
        res['host'] = rows_config(REPO, {'KW_EMIT_DEVICE': '0'}, info_dir, csv_path, args.chunksize, args.runs, EMIT_CHILD)
        if args.parent_tree:
            res['parent'] = rows_config(os.path.abspath(args.parent_tree), {}, info_dir, csv_path, args.chunksize,
                                        args.runs, EMIT_CHILD)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert res['device']['cells']['device_calls'] > 0 and res['device']['cells']['host_calls'] == 0
    assert res['host']['cells']['device_calls'] == 0 and res['host']['cells']['host_calls'] > 0
    res['same_bytes'] = len({res[k]['sha256'] for k in ('device', 'host', 'parent') if k in res}) == 1
    res['device_faster'] = res['device']['median_s'] < res['host']['median_s']
    with open(args.emit_ab, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res), flush=True)
    assert res['same_bytes'], 'the configurations wrote different bytes'


def ingest_ab(args):
    import bench
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    info_dir = os.path.join(work, 'ticker')
    processed = bench.load_kb(info_dir)
    names, kinds = synth.injectable_names(compile_kb(processed))
    corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=0)
    csv_path = os.path.join(work, 'articles.csv')
    synth.to_dataframe(corpus).to_csv(csv_path, index=False)
    del corpus
    res = {'docs': args.docs, 'chunksize': args.chunksize, 'csv_bytes': os.path.getsize(csv_path),
           'runs_per_config': args.runs,
           'timed': 'match_keywords.main() wall time in a fresh child per run; 1 warm-up + the median of the runs; '
                    'cells: the median run\'s ingest span -- device_s: the wall time of staging, upload and '
                    'kw_ingest_parse on the main thread; host_s: the wall time the host tokenizer took on its prefetch '
                    'thread (overlapped with the matching) -- and the device times (ms) of kw_ingest_last_ms summed over '
                    'the chunks'}
    try:
        res['device'] = rows_config(REPO, {'KW_INGEST_DEVICE': '1'}, info_dir, csv_path, args.chunksize, args.runs, INGEST_CHILD)
        res['host'] = rows_config(REPO, {'KW_INGEST_DEVICE': '0'}, info_dir, csv_path, args.chunksize, args.runs, INGEST_CHILD)
        if args.parent_tree:
            res['parent'] = rows_config(os.path.abspath(args.parent_tree), {}, info_dir, csv_path, args.chunksize,
                                        args.runs, INGEST_CHILD)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    d, hst = res['device']['cells'], res['host']['cells']
    assert d['device_calls'] > 0 and d['host_calls'] == 0 and d['routes'].get('device', 0) == d['chunks'] > 0
    assert hst['device_calls'] == 0 and hst['host_calls'] > 0
    res['same_bytes'] = len({res[k]['sha256'] for k in ('device', 'host', 'parent') if k in res}) == 1
    res['ingest_span_ms_per_chunk'] = {'device': round(1e3 * d['device_s'] / d['chunks'], 3),
                                       'host': round(1e3 * hst['host_s'] / max(hst['chunks'], 1), 3)}
    res['parse_GBps'] = round(d['bytes'] / (d['all'] * 1e-3) / 1e9, 2) if d['all'] else None
    res['device_faster'] = res['device']['median_s'] < res['host']['median_s']
    res['default'] = 'device' if res['device_faster'] else 'host (the device route behind KW_INGEST_DEVICE=1)'
    with open(args.ingest_ab, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res), flush=True)
    assert res['same_bytes'], 'the configurations wrote different bytes'


def dates_ab(args):
    import bench
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    info_dir = os.path.join(work, 'ticker')
    processed = bench.load_kb(info_dir)
    names, kinds = synth.injectable_names(compile_kb(processed))
    corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=0)
    paths = {}
    for layout in ('z_ms', 'naive'):
        paths[layout] = os.path.join(work, f'articles_{layout}.csv')
        synth.to_dataframe(corpus, date_layout=layout).to_csv(paths[layout], index=False)
    del corpus
    res = {'docs': args.docs, 'chunksize': args.chunksize, 'runs_per_config': args.runs,
           'csv_bytes': {k: os.path.getsize(p) for k, p in paths.items()},
           'timed': 'match_keywords.main() wall time in a fresh child per run; 1 warm-up + the median of the runs, the '
                    'configurations in turn in one call; cells: the median run\'s wall time inside chunk.dates() '
                    '(dates_s), the rows that went to dateutil (dates_slow; the parent does not count them) and the '
                    'device times (ms) of kw_ingest_last_ms summed over the chunks (arena: arena + dates; all)'}
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    try:
        for layout in ('z_ms', 'naive'):
            r = res[layout] = {}
            r['iso'] = rows_config(REPO, {}, info_dir, paths[layout], args.chunksize, args.runs, DATES_CHILD, ('arena', 'dates_s'))
            if layout == 'z_ms':
                r['iso_off'] = rows_config(REPO, {'KW_DATES_ISO': '0'}, info_dir, paths[layout], args.chunksize, args.runs,
                                           DATES_CHILD, ('arena', 'dates_s'))
            if parent:
                r['parent'] = rows_config(parent, {}, info_dir, paths[layout], args.chunksize, args.runs, DATES_CHILD, ('arena', 'dates_s'))
            r['same_bytes'] = len({v['sha256'] for v in r.values()}) == 1
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert res['z_ms']['iso']['cells']['dates_slow'] == 0 == res['naive']['iso']['cells']['dates_slow']
    assert res['z_ms']['iso_off']['cells']['dates_slow'] == args.docs
    with open(args.dates_ab, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res), flush=True)
    assert res['z_ms']['same_bytes'] and res['naive']['same_bytes'], 'the configurations wrote different bytes'


TZ_AB_ZONE = 'EST5EDT,M3.2.0,M11.1.0'


def tz_ab(args):
    import bench
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    info_dir = os.path.join(work, 'ticker')
    processed = bench.load_kb(info_dir)
    names, kinds = synth.injectable_names(compile_kb(processed))
    corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=0)
    csv_path = os.path.join(work, 'articles.csv')
    synth.to_dataframe(corpus, date_layout='naive').to_csv(csv_path, index=False)
    del corpus
    res = {'docs': args.docs, 'chunksize': args.chunksize, 'runs_per_config': args.runs, 'zone': TZ_AB_ZONE,
           'csv_bytes': os.path.getsize(csv_path),
           'timed': 'match_keywords.main() wall time in a fresh child per run; 1 warm-up + the median of the runs, the '
                    'configurations in turn in one call; cells: the median run\'s wall time of the stamp step '
                    '(stamp_step_s: match_keywords._native_rows without the calls that build the JSON cells and '
                    'render the rows), the rendered documents whose time_unix came from a per-row timestamp() '
                    '(stamps_slow; the parent does not count them), kw_ingest_last_ms[4] summed over the chunks '
                    '(stamps_kernel_ms) and the zone table\'s build time (zone_build_ms, on the start-up thread)'}
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    spans = ('stamp_step_s',)

    def config(tree, env):
        out = rows_config(tree, env, info_dir, csv_path, args.chunksize, args.runs, TZ_CHILD, spans)
        print('tz-ab', os.path.relpath(tree, REPO), env, round(out['median_s'], 3), file=sys.stderr, flush=True)
        return out

    try:
        r = res['zone_runs'] = {}
        r['native'] = config(REPO, {'TZ': TZ_AB_ZONE})
        r['native_off'] = config(REPO, {'TZ': TZ_AB_ZONE, 'KW_STAMPS_NATIVE': '0'})
        if parent:
            r['parent'] = config(parent, {'TZ': TZ_AB_ZONE})
        r['same_bytes'] = len({v['sha256'] for v in r.values()}) == 1
        u = res['utc_runs'] = {}
        u['native'] = config(REPO, {'TZ': 'UTC'})
        if parent:
            u['parent'] = config(parent, {'TZ': 'UTC'})
        u['same_bytes'] = len({v['sha256'] for v in u.values()}) == 1
        if parent:
            u['inside_parent_spread'] = u['parent']['min_s'] <= u['native']['median_s'] <= u['parent']['max_s']
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(args.tz_ab, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res), flush=True)
    assert res['zone_runs']['native']['cells']['stamps_slow'] == 0
    assert res['zone_runs']['same_bytes'] and res['utc_runs']['same_bytes'], 'the configurations wrote different bytes'


def sort_ab(args):
    import statistics
    import subprocess
    import bench
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    info_dir = os.path.join(work, 'ticker')
    processed = bench.load_kb(info_dir)
    names, kinds = synth.injectable_names(compile_kb(processed))
    csvs = []
    for part in range(2):
        corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=part * args.docs)
        csvs.append(os.path.join(work, f'articles{part}.csv'))
        synth.to_dataframe(corpus).to_csv(csvs[-1], index=False)
        del corpus
    configs = [('device', REPO, {'KW_SORT_DEVICE': '1'}), ('host', REPO, {'KW_SORT_DEVICE': '0'})]
    if args.parent_tree:
        configs.append(('parent', os.path.abspath(args.parent_tree), {}))
    base = {k: v for k, v in os.environ.items() if k not in ('KW_SORT_DEVICE', 'KW_ROWS_DEVICE', 'KW_EMIT_DEVICE',
                                                             'KW_INGEST_DEVICE', 'KW_INGEST_WINDOW')}
    res = {'docs_per_run': args.docs, 'chunksize': args.chunksize, 'csv_bytes': [os.path.getsize(c) for c in csvs],
           'runs_per_config': args.runs,
           'timed': 'the second match_keywords.main() (another docs_per_run articles) into a copy of the directory an '
                    'untimed first main() filled; wall time in a fresh child per run, the configurations in turn; '
                    '1 warm-up + the median of the runs; sort_s: the median run\'s wall time inside sort_matched_csv '
                    '(the files the first run left), loop_s: that of run()\'s whole final loop; stats: '
                    'sortfiles.LAST_STATS of that run (ms: device times summed over the files; the copies to and '
                    'from the host are part of the wall times, not of the gather kernel\'s share of the HBM peak)'}
    try:
        # the first run, once: its directory is copied for every timed run
        seed = os.path.join(work, 'seed')
        os.makedirs(seed)
        p = subprocess.run([sys.executable, '-m', 'advanced_scrapper_amd.match_keywords', '--info-dir', info_dir,
                            '--articles', csvs[0], '--chunksize', str(args.chunksize), '--device', '0'],
                           env=dict(base, PYTHONPATH=REPO), cwd=seed, capture_output=True, text=True, timeout=1800)
        if p.returncode != 0:
            raise RuntimeError(f"the first run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        seed_dir = os.path.join(seed, 'yahoo_ticker_matched_articles')
        res['seed_files'] = len(os.listdir(seed_dir))
        res['seed_bytes'] = sum(os.path.getsize(os.path.join(seed_dir, f)) for f in os.listdir(seed_dir))
        got = {name: [] for name, _t, _e in configs}
        for _ in range(args.runs + 1):
            for name, tree, extra in configs:
                p = subprocess.run([sys.executable, '-c', SORT_CHILD, tree, info_dir, csvs[1], str(args.chunksize),
                                    seed_dir], env=dict(base, **extra), cwd=tree, capture_output=True, text=True,
                                   timeout=1800)
                if p.returncode != 0:
                    raise RuntimeError(f"{name}: child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                line = [ln for ln in p.stdout.splitlines() if ln.startswith('E2E_ROWS ')][-1]
                got[name].append(json.loads(line[len('E2E_ROWS '):]))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    for name, _tree, extra in configs:
        runs = got[name]
        assert len({r['sha256'] for r in runs}) == 1, f'{name}: runs wrote different bytes'
        timed = runs[1:]
        v = [r['seconds'] for r in timed]
        mid = sorted(timed, key=lambda r: r['seconds'])[len(timed) // 2]
        res[name] = {'env': extra, 'sha256': mid['sha256'], 'runs': v, 'median_s': statistics.median(v),
                     'min_s': min(v), 'max_s': max(v), 'sort': mid['span']}
    res['same_bytes'] = len({res[name]['sha256'] for name, _t, _e in configs}) == 1
    st = res['device']['sort']['stats']
    ms = st['ms']
    res['routes'] = {k: st[k] for k in ('device', 'unchanged', 'native', 'pandas', 'refused', 'prefetched')}
    res['parse_GBps'] = round(st['bytes'] / (ms['parse'] * 1e-3) / 1e9, 2) if ms['parse'] else None
    res['gather_GBps'] = round(st['gather_bytes'] / (ms['gather'] * 1e-3) / 1e9, 2) if ms['gather'] else None
    # the gather kernel reads every file byte it lays out and writes it once
    res['gather_share_of_hbm_peak'] = (round(2 * st['gather_bytes'] / (ms['gather'] * 1e-3) / 8e12, 4)
                                       if ms['gather'] else None)
    res['sort_wall_s'] = {name: res[name]['sort']['sort_s'] for name, _t, _e in configs}
    res['device_faster'] = res['device']['median_s'] < res['host']['median_s']
    res['default'] = 'device' if res['device_faster'] else 'host (the device route behind KW_SORT_DEVICE=1)'
    with open(args.sort_ab, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res), flush=True)
    assert res['same_bytes'], 'the configurations wrote different bytes'


def finish_ab(args):
    import math
    import statistics
    import bench
    from advanced_scrapper_amd import synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    info_dir = os.path.join(work, 'ticker')
    processed = bench.load_kb(info_dir)
    names, kinds = synth.injectable_names(compile_kb(processed))
    corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=0)
    mult = 3_000_017
    while math.gcd(mult, args.docs) != 1:
        mult += 2
    csvs = {k: os.path.join(work, f'articles_{k}.csv') for k in ('newest_first', 'date_perm', 'ascending')}
    frame = synth.to_dataframe(corpus)
    frame.to_csv(csvs['ascending'], index=False)
    frame.iloc[::-1].to_csv(csvs['newest_first'], index=False)
    del frame
    synth.to_dataframe(corpus, span_docs=args.docs, date_perm=(mult, 123_457 % args.docs)).to_csv(csvs['date_perm'],
                                                                                                 index=False)
    del corpus
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    res = {'docs': args.docs, 'chunksize': args.chunksize, 'runs_per_config': args.runs,
           'date_perm': [mult, 123_457 % args.docs], 'csv_bytes': {k: os.path.getsize(v) for k, v in csvs.items()},
           'timed': 'a first match_keywords.main() into an empty directory, wall time in a fresh child per run; 1 warm-up '
                    '+ the median of the runs, the configurations in turn in one call; finish_s: the wall time inside '
                    'egress.RunFiles.finish summed over the files (per timed run in finish_s_runs); cells.stats: '
                    'sortfiles.LAST_STATS of the median run (indexed: files rewritten on the device from the write '
                    'index, index_host: by the host branch; ms: kw_sort_last_ms summed over the files); maxrss_kib: '
                    'the process\'s peak resident size'}

    def config(tree, env, csv_path):
        out = rows_config(tree, env, info_dir, csv_path, args.chunksize, args.runs, FINISH_CHILD, ('finish_s',))
        out['finish_median_s'] = statistics.median(out['finish_s_runs'])
        out['finish_range_s'] = [min(out['finish_s_runs']), max(out['finish_s_runs'])]
        print('finish-ab', os.path.basename(csv_path), os.path.relpath(tree, REPO), env, round(out['median_s'], 3),
              round(out['finish_median_s'], 3), file=sys.stderr, flush=True)
        return out

    try:
        for k in ('newest_first', 'date_perm'):
            r = res[k] = {}
            r['device'] = config(REPO, {'KW_FINISH_DEVICE': '1'}, csvs[k])
            r['host'] = config(REPO, {'KW_FINISH_DEVICE': '0'}, csvs[k])
            if parent:
                r['parent'] = config(parent, {}, csvs[k])
            r['same_bytes'] = len({v['sha256'] for v in r.values()}) == 1
            r['device_faster'] = r['device']['finish_median_s'] < r['host']['finish_median_s']
        a = res['ascending'] = {}
        a['device'] = config(REPO, {'KW_FINISH_DEVICE': '1'}, csvs['ascending'])
        if parent:
            a['parent'] = config(parent, {}, csvs['ascending'])
            a['inside_parent_spread'] = a['parent']['min_s'] <= a['device']['median_s'] <= a['parent']['max_s']
        a['same_bytes'] = len({v['sha256'] for v in a.values() if isinstance(v, dict)}) == 1
        a['device_calls'] = a['device']['cells']['stats']['indexed']
    finally:
        shutil.rmtree(work, ignore_errors=True)
    res['device_faster_on_both'] = res['newest_first']['device_faster'] and res['date_perm']['device_faster']
    res['default'] = 'device' if res['device_faster_on_both'] else 'host (the device route behind KW_FINISH_DEVICE=1)'
    with open(args.finish_ab, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res), flush=True)
    assert res['newest_first']['same_bytes'] and res['date_perm']['same_bytes'] and res['ascending']['same_bytes'], \
        'the configurations wrote different bytes'
    assert res['ascending']['device_calls'] == 0, 'the ascending corpus made a device call in the finish loop'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--finish-ab', metavar='OUT.json', help='compare the routes that finish a run\'s own files (see the module doc)')
    ap.add_argument('--sort-ab', metavar='OUT.json', help='compare the final sort\'s routes on a re-run (see the module doc)')
    ap.add_argument('--ingest-ab', metavar='OUT.json', help='compare the article ingest\'s routes (see the module doc)')
    ap.add_argument('--tz-ab', metavar='OUT.json', help='compare the time_unix routes in a zone that is not UTC (see the module doc)')
    ap.add_argument('--dates-ab', metavar='OUT.json', help='compare the date routes on ISO-8601 layouts (see the module doc)')
    ap.add_argument('--emit-ab', metavar='OUT.json', help='compare the CSV rows\' routes (see the module doc)')
    ap.add_argument('--rows-ab', metavar='OUT.json', help='compare the JSON cells\' routes (see the module doc)')
    ap.add_argument('--parent-tree', help='--rows-ab / --emit-ab: a built checkout of the parent commit')
    ap.add_argument('--runs', type=int, default=5, help='--rows-ab / --emit-ab: timed runs per configuration')
    ap.add_argument('--docs', type=int, default=200000)
    ap.add_argument('--chunksize', type=int, default=20000)
    ap.add_argument('--profile', action='store_true', help='cProfile main() (top functions by cumulative time)')
    args = ap.parse_args()
    os.environ.setdefault('TZ', 'UTC')
    time.tzset()
    if args.rows_ab:
        args.rows_ab = os.path.abspath(args.rows_ab)
        return rows_ab(args)
    if args.emit_ab:
        args.emit_ab = os.path.abspath(args.emit_ab)
        return emit_ab(args)
    if args.ingest_ab:
        args.ingest_ab = os.path.abspath(args.ingest_ab)
        return ingest_ab(args)
    if args.dates_ab:
        args.dates_ab = os.path.abspath(args.dates_ab)
        return dates_ab(args)
    if args.tz_ab:
        args.tz_ab = os.path.abspath(args.tz_ab)
        return tz_ab(args)
    if args.sort_ab:
        args.sort_ab = os.path.abspath(args.sort_ab)
        return sort_ab(args)
    if args.finish_ab:
        args.finish_ab = os.path.abspath(args.finish_ab)
        return finish_ab(args)
    import bench
    from advanced_scrapper_amd import ingest, match_keywords as mk, synth
    from advanced_scrapper_amd.kb import compile_kb
    work = tempfile.mkdtemp(prefix='e2e_')
    processed = bench.load_kb(os.path.join(work, 'ticker'))      # the reference's KB files, materialised
    names, kinds = synth.injectable_names(compile_kb(processed))
    corpus = synth.generate(args.docs, names, kinds, seed=20250905, doc_base=0)
    csv_path = os.path.join(work, 'articles.csv')
    synth.to_dataframe(corpus).to_csv(csv_path, index=False)
    csv_bytes = os.path.getsize(csv_path)
    del corpus
    os.chdir(work)
    # 1) the product's driver, end to end
    sink = io.StringIO()
    prof = None
    if args.profile:
        import cProfile
        prof = cProfile.Profile()
        prof.enable()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(sink):
        rc = mk.main(['--info-dir', os.path.join(work, 'ticker'), '--articles', csv_path,
                      '--chunksize', str(args.chunksize), '--device', '0'])
    total = time.perf_counter() - t0
    if prof is not None:
        import pstats
        prof.disable()
        pstats.Stats(prof, stream=sys.stderr).sort_stats('cumtime').print_stats(40)
    assert rc == 0
    d_main = _digest('yahoo_ticker_matched_articles')
    n_files = len(os.listdir('yahoo_ticker_matched_articles'))
    shutil.rmtree('yahoo_ticker_matched_articles')
    # 2) the split (the KB compile happens before the first chunk's phases and is not in them)
    split = phases(args, csv_path, processed)
    d_split = _digest('yahoo_ticker_matched_articles')
    out = {'docs': args.docs, 'chunksize': args.chunksize, 'csv_bytes': csv_bytes, 'files': n_files,
           'main_s': round(total, 3), 'articles_per_s': round(args.docs / total, 1),
           'phases_s': split, 'same_bytes': d_main == d_split, 'host_threads': ingest.host_threads(),
           'what': 'match_keywords.main() wall time: KB load from the reference JSON files + compile + ingest + '
                   'GPU match + render + append + final sort'}
    print(json.dumps(out), flush=True)
    os.chdir(REPO)
    shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
