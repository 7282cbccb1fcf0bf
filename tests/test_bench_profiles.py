"""bench.py's roofline `traffic` comes from the committed PMC profiles: the default files must exist, name
the bench's own default workloads and the library they profiled, and hold the dominant kernel of each line
(CPU only: JSON lookups).  Also bench.py's options: a plain run, --full and --dump-outputs."""
import json

import pytest

import bench


def _sha(path):
    return json.load(open(path))['workload']['library_sha256']


def test_default_traffic_profiles_resolve():
    kw_sha, dd_sha = _sha(bench.TRAFFIC_KW), _sha(bench.TRAFFIC_DEDUP)
    kw = bench.pmc_traffic(bench.TRAFFIC_KW, 'kw_filter_kernel', docs_per_gpu=1_000_000, seed=20250905,
                           library_sha256=kw_sha)
    dd = bench.pmc_traffic(bench.TRAFFIC_DEDUP, 'dd_transform_kernel', rows_per_gpu=500_000_000, seed=20250905,
                           library_sha256=dd_sha)
    assert kw and kw > 2_000_000_000
    assert dd and dd > 40_000_000_000
    step = bench.pmc_step_traffic(bench.TRAFFIC_KW, docs_per_gpu=1_000_000, seed=20250905, library_sha256=kw_sha)
    assert step and step > kw
    # every kernel of the library counts, template instances included ("void kw::kw_epi_flat_kernel<true>(...)")
    ks = json.load(open(bench.TRAFFIC_KW))['kernels']
    want = sum(v['hbm_bytes_per_launch'] * v.get('launches_per_step', 1) for k, v in ks.items() if 'kw::' in k)
    assert any(k.startswith('void kw::') for k in ks) and step == int(want)
    assert all(v.get('launches_per_step', 1) in (1.0, 2.0) for k, v in ks.items() if 'kw::' in k)
    c4 = bench.pmc_traffic(bench.TRAFFIC_C4, 'kw_filter_kernel', docs_per_gpu=1_000_000, seed=20250905,
                           workload='kb50k', library_sha256=_sha(bench.TRAFFIC_C4))
    assert c4 and c4 > 2_000_000_000


def test_traffic_lookup_refuses_other_workloads_and_libraries():
    sha = _sha(bench.TRAFFIC_KW)
    assert bench.pmc_traffic(bench.TRAFFIC_KW, 'kw_filter_kernel', docs_per_gpu=10_000, seed=20250905,
                             library_sha256=sha) is None
    assert bench.pmc_traffic(bench.TRAFFIC_KW, 'kw_filter_kernel', docs_per_gpu=1_000_000, seed=1,
                             library_sha256=sha) is None
    # a profile of another build prices nothing
    assert bench.pmc_traffic(bench.TRAFFIC_KW, 'kw_filter_kernel', docs_per_gpu=1_000_000, seed=20250905,
                             library_sha256='0' * 64) is None
    assert bench.pmc_step_traffic(bench.TRAFFIC_KW, docs_per_gpu=1_000_000, seed=20250905,
                                  library_sha256='0' * 64) is None
    assert bench.pmc_traffic('none', 'kw_filter_kernel') is None


def test_shard_plan_config3_and_labels():
    import argparse
    a = argparse.Namespace(docs_per_gpu=None, total_docs=None)
    assert bench.shard_plan(a, 0, 1) == (0, 1_000_000, 1_000_000, 'strong')
    plans = [bench.shard_plan(a, r, 8) for r in range(8)]
    assert [p[0] for p in plans] == [r * 1_250_000 for r in range(8)]
    assert sum(p[1] for p in plans) == 10_000_000 and {p[2] for p in plans} == {10_000_000}
    plans = [bench.shard_plan(a, r, 3) for r in range(3)]     # ragged: the last shard takes the remainder
    assert sum(p[1] for p in plans) == 10_000_000 and plans[2][0] + plans[2][1] == 10_000_000
    assert bench.workload_label(10_000_000, 8) == 'config 3' and bench.workload_label(10_000_000, 1) == 'config 3'
    assert bench.workload_label(1_000_000, 1) == 'config 2' and bench.workload_label(8_000_000, 8) != 'config 3'
    w = argparse.Namespace(docs_per_gpu=1000, total_docs=None)
    assert bench.shard_plan(w, 3, 4) == (3000, 1000, 4000, 'weak')


def test_bench_kb_is_the_products_loader_on_the_reference_files(tmp_path, golden):
    assert bench.load_kb(str(tmp_path / 'ticker')) == golden.kb_processed()


def _parse(monkeypatch, argv):
    import sys
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    return bench._parse()


def test_plain_run_options(monkeypatch):
    """A plain run does neither the CPU baseline nor the dump; --full and --dump-outputs ask for them."""
    import pytest
    a = _parse(monkeypatch, ['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, ['--full', '--dump-outputs', 'somewhere'])
    assert a.full and a.dump_outputs == 'somewhere'
    with pytest.raises(SystemExit):
        _parse(monkeypatch, ['--steps', '0'])


def test_dump_match_outputs_sorted_sample_is_order_independent(tmp_path):
    """The dumped records do not depend on the order the library left them in: per-document counts of every
    document, every record of the seeded document sample in (doc, field, pos, pattern) order, float arrays."""
    import numpy as np
    import torch
    rng = np.random.default_rng(3)
    n, total = 30_000, bench.DUMP_SAMPLE_DOCS + 1000          # more documents than the sample holds
    rec = np.stack([rng.integers(0, total, n), rng.integers(0, 2000, n), rng.integers(0, 3000, n),
                    rng.integers(0, 2, n)], 1).astype(np.uint32)
    rec[0] = (total - 1, 0xFFFFFFFF, 0x80000000, 1)           # the int32 view's sign bit is value, not sign
    t = torch.from_numpy(rec.view(np.int32))
    bench.dump_match_outputs(str(tmp_path / 'a'), t, n, total, 11)
    bench.dump_match_outputs(str(tmp_path / 'b'), t[torch.randperm(n)], n, total, 11)
    got = {}
    for name, dtype in (('hits_total', np.float64), ('hits_per_doc', np.float32), ('hits_sample', np.float64)):
        got[name] = np.load(tmp_path / 'a' / f'{name}.npy')
        assert got[name].dtype == dtype
        assert np.array_equal(got[name], np.load(tmp_path / 'b' / f'{name}.npy')), name
    assert got['hits_total'].tolist() == [n]
    assert np.array_equal(got['hits_per_doc'], np.bincount(rec[:, 0], minlength=total))
    s = got['hits_sample']
    docs = np.unique(s[:, 0]).astype(np.int64)
    assert 0 < len(docs) <= bench.DUMP_SAMPLE_DOCS and len(s) < n
    # every record of a sampled document is there, and the rows are in the stated order
    want = rec[np.isin(rec[:, 0], docs)].astype(np.float64)
    want = want[np.lexsort((want[:, 1], want[:, 2], want[:, 3], want[:, 0]))]
    assert np.array_equal(s, want)
    # counts only (the exchange carried no records): the total alone
    bench.dump_match_outputs(str(tmp_path / 'c'), None, n, total, 11)
    assert sorted(p.name for p in (tmp_path / 'c').iterdir()) == ['hits_total.npy']


def test_dump_dedup_outputs_samples_rows_from_the_seed(tmp_path, monkeypatch):
    import numpy as np
    import torch
    monkeypatch.setattr(bench, 'DUMP_SAMPLE_ROWS', 1000)
    code = torch.from_numpy(np.random.default_rng(5).integers(0, 4, 5000).astype(np.uint8))
    bench.dump_dedup_outputs(str(tmp_path), code, [1, 2, 3, 4], 11)
    c = np.load(tmp_path / 'codes.npy')
    rows = np.sort(np.random.default_rng(11).integers(0, 5000, 1000))
    assert c.dtype == np.float32 and np.array_equal(c, code.numpy()[rows])
    assert np.load(tmp_path / 'counts.npy').tolist() == [1.0, 2.0, 3.0, 4.0]
    bench.dump_dedup_outputs(str(tmp_path), code[:1000], [1, 2, 3, 4], 11)
    assert np.array_equal(np.load(tmp_path / 'codes.npy'), code[:1000].numpy())


@pytest.mark.gpu
def test_plain_bench_run_dumps_its_last_step(tmp_path, monkeypatch, capsys):
    """bench.main() itself (in this process, on the in-tree library), on a small corpus: --steps sets the
    timed steps, the line holds ms_per_step and no CPU baseline, and the dump holds every record of the step
    the line counts."""
    import os
    import numpy as np
    from advanced_scrapper_amd import _native
    out = tmp_path / 'dump'
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'KW_LIB'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr('sys.argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1',
                                     '--total-docs', '20000', '--dump-outputs', str(out)])
    bench.main()
    assert os.path.dirname(_native.LIB_PATH) == os.path.join(bench.REPO, 'advanced_scrapper_amd', 'lib')
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j['steps'] == 3 and j['warmup'] == 1 and j['ms_per_step'] > 0 and j['cpu_baseline'] is None
    assert j['unit'] == 'GB/s' and j['dtype'] == 'u8' and j['higher_is_better'] is True
    assert abs(j['value'] - j['config']['total_bytes'] / (j['ms_per_step'] * 1e-3) / 1e9) <= 0.01 * j['value']
    total = j['config']['hits_total']
    s = np.load(out / 'hits_sample.npy')
    per_doc = np.load(out / 'hits_per_doc.npy')
    assert np.load(out / 'hits_total.npy').tolist() == [total] and total > 0
    assert per_doc.shape == (20000,) and per_doc.sum() == total
    assert s.shape == (total, 4) and s.dtype == np.float64      # 20 000 documents: all of them are in the sample
    assert np.array_equal(np.bincount(s[:, 0].astype(np.int64), minlength=20000), per_doc)
    key = np.lexsort((s[:, 1], s[:, 2], s[:, 3], s[:, 0]))
    assert np.array_equal(key, np.arange(total))
