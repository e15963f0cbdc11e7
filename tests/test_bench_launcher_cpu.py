"""bench.py's launch contract on the CPU: `python bench.py --gpus N` outside torch.distributed.run starts the N ranks
itself (before any GPU call), the ranks rendezvous over gloo on 127.0.0.1, rank 0's ONE JSON line is relayed with
n_gpus = the ranks that actually joined, and a failing rank fails the launcher.  The `stub` workload does host
arithmetic only (no kernels): this tests the plumbing, not a measurement."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def _run(argv, env=None, timeout=300):
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv, capture_output=True, text=True,
                          timeout=timeout, env=e)


def test_gpus_2_starts_two_ranks_and_reports_them():
    r = _run(['--gpus', '2', '--workload', 'stub', '--steps', '4', '--warmup', '1'])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout                      # exactly one result line, from rank 0
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 4 and d['warmup'] == 1 and d['scaling'] == 'weak'
    assert d['value'] > 0 and abs(d['value'] - 25600 * 2 * 4 / (d['ms_per_step'] * 4e-3)) < 1e-3 * d['value']
    assert 'cpu_baseline' not in d                        # N = 1 only


def test_single_rank_stub_line():
    r = _run(['--workload', 'stub', '--steps', '2', '--warmup', '0'])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert d['n_gpus'] == 1


def test_world_size_must_match_gpus():
    r = _run(['--gpus', '2', '--workload', 'stub'], env={'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert r.returncode != 0 and '--gpus 2' in r.stderr


def test_failing_rank_fails_the_launcher():
    r = _run(['--gpus', '2', '--workload', 'stub', '--steps', '2'], env={'BENCH_STUB_FAIL_RANK': '1'})
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith('{')]


def test_dump_outputs_writes_the_last_step_repeatably(tmp_path):
    """--dump-outputs DIR: the timed path's results as DIR/<name>.npy in float32 / float64, identical from run to run."""
    got = []
    for run in ('a', 'b'):
        d = tmp_path / run
        r = _run(['--workload', 'stub', '--steps', '3', '--warmup', '1', '--dump-outputs', str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
        assert line['steps'] == 3 and line['ms_per_step'] > 0
        files = sorted(os.listdir(d))
        assert files == ['x.npy']
        got.append(np.load(d / 'x.npy'))
    assert got[0].dtype == np.float32 and got[0].shape == (256, 256)
    assert np.array_equal(got[0], got[1])


def test_full_is_an_option_and_plain_lines_keep_the_headline_keys():
    for extra in ([], ['--full']):
        r = _run(['--workload', 'stub', '--steps', '2', '--warmup', '0'] + extra)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in d, (extra, k)
        assert d['steps'] == 2


def test_dump_sample_is_seeded_and_within_the_limit(tmp_path):
    """Above the limit small arrays stay whole and every large one keeps the same seeded share of its elements (in a
    child: importing bench.py sets the runtime's queue count for the process)."""
    code = ('import sys, numpy as np, bench\n'
            'bench.DUMP_LIMIT_BYTES = 6400\n'
            'a = {"u": np.arange(1500, dtype=np.float32), "v": np.arange(500, dtype=np.float64).reshape(50, 10),\n'
            '     "s": np.array(3.5, dtype=np.float32)}\n'
            'for d in sys.argv[1:]:\n'
            '    bench.dump_outputs(d, a)\n')
    r = subprocess.run([sys.executable, '-c', code, str(tmp_path / 'a'), str(tmp_path / 'b')], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    u, v, s = (np.load(tmp_path / 'a' / n) for n in ('u.npy', 'v.npy', 's.npy'))
    assert s.shape == () and float(s) == 3.5                                 # small: whole
    assert u.nbytes + v.nbytes + s.nbytes <= 6400 and 0 < u.size < 1500 and 0 < v.size < 500
    assert np.array_equal(u, np.load(tmp_path / 'b' / 'u.npy')) and np.array_equal(v, np.load(tmp_path / 'b' / 'v.npy'))
    assert np.all(np.diff(u) > 0) and set(u.tolist()) <= set(range(1500))
