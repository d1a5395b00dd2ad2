"""bench.py --dump-outputs: what the timed solve hands its caller after the last timed step, written as DIR/<name>.npy
(float64, arrays beyond 2^20 values as a fixed, seeded sample of their rows, below 64 MB in all)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('u', 'f', 'du', 'sig', 'eps', 'epl', 'sgl', 'egl', 'epgl')


def test_dump_rows_small_arrays_whole():
    import bench
    a = np.arange(12, dtype=np.float32).reshape(6, 2)
    b = bench.dump_rows(a, max_values=12)
    assert b.dtype == np.float64 and np.array_equal(b, a)


def test_dump_rows_sample_is_fixed_and_in_order():
    import bench
    a = np.arange(3000.).reshape(500, 6)
    b = bench.dump_rows(a, max_values=600)
    assert b.shape == (100, 6)
    rows = b[:, 0] / 6.
    assert np.array_equal(rows, np.round(rows)) and np.all(np.diff(rows) > 0)   # whole rows of `a`, each once, in index order
    assert np.array_equal(b, a[rows.astype(int)])
    assert np.array_equal(bench.dump_rows(a.copy(), max_values=600), b)         # the same rows on every call
    c = bench.dump_rows(-a, max_values=600)                                      # ... and for every array of that shape
    assert np.array_equal(c, -b)


class _Solved(object):
    """the attributes dump_outputs reads, at the size of BASELINE config 5 (2048 x 2048 elements, 20 load steps)"""

    def __init__(self, n=2048, nsteps=20):
        self.u = self.f = self.du = np.zeros(2 * (n + 1) ** 2)
        self.sgl = self.egl = self.epgl = np.zeros((nsteps, 6))
        self._el = np.broadcast_to(np.arange(6.), (n * n, 6))

    def _state(self, name):
        return self._el


def test_dump_outputs_budget_at_the_largest_mesh(tmp_path):
    import bench
    bench.dump_outputs(_Solved(), str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == sorted(k + '.npy' for k in NAMES)
    got = {k: np.load(str(tmp_path / (k + '.npy'))) for k in NAMES}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(str(tmp_path / (k + '.npy'))) for k in NAMES) < 64e6
    assert got['sig'].shape == (bench.DUMP_MAX_VALUES // 6, 6) and got['u'].shape == (bench.DUMP_MAX_VALUES // 2, 2)
    assert got['sgl'].shape == (20, 6)


@pytest.mark.gpu
def test_bench_dump_is_what_the_solve_returns(tmp_path):
    """bench.py --steps 3 --warmup 1 on 128 x 128 elements: the dumped arrays are those of the same model solved here up to the
    last timed load step, and the result line states the steps and the milliseconds per timed step"""
    K, W, n = 3, 1, 128
    out_dir = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(K), '--warmup', str(W),
                        '--mesh', str(n), '--no-cpu', '--no-svc', '--no-inclusion', '--no-2048', '--no-reuse-off',
                        '--dump-outputs', str(out_dir)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert d['steps'] == K and d['ms_per_step'] > 0. and sorted(os.listdir(str(out_dir))) == sorted(k + '.npy' for k in NAMES)
    got = {k: np.load(str(out_dir / (k + '.npy'))) for k in NAMES}
    import bench
    import pylabfea_amd as FE
    fe = bench.tension_model(FE, bench.hill_material(FE), n, 0.005)
    ninc, pre = bench.schedule(K, W)
    fe._max_load_steps = pre + W + K
    fe.solve(min_step=ninc)
    assert fe.nsteps == pre + W + K and got['sgl'].shape == (1 + pre + W + K, 6)     # the zero state, then one row per load step
    want = {'u': fe.u.reshape(-1, 2), 'f': fe.f.reshape(-1, 2), 'du': fe.du.reshape(-1, 2), 'sig': fe._state('sig'),
            'eps': fe._state('eps'), 'epl': fe._state('epl'), 'sgl': fe.sgl, 'egl': fe.egl, 'epgl': fe.epgl}
    assert np.max(want['epl']) > 0.                      # the last timed step is a plastic one
    for k in NAMES:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert np.max(np.abs(got[k] - want[k])) <= 1e-12 * max(np.max(np.abs(want[k])), 1e-300), k


@pytest.mark.gpu
def test_plain_bench_runs_the_headline_only():
    """bench.py without --full: the result line of the timed steps, and none of the legs that take a run of their own"""
    K, W, n = 2, 1, 128
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(K), '--warmup', str(W),
                        '--mesh', str(n)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d['steps'] == K and d['warmup'] == W and d['ms_per_step'] > 0. and d['value'] > 0. and d['sweeps'] > 0
    assert d['unit'] == 'element-updates/s' and d['higher_is_better'] is True and d['dtype'] == 'f64'
    assert d['config']['elements'] == n * n
    for k in ('config5_leg', 'roofline_2048', 'inclusion_variant', 'roofline_svc', 'reuse_off', 'roofline_mg_smooth', 'vs_cpu_baseline'):
        assert k not in d, k
    assert d['cpu_baseline'] is None and d['ms_per_step_reuse_off'] is None and d['ms_per_step_inclusion_variant'] is None
    assert 'plfx_precond_bench' not in d.get('vcycle', {}).get('note', '')     # no V-cycle tight loop either
