#!/usr/bin/env python3
"""GPU time of Material.load_path (k_path_batch / k_path_row: N whole load paths in one launch) beside the host
loop that gives the same states: K response_batch calls with epl += depl in NumPy between them, each with its copies in and
out.  Runs: the Hill material of tests/flow_curve_cases.py at N = 1, 1000 and 100 000 and the 1585-vector SVC of
tests/golden/svc_hill.npz at N = 1 and 10 000, K = 20 seeded strain paths (tests/load_path_cases.py); and the nine load cases
of the reference's examples/UMAT/calc_properties.py -- driven normal strains, every other component stress-free -- on a
texture field of T = 6 textures, 54 paths in one launch under mixed control.  For that run the loop is the strain-controlled
replay of the increments load_path took: K calls, without the Newton iterations a host loop would have to add, so a lower
bound of it.  Kernel time from the library's HIP events on its stream (timing family 0), wall time of the whole call beside
it: one warm-up call, then the median of --reps calls with the smallest and largest.  Every run is a child process under its
own time limit, and nothing more is started after one that fails.  One JSON line per run.

    python tools/load_path_bench.py [--reps 11] [--limit 300] [--runs hill:1 hill:1000 hill:100000 svc:1 svc:10000 umat:54]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
RUNS = ('hill:1', 'hill:1000', 'hill:100000', 'svc:1', 'svc:10000', 'umat:54')
STEPS = 20
UMAT_CASES = ([1, 0, 0], [0, 1, 0], [1, 1, 0], [-1, 1, 0], [0, 0, 1], [0, 1, 1], [1, 0, 1], [0, -1, 1], [1, 0, -1])


def loop(ctx, dload, tid):
    """the states as the façade could follow them before load_path: sig, epl (K, N, 6)"""
    K, n = dload.shape[:2]
    sig, epl = np.zeros((n, 6)), np.zeros((n, 6))
    S, E = np.empty((K, n, 6)), np.empty((K, n, 6))
    for k in range(K):
        fy, sig, dp, ct, ns = ctx.response(sig, epl, np.ascontiguousarray(dload[k]), tex_id=tid)
        epl = epl + dp
        S[k], E[k] = sig, epl
    return S, E


def run(what, n, reps):
    import flow_curve_cases as FC
    import load_path_cases as LP
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    tid, control = None, None
    if what == 'hill':
        m = FC.hill_material(FE)
        CV = np.array(m.CV)
        dload = LP.strain_paths(float(m.sy), float(m.E), K=STEPS, N=n, seed=n)
    elif what == 'svc':
        m, _ = FC.svc6_material()
        CV = np.array(m.CV)
        dload = LP.strain_paths(float(m.sy), float(m.E), K=STEPS, N=n, seed=n)
    else:
        import texture_cases as TC
        import texture_field_cases as TX
        z = TC.load()
        base = TC.facade(FE, z, tempfile.mkdtemp(), 'GSH_3')[0]
        tex = TX.field_textures(TC.textures(z, 'GSH_3'), 6)
        _, m, CV, _, _, _ = TX.field_case(FE, base, TC.tables(z, 'GSH_3'), tex, 91)
        cases = np.array(UMAT_CASES, dtype=float)
        n = len(cases) * len(tex)
        d = np.zeros((len(cases), 6))
        d[:, :3] = 0.2 * float(m.sy) / float(m.E) * cases
        dload = np.ascontiguousarray(np.tile(d, (STEPS, len(tex), 1)))
        control = np.tile(np.concatenate((cases == 0., np.ones((len(cases), 3), dtype=bool)), axis=1), (len(tex), 1))
        tid = np.repeat(np.arange(len(tex)), len(cases)).astype(np.int32)
    ctx = m._load(CV)
    name, cus, _ = ctx.device_info()
    ctx.timing_enable(True)
    ctx.timing_select([_lib.T_SWEEP])

    def timed(call):
        out = call()                                 # warm-up: code object load, allocations
        ms, wall, launches = [], [], 0
        for _ in range(reps):
            ctx.timing_reset()
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
            t, launches = ctx.timing_get(_lib.T_SWEEP)
            ms.append(t)
        return out, ms, wall, int(launches)

    def stats(prefix, ms, wall, launches):
        return {prefix + '_kernel_ms': float(np.median(ms)), prefix + '_kernel_ms_range': [float(min(ms)), float(max(ms))],
                prefix + '_wall_ms': float(np.median(wall)), prefix + '_wall_ms_range': [float(min(wall)), float(max(wall))],
                prefix + '_launches': launches}
    res = dict(device=name, cus=cus, run=what, n=n, steps=STEPS, reps=reps, mixed=control is not None)
    P, ms, wall, nl = timed(lambda: m.load_path(dload, control=control, CV=CV, tex_id=tid))
    assert nl == 1
    res.update(stats('load_path', ms, wall, nl))
    res.update(complete=int(np.sum(P['status'] == 0)), status_counts=np.bincount(P['status'], minlength=4).tolist(),
               corrections_max=int(P['newton'].max()), trials_per_step_mean=float(1. + np.mean(P['newton'][P['newton'] >= 0])))
    done = P['status'] == 0
    deps = np.where(np.isnan(P['deps']), 0., P['deps'])   # (a path that ended early idles in the replay)
    (S, E), lms, lwall, ll = timed(lambda: loop(ctx, deps, tid))
    res.update(stats('loop', lms, lwall, ll))
    res.update(kernel_ratio=float(np.median(lms) / np.median(ms)), wall_ratio=float(np.median(lwall) / np.median(wall)),
               same_bits=bool(np.array_equal(S[:, done], P['sig'][:, done]) and np.array_equal(E[:, done], P['epl'][:, done])))
    ctx.timing_enable(False)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--limit', type=int, default=300, help='time limit of one run in seconds')
    ap.add_argument('--runs', nargs='*', default=list(RUNS), help='material:N, of hill, svc, umat')
    ap.add_argument('--run', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run:
        what, n = a.run.split(':')
        return run(what, int(n), a.reps)
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 calls)')
    for r in a.runs:   # a fresh child per run, each under its own limit; stop at the first that fails
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--run', r,
                              '--reps', str(a.reps)])
        if rc != 0:
            print('run %s ended with status %d; nothing more is started' % (r, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
