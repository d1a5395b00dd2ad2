#!/usr/bin/env python3
"""GPU time of Material.flow_curve (k_flow_curve: N whole chains in one launch) beside the per-step Python
loop over yield_scale(x0=previous root) and calc_fgrad that gives the same curves with two launches and two host round trips
per step, on the work-hardening material of tests/golden/flow_curve.npz (1018 support vectors, 15 features): N = 1, 4, 300
and 100 000 curves x 20 steps, predictor 1000.  Kernel time from the library's HIP events on its stream (timing family 0):
one warm-up call, then the median of --reps calls; wall time of the whole call beside it.  The loop needs nothing of this
library that its predecessor lacks, so with --old-lib it is timed on that library too, in a child of its own (PLFX_LIB).
Every step runs in a child process under its own time limit, and nothing more is started after one that fails.  One JSON
line per step.

    python tools/flow_curve_bench.py [--reps 11] [--limit 300] [--old-lib path/to/libplfx.so]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SIZES = (1, 4, 300, 100000)
STEPS, DEPL, PRED = 20, 1.e-3, 1000.


def loop(m, ctx, su):
    """the curves as the façade could trace them before flow_curve: x (N, STEPS + 1)"""
    from pylabfea_amd.basic import eps_eq
    n = len(su)
    e = np.zeros((n, 6))
    x, _ = ctx.yield_scale(0, su, e, np.full(n, float(m.sy)))
    xs = [x]
    for _ in range(STEPS):
        peeq = eps_eq(e) + DEPL
        a, _ = ctx.fgrad_wh(0, su * (x + peeq * PRED)[:, None], e)
        e = e + a * DEPL / eps_eq(a)[:, None]
        x, _ = ctx.yield_scale(0, su, e, x)
        xs.append(x)
    return np.stack(xs, axis=1)


def step(n, reps, which):
    import flow_curve_cases as FC
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    m, p = FC.wh_material()
    su = np.tile(FC.directions(FE.load_cases), (n // 12 + 1, 1))[:n]
    if n > 12:   # distinct directions: the twelve of the fixture, each tilted a little
        su = su + 0.05 * np.random.default_rng(n).normal(size=su.shape)
        su = np.ascontiguousarray(su / FE.sig_eq_j2(su)[:, None])
    ctx = m._load()
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
        return out, float(np.median(ms)), float(np.median(wall)), int(launches)

    res = dict(device=name, cus=cus, n=n, steps=STEPS, nsv=int(len(p['sv'])), reps=reps, lib=os.path.basename(_lib.LIB_PATH),
               which=which)
    xl, l_ms, l_wall, l_l = timed(lambda: loop(m, ctx, su))
    res.update(loop_kernel_ms=l_ms, loop_wall_ms=l_wall, loop_launches=l_l)
    if which == 'new':
        r, k_ms, k_wall, k_l = timed(lambda: ctx.flow_curve(0, su, None, max_steps=STEPS, depl=DEPL, epl_max=np.inf,
                                                            predictor=PRED))
        assert k_l == 1
        res.update(flow_curve_kernel_ms=k_ms, flow_curve_wall_ms=k_wall, flow_curve_launches=k_l,
                   kernel_ratio=l_ms / k_ms, wall_ratio=l_wall / k_wall, same_x_bits=bool(np.array_equal(r['x'], xl)),
                   max_rel_difference=float(np.max(np.abs(r['x'] - xl) / xl)))
    ctx.timing_enable(False)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--limit', type=int, default=300, help='time limit of one step in seconds')
    ap.add_argument('--old-lib', default=None, help='the predecessor library: the loop is timed on it too')
    ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
    ap.add_argument('--step', type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument('--which', default='new', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.which)
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 launches)')
    for n in a.sizes:   # a fresh child per step, each under its own limit; stop at the first that fails
        for which in ('new', 'old') if a.old_lib else ('new',):
            env = dict(os.environ, PLFX_LIB=os.path.abspath(a.old_lib)) if which == 'old' else dict(os.environ)
            rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__),
                                  '--step', str(n), '--reps', str(a.reps), '--which', which], env=env)
            if rc != 0:
                print('step n = %d (%s) ended with status %d; nothing more is started' % (n, which, rc), file=sys.stderr)
                return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
