#!/usr/bin/env python3
"""GPU time of Material.yield_scale (k_yield_scale: the whole root search of a ray in one launch) beside the host loop of
Material._yield_scale (up to 60 + 64 batched calc_yf calls with a round trip each) on the same N rays of the config-4
material (the trained SVC of tests/golden/svc_hill.npz, 1585 support vectors, 6 features), N = 72, 300 and 10 000 random
directions.  Kernel time from the library's HIP events on its stream (timing family 0, plfx_timing_get): one warm-up call,
then the median of --reps calls; wall time of the whole call beside it.  Every N runs in a child process of its own under
its own time limit, and nothing more is started after one that fails.  One JSON line per N.

    python tools/yield_locus_bench.py [--reps 11] [--limit 120]
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
SIZES = (72, 300, 10000)


def step(n, reps):
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_hill.npz'))
    m = FE.Material(name='ML')
    m.elasticity(CV=z['par_CV'])
    m.plasticity(sy=float(z['par_sy']), sdim=6)
    m.set_svc(z['par_sv'], z['par_dual'], float(z['par_intercept']), float(z['par_gamma']), float(z['par_scale_seq']),
              dev_only=bool(z['par_dev_only']))
    rng = np.random.default_rng(n)
    u = rng.normal(size=(n, 6))
    su = u / np.linalg.norm(u, axis=1)[:, None] * m.sy
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

    x, k_ms, k_wall, k_l = timed(lambda: m.yield_scale(su))
    xh, h_ms, h_wall, h_l = timed(lambda: m._yield_scale(su))
    ctx.timing_enable(False)
    assert k_l == 1
    print(json.dumps(dict(device=name, cus=cus, n=n, nsv=int(len(z['par_sv'])), reps=reps,
                          yield_scale_kernel_ms=k_ms, yield_scale_wall_ms=k_wall, yield_scale_launches=k_l,
                          host_loop_kernel_ms=h_ms, host_loop_wall_ms=h_wall, host_loop_launches=h_l,
                          kernel_ratio=h_ms / k_ms, wall_ratio=h_wall / k_wall,
                          max_rel_difference=float(np.max(np.abs(x - xh) / x)))))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--limit', type=int, default=120, help='time limit of one step in seconds')
    ap.add_argument('--step', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps)
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 launches)')
    for n in SIZES:   # a fresh child per step, each under its own limit; stop at the first that fails
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__),
                              '--step', str(n), '--reps', str(a.reps)])
        if rc != 0:
            print('step n = %d ended with status %d; nothing more is started' % (n, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
