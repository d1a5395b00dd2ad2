#!/usr/bin/env python3
"""GPU time of Committee.calc_yf / variance / query (k_committee_yf: M yield functions on N shared unit stresses, mean,
variance and the largest variance in one launch) beside the only other way to the same numbers: M Material.calc_yf calls on
the N points, and for N = 450 also 450 x M single-point calls as the reference's query-by-committee example issues them
(one differential-evolution generation of popsize 90 x 5 angles).  Committee: the five members of
tests/golden/committee.npz (200 to 334 support vectors); N = 1, 450 and 100 000 random unit stresses.  Kernel time from the
library's HIP events on its stream (timing family 0, plfx_timing_get): one warm-up call, then the median of --reps calls;
wall time of the whole call beside it.  Every N runs in a child process of its own under its own time limit, and nothing
more is started after one that fails.  One JSON line per N.

    python tools/committee_bench.py [--reps 11] [--limit 240]
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
SIZES = (1, 450, 100000)


def step(n, reps):
    import committee_cases as CC
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    z = CC.load()
    mats = [CC.facade(CC.member_params(z, k), 'm%d' % k) for k in range(5)]
    com = FE.Committee(mats)
    rng = np.random.default_rng(n)
    u = rng.normal(size=(n, 6))
    su = u / np.linalg.norm(u, axis=1)[:, None]
    ctx = com._load()
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

    def members_batched():
        y = np.array([m.calc_yf(su * 0.5 * m.sy) for m in mats])
        return y, np.var(y, axis=0)

    def members_pointwise():
        v = np.empty(n)
        for i in range(n):
            v[i] = np.var([m.calc_yf(su[i] * 0.5 * m.sy) for m in mats])
        return v

    res = dict(device=name, cus=cus, n=n, members=5, nsv=[int(len(m.svc['dual'])) for m in mats], reps=reps)
    y, k_ms, k_wall, k_l = timed(lambda: com.calc_yf(su))
    assert k_l == 1
    res.update(calc_yf_kernel_ms=k_ms, calc_yf_wall_ms=k_wall)
    (i, _, v), q_ms, q_wall, q_l = timed(lambda: com.query(su))
    assert q_l == 1
    res.update(query_kernel_ms=q_ms, query_wall_ms=q_wall)
    (yb, vb), b_ms, b_wall, b_l = timed(members_batched)
    res.update(members_kernel_ms=b_ms, members_wall_ms=b_wall, members_launches=b_l,
               calc_yf_wall_ratio=b_wall / k_wall, query_wall_ratio=b_wall / q_wall,
               max_abs_difference=float(np.max(np.abs(y - yb))), same_query=bool(i == int(np.argmax(vb))))
    if n == 450:
        vp, p_ms, p_wall, p_l = timed(members_pointwise)
        res.update(pointwise_kernel_ms=p_ms, pointwise_wall_ms=p_wall, pointwise_launches=p_l,
                   pointwise_query_wall_ratio=p_wall / q_wall)
    ctx.timing_enable(False)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--limit', type=int, default=240, help='time limit of one step in seconds')
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
