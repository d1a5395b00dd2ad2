#!/usr/bin/env python3
"""Time of Model.field / fields / field_range on the headline model (1024 x 1024 Hill elements after one solve), DESIGN §23.

Prints one JSON line with the median of --reps calls (wall time of the whole call: kernel, download, placement) of
  field('seq'), fields(all sixteen selectors), field_range('peeq'),
the kernel alone for each of them (the library's HIP events on its stream, timing family 0), and -- for comparison -- the
route to the same seq array without Model.field: _state('sig') plus Material.calc_seq.  With --old-route-lib PATH that
route is measured in a child process that loads the library at PATH (a build of the parent commit) instead of this tree's.
The cache of the model is emptied before every call, so every call is a device pass.

    timeout -k 10 600 python tools/field_bench.py [--mesh 1024] [--reps 11] [--old-route-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def solved_model(n, steps):
    import pylabfea_amd as FE
    mat = FE.Material(name='Hill-48')
    mat.elasticity(E=200.e3, nu=0.3)
    mat.plasticity(sy=100., hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6)
    fe = FE.Model(dim=2, planestress=False)
    fe.geom([4.], LY=4.)
    fe.assign([mat])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.002 * fe.leny, 'disp')
    fe.mesh(NX=n, NY=n)
    fe._max_load_steps = steps
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve()
    return fe, mat


def median_of(call, reps, before=None):
    call()   # warm-up: buffers, code objects
    t = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), [min(t), max(t)]


def old_route(a):
    fe, mat = solved_model(a.mesh, a.steps)

    def drop():
        fe._cache = {}
    ms, mm = median_of(lambda: mat.calc_seq(fe._state('sig')), a.reps, drop)
    ms_get, _ = median_of(lambda: fe._state('sig'), a.reps, drop)
    return dict(old_route_seq_ms=ms, old_route_seq_ms_min_max=mm, old_route_state_sig_ms=ms_get)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--mesh', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--steps', type=int, default=4, help='load steps of the solve in front of the measurement')
    ap.add_argument('--old-route-lib', default=None)
    ap.add_argument('--old-route-only', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.old_route_only:
        print(json.dumps(old_route(a)))
        return 0
    from pylabfea_amd import _lib
    from pylabfea_amd.model import FIELD_SELECTORS
    fe, mat = solved_model(a.mesh, a.steps)
    eng = fe._ensure_engine()

    def drop():
        fe._cache = {}
    res = dict(device=eng.device_info()[0], mesh=a.mesh, nel=fe.Nel, reps=a.reps, load_steps=fe.nsteps)
    calls = {'field_seq': lambda: fe.field('seq'), 'fields_all16': lambda: fe.fields(FIELD_SELECTORS),
             'field_range_peeq': lambda: fe.field_range('peeq')}
    for k, call in calls.items():
        res[k + '_ms'], res[k + '_ms_min_max'] = median_of(call, a.reps, drop)
    eng.timing_enable(True)
    eng.timing_select([_lib.T_SWEEP])
    for k, call in calls.items():
        ms = []
        for _ in range(a.reps):
            drop()
            eng.timing_reset()
            call()
            t, launches = eng.timing_get(_lib.T_SWEEP)
            assert launches == 1
            ms.append(1e3 * t)
        res[k + '_kernel_us'] = float(np.median(ms))
    eng.timing_enable(False)
    # the same numbers as the route without Model.field
    drop()
    seq_old = mat.calc_seq(fe._state('sig'))
    res['max_abs_seq_difference'] = float(np.max(np.abs(seq_old - fe.field('seq'))))
    if a.old_route_lib:
        env = dict(os.environ, PLFX_LIB=os.path.abspath(a.old_route_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--old-route-only', '--mesh', str(a.mesh), '--reps', str(a.reps),
                              '--steps', str(a.steps)], env=env, check=True, capture_output=True, text=True, timeout=540).stdout
        res.update(json.loads(out.strip().splitlines()[-1]))
        res['old_route_lib'] = 'given'
    else:
        res.update(old_route(a))
        res['old_route_lib'] = 'this tree'
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())
