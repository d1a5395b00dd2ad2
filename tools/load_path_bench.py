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

--wh: the work-hardening SVC of tests/golden/svc_workhard.npz (1018 vectors, 15 features), whose hardening
modulus is state of a path.  wh:N -- K = 20 seeded strain paths, khard0 = 0, in the wave form (k_path_wh_wave), the thread form
(k_path_batch<7>) and the host loop over response(khard_in=, return_khard=True) with the modulus carried, all on the same
build; same_bits compares the thread form with the loop.  whumat:9 -- the nine UMAT load cases under mixed control in the wave
form, with the strain-controlled replay of the increments it took in place of a loop.  --forms leaves forms of wh:N out.

    python tools/load_path_bench.py [--reps 11] [--limit 300] [--runs hill:1 hill:1000 hill:100000 svc:1 svc:10000 umat:54]
    python tools/load_path_bench.py --wh [--runs wh:1 wh:9 wh:54 wh:1000 wh:10000 wh:100000 whumat:9] [--forms wave thread loop]
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
WH_RUNS = ('wh:1', 'wh:9', 'wh:54', 'wh:1000', 'wh:10000', 'wh:100000', 'whumat:9')
FORMS = ('wave', 'thread', 'loop')
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


def timer(ctx, reps):
    """timed(call) -> (result, kernel ms per call, wall ms per call, launches of the last call) after one warm-up call, and
    stats(prefix, ...) -> the entries of the JSON line"""
    from pylabfea_amd import _lib

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
    return timed, stats


def run_wh(what, n, reps, forms):
    import load_path_cases as LP
    import load_path_wh_cases as LW
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    z = LW.golden()
    m, _ = LW.table(FE, z, 'full')
    CV = np.array(z['par_CV'], dtype=float).reshape(6, 6)
    sy, E = float(z['par_sy']), float(CV[0, 0])
    ctx = m._load(CV)
    name, cus, _ = ctx.device_info()
    ctx.timing_enable(True)
    ctx.timing_select([_lib.T_SWEEP])
    timed, stats = timer(ctx, reps)
    res = dict(device=name, cus=cus, run=what, n=n, steps=STEPS, reps=reps, mixed=what == 'whumat')
    if what == 'whumat':
        cases = np.array(UMAT_CASES, dtype=float)
        n = len(cases)
        d = np.zeros((n, 6))
        d[:, :3] = 0.2 * sy / E * cases
        dload = np.ascontiguousarray(np.tile(d, (STEPS, 1, 1)))
        control = np.concatenate((cases == 0., np.ones((n, 3), dtype=bool)), axis=1)
        P, ms, wall, nl = timed(lambda: m.load_path(dload, control=control, CV=CV, khard0=0., form='wave'))
        assert nl == 1
        res.update(n=n, **stats('wave', ms, wall, nl))
        took = P['newton'][P['newton'] >= 0]
        res.update(complete=int(np.sum(P['status'] == 0)), status_counts=np.bincount(P['status'], minlength=4).tolist(),
                   ksteps=P['ksteps'].tolist(), corrections_max=int(P['newton'].max()),
                   trials_per_step_mean=float(1. + np.mean(took)), khard_last=[float(P['khard'][k - 1, i]) if k else None
                                                                               for i, k in enumerate(P['ksteps'])])
        deps = np.where(np.isnan(P['deps']), 0., P['deps'])   # (a path that ended early idles in the replay)
        R, rms, rwall, rl = timed(lambda: m.load_path(deps, CV=CV, khard0=0., form='wave'))
        res.update(stats('replay_wave', rms, rwall, rl))
        done = P['status'] == 0
        res.update(replay_same_bits=bool(np.array_equal(R['sig'][:, done], P['sig'][:, done])
                                         and np.array_equal(R['khard'][:, done], P['khard'][:, done])))
    else:
        dload = LP.strain_paths(sy, E, K=STEPS, N=n, seed=n)
        out = {}
        for form in ('wave', 'thread'):
            if form in forms:
                out[form], ms, wall, nl = timed(lambda: m.load_path(dload, CV=CV, khard0=0., form=form))
                assert nl == 1
                res.update(stats(form, ms, wall, nl))
                res[form + '_nsteps_pos'] = int(np.sum(out[form]['nsteps'] > 0))
        if 'loop' in forms:
            Y, lms, lwall, ll = timed(lambda: LW.yardstick(m, CV, dload, 50, 0.))
            res.update(stats('loop', lms, lwall, ll))
            if 'thread' in out:
                res.update(same_bits=bool(all(np.array_equal(Y[w], out['thread'][w]) for w in LW.NAMES)))
        for a, b in (('thread', 'wave'), ('loop', 'wave'), ('loop', 'thread')):
            if a + '_kernel_ms' in res and b + '_kernel_ms' in res:
                res['%s_over_%s_kernel' % (a, b)] = res[a + '_kernel_ms'] / res[b + '_kernel_ms']
                res['%s_over_%s_wall' % (a, b)] = res[a + '_wall_ms'] / res[b + '_wall_ms']
        if 'wave' in out and 'thread' in out:
            res.update(nsteps_equal=bool(np.array_equal(out['wave']['nsteps'], out['thread']['nsteps'])),
                       sig_diff_max=float(np.max(np.abs(out['wave']['sig'] - out['thread']['sig']))))
    ctx.timing_enable(False)
    print(json.dumps(res))
    return 0


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
    ap.add_argument('--wh', action='store_true', help='the runs of the work-hardening SVC: ' + ' '.join(WH_RUNS))
    ap.add_argument('--forms', nargs='*', default=list(FORMS), choices=FORMS, help='forms of a wh:N run')
    ap.add_argument('--quick', action='store_true', help='with --wh: fewer than 10 calls per figure, for the thread form and the loop, whose calls take seconds (the JSON line says reps)')
    ap.add_argument('--run', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run:
        what, n = a.run.split(':')
        return run_wh(what, int(n), a.reps, a.forms) if what.startswith('wh') else run(what, int(n), a.reps)
    if a.wh and a.runs == list(RUNS):
        a.runs = list(WH_RUNS)
    if a.quick and not all(r.startswith('wh') for r in a.runs):
        ap.error('--quick is for the runs of --wh alone')
    if a.reps < 10 and not a.quick:
        ap.error('--reps must be at least 10 (median of >= 10 calls)')
    for r in a.runs:   # a fresh child per run, each under its own limit; stop at the first that fails
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--run', r,
                              '--reps', str(a.reps), '--forms'] + list(a.forms))
        if rc != 0:
            print('run %s ended with status %d; nothing more is started' % (r, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
