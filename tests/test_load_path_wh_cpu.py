"""What of Material.load_path on a work-hardening SVC needs no GPU: the two entry points in the header, in the
built library and in the binding, every argument error and refusal of the façade around `khard0` and `form` (all raised before
the device is touched), and the CPU record: §40's iteration with the modulus carried, in NumPy around the CPU oracle's
response_wh, on the six mixed-control cases."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import flow_curve_cases as FC
import load_path_cases as LP
import load_path_wh_cases as LW
import pylabfea_amd as FE
from pylabfea_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_in_header_library_and_binding():
    txt = open(os.path.join(ROOT, 'include', 'plfx.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    m = re.search(r'int\s+plfx_load_path_wh\s*\(([^)]*)\)\s*;', code)
    assert m, 'plfx_load_path_wh is not declared'
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args == ['plfx_ctx *ctx', 'int mat', 'int n', 'int K', 'const double *dload', 'int shared', 'const int32_t *control',
                    'const double *sig0', 'const double *epl0', 'const double *khard0', 'int form', 'int maxit', 'int newton',
                    'double stol', 'double eps_cap', 'double *sig', 'double *epl', 'double *deps', 'double *fy', 'double *khard',
                    'int32_t *nsteps', 'int32_t *newton_out', 'int32_t *ksteps', 'int32_t *status', 'double *ct']
    assert re.search(r'int\s+plfx_load_path_wh_info\s*\(\s*plfx_ctx \*ctx,\s*int64_t \*launches_thread,\s*'
                     r'int64_t \*launches_wave\s*\)\s*;', code)
    lib = _lib.load()
    assert hasattr(lib, 'plfx_load_path_wh') and hasattr(lib, 'plfx_load_path_wh_info')
    assert 'plfx_load_path_wh' in _lib.SYMBOLS and 'plfx_load_path_wh_info' in _lib.SYMBOLS
    assert callable(_lib.Context.load_path_wh) and callable(_lib.Context.load_path_wh_info)
    assert lib.plfx_load_path_wh_info(None, None, None) == -2              # no context: an argument error, nothing touched
    assert lib.plfx_load_path_wh(None, 0, 1, 1, None, 0, None, None, None, None, 0, 50, 30, C.c_double(1.), C.c_double(0.05),
                                 *([None] * 10)) == -3


class FakeContext:
    """stands in for the point context: records what the façade hands to the library"""
    def __init__(self):
        self.calls = []

    def load_path(self, mat, dload, **kw):
        self.calls.append(dict(kw, mat=mat, dload=dload, entry='load_path'))
        return dict(ok=True)

    def load_path_wh(self, mat, dload, khard0, **kw):
        self.calls.append(dict(kw, mat=mat, dload=dload, khard0=khard0, entry='load_path_wh'))
        return dict(ok=True)


@pytest.fixture
def wh(monkeypatch):
    m, _ = FC.wh_material()
    ctx = FakeContext()
    monkeypatch.setattr(m, '_load', lambda CV=None, ana=False: ctx)
    return m, ctx


def test_khard0_maps_to_the_new_entry_and_counts_towards_n(wh):
    m, ctx = wh
    d3, d2 = np.zeros((4, 5, 6)), np.zeros((4, 6))
    state = dict(khard=m.khard, msg=dict(m.msg))
    assert m.load_path(d3, khard0=0.) == dict(ok=True)
    c = ctx.calls[-1]
    assert c['entry'] == 'load_path_wh' and c['form'] == 'auto' and c['mat'] == 0 and c['khard0'].shape == (5,)
    assert np.all(c['khard0'] == 0.) and c['control'] is None and c['maxit'] == 50 and c['newton'] == 30
    assert c['stol'] == 1.e-9 * m.sy and c['eps_cap'] == 0.05 and c['return_tangent'] is False and 'tex_id' not in c
    for form in ('auto', 'thread', 'wave'):
        m.load_path(d3, khard0=np.arange(5.), form=form)
        assert ctx.calls[-1]['form'] == form and ctx.calls[-1]['khard0'].tolist() == [0., 1., 2., 3., 4.]
    m.load_path(d2, khard0=3.)                                              # a shared path and a scalar: one point
    assert ctx.calls[-1]['dload'].shape == (4, 6) and ctx.calls[-1]['khard0'].tolist() == [3.]
    m.load_path(d2, khard0=np.full(7, 2.), sig0=np.ones(6))                 # N from khard0; the (6,) row is repeated
    assert ctx.calls[-1]['khard0'].shape == (7,) and ctx.calls[-1]['sig0'].shape == (7, 6)
    m.load_path(d2, khard0=1., epl0=np.zeros((3, 6)), control=[False, True, True, True, True, True])
    assert ctx.calls[-1]['khard0'].tolist() == [1., 1., 1.] and ctx.calls[-1]['control'].tolist() == [62] * 3
    assert m.khard == state['khard'] and m.msg == state['msg']             # neither khard nor msg is touched


def test_facade_errors(wh):
    m, ctx = wh
    d3, d2 = np.zeros((4, 5, 6)), np.zeros((4, 6))
    for bad, msg in ((np.zeros((5, 1)), 'khard0 must be a scalar or'), (np.zeros((1, 5)), 'khard0 must be a scalar or'),
                     (-1., 'khard0 must be finite and >= 0'), (np.array([0., 1., -1.e-300, 0., 0.]), 'khard0 must be finite and >= 0'),
                     (np.nan, 'khard0 must be finite and >= 0'), (np.inf, 'khard0 must be finite and >= 0'),
                     (np.array([0., np.nan, 0., 0., 0.]), 'khard0 must be finite and >= 0')):
        with pytest.raises(ValueError, match='load_path: ' + msg):
            m.load_path(d3, khard0=bad)
    for kw in (dict(khard0=np.zeros(4)), dict(khard0=np.zeros(6), sig0=np.ones((5, 6))), dict(khard0=np.zeros(5), epl0=np.ones((4, 6))),
               dict(khard0=np.zeros(5), control=np.zeros((2, 6), dtype=bool))):
        with pytest.raises(ValueError, match='the number of points differs.*khard0'):
            m.load_path(d3, **kw)
    with pytest.raises(ValueError, match='the number of points differs.*khard0'):
        m.load_path(d2, khard0=np.zeros(3), sig0=np.ones((4, 6)))
    for form in ('row', 'Wave', '', 0, 2, True):
        with pytest.raises(ValueError, match="load_path: form must be 'auto', 'thread' or 'wave'"):
            m.load_path(d3, khard0=0., form=form)
    for form in ('auto', 'thread', 'wave', 'row'):
        with pytest.raises(ValueError, match='load_path: form .* only together with khard0'):
            FC.hill_material(FE).load_path(d3, form=form)
    with pytest.raises(ValueError, match='load_path: khard0 is the initial hardening modulus of a work-hardening ML yield function'):
        FC.hill_material(FE).load_path(d3, khard0=0.)
    with pytest.raises(ValueError, match='load_path: khard0 is the initial hardening modulus'):
        FC.svc6_material()[0].load_path(d3, khard0=0., form='wave')
    assert ctx.calls == []                                                  # nothing reached the library


def test_refusal_without_khard0_still_stands(wh):
    m, ctx = wh
    with pytest.raises(NotImplementedError, match='load_path: not offered for work-hardening ML yield functions.*khard0'):
        m.load_path(np.zeros((4, 5, 6)))
    with pytest.raises(NotImplementedError, match='load_path: not offered for work-hardening ML yield functions'):
        m.load_path(np.zeros((4, 6)), form='wave')                          # (form alone does not lift it)
    assert ctx.calls == []


def test_binding_errors_need_no_device():
    ctx = object.__new__(_lib.Context)                                      # no device: every error below precedes the library call
    with pytest.raises(ValueError, match="form must be 'auto', 'thread' or 'wave'"):
        _lib.Context.load_path_wh(ctx, 0, np.zeros((2, 3, 6)), 0., form='both')
    with pytest.raises(ValueError, match='dload of shape'):
        _lib.Context.load_path_wh(ctx, 0, np.zeros((2, 3, 5)), 0.)
    with pytest.raises(ValueError, match='khard0 must be a scalar or'):
        _lib.Context.load_path_wh(ctx, 0, np.zeros((2, 3, 6)), np.zeros((3, 1)))
    with pytest.raises(ValueError, match='one row of control, sig0, epl0 and khard0 per point'):
        _lib.Context.load_path_wh(ctx, 0, np.zeros((2, 3, 6)), np.zeros(4))


def test_cpu_record_of_the_mixed_cases():
    """§40's iteration around oracle.response_wh(khard_in=...) with the modulus carried, on the six cases of
    load_path_cases.MIXED: K = 12, steps of 0.2 sy / E with E = CV[0,0], khard0 = 0, stol = 1e-9 sy, newton = 30.  The counts
    are printed; DESIGN.md §45 holds them."""
    from oracle import oracle as O
    z = LW.golden()
    om = O.Material.from_golden(z)
    CV = np.array(z['par_CV'], dtype=float).reshape(6, 6)
    sy = float(z['par_sy'])
    dload, control = LW.mixed_paths(sy, CV[0, 0])
    done = subdivided = hardened = 0
    for i, (name, _, _) in enumerate(LP.MIXED):
        t0 = time.perf_counter()
        R = LW.oracle_load_path(om, CV, dload[:, i], control[i], 1.e-9 * sy)
        k = R['ksteps']
        print('%-45s status %d ksteps %2d  corrections at most %2d  sub-divided steps %s  khard after the last step %.1f  (%.2f s)'
              % (name, R['status'], k, int(R['newton'][:k].max()) if k else -1, np.nonzero(R['nsteps'][:k] > 0)[0].tolist(),
                 R['khard'][k - 1] if k else float('nan'), time.perf_counter() - t0))
        assert R['status'] in (0, 1, 2, 3) and 0 <= k <= LW.K_PATH and (R['status'] == 0) == (k == LW.K_PATH)
        assert np.all(np.isfinite(R['sig'][:k])) and np.all(np.isnan(R['sig'][k:])) and np.all(R['khard'][:k] >= 0.)
        F = control[i]
        t = LP.targets(dload[:, i:i + 1], control[i:i + 1])[:, 0]
        assert np.all(np.abs(R['sig'][:k] - t[:k])[:, F] <= 1.e-9 * sy)    # accepted steps are on their stress targets
        done += R['status'] == 0
        subdivided += int(np.sum(R['nsteps'][:k] > 0))
        hardened += int(np.sum(R['khard'][:k] > 0.))
    print('complete %d of 6, accepted steps with nsteps > 0: %d, with khard > 0: %d' % (done, subdivided, hardened))
    assert done >= 4 and subdivided >= 1 and hardened >= 1


def test_carry_of_the_oracle_against_the_reference_chains():
    """The carry load_path implements -- response_wh(khard_in = the modulus the last call left) with epl += depl -- on the CPU
    oracle against tests/golden/load_path_wh.npz: chains of 12 consecutive response calls of the reference on ONE material
    object each, which carries the modulus in its attribute.  Equal nsteps, outputs within 4 max(calib, 1e-12 max|output|) of
    the reference's own two runs.  (The oracle's response has maxit = 50: the maxit = 5 chain is left to the GPU test.)"""
    from oracle import oracle as O
    z = LW.golden()
    om = O.Material.from_golden(z)
    g = np.load(os.path.join(LW.GOLD, 'load_path_wh.npz'))
    CV, K = g['CV'], g['dload'].shape[1]
    assert np.array_equal(CV, z['par_CV']) and np.all(g['first'] == K)
    worst = 0.
    for c in np.nonzero(g['maxit'] == 50)[0]:
        sig, epl, kh = g['sig0'][c].copy(), g['epl0'][c].copy(), float(g['khard0'][c])
        for k in range(K):
            fy, so, dp, ct, ns, ko = O.response_wh(om, CV.reshape(1, 36), sig[None], epl[None], g['dload'][c, k][None], khard_in=[kh])
            sig, epl, kh = so[0], epl + dp[0], float(ko[0])
            assert ns[0] == g['nsteps'][c, k], (c, k)
            for w, v in (('sig', sig), ('epl', epl), ('khard', kh), ('fy', fy[0])):
                bar = 4. * max(g['calib_' + w][c, k], 1.e-12 * np.max(np.abs(g[w])))
                r = float(np.max(np.abs(v - g[w][c, k])) / bar)
                worst = max(worst, r)
                assert r <= 1., (str(g['names'][c]), k, w, r)
    print('oracle carry against the reference chains: worst ratio to the bar %.3f' % worst)
    assert np.sum(g['nsteps'] > 0) >= 8 and np.sum(g['khard'] > 0.) >= 8
