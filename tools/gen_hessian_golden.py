#!/usr/bin/env python3
"""Golden-vector generator for Material.calc_hessian (TEST INFRASTRUCTURE, development machine only): calls the unmodified
reference's calc_hessian (material.py:860-972) for the trained SVC yield functions of tests/golden/svc_hill.npz (6 features)
and tests/golden/svc_workhard.npz (15 features), plus the first with dev_only switched on, and writes
tests/golden/svc_hessian.npz.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_hessian_golden.py

The SVC parameters enter the reference Material through a stand-in for the scikit-learn estimator that carries
support_vectors_ / dual_coef_ (calc_hessian reads nothing else of it); everything evaluated is the reference's code.

Per material ~200 stresses: a third on the yield locus (calc_seq = sy), a third scaled by 0.3 ... 2, the rest so far out that
every kernel value underflows to zero in FP64, and one stress in the single-point (6,) form; non-zero plastic strains for the
work-hardening material.

Tolerance gauge (stored as <tag>_r_ref).  Per entry the Hessian is a sum of nsv signed terms; with
    A[a][b] = sum_i |c_i| k_i |4 gamma^2 d_i[a] d_i[b] - 2 gamma delta_ab| / scale_seq
r_ref is the reference's own worst deviation from an np.longdouble evaluation of the same formula, in units of A 2^-53, over
all rows and entries.  The GPU tests allow 4 max(r_ref, 1) of those units per entry."""
import os
import sys

import numpy as np

import pylabfea as FE  # the reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


class SvmStub(object):
    def __init__(self, sv, dual):
        self.support_vectors_ = sv
        self.dual_coef_ = dual[None, :]


def ref_material(z, dev_only=False):
    m = FE.Material(name='hessian-fixture')
    m.elasticity(E=float(z['par_E']), nu=float(z['par_nu']))
    m.plasticity(sy=float(z['par_sy']), hill=list(z['par_hill']), sdim=6)
    m.svm_yf = SvmStub(np.array(z['par_sv']), np.array(z['par_dual']))
    m.gam_yf = float(z['par_gamma'])
    m.scale_seq = float(z['par_scale_seq'])
    m.dev_only = bool(dev_only)
    m.ML_yf, m.ML_grad = True, False
    m.Ndof = int(z['par_Ndof'])
    if m.Ndof == 15:
        m.whdat = True
        m.ind_wh = int(z['par_ind_wh'])
        m.scale_wh = float(z['par_scale_wh'])
    return m


def longdouble_hessian(m, sig, epl):
    """(H, A) of the formula in np.longdouble from the reference's own (double) feature vectors; both / scale_seq"""
    x = m.create_scaled_input(sig, epl, 0.0, 0.0, 0.0, None).astype(np.longdouble)
    sv = m.svm_yf.support_vectors_.astype(np.longdouble)
    dc = m.svm_yf.dual_coef_[0].astype(np.longdouble)
    g = np.longdouble(m.gam_yf)
    H = np.zeros((len(x), 6, 6), dtype=np.longdouble)
    A = np.zeros((len(x), 6, 6), dtype=np.longdouble)
    for n in range(len(x)):
        d = sv - x[n]
        w = dc * np.exp(-g * np.sum(d * d, axis=1))
        t = 4 * g * g * d[:, :6, None] * d[:, None, :6] - 2 * g * np.eye(6, dtype=np.longdouble)
        H[n] = np.sum(w[:, None, None] * t, axis=0)
        A[n] = np.sum(np.abs(w)[:, None, None] * np.abs(t), axis=0)
    s = np.longdouble(m.scale_seq)
    return H / s, A / s


def points(m, rng, n_loc, n_scaled, n_far, with_epl):
    n = n_loc + n_scaled + n_far
    u = rng.normal(size=(n, 6))
    u /= np.linalg.norm(u, axis=1)[:, None]
    loc = u * (m.sy / m.calc_seq(u))[:, None]          # on the yield locus of the analytic form: calc_seq = sy
    f = np.ones(n)
    f[n_loc:n_loc + n_scaled] = rng.uniform(0.3, 2.0, size=n_scaled)
    # far away: |x - v| >= |x| - max|v| for every support vector; ask for gamma |d|^2 >= 800, assert > 745 below
    sv = m.svm_yf.support_vectors_
    xn = np.linalg.norm(m.create_scaled_input(loc[n - n_far:], np.zeros((n_far, 6)), 0.0, 0.0, 0.0, None)[:, :6], axis=1)
    far = (np.sqrt(800. / m.gam_yf) + np.max(np.linalg.norm(sv, axis=1))) / np.min(xn) * 1.05
    f[n - n_far:] = far * rng.uniform(1.0, 3.0, size=n_far)
    sig = loc * f[:, None]
    epl = np.zeros((n, 6))
    if with_epl:
        e = rng.normal(size=(n, 6))
        e[:, :3] -= np.mean(e[:, :3], axis=1)[:, None]
        e *= (rng.uniform(0., 1.5, size=n) * m.scale_wh / np.linalg.norm(e, axis=1))[:, None]
        e[::7] = 0.                                     # some rows at zero plastic strain
        epl = e
    x = m.create_scaled_input(sig[n - n_far:], epl[n - n_far:], 0.0, 0.0, 0.0, None)
    d2 = np.sum((sv[None, :, :] - x[:, None, :]) ** 2, axis=2)
    assert np.min(m.gam_yf * d2) > 745., 'far points: a kernel value does not underflow'
    assert np.all(np.exp(-m.gam_yf * d2) == 0.)
    return sig, epl, far


def main():
    rec = {}
    cases = (('hill', 'svc_hill.npz', False, 67, 67, 66), ('hilldev', 'svc_hill.npz', True, 24, 24, 12),
             ('wh', 'svc_workhard.npz', False, 67, 67, 66))
    for seed, (tag, src, dev_only, n_loc, n_scaled, n_far) in enumerate(cases):
        z = np.load(os.path.join(GOLD, src))
        m = ref_material(z, dev_only)
        rng = np.random.default_rng(860 + seed)
        sig, epl, far = points(m, rng, n_loc, n_scaled, n_far, m.whdat)
        khard, msg = m.khard, dict(m.msg)
        hess = m.calc_hessian(sig, epl=epl) if m.whdat else m.calc_hessian(sig)
        assert hess.shape == (len(sig), 6, 6)
        k1 = n_loc // 2                                  # the single-point (6,) form
        one = m.calc_hessian(sig[k1], epl=epl[k1]) if m.whdat else m.calc_hessian(sig[k1])
        assert one.shape == (1, 6, 6)
        assert m.khard == khard and m.msg == msg, 'the reference calc_hessian has side effects after all'
        Hl, Al = longdouble_hessian(m, sig, epl)
        ok = Al.astype(np.float64) > 0                   # the gauge underflows where FP64 does
        r = np.abs(hess.astype(np.longdouble) - Hl)[ok] / (Al[ok] * np.longdouble(2.) ** -53)
        r_ref = float(np.max(r))
        assert np.all(hess[~ok] == 0.)
        assert np.all(hess[len(sig) - n_far:] == 0.)
        rec[tag + '_sig'], rec[tag + '_epl'], rec[tag + '_hess'] = sig, epl, hess
        rec[tag + '_single'] = np.array(k1)
        rec[tag + '_hess_single'] = one
        rec[tag + '_r_ref'] = np.array(r_ref)
        rec[tag + '_n'] = np.array([n_loc, n_scaled, n_far])
        rec[tag + '_dev_only'] = np.array(bool(dev_only))
        rec[tag + '_sv_sum'] = np.array(float(np.sum(z['par_sv'])))   # the parameters the rows belong to
        print('%-8s %3d rows, far factor %.1f, r_ref = %.3f (mean %.3f), max|H| = %.3e, asymmetry %.1e'
              % (tag, len(sig), far, r_ref, float(np.mean(r)), np.max(np.abs(hess)),
                 np.max(np.abs(hess - hess.transpose(0, 2, 1)))))
    out = os.path.join(GOLD, 'svc_hessian.npz')
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 300 * 1024


if __name__ == '__main__':
    sys.exit(main())
