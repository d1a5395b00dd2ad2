#!/usr/bin/env python3
"""Golden-vector generator for Committee / plfx_committee_yf (TEST INFRASTRUCTURE, development machine only): runs the
unmodified reference and scikit-learn and writes tests/golden/committee.npz.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_committee.py

The material of the reference's examples/Active_Learning/qbc_svc.py (E = 2e5, nu = 0.3, sy = 50, Hill 1.4 / 1.0 / 0.7 / 1.3 /
0.8 / 1.0), its 42 load cases load_cases(14, 28) and their yield stresses by the example's fsolve.  Five members by
train_SVC(sdata=subset, Ce=0.99, Fe=0.1, Nseq=25, gridsearch=False) on seeded 80 % subsets with distinct (C, gamma) from the
example's grid; a sixth on member 0's data with dev_only set before the reference's train_SVC (its training path honours the
attribute: create_scaled_input, material.py:2336).  Per member: support vectors (as the indices of the training rows they are, where those rows are
rebuilt to the bit from the recorded yield stresses; tests/committee_cases.py), dual coefficients, intercept, gamma,
scale_seq, sy, dev_only.

Candidates: 256 seeded angle vectors in the example's bounds, their unit stresses through the reference's
sig_spherical_to_cartesian; eight (angles, seq) pairs with their vectors.  The reference's calc_yf(su * 0.5 * sy_m) per member,
np.var over the first five, and per member r_ref: the reference's worst |calc_yf - f_L| over the candidates in units of
A 2^-53 (tests/committee_cases.py).  The largest reference variance must exceed the runner-up by more than twice the variance
bar of the tests; if not, the next candidate seed is taken.  The margin is printed."""
import contextlib
import io
import os
import sys

import numpy as np
from scipy.optimize import fsolve

import pylabfea as FE  # the reference
from pylabfea.training import load_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import committee_cases as CC  # noqa: E402

SUBSET_SEED = 20231
NCAND = 256


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def main():
    rec = {}
    mat_h = FE.Material(name='Hill-reference')
    mat_h.elasticity(E=CC.REF['E'], nu=CC.REF['nu'])
    mat_h.plasticity(sy=CC.REF['sy'], hill=CC.REF['hill'])
    sunit = load_cases(number_3d=14, number_6d=28)
    x1 = fsolve(mat_h.find_yloc, np.ones(len(sunit)) * mat_h.sy, args=(sunit,), xtol=1.e-5)
    sig = sunit * x1[:, None]
    rec['sunit'], rec['sig'] = sunit, sig

    rng = np.random.default_rng(SUBSET_SEED)
    subsets = [rng.choice(len(sig), int(len(sig) * 0.8), replace=False) for _ in range(5)]
    rec['subsets'] = np.array(subsets)
    rec['cgamma'] = np.array(CC.CGAMMA, dtype=float)
    members = []
    for k in range(CC.NMEM):
        C, gamma = CC.CGAMMA[k % 5]
        m = FE.Material(name='ML-Hill_%d' % k)
        if k == 5:
            m.dev_only = True
        quiet(m.train_SVC, C=C, gamma=gamma, sdata=sig[subsets[k % 5], :], verbose=0, **CC.TRAIN)
        assert m.dev_only == (k == 5) and m.sdim == 6 and m.Ndof == 6
        svm = m.svm_yf
        rec['m%d_dual' % k] = np.array(svm.dual_coef_[0], dtype=float)
        rec['m%d_intercept' % k] = np.array(float(svm.intercept_[0]))
        rec['m%d_gamma' % k] = np.array(float(svm._gamma))
        rec['m%d_scale_seq' % k] = np.array(float(m.scale_seq))
        rec['m%d_sy' % k] = np.array(float(m.sy))
        rec['m%d_dev_only' % k] = np.array(bool(m.dev_only))
        # the support vectors are rows of the training matrix: recorded as scikit-learn's support_ where
        # committee_cases.training_rows rebuilds them to the bit from the recorded yield stresses, else as they are
        rows = CC.training_rows(sig[subsets[k % 5], :], float(m.scale_seq), bool(m.dev_only))
        sv = np.array(svm.support_vectors_, dtype=float)
        if rows.shape[0] < 32768 and np.array_equal(rows[svm.support_], sv):
            rec['m%d_support' % k] = np.array(svm.support_, dtype=np.int16)
        else:
            print('member %d: support vectors recorded in full' % k)
            rec['m%d_sv' % k] = sv
        members.append(m)
    rec['dev_only_from_training'] = np.array(True)   # member 5 comes out of the reference's train_SVC, not from a copied table

    # the helper's own cases
    hrng = np.random.default_rng(7)
    ha = hrng.uniform(0., 1., (8, 5)) * np.array([np.pi] + [2 * np.pi] * 4)
    hs = np.concatenate(([1.], hrng.uniform(0.5, 80., 7)))
    rec['helper_angles'], rec['helper_seq'] = ha, hs
    rec['helper_out'] = np.array([FE.sig_spherical_to_cartesian(ha[i], seq=hs[i]) for i in range(8)])

    P = [CC.member_params(rec, k) for k in range(CC.NMEM)]
    for seed in range(100, 140):
        crng = np.random.default_rng(seed)
        ang = crng.uniform(0., 1., (NCAND, 5)) * np.array([np.pi] + [2 * np.pi] * 4)
        su = np.array([FE.sig_spherical_to_cartesian(a) for a in ang])
        yf = np.array([np.asarray(m.calc_yf(su * 0.5 * m.sy), dtype=float) for m in members])
        var = np.var(yf[:5], axis=0)
        r_ref, bars = [], []
        for k in range(CC.NMEM):
            f, A, G, xm = CC.restate(P[k], su, 0.5 * P[k]['sy'])
            r_ref.append(CC.r_units(yf[k], f, A))
            bars.append(np.asarray(CC.value_bar(r_ref[-1], A, G, xm), dtype=float))
        delta = np.max(np.array(bars[:5]), axis=0)
        vbar = CC.variance_bar(yf[:5], delta, var)
        order = np.argsort(var)
        top, second = order[-1], order[-2]
        margin = var[top] - var[second]
        need = 2. * max(vbar[top], vbar[second])
        print('candidate seed %d: largest variance %.6e at %d, runner-up %.6e, margin %.3e, twice the bar %.3e'
              % (seed, var[top], top, var[second], margin, need))
        if margin > need:
            break
    else:
        raise SystemExit('no candidate seed with a clear maximiser')
    rec['cand_seed'] = np.array(seed)
    rec['cand_angles'], rec['cand_su'] = ang, su
    rec['yf_ref'], rec['var_ref'], rec['r_ref'] = yf, var, np.array(r_ref)
    rec['argmax_ref'] = np.array(int(top))
    for k in range(CC.NMEM):
        print('member %d: nsv %4d, sy %.4f, C %g, gamma %g, dev_only %d, r_ref %.2f'
              % (k, len(P[k]['sv']), P[k]['sy'], CC.CGAMMA[k % 5][0], P[k]['gamma'], P[k]['dev_only'], r_ref[k]))

    out = os.path.join(CC.GOLD, 'committee.npz')
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 100 * 1024


if __name__ == '__main__':
    sys.exit(main())
