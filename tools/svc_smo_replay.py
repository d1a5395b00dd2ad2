#!/usr/bin/env python3
"""CPU replay of the SMO rules that the device solver (pylabfea_amd/csrc/plfx_svm.hpp) follows, in NumPy.

This is the debugging aid for the device solver: libsvm's non-shrinking C-SVC solver step for step (second-order working-set
selection, the analytic two-variable update, G from both kernel rows), with kernel rows computed in FP64 and stored as FP32
like libsvm's ``Qfloat``.  It can print the working pair (i, j) of every iteration, so the first iteration where the device
and this replay (or libsvm) part can be found.  It is also the reference of tests/test_gpu_svc_smo.py (pinned to libsvm by
tests/test_svc_replay_cpu.py), together with the FP64 checks ``kkt_gap`` and ``dual_obj``.  ``svr`` is the same for the epsilon-SVR dual (k_svr, Material.setup_fgrad_SVM), the reference of
tests/test_gpu_svr.py, pinned to libsvm by tests/test_svr_replay_cpu.py.

The problem is laid out as libsvm sees it inside scikit-learn: the classes are sorted, so the rows of label -1 come first
(internal y = +1) and the rows of label +1 follow (internal y = -1).  Results are returned in scikit-learn's convention
(``dual_coef_ = label * alpha``, ``intercept_ = -rho``, decision > 0 <-> label +1) with ``support_`` in libsvm's order.

Usage:  python tools/svc_smo_replay.py FIXTURE.npz CASE [--trace N]     (FIXTURE from tools/gen_svc_training.py)
"""
import argparse
import sys

import numpy as np

TAU = 1e-12


def libsvm_order(y):
    """row order of libsvm's binary sub-problem (label -1 first) and the internal labels in that order"""
    y = np.asarray(y)
    perm = np.concatenate([np.nonzero(y < 0)[0], np.nonzero(y > 0)[0]])
    return perm, np.where(y[perm] < 0, 1, -1).astype(np.int8)


def dot_seq(A, x):
    """A @ x summed feature by feature in order, as libsvm's dense dot and the device do (a BLAS dot may not)"""
    s = np.zeros(len(A))
    for f in range(A.shape[1]):
        s = s + A[:, f] * x[f]
    return s


def smo(X, y, C, gamma, tol=1e-3, max_iter=-1, trace=0):
    """non-shrinking libsvm SMO on (X, y in {-1, +1}); returns dict(support_, dual_coef_, intercept_, n_iter_, obj, alpha,
    perm, status).  max_iter <= 0 (or None) means libsvm's default max(10 000 000, 100 n); status is 1 when the loop ended
    because the iteration count reached max_iter (libsvm's warning), else 0."""
    X = np.ascontiguousarray(X, dtype=float)
    perm, yi = libsvm_order(y)
    Xp = X[perm]
    n = len(Xp)
    if max_iter is None or max_iter <= 0:
        max_iter = max(10000000, 100 * n)
    xsq = np.zeros(n)
    for f in range(Xp.shape[1]):
        xsq = xsq + Xp[:, f] * Xp[:, f]
    yd = yi.astype(float)

    def row(i):   # Q_i as libsvm's SVC_Q::get_Q: (Qfloat)(y_i y_t K(i, t))
        k = np.exp(-gamma * (xsq[i] + xsq - 2 * dot_seq(Xp, Xp[i])))
        return (yd[i] * yd * k).astype(np.float32)

    QD = np.exp(-gamma * (xsq + xsq - 2 * xsq))
    alpha = np.zeros(n)
    G = -np.ones(n)
    it = 0
    while it < max_iter:
        up = alpha >= C
        lo = alpha <= 0
        # i: argmax of -y G over I_up, ties to the LAST index (libsvm compares with >=)
        v = np.where(yi > 0, np.where(~up, -G, -np.inf), np.where(~lo, G, -np.inf))
        Gmax = v.max()
        if Gmax == -np.inf:
            break
        i = n - 1 - int(np.argmax(v[::-1]))
        Qi = row(i)
        cand = np.where(yi > 0, ~lo, ~up)
        g2 = np.where(yi > 0, G, -G)
        Gmax2 = np.max(np.where(cand, g2, -np.inf))
        gd = np.where(yi > 0, Gmax + G, Gmax - G)
        quad = QD[i] + QD - np.where(yi > 0, 1., -1.) * (2.0 * yd[i] * Qi.astype(float))
        quad = np.where(quad > 0, quad, TAU)
        od = np.where(cand & (gd > 0), -(gd * gd) / quad, np.inf)
        if Gmax + Gmax2 < tol or not np.any(cand & (gd > 0)):
            break
        j = n - 1 - int(np.argmin(od[::-1]))
        it += 1
        if trace and it <= trace:
            print('iter %d  i=%d j=%d  Gmax=%.17g' % (it, i, j, Gmax))
        Qj = row(j)
        ai, aj = alpha[i], alpha[j]
        if yi[i] != yi[j]:
            q = QD[i] + QD[j] + 2 * float(Qi[j])
            if q <= 0:
                q = TAU
            delta = (-G[i] - G[j]) / q
            diff = ai - aj
            ni, nj = ai + delta, aj + delta
            if diff > 0:
                if nj < 0:
                    nj, ni = 0., diff
            elif ni < 0:
                ni, nj = 0., -diff
            if diff > 0:    # C_i - C_j = 0
                if ni > C:
                    ni, nj = C, C - diff
            elif nj > C:
                nj, ni = C, C + diff
        else:
            q = QD[i] + QD[j] - 2 * float(Qi[j])
            if q <= 0:
                q = TAU
            delta = (G[i] - G[j]) / q
            s = ai + aj
            ni, nj = ai - delta, aj + delta
            if s > C:
                if ni > C:
                    ni, nj = C, s - C
            elif nj < 0:
                nj, ni = 0., s
            if s > C:
                if nj > C:
                    nj, ni = C, s - C
            elif ni < 0:
                ni, nj = 0., s
        alpha[i], alpha[j] = ni, nj
        G += Qi.astype(float) * (ni - ai) + Qj.astype(float) * (nj - aj)
    rho = calc_rho(alpha, G, yi, C)
    sv = np.nonzero(alpha > 0)[0]
    return dict(support_=perm[sv], dual_coef_=-(yd[sv] * alpha[sv]), intercept_=rho, n_iter_=it,
                obj=0.5 * float(np.sum(alpha * (G - 1.))), alpha=alpha, perm=perm, status=int(it >= max_iter))


def svr(X, t, C, gamma, epsilon=0.1, tol=1e-3, max_iter=-1, trace=0):
    """non-shrinking libsvm SMO for the epsilon-SVR dual (solve_epsilon_svr) on (X, targets t), rows in the order given:
    2l variables, k < l with sign +1 and linear term epsilon - t_k, k + l with sign -1 and epsilon + t_k,
    Q_ab = s_a s_b K(a mod l, b mod l) from FP32 kernel rows, alpha = 0 and G = p at the start; selection, update and rho as in
    ``smo``.  Returns dict(support_, dual_coef_ (over the support), intercept_ (= -rho), n_iter_, obj, coef (l,), alpha
    (2l,), G (2l,), status) in scikit-learn's convention (prediction = sum coef K + intercept_).  max_iter <= 0 (or None)
    means libsvm's default max(10 000 000, 100 * 2l)."""
    X = np.ascontiguousarray(X, dtype=float)
    t = np.asarray(t, dtype=float).reshape(-1)
    l = len(X)
    n = 2 * l
    if max_iter is None or max_iter <= 0:
        max_iter = max(10000000, 100 * n)
    xsq = np.zeros(l)
    for f in range(X.shape[1]):
        xsq = xsq + X[:, f] * X[:, f]
    yi = np.concatenate([np.ones(l, dtype=np.int8), -np.ones(l, dtype=np.int8)])
    yd = yi.astype(float)
    p = np.concatenate([epsilon - t, epsilon + t])

    def row(i):   # SVR_Q::get_Q: (Qfloat)K(i mod l, .) once, then the signs (exact)
        k = np.exp(-gamma * (xsq[i % l] + xsq - 2 * dot_seq(X, X[i % l]))).astype(np.float32)
        return (yd[i] * yd).astype(np.float32) * np.concatenate([k, k])

    qd = np.exp(-gamma * (xsq + xsq - 2 * xsq))
    QD = np.concatenate([qd, qd])
    alpha = np.zeros(n)
    G = p.copy()
    it = 0
    while it < max_iter:
        up = alpha >= C
        lo = alpha <= 0
        v = np.where(yi > 0, np.where(~up, -G, -np.inf), np.where(~lo, G, -np.inf))
        Gmax = v.max()
        if Gmax == -np.inf:
            break
        i = n - 1 - int(np.argmax(v[::-1]))
        Qi = row(i)
        cand = np.where(yi > 0, ~lo, ~up)
        g2 = np.where(yi > 0, G, -G)
        Gmax2 = np.max(np.where(cand, g2, -np.inf))
        gd = np.where(yi > 0, Gmax + G, Gmax - G)
        quad = QD[i] + QD - np.where(yi > 0, 1., -1.) * (2.0 * yd[i] * Qi.astype(float))
        quad = np.where(quad > 0, quad, TAU)
        od = np.where(cand & (gd > 0), -(gd * gd) / quad, np.inf)
        if Gmax + Gmax2 < tol or not np.any(cand & (gd > 0)):
            break
        j = n - 1 - int(np.argmin(od[::-1]))
        it += 1
        if trace and it <= trace:
            print('iter %d  i=%d j=%d  Gmax=%.17g' % (it, i, j, Gmax))
        Qj = row(j)
        ai, aj = alpha[i], alpha[j]
        if yi[i] != yi[j]:
            q = QD[i] + QD[j] + 2 * float(Qi[j])
            if q <= 0:
                q = TAU
            delta = (-G[i] - G[j]) / q
            diff = ai - aj
            ni, nj = ai + delta, aj + delta
            if diff > 0:
                if nj < 0:
                    nj, ni = 0., diff
            elif ni < 0:
                ni, nj = 0., -diff
            if diff > 0:
                if ni > C:
                    ni, nj = C, C - diff
            elif nj > C:
                nj, ni = C, C + diff
        else:
            q = QD[i] + QD[j] - 2 * float(Qi[j])
            if q <= 0:
                q = TAU
            delta = (G[i] - G[j]) / q
            s = ai + aj
            ni, nj = ai - delta, aj + delta
            if s > C:
                if ni > C:
                    ni, nj = C, s - C
            elif nj < 0:
                nj, ni = 0., s
            if s > C:
                if nj > C:
                    nj, ni = C, s - C
            elif ni < 0:
                ni, nj = 0., s
        alpha[i], alpha[j] = ni, nj
        G += Qi.astype(float) * (ni - ai) + Qj.astype(float) * (nj - aj)
    rho = calc_rho(alpha, G, yi, C)
    coef = alpha[:l] - alpha[l:]
    sv = np.nonzero(np.abs(coef) > 0)[0]
    return dict(support_=sv, dual_coef_=coef[sv], intercept_=-rho, n_iter_=it, obj=0.5 * float(np.sum(alpha * (G + p))),
                coef=coef, alpha=alpha, G=G, status=int(it >= max_iter))


def svr_kkt_gap(X, t, coef, alpha, C, gamma, epsilon):
    """m(a) - M(a) of an epsilon-SVR fit in FP64: G = s (K coef) + p over the 2l variables (alpha as ``svr`` returns it
    decides which variables sit at a bound); -inf when one of the two index sets is empty"""
    X, t = np.asarray(X, dtype=float), np.asarray(t, dtype=float)
    l = len(X)
    f = kernel_fp64(X, X, gamma) @ np.asarray(coef, dtype=float)
    y = np.concatenate([np.ones(l), -np.ones(l)])
    G = y * np.concatenate([f, f]) + np.concatenate([epsilon - t, epsilon + t])
    a = np.asarray(alpha, dtype=float)
    v = -y * G
    up = ((y > 0) & (a < C)) | ((y < 0) & (a > 0))
    low = ((y > 0) & (a > 0)) | ((y < 0) & (a < C))
    if not np.any(up) or not np.any(low):
        return -np.inf
    return np.max(v[up]) - np.min(v[low])


def calc_rho(alpha, G, yi, C):
    """libsvm's Solver::calculate_rho, sequential sum as there"""
    ub, lb, s, nf = np.inf, -np.inf, 0., 0
    for a, g, y in zip(alpha, G, yi):
        yG = y * g
        if a >= C:
            if y == -1:
                ub = min(ub, yG)
            else:
                lb = max(lb, yG)
        elif a <= 0:
            if y == 1:
                ub = min(ub, yG)
            else:
                lb = max(lb, yG)
        else:
            nf += 1
            s += yG
    return s / nf if nf else 0.5 * (ub + lb)


def kernel_fp64(A, B, gamma):
    """RBF kernel matrix K(A, B) in FP64 (squared distances from the norms, clipped at 0)"""
    sa, sb = np.sum(A * A, axis=1), np.sum(B * B, axis=1)
    return np.exp(-gamma * np.maximum(sa[:, None] + sb[None, :] - 2. * A @ B.T, 0.))


def kkt_gap(X, y, alpha, C, gamma):
    """m(a) - M(a) of a fit in FP64 (labels y in {-1, +1}, alpha in the order of X): the maximal violation of the KKT
    conditions, which the solver drives below tol; -inf when one of the two index sets is empty"""
    X, y, a = np.asarray(X, dtype=float), np.asarray(y, dtype=float), np.asarray(alpha, dtype=float)
    sv = np.nonzero(a > 0)[0]
    G = y * (kernel_fp64(X, X[sv], gamma) @ (y[sv] * a[sv])) - 1.
    v = -y * G
    up = ((y > 0) & (a < C)) | ((y < 0) & (a > 0))
    low = ((y > 0) & (a > 0)) | ((y < 0) & (a < C))
    if not np.any(up) or not np.any(low):
        return -np.inf
    return np.max(v[up]) - np.min(v[low])


def dual_obj(X, y, alpha, gamma):
    """1/2 a'Qa - e'a in FP64"""
    X, y, a = np.asarray(X, dtype=float), np.asarray(y, dtype=float), np.asarray(alpha, dtype=float)
    sv = np.nonzero(a > 0)[0]
    ya = y[sv] * a[sv]
    return 0.5 * float(ya @ (kernel_fp64(X[sv], X[sv], gamma) @ ya)) - float(np.sum(a))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('fixture')
    ap.add_argument('case')
    ap.add_argument('--trace', type=int, default=0, help='print (i, j) of the first N iterations')
    a = ap.parse_args()
    z = np.load(a.fixture)
    c = a.case
    if c + '_X' in z.files:
        X, y = z[c + '_X'], z[c + '_y']
    else:   # compact form: the training stresses are seq[i] * sdata block by block, the features those over sy
        sd, seq = z[c + '_sdata'], z[c + '_seq']
        X = (seq[:, None, None] * sd[None, :, :]).reshape(-1, sd.shape[1]) / float(z[c + '_sy'])
        y = np.repeat(np.where(np.arange(len(seq)) < int(z[c + '_Nseq']), -1., 1.), len(sd))
    r = smo(X, y, float(z[c + '_C']), float(z[c + '_gamma']), trace=a.trace)
    print('n_iter %d (libsvm without shrinking: %d), status %d, nSV %d (%d), intercept %.17g (%.17g)' % (
        r['n_iter_'], int(z[c + '_ns_n_iter']), r['status'], len(r['support_']), len(z[c + '_ns_support']), r['intercept_'],
        float(z[c + '_ns_intercept'])))
    return 0


if __name__ == '__main__':
    sys.exit(main())
