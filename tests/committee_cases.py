"""Shared by tools/gen_committee.py and the committee tests: the members of tests/golden/committee.npz as parameter dicts and
as façade Materials, the np.longdouble restatement of a member's yield function with its gauge, and the bars of the tests.

Restatement of member m at the unit stress su with the stress scale s, from the recorded tables (all in np.longdouble from
the double inputs; nothing is rounded to double on the way):
    x    = (su s - p 1 if dev_only) / scale_seq,   p = (su_0 + su_1 + su_2) s / 3
    f_L  = sum_k c_k k_k + b,   k_k = exp(-gamma |x - v_k|^2)
    A    = sum_k |c_k| k_k + |b|                                   (the gauge of svc_hessian.npz and yield_locus.npz)
    G    = || grad_x f_L ||_1,  grad_x f_L = -2 gamma sum_k c_k k_k (x - v_k)
Bar (1) of a value:  U A 2^-53 + G 2 ulp(max_j |x_j|),  U = 4 max(r_ref, 1): evaluation noise in units of the reference's
own, plus the two roundings of the features (su s, then the division)."""
import os

import numpy as np

LD = np.longdouble
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS53 = LD(2.) ** -53
NMEM = 6          # five members of the committee and a sixth, dev_only, on member 0's data
REF = dict(E=2.e5, nu=0.3, sy=50., hill=[1.4, 1.0, 0.7, 1.3, 0.8, 1.0])   # the example's reference material
TRAIN = dict(Ce=0.99, Fe=0.1, Nseq=25, gridsearch=False)
CGAMMA = ((3, 1.0), (2, 0.7), (4, 1.5), (1, 2.0), (5, 2.5))               # from the example's grid


def load():
    return np.load(os.path.join(GOLD, 'committee.npz'))


def _dev(s):
    """the reference's sig_dev on (N,6) rows (basic.py:316-325), operation for operation"""
    hyd = np.zeros(s.shape)
    hyd[:, 0:3] = (np.sum(s[:, 0:3], axis=1) / 3.)[:, None]
    return s - hyd


def training_rows(sdata, scale_seq, dev_only):
    """The rows the reference's train_SVC(sdata=..., **TRAIN) fits on, operation for operation (create_sig_data,
    material.py:2032-2054, then create_scaled_input, :2336-2339): every yield stress scaled by the 2 Nseq factors, sequence
    by sequence, divided by scale_seq; the deviator before the scaling and again before the division where dev_only."""
    sd = _dev(sdata) if dev_only else sdata
    seq = np.append(np.linspace(TRAIN['Fe'], TRAIN['Ce'], TRAIN['Nseq']),
                    np.linspace(2. - TRAIN['Ce'], 2. - TRAIN['Fe'], TRAIN['Nseq']))
    st = np.zeros((len(sd) * len(seq), 6))
    for i in range(len(seq)):
        st[i * len(sd):(i + 1) * len(sd), :] = sd[:, 0:6] * seq[i]
    if dev_only:
        st = _dev(st)
    return st / scale_seq


def member_params(z, k):
    """Tables of member k.  The support vectors are rows of the member's training matrix; the fixture records which
    (scikit-learn's support_) and the generator has asserted that `training_rows` rebuilds the reference's
    support_vectors_ bit for bit from the recorded yield stresses -- an eighth of the bytes of the vectors themselves."""
    dev_only, scale_seq = bool(z['m%d_dev_only' % k]), float(z['m%d_scale_seq' % k])
    if 'm%d_sv' % k in z:
        sv = np.array(z['m%d_sv' % k])
    else:
        sdata = np.asarray(z['sig'])[np.asarray(z['subsets'])[k % 5]]
        sv = np.ascontiguousarray(training_rows(sdata, scale_seq, dev_only)[np.asarray(z['m%d_support' % k], dtype=int)])
    return dict(sv=sv, dual=np.array(z['m%d_dual' % k]), intercept=float(z['m%d_intercept' % k]),
                gamma=float(z['m%d_gamma' % k]), scale_seq=scale_seq, sy=float(z['m%d_sy' % k]), dev_only=dev_only)


def cut(p, nsv=None, pad=0, dev_only=None):
    """the member's tables cut to their first nsv vectors, `pad` vectors with a zero coefficient appended (another table
    size, the same function), another dev_only flag"""
    sv, dual = p['sv'][:nsv], p['dual'][:nsv]
    if pad:
        sv = np.vstack((sv, np.tile(sv[:1], (pad, 1))))
        dual = np.concatenate((dual, np.zeros(pad)))
    return dict(p, sv=np.ascontiguousarray(sv), dual=np.ascontiguousarray(dual),
                dev_only=p['dev_only'] if dev_only is None else bool(dev_only))


def facade(p, name='member'):
    """façade Material of a parameter dict, through set_svc"""
    import pylabfea_amd as FE
    m = FE.Material(name=name)
    m.elasticity(E=REF['E'], nu=REF['nu'])
    m.plasticity(sy=p['sy'], sdim=6)
    m.set_svc(p['sv'], p['dual'], p['intercept'], p['gamma'], p['scale_seq'], dev_only=p['dev_only'])
    return m


def restate(p, su, scale, LD=LD):
    """(f_L, A, G, xmax) of the member p at su (N,6) with the stress scale `scale`; with LD=np.float64 the same formula in
    plain FP64 NumPy"""
    su = np.asarray(su, dtype=float).reshape(-1, 6)
    s = su.astype(LD) * LD(scale)
    if p['dev_only']:
        s = s.copy()
        s[:, :3] -= (np.sum(s[:, :3], axis=1) / LD(3))[:, None]
    x = s / LD(p['scale_seq'])
    sv, dual, g, b = p['sv'].astype(LD), p['dual'].astype(LD), LD(p['gamma']), LD(p['intercept'])
    n = len(su)
    f, A, G = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for i in range(n):
        d = x[i][None, :] - sv
        k = np.exp(-g * np.sum(d * d, axis=1))
        f[i] = np.sum(dual * k) + b
        A[i] = np.sum(np.abs(dual) * k) + abs(b)
        G[i] = np.sum(np.abs(-2 * g * ((dual * k) @ d)))
    return f, A, G, np.max(np.abs(x), axis=1).astype(float)


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=float)))


def value_bar(r, A, G, xmax):
    """bar (1) with U = 4 max(r, 1)"""
    return LD(4. * max(float(r), 1.)) * A * EPS53 + G * 2 * ulp(xmax)


def r_units(y, f, A):
    """worst |y - f_L| over the points in units of A 2^-53"""
    return float(np.max(np.abs(np.asarray(y).astype(LD) - f) / (A * EPS53)))


def variance_bar(y, delta, var_ref):
    """bar 2(b): |var - var_ref| <= (4/M) sum_m |y_m - ybar| delta + 4 delta^2 + (M + 2) ulp(var_ref); y (M,N) the
    reference's values, delta (N,) the largest value bar over the members at each point"""
    M = y.shape[0]
    dev = np.sum(np.abs(y - np.mean(y, axis=0)), axis=0)
    d = np.asarray(delta, dtype=float)
    return 4. / M * dev * d + 4. * d * d + (M + 2) * ulp(var_ref)


def two_pass(y):
    """mean and variance over the members in FP64, in member order, as the kernel forms them"""
    M = y.shape[0]
    s = np.zeros(y.shape[1])
    for k in range(M):
        s = s + y[k]
    mean = s / float(M)
    q = np.zeros(y.shape[1])
    for k in range(M):
        d = y[k] - mean
        q = q + d * d
    return mean, q / float(M)
