"""Host side of SVC training: the reference's training data directions and scores (pylabfea/training.py) and the
cross-validation bookkeeping of its grid search, in NumPy only (no SciPy, no scikit-learn).

``load_cases`` places unit stresses on the 3-d / 6-d hypersphere with the reference's low-discrepancy construction
(training.py:83-149); its root finder is Brent's method with the same bracket, tolerances and step rules as the one the
reference calls, so the directions agree with the reference's to rounding.  ``stratified_folds`` and ``param_grid`` reproduce
the fold assignment of ``StratifiedKFold(5)`` without shuffling and the candidate order of ``ParameterGrid`` that the
reference's ``GridSearchCV`` uses; the fits themselves run on the GPU (``_lib.Context.svc_fit_batch``).
``texture_folds`` gives the shuffled ``KFold`` over data sets of the reference's grid search over textures.
"""
import math

import numpy as np

from .basic import sig_eq_j2


def _int_sin_m(x, m):
    """integral of sin^m(t) dt from 0 to x (recursion of training.py:33-55)"""
    if m == 0:
        return x
    if m == 1:
        return 1. - np.cos(x)
    return (m - 1) / m * _int_sin_m(x, m - 2) - np.cos(x) * np.sin(x) ** (m - 1) / m


def _primes():
    k = 2
    while True:
        if all(k % p for p in range(2, int(k ** 0.5) + 1)):
            yield k
        k += 1


def _brentq(f, xa, xb, xtol=1e-8, rtol=4 * np.finfo(float).eps, maxiter=100):
    """Brent's method (R. P. Brent, Algorithms for Minimization without Derivatives, 1973, ch. 4) in the form of the
    bracketing solver the reference calls: inverse quadratic / secant steps accepted when short enough, else bisection."""
    xpre, xcur = float(xa), float(xb)
    fpre, fcur = f(xpre), f(xcur)
    if fpre == 0:
        return xpre
    if fcur == 0:
        return xcur
    if np.signbit(fpre) == np.signbit(fcur):
        raise ValueError('_brentq: f(a) and f(b) must have different signs')
    xblk = fblk = spre = scur = 0.
    for _ in range(maxiter):
        if fpre != 0 and fcur != 0 and np.signbit(fpre) != np.signbit(fcur):
            xblk, fblk = xpre, fpre
            spre = scur = xcur - xpre
        if abs(fblk) < abs(fcur):
            xpre, xcur, xblk = xcur, xblk, xcur
            fpre, fcur, fblk = fcur, fblk, fcur
        delta = (xtol + rtol * abs(xcur)) / 2
        sbis = (xblk - xcur) / 2
        if fcur == 0 or abs(sbis) < delta:
            return xcur
        if abs(spre) > delta and abs(fcur) < abs(fpre):
            if xpre == xblk:   # secant
                stry = -fcur * (xcur - xpre) / (fcur - fpre)
            else:              # inverse quadratic
                dpre = (fpre - fcur) / (xpre - xcur)
                dblk = (fblk - fcur) / (xblk - xcur)
                stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre))
            if 2 * abs(stry) < min(abs(spre), 3 * abs(sbis) - delta):
                spre, scur = scur, stry
            else:
                spre = scur = sbis
        else:
            spre = scur = sbis
        xpre, fpre = xcur, fcur
        xcur += scur if abs(scur) > delta else (delta if sbis > 0 else -delta)
        fcur = f(xcur)
    return xcur


def uniform_hypersphere(d, n):
    """n unit vectors on the d-dimensional hypersphere (training.py:83-121)"""
    points = np.ones((n, d))
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    points[:, 0] = np.sin(t)
    points[:, 1] = np.cos(t)
    for dim, prime in zip(range(2, d), _primes()):
        offset = np.sqrt(prime)
        mult = math.gamma(0.5 * (dim + 1)) / (math.gamma(0.5 * dim) * np.sqrt(np.pi))
        for i in range(n):
            x = i * offset % 1
            deg = _brentq(lambda y: mult * _int_sin_m(y, dim - 1) - x, 0., np.pi)
            for j in range(dim):
                points[i, j] *= np.sin(deg)
            points[i, dim] *= np.cos(deg)
    return points


def load_cases(number_3d, number_6d):
    """Unit stresses (J2 equivalent stress 1): number_3d principal stresses followed by number_6d full Voigt stresses
    (training.py:124-149)"""
    sig_3d = np.zeros((number_3d, 6))
    sig_3d[:, 0:3] = uniform_hypersphere(3, number_3d)
    sig_6d = uniform_hypersphere(6, number_6d)
    allsig = np.concatenate((sig_3d, sig_6d))
    seq = sig_eq_j2(allsig)
    ind = np.nonzero(seq < 1.e-3)[0]
    if len(ind) > 0:
        print('WARNING: Small stresses detected:', ind)
    return allsig / seq[:, None]


def _mcc(a, b):
    """Matthews correlation coefficient of two label vectors (binary; 0 when undefined, as scikit-learn)"""
    a, b = np.asarray(a), np.asarray(b)
    labels = np.unique(np.concatenate([a, b]))
    cm = np.array([[np.sum((a == u) & (b == v)) for v in labels] for u in labels], dtype=float)
    t, p = cm.sum(axis=1), cm.sum(axis=0)
    c, s = np.trace(cm), cm.sum()
    cov_ytyp = c * s - np.dot(t, p)
    cov_ypyp = s ** 2 - np.dot(p, p)
    cov_ytyt = s ** 2 - np.dot(t, t)
    if cov_ypyp * cov_ytyt == 0:
        return 0.0
    return float(cov_ytyp / np.sqrt(cov_ytyt * cov_ypyp))


def training_score(yf_ref, yf_ml, plot=False):
    """MAE, precision, accuracy, recall, F1 score and MCC of an ML yield function against reference values at the same
    stresses (training.py:151-241); points with yield function 0 count as plastic.  ``plot`` is not supported."""
    if plot:
        raise NotImplementedError('training_score: plotting is not supported')
    yf_ref = np.asarray(yf_ref, dtype=float)
    yf_ml = np.asarray(yf_ml, dtype=float)
    r = np.where(np.abs(np.sign(yf_ref)) < 0.9, 1., np.sign(yf_ref))
    m = np.where(np.abs(np.sign(yf_ml)) < 0.9, 1., np.sign(yf_ml))
    TP = int(np.sum((r == 1) & (m == 1)))
    FN = int(np.sum((r == 1) & (m == -1)))
    FP = int(np.sum((r == -1) & (m == 1)))
    TN = int(np.sum((r == -1) & (m == -1)))
    mae = float(np.mean(np.abs(yf_ref - yf_ml)))
    MCC = _mcc(np.sign(yf_ref), np.sign(yf_ml))
    precision = TP / (TP + FP) if TP + FP > 0 else 0.0
    Accuracy = (TP + TN) / (TP + FP + FN + TN) if TP + FP + FN + TN > 0 else 0.0
    Recall = TP / (TP + FN) if TP + FN > 0 else 0.0
    F1Score = 2 * (Recall * precision) / (Recall + precision) if Recall + precision > 1.0e-4 else 0.0
    print('Mean Absolut Error is', mae)
    print('True Positives:', TP, ' True Negatives:', TN, ' False Positives:', FP, ' False Negatives:', FN)
    print('Precision:', precision, ' Accuracy:', Accuracy, ' Recall:', Recall, ' F1score:', F1Score, ' MCC score:', MCC)
    return mae, precision, Accuracy, Recall, F1Score, MCC


TEST_SIG_FACTORS = ((1.5, 1.2, 1.1, 1.01), (0.99, 0.9, 0.8, 0.5))   # outside / inside the yield locus (training.py:282-289)


def create_test_sig(file, number_sig_per_strain=4):
    """Test stresses for a trained yield function from a JSON database of stress-strain data (training.py:244-302):
    ``(ts_sig, epl_tot, yf_ref)``.  The database is read as the reference reads it, ``Data(file, epl_crit=2e-3,
    epl_start=1e-3, epl_max=0.03, depl=0.0)``; every flow stress is scaled by 1.5, 1.2, 1.1, 1.01 (plastic) and by 0.99,
    0.9, 0.8, 0.5 (elastic).  ``ts_sig``: all plastic stresses, data row by data row, then all elastic ones; ``epl_tot``:
    each row's plastic strain ``number_sig_per_strain`` times, the whole list twice; ``yf_ref``: +1 for the first half of
    ``ts_sig``, -1 for the rest.  As in the reference the rows of ``ts_sig`` and ``epl_tot`` pair up only for the default
    ``number_sig_per_strain = 4``."""
    from .data import Data
    md = Data(file, epl_crit=2.e-3, epl_start=1.e-3, epl_max=0.03, depl=0.0).mat_data
    fs = np.asarray(md['flow_stress'], dtype=float)
    ep = np.asarray(md['plastic_strain'], dtype=float)
    ts_sig = np.concatenate([(fs[:, None, :] * np.array(f)[None, :, None]).reshape(-1, fs.shape[1]) for f in TEST_SIG_FACTORS])
    epl_tot = np.tile(np.repeat(ep, int(number_sig_per_strain), axis=0), (2, 1))
    half = len(ts_sig) // 2
    yf_ref = np.concatenate((np.ones(half), -np.ones(len(ts_sig) - half)))
    return ts_sig, epl_tot, yf_ref


def stratified_folds(y, n_splits=5):
    """Test-fold index arrays of stratified k-fold cross-validation without shuffling, in the assignment of
    scikit-learn's ``StratifiedKFold(n_splits)`` (what ``GridSearchCV(cv=5)`` uses for a classifier): the samples,
    sorted by class in order of first appearance, are dealt to the folds round-robin, so each fold holds every class in
    proportion; within a class the samples keep their order."""
    y = np.asarray(y)
    _, first, y_inv = np.unique(y, return_index=True, return_inverse=True)
    # classes re-encoded in order of appearance
    order = np.argsort(first, kind='stable')
    enc = np.empty(len(order), dtype=int)
    enc[order] = np.arange(len(order))
    y_enc = enc[y_inv]
    n_classes = len(order)
    counts = np.bincount(y_enc)
    if np.all(n_splits > counts):
        raise ValueError('n_splits=%d cannot be greater than the number of members in each class.' % n_splits)
    alloc = np.asarray([np.bincount(np.sort(y_enc)[i::n_splits], minlength=n_classes) for i in range(n_splits)])
    test_folds = np.empty(len(y), dtype=int)
    for k in range(n_classes):
        folds_for_class = np.arange(n_splits).repeat(alloc[:, k])
        test_folds[y_enc == k] = folds_for_class
    return [np.nonzero(test_folds == i)[0] for i in range(n_splits)]


def param_grid(cvals, gvals):
    """candidates of ``ParameterGrid({'C': cvals, 'gamma': gvals})``: C outer, gamma inner, lists in the given order"""
    return [(c, g) for c in cvals for g in gvals]


def texture_folds(nset, n_splits=5, seed=42):
    """(train, test) index arrays of the texture grid search (material.py:1551-1552): scikit-learn's
    ``KFold(n_splits, shuffle=True, random_state=seed).split`` over ``nset`` data sets.  The indices 0 .. nset - 1 are
    shuffled by ``numpy.random.RandomState(seed)``, cut into ``n_splits`` consecutive test folds of which the first
    ``nset % n_splits`` hold one index more, and every fold's train and test indices come back in ascending order."""
    if n_splits > nset:
        raise ValueError('Cannot have number of splits n_splits={0} greater than the number of samples: '
                         'n_samples={1}.'.format(n_splits, nset))
    idx = np.arange(nset)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(n_splits, nset // n_splits, dtype=int)
    sizes[:nset % n_splits] += 1
    out, start = [], 0
    for sz in sizes:
        test = np.sort(idx[start:start + sz])
        out.append((np.setdiff1d(np.arange(nset), test), test))
        start += sz
    return out
