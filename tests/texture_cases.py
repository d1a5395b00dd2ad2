"""Shared by tools/gen_texture_svc.py and the texture tests: the cases of tests/golden/texture_svc.npz, its
JSON databases, the trained tables as parameter dicts, the kernel's arithmetic as a NumPy transcription and the np.longdouble
restatement of the texture SVC along a ray.

Parameter dict p: sv (nsv, 6 + tdim) standardised support vectors, dual (nsv,), intercept, gamma, mean / scale (6 + tdim,)
of the scaler, dev_only, tdim.

Specification of the device's arithmetic (`transcribe`), all FP64:
    s       = sig, or sig with the mean of its three normal components taken off them when dev_only
    f_j     = (s_j - mean_j) / scale_j, j < 6;   f_{6+t} = (tex_t - mean_{6+t}) / scale_{6+t}
    d2_i    = sum_j (f_j - v_ij)^2, accumulated in feature order
    term_i  = dual_i exp(-gamma d2_i)
    y       = [sum of the terms in the order of the 16-lane row] + intercept
The row order: lane L of 16 takes the vectors L, L + 16, ... into two accumulators (vectors L, L + 32, ... and L + 16,
L + 48, ...), adds the two, and the lanes are closed by the butterfly (L ^ 1, L ^ 2, the mirrored half of 8, the mirrored row).  The
transcription differs from the device in the exponential (NumPy's against the device's exp2 polynomial) and in the fused
multiply-adds; both are covered by the fixture's `calib`."""
import json
import os

import numpy as np

from ray_cases import march_replay as _march_replay, ulp

LD = np.longdouble
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = os.path.join(GOLD, 'texture_svc.npz')
EPS53 = LD(2.) ** -53
DESCRIPTORS = ('GSH_3', 'GSH_7')
NSET, TRAIN, HOLD, NA = 6, (0, 1, 2, 3, 4), (5,), 72
DATA_KW = dict(epl_crit=2.e-3, epl_start=1.e-3, epl_max=0.03, depl=1.e-3, wh_data=False, tx_data=True)
TRAIN_KW = dict(C=10, gamma=1, Fe=0.8, Ce=0.95, Nseq=2)
GRID = dict(cvals=[1, 10], gvals=[0.5, 1])
# mat_data fields recorded per data set (flow_stress and plastic_strain for set 0 only: they are rows of the database)
MD_SCALAR = ('epc', 'ep_start', 'ep_max', 'peeq_max', 'sy_av', 'Nlc', 'Ncyl', 'tdim', 'tx_index', 'sdim', 'Ntext')
MD_ARRAY = ('lc_indices', 'elast_const', 'sig_ideal', 'transition_ind', 'texture')
MD_BIG = ('flow_stress', 'plastic_strain')


def load():
    return np.load(FIXTURE, allow_pickle=False)


def write_databases(z, directory):
    """the six JSON databases of the fixture as files; returns their names"""
    names = []
    for k in range(NSET):
        name = 'texture_db_%d.json' % k
        with open(os.path.join(str(directory), name), 'wb') as fp:
            fp.write(bytes(np.asarray(z['db_%d' % k]).tobytes()))
        names.append(name)
    return names


def read_sets(FE, z, directory, desc):
    """Data of package FE on the six databases with the descriptor `desc`"""
    import contextlib
    import io
    import random
    import warnings
    out = []
    for name in write_databases(z, directory):
        random.seed(0)   # the reference's elastic fit permutes its pairs with random.sample
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            out.append(FE.Data(name, path_data=str(directory), tx_descriptor=desc, **DATA_KW))
    return out


def stress_dev(s):
    s = np.array(s, dtype=float)
    s[:, :3] -= (np.sum(s[:, :3], axis=1) / 3.)[:, None]
    return s


def tables(z, desc, dev=False):
    """parameter dict of the fit recorded for the descriptor (trained on the sets TRAIN)"""
    pre = '%s_%s' % (desc, 'dev' if dev else 'full')
    tdim = int(desc.split('_')[1])
    rows = train_rows(z, desc)
    mean, scale = np.array(z[pre + '_mean']), np.array(z[pre + '_scale'])
    x = np.array(rows)
    if dev:
        x[:, :6] = stress_dev(x[:, :6])
    X = (x - mean) / scale
    sup = np.asarray(z[pre + '_support'], dtype=int)
    # (dev: the reference's rows hold the deviator already and take it once more; its vectors are recorded where the two
    # roundings differ in the last place)
    sv = np.array(z[pre + '_sv']) if pre + '_sv' in z else X[sup]
    return dict(sv=np.ascontiguousarray(sv), dual=np.array(z[pre + '_dual']), intercept=float(z[pre + '_intercept']),
                gamma=float(TRAIN_KW['gamma']), mean=mean, scale=scale, dev_only=bool(dev), tdim=tdim, X=X,
                y=np.array(z['y_train']), support=sup, n_iter=int(z[pre + '_n_iter']))


def all_rows(z, desc):
    """unscaled rows [stress | texture] of all six sets, in set order"""
    tdim = int(desc.split('_')[1])
    st = np.array(z['rows_stress'])
    per = len(st) // NSET
    tex = np.repeat(np.array(z['gsh'])[:, 1:1 + tdim], per, axis=0)
    return np.concatenate((st, tex), axis=1)


def train_rows(z, desc):
    r = all_rows(z, desc)
    per = len(r) // NSET
    return r[:per * len(TRAIN)]


def textures(z, desc):
    tdim = int(desc.split('_')[1])
    return np.ascontiguousarray(np.array(z['gsh'])[:, 1:1 + tdim])


def cut(p, nsv=None, pad=0, tdim=None, intercept=None):
    """the tables cut to their first nsv vectors and to tdim texture columns, `pad` vectors with a zero coefficient
    appended (another table size, the same function), another intercept"""
    d = 6 + (p['tdim'] if tdim is None else tdim)
    sv, dual = p['sv'][:nsv, :d], p['dual'][:nsv]
    if pad:
        sv = np.vstack((sv, np.tile(sv[:1], (pad, 1))))
        dual = np.concatenate((dual, np.zeros(pad)))
    return dict(p, sv=np.ascontiguousarray(sv), dual=np.ascontiguousarray(dual), mean=p['mean'][:d].copy(),
                scale=p['scale'][:d].copy(), tdim=d - 6, intercept=p['intercept'] if intercept is None else float(intercept))


def features(p, sig, tex, LD=np.float64):
    """standardised features (N, 6 + tdim) of stresses sig (N,6) and textures tex (1 or N, tdim)"""
    s = np.array(sig).reshape(-1, 6).astype(LD)
    if p['dev_only']:
        s[:, :3] -= (np.sum(s[:, :3], axis=1) / LD(3))[:, None]
    t = np.broadcast_to(np.asarray(tex, dtype=float).reshape(-1, p['tdim']), (len(s), p['tdim'])).astype(LD)
    return (np.concatenate((s, t), axis=1) - p['mean'].astype(LD)) / p['scale'].astype(LD)


def row_sum(terms):
    """sum of the terms (nsv,) in the order of the 16-lane row"""
    n = len(terms)
    lane = np.zeros(16)
    for L in range(16):
        acc = [0., 0.]
        for k in range(L, n, 32):
            acc[0] = acc[0] + terms[k]
            if k + 16 < n:
                acc[1] = acc[1] + terms[k + 16]
        lane[L] = acc[0] + acc[1]
    v = lane
    v = v + v[np.arange(16) ^ 1]
    v = v + v[np.arange(16) ^ 2]
    v = v + v[np.array([7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8])]
    v = v + v[::-1]
    return v[0]


def transcribe(p, sig, tex):
    """the device's arithmetic as specified in the module docstring, FP64 NumPy"""
    f = features(p, sig, tex)
    out = np.empty(len(f))
    for i in range(len(f)):
        d2 = np.zeros(len(p['sv']))
        for j in range(f.shape[1]):
            d = f[i, j] - p['sv'][:, j]
            d2 = d2 + d * d
        out[i] = row_sum(p['dual'] * np.exp(-p['gamma'] * d2)) + p['intercept']
    return out


def restate(p, su, tex, x, LD=LD):
    """(f_L, f_L', A) at the factors x (N,) along su (N,6) at the textures tex (1 or N, tdim): the decision function, its
    derivative along the ray and the gauge A = sum |c_i| k_i + |b|, in np.longdouble from the double inputs"""
    su = np.asarray(su, dtype=float).reshape(-1, 6)
    x = np.asarray(x, dtype=LD).reshape(-1)
    phi = features(p, su.astype(LD) * x[:, None], tex, LD=LD)
    s = su.astype(LD)
    if p['dev_only']:
        s = s.copy()
        s[:, :3] -= (np.sum(s[:, :3], axis=1) / LD(3))[:, None]
    dphi = np.zeros_like(phi)
    dphi[:, :6] = s / p['scale'][:6].astype(LD)
    sv, dual, g, b = p['sv'].astype(LD), p['dual'].astype(LD), LD(p['gamma']), LD(p['intercept'])
    n = len(su)
    f, df, A = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for i in range(n):
        d = phi[i][None, :] - sv
        k = np.exp(-g * np.sum(d * d, axis=1))
        f[i] = np.sum(dual * k) + b
        df[i] = -2 * g * np.sum(dual * k * (d @ dphi[i]))
        A[i] = np.sum(np.abs(dual) * k) + abs(b)
    return f, df, A


def value_bar(calib, yf):
    """bar (1), the bar of DESIGN.md §21: 4 max(calib, 1e-12 max|yf|)"""
    return 4. * max(float(calib), 1e-12 * float(np.max(np.abs(yf))))


def snorm(Na=NA):
    """the rays of examples/Texture/train_texture.py: sig_cyl2princ([1, theta]) padded to six components"""
    theta = np.linspace(-np.pi, np.pi, Na)
    a = np.array([1., -0.5, -0.5]) / np.sqrt(1.5)
    b = np.array([0., 0.5, -0.5]) * np.sqrt(2)
    sp = (np.tensordot(np.cos(theta), a, axes=0) + np.tensordot(np.sin(theta), b, axes=0)) * np.sqrt(2. / 3.) * \
        np.array([np.ones(Na)] * 3).T
    return theta, np.concatenate((sp, np.zeros_like(sp)), axis=1)


def facade(FE, z, directory, desc, dev=False):
    """façade texture material on the fixture's databases, untrained"""
    sets = read_sets(FE, z, directory, desc)
    m = FE.Material(name='ML-texture-' + desc)
    m.dev_only = bool(dev)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m.from_data([d.mat_data for d in sets])
    return m, sets


def install(m, p):
    """install the parameter dict p in the façade texture material m"""
    m.tdim, m.Ndof = p['tdim'], 6 + p['tdim']
    m.set_tex_svc(p['sv'], p['dual'], p['intercept'], p['gamma'], p['mean'], p['scale'], dev_only=p['dev_only'])
    return m


def database_json(name, tx_index, gsh, sig_y, normal, CV):
    """One JSON database in the reference's legacy layout: per load case a proportional path 0, 0.5, 1 x the yield stress
    (elastic), then five steps of ideal plastic flow along `normal` with PEEQ 0.001 .. 0.005, the numbers rounded so that the
    text stays small; the `Texture` entry carries name, texture_index and the 38 GSH coefficients."""
    SV = np.linalg.inv(CV)
    comp = ('11', '22', '33', '23', '13', '12')
    db = {'Texture': {'name': name, 'texture_index': float(tx_index), 'gsh_coeff_reconstructed_random': [float(v) for v in gsh]}}
    for i, (sy, a) in enumerate(zip(sig_y, normal)):
        S = np.array([0. * sy, 0.5 * sy, sy] + [sy] * 5)
        peeq = np.array([0., 0., 0., 1e-3, 2e-3, 3e-3, 4e-3, 5e-3])
        an = a / np.sqrt(2. / 3. * (np.sum(a[:3] ** 2) + 0.5 * np.sum(a[3:] ** 2)))
        Ep = peeq[:, None] * an[None, :]
        S, Ep = np.round(S, 4), np.round(Ep, 8)
        E = np.round(S @ SV.T + Ep, 8)
        res = {}
        for c, k in zip(comp, range(6)):
            res['S' + c], res['E' + c], res['Ep' + c] = S[:, k].tolist(), E[:, k].tolist(), Ep[:, k].tolist()
        db['Us_A0B0C0D0E0F0_TX%03d_NNNNN_Tx_NN' % i] = {'Results': res}
    return json.dumps(db, separators=(',', ':')).encode()


def widen(p, tex, tdim):
    """tables and textures of more texture columns than the fixture trained: the leading texture columns repeated (with
    their mean and scale) up to tdim -- a table that exercises another padded width"""
    extra = tdim - p['tdim']
    col = 6 + np.arange(extra) % p['tdim']
    q = dict(p, sv=np.ascontiguousarray(np.concatenate((p['sv'], p['sv'][:, col]), axis=1)),
             mean=np.concatenate((p['mean'], p['mean'][col])), scale=np.concatenate((p['scale'], p['scale'][col])), tdim=tdim)
    return q, np.ascontiguousarray(np.concatenate((tex, tex[:, col - 6]), axis=1))


def crossing_intercept(p, tex0):
    """an intercept with which a CUT table (vectors of the inner class only: negative coefficients) still changes sign
    along rays from the origin: half of what the vectors sum to at zero stress and the texture tex0"""
    q = dict(p, intercept=0.)
    f, _, _ = restate(q, np.zeros((1, 6)), tex0, np.ones(1))
    return 0.5 * abs(float(f[0]))


def march_replay(p, su, tex, x0):
    """status per ray (0 bracket found, 1 none) of the march of yield_scale replayed with the restatement
    (ray_cases.march_replay), and the smallest |f_L| met on the march (how clear of rounding the decisions were)"""
    clear = np.full(len(su), np.inf)

    def seen(act, f, A):
        clear[act] = np.minimum(clear[act], np.asarray(np.abs(f), dtype=float))
    return _march_replay(lambda act, x: restate(p, su[act], tex, x)[::2], x0, seen), clear
