"""Query by committee for SVC yield functions (the reference's ``examples/Active_Learning/qbc_svc.py``): a committee of
trained ``Material``s is evaluated on shared unit stresses in ONE device pass (``plfx_committee_yf``) -- the
yield function of every member, their mean and variance per point, and the point on which the members disagree most.

``Committee`` holds the members, ``train_committee`` trains them on random subsets of the yield stresses as the example does,
``active_learning`` runs the example's loop with the maximiser taken over a candidate set.
"""
import hashlib
import warnings

import numpy as np

from . import _lib
from .material import Material, _ctx

MAX_MEMBERS = 16    # MAXMAT of the library: the committee is loaded as materials 0 .. M-1 of the shared point context

_standin = None


def _standin_elasticity():
    """(CV, E, nu) for the record of a member without elastic constants (``train_SVC(sdata=...)`` sets none): the yield
    function does not depend on them, the record needs a regular matrix"""
    global _standin
    if _standin is None:
        m = Material(name='committee-standin')
        m.elasticity(E=2.e5, nu=0.3)
        _standin = (np.array(m.CV, dtype=float), float(m.E), float(m.nu))
    return _standin


class Committee(object):
    """A committee of 1-16 trained SVC yield functions (6 stress features on Voigt stresses, ``dev_only`` or not), evaluated
    together on the device.  ``scale``: the stress scale per member -- member m sees ``su * scale[m]`` -- a float, an (M,)
    array, or None for the example's ``0.5 * m.sy``.

    ValueError for an untrained member, a member with sdim = 3, a work-hardening member, a member with ``ML_grad`` set, and
    for 0 or more than 16 members; NotImplementedError for a texture material."""

    def __init__(self, members, scale=None):
        members = list(members)
        if not 1 <= len(members) <= MAX_MEMBERS:
            raise ValueError('Committee: %d members, 1 to %d are supported' % (len(members), MAX_MEMBERS))
        for k, m in enumerate(members):
            if isinstance(m, Material) and getattr(m, 'txdat', False):
                m._tex_refuse('Committee')
            if isinstance(m, Material):
                m._bound_refuse('Committee')
            if not isinstance(m, Material) or not m.ML_yf or m.svc is None:
                raise ValueError('Committee: member %d has no trained SVC yield function' % k)
            if m.sdim != 6:
                raise ValueError('Committee: member %d has sdim = %s; only yield functions on Voigt stresses (sdim = 6) '
                                 'are supported' % (k, m.sdim))
            if getattr(m, 'whdat', False):
                raise ValueError('Committee: member %d has work-hardening features, which are not supported' % k)
            if getattr(m, 'ML_grad', False):
                raise ValueError('Committee: member %d has ML_grad set; committees evaluate the SVC yield function only' % k)
        self.members = members
        if scale is None:
            self._scale = None
        else:
            sc = np.asarray(scale, dtype=float)
            sc = np.full(len(members), float(sc)) if sc.ndim == 0 else sc.reshape(-1).copy()
            if len(sc) != len(members):
                raise ValueError('Committee: scale must be a float or one value per member')
            if not np.all(np.isfinite(sc) & (sc > 0.)):
                raise ValueError('Committee: scale must be finite and positive')
            self._scale = sc

    def __len__(self):
        return len(self.members)

    @property
    def scale(self):
        """(M,) stress scale per member; without an explicit one ``0.5 * m.sy``, read from the members at every call"""
        if self._scale is not None:
            return self._scale
        return np.array([0.5 * m.sy for m in self.members])

    @staticmethod
    def _record(m):
        if m.CV is not None:
            return m._record(np.asarray(m.CV, dtype=float))
        cv, E, nu = _standin_elasticity()
        svc = dict(sv=m.svc['sv'], dual=m.svc['dual'], intercept=m.svc['intercept'], gamma=m.gam_yf,
                   scale_seq=m.scale_seq, dev_only=m.dev_only, scale_wh=None)
        return _lib.pack_material(_lib.SVC6, cv, E=E, nu=nu, sy=m.sy, khard=m.khard, hill=m.hill, drucker=m.drucker, svc=svc)

    def _load(self):
        """Make the members materials 0 .. M-1 of the shared point context.  The context's key becomes a digest over the
        members' content keys: a member edited in place is re-sent here, and a later ``Material._load`` re-sends its own
        record."""
        ctx = _ctx()
        recs = [self._record(m) for m in self.members]
        h = hashlib.blake2b(b'committee', digest_size=16)
        for m, rec in zip(self.members, recs):
            h.update(m._content_key(rec=rec))
        key = h.digest()
        if getattr(ctx, '_point_key', None) != key:
            ctx._point_key = None
            ctx.set_materials(recs)
            ctx._point_key = key
        return ctx

    @staticmethod
    def _su(su):
        s = np.asarray(su, dtype=float)
        if s.ndim == 1:
            s = s[None, :]
        if s.ndim != 2 or s.shape[1] != 6:
            raise ValueError('Committee: unit stresses of shape (6,) or (N,6) expected')
        return np.ascontiguousarray(s)

    def _run(self, su, **want):
        ctx = self._load()
        return ctx.committee_yf(np.arange(len(self.members)), self.scale, self._su(su), **want)

    def calc_yf(self, su):
        """(M, N): ``members[m].calc_yf(su * scale[m])`` for all members, from one device pass"""
        return self._run(su)['yf']

    def variance(self, su, return_mean=False):
        """(N,) variance of the members' yield functions per unit stress (``np.var``, ddof = 0: the example's measure of
        disagreement); with ``return_mean`` the tuple (variance, mean)"""
        r = self._run(su, want_yf=False, want_var=True, want_mean=bool(return_mean))
        return (r['var'], r['mean']) if return_mean else r['var']

    def query(self, su):
        """(index, su[index], variance) of the unit stress on which the members disagree most; points with a NaN variance
        (non-finite stresses) are skipped, equal variances resolve to the smaller index.  (-1, None, nan) with a warning if
        no point has a finite variance."""
        s = self._su(su)
        i, v = self._run(s, want_yf=False, want_best=True)['best']
        if i < 0:
            warnings.warn('Committee.query: no candidate has a finite variance')
            return -1, None, float('nan')
        return i, s[i].copy(), v


def train_committee(sig, nmembers=5, subset=0.8, rng=None, **train_SVC_kwargs):
    """Train ``nmembers`` SVC yield functions on random subsets of the yield stresses ``sig`` (N,6), drawn as the example
    does -- ``rng.choice(len(sig), int(len(sig) * subset), replace=False)`` per member -- each by the existing
    ``Material.train_SVC(sdata=sig[idx], **train_SVC_kwargs)``.  Returns the ``Committee``; its ``subsets`` lists the index
    arrays.  ``train_SVC(sdata=...)`` defines no elastic constants; with ``mat_ref`` among the keywords the members take
    its elastic matrix."""
    sig = np.asarray(sig, dtype=float)
    rng = np.random.default_rng() if rng is None else rng
    mat_ref = train_SVC_kwargs.get('mat_ref')
    train_SVC_kwargs.setdefault('verbose', 0)
    members, subsets = [], []
    for j in range(int(nmembers)):
        idx = rng.choice(len(sig), int(len(sig) * subset), replace=False)
        m = Material(name='ML-Hill_{}'.format(j))
        m.train_SVC(sdata=sig[idx, :], **train_SVC_kwargs)
        if mat_ref is not None and m.CV is None:
            m.elasticity(CV=mat_ref.CV)
        members.append(m)
        subsets.append(idx)
    com = Committee(members)
    com.subsets = subsets
    return com


def active_learning(mat_ref, sunit0, n_add, candidates, nmembers=5, subset=0.8, rng=None, **train_SVC_kwargs):
    """The loop of the reference's query-by-committee example: starting from the yield stresses of ``mat_ref`` along the unit
    stresses ``sunit0``, ``n_add`` times train a committee on the current yield stresses, take the candidate (rows of
    ``candidates``, (K,6) unit stresses) on which its members disagree most, and add the yield stress of ``mat_ref`` along
    it (``mat_ref.yield_stress``).  The maximiser is ``Committee.query`` over the candidate set, where the example runs a
    differential evolution.  Returns (material trained on all yield stresses, (n_add,6) unit stresses added, (n_add,)
    variance at each of them)."""
    rng = np.random.default_rng() if rng is None else rng
    sunit = np.array(sunit0, dtype=float)
    cand = np.ascontiguousarray(candidates, dtype=float)
    sig = np.asarray(mat_ref.yield_stress(sunit), dtype=float)
    added, var = [], []
    kw = dict(train_SVC_kwargs, mat_ref=mat_ref)
    for _ in range(int(n_add)):
        com = train_committee(sig, nmembers=nmembers, subset=subset, rng=rng, **kw)
        i, su, v = com.query(cand)
        if i < 0:
            raise RuntimeError('active_learning: the committee has no finite variance on any candidate')
        sig = np.vstack([sig, np.asarray(mat_ref.yield_stress(su), dtype=float)[None, :]])
        added.append(su)
        var.append(v)
    mat = Material(name='ML-Hill')
    kw.setdefault('verbose', 0)
    mat.train_SVC(sdata=sig, **kw)
    if mat.CV is None:
        mat.elasticity(CV=mat_ref.CV)
    return mat, np.array(added).reshape(-1, 6), np.array(var)
