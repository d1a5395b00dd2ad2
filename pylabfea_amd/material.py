"""``Material`` façade: the reference's constitutive API for the hot path, evaluated by libplfx on
the MI355X.

Mirrors pylabfea.Material (reference /root/reference/src/pylabfea/material.py) for the methods on
the path named by BASELINE.json: ``elasticity`` (:2401), ``plasticity`` (:2466), ``response`` (:207),
``calc_yf`` (:348), ``ML_full_yf`` (:414), ``calc_seq`` (:576), ``calc_fgrad`` (:704), ``get_sflow``
(:974), ``epl_dot`` (:1009), ``C_tan`` (:1057) and the test harness ``calc_properties`` (:3062).
Same names, argument meaning and error behaviour; arguments are never mutated.

Out of scope here: plotting.  What the yield-locus plots compute comes back as arrays (``yield_scale``,
``polar_yield_locus``, ``polar_field``, ``yield_slices``; ``texture_loci`` for a texture material, §28).
Texture materials (``from_data`` on data sets with ``tx_data``) are trained and evaluated as yield functions --
``train_SVC``, ``calc_yf``, ``find_yloc``, ``yield_scale``, ``texture_loci`` -- and, like in the reference, nothing past that
unless the caller passes ``tex=``: ``calc_fgrad``, ``ML_full_yf``, ``response``, ``response_batch``, ``epl_dot`` and ``C_tan``
then run at that texture (an extension).  ``at_texture(tex)`` binds a trained texture material to one texture:
the bound material is what ``Model.assign`` takes, one texture per section; ``at_textures(tex)`` binds it to a
field of textures, one per element (``Model.set_texture_ids``) or per point (``tex_id=``), as one material.
A trained SVC enters through
:meth:`Material.train_SVC` (trained on the GPU), :meth:`Material.set_svc` or :meth:`Material.from_sklearn`.
sdim=3 flow rules use the reference's axis-tracking principal stresses (exact for plane states);
Tresca and Barlat Yld2004-18p are equivalent stresses only (the reference has no normal for them).
ML materials: 6 stress features (sdim=6) or the 2 features (seq, polar angle) of ``setup_yf_SVM_3D`` (sdim=3).
"""
import hashlib
import os
import warnings

import numpy as np

from . import _lib
from .basic import eps_eq, sig_cyl2princ, sig_dev, sig_eq_j2, sig_polar_ang, sig_princ, yf_tolerance

_point_ctx = {}        # shared contexts for point evaluations, one per GPU (each remembers the record it holds)


def point_device():
    """GPU of the point-evaluation context: PLFX_DEVICE (an explicit choice: must name a visible GPU, like
    ``Model(device=...)``), else LOCAL_RANK (one process per GPU under torchrun; taken modulo the number of visible GPUs so
    that several ranks sharing one GPU -- host transport, tests -- all find a device), else 0."""
    n = _lib.device_count()
    v = os.environ.get('PLFX_DEVICE')
    if v is not None and v.strip().isdigit():
        if n > 0 and int(v) >= n:
            raise ValueError('PLFX_DEVICE=%s, but only %d GPU(s) are visible' % (v.strip(), n))
        return int(v)
    v = os.environ.get('LOCAL_RANK')
    if v is not None and v.strip().isdigit():
        return int(v) % n if n > 0 else 0
    return 0


try:    # the support-vector tables (~90 KB) are digested on every point call (in-place edits must be seen): xxh3 does it in
    import xxhash as _xxhash   # ~8 us where blake2b needs ~100 us; blake2b when the module is absent
except ImportError:  # pragma: no cover
    _xxhash = None


def _table_digest(a):
    """16-byte digest of the CONTENT of a contiguous array"""
    if _xxhash is not None:
        return _xxhash.xxh3_128_digest(a.data)
    return hashlib.blake2b(a.data, digest_size=16).digest()


def _ctx():
    dev = point_device()
    if dev not in _point_ctx:
        _point_ctx[dev] = _lib.Context(dev)
    return _point_ctx[dev]


def close_point_contexts():
    """release the shared point-evaluation contexts (HBM of the support-vector tables, streams)"""
    for c in _point_ctx.values():
        c.close()
    _point_ctx.clear()


class Material(object):
    """Material card: elastic constants, plastic parameters, optional trained SVC yield function.

    Attributes follow the reference (``sy, khard, hill, drucker, E, nu, C11, C12, C44, CV, sdim,
    ML_yf, dev_only, scale_seq, gam_yf, msg, prop, propJ2, sigeps`` ...).
    """

    def __init__(self, name='Material', num=1):
        self.name = name
        self.num = num
        self.E = self.nu = self.CV = self.C11 = self.C12 = self.C44 = None
        self.sy = None          # elasticity only unless sy is set (material.py:159)
        self.sy0 = None
        self.khard = None
        self.drucker = None
        self.lhs = None
        self.hill = None
        self.hill_3p = False
        self.hill_6p = False
        self.tresca = False
        self.barlat = False
        self.sdim = None
        self.ML_yf = False
        self.ML_grad = False
        self.dev_only = False
        self.scale_seq = None
        self.gam_yf = None
        self.C_yf = None
        self.Ndof = 2
        self.svc = None         # dict(sv, dual, intercept) of the trained SVC
        self.msg = {'yield_fct': None, 'gradient': None, 'nsteps': 0, 'equiv': None}
        lcs = ('stx', 'sty', 'et2', 'ect')
        self.prop = {k: {'ys': None, 'seq': None, 'eeq': None, 'peeq': None, 'style': None, 'name': None}
                     for k in lcs}
        self.propJ2 = {k: {'ys': None, 'seq': None, 'eeq': None, 'peeq': None} for k in lcs}
        self.sigeps = {k: {'sig': None, 'eps': None, 'epl': None} for k in lcs}
        self._version = 0
        self._bound = None      # at_texture: dict(parent, tex, scale) of a material bound to one texture

    # ------------------------------------------------------------------ definition
    def elasticity(self, C11=None, C12=None, C44=None, CV=None, E=None, nu=None):
        """Define elastic properties (material.py:2401-2464): one of (E, nu), (C11, C12, C44) or the full 6 x 6 matrix;
        the other descriptions are derived from the one given.  Same exceptions and messages as the reference."""
        clash = 'Error: Inconsistent definition of material parameters: '
        cubic = (C11, C12, C44)
        if E is not None:      # isotropic
            if nu is None:
                raise ValueError(clash + 'Only E provided')
            if any(c is not None for c in cubic):
                raise ValueError(clash + 'E provided together with C_ij')
            hh = E / ((1. + nu) * (1. - 2. * nu))
            cubic = ((1. - nu) * hh, nu * hh, (0.5 - nu) * hh)
        elif C11 is not None:  # cubic
            if nu is not None:
                raise ValueError(clash + 'nu provided together with C_ij')
            if None in (C12, C44):
                raise ValueError(clash + 'C_12 or C_44 values missing')
        elif CV is not None:   # general: Poisson ratio and modulus of the [100] direction
            self.CV = np.array(CV, dtype=float)
            cubic = (self.CV[0, 0], self.CV[0, 1], self.CV[3, 3])
        else:
            raise ValueError('elasticity: Inconsistent definition of material parameters')
        self.C11, self.C12, self.C44 = cubic
        if E is None:
            nu = self.C12 / (self.C11 + self.C12)
            E = 2 * self.C44 * (1 + nu)
        self.E, self.nu = E, nu
        if CV is None:
            M = np.full((6, 6), 0.)
            M[:3, :3] = self.C12
            for k in range(3):
                M[k, k], M[k + 3, k + 3] = self.C11, self.C44
            self.CV = M
        self._version += 1

    def plasticity(self, sy=None, sdim=6, drucker=0., khard=0., tresca=False, barlat=None,
                   barlat_exp=None, hill=None, hill_3p=None, hill_6p=None, rv=None, lhs=None):
        """Define plastic parameters (material.py:2466-2594).  Same exceptions, warnings and messages as the reference;
        the Hill coefficients end up as 6 numbers for sdim = 6 and 3 for sdim = 3, with `hill_6p` / `hill_3p` telling
        which equivalent-stress form applies (both False: J2)."""
        if sy < 0.:
            raise ValueError('Initial yield strength cannot be negative.')
        if khard < 0.:
            warnings.warn('Strain softening not supported. khard is set to 0.')
        if lhs is not None:
            # the reference stores lhs but calc_seq evaluates `if self.lhs:` on the array
            # (material.py:642), which raises for any 3-vector: the option cannot run there either
            raise NotImplementedError('lhs (Liu-Huang-Stout asymmetry) is not supported')
        if sdim not in (3, 6):
            raise ValueError('{} in plasticity: sdim must be either 3 or 6'.format(self.name))
        if barlat is not None and len(barlat) != 18:
            raise ValueError('plasticity: barlat must hold the 18 Yld2004-18p coefficients')
        if self.sdim not in (None, sdim):
            print('plasticity: Parameter sdim is changed. New value:', sdim)
        self.sdim, self.sy0, self.sy = sdim, sy, sy
        self.khard, self.drucker, self.lhs = max(khard, 0.), drucker, None
        if hill is not None:
            if rv is not None:
                warnings.warn('plasticity: Both, hill and rv, have been provided. Using Hill parameters.')
            hill = list(hill)
        elif rv is None:
            hill = [1.] * sdim
        else:  # yield-stress ratios -> Hill coefficients
            if len(rv) != sdim:
                raise ValueError(f'plasticity: wrong dimension of yield stress ratios, must be {sdim}')
            q = (1. / np.array(rv, dtype=float)) ** 2
            hill = list(q[:3] + np.roll(q[:3], -1) - np.roll(q[:3], -2)) + list(q[3:])
        given = len(hill)
        if hill_6p is None and hill_3p is None:  # decided by the number of coefficients; three ones are J2, not Hill
            six = given == 6
            three = not six and not (hill[0] == 1. and hill[1] == 1. and hill[2] == 1.)
        else:
            six, three = hill_6p, hill_3p
        if six and given != 6:
            raise ValueError('plasticity: When hill_6p is set True, 6 Hill parameters must be provided')
        if three and given != 3:
            raise ValueError('plasticity: When hill_3p is set True, only 3 Hill parameters can be provided')
        if six and sdim == 3:
            warnings.warn('plasticity: 6 Hill parameters are provided, but sdim=3; ignoring shear parameters')
            six, three = False, True
            del hill[3:]
        if three and sdim == 6:
            print('Material', self.name)
            warnings.warn('plasticity: 3 Hill parameters are provided, but sdim=6; shear parameters set to 1')
            six, three = True, False
        if sdim == 6 and len(hill) == 3:
            hill += [1., 1., 1.]
        self.hill_6p, self.hill_3p = bool(six), bool(three)
        self.hill = np.array(hill, dtype=float)
        self.tresca = bool(tresca)
        self.barlat = barlat is not None
        if self.barlat:
            self.barlat_par = np.array(barlat, dtype=float)
            self.barlat_exp = barlat_exp
            b = self.barlat_par  # the two linear maps of the stress deviator (material.py:2578-2591)
            for name, c in (('Bar_m1', b[0:9]), ('Bar_m2', b[9:18])):
                m = np.zeros((6, 6))
                m[0, 1], m[0, 2], m[1, 0], m[1, 2], m[2, 0], m[2, 1] = -c[0], -c[1], -c[2], -c[3], -c[4], -c[5]
                m[3, 3], m[4, 4], m[5, 5] = c[6], c[7], c[8]
                setattr(self, name, m)
        self._version += 1

    def set_svc(self, support_vectors, dual_coef, intercept, gamma, scale_seq, dev_only=False, C=None, scale_wh=None):
        """Install a trained RBF-SVC yield function (what ``train_SVC`` leaves in ``svm_yf``,
        ``gam_yf`` and ``scale_seq``; material.py:398-405, 797-807).  ``dual_coef``/``intercept`` are
        scikit-learn's public ``dual_coef_[0]`` / ``intercept_[0]``."""
        if self.sy is None:
            raise ValueError('set_svc: call elasticity() and plasticity(sy=..., sdim=6) first')
        nfeat = 6 if self.sdim == 6 else 2   # sdim=3: (seq_J2/scale - 1, polar angle/pi), material.py:2331-2333
        sv = np.ascontiguousarray(support_vectors, dtype=float)
        # work-hardening-aware SVC (train_SVC on Data(wh_data=True), material.py:2342-2346): 6 stress features, the plastic
        # strain / scale_wh (6), accumulated strain, max. stress / scale_seq, flag  ->  Ndof = 15, ind_wh = 6
        self.whdat = bool(self.sdim == 6 and sv.ndim == 2 and sv.shape[1] == 15)
        if self.whdat:
            if scale_wh is None or not scale_wh > 0.:
                raise ValueError('set_svc: 15-feature support vectors (work-hardening data) need scale_wh > 0')
            nfeat = 15
            self.ind_wh = 6
            self.scale_wh = float(scale_wh)
        if sv.ndim != 2 or sv.shape[1] != nfeat:
            raise ValueError('set_svc: support vectors must have shape (nsv, %d) for sdim=%d' % (nfeat, self.sdim))
        dual = np.ascontiguousarray(dual_coef, dtype=float).reshape(-1)
        if len(dual) != len(sv):
            raise ValueError('set_svc: dual_coef and support_vectors differ in length')
        self.svc = dict(sv=sv, dual=dual, intercept=float(intercept))
        self.gam_yf = float(gamma)
        self.C_yf = C
        self.scale_seq = float(scale_seq)
        self.dev_only = bool(dev_only)
        self.ML_yf = True
        self.Ndof = nfeat
        if self.khard and not self.whdat:
            # calc_fgrad of an ML material resets self.khard to 0 on every call (material.py:812-814)
            warnings.warn('set_svc: khard of an ML material is reset to 0 by the reference flow rule')
            self.khard = 0.
        self._version += 1

    @classmethod
    def from_sklearn(cls, svm, scale_seq, E, nu, sy, name='ML-material', dev_only=False):
        """Build an ML material from a fitted ``sklearn.svm.SVC`` (RBF kernel, 6 stress features)."""
        m = cls(name=name)
        m.elasticity(E=E, nu=nu)
        m.plasticity(sy=sy, sdim=6)
        gamma = svm._gamma if hasattr(svm, '_gamma') else svm.gamma
        m.set_svc(svm.support_vectors_, svm.dual_coef_[0, :], svm.intercept_[0], gamma, scale_seq,
                  dev_only=dev_only, C=getattr(svm, 'C', None))
        return m

    # ------------------------------------------------------------------ SVC parameter files (reference wire format)
    def export_MLparam(self, sname, source=None, file=None, path='../../models/', descr=None, param=None):
        """Write the trained SVC in the reference's Abaqus-UMAT layout (material.py:2130-2271): ``file-svm.csv``
        with 8 numbers per line -- header slots 0..28 (nsv, Ndof, C11, C12, C44, intercept, gamma, epc, scale_seq,
        scale_wh, C22, C33, C13, C23, C55, C66, dev_only flag, Nset, scale_text), dual coefficients from slot 29,
        then the support vectors row by row -- and ``file-svm_meta.json``."""
        import datetime, getpass, json, platform
        self._tex_refuse('export_MLparam')
        self._bound_refuse('export_MLparam')
        if not self.ML_yf:
            raise AttributeError('export_MLparam: No ML flow rule defined.')
        if descr is not None and param is not None and len(descr) != len(param):
            raise ValueError('Lists for descr and param must have the same lengths.')
        file = (path if path.endswith('/') else path + '/') + ('abq_' + self.name if file is None else file)
        dc, sv = self.svc['dual'], self.svc['sv']
        nsv, ndof = sv.shape
        nlin = int((nsv * (ndof + 1) + 30) / 8) + 1
        ndata = nlin * 8
        head = np.zeros(29)
        head[:10] = (nsv, ndof, self.C11, self.C12, self.C44, self.svc['intercept'], self.gam_yf,
                     float(getattr(self, 'epc', 0.) or 0.), self.scale_seq,
                     self.scale_wh if getattr(self, 'whdat', False) else 1.)
        head[10:16] = -1 if self.CV is None else [self.CV[i, j] for i, j in ((1, 1), (2, 2), (0, 2), (1, 2), (4, 4), (5, 5))]
        head[16:19] = (-1. if self.dev_only else 0., 1, 1.)   # dev_only flag, Nset, scale_text
        body = np.concatenate([head, dc, sv.ravel()])
        props = np.concatenate([body, np.zeros(ndata - len(body))])
        np.savetxt(file + '-svm.csv', props.reshape((nlin, 8)), delimiter=', ', newline='\n')
        descr = ([] if descr is None else list(descr)) + ['Ndata', 'gamma', 'C']
        param = ([] if param is None else list(param)) + [ndata, self.gam_yf, self.C_yf]
        sys_info = platform.uname()
        from . import __version__ as vers
        meta = {
            'Info': {'Owner': getpass.getuser(), 'Institution': None, 'Date': str(datetime.date.today()),
                     'Description': 'SVC-parameters for plasticity model', 'Method': 'Support Vector Classification',
                     'System': {'sysname': sys_info[0], 'nodename': sys_info[1], 'release': sys_info[2],
                                'version': sys_info[3], 'machine': sys_info[4]}},
            'Model': {'Creator': 'pylabfea_amd', 'Version': vers, 'Repository': None, 'Input': source, 'Script': sname,
                      'Names': descr, 'Parameters': param},
            'Data': {'Class': 'SVC_parameters', 'Type': 'CSV', 'File': file + '-svm.csv', 'Separator': ',',
                     'Header': None, 'Format': (nlin, 8),
                     'Names': ['nsv', 'nsd', 'C11', 'C12', 'C44', 'rho', 'gamma', 'epc', 'scale_seq', 'scale_wh',
                               'C22', 'C33', 'C13', 'C23', 'C55', 'C66', 'Nset', 'scale_text[0:Nset]',
                               'dual_coef[0:nsv]', 'sup_vec[0:nsv,0:nsd]'],
                     'Units': {'Stress': 'MPa', 'Strain': 'None', 'Disp': 'mm', 'Force': 'N'}}}
        with open(file + '-svm_meta.json', 'w') as fp:
            json.dump(meta, fp, indent=2)

    def from_MLparam(self, name, path='../../models/'):
        """Define the material from a parameter file written by ``export_MLparam`` (of stock pyLabFEA or of this
        package): elastic constants, yield strength (= the stress scaling factor, ``scale_seq = sy`` at training,
        material.py:1161) and the SVC yield function.  The reference declares this method but raises
        ``ModuleNotFoundError`` (material.py:2688-2703); the layout read here is the one its ``export_MLparam``
        writes and its Abaqus UMAT reads (examples/UMAT/ml_umat.f:129-151), including the rule
        ``dev_only = props[16] < 0``, and the older layout of the files shipped under examples/UMAT/models (see below).
        Files with work-hardening or texture features (Ndof > 6) are refused."""
        import json
        if path and path[-1] != '/':
            path += '/'
        trunk = path + name
        for suffix in ('-svm.csv', '.csv', ''):
            if trunk.endswith(suffix) and suffix:
                trunk = trunk[:-len(suffix)]
                break
        props = np.loadtxt(trunk + '-svm.csv', delimiter=',').ravel()
        nsv, ndof = int(round(props[0])), int(round(props[1]))
        if nsv < 1 or 29 + nsv * (ndof + 1) > len(props):
            raise ValueError('from_MLparam: inconsistent header (nsv={}, Ndof={}, {} numbers)'.format(nsv, ndof, len(props)))
        if ndof not in (2, 6, 15):
            raise NotImplementedError('from_MLparam: {} features (texture descriptors) are not supported; only the 6 '
                                      'stress features, the 2 features of sdim=3, or 15 = 6 stress + 9 work-hardening '
                                      'features'.format(ndof))
        C11, C12, C44 = props[2], props[3], props[4]
        if np.all(props[10:16] == -1.):
            self.elasticity(C11=C11, C12=C12, C44=C44)
        else:
            CV = np.zeros((6, 6))
            CV[0, 0], CV[1, 1], CV[2, 2] = C11, props[10], props[11]
            CV[0, 1] = CV[1, 0] = C12
            CV[0, 2] = CV[2, 0] = props[12]
            CV[1, 2] = CV[2, 1] = props[13]
            CV[3, 3], CV[4, 4], CV[5, 5] = C44, props[14], props[15]
            self.elasticity(CV=CV)
        scale_seq = float(props[8])
        self.plasticity(sy=scale_seq, sdim=6 if ndof in (6, 15) else 3)
        C = None
        try:
            with open(trunk + '-svm_meta.json') as fp:
                meta = json.load(fp)
            names, par = meta['Model']['Names'], meta['Model']['Parameters']
            if 'C' in names:
                C = par[names.index('C')]
        except (IOError, OSError, KeyError, ValueError):
            pass
        dual = props[29:29 + nsv]
        sv = props[29 + nsv:29 + nsv * (ndof + 1)].reshape(nsv, ndof)
        # Layouts.  Current (export_MLparam of v4.4, material.py:2212-2214): slot 16 = -1 / 0 deviatoric-feature flag, slot 17 =
        # Nset, 18.. = scale_text.  Files shipped with the reference under examples/UMAT/models (written by pyLabFEA 4.3,
        # "v4.0 layout"): slot 16 = Nset (>= 1), 17.. = scale_text, no flag -- those versions trained the 6-feature SVC on
        # DEVIATORIC stresses (every support vector is trace-free; with full-stress features the J2 file would yield under
        # hydrostatic load), so the flag is recovered from the support vectors.  Dual coefficients start at slot 29 in both.
        self.mlparam_layout = 'v4.0' if props[16] >= 1. else 'v4.4'
        if self.mlparam_layout == 'v4.0':
            dev_only = bool(ndof == 6 and np.max(np.abs(sv[:, 0:3].sum(axis=1))) < 1e-9 * max(np.max(np.abs(sv)), 1e-300))
        else:
            dev_only = bool(props[16] < 0.)
        self.set_svc(sv, dual, props[5], props[6], scale_seq, dev_only=dev_only, C=C,
                     scale_wh=float(props[9]) if ndof == 15 else None)
        if ndof == 15:
            self.epc = float(props[7])
        return self

    # ------------------------------------------------------------------ records for libplfx
    def _record(self, CV, ana=False):
        """plfx_material record of this material with the element matrix CV."""
        if self.sy is None:
            return _lib.pack_material(_lib.ELASTIC, CV, E=self.E, nu=self.nu)
        if self.ML_yf and not ana and getattr(self, '_bound', None) is not None:
            svc = dict(sv=self.svc['sv'], dual=self.svc['dual'], intercept=self.svc['intercept'], gamma=self.gam_yf,
                       scale_seq=self.scale_seq, dev_only=self.dev_only, scale_cols=self._bound['scale'],
                       coef=self._bound.get('coef'))
            return _lib.pack_material(_lib.SVC6_COLS, CV, E=self.E, nu=self.nu, sy=self.sy, khard=self.khard,
                                      hill=self.hill, drucker=self.drucker, svc=svc)
        if self.ML_yf and not ana:
            self._tex_refuse('Model.assign')
            svc = dict(sv=self.svc['sv'], dual=self.svc['dual'], intercept=self.svc['intercept'],
                       gamma=self.gam_yf, scale_seq=self.scale_seq, dev_only=self.dev_only,
                       scale_wh=getattr(self, 'scale_wh', None))
            kind = _lib.SVC_WH if getattr(self, 'whdat', False) else (_lib.SVC6 if self.sdim == 6 else _lib.SVC3)
            return _lib.pack_material(kind, CV, E=self.E, nu=self.nu, sy=self.sy, khard=self.khard,
                                      hill=self.hill, drucker=self.drucker, svc=svc)
        kind = _lib.HILL6 if self.sdim == 6 else _lib.PRINC3
        if self.tresca:
            kind = _lib.TRESCA
        elif self.barlat:
            kind = _lib.BARLAT
        return _lib.pack_material(kind, CV, E=self.E, nu=self.nu, sy=self.sy, khard=self.khard,
                                  hill=self.hill, drucker=self.drucker,
                                  barlat=self.barlat_par if self.barlat else None,
                                  barlat_exp=self.barlat_exp if self.barlat else 0.,
                                  barlat_normal=bool(self.barlat and getattr(self, 'barlat_normal', False)))

    def enable_barlat_normal(self, on=True):
        """EXTENSION (not in the reference, which has no flow rule for Barlat materials: calc_fgrad raises,
        material.py:822-825): use the analytic normal of Yld2004-18p -- d seq / d sigma through the eigen-decompositions
        of the two linearly transformed deviators -- so that ``calc_fgrad``, ``response``, ``calc_properties`` and
        ``Model.solve`` work for a Barlat material with an associated flow rule, like they do for Hill materials."""
        if not self.barlat:
            raise AttributeError('enable_barlat_normal: material has no Barlat parameters')
        self.barlat_normal = bool(on)
        self._version += 1
        return self

    # ------------------------------------------------------------------ texture materials
    # what the reference does where this engine refuses a texture material
    _TEX_REFUSALS = {
        'calc_fgrad': 'the reference raises AttributeError there (self.self.scale_seq, material.py:811); calc_fgrad(sig, tex=) '
                      'runs the gradient of this engine (DESIGN.md §32)',
        'ML_full_yf': "the reference raises ValueError there: its calls of calc_yf pass no texture (material.py:475-491); "
                      "ML_full_yf(sig, tex=) runs the search at a texture (DESIGN.md §32)",
        'response': 'the reference raises ValueError in its first calc_yf call, which passes no texture (material.py:252); '
                    'response(..., tex=) runs the update at a texture (DESIGN.md §32)',
        'response_batch': 'the reference has no response for a texture material: its calc_yf calls pass no texture '
                          '(material.py:252); response_batch(..., tex=) runs the update at a texture (DESIGN.md §32)',
        'calc_hessian': 'the reference rescales the Hessian of the scaler-standardised features by 1 / scale_seq**2, and '
                        'scale_seq is not a feature scale of a texture material (material.py:952-960)',
        'calc_properties': 'the reference fails in Model.solve, whose response calls pass no texture (model.py:1343); '
                           'at_texture(tex) binds the material to one texture, and the bound material runs (DESIGN.md §34)',
        'setup_fgrad_SVM': 'the reference needs work-hardening data, which a texture material cannot carry here',
        'export_MLparam': "the reference's file has no slots for the scaler's mean and scale (material.py:2130-2271)",
        'polar_yield_locus': 'the reference\'s polar_plot_yl calls find_yloc without a texture and raises ValueError '
                             '(material.py:3292); texture_loci traces the loci',
        'yield_slices': "the reference's plot_yield_locus calls calc_yf without a texture and raises ValueError (material.py:3017)",
        'Committee': 'the reference example forms committees of texture-free yield functions only',
        'load_path': 'the reference has no response for a texture material (material.py:252); at_texture(tex) binds the '
                     'material to one texture and at_textures(tex) to a field of them, and the bound material follows a '
                     'path (DESIGN.md §40)',
        'Model.assign': 'the reference fails in Model.solve, whose response calls pass no texture (model.py:1343); '
                        'at_texture(tex) binds the material to one texture, and a model takes the bound material (DESIGN.md §34)',
    }

    def _is_tex(self):
        """a texture material: txdat set by from_data, msparam still the one it installed"""
        ms = getattr(self, 'msparam', None)
        return bool(getattr(self, 'txdat', False)) and ms is not None and getattr(self, '_tex_from_data', None) is ms

    def _tex_refuse(self, what):
        if getattr(self, 'txdat', False):
            raise NotImplementedError('%s: not offered for a texture material (txdat); %s'
                                      % (what, self._TEX_REFUSALS.get(what, 'the reference does not support it either')))

    def _tex_rows(self, tex, n, name):
        """tex as calc_yf takes it -- (tdim,) or (N, tdim) -- as a C-contiguous (1, tdim) or (n, tdim) array"""
        t = np.asarray(tex, dtype=float)
        if t.ndim == 1:
            t = t[None, :]
        if t.ndim != 2 or t.shape[1] != self.tdim or len(t) not in (1, n):
            raise ValueError('%s: tex must be (%d,) or (N, %d) with one row per stress; got shape %s'
                             % (name, self.tdim, self.tdim, np.shape(tex)))
        return np.ascontiguousarray(t)

    def _tex_key(self):
        """digest of the tables the device evaluates for the texture SVC (cf. _content_key)"""
        h = hashlib.blake2b(b'tex_svc', digest_size=16)
        sc = self.std_scaler
        for a in (self.svc['sv'], self.svc['dual'], sc.mean_, sc.scale_,
                  np.array([self.svc['intercept'], self.gam_yf, 1. if self.dev_only else 0.])):
            h.update(_table_digest(np.ascontiguousarray(a, dtype=float).reshape(-1)))
        return h.digest()

    def _load_tex(self):
        """Make the texture SVC the table set of the shared point context; re-sent only when its content differs."""
        if not self.ML_yf or self.svc is None or getattr(self, 'std_scaler', None) is None:
            raise AttributeError('texture material has no trained ML yield function; train_SVC trains it')
        ctx = _ctx()
        key = self._tex_key()
        if getattr(ctx, '_tex_key', None) != key:
            ctx._tex_key = None
            ctx.tex_svc_set(self.svc['sv'], self.svc['dual'], self.svc['intercept'], self.gam_yf, self.std_scaler.mean_,
                            self.std_scaler.scale_, dev_only=self.dev_only)
            ctx._tex_key = key
        return ctx

    def _tex_flow_ok(self, what):
        """``tex=`` of the flow-rule methods needs a texture material, as calc_yf's does"""
        if not getattr(self, 'txdat', False):
            raise NotImplementedError('%s: tex needs a texture material (from_data on data sets with tx_data)' % what)
        if not self._is_tex():
            self._svc_refuse(what)

    def _load_tex_flow(self, CV=None):
        """The texture set and, beside it as material 0 of the shared point context, the analytic Hill / J2 record of this
        material with the call's CV: elastic matrix, sy, khard and the form of seq for ML_full_yf(tex=) and response(tex=).
        ``_tex_key`` and ``_content_key`` decide when either is re-sent."""
        self._load_tex()
        return self._load(CV, ana=True)

    def _fgrad_tex(self, s0, epl, tex):
        """calc_fgrad(sig, tex=): the stress derivative of calc_yf(sig, tex) on the device (plfx_tex_svc_fgrad).  With f the
        standardised features, v_i the vectors and K_i = exp(-gamma |f - v_i|^2):
        g_j = -2 gamma sum_i dual_i K_i (f_j - v_ij), a_j = g_j / scale_j for the six stress columns, and for a dev_only set
        (a_0 + a_1 + a_2) / 3 is taken off a_0 .. a_2, the chain rule through the deviator.  With equal scales and zero means
        on the six stress columns this is the gradient of the 6-feature SVC material up to rounding (for a dev_only set: as
        far as the vectors are deviators, since the 6-feature gradient, like the reference's, is not projected).  khard is
        set to 0 and msg['gradient'] as in the 6-feature branch."""
        self._tex_flow_ok('calc_fgrad')
        if epl is not None and np.shape(epl) != s0.shape:
            raise ValueError('Parameter sig and epl must have the same shape.')
        if s0.shape != (6,) and not (s0.ndim == 2 and s0.shape[1] == 6):
            raise ValueError('Unknown format of stress in calc_fgrad')
        s, single = self._voigt(s0, 'calc_fgrad')
        t = self._tex_rows(tex, len(s), 'calc_fgrad')
        a = self._load_tex().tex_svc_fgrad(s, t)
        self.khard = 0.
        self.msg['gradient'] = 'gradient to ML_yf'
        return a[0] if single else a

    # ------------------------------------------------------------------ a texture material bound to one texture
    def fold_texture(self, tex):
        """The texture SVC at the fixed texture ``tex`` (tdim,) as a 6-feature SVC with one scale per stress column, host
        NumPy.  With f_j = (s_j - mean_j) / scale_j the stress features, ft the standardised features of ``tex``, v_k the
        vectors and K_k = exp(-gamma |f - v_k|^2): c_k = sum_t (ft_t - v_{k,6+t})^2 is a constant per vector,
        so  calc_yf(sig, tex=tex) = sum_k d'_k exp(-gamma |x - v'_k|^2) + intercept  with  d'_k = dual_k exp(-gamma c_k),
        v'_kj = v_kj + mean_j / scale_j  and  x_j = s_j / scale_j  (s: the deviator for a dev_only set).
        Returns ``dict(sv=v' (nsv,6), dual=d' (nsv,), intercept, gamma, scale (6,), dev_only)``: what ``at_texture`` sends to
        the device."""
        if not getattr(self, 'txdat', False):
            raise NotImplementedError('fold_texture: tex needs a texture material (from_data on data sets with tx_data)')
        if not self._is_tex():
            self._svc_refuse('fold_texture')
        if not self.ML_yf or self.svc is None or getattr(self, 'std_scaler', None) is None:
            raise AttributeError('texture material has no trained ML yield function; train_SVC trains it')
        t = np.asarray(tex, dtype=float)
        if t.shape != (self.tdim,) or not np.all(np.isfinite(t)):
            raise ValueError('fold_texture: tex must be a finite (%d,) array; got shape %s' % (self.tdim, np.shape(tex)))
        mean = np.asarray(self.std_scaler.mean_, dtype=float)
        scale = np.asarray(self.std_scaler.scale_, dtype=float)
        sv = np.asarray(self.svc['sv'], dtype=float)
        ft = (t - mean[6:]) / scale[6:]
        c = np.sum((ft[None, :] - sv[:, 6:]) ** 2, axis=1)
        return dict(sv=np.ascontiguousarray(sv[:, :6] + (mean[:6] / scale[:6])[None, :]),
                    dual=np.asarray(self.svc['dual'], dtype=float) * np.exp(-self.gam_yf * c),
                    intercept=float(self.svc['intercept']), gamma=float(self.gam_yf), scale=scale[:6].copy(),
                    dev_only=bool(self.dev_only))

    def at_texture(self, tex, name=None):
        """A new Material: this trained texture material bound to the texture ``tex`` (tdim,), which an FE model can hold --
        ``Model.assign``, ``solve``, ``field``, ``calc_properties`` -- and ``response`` / ``response_batch`` / ``ML_full_yf``
        run on the 16-lane row kernels.  It carries this material's elastic constants, sy, khard, Hill form
        and sdim = 6, the folded tables of ``fold_texture``, the texture and a reference to this material, which is left as it
        is.  ``calc_yf``, ``calc_fgrad``, ``yield_scale`` and ``yield_stress`` of the bound material are this material's
        ``tex=`` calls at the bound texture.  It hardens as ``response(..., tex=)`` does: sflow = sy + khard peeq."""
        f = self.fold_texture(tex)
        b = Material(name=name if name is not None else '%s@texture' % self.name, num=self.num)
        for k in ('E', 'nu', 'C11', 'C12', 'C44', 'sy', 'sy0', 'khard', 'drucker', 'hill_3p', 'hill_6p'):
            setattr(b, k, getattr(self, k))
        b.CV = np.array(self.CV, dtype=float)
        b.hill = np.array(self.hill, dtype=float)
        b.sdim = 6
        b.svc = dict(sv=f['sv'], dual=f['dual'], intercept=f['intercept'])
        b.gam_yf, b.C_yf, b.dev_only = f['gamma'], self.C_yf, f['dev_only']
        b.scale_seq = float(f['scale'][0])   # the record's nominal scale; the device divides column j by scale[j]
        b.ML_yf = True
        b.Ndof = 6
        b._bound = dict(parent=self, tex=np.array(tex, dtype=float), scale=f['scale'])
        return b

    # ------------------------------------------------------------------ a texture field: one texture per element
    def fold_textures(self, tex):
        """``fold_texture`` for T textures, ``tex`` (T, tdim) with T >= 1: the dict of ``fold_texture`` with ``dual`` of shape
        (T, nsv).  Only the dual coefficients depend on the texture; vectors, scales, gamma and intercept are shared.  Row t
        is ``fold_texture(tex[t])['dual']`` bit for bit: the rows are folded one by one, in the summation order of the
        single fold."""
        if not getattr(self, 'txdat', False):
            raise NotImplementedError('fold_textures: tex needs a texture material (from_data on data sets with tx_data)')
        if not self._is_tex():
            self._svc_refuse('fold_textures')
        if not self.ML_yf or self.svc is None or getattr(self, 'std_scaler', None) is None:
            raise AttributeError('texture material has no trained ML yield function; train_SVC trains it')
        t = np.asarray(tex, dtype=float)
        if t.ndim != 2 or t.shape[1] != self.tdim or len(t) < 1 or not np.all(np.isfinite(t)):
            raise ValueError('fold_textures: tex must be a finite (T, %d) array with T >= 1; got shape %s'
                             % (self.tdim, np.shape(tex)))
        f = self.fold_texture(t[0])
        f['dual'] = np.ascontiguousarray(np.stack([f['dual']] + [self.fold_texture(r)['dual'] for r in t[1:]]))
        return f

    def at_textures(self, tex, name=None):
        """A new Material: this trained texture material with a FIELD of textures ``tex`` (T, tdim), one row per element of a
        model (``Model.set_texture_ids``) or per point (``tex_id=`` of ``response``, ``response_batch``, ``ML_full_yf``).  An
        element with row t behaves as ``at_texture(tex[t])`` does, in every output.  It is a bound material
        whose ``svc['dual']`` is row 0; ``_bound`` holds the textures and the coefficient rows ``coef`` (T, nsv) besides.
        One engine material and one launch per sweep phase, whatever T is."""
        f = self.fold_textures(tex)
        b = self.at_texture(np.asarray(tex, dtype=float)[0], name=name if name is not None else '%s@textures' % self.name)
        b._bound['tex'] = np.array(tex, dtype=float)
        b._bound['coef'] = f['dual']
        return b

    def _tex_ids(self, tex_id, n, what):
        """``tex_id`` of a point function: None for a material without a texture field (which takes none), else the rows of
        the n points as an (n,) int32 array (an int is shared by the points; default row 0)"""
        b = getattr(self, '_bound', None)
        if b is None or 'coef' not in b:
            if tex_id is not None:
                raise NotImplementedError('%s: tex_id needs a material with a texture field (at_textures)' % what)
            return None
        T = len(b['coef'])
        ids = np.asarray(0 if tex_id is None else tex_id)
        if ids.dtype.kind not in 'iu' or ids.ndim > 1 or (ids.ndim == 1 and len(ids) != n):
            raise ValueError('%s: tex_id must be an int or an (N,) int array with one row index per point; got dtype %s, '
                             'shape %s' % (what, ids.dtype, ids.shape))
        if ids.size and (ids.min() < 0 or ids.max() >= T):
            raise ValueError('%s: tex_id outside 0..%d' % (what, T - 1))
        return np.ascontiguousarray(np.broadcast_to(ids, (n,)), dtype=np.int32)

    # what to do instead where a bound material refuses
    _BOUND_REFUSALS = {
        'calc_hessian': 'no Hessian of the texture SVC is built',
        'flow_curve': "the parent's yield_scale(su, tex=) gives the points of the locus; response_batch follows a path",
        'polar_yield_locus': "the parent's texture_loci(tex) traces the locus",
        'yield_slices': "the parent's yield_scale(su, tex=) along the slice's directions gives the locus",
        'setup_fgrad_SVM': 'texture and work-hardening data are not combined',
        'train_SVC': 'train the parent and bind it again with at_texture',
        'export_MLparam': "the reference's file has no slots for one scale per stress column",
        'Committee': 'committees evaluate 6-feature SVC yield functions with one scale',
        'create_scaled_input': "fold_texture of the parent states the features, x_j = s_j / scale_j",
        'Model.distribute': 'a bound material runs on one GPU',
    }
    # ... and where a texture field refuses what a material bound to one texture offers
    _FIELD_REFUSALS = {
        'calc_properties': 'bind one texture with at_texture',
    }


    def _bound_refuse(self, what):
        """the one gate of a material bound to a texture (at_texture): the row kernels run it and nothing else does"""
        b = getattr(self, '_bound', None)
        if b is None:
            return
        if what in self._FIELD_REFUSALS:   # offered for one texture, refused for a field of them (at_textures)
            if 'coef' in b:
                raise NotImplementedError('%s: not offered for a texture field (at_textures); %s' % (what, self._FIELD_REFUSALS[what]))
            return
        raise NotImplementedError('%s: not offered for a material bound to a texture (at_texture); %s'
                                  % (what, self._BOUND_REFUSALS.get(what, 'use the parent material')))

    def _bound_call(self, fn, *a, tex_id=None, **kw):
        """a ``tex=`` call of the parent at the bound texture (a texture field: at the rows ``tex_id``, an int or one per
        point); the parent's khard, which its calc_fgrad(tex=) resets, is put back"""
        par = self._bound['parent']
        tex = self._bound['tex']
        if 'coef' in self._bound:
            n = len(a[0]) if np.ndim(a[0]) == 2 else 1
            ids = self._tex_ids(tex_id, n, fn)
            tex = tex[ids[0]] if np.ndim(0 if tex_id is None else tex_id) == 0 else tex[ids]
        elif tex_id is not None:
            self._tex_ids(tex_id, 1, fn)
        kh = par.khard
        try:
            return getattr(par, fn)(*a, tex=tex, **kw)
        finally:
            par.khard = kh

    def _tex_no_hardening(self, what, epl):
        """texture together with work hardening is not built: the device call of ML_full_yf(tex=) takes no plastic strain,
        so the flow stress is sy -- which is sy + khard peeq whenever khard or the plastic strain is zero"""
        if epl is not None and self.khard and np.any(np.asarray(epl, dtype=float) != 0.):
            raise NotImplementedError('%s: a plastic strain together with khard = %g on a texture material; texture and work '
                                      'hardening are not combined' % (what, self.khard))

    def set_tex_svc(self, support_vectors, dual_coef, intercept, gamma, mean, scale, dev_only=False, C=None):
        """Install a trained texture SVC on a material that ``from_data`` made a texture material: standardised support
        vectors (nsv, 6 + tdim), ``dual_coef_[0]``, ``intercept_[0]``, gamma and the scaler's ``mean_`` / ``scale_`` (what
        ``train_SVC`` leaves in ``svm_yf`` and ``std_scaler``)."""
        if not self._is_tex():
            raise ValueError('set_tex_svc: from_data must have installed texture data sets first')
        sv = np.ascontiguousarray(support_vectors, dtype=float)
        dual = np.ascontiguousarray(dual_coef, dtype=float).reshape(-1)
        mean, scale = np.array(mean, dtype=float).reshape(-1), np.array(scale, dtype=float).reshape(-1)
        if sv.ndim != 2 or sv.shape[1] != self.Ndof or len(dual) != len(sv) or len(mean) != self.Ndof or len(scale) != self.Ndof:
            raise ValueError('set_tex_svc: support vectors (nsv, %d), dual_coef (nsv,), mean and scale (%d,) expected'
                             % (self.Ndof, self.Ndof))
        sc = StdScaler.__new__(StdScaler)
        sc.mean_, sc.scale_, sc.var_, sc.n_samples_seen_ = mean, scale, scale ** 2, None
        self.std_scaler = sc
        self.svc = dict(sv=sv, dual=dual, intercept=float(intercept))
        self.gam_yf, self.C_yf = float(gamma), C
        self.dev_only = bool(dev_only)
        self.ML_yf = True
        self._version += 1

    def _no_flow_rule(self):
        if self.barlat and not getattr(self, 'barlat_normal', False):
            raise ValueError('calc_fgrad: analytical gradient for Barlat not implemented')
        if self.tresca:
            raise ValueError('calc_fgrad: analytical gradient for Tresca not implemented')

    def enable_svr_flow(self, on=True):
        """EXTENSION (the reference follows the SVR flow rule wherever ``ML_grad`` is set; this engine does so on request,
        and in the point functions only): with ``on`` and ``ML_grad`` set, ``response`` and ``response_batch`` run on the
        device with every gradient evaluation -- the normal and the hardening modulus of ``epl_dot`` / ``C_tan`` -- taken
        from the seven SVRs of ``setup_fgrad_SVM`` (material.py:207-346, 752-764), and ``response`` leaves
        ``khard`` at the value of the call's last gradient evaluation.  ``calc_properties`` and ``Model.solve`` keep
        refusing an SVR gradient.  Without this call nothing changes: while ``ML_grad`` is set, all four refuse."""
        if not hasattr(self, '_svr'):
            raise AttributeError('enable_svr_flow: setup_fgrad_SVM has not trained the SVR gradient')
        self.svr_flow = bool(on)
        self._version += 1
        return self

    def _svr_flow_on(self):
        """the point functions follow the SVR flow rule: enabled, trained, ML_grad still set, and the material is still the
        work-hardening SVC the rule attaches to (else the refusals of _no_svr_gradient hold as before)"""
        return bool(getattr(self, 'svr_flow', False) and getattr(self, 'ML_grad', False) and hasattr(self, '_svr')
                    and self.ML_yf and getattr(self, 'whdat', False))   # the record _load sends is SVC_WH: the rule attaches

    def _svr_flow_tables(self):
        """what plfx_set_svr_flow takes, in its argument order after the material index"""
        v = self._svr
        return (v['X'], v['coef'], v['intercept'], v['gamma'], self.sc_feat.mean_, self.sc_feat.scale_,
                np.concatenate((self.sc_grad.mean_, self.sc_khard.mean_)),
                np.concatenate((self.sc_grad.scale_, self.sc_khard.scale_)))

    def _no_svr_gradient(self, what):
        """the device's return mapping follows the gradient of the SVC yield function; only the point functions can follow
        an SVR gradient instead, and only on request (enable_svr_flow)"""
        if getattr(self, 'ML_grad', False) and self._svr_flow_on():
            if what in ('response', 'response_batch'):
                return
            raise NotImplementedError('%s: ML_grad is set, and the SVR gradient of setup_fgrad_SVM is followed by calc_fgrad, '
                                      'epl_dot / C_tan and, with enable_svr_flow, by the point functions response and '
                                      'response_batch only; set ML_grad = False to run with the SVC gradient' % what)
        if getattr(self, 'ML_grad', False):
            raise NotImplementedError('%s: ML_grad is set, and the SVR gradient of setup_fgrad_SVM is evaluated by calc_fgrad '
                                      '(and epl_dot / C_tan) only; set ML_grad = False to run with the SVC gradient' % what)

    def _content_key(self, CV=None, ana=False, rec=None, parameters_only=False):
        """Digest of everything the device evaluates for this material: the packed ``plfx_material`` record (kind, elastic
        and plastic parameters, Hill / Barlat coefficients, SVC scalars) and the support-vector / dual-coefficient tables.
        Two materials share a key only if the GPU would compute the same numbers for them -- never because one was
        garbage-collected and the next landed at the same address, and an attribute edited in place (``m.hill[0] = ...``,
        which the reference honours on the next call, material.py:139-205) changes the key.  ``parameters_only`` leaves
        out what is STATE rather than a parameter: the hardening modulus of a work-hardening SVC material, which every
        gradient evaluation overwrites (material.py:808-814)."""
        if rec is None:
            rec = self._record(np.asarray(self.CV if CV is None else CV, dtype=float), ana=ana)
        m, keep = rec
        h = hashlib.blake2b(digest_size=16)
        sv_ptr, dual_ptr = m.sv, m.dual
        kh = m.khard
        m.sv = m.dual = None             # host addresses of the tables are not content
        if parameters_only and m.kind == _lib.SVC_WH:
            m.khard = 0.
        h.update(bytes(m))
        m.sv, m.dual, m.khard = sv_ptr, dual_ptr, kh
        for a in keep:
            h.update(_table_digest(np.ascontiguousarray(a)))
        if m.kind == _lib.SVC_WH and self._svr_flow_on():
            # the SVR flow rule is attached to this record (_load): its tables and scalers are evaluated by the device too
            h.update(b'svr_flow')
            for a in self._svr_flow_tables():
                h.update(_table_digest(np.ascontiguousarray(a, dtype=float).reshape(-1)))
        return h.digest()

    def _load(self, CV=None, ana=False):
        """Make this material (with element matrix CV) material 0 of the shared point context.  The context keeps the last
        record it was given; it is re-sent whenever its CONTENT differs (see ``_content_key``)."""
        cv = np.asarray(self.CV if CV is None else CV, dtype=float)
        if cv.shape != (6, 6):
            raise ValueError('CV must be a (6,6) array')
        ctx = _ctx()
        rec = self._record(cv, ana=ana)
        key = self._content_key(rec=rec)
        if getattr(ctx, '_point_key', None) != key:
            ctx._point_key = None          # a failing set_materials must not leave a stale key behind
            ctx.set_materials([rec])
            if rec[0].kind == _lib.SVC_WH and self._svr_flow_on():
                ctx.set_svr_flow(0, *self._svr_flow_tables())
            ctx._point_key = key
        return ctx

    @staticmethod
    def _voigt(sig, name):
        """(3,),(6,),(N,3),(N,6) -> (N,6) Voigt (principal stresses padded with zero shear)."""
        s = np.asarray(sig, dtype=float)
        sh = s.shape
        single = sh in ((3,), (6,))
        if single:
            s = s[None, :]
        if s.ndim != 2 or s.shape[1] not in (3, 6):
            raise TypeError('Unknown format of stress in %s' % name)
        if s.shape[1] == 3:
            s = np.concatenate((s, np.zeros((len(s), 3))), axis=1)
        return np.ascontiguousarray(s), single

    def _princ_rows(self, s):
        """Principal-stress materials (sdim = 3: 3-parameter Hill; the 2-feature SVC, whose polar-angle feature is taken from
        the principal stresses, basic.py:68-104) see a Voigt stress through ``basic.sig_princ`` -- the
        general eigen-solver ``np.linalg.eig`` plus the axis-tracking re-ordering (basic.py:153-175) -- and the ORDER of the
        principal stresses enters the Hill form (material.py:667-670).  For plane states (every state of a 2-d model) the
        device reproduces that order in closed form; for states with out-of-plane shear it depends on LAPACK's eigenvalue
        order, so those rows are reduced HERE with the very same LAPACK call and handed to the device as diagonal states
        (whose order the device keeps): ``calc_seq`` and ``calc_yf`` then equal the reference for every stress state
        (fixture ``tests/golden/princ_general.npz``); ``ML_full_yf`` searches along the ray of the reduced state (the order
        does not change along a ray) and ``calc_fgrad`` with a (6,) stress takes its equivalent stress from ``calc_seq``
        (round 5; same fixture).  SCOPE: ``response`` is NOT covered -- it re-orders the principal stresses of a new stress
        in each of its up to 50 sub-steps (material.py:250-340), which the device does by the natural rule "axis i -> the
        eigenvector with the largest component i"; the reference's order there is whatever LAPACK's ``dgeev`` returns
        (measured on the fixture's 160 states: 94 % of the elastic and 25 % of the plastic results coincide).  Plane states
        -- all a 2-d ``Model`` ever produces -- are exact; ``response`` warns when it is handed anything else."""
        if self.sdim != 3 or self.tresca or self.barlat:   # (Tresca, Barlat: symmetric in the principal values)
            return s
        gen = (s[:, 3] != 0.) | (s[:, 4] != 0.)
        if not np.any(gen):
            return s
        s = s.copy()
        sp, _ = sig_princ(s[gen])
        s[gen, 0:3] = sp.reshape(-1, 3)
        s[gen, 3:6] = 0.
        return s

    # ------------------------------------------------------------------ constitutive functions
    def calc_seq(self, sig):
        """Generalised (Hill/Drucker) equivalent stress (material.py:576-676)."""
        s, single = self._voigt(sig, 'calc_seq')
        if self.sy is None:
            seq = sig_eq_j2(s)  # elastic material: J2 (material.py:637-640)
        else:
            seq = self._load(ana=True).seq(0, self._princ_rows(s))
            self.msg['equiv'] = ('6-parameter Hill, full Voigt stress'
                                 if self.sdim == 6 and not (self.tresca or self.barlat) else '3-parameter Hill')
        return seq[0] if single else seq

    def calc_seqB(self, sv):
        """Yld2004-18p (Barlat et al.) equivalent stress of Voigt stresses (material.py:678-702), evaluated by the device
        routine that `calc_seq` uses for Barlat materials (closed-form principal values of the two transformed
        deviators)."""
        if not self.barlat:
            raise AttributeError('calc_seqB: material has no Barlat parameters (plasticity(barlat=..., barlat_exp=...))')
        s, single = self._voigt(sv, 'calc_seqB')
        if s.shape[1] != 6:
            raise ValueError('calc_seqB: Voigt stress (6,) or (N,6) expected')
        seq = self._load(ana=True).seq(0, s)
        return seq[0] if single else seq

    def create_scaled_input(self, sig, epl=None, acc_strain=None, max_stress=None, flag=None, tex=None):
        """Feature vectors of the SVC yield function for stresses (material.py:2301-2346, the branch without texture and
        work-hardening features — the ones this engine evaluates): principal-stress cylinder coordinates for sdim=3,
        (deviatoric) Voigt stress / scale_seq for sdim=6.  Host-side helper for scripts; the kernels build the same
        features in registers."""
        self._bound_refuse('create_scaled_input')
        if self._is_tex():   # material.py:2347-2361 (no PCA): unscaled features through the fitted scaler
            if tex is None:
                raise ValueError('create_scaled_input: a texture material needs tex')
            if getattr(self, 'std_scaler', None) is None:
                raise AttributeError('create_scaled_input: no scaler fitted; train_SVC fits it')
            s, _ = self._voigt(sig, 'create_scaled_input')
            x = np.zeros((len(s), self.Ndof))
            x[:, 0:6] = sig_dev(s) if self.dev_only else s
            x[:, self.ind_tx:] = self._tex_rows(tex, len(s), 'create_scaled_input')
            return self.std_scaler.transform(x)
        if tex is not None or getattr(self, 'txdat', False):
            raise NotImplementedError('create_scaled_input: texture features need a texture material (from_data on data '
                                      'sets with tx_data)')
        s, _ = self._voigt(sig, 'create_scaled_input')
        x = np.zeros((len(s), self.Ndof))
        if self.sdim == 3:
            x[:, 0] = sig_eq_j2(s) / self.scale_seq - 1.
            x[:, 1] = sig_polar_ang(s) / np.pi
        else:
            if self.dev_only:
                s = sig_dev(s)
            x[:, 0:s.shape[1]] = s / self.scale_seq
        if getattr(self, 'whdat', False):   # material.py:2342-2346
            iw = self.ind_wh
            x[:, iw:iw + self.sdim] = (0. if epl is None else np.asarray(epl, dtype=float)) / self.scale_wh
            x[:, iw + self.sdim] = 0. if acc_strain is None else acc_strain
            x[:, iw + self.sdim + 1] = (0. if max_stress is None else max_stress) / self.scale_seq
            x[:, iw + self.sdim + 2] = 0. if flag is None else flag
        return x

    def get_sflow(self, epl):
        """Scalar flow stress for a plastic strain tensor or PEEQ (material.py:974-1007)."""
        peeq = epl if type(epl) in (float, np.float64) else eps_eq(epl)
        return self.sy + peeq * self.khard

    def calc_yf(self, sig, epl=None, ana=False, pred=False, tex=None, tex_id=None, **kw):
        """Yield function: analytic ``calc_seq - sflow`` or the SVC decision function (material.py:348-412).  A texture
        material takes ``tex``, one descriptor (tdim,) or one per stress (N, tdim), and raises the reference's ValueError
        without it."""
        if getattr(self, '_bound', None) is not None and not ana:   # (no plastic strain enters the texture features)
            if tex is not None:
                raise ValueError('calc_yf: the material is bound to a texture (at_texture) and takes no tex')
            f = self._bound_call('calc_yf', np.asarray(sig, dtype=float), pred=pred, tex_id=tex_id)
            self.msg['yield_fct'] = self._bound['parent'].msg['yield_fct']
            return f
        self._tex_ids(tex_id, 1, 'calc_yf')
        s, single = self._voigt(sig, 'calc_yf')
        if self.ML_yf and not ana and getattr(self, 'txdat', False):
            if tex is None:
                raise ValueError("SVM is trained on texture data but no texture data is given to evaluate yf!")
            if not self._is_tex():
                self._svc_refuse('calc_yf')
            t = self._tex_rows(tex, len(s), 'calc_yf')
            f = self._load_tex().tex_svc_yf(s, t)
            if pred:   # svm_yf.predict: decision >= 0 -> +1 (libsvm)
                f = np.where(f >= 0., 1., -1.)
                self.msg['yield_fct'] = 'ML_yf-predict'
            else:
                self.msg['yield_fct'] = 'ML_yf-decision-fct'
            return f[0] if single else f
        if tex is not None and not (getattr(self, 'txdat', False)):
            raise NotImplementedError('calc_yf: tex needs a texture material (from_data on data sets with tx_data)')
        if epl is None:
            e = np.zeros((len(s), 6))
        elif type(epl) in (float, np.float64):
            e = np.tile(epl * np.array([1., -0.5, -0.5, 0., 0., 0.]), (len(s), 1))
        else:
            e = np.asarray(epl, dtype=float)
            if e.ndim == 1:
                e = np.tile(e, (len(s), 1))
        if self.ML_yf and not ana:
            f = self._load().yf(0, self._princ_rows(s), e)
            if pred:
                f = np.where(f > 0., 1., -1.)
                self.msg['yield_fct'] = 'ML_yf-predict'
            else:
                self.msg['yield_fct'] = 'ML_yf-decision-fct'
        else:
            f = self._load(ana=True).yf(0, self._princ_rows(s), e)
            self.msg['yield_fct'] = 'analytical'
        return f[0] if single else f

    def find_yloc(self, x, su, epl=None, tex=None, **kw):
        """Yield function at ``sig = x[:, None] * su`` for N unit stresses at once (material.py:518-545): the objective
        that the reference's training / plotting scripts hand to ``scipy.optimize.fsolve`` to trace yield loci
        (``plot_yield_locus`` :3017, ``calc_yf`` on (N, sdim) grids); one batched GPU evaluation per call."""
        if getattr(self, 'txdat', False) and tex is None:
            raise ValueError("SVM is trained on texture data but no texture data was provided to this function.")
        x = np.asarray(x, dtype=float)
        su = np.asarray(su, dtype=float)
        return self.calc_yf(x[:, None] * su, epl=epl, tex=tex)

    def find_yloc_scalar(self, x, su, epl=None, tex=None, **kw):
        """scalar form of `find_yloc` (material.py:547-574): ``calc_yf(x * su)``"""
        if getattr(self, 'txdat', False) and tex is None:
            raise ValueError("SVM is trained on texture data but no texture data was provided to this function.")
        return self.calc_yf(float(x) * np.asarray(su, dtype=float), epl=epl, tex=tex)

    def ML_full_yf(self, sig, epl=None, ld=None, verb=True, tex=None, tex_id=None, **kw):
        """Distance of a stress to the ML yield locus along its ray / the loading direction
        (material.py:414-516).  Accepts a single stress like the reference, or (N,6).  EXTENSION: a texture material takes
        ``tex``, (tdim,) or (N, tdim): the same search on calc_yf(x su, tex) with seq the J2 / Hill form of the material and
        the flow stress sy + khard peeq; ``ld`` is not offered together with ``tex``.  A texture field
        (``at_textures``) takes ``tex_id``, an int or (N,) ints, the row of its texture table per stress."""
        if tex is not None:
            self._tex_ids(tex_id, 1, 'ML_full_yf')
            return self._full_yf_tex(sig, epl, ld, verb, tex)
        if getattr(self, '_bound', None) is None:
            self._tex_ids(tex_id, 1, 'ML_full_yf')   # (refused: no texture field)
        self._tex_refuse('ML_full_yf')
        if not self.ML_yf:
            raise AttributeError('ML_full_yf: material has no trained ML yield function')
        s = np.asarray(sig, dtype=float)
        if s.shape not in ((3,), (6,)) and not (s.ndim == 2 and s.shape[1] == 6):
            raise ValueError('Only individual stress tensors supported in material.ML_full_yf. '
                             'Shape of argument is {}'.format(s.shape))
        s, single = self._voigt(s, 'ML_full_yf')
        e = None
        if epl is not None:
            e = np.asarray(epl, dtype=float)
            if e.ndim == 1:
                e = np.tile(e, (len(s), 1))
        tid = self._tex_ids(tex_id, len(s), 'ML_full_yf')
        f, st = self._load().full_yf(0, self._princ_rows(s), e, ld, tex_id=tid)
        if verb and np.any(st != 0):
            warnings.warn('ML_full_yf: Could not bracket / locate the yield locus for %d stress(es); '
                          'conservative estimate seq-0.85*sflow returned' % int(np.sum(st != 0)))
        return f[0] if single else f

    def _full_yf_tex(self, sig, epl, ld, verb, tex):
        self._tex_flow_ok('ML_full_yf')
        if ld is not None:
            raise NotImplementedError('ML_full_yf: a loading direction ld together with tex is not offered')
        s = np.asarray(sig, dtype=float)
        if s.shape != (6,) and not (s.ndim == 2 and s.shape[1] == 6):
            raise ValueError('Only individual stress tensors supported in material.ML_full_yf. '
                             'Shape of argument is {}'.format(s.shape))
        s, single = self._voigt(s, 'ML_full_yf')
        t = self._tex_rows(tex, len(s), 'ML_full_yf')
        self._tex_no_hardening('ML_full_yf', epl)
        f, st = self._load_tex_flow().tex_svc_full_yf(s, t)
        if verb and np.any(st != 0):
            warnings.warn('ML_full_yf: Could not bracket / locate the yield locus for %d stress(es); '
                          'conservative estimate seq-0.85*sflow returned' % int(np.sum(st != 0)))
        return f[0] if single else f

    def calc_fgrad(self, sig, epl=None, seq=None, ana=False, tex=None, tex_id=None, **kw):
        """Gradient of the yield function w.r.t. stress (material.py:704-858).  EXTENSION: a texture material takes ``tex``,
        (tdim,) or (N, tdim), and returns the stress derivative of ``calc_yf(sig, tex=)`` (see ``_fgrad_tex``)."""
        if getattr(self, '_bound', None) is not None and not ana:   # (khard is a parameter of a bound material: left alone)
            if tex is not None:
                raise ValueError('calc_fgrad: the material is bound to a texture (at_texture) and takes no tex')
            a = self._bound_call('calc_fgrad', np.asarray(sig, dtype=float), epl=epl, tex_id=tex_id)
            self.msg['gradient'] = 'gradient to ML_yf'
            return a
        self._tex_ids(tex_id, 1, 'calc_fgrad')
        if tex is not None and not ana:
            return self._fgrad_tex(np.asarray(sig, dtype=float), epl, tex)
        if self.ML_yf and not ana:
            self._tex_refuse('calc_fgrad')
        s0 = np.asarray(sig, dtype=float)
        if epl is not None and np.shape(epl) != s0.shape:
            raise ValueError('Parameter sig and epl must have the same shape.')
        nd = self.sdim if self.sdim is not None else 6
        if s0.shape not in ((3,), (6,)) and not (s0.ndim == 2 and s0.shape[1] == nd):
            raise ValueError('Unknown format of stress in calc_fgrad')
        if getattr(self, 'ML_grad', False) and not ana:
            return self._fgrad_svr(s0, epl)
        if not (self.ML_yf and not ana):
            self._no_flow_rule()
        s, single = self._voigt(s0, 'calc_fgrad')
        nout = s0.shape[-1]  # principal stresses in -> gradient w.r.t. principal stresses out
        if self.ML_yf and not ana and getattr(self, 'whdat', False):
            # the plastic strain is part of the feature vector, and the hardening modulus is read off the gradient
            # w.r.t. the plastic-strain features: mean over the points, no softening (material.py:808-814)
            e = None if epl is None else np.asarray(epl, dtype=float).reshape(len(s), -1)
            a, hk = self._load().fgrad_wh(0, s, e)
            self.khard = max(0., float(np.sum(hk)) / len(s))
            self.msg['gradient'] = 'gradient to ML_yf'
        elif self.ML_yf and not ana:
            a = self._load().fgrad(0, s)
            self.khard = 0.  # side effect of the reference (material.py:812-814, no work-hardening data)
            self.msg['gradient'] = 'gradient to ML_yf'
        else:
            # the reference's analytic form takes the deviator of the components it is GIVEN (principal stresses for (3,) /
            # (N,3) input, Voigt normals for a (6,) stress) and the equivalent stress from `seq` or calc_seq (:834-838) --
            # for a (6,) stress of a principal-stress material that is seq in sig_princ's order over the deviator of the Voigt
            # normals, not the principal-space normal that epl_dot / C_tan build (:1044-1047, `fgrad`)
            if seq is not None or (self.sdim == 3 and nout == 6):
                q = self.calc_seq(s) if seq is None else np.broadcast_to(np.asarray(seq, dtype=float).reshape(-1), (len(s),))
                a = self._load(ana=True).fgrad_seq(0, s, np.ascontiguousarray(q))
            else:
                a = self._load(ana=True).fgrad(0, s)
            h = self.hill
            if self.sdim == 6:
                self.msg['gradient'] = ('analytical, J2 isotropic, full stress' if np.all(h == 1.)
                                        else 'analytical, 6-parameter Hill, full stress')
            else:
                self.msg['gradient'] = ('analytical, J2 isotropic, princ. stress' if np.all(h == 1.)
                                        else 'analytical, 3-parameter Hill, princ. stress')
        a = a[:, :nout]
        return a[0] if single else a

    # ------------------------------------------------------------------ SVR flow rule
    SVR_EPSILON, SVR_TOL = 0.01, 1e-4   # the reference's SVR settings (material.py:2076-2089)

    def setup_fgrad_SVM(self):
        """Train the SVR flow rule on the work-hardening data of ``from_data`` (material.py:2058-2131): seven RBF
        epsilon-SVRs on the standardised features [flow_stress | plastic_strain], six for the components of the plastic
        strain direction eps / peeq and one for the local hardening rate d seq / d peeq, all with C_yf, gam_yf,
        epsilon 0.01 and tol 1e-4, fitted in one batched call on the GPU (libsvm's epsilon-SVR without shrinking).  Sets
        svm_grad0 .. svm_grad5, svm_khard, sc_feat, sc_grad, sc_khard and ML_grad = True."""
        self._tex_refuse('setup_fgrad_SVM')
        self._bound_refuse('setup_fgrad_SVM')
        if not getattr(self, 'whdat', False):
            raise ValueError('No strain hardening data available.')
        if not self._msparam_ok():
            raise NotImplementedError('setup_fgrad_SVM: the work-hardening data must be one data set installed by from_data')
        if self.C_yf is None or self.gam_yf is None:
            raise ValueError('setup_fgrad_SVM: C_yf and gam_yf are not set; train_SVC sets them')
        eps = np.asarray(self.msparam[0]['plastic_strain'], dtype=float)
        sig = np.asarray(self.msparam[0]['flow_stress'], dtype=float)
        # seq from the principal stresses, as the reference's sig_eq_j2 forms it: the hardening rate divides differences of
        # seq, which keep the last bits the direct Voigt form of basic.sig_eq_j2 rounds differently
        peeq, seq = eps_eq(eps), sig_eq_j2(sig_princ(sig)[0])
        ndata = len(seq)
        X_gt = np.concatenate((sig, eps), axis=1)
        ok = peeq > 1.e-12
        y_gt = np.zeros((ndata, 6))
        y_gt[ok] = eps[ok] / peeq[ok, None]
        y_kh = np.zeros(ndata)   # forward difference along the rows; the last row has no successor
        hh = peeq[1:] - peeq[:-1]
        step = np.abs(hh) > 1.e-12
        y_kh[:-1][step] = (seq[1:] - seq[:-1])[step] / hh[step]
        self.sc_feat, self.sc_grad, self.sc_khard = StdScaler(X_gt), StdScaler(y_gt), StdScaler(y_kh.reshape(-1, 1))
        x_sc = self.sc_feat.transform(X_gt)
        y_sc = np.concatenate((self.sc_grad.transform(y_gt), self.sc_khard.transform(y_kh.reshape(-1, 1))), axis=1)
        ctx = _ctx()
        rows = np.arange(ndata)
        fits = ctx.svr_fit_batch(x_sc, [rows] * 7, [y_sc[:, m] for m in range(7)], self.C_yf, self.gam_yf,
                                 epsilon=self.SVR_EPSILON, tol=self.SVR_TOL)
        svr = [SVRModel(ctx, x_sc, r, self.C_yf, self.gam_yf, self.SVR_EPSILON) for r in fits]
        (self.svm_grad0, self.svm_grad1, self.svm_grad2, self.svm_grad3, self.svm_grad4, self.svm_grad5,
         self.svm_khard) = svr
        self._svr = dict(X=x_sc, coef=np.ascontiguousarray(np.stack([m.coef_ for m in svr], axis=1)),
                         intercept=np.array([m.intercept_[0] for m in svr]), gamma=float(self.gam_yf))
        self.ML_grad = True

    def _fgrad_svr(self, sig, epl):
        """the ML_grad branch of calc_fgrad (material.py:752-764): the six SVR predictions on [sig | epl], standardised and
        scaled back, all points and all seven models in one kernel pass; khard from the hardening SVR at the LAST point
        (a float; the reference leaves a (1,) array)"""
        if not hasattr(self, '_svr'):
            raise AttributeError('calc_fgrad: ML_grad is set, but setup_fgrad_SVM has not trained the SVR gradient')
        single = sig.shape == (6,)
        if not single and not (sig.ndim == 2 and sig.shape[1] == 6):
            raise ValueError('Unknown format of stress in calc_fgrad')
        s = sig.reshape(-1, 6)
        e = np.zeros_like(s) if epl is None else np.asarray(epl, dtype=float).reshape(-1, 6)
        if len(s) == 0:
            return np.zeros((0, 6))
        v = self._svr
        out = _ctx().svr_predict_multi(v['X'], v['coef'], v['intercept'], v['gamma'],
                                       self.sc_feat.transform(np.concatenate((s, e), axis=1)))
        a = self.sc_grad.inverse_transform(out[:, :6])
        self.khard = float(self.sc_khard.inverse_transform(out[-1:, 6:7])[0, 0])
        self.msg['gradient'] = 'SVR gradient'
        return a[0] if single else a

    def calc_hessian(self, sig, epl=None, seq=None, accumulated_strain=0.0, max_stress=0.0, flag=0.0, tex=None, ana=False):
        """Hessian of the SVC yield function at (6,) or (N,6) stresses, shape (N,6,6) (material.py:860-972).

        With x the scaled features, v_i the support vectors, c_i the dual coefficients and d_i = v_i - x, the device
        evaluates ``Hx[a][b] = sum_i c_i exp(-gamma |d_i|^2) (4 gamma^2 d_i[a] d_i[b] - 2 gamma delta_ab)`` -- the distance
        over all features (the plastic strain of a work-hardening material included), a and b over the stress features --
        and, like the reference, this returns ``Hx / scale_seq`` with ONE power of ``scale_seq`` (:962).  The mathematical
        second derivative in stress units is ``Hx / scale_seq**2``; ``hessian * scale_seq`` of the returned array is the
        feature-space Hessian ``Hx``.  For ``dev_only`` materials the features are the deviator's components and, again
        like the reference, no chain rule through the deviator projection is applied.  Analytic yield functions have no
        Hessian in the reference (``ValueError``), nor have sdim = 3 ML materials (``NotImplementedError``).
        Unlike ``calc_fgrad`` this touches neither ``khard`` nor ``msg``."""
        self._tex_refuse('calc_hessian')
        self._bound_refuse('calc_hessian')
        if tex is not None:
            raise NotImplementedError('calc_hessian: texture features are outside this engine; ' + self._TEX_REFUSALS['calc_hessian'])
        if getattr(self, 'ML_grad', False) and not ana:
            raise NotImplementedError('calc_hessian: analytical gradient for SVR not implemented')
        s = np.asarray(sig, dtype=float)
        if s.shape in ((3,), (6,)):
            s = s[None, :]
        elif s.ndim == 0 or s.shape != (len(s), self.sdim):
            raise ValueError('Unknown format of stress in calc_fgrad')
        if not (self.ML_yf and not ana):
            if self.barlat:
                raise ValueError('calc_hessian: analytical hessian for Barlat not implemented')
            if self.tresca:
                raise ValueError('calc_hessian: analytical hessian for Tresca not implemented')
            if self.hill is not None and len(self.hill):
                raise ValueError('calc_hessian: analytical hessian for Hill not implemented')
            return np.zeros((len(s), self.sdim, self.sdim))   # an elastic material: the reference's zeros (:907, 972)
        if self.sdim == 3:
            raise NotImplementedError('calc_hessian: not  implemented for 3D stress')
        if s.shape[1] != 6:
            raise ValueError('Unknown format of stress in calc_fgrad')
        e = None
        if getattr(self, 'whdat', False):
            if accumulated_strain or max_stress or flag:
                raise NotImplementedError('calc_hessian: the accumulated-strain, max-stress and flag features are zero '
                                          'on every path of this engine')
            if epl is not None:
                if type(epl) in (float, np.float64):   # PEEQ -> a plastic strain along the stress (:889-892)
                    e = epl * s / sig_eq_j2(s).reshape(-1, 1)
                else:
                    e = np.asarray(epl, dtype=float)
                    if e.shape == (6,):
                        e = np.tile(e, (len(s), 1))
                    elif e.shape != s.shape:
                        raise ValueError('Parameter sig and epl must have the same shape.')
        return self._load().hessian(0, np.ascontiguousarray(s), e) / self.scale_seq

    def response(self, sig, epl, deps, CV, maxit=50, tex=None, tex_id=0):
        """Elastic-predictor / plastic-corrector update of one material point (material.py:207-346).
        Returns ``fy1, sig, depl, grad_stiff``; ``msg['nsteps']`` is set as in the reference.  EXTENSION: a texture
        material takes ``tex`` (tdim,): the same update with calc_yf, ML_full_yf and calc_fgrad at that texture
        (DESIGN.md §32).  A texture field (``at_textures``) takes ``tex_id``, the row of its texture table."""
        sig = np.asarray(sig, dtype=float)
        sh = sig.shape
        if sh != (6,) and sh != (3,):
            raise ValueError('Only individual stress tensors supported in material.response. '
                             'Shape of argument is {}'.format(sh))
        if sh == (3,):
            raise NotImplementedError('response: pass the Voigt stress (6,); (3,) principal input is not supported')
        b = getattr(self, '_bound', None)
        if b is None or 'coef' not in b or tex is not None:   # (only a texture field takes a row; 0, the default, is no row)
            if np.ndim(tex_id) != 0 or tex_id != 0:
                self._tex_ids(tex_id, 1, 'response')
            tid = None
        else:
            if np.ndim(tex_id) != 0:
                raise ValueError('response: tex_id must be one int')
            tid = self._tex_ids(tex_id, 1, 'response')
        if tex is not None:
            self._tex_flow_ok('response')
            maxit = int(maxit)
            if maxit < 1:
                raise ValueError('response: maxit must be >= 1')
            t = self._tex_rows(tex, 1, 'response')
            fy, so, dp, ct, ns = self._load_tex_flow(CV).tex_svc_response(
                sig[None, :], np.asarray(epl, dtype=float)[None, :], np.asarray(deps, dtype=float)[None, :], t, maxit=maxit)
            self.msg['nsteps'] = int(ns[0])
            return fy[0], so[0], dp[0], ct[0].reshape(6, 6)
        self._tex_refuse('response')
        self._no_svr_gradient('response')
        self._no_flow_rule()
        maxit = int(maxit)
        if maxit < 1:
            raise ValueError('response: maxit must be >= 1')
        if self.sy is None:
            raise AttributeError('response called for a purely elastic material')
        if getattr(self, 'whdat', False):
            # Material.khard is state here: read on entry, overwritten by every gradient evaluation inside the call
            fy, so, dp, ct, ns, kout = self._load(CV).response(sig[None, :], np.asarray(epl, dtype=float)[None, :],
                                                               np.asarray(deps, dtype=float)[None, :],
                                                               khard_in=[self.khard], return_khard=True, maxit=maxit)
            self.khard = float(kout[0])
            if self._svr_flow_on():
                self.msg['gradient'] = 'SVR gradient'
        else:
            fy, so, dp, ct, ns = self._load(CV).response(sig[None, :], np.asarray(epl, dtype=float)[None, :],
                                                         np.asarray(deps, dtype=float)[None, :], maxit=maxit, tex_id=tid)
        self.msg['nsteps'] = int(ns[0])
        return fy[0], so[0], dp[0], ct[0].reshape(6, 6)

    def response_batch(self, sig, epl, deps, CV, khard_in=None, return_khard=False, tex=None, tex_id=None):
        """``response`` on (N,6) arrays in one launch (extension; same numbers point by point).  ``khard_in`` /
        ``return_khard``: for a material that follows the SVR flow rule (``enable_svr_flow``), the hardening modulus of
        every point on entry (default: ``khard``) and, appended to the result, on exit; ``khard`` itself is left alone.
        A texture material takes ``tex``, (tdim,) shared by the points or (N, tdim); a point with a non-finite input comes
        back as NaN with nsteps = -1.  A texture field (``at_textures``) takes ``tex_id``, an int or (N,) ints: the row of
        its texture table per point (default 0); any other material raises NotImplementedError for it."""
        if getattr(self, '_bound', None) is None or tex is not None:
            self._tex_ids(tex_id, 1, 'response_batch')   # (refused: no texture field)
        if tex is not None:
            self._tex_flow_ok('response_batch')
            if khard_in is not None or return_khard:
                raise ValueError('response_batch: khard_in / return_khard are not offered together with tex')
            s = np.asarray(sig, dtype=float)
            if s.ndim != 2 or s.shape[1] != 6 or np.shape(epl) != s.shape or np.shape(deps) != s.shape:
                raise ValueError('response_batch: sig, epl and deps of shape (N, 6) expected with tex')
            t = self._tex_rows(tex, len(s), 'response_batch')
            fy, so, dp, ct, ns = self._load_tex_flow(CV).tex_svc_response(s, epl, deps, t)
            return fy, so, dp, ct.reshape(-1, 6, 6), ns
        self._tex_refuse('response_batch')
        self._no_svr_gradient('response_batch')
        if getattr(self, '_bound', None) is not None:
            return self._response_batch_bound(sig, epl, deps, CV, khard_in, return_khard, tex_id)
        if khard_in is not None or return_khard:
            if not self._svr_flow_on():
                raise ValueError('response_batch: khard_in / return_khard are for a material that follows the SVR flow rule '
                                 '(enable_svr_flow)')
            fy, so, dp, ct, ns, kout = self._load(CV).response(sig, epl, deps, khard_in=khard_in, return_khard=True)
            return (fy, so, dp, ct.reshape(-1, 6, 6), ns) + ((kout,) if return_khard else ())
        fy, so, dp, ct, ns = self._load(CV).response(sig, epl, deps)
        return fy, so, dp, ct.reshape(-1, 6, 6), ns

    def _response_batch_bound(self, sig, epl, deps, CV, khard_in, return_khard, tex_id=None):
        """response_batch of a material bound to a texture: rows with a non-finite sig, epl or deps are masked here and never
        sent; they come back NaN with nsteps = -1, the rule of response_batch(tex=)"""
        if khard_in is not None or return_khard:
            raise ValueError('response_batch: khard_in / return_khard are not offered for a material bound to a texture')
        s, e, d = (np.asarray(a, dtype=float) for a in (sig, epl, deps))
        if s.ndim != 2 or s.shape[1] != 6 or e.shape != s.shape or d.shape != s.shape:
            raise ValueError('response_batch: sig, epl and deps of shape (N, 6) expected')
        n = len(s)
        tid = self._tex_ids(tex_id, n, 'response_batch')
        ok = np.all(np.isfinite(s) & np.isfinite(e) & np.isfinite(d), axis=1)
        fy, so, dp = np.full(n, np.nan), np.full((n, 6), np.nan), np.full((n, 6), np.nan)
        ct, ns = np.full((n, 6, 6), np.nan), np.full(n, -1, dtype=np.int32)
        if np.any(ok):
            r = self._load(CV).response(np.ascontiguousarray(s[ok]), np.ascontiguousarray(e[ok]), np.ascontiguousarray(d[ok]),
                                        tex_id=None if tid is None else np.ascontiguousarray(tid[ok]))
            fy[ok], so[ok], dp[ok], ct[ok], ns[ok] = r[0], r[1], r[2], r[3].reshape(-1, 6, 6), r[4]
        return fy, so, dp, ct, ns

    def epl_dot(self, sig, epl, Cel, deps, tex=None, **kw):
        """Plastic strain increment relaxing the stress to the yield locus (material.py:1009-1055); ``tex`` (tdim,) for a
        texture material."""
        sig = np.asarray(sig, dtype=float)
        Cel = np.asarray(Cel, dtype=float)
        deps = np.asarray(deps, dtype=float)
        yfun = self.calc_yf(sig + Cel @ deps, epl=epl, tex=tex)
        if yfun <= yf_tolerance:
            return np.zeros(6)
        a = self._flow_normal(sig, epl, tex)
        hh = a @ Cel @ a + self.khard
        return (a @ Cel @ deps / hh) * a

    def _flow_normal(self, sig, epl=None, tex=None):
        """Normal of the flow rule as epl_dot / C_tan take it: calc_fgrad of the Voigt stress for sdim = 6; for sdim = 3 the
        gradient w.r.t. the PRINCIPAL stresses in the normal Voigt rows, shear rows zero (material.py:1044-1047, 1079-1081) --
        not calc_fgrad's form for a (6,) stress of such a material (see there)."""
        if tex is not None:
            return self.calc_fgrad(sig, tex=tex)
        if self.sdim == 3 and not (self.tresca or self.barlat):
            s, _ = self._voigt(sig, 'calc_fgrad')
            if not self.ML_yf:
                self._no_flow_rule()
            return self._load(ana=not self.ML_yf).fgrad(0, self._princ_rows(s))[0]
        return self.calc_fgrad(sig) if epl is None else self.calc_fgrad(sig, epl=np.asarray(epl, dtype=float))

    def C_tan(self, sig, Cel, epl=None, tex=None):
        """Continuum tangent stiffness (material.py:1057-1086); ``tex`` (tdim,) for a texture material."""
        Cel = np.asarray(Cel, dtype=float)
        # the reference evaluates calc_fgrad(sig, epl=epl) with zeros when epl is None (material.py:1076-1082): for a
        # work-hardening SVC the plastic strain is part of the feature vector and the call sets self.khard used below
        epl = np.zeros(self.sdim) if epl is None else np.asarray(epl, dtype=float)
        a = self._flow_normal(np.asarray(sig, dtype=float), epl, tex)
        ca = Cel @ a
        return Cel - np.outer(ca, ca) / (a @ ca + self.khard)

    # ------------------------------------------------------------------ SVC training
    def create_sig_data(self, N=None, mat_ref=None, sdata=None, Nseq=2, sflow=None, offs=0.01, extend=False, rand=False,
                        Fe=0.1, Ce=0.99):
        """Training stresses and labels (material.py:1950-2056): yield-locus stresses of ``mat_ref`` along N directions
        (or the given ``sdata``), scaled by Fe .. Ce into the elastic (label -1) and by 2-Ce .. 2-Fe (and 2.4, 3, 4, 5 with
        ``extend``) into the plastic regime (label +1).  Returns (st (M, sdim), yt (M,))."""
        if sflow is not None:
            print('WARNING: Parameter "sflow" no longer used in function "create_sig_data".')
        if self.sdim not in (3, 6):
            raise ValueError('create_sig_data: call plasticity(sdim=3 or 6) first')
        if sdata is None:
            if mat_ref is None:
                raise ValueError('create_data_sig: Neither sdata nor mat_ref are provided, cannot generate training data')
            if self.sdim == 3:
                if N is None:
                    warnings.warn('create_sig_data: Neither N not theta provided. Continuing with N=36 (sdim=3)')
                    N = 36
                theta = np.linspace(-np.pi, np.pi, N) if not rand else 2. * (np.random.rand(N) - 0.5) * np.pi
                sc = np.ones((N, 2))
                sc[:, 1] = theta
                su = sig_cyl2princ(sc)
            else:
                if N is None:
                    warnings.warn('create_sig_data: Neither N not theta provided. Continuing with N=300 (sdim=6)')
                    N = 300
                from .training import load_cases
                n3 = int(N / 3)
                su = load_cases(n3, N - n3)
                if self.dev_only:
                    su = sig_dev(su)
            sdata = su * mat_ref._yield_scale(su)[:, None]   # yield stress tensors representing ground truth
        else:
            sdata = np.asarray(sdata, dtype=float)
            if N is not None and N != len(sdata):
                warnings.warn(f'create_sig_data: N and dimension of sdata do not agree. Continuing with N ={len(sdata)}')
            if mat_ref is not None:
                warnings.warn('create_sig_data: using sdata for training, ignoring mat_ref')
            N = len(sdata)
        if self.dev_only:
            sdata = sig_dev(sdata)
        if Nseq == 1:
            midpoint = 0.5 * (Fe + Ce)
            seq = np.array([midpoint, 2. - midpoint])
        else:
            seq = np.append(np.linspace(Fe, Ce, Nseq), np.linspace(2. - Ce, 2. - Fe, Nseq))
        if extend:
            seq = np.append(seq, np.array([2.4, 3., 4., 5.]))
        Nd = len(seq)
        st = np.zeros((N * Nd, self.sdim))
        yt = np.zeros(N * Nd)
        for i in range(Nd):
            st[i * N:(i + 1) * N, :] = sdata[:, 0:self.sdim] * seq[i]
            yt[i * N:(i + 1) * N] = -1. if i < Nseq else +1.
        return st, yt

    def _yield_scale(self, su):
        """factor x per unit stress with calc_yf(x su) = 0 (the root of find_yloc that the reference takes with fsolve):
        sy / calc_seq(su) for the homogeneous analytic yield functions (J2, Hill, Drucker-Prager), a bracketed bisection on
        the device's calc_yf otherwise"""
        su = np.asarray(su, dtype=float)
        if self.sy is None:
            raise ValueError('create_sig_data: the reference material has no yield strength')
        if not (self.ML_yf or self.tresca or self.barlat or getattr(self, 'whdat', False)):
            return self.sy / self.calc_seq(su)
        n = len(su)
        lo, hi = np.zeros(n), np.full(n, float(self.sy))
        for _ in range(60):   # bracket: grow hi until the yield function is positive
            f = self.find_yloc(hi, su)
            if np.all(f > 0.):
                break
            hi = np.where(f > 0., hi, 2. * hi)
        else:
            raise ValueError('create_sig_data: yield locus of the reference material could not be bracketed')
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            f = self.find_yloc(mid, su)
            lo, hi = np.where(f > 0., lo, mid), np.where(f > 0., mid, hi)
        return 0.5 * (lo + hi)

    # ------------------------------------------------------------------ yield loci as arrays
    def _epl_rows(self, epl, n, name):
        """epl as calc_yf takes it -- None, a PEEQ scalar, (6,) or (N,6) -- as (N,6) rows or None"""
        if epl is None:
            return None
        if np.ndim(epl) == 0:   # PEEQ -> an arbitrary plastic strain tensor of that equivalent strain (material.py:381-383)
            return np.tile(float(epl) * np.array([1., -0.5, -0.5, 0., 0., 0.]), (n, 1))
        e = np.asarray(epl, dtype=float)
        if e.shape == (6,):
            e = np.tile(e, (n, 1))
        if e.shape != (n, 6):
            raise ValueError('%s: epl must be None, a PEEQ value, (6,) or (N,6) with one row per stress; got shape %s'
                             % (name, e.shape))
        return e

    def yield_scale(self, su, epl=None, x0=None, return_status=False, tex=None, tex_id=None):
        """Factor ``x`` with ``calc_yf(x * su, epl) = 0`` along unit stresses ``su`` -- (sdim,), (N,3) or (N,6) -- i.e. where
        the yield locus lies along these directions: the root search behind the reference's ``polar_plot_yl``
        (material.py:3290-3293, one ``fsolve`` over all N unknowns there), done on the device ray by ray in one launch.
        ``epl`` as ``calc_yf`` takes it (None, PEEQ, (6,), (N,6)); ``x0`` start values (scalar or (N,)), default
        ``get_sflow(epl) / seq_J2(su)``.

        Rays of an ML yield function have more than one root; returned is the one the marching bracket of ``ML_full_yf``
        (material.py:468-486) isolates: from ``x0`` down in steps of 2 % while the yield function is >= 0 (to 0.01 x0), else
        up in steps of 2 % while it is < 0 (to 5 x0), refined until the bracket is two neighbouring doubles.  Analytic
        yield functions (Hill / J2 / Drucker, Tresca, Barlat) are homogeneous: ``get_sflow(epl) / calc_seq(su)``, whatever the
        value of ``x0`` (a given ``x0 <= 0`` still makes the ray degenerate).
        A single stress returns a float.  Rays without a root come back as NaN (one warning names their count);
        ``return_status`` adds the status per ray: 0 root, 1 no bracket, 2 refinement cap reached, 3 degenerate ray (zero or
        hydrostatic direction without ``x0``, non-finite input, ``x0 <= 0``).

        A texture material takes ``tex``, one descriptor (tdim,) shared by the rays or one per ray (N, tdim); the default
        ``x0`` is ``sy / seq_J2(su)`` (no plastic strain enters its features)."""
        if self.sy is None:
            raise ValueError('yield_scale: the material has no yield strength')
        if getattr(self, '_bound', None) is not None:   # (the parent's search at the bound texture; no plastic strain enters it)
            if tex is not None:
                raise ValueError('yield_scale: the material is bound to a texture (at_texture) and takes no tex')
            return self._bound_call('yield_scale', np.asarray(su, dtype=float), x0=x0, return_status=return_status, tex_id=tex_id)
        self._tex_ids(tex_id, 1, 'yield_scale')
        s, single = self._voigt(su, 'yield_scale')
        if self.ML_yf and getattr(self, 'txdat', False):
            return self._yield_scale_tex(s, single, tex, x0, return_status)
        if tex is not None:
            raise NotImplementedError('yield_scale: tex needs a texture material (from_data on data sets with tx_data)')
        e = self._epl_rows(epl, len(s), 'yield_scale')
        x0 = self._ray_x0(x0, (len(s),), None,
                          'yield_scale: x0 must be a scalar or hold one start value per stress; got shape %s')
        ml = self.ML_yf
        # (_princ_rows: principal-stress materials see general states through the host's LAPACK call; plfx_yield_scale does the
        # same for callers of the C-ABI, csrc/plfx_material.hip, and finds nothing left to reduce in these rows)
        x, st = self._load(ana=not ml).yield_scale(0, self._princ_rows(s), e, x0)
        return self._ray_result('yield_scale', 'direction', x, st, single, return_status)

    def yield_stress(self, su, epl=None, tex=None, tex_id=None):
        """Stresses on the yield locus along the unit stresses ``su``: ``su * yield_scale(su, epl)[:, None]`` (NaN rows where
        no point of the locus was found); ``tex`` for a texture material."""
        s = np.asarray(su, dtype=float)
        x = self.yield_scale(s, epl=epl, tex=tex, tex_id=tex_id)
        return s * x if s.ndim == 1 else s * x[:, None]

    # ------------------------------------------------------------------ flow curves as arrays
    def flow_curve(self, su, epl_max=0.02, depl=1.e-3, epl0=None, predictor=0., max_steps=300, return_status=False):
        """Flow curves along fixed stress directions ``su`` -- (6,) or (N,6) -- as arrays: what ``plot_sig_eps`` of the
        reference's ``examples/train_hardening.py`` (lines 83-133) computes before it draws, N curves in one launch with the
        whole chains on the device.  Every direction is normalised to unit J2 stress.  Per curve, with ``epl = epl0``
        (None: zeros; (6,) or (N,6)): ``x_0`` is the point of the yield locus along ``su`` at ``epl``; then, while
        ``eps_eq(epl) + depl <= epl_max`` and fewer than ``max_steps`` steps are done: ``peeq = eps_eq(epl) + depl``,
        ``a = calc_fgrad(su * (x_k + peeq * predictor), epl)``, ``epl += a * depl / eps_eq(a)``, and ``x_{k+1}`` is the point
        of the locus at the new ``epl``.  ``predictor`` is the hardening coefficient that the example adds to the stress
        before it takes the gradient (its script-global ``khard``); 0 takes the gradient on the locus.
        ``epl_max = np.inf`` runs exactly ``max_steps`` steps.

        The point of the locus is the root of ``yield_scale`` for an ML yield function -- started at ``sy`` for ``x_0``, then
        at the previous root, so ``x_{k+1}`` has the bits of ``yield_scale(su, epl_{k+1}, x0=x_k)``; where the yield function
        changes sign once near the locus this is the root that the example's ``fsolve(..., mat.sy, xtol=1e-5)`` converges
        to, within that tolerance -- and ``get_sflow(epl) / calc_seq(su)`` for Hill / J2 / Drucker materials.

        Returns a dict (a single direction drops the leading N): ``sig`` (N,K+1,6) = ``su * x``, ``epl`` (N,K+1,6),
        ``seq`` (N,K+1) = ``sig_eq_j2(sig)``, ``peeq`` (N,K+1) = ``eps_eq(epl)``, ``yf`` (N,K+1) the yield function at every
        recorded point (the example reports its largest magnitude per curve), ``hk`` (N,K) the raw hardening value of every
        gradient evaluation as ``calc_fgrad`` forms it before the clip at 0 (NaN for materials without work-hardening
        features), ``nsteps`` (N,).  ``K = max(nsteps)``; entries past a curve's ``nsteps`` are NaN.  Unlike ``calc_fgrad``
        this function leaves ``khard`` alone (the reference overwrites it at every gradient evaluation).
        ``return_status`` adds ``status`` (N,): 0 complete; 1 / 2 the root search's status (``yield_scale``) at the step where
        the curve ended; 3 a degenerate direction or input; 4 ``eps_eq(a)`` zero or not finite.  One warning counts the
        curves that ended early.

        Offered for Hill / J2 / Drucker materials and ML yield functions with ``sdim = 6``; ``NotImplementedError`` for
        ``sdim = 3``, Tresca, Barlat, an SVR gradient (``ML_grad``) and texture materials."""
        if self.ML_yf:
            self._tex_refuse('flow_curve')
            self._bound_refuse('flow_curve')
        self._no_svr_gradient('flow_curve')
        if self.sy is None:
            raise ValueError('flow_curve: the material has no yield strength')
        if self.sdim != 6:
            raise NotImplementedError('flow_curve: not offered for sdim = 3 materials; the example integrates Voigt stresses')
        ml = bool(self.ML_yf)
        if not ml and (self.tresca or self.barlat):
            raise NotImplementedError('flow_curve: not offered for %s materials (Hill / J2 / Drucker and ML yield functions only)'
                                      % ('Tresca' if self.tresca else 'Barlat'))
        s = np.array(su, dtype=float)
        single = s.shape == (6,)
        if single:
            s = s[None, :]
        if s.ndim != 2 or s.shape[1] != 6:
            raise ValueError('Parameter "sig0" must be given as unit Voigt stress tensor.')
        n = len(s)
        seq = sig_eq_j2(s) if n else np.zeros(0)
        if np.any(np.isclose(seq, 0.0)) or not np.all(np.isfinite(seq)):
            raise ValueError('Parameter "sig0" has zero equivalent stress.')
        s = np.ascontiguousarray(s / seq[:, None])
        if epl0 is not None:
            e0 = np.asarray(epl0, dtype=float)
            if e0.shape == (6,):
                e0 = np.tile(e0, (n, 1))
            if e0.shape != (n, 6):
                raise ValueError('flow_curve: epl0 must be None, (6,) or (N,6) with one row per direction; got shape %s'
                                 % (np.shape(epl0),))
            epl0 = np.ascontiguousarray(e0)
        max_steps = int(max_steps)
        if max_steps < 0 or not (np.isfinite(depl) and depl > 0.) or not np.isfinite(predictor) or np.isnan(epl_max):
            raise ValueError('flow_curve: max_steps >= 0, a finite depl > 0, a finite predictor and an epl_max that is a '
                             'number expected')
        r = self._load(ana=not ml).flow_curve(0, s, epl0, max_steps=max_steps, depl=float(depl), epl_max=float(epl_max),
                                              predictor=float(predictor))
        ns, st = r['nsteps'], r['status']
        K = int(np.max(ns)) if n else 0
        bad = int(np.sum(st != 0))
        if bad:
            warnings.warn('flow_curve: %d of %d curve(s) ended early (no point of the yield locus found, or a flow direction '
                          'without length); NaN returned from there on' % (bad, n))
        x, epl = r['x'][:, :K + 1], r['epl'][:, :K + 1]
        sig = s[:, None, :] * x[:, :, None]
        out = dict(sig=sig, epl=epl, seq=sig_eq_j2(sig.reshape(-1, 6)).reshape(n, K + 1),
                   peeq=eps_eq(epl.reshape(-1, 6)).reshape(n, K + 1), yf=r['yf'][:, :K + 1], hk=r['hk'][:, :K], nsteps=ns)
        if return_status:
            out['status'] = st
        if single:
            out = {k: v[0] for k, v in out.items()}
        return out

    # ------------------------------------------------------------------ load paths of a material point
    @staticmethod
    def _path_control(control):
        """``control`` of load_path -- None, (6,) or (N,6) of bools -- as (None | (1,) | (N,) int32 bit masks, N or None)"""
        if control is None:
            return None, None
        m = np.asarray(control)
        if m.dtype.kind != 'b' or m.shape[-1:] != (6,) or m.ndim not in (1, 2):
            raise ValueError('load_path: control must be None, (6,) or (N, 6) of bools (True: the component of dload is a '
                             'stress increment); got dtype %s, shape %s' % (m.dtype, m.shape))
        bits = (m.reshape(-1, 6).astype(np.int32) << np.arange(6, dtype=np.int32)).sum(axis=1).astype(np.int32)
        return bits, (len(bits) if m.ndim == 2 else None)

    def load_path(self, dload, control=None, sig0=None, epl0=None, CV=None, maxit=50, newton=30, stol=None, eps_cap=0.05,
                  tex_id=None, return_tangent=False, khard0=None, form=None):
        """EXTENSION: material points driven along load paths, every path in one launch -- what the reference's
        ``examples/UMAT/calc_properties.py`` hands to a one-element block of an FE code: uniaxial and biaxial curves,
        r-values, plane-strain compression, cyclic paths.  ``dload`` is (K,N,6): K increments of N points, or (K,6), one path
        shared by the points, whose number then comes from ``sig0`` / ``epl0`` / ``tex_id`` / a 2-d ``control`` (else 1).
        ``control``: None (every component a strain increment), (6,) or (N,6) of bools; True makes that component of
        ``dload`` a stress increment.  The mask is constant along a path.  With S the strain- and F the stress-controlled
        components, the stress target is ``t_k[F] = t_{k-1}[F] + dload[k][F]`` with ``t_{-1} = sig0[F]`` -- ``np.cumsum``
        started at ``sig0`` has its bits.  One step, from ``(sig, epl)`` and the tangent ``Ct`` of the last accepted step
        (``CV`` before the first): ``deps[S] = dload[k][S]``; ``deps[F]`` solves ``Ct_FF deps_F = (t_k - sig)[F] - Ct_FS
        deps_S``; the trial is ``response(sig, epl, deps, CV, maxit)``, accepted when F is empty or ``max|sig'[F] - t_k[F]|
        <= stol`` (default ``1e-9 sy``); else ``deps[F] -= Ct'_FF^-1 (sig'[F] - t_k[F])`` and the trial is repeated from the
        same state, at most ``newton`` times.  Then ``sig = sig'``, ``epl += depl``, ``Ct = Ct'``.  No trial is evaluated on
        an increment that is not finite or has a component beyond ``eps_cap``: the path ends there.  An elastic material
        answers a trial with ``sig + CV deps``.

        Returns a dict, step-major: ``sig``, ``epl`` (K,N,6) the state after each step -- with strain control alone the bits
        of K ``response_batch`` calls with ``epl += depl`` in between --, ``deps`` (K,N,6) the increment taken, ``fy`` (K,N)
        and ``nsteps`` (K,N) of the accepted trial, ``newton`` (K,N) corrections taken, ``ksteps`` (N,) steps completed,
        ``status`` (N,): 0 complete, 1 ``stol`` not reached within ``newton`` corrections, 2 a pivot of the masked tangent
        zero or not finite, 3 ``deps`` not finite or beyond ``eps_cap``; with ``return_tangent`` also ``ct`` (N,6,6), the
        tangent after the last completed step.  Steps from ``ksteps`` on hold NaN (-1 in the int arrays).  A path that ends
        early is a result, not an error: its completed steps are those of the same path cut to ``ksteps`` steps.
        Neither ``khard`` nor ``msg`` is touched.

        Limit: full stress control across the yield point of a weakly hardening material ends with status 1 (the elastic
        tangent overshoots, the plastic one is nearly singular); drive at least one component by strain there.

        Work-hardening ML yield functions (``from_data`` on ``wh_data``): the hardening modulus, which every
        gradient evaluation overwrites, is state of a path like ``sig`` and ``epl``.  ``khard0``, a scalar or (N,), finite
        and ``>= 0``, is the modulus at the start of each path; it is required -- ``Material.khard`` is neither read nor
        written, the initial modulus is part of the initial state and not taken from the call history -- and counts towards
        the number of points like ``sig0``.  Every trial of a step enters with the step's modulus (``response`` with
        ``khard_in``); on acceptance the modulus is the accepted trial's, unchanged where that trial evaluated no gradient.
        The dict then also holds ``khard`` (K,N): the modulus after each step, NaN past ``ksteps``.  ``form``: ``'thread'``
        runs one thread per path -- with strain control the bits of the loop over ``response(khard_in=, return_khard=True)``
        --, ``'wave'`` one wave per path with the support-vector sums split over its 64 lanes (results differ from
        ``'thread'`` by the order of those sums, §45 has the measured size), ``'auto'`` (the default with ``khard0``) picks
        the faster one by N: the wave form at every N measured, 1 to 100 000 (§45).  ``khard0`` with any other material, ``form`` without ``khard0`` and an unknown ``form`` are ``ValueError``.

        Offered for elastic, Hill / J2 / Drucker (``sdim`` 6 and 3), Barlat with ``enable_barlat_normal``, 6-feature ML
        yield functions, materials bound to a texture and texture fields (``tex_id``: int or (N,)) included, and, with
        ``khard0``, work-hardening ML yield functions.
        ``NotImplementedError`` for ``sdim = 3`` ML yield functions, work-hardening ML yield functions without ``khard0``,
        ``ML_grad``, a parent texture material, Tresca and Barlat without a flow rule."""
        if getattr(self, '_bound', None) is None:
            self._tex_refuse('load_path')
        self._no_svr_gradient('load_path')
        if self.ML_yf and self.sdim != 6:
            raise NotImplementedError('load_path: not offered for sdim = 3 ML yield functions; only the 6-feature SVC runs on '
                                      'the row kernels that follow a path')
        wh = bool(self.ML_yf and getattr(self, 'whdat', False))
        if wh and khard0 is None:
            raise NotImplementedError('load_path: not offered for work-hardening ML yield functions, whose khard is carried '
                                      'from one gradient evaluation to the next, unless khard0 gives the hardening modulus '
                                      'at the start of the paths; flow_curve follows their hardening')
        if not self.ML_yf and self.sy is not None and (self.tresca or (self.barlat and not getattr(self, 'barlat_normal', False))):
            raise NotImplementedError('load_path: %s has no flow rule (calc_fgrad raises in the reference, material.py:822-825)%s'
                                      % ('Tresca' if self.tresca else 'Barlat',
                                         '' if self.tresca else '; enable_barlat_normal() gives Barlat one'))
        if khard0 is not None and not wh:
            raise ValueError('load_path: khard0 is the initial hardening modulus of a work-hardening ML yield function; the '
                             'modulus of this material is not state of a path')
        if form is not None and khard0 is None:
            raise ValueError('load_path: form selects the kernel of a work-hardening ML yield function and is accepted only '
                             'together with khard0')
        if khard0 is not None:
            form = 'auto' if form is None else form
            if form not in ('auto', 'thread', 'wave'):
                raise ValueError("load_path: form must be 'auto', 'thread' or 'wave'; got %r" % (form,))
            if tex_id is not None:
                raise ValueError('load_path: tex_id selects rows of a texture field; a work-hardening ML yield function has none')
        d = np.asarray(dload, dtype=float)
        if d.ndim not in (2, 3) or d.shape[-1] != 6:
            raise ValueError('load_path: dload must be (K, N, 6), or (K, 6) shared by the points; got shape %s' % (d.shape,))
        bits, nc = self._path_control(control)
        sizes = {}
        k0 = None
        if khard0 is not None:
            k0 = np.asarray(khard0, dtype=float)
            if k0.ndim > 1:
                raise ValueError('load_path: khard0 must be a scalar or (N,); got shape %s' % (k0.shape,))
            if not np.all(np.isfinite(k0)) or np.any(k0 < 0.):
                raise ValueError('load_path: khard0 must be finite and >= 0')
        if d.ndim == 3:
            sizes['dload'] = d.shape[1]
        if nc is not None:
            sizes['control'] = nc
        rows = {}
        for name, a in (('sig0', sig0), ('epl0', epl0)):
            if a is None:
                continue
            a = np.asarray(a, dtype=float)
            if a.shape[-1:] != (6,) or a.ndim not in (1, 2):
                raise ValueError('load_path: %s must be None, (6,) or (N, 6); got shape %s' % (name, a.shape))
            if a.ndim == 2:
                sizes[name] = len(a)
            rows[name] = a
        if tex_id is not None and np.ndim(tex_id) == 1:
            sizes['tex_id'] = len(tex_id)
        if k0 is not None and k0.ndim == 1:
            sizes['khard0'] = len(k0)
        if len(set(sizes.values())) > 1:
            raise ValueError('load_path: the number of points differs between the arguments: %s'
                             % ', '.join('%s %d' % kv for kv in sizes.items()))
        n = next(iter(sizes.values())) if sizes else 1
        tid = self._tex_ids(tex_id, n, 'load_path')
        s0, e0 = (None if name not in rows else np.ascontiguousarray(np.broadcast_to(rows[name], (n, 6)))
                  for name in ('sig0', 'epl0'))
        if bits is not None:
            bits = np.ascontiguousarray(np.broadcast_to(bits, (n,)))
        mixed = bits is not None and bool(np.any(bits))
        maxit, newton = int(maxit), int(newton)
        if maxit < 1:
            raise ValueError('load_path: maxit must be >= 1')
        if newton < 0:
            raise ValueError('load_path: newton must be >= 0')
        if stol is None:
            if self.sy is None and mixed:
                raise ValueError('load_path: stol must be given for a material without yield strength (the default is 1e-9 sy)')
            stol = 1.e-9 * self.sy if self.sy is not None else 1.
        stol, eps_cap = float(stol), float(eps_cap)
        if not (np.isfinite(stol) and stol > 0.):
            raise ValueError('load_path: stol must be finite and positive')
        if not (np.isfinite(eps_cap) and eps_cap > 0.):
            raise ValueError('load_path: eps_cap must be finite and positive')
        for name, a in (('dload', d), ('sig0', s0), ('epl0', e0)):
            if a is not None and not np.all(np.isfinite(a)):
                raise ValueError('load_path: %s must be finite' % name)
        if d.size:
            strain = np.ones((n, 6), dtype=bool) if bits is None else ((bits[:, None] >> np.arange(6)) & 1) == 0
            dd = np.abs(d) if d.ndim == 3 else np.abs(d)[:, None, :]
            if np.any((dd > eps_cap) & strain[None]):
                raise ValueError('load_path: a strain increment of dload is beyond eps_cap = %g' % eps_cap)
        if k0 is not None:
            return self._load(CV).load_path_wh(0, np.ascontiguousarray(d), np.ascontiguousarray(np.broadcast_to(k0, (n,))),
                                               control=bits if mixed else None, sig0=s0, epl0=e0, form=form, maxit=maxit,
                                               newton=newton, stol=stol, eps_cap=eps_cap, return_tangent=bool(return_tangent))
        return self._load(CV).load_path(0, np.ascontiguousarray(d), control=bits if mixed else None, sig0=s0, epl0=e0, tex_id=tid,
                                        maxit=maxit, newton=newton, stol=stol, eps_cap=eps_cap,
                                        return_tangent=bool(return_tangent))

    def data_curve(self, ilc, epl_crit=0.002, return_status=False):
        """What ``plot_lc`` of the reference's ``examples/train_hardening.py`` (lines 135-169; the "Reconstruct Stress-Strain
        Curve" block of ``Train_CPFEM/train_cpfem.py``) computes before it draws: the ML yield stress along training load
        case ``ilc`` at every plastic strain of its data.  The rows ``lc_indices[ilc] : lc_indices[ilc + 1]`` of
        ``msparam[0]`` with ``eps_eq(plastic_strain) >= epl_crit`` are kept; ``sig0`` is the last kept stress over its J2
        stress; the yield stresses are ONE ``yield_scale`` call along ``sig0`` with the kept plastic strains as ``epl`` rows
        and ``x0 = sy`` (the example runs one ``fsolve`` from ``sy`` per row).
        Returns a dict: ``peeq`` (Np,), ``seq_data`` (Np,) = ``sig_eq_j2`` of the kept stresses, ``seq_ml`` (Np,) =
        ``sig_eq_j2(sig_ml)``, ``sig_ml`` (Np,6) = ``sig0 * x``, ``sig0`` (6,), ``index`` the kept rows within ``msparam[0]``;
        ``return_status`` adds ``status`` (Np,) of ``yield_scale``."""
        if isinstance(ilc, bool) or not isinstance(ilc, (int, np.integer)):
            raise ValueError('Parameter "ilc" must be an integer number specifying the load case.')
        ms = getattr(self, 'msparam', None)
        if ms is None:
            raise AttributeError('data_curve: the material holds no data sets (msparam); from_data installs them')
        ms = ms[0]
        if 'lc_indices' not in ms:
            raise AttributeError('data_curve: the data set holds no load-case indices (lc_indices)')
        lci = np.asarray(ms['lc_indices'])
        istart, istop = int(lci[ilc]), int(lci[ilc + 1])
        sig_dat = np.asarray(ms['flow_stress'], dtype=float)[istart:istop, :]
        epl_dat = np.asarray(ms['plastic_strain'], dtype=float)[istart:istop, :]
        keep = np.nonzero(eps_eq(epl_dat) >= epl_crit)[0] if len(epl_dat) else np.zeros(0, dtype=int)
        if len(keep) == 0:
            raise ValueError('data_curve: load case %d holds no plastic strain of at least %g' % (ilc, epl_crit))
        sig_f, epl_f = sig_dat[keep], np.ascontiguousarray(epl_dat[keep])
        sig0 = sig_f[-1] / sig_eq_j2(sig_f[-1])
        x, st = self.yield_scale(np.tile(sig0, (len(keep), 1)), epl=epl_f, x0=float(self.sy), return_status=True)
        sig_ml = sig0[None, :] * x[:, None]
        out = dict(peeq=eps_eq(epl_f), seq_data=sig_eq_j2(sig_f), seq_ml=sig_eq_j2(sig_ml), sig_ml=sig_ml, sig0=sig0,
                   index=istart + keep)
        if return_status:
            out['status'] = st
        return out

    def _ray_x0(self, x0, shape, s, message=None):
        """Start values of a ray search: a scalar, or an array of `shape` (else ValueError(message % its shape)).  None: for
        the rays s of a texture material sy / seq_J2(s); with s None it stays None and the device forms
        get_sflow(epl) / seq_J2(su)."""
        if x0 is None:
            if s is None:
                return None
            with np.errstate(divide='ignore'):
                return np.broadcast_to(self.sy / sig_eq_j2(s), shape)
        x0 = np.asarray(x0, dtype=float)
        if x0.ndim == 0:
            return np.full(shape, float(x0))
        if x0.shape != shape:
            raise ValueError(message % (x0.shape,))
        return x0

    @staticmethod
    def _ray_result(name, noun, x, st, single=False, return_status=False):
        """The tail of a ray search: one warning that counts the rays without a root (status != 0, NaN in x), then x -- a
        float for a single ray -- with the status beside it on request"""
        bad = int(np.sum(st != 0))
        if bad:
            warnings.warn('%s: no point of the yield locus found along %d of %d %s(s); NaN returned there'
                          % (name, bad, st.size, noun))
        if single:
            x, st = float(x[0]), int(st[0])
        return (x, st) if return_status else x

    def _yield_scale_tex(self, s, single, tex, x0, return_status):
        """yield_scale of a texture material through plfx_tex_svc_yield_scale: one launch for a shared texture, one per
        distinct texture when every ray has its own"""
        if tex is None:
            raise ValueError("SVM is trained on texture data but no texture data was provided to this function.")
        if not self._is_tex():
            self._svc_refuse('yield_scale')
        n = len(s)
        t = self._tex_rows(tex, n, 'yield_scale')
        x0 = self._ray_x0(x0, (n,), s, 'yield_scale: x0 must be a scalar or of shape %s; got %%s' % ((n,),))
        ctx = self._load_tex()
        if len(t) == 1 or n == 1:
            x, st = ctx.tex_svc_yield_scale(s, t[:1], np.ascontiguousarray(x0[None, :]))
            x, st = x[0], st[0]
        else:   # one texture per ray: the rays grouped by texture, one launch per distinct texture
            ut, inv = np.unique(t, axis=0, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            x, st = np.empty(n), np.empty(n, dtype=np.int32)
            for k in range(len(ut)):
                sel = np.nonzero(inv == k)[0]
                xx, ss = ctx.tex_svc_yield_scale(s[sel], ut[k:k + 1], np.ascontiguousarray(x0[None, sel]))
                x[sel], st[sel] = xx[0], ss[0]
        return self._ray_result('yield_scale', 'direction', x, st, single, return_status)

    def texture_loci(self, tex=None, Na=72, return_status=False):
        """The yield loci that the reference's ``examples/Texture/train_texture.py`` computes before it draws them, one per
        texture: ``(theta, seq_yld)`` with ``theta = linspace(-pi, pi, Na)`` and ``seq_yld`` of shape (T, Na) -- along
        ``snorm = sig_cyl2princ([1, theta])`` (padded to six components) the root ``x`` of ``find_yloc(x, snorm, tex=tex_t)``,
        searched from ``x0 = sy / seq_J2(snorm)`` like ``yield_scale``, then ``sig_eq_j2(snorm * x)``.  ``tex`` (T, tdim),
        default: the textures of the data sets of ``from_data``, in order.  All T * Na rays are searched in ONE launch
        (the example solves one coupled ``fsolve`` per texture).  NaN where a ray has no root; ``return_status`` adds the
        (T, Na) status array of ``yield_scale``."""
        if not getattr(self, 'txdat', False):
            raise NotImplementedError('texture_loci: needs a texture material (from_data on data sets with tx_data)')
        if not self._is_tex():
            self._svc_refuse('texture_loci')
        if tex is None:
            tex = np.array([np.asarray(md['texture'], dtype=float) for md in self.msparam])
        t = np.asarray(tex, dtype=float)
        if t.ndim == 1:
            t = t[None, :]
        if t.ndim != 2 or t.shape[1] != self.tdim:
            raise ValueError('texture_loci: tex must be (T, %d); got shape %s' % (self.tdim, t.shape))
        theta = np.linspace(-np.pi, np.pi, Na)
        snorm = np.zeros((Na, 6))
        snorm[:, 0:3] = sig_cyl2princ(np.array([np.ones(Na), theta]).T)
        x0 = np.ascontiguousarray(self._ray_x0(None, (len(t), Na), snorm))
        x, st = self._load_tex().tex_svc_yield_scale(snorm, np.ascontiguousarray(t), x0)
        seq = np.full(x.shape, np.nan)
        ok = st == 0
        if np.any(ok):
            seq[ok] = sig_eq_j2((snorm[None, :, :] * x[:, :, None])[ok])
        self._ray_result('texture_loci', 'ray', seq, st)   # (the warning)
        return (theta, seq, st) if return_status else (theta, seq)

    def polar_yield_locus(self, Na=72, cmat=None, scaling=None, sJ2=False):
        """The curves that the reference's ``polar_plot_yl`` draws (material.py:3290-3309), as arrays: ``(theta, s_yld)``
        with ``theta = linspace(0, 2 pi, Na)`` and ``s_yld`` of shape (1 + len(cmat), Na) -- the equivalent stress of this
        material's yield locus along ``snorm = sig_cyl2princ([sy sqrt(1.5), theta])``, searched from ``x0 = 1``, then one row
        per material of ``cmat`` along the same directions.  Like the reference (:3308), the curves of ``cmat`` are put through
        THIS material's ``calc_seq`` (``sig_eq_j2`` with ``sJ2``), not their own.  ``scaling`` divides the stresses."""
        self._tex_refuse('polar_yield_locus')
        self._bound_refuse('polar_yield_locus')
        if self.sy is None:
            raise ValueError('polar_yield_locus: the material has no yield strength')
        sf = 1. if scaling is None else 1. / scaling
        theta = np.linspace(0., 2. * np.pi, Na)
        snorm = sig_cyl2princ(np.array([self.sy * np.ones(Na) * np.sqrt(1.5), theta]).T)
        rows = []
        for mat in [self] + list(cmat or []):
            sig = snorm * mat.yield_scale(snorm, x0=np.ones(Na))[:, None]
            ok = np.all(np.isfinite(sig), axis=1)
            seq = np.full(Na, np.nan)
            if np.any(ok):
                seq[ok] = sig_eq_j2(sig[ok]) if sJ2 else self.calc_seq(sig[ok])
            rows.append(seq * sf)
        return theta, np.array(rows)

    @staticmethod
    def _symmetrise(Z):
        """colour range of the reference's field plots (material.py:2817-2823, 3276-3282): the longer tail is cut"""
        Z = np.array(Z, dtype=float)
        zmin, zmax = np.amin(Z), np.amax(Z)
        if -zmin < zmax:
            Z[Z > -zmin] = -zmin
        else:
            Z[Z < -zmax] = -zmax
        return Z

    def polar_field(self, Np=100, predict=False):
        """The field that ``polar_plot_yl(field=True)`` draws under the yield locus (material.py:3261-3285), as arrays:
        ``(theta_grid, r_grid, Z)``, each (Np, Np) -- the decision function (``predict``: its sign as -1 / +1) of a 2-feature
        (sdim = 3) ML yield function on the feature grid [-1, 1] x [-1, 1], symmetrised like the reference's colour range, at
        the polar angles ``theta_grid`` and the equivalent stresses ``r_grid = (feature + 1) * scale_seq``."""
        if not self.ML_yf:
            raise AttributeError('polar_field: material has no trained ML yield function')
        if self.Ndof != 2:
            raise ValueError('"polar_plot_yl" currently does not support texture as degree of freedom for field plots.')
        xx, yy = np.meshgrid(np.linspace(-1., 1., Np), np.linspace(-1, 1., Np))
        feat = np.c_[yy.ravel(), xx.ravel()]
        sv = self.svc['sv']
        nsv = len(sv)
        ctx = _ctx()
        Z = ctx.svc_decision_batch(np.vstack((sv, feat)), [np.arange(nsv)], [self.svc['dual']], [self.svc['intercept']],
                                   [self.gam_yf], [nsv + np.arange(len(feat))])[0]
        if predict:
            Z = np.where(Z > 0., 1., -1.)
        return xx * np.pi, (yy + 1.) * self.scale_seq, self._symmetrise(Z).reshape(xx.shape)

    @staticmethod
    def ellipsis(a=1., b=1. / np.sqrt(3.), n=72):
        """Points (x, y) of an ellipse with its long half-axis ``a`` along the 45 degree line and short half-axis ``b``: the
        plane-stress yield locus of an isotropic J2 material in units of its yield strength (material.py:2772-2792)."""
        t = np.arange(0., 2.1 * np.pi, np.pi / n)
        return a * np.cos(t) - b * np.sin(t), a * np.cos(t) + b * np.sin(t)

    @staticmethod
    def _slice_stress(c1, c2, xa, ya):
        """principal stresses (N,3) of the points (xa, ya) of a slice with axis codes c1, c2 (material.py:2915-3008):
        0, 1, 2: sigma_1, sigma_2, sigma_3; 3: p = sigma_1 = sigma_2 on the first axis, sigma_3 on the second"""
        s = [None, None, None]
        if c1 == 3:
            s[0] = s[1] = xa
        elif c1 in (0, 1, 2):
            s[c1] = xa
        else:
            warnings.warn('yield_slices: axis1 not defined properly, set to sig_1: {}'.format(c1))
            s[0] = xa
        if c2 in (0, 1):
            s[c2] = ya
        elif c2 in (2, 3):
            s[2] = ya
        else:
            warnings.warn('yield_slices: axis2 not defined properly, set to sig_2: {}'.format(c2))
            s[1] = ya
        z = np.zeros(len(xa))
        return np.c_[tuple(z if v is None else v for v in s)]

    def yield_slices(self, axis1=[0], axis2=[1], peeq=0., xstart=None, xend=None, Nmesh=100, scaling=True, ref_mat=None,
                     iso=False, Na=180):
        """What the reference's ``plot_yield_locus`` draws (material.py:2835-3060), as arrays: one dict per slice
        ``(axis1[j], axis2[j])`` through the principal stress space (codes 0, 1, 2: sigma_1, sigma_2, sigma_3; 3:
        p = sigma_1 = sigma_2 against sigma_3) with

        * ``xx``, ``yy`` (Nmesh, Nmesh): the mesh, in units of ``sy`` with ``scaling``;
        * ``Z``: ``calc_yf(sig, epl=peeq, pred=True)`` on the mesh (``/ sy`` with ``scaling``) after the symmetrisation of
          ``plot_data`` (:2817-2824) -- what the reference contours at level 0;
        * ``Z_ref``: the same of ``ref_mat``, when given (not for slices with code 3, which the reference cannot draw with a
          reference material);
        * ``ellipsis``: ``(x, y)`` of the isotropic J2 locus with ``iso``;
        * ``locus`` (Na, 2): the zero contour itself, traced by ``yield_scale`` along ``Na`` in-plane rays from the origin at
          the angles ``linspace(0, 2 pi, Na)``; NaN rows where a ray meets no yield locus (hydrostatic rays of code 3).

        The caller's ``axis1`` / ``axis2`` lists are not modified (the reference rewrites code 3 in place)."""
        self._tex_refuse('yield_slices')
        self._bound_refuse('yield_slices')
        if self.sy is None:
            raise ValueError('yield_slices: the material has no yield strength')
        if len(axis1) != len(axis2):
            raise ValueError('Error in plot_yield_locus: mismatch in dimensions of ax1 and ax2')
        if xstart is None:
            xstart = -2. if scaling else -2. * self.sy
        if xend is None:
            xend = 2. if scaling else 2. * self.sy
        xx, yy = np.meshgrid(np.linspace(xstart, xend, Nmesh), np.linspace(xstart, xend, Nmesh))
        unit = self.sy if scaling else 1.    # stress per plot unit
        sf = 1. / unit
        phi = np.linspace(0., 2. * np.pi, Na)
        out = []
        for c1, c2 in zip(axis1, axis2):
            sig = self._slice_stress(c1, c2, xx.ravel(), yy.ravel()) * unit
            d = dict(axis1=c1, axis2=c2, xx=xx, yy=yy)
            d['Z'] = self._symmetrise(self.calc_yf(sig, epl=float(peeq), pred=True) * sf).reshape(xx.shape)
            if ref_mat is not None and c1 != 3:
                d['Z_ref'] = self._symmetrise(ref_mat.calc_yf(sig, epl=float(peeq), pred=True) * sf).reshape(xx.shape)
            if iso:
                x0, y0 = self.ellipsis()
                d['ellipsis'] = (x0, y0) if scaling else (x0 * self.sy, y0 * self.sy)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')     # axis codes were reported above; rays without a locus are NaN rows
                su = self._slice_stress(c1, c2, np.cos(phi), np.sin(phi)) * self.sy
                x = self.yield_scale(su, epl=float(peeq))
            d['locus'] = np.c_[np.cos(phi), np.sin(phi)] * (x * self.sy * sf)[:, None]
            out.append(d)
        return out

    # fields of Data.mat_data that the msparam branch of train_SVC reads
    _MSPARAM_KEYS = ('Nlc', 'sdim', 'wh_data', 'sy_av', 'peeq_max')

    def from_data(self, param):
        """Define the material from one data set of ``Data`` (material.py:2596-2680): ``param`` is ``Data.mat_data``
        (or a list holding one).  Sets msparam, Nset, whdat, epc, Ndof (6, or 15 with work-hardening data; 2 for
        sdim = 3) and ind_wh; elastic constants from ``elast_const`` (a warning when the data has none) and
        ``plasticity(sy=sy_av, sdim)``.  One or several data sets of ``Data(..., tx_data=True)`` make a texture material:
        ``txdat``, ``tdim``, ``ind_tx = 6`` and ``Ndof = 6 + tdim``, elasticity and ``sy`` from set 0 as in the reference.
        Refused: several data sets without texture data, texture together with work-hardening data (more features than the
        kernels take), texture with sdim = 3, more than 10 texture coefficients, work-hardening data with sdim = 3."""
        ms = list(param) if isinstance(param, (list, tuple, np.ndarray)) else [param]
        if len(ms) < 1:
            raise ValueError('from_data: no data set given')
        md = ms[0]
        if md.get('tx_descriptor') == 'VF':
            raise NotImplementedError('from_data: texture descriptor VF is not supported')
        if md.get('tx_data', False):
            return self._from_data_tex(ms)
        if len(ms) != 1:
            raise NotImplementedError('from_data: %d data sets need texture data (Data(..., tx_data=True)) to tell them '
                                      'apart; pass one Data.mat_data' % len(ms))
        sdim = md['sdim']
        if sdim not in (3, 6):
            raise ValueError('Value of sdim must be either 3 or 6')
        whdat = bool(md['wh_data'])
        if whdat and sdim == 3:
            raise NotImplementedError('from_data: work-hardening data with sdim = 3 (8 features) is not supported; '
                                      'no kernel evaluates those features')
        if self.sdim is not None and self.sdim != sdim:
            warnings.warn('from_data: Microstructure has changed definition of sdim. New value={}'.format(sdim))
        self.sdim = sdim
        self.msparam = np.array(ms, ndmin=1)
        self._msparam_from_data = self.msparam   # marker: train_SVC accepts this msparam
        self._tex_from_data = None
        self.Nset = 1
        self.whdat = whdat
        self.txdat = False
        self.tdim = None
        self.epc = md.get('epc')
        self.Ndof = 2 if sdim == 3 else 6
        if whdat:
            self.ind_wh = self.Ndof
            self.Ndof += sdim + 3
        if md.get('elast_const') is None:
            print('WARNING: No data on elastic properties in data.')
        else:
            self.elasticity(CV=md['elast_const'])
        self.plasticity(sy=md['sy_av'], sdim=sdim)
        self._version += 1

    def _from_data_tex(self, ms):
        """from_data for data sets with texture descriptors (material.py:2618-2681)"""
        md = ms[0]
        tdim = md.get('tdim')
        if not tdim:
            raise NotImplementedError('from_data: texture data without a descriptor (tdim); Data(json, tx_data=True, '
                                      "tx_descriptor='GSH_n') reads one")
        sdim = md['sdim']
        if sdim not in (3, 6):
            raise ValueError('Value of sdim must be either 3 or 6')
        if sdim == 3:
            raise NotImplementedError('from_data: texture data with sdim = 3; the reference trains texture on full Voigt '
                                      'stresses only (create_scaled_input asserts sdim == 6)')
        if md['wh_data']:
            raise NotImplementedError('from_data: texture together with work-hardening data (15 + tdim features) exceeds '
                                      'the 16 features of the training kernels; read the data with wh_data=False')
        if tdim > 10:
            raise NotImplementedError('from_data: %d texture coefficients; at most 10 (16 features) are supported' % tdim)
        for i, other in enumerate(ms[1:], 1):   # material.py:2652-2661
            if (other['Ntext'] != md['Ntext'] or other['sdim'] != sdim or other.get('tdim') != tdim
                    or not other.get('tx_data', False) or bool(other['wh_data'])):
                print('Error: Structure of data set #', i, ' is inconsistent:', md['Nlc'], md['Ntext'], sdim)
                raise ValueError('Inconsistent data structure')
        for other in ms:
            if np.shape(other.get('texture')) != (tdim,):
                raise ValueError('Inconsistent data structure')
        if self.sdim is not None and self.sdim != sdim:
            warnings.warn('from_data: Microstructure has changed definition of sdim. New value={}'.format(sdim))
        if getattr(self, 'tdim', None) not in (None, tdim):
            warnings.warn('from_data: Microstructure has changed definition of tdim. New value={}'.format(tdim))
        self.sdim = sdim
        self.msparam = np.array(ms, ndmin=1)
        self._msparam_from_data = self.msparam
        self._tex_from_data = self.msparam       # marker: the texture paths accept this msparam
        self.Nset = len(ms)
        self.whdat = False
        self.txdat = True
        self.tdim = int(tdim)
        self.epc = md.get('epc')
        self.Ndof = 6
        self.ind_tx = self.Ndof
        self.Ndof += self.tdim
        self.std_scaler = None
        if md.get('elast_const') is None:
            print('WARNING: No data on elastic properties in data.')
        else:
            self.elasticity(CV=md['elast_const'])
        self.plasticity(sy=md['sy_av'], sdim=sdim)
        self._version += 1

    def _msparam_ok(self):
        """True when msparam is one data set that from_data installed and that holds the fields training reads"""
        ms = getattr(self, 'msparam', None)
        if ms is None or getattr(self, '_msparam_from_data', None) is not ms:
            return False
        if self._is_tex():
            need = self._MSPARAM_KEYS + ('sig_ideal', 'texture')
            return all(isinstance(md, dict) and all(k in md for k in need) for md in ms)
        if len(ms) != 1:
            return False
        md = ms[0]
        need = self._MSPARAM_KEYS + (('flow_stress', 'plastic_strain') if md.get('wh_data') else ('sig_ideal',))
        return isinstance(md, dict) and all(k in md for k in need)

    def _svc_refuse(self, what):
        ms = getattr(self, 'msparam', None) is not None
        if ((ms and not self._msparam_ok()) or (getattr(self, 'txdat', False) and not self._is_tex())
                or (getattr(self, 'whdat', False) and not ms)):
            raise NotImplementedError('%s: training from this microstructure data (msparam / texture / work hardening) '
                                      'is not supported; train from mat_ref or sdata, or from one data set installed '
                                      'by from_data' % what)

    def _create_data_for_ms(self, Ce, Fe, Nseq, extend, idx_ms=0):
        """Training rows of one data set (material.py:1734-1820): row i + j Ndinp is flow stress i (``sig_ideal`` without
        work-hardening data) scaled by the j-th factor of create_sig_data, with its plastic strain in the columns
        ind_wh .. ind_wh + 5 and the three reversal columns zero.  Returns (Nlc, N0, xt, yt)."""
        md = self.msparam[idx_ms]
        Nlc = md['Nlc']
        if self.whdat:
            src = np.asarray(md['flow_stress'], dtype=float)
            Nlc -= md.get('Ncyl', 0)
        else:
            src = np.asarray(md['sig_ideal'], dtype=float)
        Ndinp = len(src)
        Nsdata = 2 * Nseq + 4 if extend else 2 * Nseq
        N0 = Nlc * Nsdata
        sig_train, yt = self.create_sig_data(sdata=src, Nseq=Nseq, Fe=Fe, Ce=Ce, extend=extend)
        xt = np.zeros((Ndinp * Nsdata, self.Ndof))
        xt[:, 0:self.sdim] = sig_train
        if self.whdat:
            if 'normalized_accumulated_strain' in md:
                raise NotImplementedError('train_SVC: data with strain reversals (normalized_accumulated_strain) '
                                          'is not supported')
            iw = self.ind_wh
            xt[:, iw:iw + self.sdim] = np.tile(np.asarray(md['plastic_strain'], dtype=float), (Nsdata, 1))
        if self._is_tex():   # material.py:1813-1817
            xt[:, self.ind_tx:] = np.asarray(md['texture'], dtype=float)
        return Nlc, N0, xt, yt

    def _svc_fit(self, X, y, C, gamma, gridsearch, cvals, gvals, dflt_c, dflt_g, metric):
        """fit the SVC on the GPU (with grid search: all candidates x 5 folds in one batched call, then the refit) and
        install it; returns (training score, fitted model)"""
        y = np.asarray(y, dtype=float)
        if np.any((y != 1.) & (y != -1.)):
            raise NotImplementedError('train_SVC: only binary labels -1 / +1 are supported (got %s)' % np.unique(y))
        if metric not in ('acc', 'mcc'):
            raise ValueError(f"{metric} must be acc or mcc")
        if not (C > 0 and gamma > 0):
            raise ValueError('train_SVC: C and gamma must be > 0 (got C=%r, gamma=%r)' % (C, gamma))
        ctx = _ctx()
        if gridsearch:
            from .training import param_grid, stratified_folds
            if cvals is None:   # the reference's default grid, extended by the given C and gamma
                cvals = list(dflt_c) + ([] if C in dflt_c else [C])
            if gvals is None:
                gvals = list(dflt_g) + ([] if gamma in dflt_g else [gamma])
            self.grid = svc_grid_search(ctx, X, y, param_grid(cvals, gvals), stratified_folds(y))
            print('The best hyperparameters are:', self.grid['best_params_'])
            C, gamma = self.grid['best_params_']['C'], self.grid['best_params_']['gamma']
        model = SVCModel.fit(ctx, X, y, C, gamma)
        self.svm_yf = model
        self.gam_yf, self.C_yf = gamma, C
        pred = model.predict(X)
        sc = 100. * float(np.mean(pred == y)) if metric == 'acc' else _mcc(y, pred)
        return sc, model

    def _svc_score(self, model, X, y, metric='acc'):
        if X is None:
            return None
        pred = model.predict(X)
        return 100. * float(np.mean(pred == np.asarray(y))) if metric == 'acc' else _mcc(np.asarray(y), pred)

    def setup_yf_SVM_6D(self, x, y_train, x_test=None, y_test=None, C=10., gamma=1., plot=False, gridsearch=False,
                        cvals=None, gvals=None, verbose=3, pca_dim=10, metric='acc'):
        """Train the SVC yield function on (N, 6) Voigt stresses scaled by sy (material.py:1109-1278) on the GPU;
        returns (train score, test score or None) for ``metric`` 'acc' (percent) or 'mcc'."""
        self._svc_refuse('setup_yf_SVM_6D')
        if plot:
            raise NotImplementedError('setup_yf_SVM_6D: plotting is not supported')
        if self.sdim != 6:
            raise ValueError('setup_yf_SVM_6D: material must have sdim=6')
        scale_wh = None
        if getattr(self, 'msparam', None) is None:
            self.scale_seq = self.sy
            self.Ndof, self.whdat = 6, False
        else:   # scaling from the data set (material.py:1160-1172); Nset = 1
            self.scale_seq = float(self.msparam[0]['sy_av'])
            scale_wh = float(self.msparam[0]['peeq_max']) if self.whdat else 1.
            self.scale_wh = scale_wh
        x = np.asarray(x, dtype=float)

        def feat(v):
            if not self.whdat:
                return self.create_scaled_input(v[:, 0:6])
            iw = self.ind_wh
            return self.create_scaled_input(v[:, 0:6], v[:, iw:iw + 6], v[:, iw + 6], v[:, iw + 7], v[:, iw + 8])
        X_train = feat(x)
        X_test = None if x_test is None else feat(np.asarray(x_test, dtype=float))
        train_sc, m = self._svc_fit(X_train, y_train, C, gamma, gridsearch, cvals, gvals,
                                    [1, 2, 4, 10], [0.5, 1, 1.5, 2, 2.5, 3], metric)
        self.set_svc(m.support_vectors_, m.dual_coef_[0], m.intercept_[0], m.gamma, self.scale_seq, dev_only=self.dev_only,
                     C=m.C, scale_wh=scale_wh if self.whdat else None)
        return train_sc, self._svc_score(m, X_test, y_test, metric)

    def setup_yf_SVM_3D(self, x, y_train, x_test=None, y_test=None, C=10., gamma=1., fs=0.1, plot=False, cyl=False,
                        gridsearch=False, cvals=None, gvals=None, pca_dim=10):
        """Train the 2-feature SVC yield function of sdim = 3 (material.py:1280-1440) on the GPU: features
        (seq_J2 / sy - 1, polar angle / pi) of principal (or, with ``cyl``, cylindrical) stresses, with the borders
        |theta/pi| > 1 - fs copied across the period; returns (train score, test score or None) in percent."""
        self._svc_refuse('setup_yf_SVM_3D')
        if plot:
            raise NotImplementedError('setup_yf_SVM_3D: plotting is not supported')
        if self.sdim != 3:
            raise ValueError('setup_yf_SVM_3D: material must have sdim=3')
        self.scale_seq = self.sy
        self.Ndof, self.whdat = 2, False

        def feat(v):
            v = np.asarray(v, dtype=float)
            X = np.zeros((len(v), 2))
            if not cyl:
                X[:, 0] = sig_eq_j2(v[:, 0:3]) / self.scale_seq - 1.
                X[:, 1] = sig_polar_ang(v[:, 0:3]) / np.pi
            else:
                X[:, 0] = v[:, 0] / self.scale_seq - 1.
                X[:, 1] = v[:, 1] / np.pi
            return X
        X_train, y_train = feat(x), np.asarray(y_train, dtype=float)
        indr = np.nonzero(X_train[:, 1] > 1. - fs)
        indl = np.nonzero(X_train[:, 1] < fs - 1.)
        Xr, Xl = X_train[indr], X_train[indl]
        Xr[:, 1] -= 2.
        Xl[:, 1] += 2.
        X_train = np.append(X_train, np.append(Xr, Xl, axis=0), axis=0)
        y_train = np.append(y_train, np.append(y_train[indr], y_train[indl], axis=0), axis=0)
        X_test = None if x_test is None else feat(x_test)
        train_sc, m = self._svc_fit(X_train, y_train, C, gamma, gridsearch, cvals, gvals,
                                    [2, 4, 6, 8, 10, 15], [1, 1.5, 2, 2.5, 3], 'acc')
        self.set_svc(m.support_vectors_, m.dual_coef_[0], m.intercept_[0], m.gamma, self.scale_seq, C=m.C)
        return train_sc, self._svc_score(m, X_test, y_test)

    def train_SVC(self, C=10, gamma=4, Nlc=36, Nseq=25, fs=0.3, extend=False, mat_ref=None, sdata=None, plot=False,
                  fontsize=16, gridsearch=False, cvals=None, gvals=None, Fe=0.1, Ce=0.99, scaler=None, pca=None,
                  train_index=None, test_index=None, verbose=1, metric='acc', pca_dim=10, reversal=None):
        """Train the SVC yield function (material.py:1442-1640, the branch without microstructure data): elasticity and
        plasticity from ``mat_ref`` (or sy = mean J2 stress of ``sdata``), training data from ``create_sig_data``, the fit
        by the batched SMO solver on the GPU (libsvm's C-SVC).  Returns (train score, test score)."""
        self._bound_refuse('train_SVC')
        self._svc_refuse('train_SVC')
        if scaler is not None or pca is not None:
            raise NotImplementedError('train_SVC: scaler / pca (a given scaler, the PCA of address-vector descriptors) are '
                                      'not supported; a texture material fits its own StdScaler')
        if (train_index is not None or test_index is not None) and not self._is_tex():
            raise NotImplementedError('train_SVC: train_index / test_index select data sets of a texture material '
                                      '(from_data on data sets with tx_data)')
        if plot:
            raise NotImplementedError('train_SVC: plotting is not supported')
        if reversal is not None:
            print('WARNING in "train_SVC": Parameter "reversal" is depracted and will be ignored.')
        if self._is_tex():
            return self._train_SVC_tex(C, gamma, Nseq, extend, Fe, Ce, gridsearch, cvals, gvals, train_index, test_index,
                                       metric, verbose)
        if getattr(self, 'msparam', None) is not None:   # one data set from from_data (material.py:1624-1636)
            Nlc, N0, xt, yt = self._create_data_for_ms(Ce=Ce, Fe=Fe, Nseq=Nseq, extend=extend)
        elif sdata is None:
            if mat_ref is None:
                raise ValueError('create_data_sig: Neither sdata nor mat_ref are provided, cannot generate training data')
            self.elasticity(CV=mat_ref.CV)
            self.plasticity(sy=mat_ref.sy, sdim=mat_ref.sdim)
            xt, yt = self.create_sig_data(N=Nlc, mat_ref=mat_ref, Nseq=Nseq, Fe=Fe, Ce=Ce, extend=extend)
            print('Training data created from reference material', mat_ref.name, ', with', Nlc, 'load cases.')
        else:
            sdata = np.asarray(sdata, dtype=float)
            self.plasticity(sy=np.mean(sig_eq_j2(sdata)), sdim=len(sdata[0, :]))
            xt, yt = self.create_sig_data(sdata=sdata, Nseq=Nseq, Fe=Fe, Ce=Ce, extend=extend)
            print('Training data created from {}-dimensional yield stresses with {} load cases.'.format(self.sdim, len(sdata)))
        if self.sdim == 3:
            train_sc, test_sc = self.setup_yf_SVM_3D(xt, yt, C=C, gamma=gamma, fs=0.3, gridsearch=gridsearch,
                                                     cvals=cvals, gvals=gvals)
        else:
            train_sc, test_sc = self.setup_yf_SVM_6D(xt, yt, C=C, gamma=gamma, gridsearch=gridsearch, cvals=cvals,
                                                     gvals=gvals, verbose=verbose, metric=metric)
        if not gridsearch:
            print(f"Training completed with score: {train_sc}")
        return train_sc, test_sc

    # ------------------------------------------------------------------ texture training
    def _tex_data(self, index, Ce, Fe, Nseq, extend):
        """unscaled training rows [stress | texture] and labels of the data sets `index`, stacked (material.py:1631-1640)"""
        xs, ys = [], []
        for i in index:
            _, _, xt, yt = self._create_data_for_ms(Ce=Ce, Fe=Fe, Nseq=Nseq, extend=extend, idx_ms=int(i))
            xs.append(xt)
            ys.append(yt)
        return np.concatenate(xs, axis=0), np.concatenate(ys, axis=0)

    def _tex_features(self, scaler, x):
        """create_scaled_input on unscaled rows: the deviator where dev_only, then the scaler (material.py:2347-2361)"""
        x = np.array(x, dtype=float)
        if self.dev_only:
            x[:, 0:6] = sig_dev(x[:, 0:6])
        return scaler.transform(x)

    @staticmethod
    def _score(y, dec, metric):
        pred = np.where(dec >= 0., 1., -1.)
        return 100. * float(np.mean(pred == y)) if metric == 'acc' else _mcc(y, pred)

    def _train_SVC_tex(self, C, gamma, Nseq, extend, Fe, Ce, gridsearch, cvals, gvals, train_index, test_index, metric,
                       verbose):
        """train_SVC of a texture material (material.py:1523-1593, 1624-1668, 1160-1258): rows of the data sets in
        ``train_index`` (default: all), a StdScaler fitted to the unscaled rows, the fit on the standardised ones;
        ``test_index`` names held-out sets for the test score.  ``gridsearch``: the reference's search over the textures --
        KFold(5, shuffle, random_state 42) over the data sets, a scaler per fold, the mean test score per candidate, the
        best by strict ``>`` in ParameterGrid order, then the refit on all sets -- with every fold x candidate fit in
        one batched device call."""
        if metric not in ('acc', 'mcc'):
            raise ValueError(f"{metric} must be acc or mcc")
        ctx = _ctx()
        kw = dict(Ce=Ce, Fe=Fe, Nseq=Nseq, extend=extend)
        if gridsearch:
            from .training import param_grid, texture_folds
            if cvals is None:
                cvals = [1, 5, 10, 20, 50] + ([] if C in (1, 5, 10, 20, 50) else [C])
            if gvals is None:
                gvals = [0.3, 0.5, 1, 5, 10] + ([] if gamma in (0.3, 0.5, 1, 5, 10) else [gamma])
            cand = param_grid(cvals, gvals)
            folds = texture_folds(self.Nset)
            # the shared X: per fold its training rows, then its held-out rows, both through the fold's own scaler
            blocks, ys, tr_rows, te_rows, off = [], [], [], [], 0
            for tr, te in folds:
                xtr, ytr = self._tex_data(tr, **kw)
                xte, yte = self._tex_data(te, **kw)
                sc = StdScaler(xtr)
                blocks += [self._tex_features(sc, xtr), self._tex_features(sc, xte)]
                ys += [ytr, yte]
                tr_rows.append(off + np.arange(len(ytr)))
                te_rows.append(off + len(ytr) + np.arange(len(yte)))
                off += len(ytr) + len(yte)
            X, y = np.concatenate(blocks, axis=0), np.concatenate(ys)
            probs = [tr_rows[k] for _ in cand for k in range(len(folds))]
            Cs = np.array([float(c) for c, _ in cand for _ in folds])
            gs = np.array([float(g) for _, g in cand for _ in folds])
            fits = ctx.svc_fit_batch(X, y, probs, Cs, gs)
            svl, coefs, icpt = [], [], []
            for k, r in enumerate(fits):
                rows = probs[k]
                yt = y[rows]
                order = np.concatenate([np.nonzero(yt < 0)[0], np.nonzero(yt > 0)[0]])
                sv = order[r['alpha'][order] > 0.]
                svl.append(rows[sv])
                coefs.append(yt[sv] * r['alpha'][sv])
                icpt.append(-r['rho'])
            nf = len(folds)
            q = [te_rows[k % nf] for k in range(len(fits))] + [tr_rows[k % nf] for k in range(len(fits))]
            dec = ctx.svc_decision_batch(X, svl + svl, coefs + coefs, icpt + icpt, np.concatenate((gs, gs)), q)
            test = np.array([self._score(y[q[k]], dec[k], metric) for k in range(len(fits))]).reshape(len(cand), nf)
            train = np.array([self._score(y[q[len(fits) + k]], dec[len(fits) + k], metric)
                              for k in range(len(fits))]).reshape(len(cand), nf)
            best, best_score = -1, 0
            for i in range(len(cand)):   # strict >, from 0 (material.py:1536, 1573)
                cv = np.mean(test[i])
                if cv > best_score:
                    best, best_score = i, cv
            self.grid = dict(params=[{'C': c, 'gamma': g} for c, g in cand], folds=[(tr, te) for tr, te in folds],
                             split_test_scores=test, split_train_scores=train, mean_test_score=test.mean(axis=1),
                             best_index_=best, best_params_=None if best < 0 else {'C': cand[best][0], 'gamma': cand[best][1]},
                             n_iter=np.array([r['n_iter'] for r in fits]).reshape(len(cand), nf))
            if best < 0:
                raise ValueError('train_SVC: no candidate of the grid search reached a mean test score above 0; the '
                                 'reference would refit with C = 0 and fail')
            C, gamma = cand[best]
            train_index = test_index = None   # the refit runs on all sets (material.py:1583-1586)
            print(80 * "+")
            print(f"Grid Search is finished :) \n Best HP: C={C}, gamma={gamma}")
            print(80 * "+")
        if not (C > 0 and gamma > 0):
            raise ValueError('train_SVC: C and gamma must be > 0 (got C=%r, gamma=%r)' % (C, gamma))
        if train_index is None:
            train_index = range(self.Nset)
        for i in list(train_index) + list(test_index if test_index is not None else []):
            if not 0 <= int(i) < self.Nset:
                raise IndexError('train_SVC: data set %r out of range (%d sets)' % (i, self.Nset))
        xt, yt = self._tex_data(train_index, **kw)
        if np.any((yt != 1.) & (yt != -1.)):
            raise NotImplementedError('train_SVC: only binary labels -1 / +1 are supported (got %s)' % np.unique(yt))
        print('Using {} full Voigt yield stresses for training.'.format(xt.shape))
        if self.dev_only:
            print('Only deviatoric part of stress tensors is considered.')
        self.gam_yf, self.C_yf = gamma, C
        self.scale_seq = sum(float(md['sy_av']) / self.Nset for md in self.msparam)   # not a feature scale (material.py:1164-1172)
        self.scale_wh = 1.
        self.std_scaler = StdScaler(xt)
        X_train = self._tex_features(self.std_scaler, xt)
        model = SVCModel.fit(ctx, X_train, yt, C, gamma)
        self.svm_yf = model
        self.svc = dict(sv=np.ascontiguousarray(model.support_vectors_), dual=np.ascontiguousarray(model.dual_coef_[0]),
                        intercept=float(model.intercept_[0]))
        self.ML_yf = True
        self._version += 1
        train_sc = self._score(yt, model.decision_function(X_train), metric)
        test_sc = None
        if test_index is not None:
            xte, yte = self._tex_data(test_index, **kw)
            test_sc = self._score(yte, model.decision_function(self._tex_features(self.std_scaler, xte)), metric)
        if not gridsearch:
            print(f"Training completed with score: {train_sc}")
        return train_sc, test_sc

    # ------------------------------------------------------------------ harness
    def calc_properties(self, size=2, Nel=2, verb=False, eps=0.005, min_step=None, sigeps=False,
                        load_cases=['stx', 'sty', 'et2', 'ect']):
        """Stress-strain curves of a 2x2 plane-stress model under four load cases
        (material.py:3062-3166); the harness of the reference's plasticity tests."""
        from .model import Model
        self._tex_refuse('calc_properties')
        self._bound_refuse('calc_properties')
        self._no_svr_gradient('calc_properties')

        def calc_strength(vbc1, nbc1, vbc2, nbc2, sel):
            fe = Model(dim=2, planestress=True)
            fe.geom([size], LY=size)
            fe.assign([self])
            fe.bcleft(0.)
            fe.bcbot(0.)
            fe.bcright(vbc1, nbc1)
            fe.bctop(vbc2, nbc2)
            fe.mesh(NX=Nel, NY=Nel)
            fe.solve(verb=verb, min_step=min_step)
            seq = self.calc_seq(fe.sgl)
            eeq = eps_eq(fe.egl)
            peeq = eps_eq(fe.epgl)
            iys = np.nonzero(peeq < 1.e-2)
            self.prop[sel].update(ys=seq[iys[0][-1]], seq=seq, eeq=eeq, peeq=peeq)
            seq = sig_eq_j2(fe.sgl)
            iys = np.nonzero(peeq < 1.e-6)
            self.propJ2[sel].update(ys=seq[iys[0][-1]], seq=seq, eeq=eeq, peeq=peeq)
            if sigeps:
                self.sigeps[sel].update(sig=fe.sgl, eps=fe.egl, epl=fe.epgl)

        cases = {'stx': (eps * size, 'disp', 0., 'force', '-r', 'uniax-x'),
                 'sty': (0., 'force', eps * size, 'disp', '-b', 'uniax-y'),
                 'et2': (0.4 * eps * size, 'disp', 0.4 * eps * size, 'disp', '-k', 'equibiax'),
                 'ect': (-0.8 * eps * size, 'disp', 0.8 * eps * size, 'disp', '-m', 'shear')}
        for case in load_cases:
            if case not in cases:
                warnings.warn('calc_properties: Load case not supported: {}'.format(case))
                continue
            v1, n1, v2, n2, style, label = cases[case]
            calc_strength(v1, n1, v2, n2, case)
            self.prop[case]['style'] = style
            self.prop[case]['name'] = label


def _mcc(a, b):
    from .training import _mcc as m
    return m(a, b)


class SVCModel(object):
    """A fitted binary RBF C-SVC in scikit-learn's layout (``support_``, ``support_vectors_``, ``dual_coef_`` (1, nSV),
    ``intercept_`` (1,), ``n_iter_`` (1,), ``n_support_``, ``C``, ``gamma``): what ``Material.svm_yf`` holds after
    ``train_SVC``.  Fitted and evaluated on the GPU (plfx_svc_fit_batch / plfx_svc_decision_batch)."""

    def __init__(self, ctx, X, y, C, gamma, alpha, rho, n_iter, status, obj):
        X = np.asarray(X, dtype=float)
        y = np.asarray(y, dtype=float)
        order = np.concatenate([np.nonzero(y < 0)[0], np.nonzero(y > 0)[0]])   # libsvm's order: class -1 first
        sv = order[alpha[order] > 0.]
        self._ctx = ctx
        self.C, self.gamma, self._gamma = float(C), float(gamma), float(gamma)
        self.classes_ = np.array([-1., 1.])
        self.support_ = sv.astype(np.int32)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = (y[sv] * alpha[sv])[None, :]
        self.intercept_ = np.array([-rho])
        self.n_support_ = np.array([np.sum(y[sv] < 0), np.sum(y[sv] > 0)], dtype=np.int32)
        self.n_iter_ = np.array([n_iter], dtype=np.int32)
        self.fit_status_ = int(status)
        self.dual_objective_ = float(obj)
        if status:
            warnings.warn('Solver terminated early (max_iter=%d).  Consider pre-processing your data with '
                          'StandardScaler or MinMaxScaler.' % n_iter)

    # rows from which a single fit runs on the many-workgroup solver (plfx_svc_fit_wide) instead of one workgroup; the
    # crossover measured with tools/svc_data_train_bench.py.  Both give the same fit bit for bit.
    WIDE_MIN_ROWS = 4096

    @classmethod
    def fit(cls, ctx, X, y, C, gamma, tol=1e-3, max_iter=-1):
        if len(y) >= cls.WIDE_MIN_ROWS:
            r = ctx.svc_fit_wide(X, y, C, gamma, tol=tol, max_iter=max_iter)
        else:
            r = ctx.svc_fit_batch(X, y, [np.arange(len(y))], C, gamma, tol=tol, max_iter=max_iter)[0]
        return cls(ctx, X, y, C, gamma, r['alpha'], r['rho'], r['n_iter'], r['status'], r['obj'])

    def decision_function(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=float))
        Xa = np.concatenate([self.support_vectors_, X])
        nsv = len(self.support_vectors_)
        return self._ctx.svc_decision_batch(Xa, [np.arange(nsv)], [self.dual_coef_[0]], [self.intercept_[0]], [self.gamma],
                                            [nsv + np.arange(len(X))])[0]

    def predict(self, X):
        """labels as libsvm assigns them: decision >= 0 -> +1"""
        return np.where(self.decision_function(X) >= 0., 1., -1.)

    def score(self, X, y):
        return float(np.mean(self.predict(X) == np.asarray(y)))


class StdScaler(object):
    """scikit-learn's ``StandardScaler`` arithmetic (``mean_``, ``var_``, ``scale_``, ``transform``,
    ``inverse_transform``): population standard deviation per column; a column whose variance is zero (within
    rounding: var <= n eps var + (n mean eps)^2, scikit-learn's test for a constant feature) gets scale 1."""

    def __init__(self, X):
        X = np.asarray(X, dtype=float)
        n = len(X)
        self.n_samples_seen_ = n
        self.mean_ = np.mean(X, axis=0)
        self.var_ = np.var(X, axis=0)
        fe = np.finfo(np.float64).eps
        const = self.var_ <= n * fe * self.var_ + (n * self.mean_ * fe) ** 2
        self.scale_ = np.where(const, 1., np.sqrt(self.var_))

    def transform(self, X):
        return (np.asarray(X, dtype=float) - self.mean_) / self.scale_

    def inverse_transform(self, X):
        return np.asarray(X, dtype=float) * self.scale_ + self.mean_


class SVRModel(object):
    """A fitted RBF epsilon-SVR in scikit-learn's layout (``support_``, ``support_vectors_``, ``dual_coef_`` (1, nSV),
    ``intercept_`` (1,), ``n_iter_`` (1,), ``C``, ``gamma``, ``epsilon``): what ``Material.svm_grad0`` .. ``svm_khard``
    hold after ``setup_fgrad_SVM``.  ``coef_`` holds alpha - alpha* of every training row.  Fitted by plfx_svr_fit_batch and
    evaluated by plfx_svr_predict_multi."""

    def __init__(self, ctx, X, fit, C, gamma, epsilon):
        self._ctx, self._X = ctx, X
        self.C, self.gamma, self._gamma, self.epsilon = float(C), float(gamma), float(gamma), float(epsilon)
        self.coef_ = np.array(fit['coef'])
        self.support_ = np.nonzero(np.abs(self.coef_) > 0.)[0].astype(np.int32)
        self.support_vectors_ = X[self.support_]
        self.dual_coef_ = self.coef_[self.support_][None, :]
        self.intercept_ = np.array([-fit['rho']])
        self.n_iter_ = np.array([fit['n_iter']], dtype=np.int32)
        self.fit_status_ = int(fit['status'])
        self.dual_objective_ = float(fit['obj'])
        if self.fit_status_:
            warnings.warn('Solver terminated early (max_iter=%d).  Consider pre-processing your data with '
                          'StandardScaler or MinMaxScaler.' % fit['n_iter'])

    def predict(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=float))
        return self._ctx.svr_predict_multi(self._X, self.coef_[:, None], self.intercept_, self.gamma, X)[:, 0]


def svc_grid_search(ctx, X, y, candidates, folds):
    """Cross-validated grid search in ONE batched device call: every (C, gamma) candidate on every fold (train on the
    other folds), then every fitted model on its held-out fold.  Returns dict(params, mean_test_score (mean fold
    accuracy per candidate), split_test_scores, best_index_, best_params_); the best candidate is the first one with the
    highest mean accuracy (GridSearchCV's rule)."""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n = len(y)
    trains = [np.setdiff1d(np.arange(n), f) for f in folds]
    probs, Cs, gs = [], [], []
    for c, g in candidates:
        for tr in trains:
            probs.append(tr)
            Cs.append(float(c))
            gs.append(float(g))
    fits = ctx.svc_fit_batch(X, y, probs, np.array(Cs), np.array(gs))
    sv_lists, coefs, icpt, qlists = [], [], [], []
    for k, r in enumerate(fits):
        tr = probs[k]
        yt = y[tr]
        order = np.concatenate([np.nonzero(yt < 0)[0], np.nonzero(yt > 0)[0]])
        sv = order[r['alpha'][order] > 0.]
        sv_lists.append(tr[sv])
        coefs.append(yt[sv] * r['alpha'][sv])
        icpt.append(-r['rho'])
        qlists.append(folds[k % len(folds)])
    dec = ctx.svc_decision_batch(X, sv_lists, coefs, icpt, np.array(gs), qlists)
    nf = len(folds)
    split = np.array([float(np.mean(np.where(dec[k] >= 0., 1., -1.) == y[qlists[k]])) for k in range(len(fits))])
    split = split.reshape(len(candidates), nf)
    mean = np.array([np.average(s) for s in split])
    best = int(np.flatnonzero(mean == mean.max())[0])
    return dict(params=[{'C': c, 'gamma': g} for c, g in candidates], mean_test_score=mean, split_test_scores=split,
                n_iter=np.array([r['n_iter'] for r in fits]).reshape(len(candidates), nf),
                best_index_=best, best_params_={'C': candidates[best][0], 'gamma': candidates[best][1]})
