"""ctypes binding of libplfx.so (the C-ABI declared in include/plfx.h).

There is deliberately NO CPU fallback: if the HIP library is missing or no MI355X is visible,
every entry point raises.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C pylabfea_amd/csrc``).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PLFX_LIB', os.path.join(_HERE, 'libplfx.so'))  # PLFX_LIB: kernel-variant experiments

# yield-function kinds (include/plfx.h)
ELASTIC, HILL6, PRINC3, SVC6, TRESCA, BARLAT, SVC3, SVC_WH, SVC6_COLS = 0, 1, 2, 3, 4, 5, 6, 7, 8

# state ids of plfx_state_get/_set
ST_SIG, ST_EPS, ST_EPL, ST_RES_SIG, ST_RES_DEPL, ST_ELSTIFF, ST_U, ST_F, ST_DU, ST_FYN, ST_MAXSTEPS, ST_KHARD = range(12)

# selectors of plfx_element_fields (PLFX_FIELD_* of include/plfx.h), in the order of their values
FIELD_NAMES = ('strain1', 'strain2', 'strain12', 'stress1', 'stress2', 'stress12', 'plastic1', 'plastic2', 'plastic12',
               'seq', 'seqJ2', 'peeq', 'etot', 'ux', 'uy')
FIELD_ID = {n: i for i, n in enumerate(FIELD_NAMES)}

# timing families
T_SWEEP, T_SPMV, T_CGUPD, T_ASSEMBLE, T_VCYCLE, T_SMOOTH, T_SWEEP_HEAVY, T_COMM = range(8)


class PlfxError(RuntimeError):
    pass


class CMaterial(C.Structure):
    _fields_ = [('kind', C.c_int32), ('sdim', C.c_int32), ('CV', C.c_double * 36),
                ('E', C.c_double), ('nu', C.c_double), ('sy', C.c_double), ('khard', C.c_double),
                ('hill', C.c_double * 6), ('drucker', C.c_double), ('nsv', C.c_int32),
                ('nfeat', C.c_int32), ('dev_only', C.c_int32), ('_pad', C.c_int32),
                ('gamma', C.c_double), ('intercept', C.c_double), ('scale_seq', C.c_double),
                ('sv', C.c_void_p), ('dual', C.c_void_p), ('barlat', C.c_double * 18),
                ('barlat_exp', C.c_double), ('barlat_normal', C.c_int32), ('_pad2', C.c_int32),
                ('scale_wh', C.c_double)]


# every symbol include/plfx.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = [
    'plfx_create', 'plfx_destroy', 'plfx_last_error', 'plfx_version', 'plfx_device_count', 'plfx_device_info',
    'plfx_stream', 'plfx_sync', 'plfx_set_materials', 'plfx_seq_batch', 'plfx_fgrad_batch',
    'plfx_yf_batch', 'plfx_full_yf_batch', 'plfx_response_batch', 'plfx_set_mesh', 'plfx_get_bmat',
    'plfx_get_kel', 'plfx_state_get', 'plfx_state_set', 'plfx_state_reset', 'plfx_gather',
    'plfx_assemble', 'plfx_get_csr', 'plfx_apply_bc', 'plfx_solve', 'plfx_sweep', 'plfx_scf_stats',
    'plfx_update_state', 'plfx_global_sums', 'plfx_comm_unique_id', 'plfx_comm_init',
    'plfx_timing_get', 'plfx_timing_reset', 'plfx_timing_enable', 'plfx_set_grid', 'plfx_set_precond',
    'plfx_precond_info', 'plfx_set_operator', 'plfx_operator_info', 'plfx_gen_structured', 'plfx_reuse_info', 'plfx_timing_select', 'plfx_finish_fetch', 'plfx_sweep_info', 'plfx_matvec', 'plfx_set_bc_plan', 'plfx_apply_bc_plan',
    'plfx_set_finish_set', 'plfx_finish_step', 'plfx_scf_all', 'plfx_comm_info', 'plfx_comm_init_callback',
    'plfx_set_bc_sources',
    'plfx_load_step', 'plfx_set_strip', 'plfx_strip_info', 'plfx_allreduce_host',
    'plfx_response_batch_kh', 'plfx_fgrad_batch_wh', 'plfx_timing_sample', 'plfx_solve_fallbacks', 'plfx_comm_selftest',
    'plfx_indefinite_info', 'plfx_pattern_selftest', 'plfx_precond_bench', 'plfx_set_wh_mode', 'plfx_wh_info', 'plfx_wh_carry', 'plfx_set_mesh_structured',
    'plfx_svc_info', 'plfx_fgrad_seq_batch', 'plfx_precond_apply', 'plfx_predict_info',
    'plfx_set_response_maxit', 'plfx_sig_princ_host', 'plfx_eig3_host',
    'plfx_svc_fit_batch', 'plfx_svc_decision_batch', 'plfx_svc_fit_wide', 'plfx_hessian_batch',
    'plfx_svr_fit_batch', 'plfx_svr_predict_multi', 'plfx_set_svr_flow', 'plfx_svr_flow_info',
    'plfx_sweep_launch_info', 'plfx_element_fields', 'plfx_bc_info', 'plfx_yield_scale',
    'plfx_committee_yf', 'plfx_committee_info',
    'plfx_tex_svc_set', 'plfx_tex_svc_yf', 'plfx_tex_svc_yield_scale', 'plfx_tex_svc_info',
    'plfx_tex_svc_fgrad', 'plfx_tex_svc_full_yf', 'plfx_tex_svc_response', 'plfx_tex_svc_flow_info',
    'plfx_flow_curve', 'plfx_flow_info', 'plfx_load_path', 'plfx_load_path_info',
    'plfx_load_path_wh', 'plfx_load_path_wh_info',
    'plfx_dead_store_info', 'plfx_plane_info', 'plfx_short_info', 'plfx_snap_info', 'plfx_code_info', 'plfx_code_get',
    'plfx_set_svc_cols', 'plfx_mg_info',
    'plfx_set_svc_textures', 'plfx_set_element_textures', 'plfx_response_batch_tid', 'plfx_full_yf_batch_tid',
    'plfx_svc_textures_info',
]

_lib = None


def load():
    """dlopen libplfx.so; raises PlfxError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PlfxError('libplfx.so not found at %s - build it first (__graft_entry__.build()); '
                        'pylabfea_amd has no CPU fallback' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.plfx_last_error.restype = C.c_char_p
    lib.plfx_version.restype = C.c_char_p
    lib.plfx_stream.restype = C.c_void_p
    lib.plfx_destroy.restype = None
    _lib = lib
    return lib


class CStep(C.Structure):
    """plfx_step of include/plfx.h: one load step of Model.solve"""
    _fields_ = [('il', C.c_int32), ('nonlin', C.c_int32), ('has_nodeset', C.c_int32), ('warm', C.c_int32),
                ('maxit', C.c_int32), ('defer_slot', C.c_int32), ('rtol', C.c_double),
                ('bcl0', C.c_double * 2), ('bcb0', C.c_double * 2),
                ('max_dbcr', C.c_double * 2), ('max_dbct', C.c_double * 2), ('max_dbcn', C.c_double * 2),
                ('bcr', C.c_double * 2), ('bct', C.c_double * 2), ('bcn', C.c_double * 2),
                ('bcr0', C.c_double * 2), ('bct0', C.c_double * 2), ('bcn0', C.c_double * 2),
                ('sld', C.c_double * 6),
                ('dbcr', C.c_double * 2), ('dbct', C.c_double * 2), ('dbcn', C.c_double * 2),
                ('scale_bc', C.c_double),
                ('nit', C.c_int32), ('nconv', C.c_int32), ('nsweeps', C.c_int32), ('nsolves', C.c_int32),
                ('soft_fail', C.c_int32), ('inconsistent_entry', C.c_int32),
                ('its', C.c_int32 * 40), ('relres', C.c_double * 40)]


def device_count():
    """GPUs visible to this process (plfx_device_count; 0 without a GPU)"""
    return int(load().plfx_device_count())


def _dp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def gen_structured(NX, NY):
    """(conn[Nel,4], noleft, noright, nobot, notop) of the reference's structured grid from the library's own index
    generator (plfx_gen_structured; host-only, works without a GPU)"""
    lib = load()
    conn = np.empty((NX * NY, 4), dtype=np.int32)
    le, ri = np.empty(NY + 1, dtype=np.int32), np.empty(NY + 1, dtype=np.int32)
    bo, to = np.empty(NX + 1, dtype=np.int32), np.empty(NX + 1, dtype=np.int32)
    rc = lib.plfx_gen_structured(int(NX), int(NY), _dp(conn), _dp(le), _dp(ri), _dp(bo), _dp(to))
    if rc:
        raise PlfxError('plfx_gen_structured(%d, %d): error %d' % (NX, NY, rc))
    return conn, le, ri, bo, to


def sig_princ_host(sig):
    """basic.sig_princ's principal stresses (reference order) of (N,6) Voigt stresses from the library's host-side LAPACK replay"""
    lib = load()
    s = _f64(sig).reshape(-1, 6)
    sp = np.empty((len(s), 3))
    rc = lib.plfx_sig_princ_host(len(s), _dp(s), _dp(sp))
    if rc < 0:
        raise PlfxError('plfx_sig_princ_host: error %d' % rc)
    return sp


def eig3_host(sig):
    """(w[N,3], V[N,3,3]): eigenvalues in LAPACK dgeev's order and unit eigenvectors (columns) of the symmetric stress tensors"""
    lib = load()
    s = _f64(sig).reshape(-1, 6)
    w, V = np.empty((len(s), 3)), np.empty((len(s), 3, 3))
    rc = lib.plfx_eig3_host(len(s), _dp(s), _dp(w), _dp(V))
    if rc < 0:
        raise PlfxError('plfx_eig3_host: error %d' % rc)
    return w, V


def pack_material(kind, CV, E=0., nu=0., sy=0., khard=0., hill=None, drucker=0., svc=None, barlat=None,
                  barlat_exp=0., barlat_normal=False):
    """Build a plfx_material record.  svc = dict(sv, dual, gamma, intercept, scale_seq, dev_only); a SVC6_COLS record adds
    scale_cols, its six column scales, and for a texture field coef, the (T, nsv) coefficient rows.  Returns
    (struct, keepalive) - keepalive holds the arrays the struct points to (and, as its third entry, the column scales and,
    as its fourth, the coefficient rows that Context.set_materials sends after the record)."""
    m = CMaterial()
    m.kind = int(kind)
    m.sdim = 3 if kind in (PRINC3, SVC3) else 6
    if barlat is not None:
        for i in range(18):
            m.barlat[i] = float(barlat[i])
        m.barlat_exp = float(barlat_exp)
        m.barlat_normal = int(bool(barlat_normal))
    cv = _f64(CV).reshape(36)
    for i in range(36):
        m.CV[i] = cv[i]
    m.E, m.nu = float(E), float(nu)
    m.sy = 0. if sy is None else float(sy)
    m.khard = 0. if khard is None else float(khard)
    h = np.ones(6) if hill is None else np.asarray(hill, dtype=float)
    for i in range(6):
        m.hill[i] = h[i] if i < len(h) else 1.
    m.drucker = float(drucker or 0.)
    keep = []
    if svc is not None:
        sv = _f64(svc['sv'])
        dual = _f64(svc['dual']).reshape(-1)
        keep = [sv, dual]
        m.nsv, m.nfeat = sv.shape
        m.dev_only = int(bool(svc.get('dev_only', False)))
        m.gamma = float(svc['gamma'])
        m.intercept = float(svc['intercept'])
        m.scale_seq = float(svc['scale_seq'])
        m.scale_wh = float(svc.get('scale_wh', 1.) or 1.)
        m.sv = sv.ctypes.data
        m.dual = dual.ctypes.data
        if kind == SVC6_COLS:
            cols = _f64(svc['scale_cols']).reshape(-1)
            if cols.shape != (6,):
                raise ValueError('pack_material: a SVC6_COLS record needs six column scales (scale_cols)')
            keep.append(cols)
            if svc.get('coef') is not None:
                coef = _f64(svc['coef'])
                if coef.ndim != 2 or coef.shape[1] != m.nsv or len(coef) < 1:
                    raise ValueError('pack_material: the coefficient rows of a texture field must be (T, nsv) with T >= 1')
                keep.append(coef)
    return m, keep


class Context(object):
    """One libplfx context = one GPU + one HIP stream.  Thin, typed wrapper over the C-ABI."""

    def __init__(self, device=0):
        self.lib = load()
        self.h = C.c_void_p()
        rc = self.lib.plfx_create(int(device), C.byref(self.h))
        if rc != 0:
            msg = self.lib.plfx_last_error(self.h).decode() if self.h else 'plfx_create failed'
            if self.h:
                self.lib.plfx_destroy(self.h)
                self.h = C.c_void_p()
            raise PlfxError('libplfx: %s' % msg)
        self.nmat = 0
        self.nel = 0
        self.nel_owned = 0
        self.ndof = 0
        self._keep = []

    def close(self):
        if getattr(self, 'h', None):
            self.lib.plfx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, soft=False):
        if rc < 0 or (rc > 0 and not soft):
            raise PlfxError('libplfx error %d: %s' % (rc, self.lib.plfx_last_error(self.h).decode()))
        return rc

    # -- info
    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int()
        hbm = C.c_int64()
        self._chk(self.lib.plfx_device_info(self.h, name, 256, C.byref(cus), C.byref(hbm)))
        return name.value.decode(), cus.value, hbm.value

    def stream(self):
        return self.lib.plfx_stream(self.h)

    def sync(self):
        self._chk(self.lib.plfx_sync(self.h))

    # -- materials
    def set_materials(self, records):
        """records: list of (CMaterial, keepalive)"""
        arr = (CMaterial * len(records))()
        self._keep = []
        for i, (m, keep) in enumerate(records):
            arr[i] = m
            self._keep.append(keep)
        self._chk(self.lib.plfx_set_materials(self.h, len(records), arr))
        self.nmat = len(records)
        for i, (m, keep) in enumerate(records):   # the column scales of SVC6_COLS records (pack_material)
            if m.kind == SVC6_COLS:
                self.set_svc_cols(i, keep[2])
                if len(keep) > 3:   # ... and the coefficient rows of a texture field
                    self.set_svc_textures(i, keep[3])

    def set_svc_cols(self, mat, scale):
        """the six column scales of the SVC6_COLS material ``mat`` (plfx_set_svc_cols); they hold until the next set_materials"""
        sc = _f64(scale).reshape(-1)
        if sc.shape != (6,):
            raise ValueError('set_svc_cols: six scales expected')
        self._chk(self.lib.plfx_set_svc_cols(self.h, int(mat), _dp(sc)))

    def set_svc_textures(self, mat, coef):
        """the coefficient rows (T, nsv) of a texture field on the SVC6_COLS material ``mat`` (plfx_set_svc_textures); None
        detaches; they hold until the next set_materials"""
        if coef is None:
            self._chk(self.lib.plfx_set_svc_textures(self.h, int(mat), 0, None))
            return
        co = _f64(coef)
        if co.ndim != 2:
            raise ValueError('set_svc_textures: coefficient rows (T, nsv) expected')
        self._chk(self.lib.plfx_set_svc_textures(self.h, int(mat), len(co), _dp(co)))

    def set_element_textures(self, tex_id):
        """the texture row of every owned element, (nel,) int (plfx_set_element_textures); None: every element has row 0"""
        if tex_id is None:
            self._chk(self.lib.plfx_set_element_textures(self.h, None))
            return
        ids = _i32(tex_id).reshape(-1)
        if len(ids) != self.nel_owned:
            raise ValueError('set_element_textures: one row index per element expected (%d); got %d' % (self.nel_owned, len(ids)))
        self._chk(self.lib.plfx_set_element_textures(self.h, _dp(ids)))

    def svc_textures_info(self, mat):
        """dict(rows, staged, launches) of the texture field on material ``mat`` (plfx_svc_textures_info)"""
        rows, staged, nl = C.c_int(), C.c_int(), C.c_int64()
        self._chk(self.lib.plfx_svc_textures_info(self.h, int(mat), C.byref(rows), C.byref(staged), C.byref(nl)))
        return dict(rows=int(rows.value), staged=bool(staged.value), launches=int(nl.value))

    # -- batched point evaluation (host AoS arrays)
    def seq(self, mat, sig):
        sig = _f64(sig).reshape(-1, 6)
        out = np.empty(len(sig))
        self._chk(self.lib.plfx_seq_batch(self.h, int(mat), len(sig), _dp(sig), _dp(out)))
        return out

    def fgrad(self, mat, sig):
        sig = _f64(sig).reshape(-1, 6)
        out = np.empty_like(sig)
        self._chk(self.lib.plfx_fgrad_batch(self.h, int(mat), len(sig), _dp(sig), _dp(out)))
        return out

    def fgrad_seq(self, mat, sig, seq):
        """calc_fgrad(sig, seq=seq) of an analytic Hill material: Voigt deviator over 2 seq (material.py:834-847)"""
        sig = _f64(sig).reshape(-1, 6)
        seq = _f64(seq).reshape(-1)
        if len(seq) != len(sig):
            raise ValueError('fgrad_seq: one equivalent stress per stress expected')
        out = np.empty_like(sig)
        self._chk(self.lib.plfx_fgrad_seq_batch(self.h, int(mat), len(sig), _dp(sig), _dp(seq), _dp(out)))
        return out

    def fgrad_wh(self, mat, sig, epl=None):
        """calc_fgrad(sig, epl) of a work-hardening SVC material: (gradient (N,6), raw hardening value per point (N,))"""
        sig = _f64(sig).reshape(-1, 6)
        epl = np.zeros_like(sig) if epl is None else _f64(epl).reshape(-1, 6)
        out = np.empty_like(sig)
        kh = np.empty(len(sig))
        self._chk(self.lib.plfx_fgrad_batch_wh(self.h, int(mat), len(sig), _dp(sig), _dp(epl), _dp(out), _dp(kh)))
        return out, kh

    def hessian(self, mat, sig, epl=None):
        """calc_hessian of an SVC material in feature space: (N,6,6), the stress-feature block (plfx_hessian_batch);
        epl (N,6) enters the features of a work-hardening material only (None: zeros)"""
        sig = _f64(sig).reshape(-1, 6)
        epl = None if epl is None else _f64(epl).reshape(-1, 6)
        if epl is not None and len(epl) != len(sig):
            raise ValueError('hessian: one plastic strain per stress expected')
        out = np.empty((len(sig), 6, 6))
        self._chk(self.lib.plfx_hessian_batch(self.h, int(mat), len(sig), _dp(sig), _dp(epl), _dp(out)))
        return out

    def yield_scale(self, mat, su, epl=None, x0=None):
        """(x (N,), status (N,) int32): the factor with calc_yf(x su, epl) = 0 along N unit stresses su (N,6), searched on
        the device ray by ray (plfx_yield_scale).  epl (N,6) or None (zeros); x0 (N,) start values or None
        (sflow(epl) / seq_J2(su)).  status 0 root found, 1 no bracket in [0.01 x0, 5 x0], 2 refinement cap, 3 degenerate ray;
        x is NaN where status is not 0."""
        su = _f64(su).reshape(-1, 6)
        epl = None if epl is None else _f64(epl).reshape(-1, 6)
        x0 = None if x0 is None else _f64(x0).reshape(-1)
        if epl is not None and len(epl) != len(su):
            raise ValueError('yield_scale: one plastic strain per unit stress expected')
        if x0 is not None and len(x0) != len(su):
            raise ValueError('yield_scale: one start value per unit stress expected')
        x = np.empty(len(su))
        st = np.zeros(len(su), dtype=np.int32)
        self._chk(self.lib.plfx_yield_scale(self.h, int(mat), len(su), _dp(su), _dp(epl), _dp(x0), _dp(x), _dp(st)))
        return x, st

    def flow_curve(self, mat, su, epl0=None, max_steps=300, depl=1.e-3, epl_max=0.02, predictor=0.):
        """Flow curves along N unit stresses su (N,6), whole chains in one launch (plfx_flow_curve): dict of x (N,K+1),
        epl (N,K+1,6), yf (N,K+1), hk (N,K), nsteps (N,), status (N,) with K = max_steps; NaN past a curve's last recorded
        point.  epl0 (N,6) or None (zeros).  Status 0 complete, 1 / 2 the root search's status where the curve ended,
        3 degenerate direction, 4 eps_eq of the gradient zero or not finite."""
        su = _f64(su).reshape(-1, 6)
        epl0 = None if epl0 is None else _f64(epl0).reshape(-1, 6)
        if epl0 is not None and len(epl0) != len(su):
            raise ValueError('flow_curve: one initial plastic strain per unit stress expected')
        n, K = len(su), int(max_steps)
        K0 = max(K, 0)
        x, yf = np.full((n, K0 + 1), np.nan), np.full((n, K0 + 1), np.nan)
        epl, hk = np.full((n, K0 + 1, 6), np.nan), np.full((n, K0), np.nan)
        ns, st = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        self._chk(self.lib.plfx_flow_curve(self.h, int(mat), n, _dp(su), _dp(epl0), K, C.c_double(depl), C.c_double(epl_max),
                                           C.c_double(predictor), _dp(x), _dp(epl), _dp(yf), _dp(hk), _dp(ns), _dp(st)))
        return dict(x=x, epl=epl, yf=yf, hk=hk, nsteps=ns, status=st)

    def flow_info(self):
        """dict(launches): launches of the flow-curve kernels by this context"""
        nl = C.c_int64()
        self._chk(self.lib.plfx_flow_info(self.h, C.byref(nl)))
        return dict(launches=int(nl.value))

    def load_path(self, mat, dload, control=None, sig0=None, epl0=None, tex_id=None, maxit=50, newton=30, stol=1., eps_cap=0.05,
                  return_tangent=False):
        """Load paths of N points of material ``mat`` in one launch (plfx_load_path): dload (K,N,6), or (K,6) shared by the
        points, whose number then comes from sig0 / epl0 / control / tex_id (else 1); control None or (N,) int32 with bit c set
        where component c is stress-controlled; sig0, epl0 (N,6) or None (zeros); tex_id (N,) or None.  Dict, step-major: sig,
        epl, deps (K,N,6), fy (K,N), nsteps, newton (K,N) int32, ksteps, status (N,) int32 and, with return_tangent, ct
        (N,6,6).  Status 0 complete, 1 stol not reached, 2 pivot zero or not finite, 3 deps not finite or beyond eps_cap."""
        dload = _f64(dload)
        shared = dload.ndim == 2
        if dload.ndim not in (2, 3) or dload.shape[-1] != 6:
            raise ValueError('load_path: dload of shape (K, N, 6) or (K, 6) expected')
        control = None if control is None else _i32(control).reshape(-1)
        sig0 = None if sig0 is None else _f64(sig0).reshape(-1, 6)
        epl0 = None if epl0 is None else _f64(epl0).reshape(-1, 6)
        tex_id = None if tex_id is None else _i32(tex_id).reshape(-1)
        given = [len(a) for a in (control, sig0, epl0, tex_id) if a is not None]
        n = dload.shape[1] if not shared else (given[0] if given else 1)
        if any(g != n for g in given):
            raise ValueError('load_path: one row of control, sig0, epl0 and tex_id per point expected')
        K = len(dload)
        # one block in the order of the library's device buffer: the results then arrive in one copy, without staging
        KN, nct = K * n, 36 * n if return_tangent else 0
        # (not filled: a call that launches writes every entry, NaN and -1 past a path's end included, and one that does not
        # has K = 0 or n = 0, or raises)
        buf = np.empty(19 * KN + nct + KN + n)
        ints = buf[19 * KN + nct:].view(np.int32)
        out = dict(sig=buf[:6 * KN].reshape(K, n, 6), epl=buf[6 * KN:12 * KN].reshape(K, n, 6),
                   deps=buf[12 * KN:18 * KN].reshape(K, n, 6), fy=buf[18 * KN:19 * KN].reshape(K, n),
                   nsteps=ints[:KN].reshape(K, n), newton=ints[KN:2 * KN].reshape(K, n), ksteps=ints[2 * KN:2 * KN + n],
                   status=ints[2 * KN + n:])
        ct = buf[19 * KN:19 * KN + nct].reshape(n, 6, 6) if return_tangent else None
        self._chk(self.lib.plfx_load_path(self.h, int(mat), n, K, _dp(dload), int(shared), _dp(control), _dp(sig0), _dp(epl0),
                                          _dp(tex_id), int(maxit), int(newton), C.c_double(stol), C.c_double(eps_cap),
                                          _dp(out['sig']), _dp(out['epl']), _dp(out['deps']), _dp(out['fy']), _dp(out['nsteps']),
                                          _dp(out['newton']), _dp(out['ksteps']), _dp(out['status']), _dp(ct)))
        if return_tangent:
            out['ct'] = ct
        return out

    def load_path_info(self):
        """dict(launches): launches of the load-path kernels by this context"""
        nl = C.c_int64()
        self._chk(self.lib.plfx_load_path_info(self.h, C.byref(nl)))
        return dict(launches=int(nl.value))

    PATH_WH_FORMS = {'auto': 0, 'thread': 1, 'wave': 2}

    def load_path_wh(self, mat, dload, khard0, control=None, sig0=None, epl0=None, form='auto', maxit=50, newton=30, stol=1.,
                     eps_cap=0.05, return_tangent=False):
        """Load paths of N points of the work-hardening SVC material ``mat`` in one launch (plfx_load_path_wh): load_path with
        the hardening modulus as state of each path.  khard0: scalar or (N,), the modulus at the start of the paths (it counts
        towards N when it is an array); form 'thread' (a thread per path: the bits of the loop over response(khard_in=,
        return_khard=True)), 'wave' (a wave per path) or 'auto' (by N).  The dict of load_path plus khard (K,N): the modulus
        after each completed step, NaN past ksteps."""
        if form not in self.PATH_WH_FORMS:
            raise ValueError("load_path: form must be 'auto', 'thread' or 'wave'; got %r" % (form,))
        dload = _f64(dload)
        shared = dload.ndim == 2
        if dload.ndim not in (2, 3) or dload.shape[-1] != 6:
            raise ValueError('load_path: dload of shape (K, N, 6) or (K, 6) expected')
        control = None if control is None else _i32(control).reshape(-1)
        sig0 = None if sig0 is None else _f64(sig0).reshape(-1, 6)
        epl0 = None if epl0 is None else _f64(epl0).reshape(-1, 6)
        khard0 = _f64(khard0)
        if khard0.ndim > 1:
            raise ValueError('load_path: khard0 must be a scalar or (N,)')
        given = [len(a) for a in (control, sig0, epl0, khard0 if khard0.ndim else None) if a is not None]
        n = dload.shape[1] if not shared else (given[0] if given else 1)
        if any(g != n for g in given):
            raise ValueError('load_path: one row of control, sig0, epl0 and khard0 per point expected')
        khard0 = np.ascontiguousarray(np.broadcast_to(khard0, (n,)))
        K = len(dload)
        # one block in the order of the library's device buffer, as in load_path
        KN, nct = K * n, 36 * n if return_tangent else 0
        buf = np.empty(20 * KN + nct + KN + n)
        ints = buf[20 * KN + nct:].view(np.int32)
        out = dict(sig=buf[:6 * KN].reshape(K, n, 6), epl=buf[6 * KN:12 * KN].reshape(K, n, 6),
                   deps=buf[12 * KN:18 * KN].reshape(K, n, 6), fy=buf[18 * KN:19 * KN].reshape(K, n),
                   khard=buf[19 * KN:20 * KN].reshape(K, n),
                   nsteps=ints[:KN].reshape(K, n), newton=ints[KN:2 * KN].reshape(K, n), ksteps=ints[2 * KN:2 * KN + n],
                   status=ints[2 * KN + n:])
        ct = buf[20 * KN:20 * KN + nct].reshape(n, 6, 6) if return_tangent else None
        self._chk(self.lib.plfx_load_path_wh(self.h, int(mat), n, K, _dp(dload), int(shared), _dp(control), _dp(sig0), _dp(epl0),
                                             _dp(khard0), self.PATH_WH_FORMS[form], int(maxit), int(newton), C.c_double(stol),
                                             C.c_double(eps_cap), _dp(out['sig']), _dp(out['epl']), _dp(out['deps']),
                                             _dp(out['fy']), _dp(out['khard']), _dp(out['nsteps']), _dp(out['newton']),
                                             _dp(out['ksteps']), _dp(out['status']), _dp(ct)))
        if return_tangent:
            out['ct'] = ct
        return out

    def load_path_wh_info(self):
        """dict(launches_thread, launches_wave): launches of k_path_batch<7> and of k_path_wh_wave by this context"""
        nt, nw = C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_load_path_wh_info(self.h, C.byref(nt), C.byref(nw)))
        return dict(launches_thread=int(nt.value), launches_wave=int(nw.value))

    def committee_yf(self, mats, scale, su, want_yf=True, want_mean=False, want_var=False, want_best=False):
        """A committee of 6-feature SVC materials on N shared unit stresses su (N,6) in one launch (plfx_committee_yf):
        member k is material mats[k] of this context with the stress scale scale[k].  Returns a dict with the requested
        entries: 'yf' (M,N) = calc_yf(su * scale[k]) per member, 'mean' (N,), 'var' (N,) (np.var over the members, ddof = 0),
        'best' = (index of the largest variance or -1, its value or NaN)."""
        mats = _i32(mats).reshape(-1)
        scale = _f64(scale).reshape(-1)
        if len(scale) != len(mats):
            raise ValueError('committee_yf: one scale per member expected')
        su = _f64(su).reshape(-1, 6)
        n, M = len(su), len(mats)
        yf = np.empty((M, n)) if want_yf else None
        mean = np.empty(n) if want_mean else None
        var = np.empty(n) if want_var else None
        best, bvar = C.c_int32(-1), C.c_double(float('nan'))
        self._chk(self.lib.plfx_committee_yf(self.h, M, _dp(mats), _dp(scale), n, _dp(su), _dp(yf), _dp(mean), _dp(var),
                                             C.byref(best) if want_best else None, C.byref(bvar) if want_best else None))
        out = {}
        if want_yf:
            out['yf'] = yf
        if want_mean:
            out['mean'] = mean
        if want_var:
            out['var'] = var
        if want_best:
            out['best'] = (int(best.value), float(bvar.value))
        return out

    def committee_info(self):
        """(launches of k_committee_yf so far, bit mask of the last call's members whose tables were staged in LDS)"""
        n, st = C.c_int64(), C.c_int32()
        self._chk(self.lib.plfx_committee_info(self.h, C.byref(n), C.byref(st)))
        return int(n.value), int(st.value)

    # -- texture SVC: a table set of the context, independent of its materials
    def tex_svc_set(self, sv, dual, intercept, gamma, mean, scale, dev_only=False):
        """install the texture SVC: sv (nsv, 6 + tdim) standardised support vectors, dual (nsv,), the scaler's mean and
        scale per column (plfx_tex_svc_set); sv=None releases the set"""
        if sv is None:
            self._chk(self.lib.plfx_tex_svc_set(self.h, 0, 0, None, None, C.c_double(0.), C.c_double(0.), None, None, 0))
            return
        sv = _f64(sv)
        dual = _f64(dual).reshape(-1)
        mean, scale = _f64(mean).reshape(-1), _f64(scale).reshape(-1)
        if sv.ndim != 2 or len(dual) != len(sv) or len(mean) != sv.shape[1] or len(scale) != sv.shape[1]:
            raise ValueError('tex_svc_set: sv (nsv, d), dual (nsv,), mean (d,) and scale (d,) expected')
        self._chk(self.lib.plfx_tex_svc_set(self.h, len(sv), sv.shape[1] - 6, _dp(sv), _dp(dual), C.c_double(float(intercept)),
                                            C.c_double(float(gamma)), _dp(mean), _dp(scale), int(bool(dev_only))))

    def tex_svc_yf(self, sig, tex, tex_id=None):
        """calc_yf(sig, tex=) of the texture SVC at N stresses sig (N,6) in one launch (plfx_tex_svc_yf): tex (T, tdim);
        tex_id (N,) picks a row per point, None means one shared texture (T = 1) or one per point (T = N)"""
        sig = _f64(sig).reshape(-1, 6)
        tex = _f64(tex)
        if tex.ndim != 2:
            raise ValueError('tex_svc_yf: tex (T, tdim) expected')
        tid = None if tex_id is None else _i32(tex_id).reshape(-1)
        if tid is not None and len(tid) != len(sig):
            raise ValueError('tex_svc_yf: one texture index per stress expected')
        yf = np.empty(len(sig))
        self._chk(self.lib.plfx_tex_svc_yf(self.h, len(sig), _dp(sig), len(tex), _dp(tex), _dp(tid), _dp(yf)))
        return yf

    def tex_svc_yield_scale(self, su, tex, x0=None):
        """(x (T,N), status (T,N) int32): calc_yf(x[t, r] su_r, tex_t) = 0 for N unit stresses su (N,6) and T textures
        tex (T, tdim), all T N rays searched in one launch (plfx_tex_svc_yield_scale); x0 (T,N) start values or None.
        Status as in yield_scale."""
        su = _f64(su).reshape(-1, 6)
        tex = _f64(tex)
        if tex.ndim != 2:
            raise ValueError('tex_svc_yield_scale: tex (T, tdim) expected')
        T, N = len(tex), len(su)
        if x0 is not None:
            x0 = _f64(x0)
            if x0.shape != (T, N):
                raise ValueError('tex_svc_yield_scale: x0 of shape (T, N) expected')
        x = np.empty((T, N))
        st = np.zeros((T, N), dtype=np.int32)
        self._chk(self.lib.plfx_tex_svc_yield_scale(self.h, N, _dp(su), T, _dp(tex), _dp(x0), _dp(x), _dp(st)))
        return x, st

    def tex_svc_info(self):
        """dict(nsv, tdim, yf_launches, ray_launches, staged) of the texture SVC of this context (nsv = 0: none)"""
        nsv, td, st = C.c_int(), C.c_int(), C.c_int()
        ny, nr = C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_tex_svc_info(self.h, C.byref(nsv), C.byref(td), C.byref(ny), C.byref(nr), C.byref(st)))
        return dict(nsv=int(nsv.value), tdim=int(td.value), yf_launches=int(ny.value), ray_launches=int(nr.value),
                    staged=bool(st.value))

    def tex_svc_flow_info(self):
        """dict(fgrad_launches, full_yf_launches, response_launches): launches of the flow-rule kernels of the texture SVC
        since the set was installed (plfx_tex_svc_flow_info)"""
        ng, nf, nq = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_tex_svc_flow_info(self.h, C.byref(ng), C.byref(nf), C.byref(nq)))
        return dict(fgrad_launches=int(ng.value), full_yf_launches=int(nf.value), response_launches=int(nq.value))

    @staticmethod
    def _tex_args(name, sig, tex, tex_id):
        sig = _f64(sig).reshape(-1, 6)
        tex = _f64(tex)
        if tex.ndim != 2:
            raise ValueError('%s: tex (T, tdim) expected' % name)
        tid = None if tex_id is None else _i32(tex_id).reshape(-1)
        if tid is not None and len(tid) != len(sig):
            raise ValueError('%s: one texture index per stress expected' % name)
        return sig, tex, tid

    def tex_svc_fgrad(self, sig, tex, tex_id=None):
        """calc_fgrad(sig, tex=) of the texture SVC at N stresses (N,6) in one launch (plfx_tex_svc_fgrad): (N,6); tex and
        tex_id as in tex_svc_yf"""
        sig, tex, tid = self._tex_args('tex_svc_fgrad', sig, tex, tex_id)
        out = np.empty_like(sig)
        self._chk(self.lib.plfx_tex_svc_fgrad(self.h, len(sig), _dp(sig), len(tex), _dp(tex), _dp(tid), _dp(out)))
        return out

    def tex_svc_full_yf(self, sig, tex, tex_id=None):
        """(f (N,), status (N,) int32): ML_full_yf(sig, tex=) of the texture SVC beside material 0 of the context, an
        analytic Hill / J2 record (plfx_tex_svc_full_yf)"""
        sig, tex, tid = self._tex_args('tex_svc_full_yf', sig, tex, tex_id)
        out = np.empty(len(sig))
        st = np.zeros(len(sig), dtype=np.int32)
        self._chk(self.lib.plfx_tex_svc_full_yf(self.h, len(sig), _dp(sig), len(tex), _dp(tex), _dp(tid), _dp(out), _dp(st)))
        return out, st

    def tex_svc_response(self, sig, epl, deps, tex, tex_id=None, mat=0, maxit=50):
        """(fy, sig, depl, ct (N,36), nsteps): Material.response with the texture SVC as yield function beside the analytic
        Hill / J2 record `mat` of the context (plfx_tex_svc_response)"""
        sig, tex, tid = self._tex_args('tex_svc_response', sig, tex, tex_id)
        n = len(sig)
        epl = _f64(epl).reshape(-1, 6)
        deps = _f64(deps).reshape(-1, 6)
        if len(epl) != n or len(deps) != n:
            raise ValueError('tex_svc_response: sig, epl and deps of one length expected')
        fy, so, dp, ct = np.empty(n), np.empty((n, 6)), np.empty((n, 6)), np.empty((n, 36))
        ns = np.empty(n, dtype=np.int32)
        self._chk(self.lib.plfx_tex_svc_response(self.h, int(mat), n, _dp(sig), _dp(epl), _dp(deps), len(tex), _dp(tex),
                                                 _dp(tid), int(maxit), _dp(fy), _dp(so), _dp(dp), _dp(ct), _dp(ns)))
        return fy, so, dp, ct, ns

    def yf(self, mat, sig, epl=None):
        sig = _f64(sig).reshape(-1, 6)
        epl = np.zeros_like(sig) if epl is None else _f64(epl).reshape(-1, 6)
        out = np.empty(len(sig))
        self._chk(self.lib.plfx_yf_batch(self.h, int(mat), len(sig), _dp(sig), _dp(epl), _dp(out)))
        return out

    def full_yf(self, mat, sig, epl=None, ld=None, tex_id=None):
        """tex_id: (N,) texture row per point of a material with a texture field (plfx_full_yf_batch_tid)"""
        sig = _f64(sig).reshape(-1, 6)
        epl = np.zeros_like(sig) if epl is None else _f64(epl).reshape(-1, 6)
        ldp = None if ld is None else _f64(ld).reshape(6)
        out = np.empty(len(sig))
        st = np.zeros(len(sig), dtype=np.int32)
        if tex_id is not None:
            tid = _i32(tex_id).reshape(-1)
            if len(tid) != len(sig):
                raise ValueError('full_yf: one texture row per stress expected')
            self._chk(self.lib.plfx_full_yf_batch_tid(self.h, int(mat), len(sig), _dp(sig), _dp(epl), _dp(ldp),
                                                      _dp(out), _dp(st), _dp(tid)))
            return out, st
        self._chk(self.lib.plfx_full_yf_batch(self.h, int(mat), len(sig), _dp(sig), _dp(epl), _dp(ldp),
                                              _dp(out), _dp(st)))
        return out, st

    # -- SVC training (plfx_svm.hpp)
    @staticmethod
    def _lists(lists, name):
        """list of index arrays -> (off[nprob+1], idx) int32"""
        lists = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
        if not lists:
            raise ValueError('%s: at least one problem expected' % name)
        off = np.zeros(len(lists) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(l) for l in lists])
        return off, _i32(np.concatenate(lists))

    def svc_fit_batch(self, X, y, problems, C, gamma, tol=1e-3, max_iter=-1):
        """Fit one binary RBF C-SVC per problem (libsvm's non-shrinking SMO) in one batched call.
        X (n, d) shared features, y (n,) labels -1 / +1, problems: list of row-index arrays into X; C, gamma: scalars or one
        per problem.  Returns a list of dicts (alpha in the order of the index array, rho with decision = sum y alpha K - rho,
        obj, n_iter, status 0 converged / 1 max_iter reached)."""
        import ctypes   # (the argument C shadows this module's ctypes alias)
        X = _f64(X)
        if X.ndim != 2:
            raise ValueError('svc_fit_batch: X must be (n, d)')
        y = _f64(y).reshape(-1)
        if len(y) != len(X):
            raise ValueError('svc_fit_batch: X and y differ in length')
        off, idx = self._lists(problems, 'svc_fit_batch')
        npb = len(off) - 1
        Cs = _f64(np.broadcast_to(np.asarray(C, dtype=float), (npb,)))
        gs = _f64(np.broadcast_to(np.asarray(gamma, dtype=float), (npb,)))
        alpha = np.empty(len(idx))
        rho, obj = np.empty(npb), np.empty(npb)
        it, st = np.empty(npb, dtype=np.int32), np.empty(npb, dtype=np.int32)
        self._chk(self.lib.plfx_svc_fit_batch(self.h, len(X), X.shape[1], _dp(X), _dp(y), npb, _dp(off), _dp(idx),
                                              _dp(Cs), _dp(gs), ctypes.c_double(tol), ctypes.c_int64(int(max_iter)),
                                              _dp(alpha), _dp(rho), _dp(obj), _dp(it), _dp(st)))
        return [dict(alpha=alpha[off[p]:off[p + 1]], rho=float(rho[p]), obj=float(obj[p]), n_iter=int(it[p]),
                     status=int(st[p])) for p in range(npb)]

    def svc_fit_wide(self, X, y, C, gamma, tol=1e-3, max_iter=-1, nwg=0):
        """One binary RBF C-SVC fit over all rows of X spread across nwg workgroups (0: automatic): the result of
        svc_fit_batch(X, y, [arange(n)], C, gamma) bit for bit.  Returns one dict like svc_fit_batch's entries."""
        import ctypes   # (the argument C shadows this module's ctypes alias)
        X = _f64(X)
        if X.ndim != 2:
            raise ValueError('svc_fit_wide: X must be (n, d)')
        y = _f64(y).reshape(-1)
        if len(y) != len(X):
            raise ValueError('svc_fit_wide: X and y differ in length')
        alpha = np.empty(len(y))
        rho, obj = np.empty(1), np.empty(1)
        it, st = np.empty(1, dtype=np.int32), np.empty(1, dtype=np.int32)
        self._chk(self.lib.plfx_svc_fit_wide(self.h, len(X), X.shape[1], _dp(X), _dp(y), ctypes.c_double(float(C)),
                                             ctypes.c_double(float(gamma)), ctypes.c_double(tol),
                                             ctypes.c_int64(int(max_iter)), int(nwg), _dp(alpha), _dp(rho), _dp(obj),
                                             _dp(it), _dp(st)))
        return dict(alpha=alpha, rho=float(rho[0]), obj=float(obj[0]), n_iter=int(it[0]), status=int(st[0]))

    def svc_decision_batch(self, X, sv_lists, coefs, intercepts, gamma, query_lists):
        """Decision values of several RBF-SVC models whose support vectors and query points are rows of the shared X:
        model p = (rows sv_lists[p], dual coefficients coefs[p], intercepts[p], gamma[p]) on the rows query_lists[p].
        Returns a list of arrays, one per model."""
        X = _f64(X)
        so, si = self._lists(sv_lists, 'svc_decision_batch')
        qo, qi = self._lists(query_lists, 'svc_decision_batch')
        npb = len(so) - 1
        if len(qo) - 1 != npb or len(coefs) != npb:
            raise ValueError('svc_decision_batch: one support-vector list, coefficient array and query list per model')
        cf = _f64(np.concatenate([np.asarray(c, dtype=float).reshape(-1) for c in coefs]))
        if len(cf) != len(si):
            raise ValueError('svc_decision_batch: one coefficient per support vector expected')
        ic = _f64(np.broadcast_to(np.asarray(intercepts, dtype=float), (npb,)))
        gs = _f64(np.broadcast_to(np.asarray(gamma, dtype=float), (npb,)))
        out = np.empty(len(qi))
        self._chk(self.lib.plfx_svc_decision_batch(self.h, len(X), X.shape[1], _dp(X), npb, _dp(so), _dp(si), _dp(cf),
                                                   _dp(ic), _dp(gs), _dp(qo), _dp(qi), _dp(out)))
        return [out[qo[p]:qo[p + 1]] for p in range(npb)]

    # -- SVR flow rule (plfx_svm.hpp)
    def svr_fit_batch(self, X, problems, targets, C, gamma, epsilon=0.1, tol=1e-3, max_iter=-1):
        """Fit one RBF epsilon-SVR per problem (libsvm's non-shrinking SMO) in one batched call.
        X (n, d) shared features, problems: list of row-index arrays into X, targets: one array per problem in the order
        of its index array; C, gamma, epsilon: scalars or one per problem.  Returns a list of dicts (coef = alpha - alpha*
        in the order of the index array, rho with prediction = sum coef K - rho, obj, n_iter, status 0 converged / 1
        max_iter reached)."""
        import ctypes   # (the argument C shadows this module's ctypes alias)
        X = _f64(X)
        if X.ndim != 2:
            raise ValueError('svr_fit_batch: X must be (n, d)')
        off, idx = self._lists(problems, 'svr_fit_batch')
        npb = len(off) - 1
        if len(targets) != npb:
            raise ValueError('svr_fit_batch: one target array per problem expected')
        t = _f64(np.concatenate([np.asarray(v, dtype=float).reshape(-1) for v in targets]))
        if len(t) != len(idx) or any(len(np.reshape(v, -1)) != off[p + 1] - off[p] for p, v in enumerate(targets)):
            raise ValueError('svr_fit_batch: one target per row of every problem expected')
        Cs = _f64(np.broadcast_to(np.asarray(C, dtype=float), (npb,)))
        gs = _f64(np.broadcast_to(np.asarray(gamma, dtype=float), (npb,)))
        es = _f64(np.broadcast_to(np.asarray(epsilon, dtype=float), (npb,)))
        coef = np.empty(len(idx))
        rho, obj = np.empty(npb), np.empty(npb)
        it, st = np.empty(npb, dtype=np.int32), np.empty(npb, dtype=np.int32)
        self._chk(self.lib.plfx_svr_fit_batch(self.h, len(X), X.shape[1], _dp(X), npb, _dp(off), _dp(idx), _dp(t), _dp(Cs),
                                              _dp(gs), _dp(es), ctypes.c_double(tol), ctypes.c_int64(int(max_iter)),
                                              _dp(coef), _dp(rho), _dp(obj), _dp(it), _dp(st)))
        return [dict(coef=coef[off[p]:off[p + 1]], rho=float(rho[p]), obj=float(obj[p]), n_iter=int(it[p]),
                     status=int(st[p])) for p in range(npb)]

    def svr_predict_multi(self, X, coef, intercepts, gamma, Q):
        """Predictions of m <= 8 RBF models on the shared training rows X (n, d): coef (n, m) with zeros where a row is
        no support vector of a model, intercepts (m,), query points Q (nq, d).  Returns (nq, m)."""
        X, Q = _f64(X), _f64(Q)
        coef = _f64(coef)
        ic = _f64(intercepts).reshape(-1)
        if X.ndim != 2 or Q.ndim != 2 or Q.shape[1] != X.shape[1]:
            raise ValueError('svr_predict_multi: X (n, d) and Q (nq, d) expected')
        if coef.ndim != 2 or coef.shape[0] != len(X) or coef.shape[1] != len(ic):
            raise ValueError('svr_predict_multi: coef must be (n, m) with one intercept per column')
        out = np.empty((len(Q), len(ic)))
        self._chk(self.lib.plfx_svr_predict_multi(self.h, len(X), X.shape[1], _dp(X), C.c_double(float(gamma)), len(ic),
                                                  _dp(coef), _dp(ic), len(Q), _dp(Q), _dp(out)))
        return out

    def set_svr_flow(self, mat, X=None, coef=None, intercepts=None, gamma=0., feat_mean=None, feat_scale=None, out_mean=None,
                     out_scale=None):
        """Attach an SVR flow rule to the work-hardening SVC material ``mat`` of the loaded set (plfx_set_svr_flow):
        X (l, 12) standardised training rows, coef (l, 7) with zeros where a row is no support vector of a model,
        intercepts (7,), gamma, the feature scaler (12,) / (12,) and the output scaler (7,) / (7,): six gradient components,
        then the hardening rate.  ``response`` then takes every gradient evaluation of this material's points from the
        SVRs.  ``X=None`` (or no row) detaches; ``set_materials`` detaches every rule."""
        if X is None or len(X) == 0:
            self._chk(self.lib.plfx_set_svr_flow(self.h, int(mat), 0, None, None, None, C.c_double(0.), None, None, None, None))
            return
        X, coef = _f64(X), _f64(coef)
        ic = _f64(intercepts).reshape(-1)
        fm, fs = _f64(feat_mean).reshape(-1), _f64(feat_scale).reshape(-1)
        om, osc = _f64(out_mean).reshape(-1), _f64(out_scale).reshape(-1)
        if X.ndim != 2 or X.shape[1] != 12 or coef.shape != (len(X), 7) or len(ic) != 7:
            raise ValueError('set_svr_flow: X (l, 12), coef (l, 7) and 7 intercepts expected')
        if len(fm) != 12 or len(fs) != 12 or len(om) != 7 or len(osc) != 7:
            raise ValueError('set_svr_flow: 12 feature means / scales and 7 output means / scales expected')
        self._chk(self.lib.plfx_set_svr_flow(self.h, int(mat), len(X), _dp(X), _dp(coef), _dp(ic), C.c_double(float(gamma)),
                                             _dp(fm), _dp(fs), _dp(om), _dp(osc)))

    def svr_flow_info(self, mat=0):
        """(rows of the SVR flow rule attached to material ``mat`` -- 0: none --, response launches that took the SVR kernel
        for it since it was attached)"""
        rows, launches = C.c_int(0), C.c_int64(0)
        self._chk(self.lib.plfx_svr_flow_info(self.h, int(mat), C.byref(rows), C.byref(launches)))
        return rows.value, launches.value

    def set_response_maxit(self, maxit=50):
        self._chk(self.lib.plfx_set_response_maxit(self.h, int(maxit)))

    def response(self, sig, epl, deps, mat_id=None, khard_in=None, return_khard=False, maxit=50, tex_id=None):
        """khard_in / return_khard: entry / exit value of Material.khard per point (work-hardening SVC materials);
        maxit: Material.response's argument (sub-steps of a sub-divided increment); tex_id: (N,) texture row per point of
        the materials with a texture field (plfx_response_batch_tid)"""
        if maxit != 50:
            self.set_response_maxit(maxit)
            try:
                return self.response(sig, epl, deps, mat_id, khard_in, return_khard, tex_id=tex_id)
            finally:
                self.set_response_maxit(50)
        sig = _f64(sig).reshape(-1, 6)
        n = len(sig)
        epl = _f64(epl).reshape(-1, 6)
        deps = _f64(deps).reshape(-1, 6)
        mid = None if mat_id is None else _i32(mat_id)
        fy = np.empty(n)
        so = np.empty((n, 6))
        dp = np.empty((n, 6))
        ct = np.empty((n, 36))
        ns = np.empty(n, dtype=np.int32)
        if khard_in is not None or return_khard:
            kin = None if khard_in is None else _f64(np.broadcast_to(np.asarray(khard_in, dtype=float), (n,)).copy())
            kout = np.empty(n)
            self._chk(self.lib.plfx_response_batch_kh(self.h, n, _dp(mid), _dp(sig), _dp(epl), _dp(deps), _dp(kin),
                                                      _dp(fy), _dp(so), _dp(dp), _dp(ct), _dp(ns), _dp(kout)))
            if return_khard:
                return fy, so, dp, ct, ns, kout
            return fy, so, dp, ct, ns
        if tex_id is not None:
            tid = _i32(tex_id).reshape(-1)
            if len(tid) != n:
                raise ValueError('response: one texture row per point expected')
            self._chk(self.lib.plfx_response_batch_tid(self.h, n, _dp(mid), _dp(sig), _dp(epl), _dp(deps),
                                                       _dp(fy), _dp(so), _dp(dp), _dp(ct), _dp(ns), _dp(tid)))
            return fy, so, dp, ct, ns
        self._chk(self.lib.plfx_response_batch(self.h, n, _dp(mid), _dp(sig), _dp(epl), _dp(deps),
                                               _dp(fy), _dp(so), _dp(dp), _dp(ct), _dp(ns)))
        return fy, so, dp, ct, ns

    # -- mesh / state
    def set_mesh(self, conn, mat_id, lxy, nnode, thick, planestress, el_begin=0, el_end=None):
        conn = _i32(conn).reshape(-1, 4)
        nel = len(conn)
        mat_id = _i32(mat_id)
        lxy = _f64(lxy).reshape(nel, 2)
        if el_end is None:
            el_end = nel
        self._chk(self.lib.plfx_set_mesh(self.h, nel, int(nnode), _dp(conn), _dp(mat_id), _dp(lxy),
                                         C.c_double(thick), int(bool(planestress)), int(el_begin),
                                         int(el_end)))
        self.nel = nel
        self.nel_owned = el_end - el_begin
        self.ndof = 2 * int(nnode)

    def set_mesh_structured(self, NX, NY, dx_col, dy, thick, planestress, mat_col=None, mat_el=None, el_begin=0, el_end=None):
        """Model.mesh's structured grid by description (plfx_set_mesh_structured): the library writes the index arrays"""
        nel = int(NX) * int(NY)
        dx = _f64(dx_col).reshape(int(NX))
        mc = None if mat_col is None else _i32(mat_col).reshape(int(NX))
        me = None if mat_el is None else _i32(mat_el).reshape(nel)
        if el_end is None:
            el_end = nel
        self._chk(self.lib.plfx_set_mesh_structured(self.h, int(NX), int(NY), _dp(mc), _dp(me), _dp(dx), C.c_double(dy),
                                                    C.c_double(thick), int(bool(planestress)), int(el_begin), int(el_end)))
        self.nel = nel
        self.nel_owned = el_end - el_begin
        self.ndof = 2 * (int(NX) + 1) * (int(NY) + 1)

    def set_grid(self, nx, ny):
        self._chk(self.lib.plfx_set_grid(self.h, int(nx), int(ny)))

    def sweep_info(self):
        """(sweeps, element tangents rewritten by them) since the context was created"""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_sweep_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sweep_launch_info(self):
        """(sweeps that left the corrector launches out because the previous sweep's list was empty, those among them that
        had to launch the corrector after all) since the context was created"""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_sweep_launch_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def bc_info(self):
        """(apply_bc calls that rewrote rhs on the boundary rows only, those among them that kept dinv, those that formed it
        again on its own, solves whose du was composed under the wait for the first test) since the context was created"""
        a, b, r, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_bc_info(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(d)))
        return a.value, b.value, r.value, d.value

    def short_info(self):
        """(apply_bc calls that left the fine level's dinv unformed after a tangent update, k_dinv launches that made up for one
        in front of a reader of its values, solves that found the d of their interpolated start already written, 0: a merged
        launch behind the sweep's flags was not kept) since the context was created; PLFX_SHORT_SOLVE=0: all zero"""
        a, b, r, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_short_info(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(d)))
        return a.value, b.value, r.value, d.value

    def snap_info(self):
        """(sweeps that stored their rewritten generators into the operator's snapshot themselves, assemblies that found it taken
        and launched nothing, set-up passes launched after all in front of a reader of the fine diagonal or the level-1
        generators, copies of the snapshot back into the live array) since the context was created; PLFX_DIRECT_SNAP=0: all zero"""
        a, b, r, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_snap_info(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(d)))
        return a.value, b.value, r.value, d.value

    def code_info(self):
        """(node codes formed, k_cg_start_test / k_cg_start_pred launches that read the code, those among them that loaded rhs
        on the boundary rows alone, k_pred_dots / k_pred_try / k_pred_finish / k_compose_du launches that read it) since the
        context was created; PLFX_NODE_CODE=0: the last three stay zero"""
        a, b, r, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_code_info(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(d)))
        return a.value, b.value, r.value, d.value

    def code_get(self):
        """the node code of the last apply_bc, uint8[nnode]: bit 0 / 1 the x / y DOF is prescribed, bit 2 the node is a row next
        to a prescribed node"""
        out = np.empty(self.ndof // 2, dtype=np.uint8)
        self._chk(self.lib.plfx_code_get(self.h, _dp(out)))
        return out

    def dead_store_info(self):
        """(sweeps of load steps whose changed elements left res_sig / res_depl / fyn to the next sweep, tangents rewritten in
        them, solves started with the sums of the first test alone, those among them that needed the full start after all)
        since the context was created"""
        a, b, r, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_dead_store_info(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(d)))
        return a.value, b.value, r.value, d.value

    PLANE_OFF_REASONS = ('on', 'no state reset yet', 'switch', 'sharded', 'materials', 'state_set', 'tangent set')

    def plane_info(self):
        """(plane-column mode on, launches of the plane Hill sweep, launches of the plane state update since the context was
        created, why the mode is off: an index into PLANE_OFF_REASONS, 0 while it is on)"""
        on, a, b, why = C.c_int(), C.c_int64(), C.c_int64(), C.c_int()
        self._chk(self.lib.plfx_plane_info(self.h, C.byref(on), C.byref(a), C.byref(b), C.byref(why)))
        return bool(on.value), a.value, b.value, why.value

    MG_TAIL_KERNELS = ('none', 'tail', 'tail_lds', 'tail_mf', 'tail_mf_ragged')
    MG_COARSE_SOLVERS = ('dense', 'cheby', 'pcg')

    def mg_info(self):
        """dict: the form of the V-cycle the next cycle runs (plfx_mg_info) -- 'levels': [(nx, ny, rx, ry, matrix-free), ...],
        'tail_level' (-1: no tail kernel), 'tail_kernel' (one of MG_TAIL_KERNELS), 'coarse_solver' (one of MG_COARSE_SOLVERS),
        'cheby_steps', 'cheby_kappa', 'march' (marching fine-level kernels)"""
        cap = 64
        nl, tl, tk, cs, st, ma = (C.c_int() for _ in range(6))
        kap = C.c_double()
        dims, rat, mf = np.zeros((cap, 2), dtype=np.int32), np.zeros((cap, 2)), np.zeros(cap, dtype=np.int32)
        self._chk(self.lib.plfx_mg_info(self.h, cap, C.byref(nl), _dp(dims), _dp(rat), _dp(mf), C.byref(tl), C.byref(tk),
                                        C.byref(cs), C.byref(st), C.byref(kap), C.byref(ma)))
        n = min(nl.value, cap)
        return {'levels': [(int(dims[l, 0]), int(dims[l, 1]), float(rat[l, 0]), float(rat[l, 1]), bool(mf[l])) for l in range(n)],
                'tail_level': tl.value, 'tail_kernel': self.MG_TAIL_KERNELS[tk.value],
                'coarse_solver': self.MG_COARSE_SOLVERS[cs.value], 'cheby_steps': st.value, 'cheby_kappa': kap.value,
                'march': bool(ma.value)}

    def svc_info(self):
        """(bit mask of the 6-feature SVC materials on the 16-lanes-per-element kernels, mask of those run one thread per
        element, sweep launches of either form) since the context was created"""
        a, b, r, t = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_svc_info(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(t)))
        return a.value, b.value, r.value, t.value

    def reuse_info(self):
        """(assemblies, BC applications, solves) answered from unchanged inputs since the context was created"""
        a, b, s = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.plfx_reuse_info(self.h, C.byref(a), C.byref(b), C.byref(s)))
        return a.value, b.value, s.value

    def predict_info(self):
        """(applied, skipped, rejected): warm-started solves answered by the interpolation of the last two solutions /
        not tried further (alpha < 0.01) / tried and iterated from the plain warm start instead"""
        a, b, r = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_predict_info(self.h, C.byref(a), C.byref(b), C.byref(r)))
        return a.value, b.value, r.value

    def set_precond(self, kind, omega=0., nu=0):
        self._chk(self.lib.plfx_set_precond(self.h, int(kind), C.c_double(omega), int(nu)))

    def precond_info(self):
        k = C.c_int()
        lv = C.c_int()
        self._chk(self.lib.plfx_precond_info(self.h, C.byref(k), C.byref(lv)))
        return k.value, lv.value

    def precond_apply(self, r):
        """one V-cycle applied to a host vector (tests)"""
        r = _f64(r).reshape(-1)
        z = np.empty_like(r)
        self._chk(self.lib.plfx_precond_apply(self.h, _dp(r), _dp(z)))
        return z

    def precond_bench(self, reps=100):
        """(microseconds per V-cycle, microseconds of it below the fine level) from `reps` back-to-back applications"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.lib.plfx_precond_bench(self.h, int(reps), C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_wh_mode(self, sequential):
        """work-hardening SVC: hardening modulus handed from element to element like the reference (True) or per point"""
        self._chk(self.lib.plfx_set_wh_mode(self.h, 1 if sequential else 0))

    def wh_info(self):
        """(sequential carry in use, sweeps run in that mode, passes they took)"""
        a, b, c_, u = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_wh_info(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(u)))
        self.wh_unresolved = u.value
        return bool(a.value), b.value, c_.value

    def wh_unresolved_sweeps(self):
        """sweeps whose carry chain was still changing when the pass cap (PLFX_WH_MAXPASS) ended them"""
        self.wh_info()
        return self.wh_unresolved

    def wh_carry(self, mat, value=None):
        """the hardening modulus material `mat` holds now (sequential carry); value != None sets it first"""
        g = C.c_double()
        sv = None if value is None else C.byref(C.c_double(float(value)))
        self._chk(self.lib.plfx_wh_carry(self.h, int(mat), sv, C.byref(g)))
        return g.value

    def solve_fallbacks(self):
        """solves completed by Jacobi-PCG after multigrid-PCG broke down or stalled"""
        n = C.c_int64()
        self._chk(self.lib.plfx_solve_fallbacks(self.h, C.byref(n)))
        return n.value

    def indefinite_info(self):
        """dict: solves with an indefinite tangent stiffness and how many GMRES completed (plfx_indefinite_info;
        by_minres_surrogate, surrogates_built and elements_shifted are always 0)"""
        v = [C.c_int64() for _ in range(5)]
        self._chk(self.lib.plfx_indefinite_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(('solves', 'by_minres_surrogate', 'by_gmres', 'surrogates_built', 'elements_shifted'),
                        [x.value for x in v]))

    def set_operator(self, kind):
        self._chk(self.lib.plfx_set_operator(self.h, int(kind)))

    def matvec(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.ndof,):
            raise ValueError('matvec: x must have shape (ndof,)')
        y = np.empty(self.ndof)
        self._chk(self.lib.plfx_matvec(self.h, _dp(x), _dp(y)))
        return y

    def operator_info(self):
        m = C.c_int()
        lv = C.c_int()
        self._chk(self.lib.plfx_operator_info(self.h, C.byref(m), C.byref(lv)))
        return m.value, lv.value

    def get_bmat(self, e):
        B = np.empty((4, 6, 8))
        self._chk(self.lib.plfx_get_bmat(self.h, int(e), _dp(B)))
        return B

    def get_kel(self, e):
        K = np.empty((8, 8))
        self._chk(self.lib.plfx_get_kel(self.h, int(e), _dp(K)))
        return K

    def state_get(self, which):
        if which in (ST_U, ST_F, ST_DU):
            out = np.empty(self.ndof)
        elif which in (ST_FYN, ST_MAXSTEPS, ST_KHARD):
            out = np.empty(self.nel_owned)
        elif which == ST_ELSTIFF:
            out = np.empty((self.nel_owned, 36))
        else:
            out = np.empty((self.nel_owned, 6))
        self._chk(self.lib.plfx_state_get(self.h, int(which), _dp(out)))
        return out

    def state_set(self, which, arr):
        arr = _f64(arr)
        self._chk(self.lib.plfx_state_set(self.h, int(which), _dp(arr)))

    def state_reset(self):
        self._chk(self.lib.plfx_state_reset(self.h))

    def element_fields(self, sel, want_out=True, want_range=False):
        """plfx_element_fields: (rows[len(sel), nel_owned] or None, range[len(sel), 2] or None) of the selector ids ``sel``
        from one device pass"""
        sel = _i32(sel).reshape(-1)
        out = np.empty((len(sel), self.nel_owned)) if want_out else None
        rng = np.empty((len(sel), 2)) if want_range else None
        self._chk(self.lib.plfx_element_fields(self.h, len(sel), _dp(sel), _dp(out), _dp(rng)))
        return out, rng

    def gather(self, which, idx):
        idx = _i32(idx)
        out = np.empty(len(idx))
        self._chk(self.lib.plfx_gather(self.h, int(which), len(idx), _dp(idx), _dp(out)))
        return out

    # -- assembly / solve
    def assemble(self):
        self._chk(self.lib.plfx_assemble(self.h))

    def get_csr(self):
        """Assembled global matrix as scipy.sparse.csr_matrix."""
        import scipy.sparse as sp
        nnz = C.c_int64()
        self._chk(self.lib.plfx_get_csr(self.h, C.byref(nnz), None, None, None))
        rowptr = np.empty(self.ndof + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        self._chk(self.lib.plfx_get_csr(self.h, C.byref(nnz), _dp(rowptr), _dp(col), _dp(val)))
        return sp.csr_matrix((val, col, rowptr), shape=(self.ndof, self.ndof))

    def apply_bc(self, idx, du_presc, w, fext=None):
        idx = _i32(idx)
        du_presc = _f64(du_presc)
        w = _f64(w)
        fx = None if fext is None else _f64(fext)
        self._chk(self.lib.plfx_apply_bc(self.h, len(idx), _dp(idx), _dp(du_presc), _dp(w), _dp(fx)))

    def set_bc_plan(self, seg_len, idx):
        seg_len = _i32(seg_len)
        idx = _i32(idx)
        self._chk(self.lib.plfx_set_bc_plan(self.h, len(seg_len), _dp(seg_len), _dp(idx)))
        self._plan_nseg = len(seg_len)

    def apply_bc_plan(self, seg_val, fext=None):
        seg_val = _f64(seg_val)
        if len(seg_val) != self._plan_nseg:
            raise ValueError('apply_bc_plan: one value per registered segment expected')
        fx = None if fext is None else _f64(fext)
        bad = C.c_int(-1)
        self._chk(self.lib.plfx_apply_bc_plan(self.h, _dp(seg_val), _dp(fx), C.byref(bad)))
        return bad.value

    def set_bc_sources(self, src, k, fsrc, fk, flen, fidx, fshare):
        src, k, fsrc, fk, flen, fidx = (_i32(a) for a in (src, k, fsrc, fk, flen, fidx))
        fshare = _f64(fshare)
        self._chk(self.lib.plfx_set_bc_sources(self.h, len(src), _dp(src), _dp(k), len(fsrc), _dp(fsrc), _dp(fk),
                                               _dp(flen), _dp(fidx), _dp(fshare)))

    def load_step(self, step):
        """one load step (plfx_load_step); returns the data of finish_step"""
        uu, ff, sums = self._fin
        self._chk(self.lib.plfx_load_step(self.h, C.byref(step), _dp(uu), _dp(ff), _dp(sums)))
        return uu, ff, sums.reshape(3, 6)

    @staticmethod
    def lib_has_mailbox():
        """the pinned host mailbox is on unless PLFX_MAILBOX=0 (deferred end-of-step results need it)"""
        return os.environ.get('PLFX_MAILBOX', '1') != '0'

    def finish_fetch(self, slot):
        """end-of-step data of a load step that ran with step.defer_slot = slot + 1"""
        uu, ff, sums = self._fin
        self._chk(self.lib.plfx_finish_fetch(self.h, int(slot), _dp(uu), _dp(ff), _dp(sums)))
        return uu, ff, sums.reshape(3, 6)

    def set_finish_set(self, idx):
        idx = _i32(idx)
        self._chk(self.lib.plfx_set_finish_set(self.h, len(idx), _dp(idx)))
        self._fin = (np.empty(len(idx)), np.empty(len(idx)), np.empty(18))

    def finish_step(self):
        uu, ff, sums = self._fin
        self._chk(self.lib.plfx_finish_step(self.h, _dp(uu), _dp(ff), _dp(sums)))
        return uu, ff, sums.reshape(3, 6)

    def solve(self, rtol=1e-12, maxit=100000, warm=False):
        it = C.c_int()
        rr = C.c_double()
        rc = self._chk(self.lib.plfx_solve(self.h, C.c_double(rtol), int(maxit), int(bool(warm)),
                                           C.byref(it), C.byref(rr)), soft=True)
        return it.value, rr.value, rc == 0

    def sweep(self, nit):
        ch = C.c_int()
        cv = C.c_int()
        self._chk(self.lib.plfx_sweep(self.h, int(nit), C.byref(ch), C.byref(cv)))
        return bool(ch.value), bool(cv.value)

    def scf_stats(self, sld):
        """returns (count, min, sum) of the calc_scf list entries"""
        sld = _f64(sld).reshape(6)
        s = C.c_double()
        mn = C.c_double()
        cnt = C.c_int64()
        self._chk(self.lib.plfx_scf_stats(self.h, _dp(sld), C.byref(s), None, C.byref(mn), C.byref(cnt),
                                          C.c_double(0.), 0))
        return cnt.value, mn.value, s.value

    def scf_all(self, sld):
        """(count, min, sum, centred sum of squares) of the calc_scf list in one call"""
        sld = _f64(sld).reshape(6)
        s = C.c_double()
        s2 = C.c_double()
        mn = C.c_double()
        cnt = C.c_int64()
        self._chk(self.lib.plfx_scf_all(self.h, _dp(sld), C.byref(cnt), C.byref(mn), C.byref(s), C.byref(s2)))
        return cnt.value, mn.value, s.value, s2.value

    def scf_sumsq(self, mean):
        s2 = C.c_double()
        self._chk(self.lib.plfx_scf_stats(self.h, None, None, C.byref(s2), None, None, C.c_double(mean), 1))
        return s2.value

    def update_state(self):
        self._chk(self.lib.plfx_update_state(self.h))

    def global_sums(self):
        out = np.empty(18)
        self._chk(self.lib.plfx_global_sums(self.h, _dp(out)))
        return out.reshape(3, 6)

    # -- multi-GPU
    def comm_info(self):
        r, n, d = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.plfx_comm_info(self.h, C.byref(r), C.byref(n), C.byref(d)))
        return r.value, n.value, bool(d.value)

    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        self._chk(self.lib.plfx_comm_unique_id(buf))
        return bytes(buf.raw)

    def comm_init(self, uid, rank, nranks):
        buf = C.create_string_buffer(bytes(uid), 128)
        self._chk(self.lib.plfx_comm_init(self.h, buf, int(rank), int(nranks)))

    def set_strip(self, own_col0, own_col1, global_col0, global_nx, coarse_level):
        """this context holds one x-strip of a larger structured grid (plfx_set_strip)"""
        self._chk(self.lib.plfx_set_strip(self.h, int(own_col0), int(own_col1), int(global_col0), int(global_nx),
                                          int(coarse_level)))

    def strip_info(self):
        """(active, halo, coarse_level, levels of the replicated coarse hierarchy, halo refreshes, coarse gathers,
        all-reduces of partial sums, exchanges of the halo elements' stiffness generators)"""
        a, h, l, cl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        nh, nc, npart, ng = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.plfx_strip_info(self.h, C.byref(a), C.byref(h), C.byref(l), C.byref(cl), C.byref(nh),
                                           C.byref(nc), C.byref(npart), C.byref(ng)))
        return bool(a.value), h.value, l.value, cl.value, nh.value, nc.value, npart.value, ng.value

    def comm_selftest(self):
        """send / receive to self + all-reduce on scratch buffers through the RCCL communicator (raises on a mismatch)"""
        self._chk(self.lib.plfx_comm_selftest(self.h))

    def allreduce_host(self, values, op=0):
        """all-reduce <= 32 host doubles over the context's communicator (op 0 sum, 3 min)"""
        a = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._chk(self.lib.plfx_allreduce_host(self.h, a.ctypes.data_as(C.c_void_p), int(a.size), int(op)))
        return a

    _ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int)

    def comm_init_callback(self, rank, nranks, fn):
        """host-staged collectives (tests on one GPU, hosts without RCCL): ``fn(array, op)`` all-reduces the NumPy
        array in place (op 0 = sum, 3 = min) across the ranks"""
        def trampoline(user, buf, count, dtype, op):
            try:
                ct = C.c_int32 if dtype == 1 else C.c_double
                arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ct)), shape=(count,))
                fn(arr, op)
                return 0
            except Exception:  # noqa: BLE001 - reported as an error code across the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._ar_cb = self._ALLREDUCE_FN(trampoline)   # keep alive as long as the context
        self._chk(self.lib.plfx_comm_init_callback(self.h, int(rank), int(nranks), self._ar_cb, None))

    # -- instrumentation
    def timing_enable(self, on=True):
        self._chk(self.lib.plfx_timing_enable(self.h, int(bool(on))))

    def timing_select(self, families=None):
        """time only the given families (T_* constants); None = all"""
        mask = 0xFF if families is None else sum(1 << int(f) for f in set(families))
        self._chk(self.lib.plfx_timing_select(self.h, C.c_uint(mask)))

    def timing_sample(self, every=1):
        """time only every n-th launch of the selected families"""
        self._chk(self.lib.plfx_timing_sample(self.h, int(every)))

    def timing_reset(self):
        self._chk(self.lib.plfx_timing_reset(self.h))

    def timing_get(self, which):
        ms = C.c_double()
        n = C.c_int64()
        self._chk(self.lib.plfx_timing_get(self.h, int(which), C.byref(ms), C.byref(n)))
        return ms.value, n.value
