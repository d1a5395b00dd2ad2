"""Cases and from-definition references for the reductions of a load step that combine results ACROSS workgroups:
the sequential hardening carry of one sweep (k_wh_blockmax / k_wh_scan / k_wh_entry), the calc_scf statistics (k_scf_reduce /
k_scf_finish) and the 18 element sums of calc_global (k_global_partials / k_reduce_rows / k_finish_out).  Shared by
tests/test_reduction_cases_cpu.py (conditions on the inputs, held on the oracle alone) and the GPU tests
test_gpu_wh_chain_blocks.py / test_gpu_element_reductions.py.  Nothing here touches libplfx or a GPU: the models are façade
models that are meshed but never solved, the numbers come from the CPU oracle and NumPy."""
import functools
import math
import os

import numpy as np

from oracle import oracle as O
from oracle.solve_ref import RefSolver

BLOCK = 256            # elements per workgroup of the carry kernels and of every reducing kernel (plfx_kernels.hpp: BLOCK)
NY_CHAIN = 16          # element e = j * NY + k: a block of 256 elements is exactly 16 element columns
SCF_CAP = 256          # blocks of k_scf_reduce (plfx_scf_all: grid_for(nel, 256)): grid-stride loop past 65 536 elements
SUM_CAP = 2048         # blocks of k_global_partials / k_update_state<1> (plfx_host.hpp: SUMPART): past 524 288 elements
START_CARRY = 123.456  # a modulus no call leaves behind


def golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name))


def block_of(e):
    return np.asarray(e) // BLOCK


# ------------------------------------------------------------------------------------------------ A: the carry chain
def wh_material(zc, name='ML-hardening', num=1):
    """the work-hardening SVC of svc_workhard_chain.npz as a façade material (tests/test_workhard_svc.py: facade_material)"""
    import pylabfea_amd as FE
    m = FE.Material(name=name, num=num)
    m.elasticity(CV=zc['par_CV'])
    m.plasticity(sy=float(zc['par_sy']), sdim=6)
    m.set_svc(zc['par_sv'], zc['par_dual'], float(zc['par_intercept']), float(zc['par_gamma']), float(zc['par_scale_seq']),
              dev_only=bool(zc['par_dev_only']), scale_wh=float(zc['par_scale_wh']))
    return m


def _rect(j0, j1, k0=0, k1=NY_CHAIN + 1):
    return [(j, k) for j in range(j0, j1) for k in range(k0, k1)]


# name -> (NX, sections [(material key, element columns)], start carry per work-hardening object, active nodes, pushed nodes).
# A node is (column j, row k); du is zero on every node that is neither active nor pushed, so an element none of whose four
# nodes moves has deps == 0 exactly: its call stays elastic, evaluates no gradient and hands its entry modulus on ("quiet").
# Active nodes carry the field of ChainCase (rectangles of them load whole columns); pushed nodes are always a pair on the top
# or the bottom edge and load the one element that holds both.
# Material keys: A, B work-hardening SVC objects (the same fit, two Python objects), el elastic, j2 an analytic J2 material.
def _chain_table():
    T, N = {}, NY_CHAIN
    # 1. loaded only in block 0: the predecessor of every element of blocks 1.. is element 255, one, two and three blocks back
    T['block0_784'] = (49, [('A', 49)], {'A': START_CARRY}, _rect(13, 16), [])
    # (... and a mesh whose second block is nearly empty: 16 elements, all of them quiet)
    T['block0_272'] = (17, [('A', 17)], {'A': START_CARRY}, _rect(13, 16), [])
    # 2. block 0 entirely quiet: every element before the first touched one takes the start carry
    # (272: the only column of block 1 cannot be loaded as a whole without moving a node of block 0 -- its first and last
    # element are, through pushed pairs; 240 and 255 see half the strain and stay elastic, the rest of block 0 is quiet)
    T['quiet0_272'] = (17, [('A', 17)], {'A': START_CARRY}, [], [(16, 0), (17, 0), (16, N), (17, N)])
    T['quiet0_512'] = (32, [('A', 32)], {'A': START_CARRY}, _rect(17, 20), [])
    # 3. single loaded elements at the block edges with quiet neighbours on both sides: 255 = (15, 15) through the top nodes of
    # columns 15 | 16, 256 = (16, 0) through the bottom nodes of 16 | 17 -- likewise 63 | 64 (inside a block: a wave edge),
    # 511 | 512 and the last element.  254, 257, 62, 65 and the element before the last one are quiet
    edge = [(3, N), (4, N), (4, 0), (5, 0), (15, N), (16, N), (16, 0), (17, 0)]
    T['edges_512'] = (32, [('A', 32)], {'A': START_CARRY}, [], edge + [(31, N), (32, N)])
    T['edges_784'] = (49, [('A', 49)], {'A': START_CARRY}, [], edge + [(31, N), (32, N), (32, 0), (33, 0), (48, N), (49, N)])
    # 4. [A | foreign | A], the foreign section spanning block 1 and one column more: the third section starts quiet, so its
    # first elements take the modulus of element 255 across a block that holds no element of A at all
    for key in ('el', 'j2'):
        T['laminate_%s_784' % key] = (49, [('A', 16), (key, 17), ('A', 16)], {'A': START_CARRY},
                                      _rect(13, 20) + _rect(30, 33) + _rect(42, 45), [])
    # 5. two work-hardening objects in alternating sections (10 | 14 | 12 | 13 columns) with different start carries: quiet
    # columns at the start of every section but the first, so each chain reaches back across the other object's section
    T['two_objects_784'] = (49, [('A', 10), ('B', 14), ('A', 12), ('B', 13)], {'A': START_CARRY, 'B': 77.25},
                            _rect(3, 5) + _rect(15, 17) + _rect(28, 30) + _rect(41, 43), [])
    return T


CHAIN_CASES = tuple(_chain_table())


class ChainCase(object):
    """One designed sweep: the meshed façade model, the state to upload and what the reference's element loop makes of it."""

    def __init__(self, name, zc=None, seed=0):
        import pylabfea_amd as FE
        zc = golden('svc_workhard_chain.npz') if zc is None else zc
        self.name = name
        NX, sections, carry, active, pushed = _chain_table()[name]
        self.NX, self.NY = NX, NY_CHAIN
        objs = {}
        for key, _ in sections:
            if key in objs:
                continue
            if key in ('A', 'B'):
                objs[key] = wh_material(zc, name=key, num=len(objs) + 1)
            elif key == 'el':
                objs[key] = FE.Material(name='elastic', num=len(objs) + 1)
                objs[key].elasticity(E=150.e3, nu=0.25)
            else:
                objs[key] = FE.Material(name='J2', num=len(objs) + 1)
                objs[key].elasticity(E=200.e3, nu=0.3)
                objs[key].plasticity(sy=60., khard=1000., sdim=6)
        fe = FE.Model(dim=2)
        fe.geom([float(n) for _, n in sections], LY=float(NY_CHAIN))         # unit squares
        fe.assign([objs[key] for key, _ in sections])
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(0.004 * fe.leny, 'disp')
        fe.mesh(NX=NX, NY=NY_CHAIN)
        self.fe = fe
        self.nel = fe.Nel
        self.ref = RefSolver(fe)                                             # definitions only: mesh arrays, CVs, oracle materials
        # the engine numbers its materials by first occurrence among the DISTINCT objects (Model._ensure_engine), the oracle
        # by the first index in fe.mat (RefSolver): per element, and per work-hardening object
        uniq = []
        for m in fe.mat:
            if not any(m is q for q in uniq):
                uniq.append(m)
        self.engine_mat = {key: next(i for i, q in enumerate(uniq) if q is objs[key]) for key in objs}
        self.oracle_mat = {key: next(i for i, q in enumerate(fe.mat) if q is objs[key]) for key in objs}
        self.wh_keys = [key for key in objs if key in ('A', 'B')]
        self.start_carry = dict(carry)
        self.obj_of_el = np.full(self.nel, -1)                               # index into wh_keys, -1: a foreign element
        for i, key in enumerate(self.wh_keys):
            self.obj_of_el[self.ref.mat_id == self.oracle_mat[key]] = i
        # Displacement increment: zero but on the active and the pushed nodes, from the virgin state.  Active nodes carry a
        # checkerboard, u_x = a (j mod 2 + 0.05 r), u_y = -a ((k + 1) mod 2 + 0.05 r'), a = 1.3 sy / E on unit squares: the elements
        # between them see (+-a, -+a) or (+-a, +-a), all of them far beyond the yield locus of this fit, the
        # elements between an active and a resting node column a mixture with shear.  Pushed pairs: both nodes move by a along x and
        # y towards the centre of the ONE element that holds both: (-a, -a) there, plastic; (a / 2, -a / 2) without shear on its
        # two neighbours in the row, which stay elastic.
        sy, E = float(zc['par_sy']), float(zc['par_E'])
        a = 1.3 * sy / E
        rng = np.random.default_rng(1000 + seed)
        r = rng.standard_normal((NX + 1, NY_CHAIN + 1, 2))
        jj, kk = np.meshgrid(np.arange(NX + 1), np.arange(NY_CHAIN + 1), indexing='ij')
        g = np.zeros((NX + 1, NY_CHAIN + 1, 2))
        on = np.zeros((NX + 1, NY_CHAIN + 1), dtype=bool)
        for j, k in active:
            on[j, k] = True
        g[:, :, 0] = a * (jj % 2 + 0.05 * r[:, :, 0])
        g[:, :, 1] = -a * ((kk + 1) % 2 + 0.05 * r[:, :, 1])
        g[~on] = 0.
        for n in range(0, len(pushed), 2):
            (j, k), (j1, k1) = pushed[n], pushed[n + 1]
            assert j1 == j + 1 and k1 == k and k in (0, NY_CHAIN)
            g[j, k] = a * np.array([1. + 0.05 * r[j, k, 0], (-1. if k else 1.) * (1. + 0.05 * r[j, k, 1])])
            g[j1, k] = a * np.array([-1. + 0.05 * r[j1, k, 0], (-1. if k else 1.) * (1. + 0.05 * r[j1, k, 1])])
            on[j, k] = on[j1, k] = True
        self.du = g.reshape(-1)                                              # node j * (NY + 1) + k, DOFs 2 n, 2 n + 1
        self.active = on
        ej, ek = np.divmod(np.arange(self.nel), NY_CHAIN)
        self.quiet = ~(on[ej, ek] | on[ej, ek + 1] | on[ej + 1, ek] | on[ej + 1, ek + 1])
        self.sig = np.zeros((self.nel, 6))
        self.epl = np.zeros((self.nel, 6))
        self.seeded_khard = 50. + 400. * np.random.default_rng(2000 + seed).random(self.nel)   # a second guess of the entry moduli
        self._out = None

    def carry_by_oracle_mat(self):
        c = np.array([0. if m.khard is None else float(m.khard) for m in self.fe.mat])   # (as RefSolver.solve starts them)
        for key in self.wh_keys:
            c[self.oracle_mat[key]] = self.start_carry[key]
        return c

    def deps(self):
        return self.ref.strain(self.du)

    def reference(self):
        """the reference's element loop on one mutable object per material (O.response_wh, sequential=True): dict with the
        exit modulus per element (kpt), per object (kout, keyed like start_carry), res_sig, res_depl, nsteps"""
        if self._out is None:
            r = self.ref
            fy, so, dp, ct, ns, kout, kpt = O.response_wh(r.mats, r.CVs, self.sig, self.epl, self.deps(),
                                                          khard_in=self.carry_by_oracle_mat(), mat_id=r.mat_id, sequential=True)
            self._out = dict(fy=fy, res_sig=so, res_depl=dp, nsteps=ns, kpt=kpt,
                             kout={key: kout[self.oracle_mat[key]] for key in self.wh_keys})
        return self._out

    def per_point(self):
        """exit moduli if every point started from its object's start carry instead (the per-point contract)"""
        r = self.ref
        kin = self.carry_by_oracle_mat()[r.mat_id]
        return O.response_wh(r.mats, r.CVs, self.sig, self.epl, self.deps(), khard_in=kin, mat_id=r.mat_id)[5]

    def chain_walk(self, kh, check=None):
        """Walk exit moduli `kh` in element order, object by object: the running modulus starts at the start carry and becomes
        kh[e] at every element that is not quiet and holds another value (a call that evaluates a gradient overwrites the
        modulus; one that does not leaves its entry value as its exit value).  Returns (entry modulus per element, NaN on
        foreign elements; touched flags; last modulus per object).  check(e, entry): called on every quiet element."""
        entry = np.full(self.nel, np.nan)
        touched = np.zeros(self.nel, dtype=bool)
        last = {}
        for i, key in enumerate(self.wh_keys):
            run = self.start_carry[key]
            for e in np.nonzero(self.obj_of_el == i)[0]:
                entry[e] = run
                if self.quiet[e]:
                    if check is not None:
                        check(int(e), run)
                elif kh[e] != run:
                    touched[e] = True
                    run = kh[e]
            last[key] = run
        return entry, touched, last


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """the case and its reference, built once per process and shared (nobody may change it)"""
    c = ChainCase(name)
    c.reference()
    return c


def quiet_runs(case):
    """[(object key, predecessor or None, elements of the run)]: maximal runs of quiet elements in the element order of one
    object, with the last touched element of that object before the run (reference's touched flags)"""
    kpt = case.reference()['kpt']
    touched = case.chain_walk(kpt)[1]
    out = []
    for i, key in enumerate(case.wh_keys):
        last, run = None, []
        for e in np.nonzero(case.obj_of_el == i)[0]:
            if case.quiet[e]:
                run.append(int(e))
                continue
            if run:
                out.append((key, last, run))
                run = []
            if touched[e]:
                last = int(e)
        if run:
            out.append((key, last, run))
    return out


def chain_python_loop(case):
    """the chain restated point by point: O.response_wh on ONE point with an explicit entry modulus, the exit modulus carried by
    hand to the next point of the same object"""
    r = case.ref
    carry = case.carry_by_oracle_mat()
    deps = case.deps()
    kpt = np.zeros(case.nel)
    for e in range(case.nel):
        m = int(r.mat_id[e])
        if r.mats[m].c.kind != O.SVC_WH:
            continue
        out = O.response_wh(r.mats[m], r.CVs[m], case.sig[e], case.epl[e], deps[e], khard_in=[carry[m]])
        carry[m] = kpt[e] = out[5][0]
    return kpt, carry


# ------------------------------------------------------------------------------------------------ B: calc_scf statistics
TAU = 1e-9            # the analytic point kernels' bar, on hh <= 1
SCF_SIZES = {144: (12, 12), 255: (17, 15), 256: (16, 16), 257: (257, 1), 784: (49, 16), 262656: (513, 512)}


def hill_material(name='hill6', num=1):
    import pylabfea_amd as FE
    z = golden('material_hill6.npz')
    m = FE.Material(name=name, num=num)
    m.elasticity(E=float(z['par_E']), nu=float(z['par_nu']))
    m.plasticity(sy=float(z['par_sy']), hill=[float(x) for x in z['par_hill']], khard=float(z['par_khard']), sdim=6,
                 drucker=float(z['par_dp'][0]))
    return m


def scf_model(nel, laminate=False):
    """NX x NY unit-square elements of the analytic Hill material; laminate: [Hill | elastic | the same Hill object]"""
    import pylabfea_amd as FE
    NX, NY = SCF_SIZES[nel]
    m = hill_material()
    fe = FE.Model(dim=2)
    if laminate:
        el = FE.Material(name='elastic', num=2)
        el.elasticity(E=150.e3, nu=0.25)
        n1, n2 = (2 * NX) // 5, NX // 4                                       # 49 columns: 19 | 12 | 18, no block of 256 all elastic
        fe.geom([float(n1), float(n2), float(NX - n1 - n2)], LY=float(NY))
        fe.assign([m, el, m])
    else:
        fe.geom([float(NX)], LY=float(NY))
        fe.assign([m])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.004 * fe.leny, 'disp')
    fe.mesh(NX=NX, NY=NY)
    return fe


SLD = np.array([0., 1., 0., 0., 0., 0.])


class ScfCase(object):
    """State for one calc_scf evaluation and the list RefSolver.scf_list makes of it.

    du: u_x = a (j mod 2) (1 + 0.2 r), u_y = -0.6 a (k mod 2) (1 + 0.2 r') with a chosen so that the trial stress increment of a
    full element is about 1.4 flow stresses; on the nodes with k mod 8 in {3, 4}, or j mod 8 in {3, 4} and k mod 4 in {0, 1}, it is 1e-10 of
    that, so the elements with k mod 8 == 3, or j mod 8 == 3 and k mod 4 == 0, have sref ~ 1e-8 <= 0.1 and are not counted
    (mult 0) -- some in every block of 256 of every mesh of SCF_SIZES, and never a whole block.
    epl: seeded, on every third element.  sig: a seeded direction scaled to a prescribed equivalent stress -- on the odd
    counted elements 0.02 .. 0.04 below the flow stress (yf0 > -0.15: the flow-stress ratio, appended once), on the even ones
    deep inside (yf0 < -0.15: -yf0 / sref, appended twice) with the ratio aimed at 0.35 .. 0.55, and at 0.2 on element `emin`."""

    def __init__(self, fe, emin=0, seed=0):
        self.fe = fe
        r = self.ref = RefSolver(fe)
        nel, NX, NY = fe.Nel, fe._NX, fe._NY
        rng = np.random.default_rng(3000 + seed)
        hill = next(m for m in fe.mat if m.sy is not None)
        om = r.mats[next(i for i, m in enumerate(fe.mat) if m is hill)]
        sy, E = hill.sy, hill.E
        a = 1.4 * sy / E
        jj, kk = np.meshgrid(np.arange(NX + 1), np.arange(NY + 1), indexing='ij')
        g = np.zeros((NX + 1, NY + 1, 2))
        g[:, :, 0] = a * (jj % 2) * (1. + 0.2 * rng.uniform(-1., 1., jj.shape))
        g[:, :, 1] = -0.6 * a * (kk % 2) * (1. + 0.2 * rng.uniform(-1., 1., jj.shape))
        small = np.isin(kk % 8, (3, 4)) | (np.isin(jj % 8, (3, 4)) & np.isin(kk % 4, (0, 1)))
        g[small] = 1.e-10 * a * rng.uniform(-1., 1., (int(small.sum()), 2))
        self.du = g.reshape(-1)
        epl = np.zeros((nel, 6))
        w = rng.standard_normal((nel, 6)) * 1.e-3
        w[:, :3] -= w[:, :3].mean(axis=1)[:, None]
        epl[::3] = w[::3]
        self.epl = epl
        r.sig = np.zeros((nel, 6))
        r.epl = epl
        r.elstiff = np.array(r.CVs[r.mat_id])
        r.khard_mat = np.array([0. if mm.khard is None else float(mm.khard) for mm in fe.mat])
        deps = r.strain(self.du)
        dsig = np.einsum('eij,ej->ei', r.elstiff.reshape(-1, 6, 6), deps)
        sref = O.calc_seq(om, dsig)
        sflow = r.sflow(epl)
        # designed branch: 0 not counted (or elastic), 1 near the locus, 2 deep inside
        counted = r.plastic & (sref > 0.1)
        branch = np.where(counted, np.where(np.arange(nel) % 2 == 1, 1, 2), 0)
        if counted[emin]:
            branch[emin] = 2
        target = rng.uniform(0.35, 0.55, nel)
        target[emin] = 0.2
        seq = np.where(branch == 1, sflow - rng.uniform(0.02, 0.04, nel), sflow - target * sref)
        d = rng.standard_normal((nel, 6))
        d /= O.calc_seq(om, d)[:, None]
        self.sig = d * np.where(branch == 0, 0.5 * np.maximum(sflow, sy), seq)[:, None]
        r.sig = self.sig
        self.emin = emin
        self.sref, self.sflow, self.branch = sref, sflow, branch
        self.yf0 = np.where(r.plastic, O.calc_yf(om, self.sig, epl), 0.)
        self.mult = np.where(counted, np.where(self.yf0 < -0.15, 2, 1), 0)
        self.hh = np.where(self.mult == 2, np.minimum(1., -self.yf0 / np.maximum(sref, 1e-300)),
                           np.minimum(1., np.sqrt(1.5) * sflow / np.maximum(sref, 1e-300)))
        self.list = r.scf_list(self.du, SLD)                                 # the reference's own steps (oracle/solve_ref.py)

    def stats(self):
        """(count, min, sum, centred sum of squares) of the list, sums by math.fsum"""
        sc = self.list
        s = math.fsum(sc)
        mean = s / len(sc)
        return len(sc), min(sc), s, math.fsum((h - mean) ** 2 for h in sc)


# ------------------------------------------------------------------------------------------------ C: the 18 element sums
SUM_SIZES = {1: (1, 1), 255: (17, 15), 256: (16, 16), 257: (257, 1), 784: (49, 16), 262656: (513, 512), 524800: (1025, 512)}


def sums_model(nel):
    """two sections of lengths 1 and 2.3 with the same Hill material: the element volume differs by section (one element: one
    section)"""
    import pylabfea_amd as FE
    NX, NY = SUM_SIZES[nel]
    m = hill_material()
    fe = FE.Model(dim=2)
    if NX == 1:
        fe.geom([0.7], LY=1.3)
        fe.assign([m])
    else:
        fe.geom([1., 2.3], LY=1.3)
        fe.assign([m, m])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.004 * fe.leny, 'disp')
    fe.mesh(NX=NX, NY=NY)
    return fe


def sums_state(nel, seed=0):
    """sig, eps, epl [nel, 6]: random signs, magnitudes in [0.5, 1.5], one seed per field and component"""
    out = []
    for f in range(3):
        x = np.empty((nel, 6))
        for k in range(6):
            rng = np.random.default_rng(4000 + 100 * seed + 6 * f + k)
            x[:, k] = rng.uniform(0.5, 1.5, nel) * rng.choice([-1., 1.], nel)
        out.append(x)
    return out


def element_volumes(fe):
    lxy = fe._lxy
    return lxy[:, 0] * lxy[:, 1] * fe.thick                                 # Element.Vel (model.py:316), in this order


def sums_reference(fields, vel):
    """(fsum(x[:, k] * vel), gauge fsum(|x[:, k] * vel|)) as [3, 6] arrays"""
    s, g = np.empty((3, 6)), np.empty((3, 6))
    for f, x in enumerate(fields):
        for k in range(6):
            t = x[:, k] * vel
            s[f, k] = math.fsum(t)
            g[f, k] = math.fsum(np.abs(t))
    return s, g


def sums_depth(nel):
    """Roundings on the longest path of the device's summation of one component (k_global_partials -> k_reduce_rows, the same
    order in k_update_state<1> -> k_finish_out), counted from the code:
      g = min(ceil(nel / 256), 2048) blocks; ceil(nel / (256 g)) fma terms per thread (grid-stride loop, one rounding each);
      6 levels of the wave sum; 4 wave results added in turn; then k_reduce_rows: ceil(g / 256) partials per thread, 6 wave
      levels, 4 wave results;
    plus 2 on the reference's side: it rounds the product x * vel that the device's fma keeps exact, and fsum rounds once."""
    g = min(-(-nel // BLOCK), SUM_CAP)
    return -(-nel // (BLOCK * g)) + 6 + 4 + -(-g // BLOCK) + 6 + 4 + 2
