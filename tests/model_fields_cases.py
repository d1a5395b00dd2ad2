"""The models of tests/golden/model_fields.npz (helper module, no tests): ``build(FE, name)`` makes case ``name`` with the
package ``FE`` -- the reference in tools/gen_model_fields.py, pylabfea_amd in the tests -- ready for ``solve()``."""
import numpy as np

CASES = {
    'a': dict(solve=True),    # 5 x 3 laminate: Hill-6 | J2 with sdim 3 | elastic, tension
    'b': dict(solve=True),    # 7 x 6 elmts map: Hill inclusion and a Drucker material in a J2 matrix, top moved in y and x
    'c': dict(solve=False),   # case a before any solve
    'd': dict(solve=True),    # elastic two-material laminate (linear path)
}


def _mat(FE, num, E, nu, **plastic):
    m = FE.Material(num=num)
    m.elasticity(E=E, nu=nu)
    if plastic:
        m.plasticity(**plastic)
    return m


def materials(FE, name):
    if name in ('a', 'c'):
        return [_mat(FE, 1, 200.e3, 0.3, sy=100., hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6),
                _mat(FE, 2, 200.e3, 0.3, sy=150., khard=1000., sdim=3),
                _mat(FE, 3, 50.e3, 0.25)]
    if name == 'b':
        return [_mat(FE, 1, 200.e3, 0.3, sy=150., khard=1000., sdim=6),
                _mat(FE, 2, 150.e3, 0.3, sy=80., hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=500., sdim=6),
                _mat(FE, 3, 200.e3, 0.3, sy=120., drucker=0.1, khard=1000., sdim=6)]
    return [_mat(FE, 1, 200.e3, 0.3), _mat(FE, 2, 70.e3, 0.33)]


def elmts_b():
    el = np.ones((7, 6), dtype=int)
    el[2:5, 2:4] = 2       # the softer Hill inclusion
    el[5, 1:5] = 3         # a strip of the Drucker material
    el[0, 5] = 3
    return el


def build(FE, name):
    fe = FE.Model(dim=2, planestress=False)
    mats = materials(FE, name)
    if name in ('a', 'c'):
        fe.geom([2, 1, 2], LY=3.)
        fe.assign(mats)
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(0.004 * fe.leny, 'disp')
        fe.mesh(NX=5, NY=3)
    elif name == 'b':
        fe.geom(sect=3, LX=7., LY=6.)
        fe.assign(mats)
        fe.bcleft(0., 'force')
        fe.bcbot(0., 'disp', 'x')
        fe.bcbot(0., 'disp', 'y')
        fe.bcright(0., 'force')
        fe.bctop(0.003 * fe.leny, 'disp', 'y')
        fe.bctop(0.002 * fe.leny, 'disp', 'x')
        fe.mesh(elmts=elmts_b())
    else:
        fe.geom([1, 2], LY=4.)
        fe.assign(mats)
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(0.002 * fe.leny, 'disp')
        fe.mesh(NX=6, NY=4)
    return fe
