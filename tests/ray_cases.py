"""Shared by tests/yield_locus_cases.py and tests/texture_cases.py: what their ray checks have in common whatever the
restatement of the decision function behind them."""
import numpy as np


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=float)))


def march_replay(restate_fn, x0, seen):
    """Status per ray (0 bracket found, 1 none) of the march of yield_scale, replayed with a restatement: from x0 down by
    0.98 while f_L >= 0 (to 0.01 x0), else up by 1.02 while f_L < 0 (to 5 x0).  restate_fn(act, x) -> (f_L, A) at the
    factors x of the rays with the indices act; seen(act, f_L, A) is told every evaluation, so that the caller can judge how
    clear of rounding the decisions were."""
    x0 = np.asarray(x0, dtype=float)
    n = len(x0)
    x = np.array(x0)
    act = np.arange(n)
    f, A = restate_fn(act, x)
    seen(act, f, A)
    down = np.asarray(f >= 0)
    st = np.full(n, -1)
    for _ in range(260):
        act = np.flatnonzero(st < 0)
        if not len(act):
            break
        out = np.where(down[act], x[act] < 0.01 * x0[act], x[act] > 5. * x0[act])
        st[act[out]] = 1
        act = act[~out]
        if not len(act):
            break
        x[act] *= np.where(down[act], 0.98, 1.02)
        f, A = restate_fn(act, x[act])
        seen(act, f, A)
        found = np.where(down[act], f < 0, f >= 0)
        st[act[np.asarray(found)]] = 0
    st[st < 0] = 1
    return st
