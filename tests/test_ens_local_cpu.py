"""CPU checks of the localized observation update (ocn_ens_local_update): the numpy restatement the GPU
tests compare against (tests/ens_local_ref.py) is checked against an independent scalar triple loop over
Python floats, the properties the contract promises are checked on it, the serial filter built on it is
checked against the scalar Kalman update in extended precision, and the entry's errors that need no
device are exercised."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import ens_local_ref as R

ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    import ocean_model_arch_amd as amd
    if not os.path.exists(amd._lib.LIB_PATH):
        amd.build()
    return amd.lib()


# a 9 x 7 array whose first point is global (3, 2)
GI, GJ = np.arange(3, 12), np.arange(2, 9)


def _members(n, seed=91):
    """n members of the 9 x 7 array, O(1), with signed zeros and denormals among them."""
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 9, 7))
    x[0, 3, 2], x[1, 3, 2] = -0.0, 0.0
    x[:, 5, 5] = -0.0                          # every member -0.0: the sum keeps the sign
    x[0, 6, 1], x[n - 1, 6, 1] = 5e-324, -3e-320
    x[:, 8, 6] = [(-1) ** m * 1e-310 for m in range(n)]
    return x


def _obs(n, nobs, seed):
    """Observations inside the array, on its edge and outside it (one far away), two at one point, and a
    taper with interior zeros of both signs."""
    rng = np.random.default_rng(seed)
    io, jo = rng.integers(1, 15, nobs), rng.integers(1, 12, nobs)
    io[0], jo[0] = 3, 2
    io[1], jo[1] = io[2], jo[2] = 7, 5
    io[3], jo[3] = 40, 40
    y, z = R.rows(nobs, n, seed + 1)
    y[4, 0], z[4, 1] = 0.0, -0.0
    y[5] *= 1e-310                             # denormal rows
    taper = np.array([1.0, 0.9, 0.0, 0.7, 0.6, -0.0, 0.0, 0.0, 0.3, 0.25, 1e-310, 0.1, 0.05])
    return io, jo, y, z, taper


def _scalar(x, gi, gj, io, jo, y, z, taper):
    """The contract with Python floats (IEEE doubles): one point, one observation, one member at a time."""
    n = len(x)
    out = np.array(x, dtype=np.float64, copy=True)
    for a in range(len(gi)):
        for b in range(len(gj)):
            v = [float(out[m, a, b]) for m in range(n)]
            for k in range(len(io)):
                d2 = (int(gi[a]) - int(io[k])) ** 2 + (int(gj[b]) - int(jo[k])) ** 2
                if d2 >= len(taper):
                    continue
                rho = float(taper[d2])
                if rho == 0.0:
                    continue
                s = v[0]
                for m in range(1, n):
                    s = s + v[m]
                mean = s / float(n)
                acc = (v[0] - mean) * float(y[k, 0])
                for m in range(1, n):
                    p = (v[m] - mean) * float(y[k, m])
                    acc = acc + p
                g = rho * acc
                v = [v[m] + g * float(z[k, m]) for m in range(n)]
            for m in range(n):
                out[m, a, b] = v[m]
    return out


def _same(got, want):
    return len(got) == len(want) and all(R.bits_equal(g, v) for g, v in zip(got, want))


@pytest.mark.parametrize("n", [2, 3, 8, 9])
def test_restatement_matches_scalar_loop(n):
    x = _members(n)
    io, jo, y, z, taper = _obs(n, 14, 10 * n)
    want = _scalar(x, GI, GJ, io, jo, y, z, taper)
    got = R.local_rule(list(x), GI, GJ, io, jo, y, z, taper)
    assert _same(got, want)
    # the same points as a scattered list take the other branch of the restatement
    pi, pj = np.meshgrid(GI, GJ, indexing="ij")
    pts = R.local_rule([a.ravel() for a in x], pi.ravel(), pj.ravel(), io, jo, y, z, taper)
    assert _same([a.reshape(9, 7) for a in pts], want)
    # a table of one entry reaches the observed point alone; one longer than the array's diagonal, all of it
    for t in (np.array([0.5]), np.linspace(1.0, 0.1, 9 * 9 + 7 * 7 + 40 * 40 * 2)):
        assert _same(R.local_rule(list(x), GI, GJ, io, jo, y, z, t), _scalar(x, GI, GJ, io, jo, y, z, t))


def test_unreached_points_and_inputs_keep_their_bits():
    x = _members(5)
    keep = x.copy()
    io, jo, y, z, _ = _obs(5, 6, 3)
    got = R.local_rule(list(x), GI, GJ, io[:1], jo[:1], y[:1], z[:1], np.array([1.0, 0.5]))
    assert R.bits_equal(x, keep)               # the inputs are not written
    reached = np.zeros((9, 7), dtype=bool)
    reached[0, 0] = reached[1, 0] = reached[0, 1] = True    # d2 = 0 and 1 around global (3, 2)
    for m in range(5):
        assert R.bits_equal(got[m][~reached], x[m][~reached])
        assert (got[m][reached] != x[m][reached]).all()
    zero = R.local_rule(list(x), GI, GJ, io, jo, y, z, np.array([0.0, -0.0, 0.0]))
    assert _same(zero, x)                       # a taper of zeros: nothing formed, -0.0 and denormals kept


def test_composition():
    """L1 then L2 gives the bits of L1 followed by L2."""
    n = 7
    x = _members(n)
    io, jo, y, z, taper = _obs(n, 40, 77)
    one = R.local_rule(list(x), GI, GJ, io, jo, y, z, taper)
    half = R.local_rule(list(x), GI, GJ, io[:17], jo[:17], y[:17], z[:17], taper)
    two = R.local_rule(half, GI, GJ, io[17:], jo[17:], y[17:], z[17:], taper)
    assert _same(one, two)


def analytic_check(prior, post, value, r):
    """The scalar Kalman update at one observed point, in numpy.longdouble from the prior members: the
    posterior mean is m + s / (s + r) (v - m) and the posterior variance s r / (s + r).  Returns the two
    relative errors of `post`."""
    L = np.longdouble
    p, q = np.asarray(prior, dtype=L), np.asarray(post, dtype=L)
    n = len(p)
    m = p.sum() / n
    s = ((p - m) ** 2).sum() / (n - 1)
    want_mean = m + s / (s + L(r)) * (L(value) - m)
    want_var = s * L(r) / (s + L(r))
    qm = q.sum() / n
    qv = ((q - qm) ** 2).sum() / (n - 1)
    return float(abs(qm - want_mean) / abs(want_mean)), float(abs(qv - want_var) / want_var)


# the single-observation case of the filter, shared with tests/test_gpu_ens_local.py: 8 members, values
# O(1) (the prior mean kept away from 0 so that the relative error of the mean means something)
ANALYTIC_TOL = 1e-12   # about 6 n rounded operations on well-conditioned O(1) data, ~1e-14, times 100
ANALYTIC_VALUE, ANALYTIC_VAR = 1.75, 0.09


def test_single_observation_is_the_scalar_kalman_update():
    n = 8
    x = np.random.default_rng(5).uniform(0.5, 1.5, (n, 9, 7))
    ij = np.array([[6, 4]])
    a, b = 6 - GI[0], 4 - GJ[0]
    Y, Z, info = R.ensrf_obs_space(x[:, a, b][None, :], ij, [ANALYTIC_VALUE], [ANALYTIC_VAR], np.array([1.0]))
    got = R.local_rule(list(x), GI, GJ, ij[:, 0], ij[:, 1], Y, Z, np.array([1.0]))
    post = np.array([g[a, b] for g in got])
    em, ev = analytic_check(x[:, a, b], post, ANALYTIC_VALUE, ANALYTIC_VAR)
    print(f"relative error of the posterior mean {em:.3e}, of the posterior variance {ev:.3e}")
    assert em <= ANALYTIC_TOL and ev <= ANALYTIC_TOL
    assert R.bits_equal(info["hx"][0], post)    # the filter followed the observed point with the same rule
    other = np.ones((9, 7), dtype=bool)
    other[a, b] = False
    assert all(R.bits_equal(g[other], v[other]) for g, v in zip(got, x))


def test_obs_space_loop_follows_the_fields():
    """After several tapered observations the rows the filter kept are the fields' values at the observed
    points, bit for bit, repeated points and points out of each other's reach included."""
    n = 6
    x = _members(n, seed=8) + 1.0
    ij = np.array([[4, 3], [8, 6], [4, 3], [10, 7], [5, 3], [3, 2]])
    taper = R.taper_table(4.0)
    hx = np.array([[x[m, i - GI[0], j - GJ[0]] for m in range(n)] for i, j in ij])
    Y, Z, info = R.ensrf_obs_space(hx, ij, np.linspace(0.5, 1.5, len(ij)), np.full(len(ij), 0.04), taper)
    got = R.local_rule(list(x), GI, GJ, ij[:, 0], ij[:, 1], Y, Z, taper)
    after = np.array([[got[m][i - GI[0], j - GJ[0]] for m in range(n)] for i, j in ij])
    assert R.bits_equal(info["hx"], after)
    assert (info["posterior_spread"] < info["prior_spread"]).all()


@pytest.mark.parametrize("radius", [0.0, 1.0, 2.5, 6.0, 10.0, 100.0, 256.0])
def test_taper_table(radius):
    from ocean_model_arch_amd import ensemble
    t = ensemble.taper_table(radius)
    assert t.dtype == np.float64 and t.ndim == 1 and 1 <= len(t) <= 65536
    assert t[0] == 1.0
    assert len(t) == max(1, math.ceil(radius * radius))      # compact: no entry at `radius` or beyond
    assert np.isfinite(t).all() and (t >= 0.0).all() and (np.diff(t) <= 0.0).all()
    if radius >= 6.0:
        assert t[-1] < 1e-3 and t[1] > 0.5
    box = ensemble.taper_table(radius, kind="boxcar")
    assert len(box) == len(t) and (box == 1.0).all()
    with pytest.raises(ValueError):
        ensemble.taper_table(radius, kind="cone")


def test_taper_table_is_gaspari_cohn():
    """Against the published values of the function at c = radius / 2: 1 at 0, 5/24 + ... at r = c."""
    t = R.taper_table(10.0)
    # at distance c = 5 (d2 = 25): -1/4 + 1/2 + 5/8 - 5/3 + 1 = 5/24
    assert abs(t[25] - 5.0 / 24.0) < 1e-15
    with pytest.raises(ValueError):
        R.taper_table(300.0)


def test_prototype_and_null_ensemble(lib):
    from ocean_model_arch_amd import _lib
    assert lib.ocn_abi_version() == 5
    assert "ocn_ens_local_update" in _lib.ENS_SYMBOLS
    assert len(lib.ocn_ens_local_update.argtypes) == 11
    one = (C.c_int32 * 1)(1)
    d = (C.c_double * 2)(1.0, 1.0)
    assert lib.ocn_ens_local_update(None, one, 1, None, 1, one, one, d, d, d, 1) == ERR_ARG
    assert lib.ocn_ens_local_update(None, None, 1, None, 1, None, None, None, None, None, 1) == ERR_ARG
    assert b"ens_local_update" in lib.ocn_last_error()


def test_wrapper_names_the_state():
    from ocean_model_arch_amd import ensemble
    assert ensemble.STATE == R.STATE
