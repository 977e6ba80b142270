"""CPU checks of the serial filter on the device (ocn_ens_assimilate): the numpy restatement the GPU tests
compare against (tests/ens_assim_ref.py) is checked bit for bit against a plain scalar loop over Python
floats, its rows are shown to follow the fields under the update's rule, its single-observation case is the
scalar Kalman update, and what the entries do without a device is exercised.

Nothing here compares the ordered loop with `ensrf_obs_space`: the two differ in the order of two sums, and
whether numpy's order happens to give the same bits at some member count is no property of either."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import ens_assim_ref as A
from tests.test_ens_local_cpu import ANALYTIC_TOL, ANALYTIC_VALUE, ANALYTIC_VAR, GI, GJ, _members, analytic_check

ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    import ocean_model_arch_amd as amd
    if not os.path.exists(amd._lib.LIB_PATH):
        amd.build()
    return amd.lib()


def _case(n, seed=21):
    """12 observations of an O(1) ensemble with a spread of a few tenths, one point observed twice."""
    rng = np.random.default_rng(seed + n)
    ij = np.stack([rng.integers(1, 30, 12), rng.integers(1, 12, 12)], axis=1)
    ij[7] = ij[3]
    hx = 1.0 + rng.uniform(-0.3, 0.3, (12, n))
    hx[2, 0], hx[2, 1] = -0.0, 0.0
    values = hx.mean(axis=1) + rng.uniform(-0.1, 0.1, 12)
    variances = rng.uniform(0.005, 0.05, 12)
    return hx, ij, values, variances


def _spread_scalar(row):
    n = len(row)
    s = row[0]
    for m in range(1, n):
        s = s + row[m]
    mean = s / float(n)
    d = row[0] - mean
    q = d * d
    for m in range(1, n):
        d = row[m] - mean
        q = q + d * d
    return math.sqrt(q / float(n - 1))


def _scalar(hx, ij, values, variances, taper):
    """The contract with Python floats (IEEE doubles): one observation, one row, one member at a time."""
    nobs, n = hx.shape
    rows = [[float(v) for v in r] for r in hx]
    taper = [float(t) for t in taper]
    prior = [_spread_scalar(r) for r in rows]
    Y, Z, innov = [], [], []
    for k in range(nobs):
        x = rows[k]
        s1 = x[0]
        for m in range(1, n):
            s1 = s1 + x[m]
        ybar = s1 / float(n)
        yp = [x[m] - ybar for m in range(n)]
        q = yp[0] * yp[0]
        for m in range(1, n):
            p = yp[m] * yp[m]
            q = q + p
        s = q / float(n - 1)
        r = float(variances[k])
        D = s + r
        d = float(values[k]) - ybar
        t = r / D
        alpha = 1.0 / (1.0 + math.sqrt(t))
        c = float(n - 1) * D
        zk = [(d - alpha * yp[m]) / c for m in range(n)]
        Y.append(yp)
        Z.append(zk)
        innov.append(d)
        for j in range(nobs):
            d2 = (int(ij[j, 0]) - int(ij[k, 0])) ** 2 + (int(ij[j, 1]) - int(ij[k, 1])) ** 2
            if d2 >= len(taper) or taper[d2] == 0.0:
                continue
            v = rows[j]
            sj = v[0]
            for m in range(1, n):
                sj = sj + v[m]
            mean = sj / float(n)
            acc = (v[0] - mean) * yp[0]
            for m in range(1, n):
                p = (v[m] - mean) * yp[m]
                acc = acc + p
            g = taper[d2] * acc
            rows[j] = [v[m] + g * zk[m] for m in range(n)]
    post = [_spread_scalar(r) for r in rows]
    return np.array(Y), np.array(Z), {"hx": np.array(rows), "innovations": np.array(innov), "prior_spread": np.array(prior),
                                      "posterior_spread": np.array(post)}


@pytest.mark.parametrize("n", [2, 5, 8, 9, 33])
def test_restatement_matches_scalar_loop(n):
    hx, ij, values, variances = _case(n)
    keep = hx.copy()
    for taper in (A.taper_table(6.0), A.ringed_taper(50), np.array([0.75])):
        Y, Z, info = A.ensrf_obs_space_ordered(hx, ij, values, variances, taper)
        Ys, Zs, want = _scalar(hx, ij, values, variances, taper)
        assert A.bits_equal(Y, Ys) and A.bits_equal(Z, Zs)
        assert not A.info_mismatches(info, want)
        assert info["nonfinite"] == 0
        assert info["hx"].shape == (12, n) and Y.shape == Z.shape == (12, n)
    assert A.bits_equal(hx, keep)               # the input is not written


def test_rows_follow_the_fields():
    """After several tapered observations the rows the ordered loop kept are the fields' values at the
    observed points under the update's rule with its Y and Z, repeated points and points out of each other's
    reach included."""
    n = 6
    x = _members(n, seed=8) + 1.0
    ij = np.array([[4, 3], [8, 6], [4, 3], [10, 7], [5, 3], [3, 2]])
    taper = A.taper_table(4.0)
    hx = np.array([[x[m, i - GI[0], j - GJ[0]] for m in range(n)] for i, j in ij])
    Y, Z, info = A.ensrf_obs_space_ordered(hx, ij, np.linspace(0.5, 1.5, len(ij)), np.full(len(ij), 0.04), taper)
    got = A.local_rule(list(x), GI, GJ, ij[:, 0], ij[:, 1], Y, Z, taper)
    after = np.array([[got[m][i - GI[0], j - GJ[0]] for m in range(n)] for i, j in ij])
    assert A.bits_equal(info["hx"], after)
    assert (info["posterior_spread"] < info["prior_spread"]).all()


def test_single_observation_is_the_scalar_kalman_update():
    n = 8
    x = np.random.default_rng(5).uniform(0.5, 1.5, (n, 9, 7))
    ij = np.array([[6, 4]])
    a, b = 6 - GI[0], 4 - GJ[0]
    Y, Z, info = A.ensrf_obs_space_ordered(x[:, a, b][None, :], ij, [ANALYTIC_VALUE], [ANALYTIC_VAR], np.array([1.0]))
    em, ev = analytic_check(x[:, a, b], info["hx"][0], ANALYTIC_VALUE, ANALYTIC_VAR)
    print(f"relative error of the posterior mean {em:.3e}, of the posterior variance {ev:.3e}")
    assert em <= ANALYTIC_TOL and ev <= ANALYTIC_TOL


def test_nonfinite_propagates_and_is_counted():
    hx, ij, values, variances = _case(5)
    hx[4, 2] = np.nan
    Y, Z, info = A.ensrf_obs_space_ordered(hx, ij, values, variances, np.array([1.0]))
    assert info["nonfinite"] >= 1 and np.isnan(info["innovations"][4]) and np.isnan(info["hx"][4]).all()
    assert np.isfinite(info["hx"][0]).all()     # taper [1.0]: a point poisons its own row only
    for bad in ([0.0], [-1.0], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            A.ensrf_obs_space_ordered(hx[:1], ij[:1], values[:1], bad, np.array([1.0]))
    with pytest.raises(ValueError):
        A.ensrf_obs_space_ordered(hx[:1], ij[:1], [np.inf], variances[:1], np.array([1.0]))


def test_prototypes_and_null_ensemble(lib):
    from ocean_model_arch_amd import _lib
    assert lib.ocn_abi_version() == 5
    for nm, nargs in (("ocn_ens_assimilate", 12), ("ocn_ens_assimilate_info", 2), ("ocn_ens_assimilate_result", 3)):
        assert nm in _lib.ENS_SYMBOLS
        assert len(getattr(lib, nm).argtypes) == nargs
    assert C.sizeof(_lib.OcnEnsAssimInfo) == 16
    assert _lib.ENS_ASSIM == {"hx": 0, "y": 1, "z": 2, "innovations": 3, "prior_spread": 4, "posterior_spread": 5}
    one = (C.c_int32 * 1)(1)
    d = (C.c_double * 2)(1.0, 1.0)
    assert lib.ocn_ens_assimilate(None, 32, one, 1, None, 1, one, one, d, d, d, 1) == ERR_ARG
    assert b"ens_assimilate" in lib.ocn_last_error()
    assert lib.ocn_ens_assimilate(None, 32, None, 1, None, 1, None, None, None, None, None, 1) == ERR_ARG
    info = _lib.OcnEnsAssimInfo()
    assert lib.ocn_ens_assimilate_info(None, C.byref(info)) == ERR_ARG
    assert lib.ocn_ens_assimilate_result(None, 0, d) == ERR_ARG


def test_wrapper_takes_device():
    import inspect
    from ocean_model_arch_amd import ensemble
    p = inspect.signature(ensemble.OceanEnsemble.assimilate).parameters
    assert p["device"].default is False
