"""The filter's three routes against the batch Kalman update (CPU, no device).

Every other comparison of the filter is bitwise against a numpy restatement that lives in the package
(ens_local_rule.py, ens_obs_rule.py, ens_record_rule.py); the scalar update of tests/test_ens_local_cpu.py is the
only mathematics written independently of them, and it covers one observed point.  Here the whole state is
checked: with a taper that is 1.0 over the whole array, a serial square-root filter with uncorrelated
observation errors equals the batch update

    mean  m + P H^T (H P H^T + R)^-1 (y - H m)        covariance  P - P H^T (H P H^T + R)^-1 H P

with P the (n - 1) sample covariance of the stacked fields -- the regression onto unobserved points and other
variables, the carrying of the rows from one observation to the next, and the augmented state of the off-grid and
recorded routes included.  `batch_kalman` is written in numpy.longdouble with a Cholesky solve of its own and
shares no code with the rule modules.

The error of a mean is the worst absolute difference over the largest |mean|, that of a covariance the worst
absolute difference over the largest |P| entry of the prior.  Tolerance: ANALYTIC_TOL (1e-12,
tests/test_ens_local_cpu.py).  Each comparison is repeated against a reference whose variances are scaled by
1.01, which must be off by more than 1e-6: none of them can pass vacuously.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from ocean_model_arch_amd import ens_record_rule
from tests import ens_obs_ref as O
from tests.test_ens_local_cpu import ANALYTIC_TOL

L = np.longdouble
CONTROL_SCALE, CONTROL_MIN = 1.01, 1e-6
COUNTS = (3, 9, 33, 129)

# a 9 x 7 array whose first point is global (3, 2), in a basin of 14 x 10 points
GI, GJ = np.arange(3, 12), np.arange(2, 9)
BLOCK = SimpleNamespace(k=0, bnd_x1=3, bnd_x2=11, bnd_y1=2, bnd_y2=8)
BASIN = (14, 10)
ONES = np.ones(9 * 9 + 7 * 7 + 1)          # len > w^2 + h^2: every observation reaches every point with 1.0


# ---------------------------------------------------------------- the independent reference
def _cholesky(a):
    """The lower factor of a symmetric positive definite longdouble matrix, column by column."""
    n = len(a)
    c = np.zeros((n, n), dtype=L)
    for j in range(n):
        d = a[j, j] - (c[j, :j] * c[j, :j]).sum()
        assert d > 0, "batch_kalman: H P H^T + R is not positive definite"
        c[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            c[i, j] = (a[i, j] - (c[i, :j] * c[j, :j]).sum()) / c[j, j]
    return c


def _solve(c, b):
    """(c c^T)^-1 b for the lower factor c and a matrix b of right-hand sides: forward, then back substitution."""
    n = len(c)
    u = np.zeros(b.shape, dtype=L)
    for i in range(n):
        u[i] = (b[i] - c[i, :i] @ u[:i]) / c[i, i]
    v = np.zeros(b.shape, dtype=L)
    for i in range(n - 1, -1, -1):
        v[i] = (u[i] - c[i + 1:, i] @ v[i + 1:]) / c[i, i]
    return v


def moments(X):
    """The mean and the (n - 1) sample covariance of the columns of X (state, n), in longdouble."""
    X = np.asarray(X, dtype=L)
    n = X.shape[1]
    m = X.sum(axis=1) / n
    A = X - m[:, None]
    return m, A @ A.T / (n - 1)


def _update(m, P, H, values, variances):
    """The batch update of the mean m and the covariance P."""
    H, y, r = np.asarray(H, dtype=L), np.asarray(values, dtype=L), np.asarray(variances, dtype=L)
    PHt = P @ H.T
    c = _cholesky(H @ PHt + np.diag(r))
    return m + PHt @ _solve(c, (y - H @ m)[:, None])[:, 0], P - PHt @ _solve(c, PHt.T)


def batch_kalman(X, H, values, variances):
    """The batch Kalman update of the ensemble X (state, n) -- the stacked fields, one column per member -- under
    the dense observation matrix H (nobs, state), the observed values and their uncorrelated error variances:
    the analysis mean (state,) and covariance (state, state), in numpy.longdouble."""
    return _update(*moments(X), H, values, variances)


def kalman_errors(before, after, H, values, *variances):
    """[(error of the mean, error of the covariance), ...] of the ensemble `after` (state, n) as the analysis of
    `before` under (H, values, v), against the batch update, for each v of `variances` (the moments of both
    ensembles are formed once)."""
    m, P = moments(before)
    gm, gc = moments(after)
    out = []
    for v in variances:
        mean, cov = _update(m, P, H, values, v)
        out.append((float(np.abs(gm - mean).max() / np.abs(mean).max()), float(np.abs(gc - cov).max() / np.abs(P).max())))
    return out


def check(what, before, after, H, values, variances):
    """The comparison, printed, and its control: the same against a reference with the variances scaled by 1.01."""
    (em, ev), (cm, cv) = kalman_errors(before, after, H, values, variances, np.asarray(variances) * CONTROL_SCALE)
    print(f"{what}: error of the mean {em:.3e}, of the covariance {ev:.3e}; with R * {CONTROL_SCALE}: {cm:.3e}, {cv:.3e}")
    assert em <= ANALYTIC_TOL and ev <= ANALYTIC_TOL, (what, em, ev)
    assert cm > CONTROL_MIN and cv > CONTROL_MIN, (what, cm, cv)
    return em, ev


# ---------------------------------------------------------------- the data
def _fields(names, n, seed):
    """{name: the n members' 9 x 7 arrays}, uniform in [0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    return {nm: list(rng.uniform(0.5, 1.5, (n, 9, 7))) for nm in names}


def _stack(fields, names, rows=None):
    """(state, n): the named fields' arrays, raveled and stacked in order, then the rows (nobs, n) if given."""
    parts = [np.stack([a.ravel() for a in fields[nm]], axis=1) for nm in names]
    return np.concatenate(parts + ([] if rows is None else [np.asarray(rows)]), axis=0)


def _values(hx, seed):
    """Values the prior mean + uniform [-0.3, 0.3], variances 0.01 + 0.5 prior variance."""
    rng = np.random.default_rng(seed)
    return hx.mean(axis=1) + rng.uniform(-0.3, 0.3, len(hx)), 0.01 + 0.5 * hx.var(axis=1, ddof=1)


def _at(name, names, i, j):
    """The index of point (i, j) -- global -- of field `name` in the stacked state."""
    return names.index(name) * 63 + (i - GI[0]) * 7 + (j - GJ[0])


# ---------------------------------------------------------------- 1. the grid route
@pytest.mark.parametrize("n", COUNTS)
def test_grid_route(n):
    """ensrf_obs_space_ordered + local_rule: ssh observed at 8 + n % 17 points, one of them twice (with n = 3 more
    observations than n - 1), ssh and ubrtr updated."""
    names = ("ssh", "ubrtr")
    nobs = 8 + n % 17
    rng = np.random.default_rng(100 + n)
    ij = np.stack([rng.integers(3, 12, nobs), rng.integers(2, 9, nobs)], axis=1)
    ij[5] = ij[2]
    assert n != 3 or nobs > n - 1                              # (H P H^T alone is singular there: R carries it)
    f = _fields(names, n, n)
    hx = np.array([[a[i - GI[0], j - GJ[0]] for a in f["ssh"]] for i, j in ij])
    values, variances = _values(hx, 200 + n)
    Y, Z, info = O.ensrf_obs_space_ordered(hx, ij, values, variances, ONES)
    g = {nm: O.local_rule(f[nm], GI, GJ, ij[:, 0], ij[:, 1], Y, Z, ONES) for nm in names}
    H = np.zeros((nobs, 2 * 63))
    for k, (i, j) in enumerate(ij):
        H[k, _at("ssh", names, int(i), int(j))] = 1.0
    check(f"grid route, n = {n}, {nobs} observations", _stack(f, names), _stack(g, names), H, values, variances)
    assert all(not O.bits_equal(a, b) for nm in names for a, b in zip(f[nm], g[nm]))


# ---------------------------------------------------------------- 2. the off-grid route
@pytest.mark.parametrize("n", COUNTS)
def test_off_grid_route(n):
    """ens_obs_ref.analysis with 6 radial velocities cos(theta) u + sin(theta) v of bilinearly interpolated ubrtr and
    vbrtr, updating ssh, ubrtr and vbrtr; H densely from the operator's rows.  The returned hx -- the rows the
    filter carried as an augmented state -- is H of the updated fields."""
    names = ("ssh", "ubrtr", "vbrtr")
    rng = np.random.default_rng(300 + n)
    xy = np.stack([rng.uniform(3.0, 10.99, 6), rng.uniform(2.0, 7.99, 6)], axis=1)
    xy[4] = np.floor(xy[4])                                     # a grid point: a one-term row
    theta = rng.uniform(0.0, 2.0 * np.pi, 6)
    op = O.combine([O.bilinear("ubrtr", xy, shape=BASIN), O.bilinear("vbrtr", xy, shape=BASIN)], [np.cos(theta), np.sin(theta)])
    f = _fields(names, n, 10 + n)
    fields = {nm: {0: f[nm]} for nm in names}
    find = lambda i, j: 0                                       # noqa: E731
    values, variances = _values(O.apply(op, fields, [BLOCK], find), 400 + n)
    hx0, Y, Z, info, after = O.analysis(op, fields, [BLOCK], find, values, variances, ONES, names)
    H = np.zeros((6, 3 * 63))
    for k in range(6):
        for nm, i, j, w in op.row(k):
            H[k, _at(nm, names, i, j)] += w
    g = {nm: after[nm][0] for nm in names}
    check(f"off-grid route, n = {n}", _stack(f, names), _stack(g, names), H, values, variances)
    again = O.apply(op, {nm: {0: g[nm]} for nm in names}, [BLOCK], find)
    eh = float(np.abs(info["hx"].astype(L) - again.astype(L)).max() / np.abs(again).max())
    print(f"off-grid route, n = {n}: the carried rows against H of the updated fields {eh:.3e}")
    assert eh <= ANALYTIC_TOL


# ---------------------------------------------------------------- 3. the recorded route
@pytest.mark.parametrize("n", COUNTS)
def test_recorded_route(n):
    """ens_record_rule.interp rows of a synthetic series (5 records of 4 rows; times at and between the records, a
    row observed twice at one time) as an augmented state: the batch update acts on [fields; rows] with H selecting
    the rows.  The series is correlated with the fields, so that the fields move."""
    names = ("ssh", "ubrtr")
    rng = np.random.default_rng(500 + n)
    f = _fields(names, n, 20 + n)
    ssh = np.stack([a.ravel() for a in f["ssh"]], axis=1)      # (63, n)
    series = np.stack([[0.5 * ssh[7 * r + 3 * t] + 0.5 * rng.uniform(0.5, 1.5, n) for r in range(4)] for t in range(5)])
    at = np.array([1.0, 5.0, 2.5, 3.25, 4.75, 2.5, 1.5, 3.0])
    rows = np.array([0, 3, 1, 2, 0, 1, 3, 2])
    rec, wt = ens_record_rule.at_steps(at, 1, 5)
    hx0 = ens_record_rule.interp(series, rows, rec, wt)
    anchors = np.stack([rng.integers(3, 12, len(at)), rng.integers(2, 9, len(at))], axis=1)
    values, variances = _values(hx0, 600 + n)
    Y, Z, info = O.ensrf_obs_space_ordered(hx0, anchors, values, variances, ONES)
    g = {nm: O.block_update(f[nm], BLOCK, anchors[:, 0], anchors[:, 1], Y, Z, ONES) for nm in names}
    H = np.zeros((len(at), 2 * 63 + len(at)))
    H[:, 2 * 63:] = np.eye(len(at))
    check(f"recorded route, n = {n}", _stack(f, names, hx0), _stack(g, names, info["hx"]), H, values, variances)
    assert all(not O.bits_equal(a, b) for nm in names for a, b in zip(f[nm], g[nm]))
