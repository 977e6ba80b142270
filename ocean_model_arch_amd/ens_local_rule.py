"""The localized serial observation update in numpy (include/ocn_sw.h ocn_ens_local_update): the rule the
device applies, restated on whole arrays with the members and the observations in loop order, the
observation-space loop of a serial ensemble square-root filter built on it, and the taper tables.

numpy's elementwise subtract, multiply, add and divide are single IEEE double operations per element and
nothing here is fused, so `local_rule` gives the device's bits.  OceanEnsemble.assimilate tracks the
ensemble at the observed points with it; tests/ens_local_ref.py hands the same function to the tests, which
check it against a scalar loop.  `ensrf_obs_space_ordered` is that loop as ocn_ens_assimilate runs it on the
device: its sums in member order (tests/ens_assim_ref.py hands it to the tests).  Pure numpy: no device, no
library.
"""
from __future__ import annotations

import numpy as np

MAX_OBS = 8192        # ocn_ens_local_update: observations per call
MAX_TAPER = 65536     # ... and taper entries


def reach_of(ntaper: int) -> int:
    """The largest r with r * r < ntaper: no point farther than this from an observation, along either
    axis, is within its taper."""
    r = 0
    while (r + 1) * (r + 1) < ntaper:
        r += 1
    return r


def _update(xs, rho, yk, zk):
    """The rule at points that all take observation k: xs the members' values there, rho their (nonzero)
    taper values.  Returns the new values."""
    n = len(xs)
    s = xs[0]
    for m in range(1, n):
        s = s + xs[m]
    mean = s / float(n)
    a = (xs[0] - mean) * yk[0]
    for m in range(1, n):
        p = (xs[m] - mean) * yk[m]
        a = a + p
    g = rho * a
    return [xs[m] + g * zk[m] for m in range(n)]


def local_rule(x, gi, gj, io, jo, y, z, taper):
    """The members' arrays after the observations (io[k], jo[k]), k ascending, with the rows y[k], z[k] and
    the taper table indexed by the squared index distance.

    x: the n >= 2 members' arrays in member order, all of one shape.  Either 2-D arrays with gi and gj the
    1-D global indices of their rows and columns (consecutive integers: a block's array), or arrays of any
    shape with gi and gj index arrays of that shape (scattered points).  Fresh arrays: the inputs are not
    written."""
    x = [np.array(a, dtype=np.float64, order="F", copy=True) for a in x]
    n = len(x)
    io, jo = np.asarray(io, dtype=np.int64).ravel(), np.asarray(jo, dtype=np.int64).ravel()
    y, z = np.asarray(y, dtype=np.float64).reshape(len(io), n), np.asarray(z, dtype=np.float64).reshape(len(io), n)
    taper = np.asarray(taper, dtype=np.float64).ravel()
    nt = len(taper)
    assert n >= 2 and nt >= 1
    gi, gj = np.asarray(gi, dtype=np.int64), np.asarray(gj, dtype=np.int64)
    grid = x[0].ndim == 2 and gi.ndim == 1 and gj.ndim == 1 and gi.shape + gj.shape == x[0].shape
    if grid:
        assert (np.diff(gi) == 1).all() and (np.diff(gj) == 1).all()
        reach = reach_of(nt)
    else:
        assert gi.shape == x[0].shape and gj.shape == x[0].shape
    with np.errstate(all="ignore"):
        for k in range(len(io)):
            if grid:   # the part of the array within the observation's box
                a0, a1 = max(int(io[k]) - reach - int(gi[0]), 0), min(int(io[k]) + reach - int(gi[0]) + 1, len(gi))
                b0, b1 = max(int(jo[k]) - reach - int(gj[0]), 0), min(int(jo[k]) + reach - int(gj[0]) + 1, len(gj))
                if a0 >= a1 or b0 >= b1:
                    continue
                view = [a[a0:a1, b0:b1] for a in x]
                d2 = ((gi[a0:a1] - io[k]) ** 2)[:, None] + ((gj[b0:b1] - jo[k]) ** 2)[None, :]
            else:
                view = x
                d2 = (gi - io[k]) ** 2 + (gj - jo[k]) ** 2
            rho = np.zeros(d2.shape)
            within = d2 < nt
            rho[within] = taper[d2[within]]
            act = rho != 0.0           # +0.0 and -0.0 alike: the observation is skipped there
            if not act.any():
                continue
            new = _update([v[act] for v in view], rho[act], y[k], z[k])
            for v, a in zip(view, new):
                v[act] = a
    return x


def gate2_of(gate, who: str = "assimilate"):
    """The squared threshold ocn_ens_set_gate takes, from a gate in sigma: gate * gate as one float64 product.
    None stays None (no gate).  TypeError for what is not a number, ValueError unless gate > 0 (inf allowed) and
    its square is too (0.0 would turn the gate off)."""
    if gate is None:
        return None
    if isinstance(gate, (bool, np.bool_)) or not isinstance(gate, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: gate = {gate!r}, not a number")
    g = np.float64(gate)
    with np.errstate(all="ignore"):
        g2 = g * g
    if not (g > 0.0 and g2 > 0.0):
        raise ValueError(f"{who}: gate = {gate!r}, not a float > 0 (inf allowed) whose square is > 0")
    return float(g2)


def _check_gate2(gate2, who):
    """gate2 as ocn_ens_set_gate takes it with the gate on: > 0 and not NaN, +inf allowed."""
    if isinstance(gate2, (bool, np.bool_)) or not isinstance(gate2, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: gate2 = {gate2!r}, not a number")
    if not np.float64(gate2) > 0.0:
        raise ValueError(f"{who}: gate2 = {gate2!r}, not > 0 (inf allowed)")
    return np.float64(gate2)


def _gate_ok(gate2, D, d):
    """ocn_ens_set_gate's test: lim = gate2 * D (one rounded product); finite D and d, and d * d <= lim."""
    lim = gate2 * np.float64(D)
    return bool(np.isfinite(D) and np.isfinite(d) and np.float64(d) * np.float64(d) <= lim)


def ensrf_obs_space(hx, obs_ij, values, variances, taper, gate2=None):
    """The observation-space loop of a serial ensemble square-root filter (Whitaker & Hamill 2002) with a
    taper: from hx, the (nobs, n) members' values at the observed points (i, j) = obs_ij[k], the observed
    values and the observation error variances, the rows Y[k], Z[k] that ocn_ens_local_update needs, and
    what the ensemble holds at the observed points afterwards.

    For k in order, with yv the CURRENT row k:  ybar = mean(yv), y' = yv - ybar, s = sum(y'^2) / (n - 1),
    D = s + r_k, d = value_k - ybar, alpha = 1 / (1 + sqrt(r_k / D));  Y[k] = y',
    Z[k][m] = (d - alpha y'_m) / ((n - 1) D);  then every row -- the observed points are state points like
    any other -- takes observation k by `local_rule`, so the rows stay bit for bit what the device's
    fields hold there.  Returns (Y, Z, info): info["hx"] the final rows, "innovations" the d of each step,
    "prior_spread" / "posterior_spread" the rows' standard deviations (n - 1) before and after.

    gate2 (None: no gate, nothing changes in any bit or key): ocn_ens_set_gate's squared threshold.  After D and d
    of observation k, ok = isfinite(D) and isfinite(d) and d * d <= gate2 * D; not ok, the observation is
    rejected: Y[k] as formed, Z[k] = +0.0, innovations[k] = d, and no row takes it.  The test is against the
    CURRENT row, so it depends on the order of the observations.  info gains "accepted" (a bool array) and
    "rejected" (their number)."""
    if gate2 is not None:
        gate2 = _check_gate2(gate2, "ensrf_obs_space")
        accepted = np.ones(len(hx), dtype=bool)
    hx = np.array(hx, dtype=np.float64, copy=True)
    nobs, n = hx.shape
    ij = np.asarray(obs_ij, dtype=np.int64).reshape(nobs, 2)
    values, variances = np.asarray(values, dtype=np.float64).ravel(), np.asarray(variances, dtype=np.float64).ravel()
    if n < 2 or len(values) != nobs or len(variances) != nobs:
        raise ValueError("ensrf_obs_space: hx (nobs, n >= 2) with nobs values and variances")
    if not (variances > 0.0).all() or not np.isfinite(variances).all() or not np.isfinite(values).all():
        raise ValueError("ensrf_obs_space: finite values and positive finite variances")
    Y, Z = np.zeros((nobs, n)), np.zeros((nobs, n))
    innov = np.zeros(nobs)
    prior = hx.std(axis=1, ddof=1)
    for k in range(nobs):
        yv = hx[k]
        ybar = float(np.sum(yv)) / n
        yp = yv - ybar
        s = float(np.sum(yp * yp)) / (n - 1)
        r = float(variances[k])
        D = s + r
        d = float(values[k]) - ybar
        if gate2 is not None:
            with np.errstate(all="ignore"):
                accepted[k] = _gate_ok(gate2, D, d)
            if not accepted[k]:
                Y[k] = yp
                innov[k] = d
                continue
        alpha = 1.0 / (1.0 + np.sqrt(r / D))
        Y[k] = yp
        Z[k] = (d - alpha * yp) / ((n - 1) * D)
        innov[k] = d
        cols = local_rule([hx[:, m] for m in range(n)], ij[:, 0], ij[:, 1], ij[k:k + 1, 0], ij[k:k + 1, 1],
                          Y[k:k + 1], Z[k:k + 1], taper)
        hx = np.stack(cols, axis=1)
    info = {"hx": hx, "innovations": innov, "prior_spread": prior, "posterior_spread": hx.std(axis=1, ddof=1)}
    if gate2 is not None:
        info["accepted"], info["rejected"] = accepted, int((~accepted).sum())
    return Y, Z, info


def _spread(row):
    """SPREAD of ocn_ens_stats over one row: ordered sum, / n, d = x - mean, q = d0 d0, q = q + d d,
    / (n - 1), sqrt."""
    n = len(row)
    s = row[0]
    for m in range(1, n):
        s = s + row[m]
    mean = s / np.float64(n)
    d = row[0] - mean
    q = d * d
    for m in range(1, n):
        d = row[m] - mean
        q = q + d * d
    return np.sqrt(q / np.float64(n - 1))


def ensrf_obs_space_ordered(hx, obs_ij, values, variances, taper, gate2=None):
    """ocn_ens_assimilate's observation-space loop (include/ocn_sw.h) in numpy, with explicit member loops:
    `ensrf_obs_space` with its two np.sum calls -- whose reduction order is numpy's own -- replaced by sums in
    member order, and the spreads by ocn_ens_stats' ordered definitions.  Every operation is one IEEE double
    operation on numpy float64 scalars, nothing is fused: the device's bits.

    For k in order, with x the CURRENT row k:  s1 = x_0, s1 = s1 + x_m;  ybar = s1 / n;  y'_m = x_m - ybar;
    q = y'_0 y'_0, p = y'_m y'_m, q = q + p;  s = q / (n - 1);  D = s + r_k;  d = value_k - ybar;  t = r_k / D;
    alpha = 1 / (1 + sqrt(t));  c = (n - 1) D;  Y[k][m] = y'_m, Z[k][m] = (d - alpha y'_m) / c;  then every row
    takes observation k by `local_rule`.  Returns (Y, Z, info) as `ensrf_obs_space` does; a non-finite row
    value, D or d propagates, and info["nonfinite"] counts the observations whose D or d was not finite.

    gate2 (None: no gate, nothing changes in any bit or key): ocn_ens_set_gate's squared threshold, > 0, inf
    allowed.  After D and d of observation k:  lim = gate2 * D (one rounded product);  ok = isfinite(D) and
    isfinite(d) and d * d <= lim.  Not ok, the observation is rejected: Y[k][m] = y'_m as formed, Z[k][m] = +0.0,
    innovations[k] = d, "nonfinite" counts as ever, and no row takes observation k (a rejected observation forms
    nothing: no bit of any row changes).  The test is against the CURRENT row, so it depends on the order of the
    observations.  info gains "accepted" (a bool array) and "rejected" (their number)."""
    if gate2 is not None:
        gate2 = _check_gate2(gate2, "ensrf_obs_space_ordered")
        accepted = np.ones(len(hx), dtype=bool)
    hx = np.array(hx, dtype=np.float64, copy=True)
    nobs, n = hx.shape
    ij = np.asarray(obs_ij, dtype=np.int64).reshape(nobs, 2)
    values, variances = np.asarray(values, dtype=np.float64).ravel(), np.asarray(variances, dtype=np.float64).ravel()
    if n < 2 or len(values) != nobs or len(variances) != nobs:
        raise ValueError("ensrf_obs_space_ordered: hx (nobs, n >= 2) with nobs values and variances")
    if not (variances > 0.0).all() or not np.isfinite(variances).all() or not np.isfinite(values).all():
        raise ValueError("ensrf_obs_space_ordered: finite values and positive finite variances")
    Y, Z = np.zeros((nobs, n)), np.zeros((nobs, n))
    innov = np.zeros(nobs)
    nonfinite = 0
    dn, dn1, one = np.float64(n), np.float64(n - 1), np.float64(1.0)
    with np.errstate(all="ignore"):
        prior = np.array([_spread(hx[j]) for j in range(nobs)])
        for k in range(nobs):
            x = hx[k]
            s1 = x[0]
            for m in range(1, n):
                s1 = s1 + x[m]
            ybar = s1 / dn
            yp = [x[m] - ybar for m in range(n)]
            q = yp[0] * yp[0]
            for m in range(1, n):
                p = yp[m] * yp[m]
                q = q + p
            s = q / dn1
            r = variances[k]
            D = s + r
            d = values[k] - ybar
            t = r / D
            alpha = one / (one + np.sqrt(t))
            c = dn1 * D
            ok = True
            if gate2 is not None:
                ok = accepted[k] = _gate_ok(gate2, D, d)
            for m in range(n):
                Y[k, m] = yp[m]
                Z[k, m] = (d - alpha * yp[m]) / c if ok else 0.0
            innov[k] = d
            if not (np.isfinite(D) and np.isfinite(d)):
                nonfinite += 1
            if not ok:
                continue
            cols = local_rule([hx[:, m] for m in range(n)], ij[:, 0], ij[:, 1], ij[k:k + 1, 0], ij[k:k + 1, 1],
                              Y[k:k + 1], Z[k:k + 1], taper)
            hx = np.stack(cols, axis=1)
        post = np.array([_spread(hx[j]) for j in range(nobs)])
    info = {"hx": hx, "innovations": innov, "prior_spread": prior, "posterior_spread": post, "nonfinite": nonfinite}
    if gate2 is not None:
        info["accepted"], info["rejected"] = accepted, int((~accepted).sum())
    return Y, Z, info


def taper_table(radius: float, kind: str = "gaspari_cohn") -> np.ndarray:
    """The taper over the squared index distance d2 = 0, 1, ... with compact support at `radius` grid
    points: entry d2 is the taper at distance sqrt(d2), the table ends before d2 = radius^2 (a point at
    `radius` or beyond is out of reach), entry 0 is 1.0 and the entries never increase.

    "gaspari_cohn": the fifth-order piecewise rational function of Gaspari & Cohn (1999, eq. 4.10) with
    half-width radius / 2, so that it reaches zero at `radius`; "boxcar": 1.0 within the radius."""
    radius = float(radius)
    if not 0.0 <= radius <= 256.0:
        raise ValueError(f"taper_table: radius {radius} outside 0..256 (at most {MAX_TAPER} entries)")
    nt = max(1, min(MAX_TAPER, int(np.ceil(radius * radius))))
    if kind == "boxcar":
        return np.ones(nt)
    if kind != "gaspari_cohn":
        raise ValueError(f"taper_table: unknown kind {kind!r}")
    if nt == 1:
        return np.ones(1)
    r = np.sqrt(np.arange(nt, dtype=np.longdouble)) / np.longdouble(radius / 2.0)
    inner = (((-0.25 * r + 0.5) * r + 0.625) * r - 5.0 / np.longdouble(3.0)) * r * r + 1.0
    ro = np.maximum(r, 1.0)   # (the outer branch divides by r)
    outer = ((((ro / 12.0 - 0.5) * ro + 0.625) * ro + 5.0 / np.longdouble(3.0)) * ro - 5.0) * ro + 4.0 - 2.0 / (3.0 * ro)
    t = np.where(r <= 1.0, inner, outer).astype(np.float64)
    # the polynomial's rounding near the edge of the support, where it cancels to almost nothing, must
    # not make the table negative or let it rise
    t = np.minimum.accumulate(np.clip(t, 0.0, 1.0))
    t[0] = 1.0
    return t
