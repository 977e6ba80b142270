"""Covariance inflation per point in numpy (include/ocn_sw.h ocn_ens_inflate): the rule the device applies,
restated on whole arrays with the members in loop order.

    s = x_0;  s = s + x_m (m = 1 .. n-1);  mean = s / n
    d_m = x_m - mean
    q = d_0 d_0;  p = d_m d_m, q = q + p;  var = q / (n-1);  sa = sqrt(var)
    CONST:  f = alpha                       (applies where sa > 0 and sa is finite)
    RTPS:   sb = the saved spread           (applies where sa > 0, sa finite and sb finite)
            t = sb - sa;  r = t / sa;  g = alpha r;  f = 1.0 + g
    where the rule applies and f != 1.0:  p = f d_m;  x_m = mean + p  for every m

numpy's elementwise subtract, multiply, add, divide and sqrt are single IEEE double operations per element
and nothing here is fused, so `inflate_rule` gives the device's bits; tests/ens_inflate_ref.py hands it to the
tests, which check it against a scalar loop.  Pure numpy: no device, no library.
"""
from __future__ import annotations

import numpy as np

CONST, RTPS = 0, 1                    # OCN_ENS_INFLATE_CONST, OCN_ENS_INFLATE_RTPS
MODES = {"const": CONST, "rtps": RTPS}


def spread(x):
    """SPREAD by ocn_ens_stats' definition over the members' arrays x, in member order: what
    ocn_ens_spread_save keeps."""
    x = [np.asarray(a, dtype=np.float64) for a in x]
    n = len(x)
    assert n >= 2
    with np.errstate(all="ignore"):
        s = x[0].copy()
        for m in range(1, n):
            s = s + x[m]
        mean = s / np.float64(n)
        d = x[0] - mean
        q = d * d
        for m in range(1, n):
            d = x[m] - mean
            p = d * d
            q = q + p
        return np.sqrt(q / np.float64(n - 1))


def inflate_rule(x, sb, mode, alpha):
    """(new_x, factor): the n >= 2 members' arrays x (member order, one shape) after the rule, as fresh
    arrays, and the factor applied at every point (1.0 where the point is not written).  sb: the saved
    spread, of the members' shape (RTPS; ignored in CONST, may be None); mode: "const" / "rtps" or the
    enum's value; alpha: a finite float, >= 0 in RTPS."""
    mode = MODES.get(mode, mode)
    assert mode in (CONST, RTPS)
    alpha = float(alpha)
    assert np.isfinite(alpha) and (mode == CONST or alpha >= 0.0)
    x = [np.array(a, dtype=np.float64, order="F", copy=True) for a in x]
    n = len(x)
    assert n >= 2
    with np.errstate(all="ignore"):
        s = x[0].copy()
        for m in range(1, n):
            s = s + x[m]
        mean = s / np.float64(n)
        d = x[0] - mean
        q = d * d
        for m in range(1, n):
            d = x[m] - mean
            p = d * d
            q = q + p
        var = q / np.float64(n - 1)
        sa = np.sqrt(var)
        applies = (sa > 0.0) & np.isfinite(sa)
        if mode == CONST:
            f = np.full(sa.shape, alpha, dtype=np.float64, order="F")
        else:
            sb = np.asarray(sb, dtype=np.float64)
            assert sb.shape == sa.shape
            applies &= np.isfinite(sb)
            t = sb - sa
            r = t / sa
            g = np.float64(alpha) * r
            f = 1.0 + g
        write = applies & (f != 1.0)
        for m in range(n):
            d = x[m] - mean
            p = f * d
            new = mean + p
            x[m][write] = new[write]
    factor = np.asfortranarray(np.where(write, f, 1.0))
    return x, factor
