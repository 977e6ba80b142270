"""The moving-storm forcing in Python (include/ocn_sw.h ocn_ens_forcing_*): the storm and the model as the library
takes them, their defaults, the validation that mirrors the C errors, and the point function restated in numpy.
Pure Python and numpy: no device, no library.

A storm is a Gaussian vortex that moves across the basin: its wind stress and the gradient of its air pressure
become OCN_RHSX / OCN_RHSY, the external momentum forcing of sw_update_uv.  The rule, operation by operation, is
in include/ocn_sw.h; `rhs` below follows it line by line on whole arrays.  numpy's elementwise add, subtract,
multiply, divide and sqrt are single IEEE double operations and nothing here is fused; exp goes through math.exp
per element -- glibc's, which tests/test_init_exp.py pins to the device's exp_libm -- never through np.exp.  So
`rhs` gives the device's bits.
"""
from __future__ import annotations

import math
from dataclasses import astuple, dataclass, fields

import numpy as np


@dataclass(frozen=True)
class Storm:
    """ocn_ens_storm: x0, y0 the centre at t = 0 in global 1-based index coordinates (fractional); cx, cy index
    steps per second; radius in m; vmax in m/s; dp the central pressure deficit in Pa; cos_in, sin_in the inflow
    angle's cosine and sine (`inflow` forms them); turn +1.0 or -1.0, the sense of rotation (+1: counter-clockwise
    in index space)."""
    x0: float
    y0: float
    cx: float = 0.0
    cy: float = 0.0
    radius: float = 50.0e3
    vmax: float = 30.0
    dp: float = 3000.0
    cos_in: float = 1.0
    sin_in: float = 0.0
    turn: float = 1.0


@dataclass(frozen=True)
class ForcingModel:
    """ocn_ens_forcing_model: the densities (kg/m^3), the drag cd = min(cd0 + cd1 |U|, cd_max) (Garratt 1977's
    linear law with a cap) and a background wind ub, vb (m/s)."""
    rho_air: float = 1.225
    rho_water: float = 1025.0
    cd0: float = 0.75e-3
    cd1: float = 0.067e-3
    cd_max: float = 3.0e-3
    ub: float = 0.0
    vb: float = 0.0


def inflow(degrees: float):
    """(cos_in, sin_in) of an inflow angle in degrees, formed on the host: the device takes no sin or cos."""
    a = math.radians(float(degrees))
    return math.cos(a), math.sin(a)


def _numbers(who, obj):
    out = []
    for f in fields(obj):
        v = getattr(obj, f.name)
        if isinstance(v, (str, bytes, bool)) or np.ndim(v) != 0:
            raise TypeError(f"{who}: {f.name} = {v!r}, not a number")
        try:
            out.append(float(v))
        except (TypeError, ValueError):
            raise TypeError(f"{who}: {f.name} = {v!r}, not a number") from None
    return out


def check_model(model) -> ForcingModel:
    """TypeError for a model that is not a ForcingModel of numbers, ValueError as ocn_ens_forcing_set refuses it."""
    if not isinstance(model, ForcingModel):
        raise TypeError(f"a ForcingModel, not {type(model).__name__}")
    v = _numbers("forcing model", model)
    if not all(math.isfinite(x) for x in v):
        raise ValueError("forcing model: a value that is not finite")
    if model.rho_air < 0.0 or not model.rho_water > 0.0:
        raise ValueError("forcing model: rho_air < 0 or rho_water <= 0")
    if model.cd0 < 0.0 or model.cd1 < 0.0 or model.cd_max < 0.0:
        raise ValueError("forcing model: a negative drag coefficient")
    return model


def check_storm(storm, who: str = "storm") -> Storm:
    """TypeError for a storm that is not a Storm of numbers, ValueError as ocn_ens_forcing_set refuses it."""
    if not isinstance(storm, Storm):
        raise TypeError(f"{who}: a Storm, not {type(storm).__name__}")
    v = _numbers(who, storm)
    if not all(math.isfinite(x) for x in v):
        raise ValueError(f"{who}: a value that is not finite")
    if not storm.radius > 0.0:
        raise ValueError(f"{who}: radius = {storm.radius} <= 0")
    if storm.vmax < 0.0 or storm.dp < 0.0:
        raise ValueError(f"{who}: vmax or dp negative")
    if storm.turn not in (1.0, -1.0):
        raise ValueError(f"{who}: turn = {storm.turn}, neither +1 nor -1")
    if abs(storm.cos_in * storm.cos_in + storm.sin_in * storm.sin_in - 1.0) > 1e-12:
        raise ValueError(f"{who}: cos_in^2 + sin_in^2 is not 1")
    return storm


def storm_values(storm) -> tuple:
    """The ten doubles of ocn_ens_storm, in its order."""
    return tuple(float(x) for x in astuple(storm))


def model_values(model) -> tuple:
    """The seven doubles of ocn_ens_forcing_model, in its order."""
    return tuple(float(x) for x in astuple(model))


def step_time(t0: float, s: int, tau: float) -> float:
    """t_s of step s (0-based) of ocn_ens_step_forced: a product, then a sum."""
    return float(t0) + float(s) * float(tau)


# ---------------------------------------------------------------- the point function on whole arrays
_exp = np.frompyfunc(math.exp, 1, 1)


def _exp_libm(a):
    return np.asarray(_exp(a), dtype=np.float64)


def _at(s: Storm, m: ForcingModel, t: float):
    f = np.float64
    p = f(s.cx) * f(t)
    xc = f(s.x0) + p
    p = f(s.cy) * f(t)
    yc = f(s.y0) + p
    rr = f(s.radius) * f(s.radius)
    sv = f(s.vmax) / f(s.radius)
    ra = f(m.rho_air) / f(m.rho_water)
    return xc, yc, rr, sv, ra


def _q(at, xi, yj, sx, sy):
    xc, yc, rr, _, _ = at
    d = xi - xc
    ex = d * sx
    d = yj - yc
    ey = d * sy
    a = ex * ex
    b = ey * ey
    s = a + b
    return ex, ey, s / rr


def stress(s: Storm, m: ForcingModel, t: float, xi, yj, sx, sy):
    """(taux, tauy, uw, vw): the kinematic wind stress and the wind at the index positions (xi, yj) -- float64
    arrays of one shape -- with sx, sy metres per index step there."""
    f = np.float64
    at = _at(s, m, t)
    xi, yj, sx, sy = (np.asarray(a, dtype=np.float64) for a in (xi, yj, sx, sy))
    with np.errstate(all="ignore"):
        ex, ey, q = _q(at, xi, yj, sx, sy)
        h = f(0.5) * q
        a = f(0.5) - h
        a = np.where(a > -500.0, a, f(-500.0))
        e = _exp_libm(a)
        sp = at[3] * e
        te = f(s.turn) * ey
        a1 = te * f(s.cos_in)
        a1 = -a1
        b1 = ex * f(s.sin_in)
        c1 = a1 - b1
        c1 = sp * c1
        uw = f(m.ub) + c1
        te = f(s.turn) * ex
        a1 = te * f(s.cos_in)
        b1 = ey * f(s.sin_in)
        c1 = a1 - b1
        c1 = sp * c1
        vw = f(m.vb) + c1
        a1 = uw * uw
        b1 = vw * vw
        ss = a1 + b1
        w = np.sqrt(ss)
        cd = f(m.cd1) * w
        cd = f(m.cd0) + cd
        cd = np.where(cd < f(m.cd_max), cd, f(m.cd_max))
        k = at[4] * cd
        k = k * w
        return k * uw, k * vw, uw, vw


def pressure(s: Storm, m: ForcingModel, t: float, xi, yj, sx, sy):
    """The air pressure anomaly (Pa, <= 0) at the index positions (xi, yj)."""
    f = np.float64
    at = _at(s, m, t)
    xi, yj, sx, sy = (np.asarray(a, dtype=np.float64) for a in (xi, yj, sx, sy))
    with np.errstate(all="ignore"):
        _, _, q = _q(at, xi, yj, sx, sy)
        h = f(-0.5) * q
        h = np.where(h > -500.0, h, f(-500.0))
        e = _exp_libm(h)
        pa = f(s.dp) * e
        return -pa


def _face(m: ForcingModel, tau, da, db, dg, pa0, pa1, h0, h1):
    f = np.float64
    ar = da * db
    a = tau * ar
    d = pa1 - pa0
    d = d / f(m.rho_water)
    d = d * dg
    hf = h0 + h1
    hf = f(0.5) * hf
    d = d * hf
    return a - d


def rhs(storm: Storm, model: ForcingModel, t: float, f: dict, bounds, interior, old=None):
    """(RHSx, RHSy) of one block for time t: float64 arrays of the block's array shape, Fortran order.

    f: the block's arrays by name -- lcu, lcv, dx, dy, dxt, dyt, dxh, dyh (real(4)) and hhq_rest (real(8)).
    bounds = (bnd_x1, bnd_y1): the global 1-based indices of the arrays' first element; interior = (nx_start,
    nx_end, ny_start, ny_end): the points written.  old: the arrays' contents before, (RHSx, RHSy) -- everything
    outside the interior keeps them (None: +0.0)."""
    bx1, by1 = bounds
    nxs, nxe, nys, nye = interior
    D = lambda nm: np.asarray(f[nm]).astype(np.float64)   # noqa: E731  (the real(4) operands promoted)
    shape = np.asarray(f["lcu"]).shape
    out = [np.zeros(shape, dtype=np.float64, order="F") if old is None else np.array(o, dtype=np.float64, order="F", copy=True)
           for o in ((None, None) if old is None else old)]
    i0, i1, j0, j1 = nxs - bx1, nxe - bx1, nys - by1, nye - by1
    I = slice(i0, i1 + 1)
    J = slice(j0, j1 + 1)
    E = slice(i0 + 1, i1 + 2)      # the point one to the east
    N = slice(j0 + 1, j1 + 2)      # ... one to the north
    m_, n_ = np.meshgrid(np.arange(nxs, nxe + 1, dtype=np.float64), np.arange(nys, nye + 1, dtype=np.float64), indexing="ij")
    dx, dy, hr = D("dx"), D("dy"), np.asarray(f["hhq_rest"], dtype=np.float64)
    with np.errstate(all="ignore"):
        pa0 = pressure(storm, model, t, m_, n_, dx[I, J], dy[I, J])
        pa1 = pressure(storm, model, t, m_ + 1.0, n_, dx[E, J], dy[E, J])
        pa2 = pressure(storm, model, t, m_, n_ + 1.0, dx[I, N], dy[I, N])
        dxt, dyt, dxh, dyh = D("dxt")[I, J], D("dyt")[I, J], D("dxh")[I, J], D("dyh")[I, J]
        taux, _, _, _ = stress(storm, model, t, m_ + 0.5, n_, dxt, dyh)
        _, tauy, _, _ = stress(storm, model, t, m_, n_ + 0.5, dxh, dyt)
        rx = _face(model, taux, dxt, dyh, dyh, pa0, pa1, hr[I, J], hr[E, J])
        ry = _face(model, tauy, dyt, dxh, dxh, pa0, pa2, hr[I, J], hr[I, N])
    out[0][I, J] = np.where(np.asarray(f["lcu"])[I, J] > np.float32(0.5), rx, 0.0)
    out[1][I, J] = np.where(np.asarray(f["lcv"])[I, J] > np.float32(0.5), ry, 0.0)
    return out[0], out[1]
