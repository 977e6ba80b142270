"""The moving-storm forcing for the tests (include/ocn_sw.h ocn_ens_forcing_*): the numpy restatement
(ocean_model_arch_amd/ens_forcing_rule.py rhs -- exp through math.exp per element, glibc's, which
tests/test_init_exp.py pins to the device's exp_libm; never np.exp), a scalar loop in plain Python floats to check
it against, the storms the cases use, and the CPU oracle stepped one step at a time with RHSx / RHSy set from the
restatement before each step (tests/shapes.py oracle_model, as tests/test_gpu_ensemble.py does).  No device, no
library.
"""
import functools
import math

import numpy as np

from ocean_model_arch_amd.ens_forcing_rule import (ForcingModel, Storm, inflow, pressure, rhs, step_time,  # noqa: F401
                                                   stress)
from tests import shapes as S
from tests.test_gpu_ensemble import member_uploads

NAMES = ("lcu", "lcv", "dx", "dy", "dxt", "dyt", "dxh", "dyh", "hhq_rest")
MODEL = ForcingModel(ub=3.0, vb=-2.0)          # a background wind: the stress is far from zero everywhere
CALM = ForcingModel()                           # none: the vortex alone
STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")
# the steps of the usual first short call (a plain step(), the storms attached and the arrays as init and the
# uploads left them): it opens the members' sequences, which a forcing launch goes on with
FIRST = 2


def storm_for(shape, i, **kw):
    """Member i's storm on a shape: the centre starts inside the basin, a little off the grid points, and moves
    0.3 index steps per second one way and 0.26 the other (at tau = 1: at least a quarter of an index step per
    step, so a forcing one step early or late differs in nearly every bit); the radius is 8 km, about 32 index
    steps of the default grid, so the whole of the small test basins lies inside the vortex' core and flank; the
    sense of rotation and the inflow angle alternate with i."""
    nx, ny = shape.W + 4, shape.H + 4
    c, s = inflow(20.0 if i % 2 else 0.0)
    base = dict(x0=0.31 * nx + 1.37 * i, y0=0.62 * ny - 0.81 * i, cx=0.3, cy=-0.26, radius=8.0e3 + 500.0 * i,
                vmax=30.0 + 2.0 * i, dp=3000.0 + 100.0 * i, cos_in=c, sin_in=s, turn=-1.0 if i % 3 == 1 else 1.0)
    base.update(kw)
    return Storm(**base)


def block_fields(om, k):
    return {nm: om.f[k][nm] for nm in NAMES}


def block_rhs(om, k, storm, model, t, old=True):
    """(RHSx, RHSy) of oracle block k for time t; old: outside the interior the arrays keep what they hold."""
    b = om.blocks[k]
    return rhs(storm, model, t, block_fields(om, k), (b.bx1, b.by1), (b.nxs, b.nxe, b.nys, b.nye),
               old=(om.f[k]["RHSx"], om.f[k]["RHSy"]) if old else None)


def set_forcing(om, storm, model, t):
    """The oracle's RHSx / RHSy of every block for time t, in place."""
    for k in range(len(om.blocks)):
        rx, ry = block_rhs(om, k, storm, model, t)
        om.f[k]["RHSx"][...] = rx
        om.f[k]["RHSy"][...] = ry


def loaded(shape, cls, off, params=None):
    """tests/shapes.py oracle_model with member `off`'s uploads of class cls written into its fields."""
    om = S.oracle_model(shape, params=params)
    for k, b in enumerate(om.blocks):
        for nm, a in member_uploads(shape, cls, off, params).get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    return om


def call_times(calls, tau, t_start=0.0):
    """The forcing times of the steps of step_forced calls of `calls` steps each, the c-th call made with
    t0 = t_start + (steps before it) * tau: a tuple, one entry per step (step_time's bits, call by call)."""
    out, done = [], 0
    for n in calls:
        t0 = float(t_start) + float(done) * float(tau)
        out += [step_time(t0, s, tau) for s in range(n)]
        done += n
    return tuple(out)


@functools.lru_cache(maxsize=64)
def forced_reference(shape, cls, off, storm, model, times, params=None, hold=0, first=0):
    """{(bm, bn): {field: array}} of the oracle after `first` plain steps, then one step per entry of `times` with
    the forcing of that time set before it, then `hold` more steps with the last forcing held -- from the member's
    inputs (tests/test_gpu_ensemble.py member_uploads).  storm None: no forcing at all.  Also, under "max_ssh", the
    largest |ssh| after any step and, under "series", the state fields after every step ({(bm, bn): {field:
    array}} per step).  Computed once per key; callers do not write into it."""
    om = loaded(shape, cls, off, params)
    tau = S.tau_of(params)
    top, series = 0.0, []

    def one():
        nonlocal top
        om.step(tau)
        top = max([top] + [float(np.nanmax(np.abs(f["ssh"]))) for f in om.f])
        series.append({(b.bm, b.bn): {nm: om.f[k][nm].copy(order="F") for nm in STATE} for k, b in enumerate(om.blocks)})

    for _ in range(first):
        one()
    for t in times:
        if storm is not None:
            set_forcing(om, storm, model, t)
        one()
    for _ in range(hold):
        one()
    out = {(b.bm, b.bn): om.f[k] for k, b in enumerate(om.blocks)}
    out["max_ssh"] = top
    out["series"] = series
    return out


# ---------------------------------------------------------------- a scalar loop: the header's lines in Python floats
def point(storm, model, t, m, n, p):
    """(RHSx, RHSy) at the global point (m, n) from the header's operations on Python floats (IEEE doubles, one
    operation per line, math.exp and math.sqrt).  p: the point's operands -- lcu, lcv, dxt, dyt, dxh, dyh, dx0,
    dy0, dx1, dy1, dx2, dy2 (real(4) values as Python floats: promoted exactly) and h0, h1, h2."""
    s, mo = storm, model
    q = s.cx * t
    xc = s.x0 + q
    q = s.cy * t
    yc = s.y0 + q
    rr = s.radius * s.radius
    sv = s.vmax / s.radius
    ra = mo.rho_air / mo.rho_water

    def qq(xi, yj, sx, sy):
        d = xi - xc
        ex = d * sx
        d = yj - yc
        ey = d * sy
        a = ex * ex
        b = ey * ey
        return ex, ey, (a + b) / rr

    def wind(xi, yj, sx, sy):
        ex, ey, q_ = qq(xi, yj, sx, sy)
        h = 0.5 * q_
        a = 0.5 - h
        a = a if a > -500.0 else -500.0
        sp = sv * math.exp(a)
        te = s.turn * ey
        a1 = te * s.cos_in
        a1 = -a1
        b1 = ex * s.sin_in
        c1 = sp * (a1 - b1)
        uw = mo.ub + c1
        te = s.turn * ex
        a1 = te * s.cos_in
        b1 = ey * s.sin_in
        c1 = sp * (a1 - b1)
        vw = mo.vb + c1
        w = math.sqrt(uw * uw + vw * vw)
        cd = mo.cd1 * w
        cd = mo.cd0 + cd
        cd = cd if cd < mo.cd_max else mo.cd_max
        k = ra * cd
        k = k * w
        return k * uw, k * vw

    def pa(xi, yj, sx, sy):
        _, _, q_ = qq(xi, yj, sx, sy)
        h = -0.5 * q_
        h = h if h > -500.0 else -500.0
        return -(s.dp * math.exp(h))

    def face(tau_, da, db, dg, pa0, pa1, h0, h1):
        a = tau_ * (da * db)
        d = pa1 - pa0
        d = d / mo.rho_water
        d = d * dg
        hf = 0.5 * (h0 + h1)
        d = d * hf
        return a - d

    xm, yn = float(m), float(n)
    pa0 = pa(xm, yn, p["dx0"], p["dy0"])
    rx = ry = 0.0
    if p["lcu"] > 0.5:
        tx, _ = wind(xm + 0.5, yn, p["dxt"], p["dyh"])
        rx = face(tx, p["dxt"], p["dyh"], p["dyh"], pa0, pa(xm + 1.0, yn, p["dx1"], p["dy1"]), p["h0"], p["h1"])
    if p["lcv"] > 0.5:
        _, ty = wind(xm, yn + 0.5, p["dxh"], p["dyt"])
        ry = face(ty, p["dyt"], p["dxh"], p["dxh"], pa0, pa(xm, yn + 1.0, p["dx2"], p["dy2"]), p["h0"], p["h2"])
    return rx, ry


def point_operands(f, i, j):
    """point()'s operands at array element (i, j) of a block's arrays f."""
    g = lambda nm, a, b: float(f[nm][a, b])   # noqa: E731
    return dict(lcu=g("lcu", i, j), lcv=g("lcv", i, j), dxt=g("dxt", i, j), dyt=g("dyt", i, j), dxh=g("dxh", i, j),
                dyh=g("dyh", i, j), dx0=g("dx", i, j), dy0=g("dy", i, j), dx1=g("dx", i + 1, j), dy1=g("dy", i + 1, j),
                dx2=g("dx", i, j + 1), dy2=g("dy", i, j + 1), h0=g("hhq_rest", i, j), h1=g("hhq_rest", i + 1, j),
                h2=g("hhq_rest", i, j + 1))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the GPU cases' runs
# name -> (shape, parameter set, the members' input classes, the forced members (None: all), the step_forced calls
# after the first short one).  tests/test_gpu_ens_forcing.py runs them; tests/test_ens_forcing_cpu.py asserts their
# premises on the oracle.  What each reaches:
#   one_tile    61 x 9: one tile per member, five members of three variants' inputs, odd and even step counts, a
#               1-step call
#   many_tiles  121 x 65: 51 tiles per member, the rough coast (masked faces) and members whose h_r varies
#   groups      nine members (under capacities 2 and 7: several launch groups, 16-row tiles)
#   subset      members 1 and 3 forced beside unforced known-constant ones in one call
#   tau03       tau = 0.3, no power of two: t_s = t0 + s tau rounds
#   grid        a 2 x 2 block grid: global indices across blocks, halo exchanges between the steps
#   tracer      a tracer run
#   one_point   1 x 1: a block with no wet face -- both arrays stay +0.0 whatever the storm
MIXED = ("plain", "noise", "hr", "general", "noise")
RUNS = {
    "one_tile": (S.Shape(61, 9), None, MIXED, None, (2, 5, 4, 1, 6)),
    "many_tiles": (S.Shape(121, 65, mask="rough"), None, ("plain", "noise", "hr", "general"), None, (2, 5, 4, 1, 6)),
    "groups": (S.Shape(61, 9), None, ("noise",) * 9, None, (2, 5, 4)),
    "subset": (S.Shape(61, 9), None, MIXED, (1, 3), (2, 5, 4)),
    "tau03": (S.Shape(61, 9, mask="rough"), "tau03", ("noise", "hr", "general"), None, (2, 5, 4)),
    "grid": (S.Shape(17, 19, (2, 2)), None, ("noise", "hr"), None, (2, 3)),
    "tracer": (S.Shape(13, 11, (1, 1), 1), None, ("noise", "noise"), None, (2, 3)),
    "one_point": (S.Shape(1, 1), None, ("noise", "noise"), None, (2, 3)),
}


def run_storm(name, i):
    """Member i's storm in run `name`: storm_for, with the speed raised where tau is smaller so that the centre
    still moves at least a quarter of an index step per step."""
    shape, params = RUNS[name][:2]
    tau = S.tau_of(params)
    return storm_for(shape, i) if tau >= 1.0 else storm_for(shape, i, cx=0.3 / tau, cy=-0.26 / tau)


def run_forced(name):
    """The forced members of run `name`, in member order."""
    forced = RUNS[name][3]
    return list(range(len(RUNS[name][2]))) if forced is None else sorted(forced)


def run_reference(name, i, calls=None, hold=0, first=FIRST):
    """Member i's forced_reference in run `name` (unforced members: storm None) over `calls` (None: the run's),
    behind `first` plain steps."""
    shape, params, classes, _, run_calls = RUNS[name]
    calls = run_calls if calls is None else tuple(calls)
    times = call_times(calls, S.tau_of(params))
    storm = run_storm(name, i) if i in run_forced(name) else None
    return forced_reference(shape, classes[i], 1000 * i, storm, MODEL if storm is not None else None, times, params,
                            hold, first)
