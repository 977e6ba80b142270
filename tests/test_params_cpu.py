"""What the GPU parameter sweep (tests/test_gpu_params.py) relies on, shown with the oracle alone (no GPU).

Bounded runs: for every (parameter set, shape, input class) the sweep runs, the oracle's run over the
sweep's longest call sequence trips no check_ssh_err, stays finite and keeps max |ssh| < 1 m after EVERY
step.  A condition, not a measurement: a set that breaks it is retuned (tests/shapes.py PARAMS), the bound
stays.  The abyss cases also stay in the range where udiv's IEEE re-runs change the bits (below 2^-900
and nonzero on every wet velocity point), as tests/test_shapes_cpu.py asserts for tau = 1.

What each set promises: equator has both signs of rlh_s, coarse has rows that all differ, rot has an rlh_s
that varies along a row and every other set has row-constant metrics (so the compact tables hold them);
the taus fall on the side of std::frexp's 0.5 that selects the MarchStep<P2> variant they are meant for.
"""
import math

import numpy as np
import pytest

from tests import shapes as S
from tests import test_gpu_params as G
from tests.test_gpu_ensemble import member_uploads
from tests.test_gpu_shapes import SINGLE_MODES

METRICS = ("dx", "dy", "dxt", "dyt", "dxh", "dyh", "dxb", "dyb", "rlh_s")
UDIV_MIN = 2.0 ** -900   # sw_kernels.hip kUdivMinExp


def _runs():
    """(params, shape, class, flags, seed offset, ((steps, tau), ...)) of every run of the GPU sweep."""
    runs = set()

    def add(p, shape, cls, steps, flags=(1, 1, 1), off=0):
        runs.add((p, shape, cls, flags, off, ((steps, S.tau_of(p)),)))

    for p, s, md in G.SINGLE_CASES:
        for cls in G.SINGLE_CLASSES:
            add(p, s, cls, sum(SINGLE_MODES[md][1]))
    for p in S.PARAM_DEEP:
        add(p, G.DEEP_SHAPE, "abyss", sum(SINGLE_MODES[G.DEEP_MODE][1]))
    for p, s in [(p, s) for p, s, _, _ in G.GRID_CASES] + [(p, s) for p, s, _ in G.TRACER_CASES]:
        for cls in G.GRID_CLASSES:
            add(p, s, cls, 7)
    for p, s in G.RANK_CASES:
        add(p, s, "noise", sum(G.RANK_CALLS))
    for p in S.CORE_PARAMS:
        for i, cls in enumerate(S.COAST_ENSEMBLE_CLASSES):
            add(p, S.PARAM_ENSEMBLE, cls, 7, off=1000 * i)
    for p in S.OTHER_PARAMS:
        for md in G.OTHER_MODES:
            for cls in G.SINGLE_CLASSES:
                add(p, G.OTHER_SINGLE, cls, sum(SINGLE_MODES[md][1]))
        for cls in G.GRID_CLASSES:
            add(p, G.OTHER_GRID, cls, 7)
    for s in S.PARAM_ROT:
        for cls in (G.SINGLE_CLASSES if s.grid == (1, 1) else G.GRID_CLASSES):
            add("rot", s, cls, 7)
    for flags in G.FLAG_SETTINGS:
        add(G.FLAG_PARAMS, G.FLAG_SHAPE, "noise", 7, flags=flags)
    for shape, _, _ in G.TAU_LAYOUTS.values():
        runs.add((None, shape, G.TAU_CLASS, (1, 1, 1), 0, S.TAU_CALLS))
    return sorted(runs, key=lambda r: (str(r[0]), r[1].id, r[2], r[3], r[4], r[5]))


RUNS = _runs()


def _run_id(r):
    p, s, cls, flags, off, calls = r
    return f"{p}-{s.id}-{cls}" + ("" if flags == (1, 1, 1) else "-ffs%d_trans%d_ksw%d" % flags) + \
        (f"-m{off // 1000}" if off else "") + ("" if len(calls) == 1 else "-taus") + f"-s{sum(n for n, _ in calls)}"


@pytest.mark.parametrize("run", RUNS, ids=[_run_id(r) for r in RUNS])
def test_param_runs_stay_bounded(run):
    params, shape, cls, flags, off, calls = run
    om = S.oracle_model(shape, flags, params)
    ups = member_uploads(shape, cls, off, params) if off else S.uploads_for(shape, cls, params)
    for k, b in enumerate(om.blocks):
        for nm, a in ups.get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    step = 0
    for n, tau in calls:
        for _ in range(n):
            om.step(tau)   # raises FloatingPointError on a blow-up (check_ssh_err)
            step += 1
            for f in om.f:
                for nm, a in f.items():
                    assert np.isfinite(a).all(), f"step {step}: {nm} not finite"
                assert np.abs(f["ssh"]).max() < 1.0, (step, np.abs(f["ssh"]).max())
                if cls == "abyss":
                    for nm, msk in (("ubrtr", "lcu"), ("vbrtr", "lcv")):
                        a, wet = np.abs(f[nm]), f[msk] > 0.5
                        assert wet.any() and 0.0 < a[wet].min() and a[wet].max() < UDIV_MIN, (step, nm, a[wet].max())


def _rows(shape, params):
    """Per block of the oracle's initial state: (block, its fields, the index range of the rows and columns
    the stencils read: [start - 1, end + 1] -- sw_stencils.h Prepare's window)."""
    om = S.oracle_model(shape, params=params)
    out = []
    for k, b in enumerate(om.blocks):
        xs = slice(b.nxs - 1 - b.bx1, b.nxe + 1 - b.bx1 + 1)
        ys = slice(b.nys - 1 - b.by1, b.nye + 1 - b.by1 + 1)
        out.append((b, om.f[k], xs, ys))
    return out


PROMISE_SHAPES = sorted(set(S.PARAM_SINGLE + S.PARAM_GRIDS + S.PARAM_TRACER_GRIDS + S.PARAM_RANK_GRIDS +
                            [S.PARAM_ENSEMBLE]), key=lambda s: s.id)


@pytest.mark.parametrize("params", [p for p in S.PARAMS if p != "rot"])
def test_metrics_are_row_constant(params):
    """Every set but rot: each metric and rlh_s is one value along a row, so the compact tables hold them."""
    shapes = PROMISE_SHAPES if params in S.CORE_PARAMS else [G.OTHER_SINGLE, G.OTHER_GRID]
    for shape in shapes:
        for b, f, xs, ys in _rows(shape, params):
            for nm in METRICS:
                a = f[nm][xs, ys]
                assert (a == a[:1, :]).all(), (params, shape.id, (b.bm, b.bn), nm)


@pytest.mark.parametrize("shape", S.PARAM_ROT, ids=[s.id for s in S.PARAM_ROT])
def test_rot_varies_along_rows(shape):
    for b, f, xs, ys in _rows(shape, "rot"):
        a = f["rlh_s"][xs, ys]
        assert (a != a[:1, :]).any(axis=0).all(), (shape.id, (b.bm, b.bn))   # in every row of every block


@pytest.mark.parametrize("shape", PROMISE_SHAPES, ids=[s.id for s in PROMISE_SHAPES])
def test_equator_has_both_signs(shape):
    """rlh_s of both signs on interior rows, and of both signs among the rows ONE block's stencils read
    ([start - 1, end + 1]); with two block rows, negative rows in the blocks below the horizontal boundary
    and positive rows in the blocks above it."""
    blocks = _rows(shape, "equator")
    neg = pos = False
    for b, f, xs, ys in blocks:
        inner = f["rlh_s"][2:-2, 2:-2]
        neg, pos = neg or (inner < 0).any(), pos or (inner > 0).any()
    assert neg and pos
    assert any((f["rlh_s"][xs, ys] < 0).any() and (f["rlh_s"][xs, ys] > 0).any() for _, f, xs, ys in blocks)
    if shape.grid[1] == 2:
        for b, f, xs, ys in blocks:
            inner = f["rlh_s"][2:-2, 2:-2]
            assert (inner < 0).any() if b.bn == 1 else (inner > 0).any(), (b.bm, b.bn)


@pytest.mark.parametrize("shape", PROMISE_SHAPES, ids=[s.id for s in PROMISE_SHAPES])
def test_coarse_rows_differ(shape):
    """Adjacent rows of dx and dxh differ in every row a block's stencils read (by far more than an ulp:
    at least 1e-4 of the value), so row n +- 1 taken for row n cannot give the same bits."""
    for b, f, xs, ys in _rows(shape, "coarse"):
        for nm in ("dx", "dxh"):
            col = f[nm][2, ys].astype(np.float64)
            rel = np.abs(np.diff(col)) / col[:-1]
            assert (rel > 1.0e-4).all(), (shape.id, (b.bm, b.bn), nm, rel.min())


def test_taus_select_the_variants_they_are_meant_for():
    """sw_kernels.hip: p2 = std::frexp(tau, &ex) == 0.5 (tau = 2^k) at each launch site."""
    taus = {p: S.tau_of(p) for p in S.PARAMS}
    assert sorted(set(taus.values())) == [0.25, 0.3, 0.75, 2.0, 3.0, 30.0]
    for tau in (0.3, 0.75, 3.0, 30.0):
        assert math.frexp(tau)[0] != 0.5, tau
    for tau in (2.0, 0.25):
        assert math.frexp(tau)[0] == 0.5 and 1.0 / tau != 1.0, tau
    # the tau-change sequence crosses the boundary at every call but one
    p2 = [math.frexp(tau)[0] == 0.5 for _, tau in S.TAU_CALLS]
    assert p2 == [True, False, False, True, False]
    assert {p: math.frexp(t)[0] == 0.5 for p, t in taus.items() if p in S.CORE_PARAMS} == \
        {"tau03": False, "tau075_ts03": False, "tau2": True, "coarse": False, "equator": False}


def test_parameter_sets_are_what_the_oracle_is_pinned_at():
    """Every set has a fixture from the compiled reference with the set's own keywords and tau."""
    from tests.golden import cases
    seen = {}
    for name in cases.PARAM_CASES:
        c = cases.load_e2e(name)
        pname = [p for p in S.PARAMS if name in (f"coast40x32_{p}_s5", f"coast40x32_b2x2_{p}_s5")]
        assert len(pname) == 1, name
        p = pname[0]
        shape = S.Shape(36, 28, c["bxy"], 0, "rough")
        want = dict(dict(dxst=0.00312, dyst=0.00225, rlon=34.751560, rlat=44.801125, curve_grid=1,
                         rotation_on_lon=0.0, rotation_on_lat=0.0), **S.basin_kwargs(shape, p))
        assert c["basin"] == want, (name, c["basin"], want)
        assert c["tau"] == S.tau_of(p) and c["steps"] == 5
        assert c["sw"]["time_smooth"] == S.PARAMS[p][1].get("time_smooth", 0.5)
        assert np.array_equal(c["mask"], S.mask_of(shape))
        seen[p] = c
    assert sorted(seen) == sorted(S.PARAMS)
    assert seen["coarse"]["bxy"] == seen["equator"]["bxy"] == (2, 2)
    assert seen["tau075_ts03"]["sw"].get("use_tracers") == 1
