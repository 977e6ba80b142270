"""CPU checks of the moving-storm forcing (include/ocn_sw.h ocn_ens_forcing_*): the point function's header
(csrc/ens_forcing_point.h, the text the device compiles) built with g++ against the numpy restatement
(ens_forcing_rule.rhs) and a scalar loop, bit for bit; properties of the restatement; the premises of the GPU
cases (tests/test_gpu_ens_forcing.py) on the oracle; and the validation errors from Python and from the library.
No device anywhere."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from ocean_model_arch_amd import ens_forcing_rule as FR
from tests import ens_forcing_ref as R
from tests import shapes as S

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ocean_model_arch_amd", "csrc")
ERR_ARG = 1

# per record: the storm (10), the model (7), t, m, n, the point's six metrics and masks (lcu, lcv, dxt, dyt, dxh,
# dyh), dx and dy at the three t-points (6), h_r there (3) -- doubles in, (RHSx, RHSy) out
HARNESS = r"""
#define __host__
#define __device__
#include <cstdio>
#include <vector>
#include "ens_forcing_point.h"
int main(int argc, char **argv) {
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    double r[35];
    long n = 0;
    while (std::fread(r, sizeof(double), 35, in) == 35) {
        const ocn_ens_storm s{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]};
        const ocn_ens_forcing_model m{r[10], r[11], r[12], r[13], r[14], r[15], r[16]};
        ocn::FrcPoint p;
        p.lcu = (float)r[20]; p.lcv = (float)r[21]; p.dxt = (float)r[22]; p.dyt = (float)r[23];
        p.dxh = (float)r[24]; p.dyh = (float)r[25];
        p.dx0 = (float)r[26]; p.dy0 = (float)r[27]; p.dx1 = (float)r[28]; p.dy1 = (float)r[29];
        p.dx2 = (float)r[30]; p.dy2 = (float)r[31];
        p.h0 = r[32]; p.h1 = r[33]; p.h2 = r[34];
        const ocn::FrcAt c = ocn::frc_at(s, m, r[17]);
        double o[2];
        ocn::frc_point(s, m, c, (int)r[18], (int)r[19], p, o[0], o[1]);
        std::fwrite(o, sizeof(double), 2, out);
        ++n;
    }
    std::fclose(out);
    std::printf("%ld points\n", n);
    return 0;
}
"""

SHAPE = S.Shape(61, 9, mask="rough")   # masked faces among the wet ones


def _block():
    om = R.loaded(SHAPE, "hr", 0)      # h_r varies from point to point
    return om, om.blocks[0], R.block_fields(om, 0)


def _storms(b):
    """name -> (storm, model, t): what the header's text must get right."""
    mid_x, mid_y = float((b.nxs + b.nxe) // 2), float((b.nys + b.nye) // 2)
    c20, s20 = FR.inflow(20.0)
    base = dict(x0=mid_x + 0.37, y0=mid_y - 0.21, cx=0.3, cy=-0.26, radius=8.0e3, vmax=30.0, dp=3000.0, cos_in=c20, sin_in=s20)
    on_point = dict(base, x0=mid_x, y0=mid_y, cx=0.0, cy=0.0)
    return {
        "moving": (FR.Storm(**base), R.MODEL, 7.25),
        "centre_on_a_point": (FR.Storm(**on_point), R.CALM, 0.0),             # d = 0 at a t-point: q = 0
        "r_equals_R": (FR.Storm(**dict(on_point, radius=8.0 * 250.0)), R.CALM, 0.0),   # faces about 8 index steps away
        "clamp": (FR.Storm(**dict(base, radius=5.0)), R.MODEL, 3.0),           # q > 1001 one index step away
        "turn_minus": (FR.Storm(**dict(base, turn=-1.0)), R.MODEL, 7.25),
        "no_wind": (FR.Storm(**dict(base, vmax=0.0)), R.CALM, 7.25),           # pure pressure
        "no_pressure": (FR.Storm(**dict(base, dp=0.0)), R.MODEL, 7.25),
        "capped_drag": (FR.Storm(**dict(base, vmax=80.0)), R.MODEL, 7.25),
    }


def test_point_header_matches_the_restatement_bitwise(tmp_path):
    om, b, f = _block()
    cases = _storms(b)
    recs, want_np, want_py = [], [], []
    pts = [(i, j) for i in range(b.nxs - b.bx1, b.nxe - b.bx1 + 1) for j in range(b.nys - b.by1, b.nye - b.by1 + 1)]
    masked = sum(1 for i, j in pts if f["lcu"][i, j] < 0.5) + sum(1 for i, j in pts if f["lcv"][i, j] < 0.5)
    assert 0 < masked < 2 * len(pts)                      # masked and wet faces both
    for name, (storm, model, t) in cases.items():
        rx, ry = R.block_rhs(om, 0, storm, model, t, old=False)
        for i, j in pts:
            p = R.point_operands(f, i, j)
            recs.append(FR.storm_values(storm) + FR.model_values(model) + (t, float(b.bx1 + i), float(b.by1 + j)) +
                        tuple(p[k] for k in ("lcu", "lcv", "dxt", "dyt", "dxh", "dyh", "dx0", "dy0", "dx1", "dy1", "dx2",
                                             "dy2", "h0", "h1", "h2")))
            want_np.append((rx[i, j], ry[i, j]))
            want_py.append(R.point(storm, model, t, b.bx1 + i, b.by1 + j, p))
        # what the case is there for
        q = (FR.pressure(storm, model, t, *np.meshgrid(np.arange(b.nxs, b.nxe + 1.0), np.arange(b.nys, b.nye + 1.0), indexing="ij"),
                         250.0, 250.0) / -max(storm.dp, 1e-300))
        if name == "clamp":
            assert (q == math.exp(-500.0)).sum() > 0.9 * q.size          # nearly every point is clamped
        if name == "centre_on_a_point":
            assert (q == 1.0).sum() == 1                                   # one t-point is the centre itself
    src = tmp_path / "t.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", str(src), "-o", str(exe), "-lm"])
    np.asarray(recs, dtype=np.float64).tofile(tmp_path / "in.bin")
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith(f"{len(recs)} points"), r.stdout + r.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64).reshape(-1, 2)
    want_np, want_py = np.asarray(want_np), np.asarray(want_py)
    assert got.shape == want_np.shape
    assert R.bits_equal(want_py, want_np), "the scalar loop and the numpy restatement differ"
    differ = np.flatnonzero((got.view(np.uint64) != want_np.view(np.uint64)).any(axis=1))
    assert differ.size == 0, f"{differ.size} of {len(recs)} points differ, first at record {differ[:5]}"
    assert np.isfinite(got).all() and (got != 0.0).mean() > 0.5


def test_speed_at_r_equals_R_is_vmax():
    """No background wind, no inflow: the speed at r = R is vmax within 4 ulp, in every direction from the centre."""
    for turn in (1.0, -1.0):
        s = FR.Storm(x0=40.0, y0=30.0, radius=8000.0, vmax=37.3, dp=0.0, turn=turn)
        for k in range(16):
            a = 2.0 * math.pi * k / 16.0
            xi, yj = 40.0 + 32.0 * math.cos(a), 30.0 + 32.0 * math.sin(a)     # 32 index steps of 250 m: r = R to rounding
            _, _, uw, vw = FR.stress(s, R.CALM, 0.0, xi, yj, 250.0, 250.0)
            r = math.hypot((xi - 40.0) * 250.0, (yj - 30.0) * 250.0)
            assert abs(r - 8000.0) < 1e-9
            speed = math.hypot(float(uw), float(vw))
            # (r is R to a few ulp, and d speed / d r = 0 at r = R: the speed's own rounding is all that is left)
            assert abs(speed - 37.3) <= 4 * np.spacing(37.3), (k, speed)


def test_pressure_at_the_centre_is_minus_dp():
    s = FR.Storm(x0=12.0, y0=7.0, cx=0.5, cy=0.25, radius=3000.0, dp=2750.0)
    pa = FR.pressure(s, R.CALM, 8.0, 16.0, 9.0, 246.0, 250.0)     # the centre at t = 8: (12 + 4, 7 + 2)
    assert float(pa) == -2750.0
    far = FR.pressure(s, R.CALM, 8.0, 16.0 + 1000.0, 9.0, 246.0, 250.0)
    assert -1e-200 < float(far) < 0.0                                # the clamp: tiny, not zero


def test_rotation_sense_follows_turn():
    """East of the centre the wind blows north with turn = +1 and south with turn = -1; with an inflow angle it
    also blows toward the centre."""
    for turn in (1.0, -1.0):
        s = FR.Storm(x0=20.0, y0=20.0, radius=5000.0, vmax=25.0, turn=turn)
        _, _, uw, vw = FR.stress(s, R.CALM, 0.0, 30.0, 20.0, 250.0, 250.0)
        assert float(uw) == 0.0 and float(vw) * turn > 0.0
        c, sn = FR.inflow(25.0)
        s = FR.Storm(x0=20.0, y0=20.0, radius=5000.0, vmax=25.0, turn=turn, cos_in=c, sin_in=sn)
        _, _, uw, vw = FR.stress(s, R.CALM, 0.0, 30.0, 20.0, 250.0, 250.0)
        assert float(uw) < 0.0 and float(vw) * turn > 0.0


@pytest.mark.parametrize("name", sorted(R.RUNS))
def test_premises_of_the_gpu_cases(name):
    """On each run of the GPU file: the forcing is nonzero at >= 50 % of the sea u-points and differs in bits
    between consecutive steps at >= 90 % of them (so a forcing one step early or late cannot pass); the oracle's
    ssh stays below 1e4; the forced oracle run differs from the unforced one.  one_point has no wet face: there
    the arrays stay +0.0 and the two runs agree, which is what its GPU case checks."""
    shape, params, classes, _, calls = R.RUNS[name]
    tau = S.tau_of(params)
    times = R.call_times(calls, tau)
    for i in R.run_forced(name):
        storm = R.run_storm(name, i)
        assert abs(storm.cx * tau) >= 0.25
        om = R.loaded(shape, classes[i], 1000 * i, params)
        wet = [np.zeros(om.f[k]["lcu"].shape, dtype=bool) for k in range(len(om.blocks))]
        for k, b in enumerate(om.blocks):
            wet[k][b.nxs - b.bx1:b.nxe - b.bx1 + 1, b.nys - b.by1:b.nye - b.by1 + 1] = True
            wet[k] &= om.f[k]["lcu"] > 0.5
        total = sum(int(w.sum()) for w in wet)
        prev = [R.block_rhs(om, k, storm, R.MODEL, times[0])[0] for k in range(len(om.blocks))]
        nonzero = sum(int((p[w] != 0.0).sum()) for p, w in zip(prev, wet))
        assert nonzero >= 0.5 * total, (name, i, nonzero, total)
        for t in times[1:4]:
            now = [R.block_rhs(om, k, storm, R.MODEL, t)[0] for k in range(len(om.blocks))]
            changed = sum(int((a.view(np.uint64)[w] != p.view(np.uint64)[w]).sum()) for a, p, w in zip(now, prev, wet))
            assert changed >= 0.9 * total, (name, i, t, changed, total)
            prev = now
        forced = R.run_reference(name, i)
        plain = R.forced_reference(shape, classes[i], 1000 * i, None, None, times, params, 0, R.FIRST)
        assert forced["max_ssh"] < 1.0e4 and plain["max_ssh"] < 1.0e4
        same = all(R.bits_equal(forced[key]["ssh"], plain[key]["ssh"]) for key in forced if isinstance(key, tuple))
        if name == "one_point":
            assert total == 0 and same
        else:
            assert total > 0 and not same, (name, i)


# ---------------------------------------------------------------- validation
BAD_STORMS = [dict(radius=0.0), dict(radius=-1.0), dict(vmax=-1.0), dict(dp=-1.0), dict(turn=0.0), dict(turn=2.0),
              dict(cos_in=1.0, sin_in=1e-5), dict(x0=float("nan")), dict(cx=float("inf")), dict(radius=float("inf"))]
BAD_MODELS = [dict(rho_air=-1.0), dict(rho_water=0.0), dict(rho_water=-1.0), dict(cd0=-1e-3), dict(cd1=-1e-3),
              dict(cd_max=-1.0), dict(ub=float("nan")), dict(vb=float("inf"))]


def _c_storm(s):
    from ocean_model_arch_amd import _lib
    return _lib.OcnEnsStorm(*FR.storm_values(s))


def test_validation_from_python():
    good = FR.Storm(x0=5.0, y0=5.0)
    assert FR.check_storm(good) is good and FR.check_model(FR.ForcingModel()) is not None
    for kw in BAD_STORMS:
        with pytest.raises(ValueError):
            FR.check_storm(FR.Storm(**dict(dict(x0=5.0, y0=5.0), **kw)))
    for kw in BAD_MODELS:
        with pytest.raises(ValueError):
            FR.check_model(FR.ForcingModel(**kw))
    for bad in (None, (1.0, 2.0), {"x0": 1.0}):
        with pytest.raises(TypeError):
            FR.check_storm(bad)
        with pytest.raises(TypeError):
            FR.check_model(bad)
    with pytest.raises(TypeError):
        FR.check_storm(FR.Storm(x0="5", y0=5.0))
    with pytest.raises(TypeError):
        FR.check_model(FR.ForcingModel(cd0=[1.0]))


def test_validation_from_the_library():
    """ocn_ens_forcing_check is ocn_ens_forcing_set's validation without an ensemble: the same refusals as Python's."""
    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    model = _lib.OcnEnsForcingModel(*FR.model_values(FR.ForcingModel()))
    good = FR.Storm(x0=5.0, y0=5.0)
    arr = (_lib.OcnEnsStorm * 3)(*[_c_storm(good)] * 3)
    assert L.ocn_ens_forcing_check(arr, 3, C.byref(model)) == 0
    assert L.ocn_ens_forcing_check(None, 3, C.byref(model)) == ERR_ARG
    assert L.ocn_ens_forcing_check(arr, 3, None) == ERR_ARG
    assert L.ocn_ens_forcing_check(arr, 0, C.byref(model)) == ERR_ARG
    for kw in BAD_STORMS:
        arr[1] = _c_storm(FR.Storm(**dict(dict(x0=5.0, y0=5.0), **kw)))
        assert L.ocn_ens_forcing_check(arr, 3, C.byref(model)) == ERR_ARG, kw
        assert b"storm 1" in L.ocn_last_error()
        assert L.ocn_ens_forcing_check(arr, 1, C.byref(model)) == 0          # (the bad one is not among the first)
    arr[1] = _c_storm(good)
    for kw in BAD_MODELS:
        bad = _lib.OcnEnsForcingModel(*FR.model_values(FR.ForcingModel(**kw)))
        assert L.ocn_ens_forcing_check(arr, 3, C.byref(bad)) == ERR_ARG, kw
    # the null-ensemble refusals of the entries that need one
    assert L.ocn_ens_forcing_set(None, None, arr, C.byref(model)) == ERR_ARG
    assert L.ocn_ens_forcing_clear(None) == ERR_ARG
    assert L.ocn_ens_forcing_apply(None, 0.0) == ERR_ARG
    assert L.ocn_ens_step_forced(None, 1.0, 1, 1, 0.0) == ERR_ARG
    assert L.ocn_ens_forcing_info(None, None) == ERR_ARG


def test_step_times():
    """t_s = t0 + (double)s tau: a product and a sum, call by call."""
    assert FR.step_time(0.6, 1, 0.3) == 0.6 + 0.3 and R.call_times((2, 2), 0.3) == (0.0, 0.3, 0.6, 0.6 + 0.3)
    assert R.call_times((1, 2), 2.0, 10.0) == (10.0, 12.0, 14.0)
