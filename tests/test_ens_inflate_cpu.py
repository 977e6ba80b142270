"""CPU checks of the per-point covariance inflation (ocn_ens_spread_save, ocn_ens_inflate): the numpy
restatement the GPU tests compare against (tests/ens_inflate_ref.py) is checked against an independent scalar
loop over Python floats, the identities and the relaxation property the contract promises are checked on it,
and the entries' errors that need no device and the header's enum values are exercised."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import ens_inflate_ref as R
from tests.test_ens_local_cpu import ANALYTIC_TOL, _members

ERR_ARG = 1
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ocn_sw.h")
COUNTS = [2, 5, 8, 9, 32, 33]


@pytest.fixture(scope="module")
def lib():
    import ocean_model_arch_amd as amd
    if not os.path.exists(amd._lib.LIB_PATH):
        amd.build()
    return amd.lib()


def _inputs(n):
    """n members of the 9 x 7 array of tests/test_ens_local_cpu.py (signed zeros, an all -0.0 point,
    denormals), plus an all-equal point and a point with NaN in one member; and a saved spread with a NaN, an
    Inf, a zero, a denormal and entries below and above the members' own spread."""
    x = _members(n)
    x[:, 2, 4] = 0.375                        # every member the same: sa = 0
    x[n // 2, 4, 3] = np.nan                  # one member NaN
    x[0, 7, 2] = np.inf
    sb = np.random.default_rng(7 * n).uniform(0.0, 1.5, (9, 7))
    sb[1, 1], sb[1, 2], sb[1, 3], sb[1, 4] = np.nan, np.inf, 0.0, 4e-320
    own = R.spread(list(x))
    sb[0, 5] = own[0, 5]                      # t = 0: f exactly 1.0 whatever alpha
    sb[8, 6] = own[8, 6] * 3.0                # the denormal point against a denormal saved spread
    return x, sb


def _scalar(x, sb, mode, alpha):
    """The contract with Python floats (IEEE doubles): one point and one member at a time."""
    n = len(x)
    out = np.array(x, dtype=np.float64, copy=True)
    fac = np.ones(out.shape[1:])
    for a in range(out.shape[1]):
        for b in range(out.shape[2]):
            v = [float(out[m, a, b]) for m in range(n)]
            s = v[0]
            for m in range(1, n):
                s = s + v[m]
            mean = s / float(n)
            d = [v[m] - mean for m in range(n)]
            q = d[0] * d[0]
            for m in range(1, n):
                p = d[m] * d[m]
                q = q + p
            var = q / float(n - 1)
            sa = math.sqrt(var)                     # (var is >= 0, Inf or NaN: no ValueError)
            if not (sa > 0.0 and math.isfinite(sa)):
                continue
            if mode == R.CONST:
                f = float(alpha)
            else:
                p0 = float(sb[a, b])
                if not math.isfinite(p0):
                    continue
                t = p0 - sa
                r = t / sa                          # (sa > 0: no ZeroDivisionError; an overflow gives Inf)
                g = float(alpha) * r
                f = 1.0 + g
            if f == 1.0:
                continue
            fac[a, b] = f
            for m in range(n):
                p = f * d[m]
                out[m, a, b] = mean + p
    return out, fac


@pytest.mark.parametrize("n", COUNTS)
def test_restatement_matches_scalar_loop(n):
    x, sb = _inputs(n)
    keep = x.copy()
    for mode, alpha in ((R.RTPS, 0.7), (R.RTPS, 1.0), (R.RTPS, 0.0), (R.CONST, 1.05), (R.CONST, -0.5), (R.CONST, 1.0)):
        want, wfac = _scalar(x, sb, mode, alpha)
        got, fac = R.inflate_rule(list(x), sb, mode, alpha)
        assert R.same(got, list(want)), (mode, alpha)
        assert R.bits_equal(fac, wfac), (mode, alpha)
    assert R.bits_equal(x, keep)                # the inputs are not written
    got, fac = R.inflate_rule(list(x), sb, "rtps", 0.7)
    for a, b in ((2, 4), (5, 5), (4, 3), (7, 2), (1, 1), (1, 2), (0, 5)):   # all equal, all -0.0, NaN, Inf, sb NaN / Inf, t = 0
        assert fac[a, b] == 1.0 and all(R.bits_equal(g[a, b], v[a, b]) for g, v in zip(got, x)), (a, b)
    assert np.signbit([g[5, 5] for g in got]).all()
    assert (fac != 1.0).sum() >= 50


@pytest.mark.parametrize("n", COUNTS)
def test_identities(n):
    """alpha = 0 (RTPS) and alpha = 1 (CONST) return the inputs bit for bit with factor 1.0 everywhere --
    signed zeros and denormal values included; the saved spread is that of the same members with their
    anomalies doubled, so that t / sa is about 1 at every point, the denormal ones included -- and an
    all-equal point and a NaN point keep their bits whatever alpha."""
    x, _ = _inputs(n)
    sb = R.spread([2.0 * a for a in x])
    sb[3, 3], sb[6, 0] = np.nan, np.inf
    for mode, alpha in ((R.RTPS, 0.0), (R.CONST, 1.0)):
        got, fac = R.inflate_rule(list(x), sb, mode, alpha)
        assert R.same(got, list(x)), (mode, alpha)
        assert (fac == 1.0).all(), (mode, alpha)
    for mode, alpha in ((R.RTPS, 0.9), (R.CONST, 1.3)):
        got, fac = R.inflate_rule(list(x), sb, mode, alpha)
        for a, b in ((2, 4), (5, 5), (4, 3), (7, 2)):
            assert fac[a, b] == 1.0 and all(R.bits_equal(g[a, b], v[a, b]) for g, v in zip(got, x)), (mode, a, b)
        assert not R.same(got, list(x))
        assert np.isfinite([g[4, 3] for m, g in enumerate(got) if m != n // 2]).all()   # the NaN did not spread


@pytest.mark.parametrize("alpha", [1.0, 0.6])
@pytest.mark.parametrize("n", COUNTS)
def test_relaxation_property(n, alpha):
    """Members uniform(-1, 1) on a 65 x 13 array; the "analysis" is the prior with its anomalies shrunk by a
    per-point factor in [0.05, 0.9] and its mean shifted by 0.1.  After RTPS the spread is alpha sb +
    (1 - alpha) sa within a relative ANALYTIC_TOL (1e-12: some 6 n rounded operations on O(1) data, ~1e-14,
    times 100), and the mean has not moved by more than that."""
    rng = np.random.default_rng(1000 * n + int(10 * alpha))
    prior = rng.uniform(-1.0, 1.0, (n, 65, 13))
    shrink = rng.uniform(0.05, 0.9, (65, 13))
    pm = prior.mean(axis=0)
    post = [pm + 0.1 + shrink * (a - pm) for a in prior]
    sb, sa = R.spread(list(prior)), R.spread(post)
    got, fac = R.inflate_rule(post, sb, "rtps", alpha)
    L = np.longdouble
    want = L(alpha) * sb.astype(L) + (L(1.0) - L(alpha)) * sa.astype(L)
    g = np.array(got, dtype=L)
    gm = g.sum(axis=0) / n
    new = np.sqrt(((g - gm) ** 2).sum(axis=0) / (n - 1))
    err = float(np.max(np.abs(new - want) / want))
    drift = float(np.max(np.abs(gm - np.array(post, dtype=L).sum(axis=0) / n)))
    print(f"n {n} alpha {alpha}: worst relative error of the spread {err:.3e}, worst drift of the mean {drift:.3e}")
    assert err <= ANALYTIC_TOL and drift <= ANALYTIC_TOL
    assert (fac > 1.0).all()                    # the analysis had shrunk the spread everywhere


def test_prototypes_and_null_arguments(lib):
    from ocean_model_arch_amd import _lib
    assert lib.ocn_abi_version() == 5
    for nm, nargs in (("ocn_ens_spread_save", 4), ("ocn_ens_inflate", 6), ("ocn_ens_inflate_download", 5)):
        assert nm in _lib.ENS_SYMBOLS and len(getattr(lib, nm).argtypes) == nargs
    one = (C.c_int32 * 1)(_lib.FIELD_ID["ssh"])
    host = (C.c_double * 4)()
    assert lib.ocn_ens_spread_save(None, one, 1, None) == ERR_ARG
    assert b"ens_spread_save" in lib.ocn_last_error()
    assert lib.ocn_ens_spread_save(None, None, 1, None) == ERR_ARG
    assert lib.ocn_ens_inflate(None, one, 1, None, 1, 0.5) == ERR_ARG
    assert b"ens_inflate" in lib.ocn_last_error()
    assert lib.ocn_ens_inflate(None, None, 1, None, 0, 1.0) == ERR_ARG
    assert lib.ocn_ens_inflate_download(None, 0, _lib.FIELD_ID["ssh"], 1, host) == ERR_ARG
    assert b"ens_inflate_download" in lib.ocn_last_error()
    assert lib.ocn_ens_inflate_download(None, 0, _lib.FIELD_ID["ssh"], 0, None) == ERR_ARG


def test_enum_values(tmp_path):
    from ocean_model_arch_amd import _lib, ens_inflate_rule
    names = ["OCN_ENS_INFLATE_CONST", "OCN_ENS_INFLATE_RTPS", "OCN_ENS_INFLATE_PRIOR_SPREAD", "OCN_ENS_INFLATE_FACTOR"]
    lines = ['#include <stdio.h>', f'#include "{HEADER}"', "int main(void) {"]
    lines += [f'printf("{nm} %d\\n", {nm});' for nm in names]
    lines.append("return 0; }")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines() if line)
    want = {"OCN_ENS_INFLATE_CONST": _lib.ENS_INFLATE_MODE["const"], "OCN_ENS_INFLATE_RTPS": _lib.ENS_INFLATE_MODE["rtps"],
            "OCN_ENS_INFLATE_PRIOR_SPREAD": _lib.ENS_INFLATE_WHAT["prior_spread"],
            "OCN_ENS_INFLATE_FACTOR": _lib.ENS_INFLATE_WHAT["factor"]}
    assert {k: int(v) for k, v in got.items()} == want
    assert (ens_inflate_rule.CONST, ens_inflate_rule.RTPS) == (want["OCN_ENS_INFLATE_CONST"], want["OCN_ENS_INFLATE_RTPS"])


def test_wrapper_names_the_state():
    from ocean_model_arch_amd import ensemble
    assert ensemble.STATE == R.STATE
