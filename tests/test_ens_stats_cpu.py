"""CPU checks of the ensemble statistics (ocn_ens_stats, ocn_ens_extrema): the numpy restatement that the
GPU tests compare against (tests/ens_stats_ref.py) is itself checked against an independent scalar loop
over Python floats; the new struct's layout and the entries' null-ensemble errors need no device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import ens_stats_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ocn_sw.h")


@pytest.fixture(scope="module")
def lib():
    import ocean_model_arch_amd as amd
    if not os.path.exists(amd._lib.LIB_PATH):
        amd.build()
    return amd.lib()


def _members():
    """7 members of a 5 x 4 array with a NaN, an Inf, a +0 / -0 tie and an all-NaN column."""
    x = np.random.default_rng(77).uniform(-1.0, 1.0, (7, 5, 4))
    x[1, 0, 0] = np.nan                    # one NaN: dropped by min / max, poisons the mean
    x[0, 3, 3] = np.nan                    # a NaN in the first member: `c != c` takes the next number
    x[3, 1, 0] = np.inf                    # an Inf: mean Inf, variance NaN (Inf - Inf)
    x[:, 2, 1] = 1.0 + np.arange(7)        # the others larger than the tie
    x[0, 2, 1], x[2, 2, 1] = 0.0, -0.0     # +0 then -0: min keeps +0 (the earlier member's bits)
    x[:, 4, 2] = -1.0 - np.arange(7)
    x[1, 4, 2], x[5, 4, 2] = -0.0, 0.0     # -0 then +0: max keeps -0
    x[:, 4, 3] = np.nan                    # all NaN
    return x


def _scalar(col, what):
    """One column by the definitions, in Python floats."""
    n = len(col)
    s = col[0]
    for v in col[1:]:
        s = s + v
    mean = s / float(n)
    if what == "mean":
        return mean
    if what in ("var", "spread"):
        d = col[0] - mean
        q = d * d
        for v in col[1:]:
            d = v - mean
            q = q + d * d
        var = q / float(n - 1)
        if what == "var":
            return var
        return math.sqrt(var) if var >= 0.0 else float("nan")   # (a variance is a sum of squares: NaN or >= 0)
    c = col[0]
    for v in col[1:]:
        if ((v < c) if what == "min" else (v > c)) or c != c:
            c = v
    return c


@pytest.mark.parametrize("use", [list(range(7)), [0, 2, 4], [1, 3], [5]], ids=str)
def test_restatement_against_scalar_loop(use):
    x = _members()[use]
    what = R.STATS if len(use) > 1 else ("mean", "min", "max")
    got = R.stats(list(x), what)
    assert set(got) == set(what)
    for nm in what:
        want = np.empty(x.shape[1:])
        for i in range(x.shape[1]):
            for j in range(x.shape[2]):
                want[i, j] = _scalar([float(v) for v in x[:, i, j]], nm)
        assert R.bits_equal(got[nm], want), (nm, got[nm], want)


def test_special_values_of_the_restatement():
    x = _members()
    got = R.stats(list(x))
    sign = lambda v: math.copysign(1.0, v)   # noqa: E731
    assert got["min"][2, 1] == 0.0 and sign(got["min"][2, 1]) == 1.0      # +0 (member 0) kept over -0 (member 2)
    assert got["max"][4, 2] == 0.0 and sign(got["max"][4, 2]) == -1.0     # -0 (member 1) kept over +0 (member 5)
    assert got["min"][0, 0] == x[[0, 2, 3, 4, 5, 6], 0, 0].min() and np.isnan(got["mean"][0, 0])
    assert got["max"][3, 3] == x[1:, 3, 3].max()                          # a leading NaN is dropped
    assert got["max"][1, 0] == np.inf and got["mean"][1, 0] == np.inf and np.isnan(got["var"][1, 0])
    assert all(np.isnan(got[nm][4, 3]) for nm in R.STATS)
    assert not R.bits_equal(np.array([0.0]), np.array([-0.0])) and R.bits_equal(np.array([np.nan]), np.array([-np.nan]))
    assert not R.bits_equal(np.array([np.nan, 1.0]), np.array([1.0, np.nan]))


def test_extrema_restatement():
    a = np.arange(48, dtype=np.float64).reshape(8, 6, order="F")
    lu = np.ones((8, 6), dtype=np.float32, order="F")
    lu[3, 3] = 0.0
    # a(i, j) = i + 8 j; the interior holds 18 .. 21 and 26 .. 29; (0, 0) is halo and (3, 3) land: ignored
    a[2, 2], a[4, 3], a[5, 2], a[0, 0], a[3, 3] = np.nan, np.inf, -np.inf, -99.0, 1.0e9
    got = R.extrema([a], [lu], [(2, 6, 2, 4)])
    assert got == {"min": 19.0, "max": 29.0, "nonfinite": 3, "count": 7}, got
    assert R.extrema([a], [np.zeros_like(lu)], [(2, 6, 2, 4)]) == {"min": np.inf, "max": -np.inf, "nonfinite": 0, "count": 0}


def test_extrema_struct_layout(tmp_path):
    """sizeof / offsetof of ocn_ens_extrema_t from the C header (gcc probe) == the ctypes mirror."""
    from ocean_model_arch_amd import _lib
    cs, t = "ocn_ens_extrema_t", _lib.OcnEnsExtrema
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             f'printf("size %zu\\n", sizeof({cs}));']
    for fname, _ in t._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cs}, {fname}));')
    lines += ['printf("bits %d %d %d %d %d\\n", OCN_ENS_STAT_MEAN, OCN_ENS_STAT_VAR, OCN_ENS_STAT_SPREAD, '
              'OCN_ENS_STAT_MIN, OCN_ENS_STAT_MAX);', "return 0; }"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(ln.split(None, 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert C.sizeof(t) == int(got["size"]) == 32
    for fname, _ in t._fields_:
        assert getattr(t, fname).offset == int(got[fname]), fname
    assert [int(v) for v in got["bits"].split()] == [_lib.ENS_STATS[n] for n in R.STATS]


def test_null_ensemble_is_an_argument_error(lib):
    from ocean_model_arch_amd import _lib
    host = (C.c_double * 4)()
    ext = (_lib.OcnEnsExtrema * 1)()
    assert lib.ocn_ens_stats(None, 0, _lib.FIELD_ID["ssh"], None, 1) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_stats_download(None, 0, 1, host) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_stats_output_r4(None, 0, 1, C.c_float(0.0), host) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_extrema(None, _lib.FIELD_ID["ssh"], ext) == _lib.OCN_ERR_ARG
    assert b"null ensemble" in lib.ocn_last_error()


def test_abi_version_unchanged(lib):
    assert lib.ocn_abi_version() == 5
