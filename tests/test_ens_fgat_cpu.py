"""The rule of observations at their own times (include/ocn_sw.h ocn_ens_record_sample, ocn_ens_assimilate_rec) in
Python, without a device: ens_record_rule.interp against a scalar loop over Python floats, ens_record_rule.at_steps
at and between the records, and every refusal of ens_record_rule.check_obs.  Every comparison is bitwise
(bits_equal: the int64 views, NaN by position).  Tolerance: none.
"""
import math

import numpy as np
import pytest

from ocean_model_arch_amd import _lib
from ocean_model_arch_amd import ens_record_rule as R
from tests.ens_assim_ref import bits_equal


def scalar_interp(series, rows, rec, wt, cols):
    """The rule one observation and one member at a time, on Python floats."""
    out = np.zeros((len(rows), len(cols)))
    for j in range(len(rows)):
        for m, c in enumerate(cols):
            a = float(series[rec[j], rows[j], c])
            w = float(wt[j])
            if w == 0.0:
                out[j, m] = series[rec[j], rows[j], c]     # (the copy itself: a NaN keeps its payload)
                continue
            b = float(series[rec[j] + 1, rows[j], c])
            p = b - a
            q = w * p
            out[j, m] = a + q
    return out


def _series(records=7, nobs=5, n=9, seed=0):
    """Random values over 40 binades with a -0.0, a NaN with a payload, an infinity and subnormals planted."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((records, nobs, n)) * 2.0 ** rng.integers(-20, 20, (records, nobs, n))
    s[1, 2, 3] = -0.0
    s[2, 2, 3] = 0.0
    s[3, 1, 4] = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]
    s[4, 0, 0] = np.inf
    s[0, 4, :] = 5e-324 * np.arange(1, n + 1)
    s[1, 4, :] = 2.5e-310
    return s


def _obs(records, nobs, count, seed):
    """`count` observations over every row and record, the weights 0, -0.0, 0.5, a non-dyadic one and the largest
    below 1 in turn (0 at the last record)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, nobs, count)
    rec = rng.integers(0, records, count)
    kinds = np.array([0.0, -0.0, 0.5, 0.3, np.nextafter(1.0, 0.0), 1.0 / 3.0])
    wt = kinds[np.arange(count) % len(kinds)]
    wt = np.where(rec == records - 1, 0.0, wt)
    return rows, rec, wt


def test_interp_is_the_scalar_loop():
    s = _series()
    rows, rec, wt = _obs(7, 5, 400, 1)
    # the planted values, read with and without a weight
    rows[:8] = [2, 2, 2, 1, 1, 0, 4, 4]
    rec[:8] = [1, 1, 2, 3, 2, 4, 0, 0]
    wt[:8] = [0.0, 0.5, 0.3, 0.0, 0.5, 0.3, 0.0, 0.7]
    for cols in (None, [0, 3, 4], [8, 1]):
        got = R.interp(s, rows, rec, wt, cols)
        want = scalar_interp(s, rows, rec, wt, list(range(9)) if cols is None else cols)
        assert got.shape == want.shape and bits_equal(got, want), cols
    got = R.interp(s, rows, rec, wt)
    assert np.signbit(got[0, 3]) and got[0, 3] == 0.0                  # -0.0 copied
    assert got[3].view(np.uint64)[4] == 0x7FF8000000ABCDEF             # the NaN's payload copied
    assert np.isnan(got[4, 4]) and np.isnan(got[5, 0])                 # NaN and inf - inf propagate
    assert bits_equal(got[6], s[0, 4])                                 # subnormals copied


def test_zero_weight_is_a_bit_copy():
    """wt = +0.0 and -0.0: the record itself, whatever it holds and whatever follows it; the last record included."""
    s = _series()
    rows = np.repeat(np.arange(5), 7)
    rec = np.tile(np.arange(7), 5)
    for w in (0.0, -0.0):
        got = R.interp(s, rows, rec, np.full(35, w))
        assert bits_equal(got, s[rec, rows])
    # a + 0.0 * (b - a) would not be: -0.0 turns +0.0, and an infinity next door turns the value NaN
    s2 = _series()
    s2[2, 2, 3] = np.inf
    assert bits_equal(R.interp(s2, [2], [1], [0.0])[0, 3], np.float64(-0.0))


def test_repeated_rows_and_one_observation():
    s = _series()
    got = R.interp(s, [1, 1, 1, 1], [0, 0, 1, 1], [0.0, 0.25, 0.75, 0.0])
    assert bits_equal(got, scalar_interp(s, [1, 1, 1, 1], [0, 0, 1, 1], [0.0, 0.25, 0.75, 0.0], list(range(9))))
    one = R.interp(s, [0], [6], [0.0], cols=[1])
    assert one.shape == (1, 1) and bits_equal(one[0, 0], s[6, 0, 1])


@pytest.mark.parametrize("every", [1, 3])
def test_at_steps(every):
    records = 6
    for r in range(records):                                   # the record times, first and last included
        assert R.at_steps(float((r + 1) * every), every, records) == (r, 0.0)
        assert R.at_steps((r + 1) * every, every, records) == (r, 0.0)
    for r in range(records - 1):                               # between records
        rec, wt = R.at_steps((r + 1.5) * every, every, records)
        assert (rec, wt) == (r, 0.5)
        rec, wt = R.at_steps((r + 1) * every + 0.25 * every, every, records)
        assert (rec, wt) == (r, 0.25)
    s = every * 2.3                                            # a non-dyadic one: x = s / every - 1.0, as stated
    x = s / every - 1.0
    assert R.at_steps(s, every, records) == (math.floor(x), x - math.floor(x))
    rec, wt = R.at_steps(np.nextafter((records) * every, 0.0), every, records)
    assert rec == records - 2 and 0.0 < wt < 1.0               # just before the last record
    rec, wt = R.at_steps(np.array([every, 1.5 * every, records * every]), every, records)
    assert rec.dtype == np.int32 and wt.dtype == np.float64
    assert rec.tolist() == [0, 0, records - 1] and wt.tolist() == [0.0, 0.5, 0.0]
    for bad in (every - 0.5, 0.0, -1.0, records * every + 0.5, np.nextafter(float(every), 0.0), np.nan, np.inf):
        with pytest.raises(ValueError):
            R.at_steps(bad, every, records)
    with pytest.raises(ValueError):
        R.at_steps(np.array([every, records * every + 1.0]), every, records)


def test_at_steps_arguments():
    with pytest.raises(ValueError):
        R.at_steps(1.0, 0, 3)
    with pytest.raises(ValueError):
        R.at_steps(1.0, 1, 0)                                  # no record taken yet
    with pytest.raises(TypeError):
        R.at_steps(1.0, 1.5, 3)
    with pytest.raises(TypeError):
        R.at_steps(1.0, 1, True)
    assert R.at_steps(1.0, 1, 1) == (0, 0.0)                   # one record: first and last


def test_every_validation_error():
    ok = dict(rows=[0, 4, 2], rec=[0, 5, 6], wt=[0.0, 0.5, 0.0], nobs_r=5, records=7)
    ra, ca, wa = R.check_obs(**ok)
    assert ra.dtype == ca.dtype == np.int32 and wa.dtype == np.float64 and wa.flags.c_contiguous
    assert R.check_obs([1], [0], [-0.0], 5, 1)[2][0] == 0.0    # -0.0 is a zero weight, at the last record too
    cases = {"no record taken yet": dict(records=0), "no observation": dict(rows=np.zeros(0, dtype=np.int64), rec=np.zeros(0, dtype=np.int64), wt=[]),
             "too many": dict(max_obs=2), "unequal lengths": dict(wt=[0.0, 0.5]), "2-D": dict(rows=[[0, 4, 2]]),
             "row -1": dict(rows=[0, -1, 2]), "row nobs_r": dict(rows=[0, 5, 2]),
             "rec -1": dict(rec=[-1, 5, 6]), "rec records": dict(rec=[0, 5, 7]),
             "wt -tiny": dict(wt=[0.0, -5e-324, 0.0]), "wt 1": dict(wt=[0.0, 1.0, 0.0]), "wt nan": dict(wt=[0.0, np.nan, 0.0]),
             "wt inf": dict(wt=[0.0, np.inf, 0.0]), "wt at the last record": dict(wt=[0.0, 0.5, 5e-324])}
    for what, change in cases.items():
        with pytest.raises(ValueError):
            R.check_obs(**{**ok, **change})
            pytest.fail(what)
    for what, change in {"float rows": dict(rows=[0.0, 4.0, 2.0]), "float records": dict(rec=[0.0, 5.0, 6.0])}.items():
        with pytest.raises(TypeError):
            R.check_obs(**{**ok, **change})
            pytest.fail(what)
    s = _series()
    with pytest.raises(ValueError):
        R.interp(s[0], [0], [0], [0.0])                        # not (records, nobs, n)
    with pytest.raises(ValueError):
        R.interp(s, [0], [0], [0.0], cols=[9])
    with pytest.raises(ValueError):
        R.interp(s, [0], [6], [0.5])                           # record 7 does not exist
    with pytest.raises(ValueError):
        R.interp(s, [5], [0], [0.0])


def test_interface():
    assert {"ocn_ens_record_sample", "ocn_ens_assimilate_rec"} <= set(_lib.ENS_SYMBOLS)
    assert R.MAX_SAMPLE_OBS == 65536
    from ocean_model_arch_amd.ensemble import OceanEnsemble
    assert callable(OceanEnsemble.sample_recorded) and callable(OceanEnsemble.assimilate_recorded)
