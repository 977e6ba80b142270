"""The station recorder's schedule in Python (include/ocn_sw.h ocn_ens_record_due, ocn_ens_step_record): which
steps of a call write a record.  Pure Python: no device, no library.

A recorder counts the steps of its step_record() calls.  After the counted step (r + 1) * every it writes
record r, so a call of `nsteps` steps made after `counted` counted steps writes a record after each of its
1-based steps s with (counted + s) % every == 0.

Observations at their own times (ocn_ens_record_sample, ocn_ens_assimilate_rec): `at_steps` maps an
observation's time to a record and a weight, `interp` restates the rule that forms the members' equivalents
from the series, `check_obs` refuses what the entries refuse.  With a = series[rec][row][col] and
b = series[rec + 1][row][col]:

    hx[j][m] = a                                  if wt == 0.0  (a bit copy; b is not read)
             = a + q,  p = b - a;  q = wt * p     otherwise     (one IEEE double operation each, nothing fused)
"""
from __future__ import annotations

import numpy as np

MAX_SERIES_BYTES = 1 << 30   # max_records x nobs x n doubles
MAX_SAMPLE_OBS = 65536       # ocn_ens_record_sample: observations per call


def check(every: int, max_records: int) -> None:
    """ValueError as ocn_ens_record_begin refuses them."""
    if every < 1:
        raise ValueError(f"record: every = {every} < 1")
    if max_records < 1:
        raise ValueError(f"record: max_records = {max_records} < 1")


def due(counted: int, nsteps: int, every: int) -> list[int]:
    """The 1-based steps of a call at which a record is due, in rising order."""
    if counted < 0 or nsteps < 0 or every < 1:
        raise ValueError(f"due: counted = {counted}, nsteps = {nsteps}, every = {every}")
    return [s for s in range(1, nsteps + 1) if (counted + s) % every == 0]


def at_steps(steps, every: int, records: int):
    """An observation's time -> (rec, wt).  `steps`: the time in counted steps since record_begin, a float (it
    may lie between steps) or an array of them; record r lies at step (r + 1) * every, so with
    x = steps / every - 1.0:  rec = floor(x), wt = x - rec (exact: 0.0 <= wt < 1.0), and the last record itself
    maps to (records - 1, 0.0).  A scalar gives (int, float), an array (int32 array, float64 array).  ValueError
    for a time before the first record, after the last, or not finite."""
    if isinstance(every, bool) or isinstance(records, bool) or not isinstance(every, (int, np.integer)) or \
            not isinstance(records, (int, np.integer)):
        raise TypeError(f"at_steps: every = {every!r}, records = {records!r}, not integers")
    if every < 1 or records < 1:
        raise ValueError(f"at_steps: every = {every} < 1 or no record taken yet (records = {records})")
    s = np.asarray(steps, dtype=np.float64)
    x = s / np.float64(every) - 1.0
    if not np.isfinite(x).all() or (x < 0.0).any() or (x > records - 1).any():
        raise ValueError(f"at_steps: a time outside the records taken, steps {every} .. {records * every}")
    rec = np.floor(x)
    wt = x - rec
    if s.ndim == 0:
        return int(rec), float(wt)
    return rec.astype(np.int32), wt


def check_obs(rows, rec, wt, nobs_r: int, records: int, max_obs: int = MAX_SAMPLE_OBS):
    """The observations of a call as ocn_ens_record_sample takes them: (rows int32, rec int32, wt float64), each of
    shape (nobs,).  TypeError for rows or records that are not integers, ValueError as the entry refuses them: no
    record taken yet, no observation or more than `max_obs`, unequal lengths, a row outside 0 .. nobs_r - 1, a
    record outside 0 .. records - 1, a weight that is not finite or outside [0, 1), a nonzero weight at the last
    record."""
    ra, ca, wa = np.asarray(rows), np.asarray(rec), np.asarray(wt, dtype=np.float64)
    for what, a in (("rows", ra), ("records", ca)):
        if a.dtype.kind not in "iu":
            raise TypeError(f"{what} of dtype {a.dtype}, not integers")
    if records < 1:
        raise ValueError("no record taken yet")
    if ra.ndim != 1 or ra.shape != ca.shape or ra.shape != wa.shape:
        raise ValueError(f"rows, records and weights of shapes {ra.shape}, {ca.shape}, {wa.shape}, not one (nobs,)")
    if not 1 <= len(ra) <= max_obs:
        raise ValueError(f"{len(ra)} observations, not 1..{max_obs}")
    if (ra < 0).any() or (ra >= nobs_r).any():
        raise ValueError(f"a row outside 0 .. {nobs_r - 1}, the recorder's operator")
    if (ca < 0).any() or (ca >= records).any():
        raise ValueError(f"a record outside 0 .. {records - 1}, the records taken")
    if not np.isfinite(wa).all() or (wa < 0.0).any() or (wa >= 1.0).any():
        raise ValueError("a weight that is not finite and in [0, 1)")
    if ((wa != 0.0) & (ca + 1 >= records)).any():
        raise ValueError("a nonzero weight at the last record")
    return ra.astype(np.int32), ca.astype(np.int32), np.ascontiguousarray(wa)


def interp(series, rows, rec, wt, cols=None) -> np.ndarray:
    """The rule in numpy: hx (nobs, n) from `series` (records, nobs_r, n_r), the observations' rows, records and
    weights (check_obs's conditions) and `cols`, the recorder's columns of the members in use (None: all).  numpy's
    elementwise subtract, multiply and add are single IEEE double operations and nothing is fused: the device's
    bits.  Where wt == 0.0 the value is copied, bit for bit, and record rec + 1 is not read."""
    s = np.asarray(series, dtype=np.float64)
    if s.ndim != 3:
        raise ValueError(f"interp: a series of shape {s.shape}, not (records, nobs, n)")
    ra, ca, wa = check_obs(rows, rec, wt, s.shape[1], s.shape[0], max_obs=max(len(np.atleast_1d(rows)), 1))
    ci = np.arange(s.shape[2]) if cols is None else np.asarray(cols, dtype=np.int64).ravel()
    if ((ci < 0) | (ci >= s.shape[2])).any():
        raise ValueError(f"interp: a column outside 0 .. {s.shape[2] - 1}")
    a = s[ca[:, None], ra[:, None], ci[None, :]]
    out = a.copy()
    mix = wa != 0.0
    if mix.any():
        am = a[mix]
        b = s[ca[mix][:, None] + 1, ra[mix][:, None], ci[None, :]]
        with np.errstate(all="ignore"):
            p = b - am
            q = wa[mix][:, None] * p
            out[mix] = am + q
    return out
