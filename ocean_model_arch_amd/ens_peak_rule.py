"""The peak map's rule in numpy (include/ocn_sw.h ocn_ens_peak_*; csrc/ens_peak_point.h is the text the device
compiles).  Pure numpy: no device, no library.

After ocn_ens_peak_begin, P holds the field's value and S is 0 at every interior point; outside the interior both
stay +0.0 / 0.  After the k-th step since then, with x the field's value after that step:

    MAX:  if (x > P or P != P): P = x; S = k          MIN: the same with <

-- ocn_ens_stats' MIN / MAX comparisons: a tie, +0.0 against -0.0 included, keeps the earlier step and its bits; a
NaN in P goes as soon as a number arrives; a NaN x never replaces a number.
"""
from __future__ import annotations

import operator

import numpy as np

FIELDS = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")   # the recorder's set
WHAT = {"max": 1, "min": 2}                                     # OCN_ENS_PEAK_MAX, OCN_ENS_PEAK_MIN
MAX_STEPS = 2 ** 31 - 1                                         # S is int32


def what_bits(what, who: str = "peak_begin") -> int:
    """The mask of a name or a sequence of names of WHAT.  TypeError for anything else than strings, ValueError for
    an unknown name or none at all."""
    names = (what,) if isinstance(what, str) else tuple(what)
    bits = 0
    for n in names:
        if not isinstance(n, str):
            raise TypeError(f"{who}: what holds {n!r}, not a string")
        if n not in WHAT:
            raise ValueError(f"{who}: what holds {n!r}, not one of {sorted(WHAT)}")
        bits |= WHAT[n]
    if not bits:
        raise ValueError(f"{who}: no extreme asked for")
    return bits


def which_bit(which, who: str = "peak") -> int:
    """One extreme's bit.  TypeError for anything else than a string, ValueError for an unknown name."""
    if not isinstance(which, str):
        raise TypeError(f"{who}: which = {which!r}, not a string")
    if which not in WHAT:
        raise ValueError(f"{who}: which = {which!r}, not one of {sorted(WHAT)}")
    return WHAT[which]


def check_field(name, who: str = "peak_begin") -> str:
    if not isinstance(name, str):
        raise TypeError(f"{who}: field = {name!r}, not a string")
    if name not in FIELDS:
        raise ValueError(f"{who}: field {name!r}, not one of {FIELDS}")
    return name


def check_threshold(threshold, who: str = "peak_exceed") -> float:
    if isinstance(threshold, (str, bytes, bool)) or np.ndim(threshold) != 0:
        raise TypeError(f"{who}: threshold = {threshold!r}, not a number")
    t = float(threshold)
    if t != t:
        raise ValueError(f"{who}: a threshold that is NaN")
    return t


def begin(x, interior):
    """(P, S) as ocn_ens_peak_begin leaves them for the field's array x: x and 0 on interior = (i0, i1, j0, j1),
    inclusive array indices, +0.0 and 0 elsewhere."""
    x = np.asarray(x, dtype=np.float64)
    i0, i1, j0, j1 = (operator.index(v) for v in interior)
    P = np.zeros(x.shape, dtype=np.float64, order="F")
    S = np.zeros(x.shape, dtype=np.int32, order="F")
    P[i0:i1 + 1, j0:j1 + 1] = x[i0:i1 + 1, j0:j1 + 1]
    return P, S


def update(P, S, x, k: int, interior, minimum: bool = False):
    """The rule for step k (1-based since begin) with the field's array x, in place on the interior of P and S."""
    k = operator.index(k)
    if not 1 <= k <= MAX_STEPS:
        raise ValueError(f"update: step {k} outside 1..{MAX_STEPS}")
    i0, i1, j0, j1 = (operator.index(v) for v in interior)
    sl = (slice(i0, i1 + 1), slice(j0, j1 + 1))
    p, s, v = P[sl], S[sl], np.asarray(x, dtype=np.float64)[sl]
    with np.errstate(invalid="ignore"):
        take = ((v < p) if minimum else (v > p)) | (p != p)
    p[take] = v[take]
    s[take] = k
    return P, S


def exceed(pmax, threshold: float):
    """ocn_ens_peak_exceed: per point the fraction of the arrays pmax[0 .. n) with a value > threshold (a NaN is
    not counted), (double)c / (double)n."""
    a = np.asarray(pmax, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = (a > float(threshold)).sum(axis=0)
    return np.asfortranarray(c.astype(np.float64) / float(len(a)))
