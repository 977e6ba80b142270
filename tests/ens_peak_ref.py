"""The peak map for the tests (include/ocn_sw.h ocn_ens_peak_*): the CPU oracle stepped one step(tau) at a time
(tests/ens_forcing_ref.py forced_reference: its "series" holds the state after every step; the forcing of a forced
member is set from the numpy restatement before each step) with the numpy rule
(ocean_model_arch_amd/ens_peak_rule.py) applied after each step.  No device, no library.

A run is one of tests/ens_forcing_ref.py RUNS, forced as there or with no storm at all: the first short call of
FIRST plain steps, then peak_begin, then the run's calls.  reference() gives P and S of one member after every call.
"""
import functools

from ocean_model_arch_amd import ens_peak_rule as PR
from tests import ens_forcing_ref as R
from tests import shapes as S

FIRST = R.FIRST
CALLS = (2, 5, 4, 1, 6)


def interiors(shape, params=None):
    """{(bm, bn): (i0, i1, j0, j1)}: the interior of every oracle block as inclusive array indices."""
    om = S.oracle_model(shape, params=params)
    return {(b.bm, b.bn): (b.nxs - b.bx1, b.nxe - b.bx1, b.nys - b.by1, b.nye - b.by1) for b in om.blocks}


def series(name, i, forced, calls=CALLS, first=FIRST):
    """The state after every step of member i of run `name` ({(bm, bn): {field: array}} per step, the first
    `first` plain steps included), with its storm (forced and the run forces it) or with none."""
    shape, params, classes, _, _ = R.RUNS[name]
    storm = R.run_storm(name, i) if forced and i in R.run_forced(name) else None
    times = R.call_times(tuple(calls), S.tau_of(params))
    ref = R.forced_reference(shape, classes[i], 1000 * i, storm, R.MODEL if storm is not None else None, times, params, 0, first)
    return ref["series"], ref


@functools.lru_cache(maxsize=256)
def reference(name, i, field, forced, calls=CALLS, first=FIRST):
    """Member i's peaks of `field` in run `name`: a list with one entry per call, {(bm, bn): {"max": (P, S),
    "min": (P, S)}} as they stand after that call (copies), peak_begin having come after the first `first` steps
    (first = 0: before any step).  Callers do not write into it."""
    shape, params, classes = R.RUNS[name][:3]
    ser, _ = series(name, i, forced, calls, first)
    inner = interiors(shape, params)
    start = None
    if first == 0:   # (peak_begin on the state as init and the uploads left it)
        om = R.loaded(shape, classes[i], 1000 * i, params)
        start = {(b.bm, b.bn): om.f[k] for k, b in enumerate(om.blocks)}
    cur = {}
    for key, box in inner.items():
        x = (start if first == 0 else ser[first - 1])[key][field]
        cur[key] = {"max": PR.begin(x, box), "min": PR.begin(x, box)}
    out, k = [], 0
    for n in calls:
        for _ in range(n):
            k += 1
            for key, box in inner.items():
                x = ser[first + k - 1][key][field]
                PR.update(*cur[key]["max"], x, k, box, minimum=False)
                PR.update(*cur[key]["min"], x, k, box, minimum=True)
        out.append({key: {w: (P.copy(order="F"), Sx.copy(order="F")) for w, (P, Sx) in v.items()} for key, v in cur.items()})
    return out


def final_state(name, i, forced, calls=CALLS, first=FIRST):
    """Every field of member i after the calls ({(bm, bn): {field: array}}): what complete() must leave."""
    return series(name, i, forced, calls, first)[1]


def unchecked_series(shape, cls, off, storm, model, times, params=None, first=FIRST):
    """forced_reference's "series" of `field`s for a member that blows up: the oracle's step raises once
    check_ssh_err finds |ssh| >= 1e4 -- behind the step's last stage, so the state is that step's -- and the run
    goes on from it, as the device's does.  One {field: array} of block (1, 1) per step, the `first` plain steps
    included."""
    om = R.loaded(shape, cls, off, params)
    tau, out = S.tau_of(params), []
    for s in range(first + len(times)):
        if s >= first:
            R.set_forcing(om, storm, model, times[s - first])
        try:
            om.step(tau)
        except FloatingPointError:
            pass
        out.append({nm: om.f[0][nm].copy(order="F") for nm in R.STATE})
    return out


@functools.lru_cache(maxsize=8)
def still_reference(shape, field, steps, first=FIRST):
    """A member whose six state fields are +0.0 everywhere (uploaded over what init left): ({"max": (P, S), "min":
    (P, S)} of block (1, 1) after `first` + `steps` oracle steps with peak_begin behind the first `first`, the
    largest |value| of any state field after any step)."""
    om = S.oracle_model(shape)
    for nm in R.STATE:
        om.f[0][nm][...] = 0.0
    box = interiors(shape)[(1, 1)]
    top, cur = 0.0, None
    for s in range(first + steps):
        om.step(1.0)
        top = max([top] + [float(abs(om.f[0][nm]).max()) for nm in R.STATE])
        if s == first - 1:
            cur = {"max": PR.begin(om.f[0][field], box), "min": PR.begin(om.f[0][field], box)}
        elif s >= first:
            PR.update(*cur["max"], om.f[0][field], s - first + 1, box, minimum=False)
            PR.update(*cur["min"], om.f[0][field], s - first + 1, box, minimum=True)
    return cur, top


def land(shape, params=None):
    """{(bm, bn): bool array}: lu < 0.5 on the block's array."""
    om = S.oracle_model(shape, params=params)
    return {(b.bm, b.bn): om.f[k]["lu"] < 0.5 for k, b in enumerate(om.blocks)}
