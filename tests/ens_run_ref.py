"""The reference of OceanEnsemble.run() for the tests (include/ocn_sw.h ocn_ens_run): the CPU oracle stepped one
step(tau) at a time (tests/ens_forcing_ref.py forced_reference, through tests/ens_peak_ref.py series: the state after
every step, a forced member's forcing set from the numpy restatement before each step), with the operator's numpy
restatement (ens_obs_rule.apply) applied after every due step (ens_record_rule.due) and the peak rule after every
step (tests/ens_peak_ref.py reference).  No device, no library.

A run is one of tests/ens_forcing_ref.py RUNS whose members all have a storm there; which of them are forced in a
case is the case's own (`storms`: the forced members; a member outside it steps with no storm at all).  The first
short call of FIRST plain steps comes first, then record(), peak_begin() and the calls.
"""
import functools
from types import SimpleNamespace

import numpy as np

from ocean_model_arch_amd import ens_obs_rule, ens_record_rule
from tests import ens_forcing_ref as R
from tests import ens_obs_ref as O
from tests import ens_peak_ref as K
from tests import shapes as S

FIRST = R.FIRST
CALLS = K.CALLS            # (2, 5, 4, 1, 6)
SHORT = (2, 5, 4)
# the "groups" run's three member sets (nine members): under capacity 7 the forced members (general bodies) plan
# apart from the others -- {0, 1, 2} records, tracks and forces, {6} only forces, {3, 4, 5} records and tracks with
# no storm, {7, 8} only tracks: two groups hold no recorded member
GROUPS_FORCED = (0, 1, 2, 6)
GROUPS_RECORDED = (1, 2, 3, 4)
GROUPS_TRACKED = (2, 4, 5, 8)


def members_of(name):
    return len(R.RUNS[name][2])


def all_members(name):
    assert R.RUNS[name][3] is None, name   # (K.series' `forced` flag is then the member's own)
    return tuple(range(members_of(name)))


@functools.lru_cache(maxsize=16)
def blocks_of(name):
    """The oracle's blocks of run `name` as ens_obs_rule.apply and tests/ens_obs_ref.py block_of take them (k: the
    index in the oracle's order), and {k: (bm, bn)}."""
    shape, params = R.RUNS[name][:2]
    om = S.oracle_model(shape, params=params)
    blocks = [SimpleNamespace(k=k, bm=b.bm, bn=b.bn, nx_start=b.nxs, nx_end=b.nxe, ny_start=b.nys, ny_end=b.nye,
                              bnd_x1=b.bx1, bnd_x2=b.bx2, bnd_y1=b.by1, bnd_y2=b.by2) for k, b in enumerate(om.blocks)]
    return blocks, {b.k: (b.bm, b.bn) for b in blocks}


# ---------------------------------------------------------------- the stations
MASK_OF = {"ssh": "lu", "sshp": "lu", "ubrtr": "lcu", "ubrtrp": "lcu", "vbrtr": "lcv", "vbrtrp": "lcv"}


@functools.lru_cache(maxsize=16)
def wet_points(name, field):
    """The 1-based global points of the interiors at which `field` lives on water (its own mask > 0.5), row by row
    of the basin: where a forced run moves the field at every step."""
    shape, params = R.RUNS[name][:2]
    om = S.oracle_model(shape, params=params)
    pts = []
    for k, b in enumerate(om.blocks):
        m = om.f[k][MASK_OF[field]]
        for j in range(b.nys, b.nye + 1):
            for i in range(b.nxs, b.nxe + 1):
                if m[i - b.bx1, j - b.by1] > 0.5:
                    pts.append((i, j))
    return tuple(sorted(pts, key=lambda p: (p[1], p[0])))


def _spread(pts, n, phase=0):
    """n of the points, evenly spread over the list (all of them, cycled, where there are fewer)."""
    assert pts
    return [pts[(phase + (q * len(pts)) // n) % len(pts)] for q in range(n)]


@functools.lru_cache(maxsize=32)
def operator(name, kind):
    """The cases' operators, every term on a wet interior point of its field.  Every row reads a velocity: ssh
    feels a storm one step after the velocities do, so a row of ssh alone is the unforced run's at the first
    forced step.
      one    nobs = 1: ubrtr at one point
      five   3 rows: a row of 5 terms over three fields (more than the device's group of 4 terms), a unit row and
             a 2-term row
      wrap   300 rows (more than one tile's 256 threads): ssh + ubrtr, ubrtr alone and vbrtr alone in turn
    (a basin with no wet point of a field -- the 1 x 1 block -- takes ssh at its interior points instead)."""
    shape = R.RUNS[name][0]
    wet = {f: wet_points(name, f) for f in ("ssh", "ubrtr", "vbrtr")}
    if not wet["ssh"]:   # (no water at all: the interior's points as they are)
        blocks, _ = blocks_of(name)
        wet["ssh"] = tuple((i, j) for b in blocks for j in range(b.ny_start, b.ny_end + 1) for i in range(b.nx_start, b.nx_end + 1))
    for f in ("ubrtr", "vbrtr"):
        if not wet[f]:
            wet[f] = wet["ssh"]
    fld = lambda f: f if wet_points(name, f) else "ssh"   # noqa: E731
    if kind == "one":
        rows = [[(fld("ubrtr"),) + _spread(wet["ubrtr"], 3)[1] + (1.0,)]]
    elif kind == "five":
        a, b, c = _spread(wet["ssh"], 3), _spread(wet["ubrtr"], 3, 1), _spread(wet["vbrtr"], 3, 2)
        rows = [[("ssh",) + a[0] + (0.5,), (fld("ubrtr"),) + b[0] + (-1.25,), ("ssh",) + a[1] + (0.25,),
                 (fld("vbrtr"),) + c[0] + (2.0,), (fld("ubrtr"),) + b[1] + (0.75,)],
                [(fld("vbrtr"),) + c[1] + (1.0,)],
                [("ssh",) + a[2] + (-0.5,), (fld("ubrtr"),) + b[2] + (3.0,)]]
    elif kind == "wrap":
        n = 300
        pick = {f: _spread(wet[f], n // 3, q) for q, f in enumerate(("ssh", "ubrtr", "vbrtr"))}
        rows = [([("ssh",) + pick["ssh"][r // 3] + (0.5,)] if r % 3 == 0 else []) +
                [(fld(f),) + pick[f][r // 3] + (1.0,)] for r in range(n) for f in [("ubrtr", "ubrtr", "vbrtr")[r % 3]]]
    else:
        raise ValueError(kind)
    anchors = np.array([[r[0][1], r[0][2]] for r in rows], dtype=np.int64)
    op = ens_obs_rule.ObsOperator.from_rows(rows, anchors)
    assert len(op.names) <= 3, (name, kind, shape)
    return op


# ---------------------------------------------------------------- the schedule
def due(calls, every, counted=0):
    """(the counted steps at which a record is due, the due steps of each call 1-based within it)."""
    at, per_call = [], []
    for n in calls:
        d = ens_record_rule.due(counted, n, every)
        per_call.append(d)
        at += [counted + s for s in d]
        counted += n
    return at, per_call


# ---------------------------------------------------------------- the products
def states(name, i, forced, calls, first=FIRST):
    """Member i's six state fields after every counted step ({(bm, bn): {field: array}} per step), with its storm
    (forced) or with none."""
    return K.series(name, i, bool(forced), tuple(calls), first)[0][first:]


@functools.lru_cache(maxsize=128)
def records(name, kind, recorded, storms, calls, every, first=FIRST):
    """The series of the whole run: (records, nobs, len(recorded)), column m the m-th recorded member; storms: the
    forced members.  Callers do not write into it."""
    op = operator(name, kind)
    blocks, key = blocks_of(name)
    find = O.block_of(blocks)
    at, _ = due(calls, every)
    runs = [states(name, i, i in storms, calls, first) for i in recorded]
    out = np.zeros((len(at), op.nobs, len(recorded)))
    for r, s in enumerate(at):
        fields = {nm: {b.k: [run[s - 1][key[b.k]][nm] for run in runs] for b in blocks} for nm in op.names}
        out[r] = ens_obs_rule.apply(op, fields, blocks, find)
    return out


def peaks(name, i, forced, calls, field="ssh", first=FIRST):
    """Member i's peaks after every call (tests/ens_peak_ref.py reference)."""
    return K.reference(name, i, field, bool(forced), tuple(calls), first)


def final_state(name, i, forced, calls, first=FIRST):
    return K.final_state(name, i, bool(forced), tuple(calls), first)


def same(got, want):
    """Bitwise, NaN by position."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        if not np.array_equal(np.isnan(got), nan):
            return False
        return got[~nan].tobytes() == want[~nan].tobytes()
    return got.tobytes() == want.tobytes()
