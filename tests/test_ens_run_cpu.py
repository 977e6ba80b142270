"""CPU checks of the one entry that steps with everything that is active (include/ocn_sw.h ocn_ens_run,
OceanEnsemble.run): the exceptions run() raises before any device call, the library's export and its refusals
that need no device, and the premises of the GPU runs (tests/test_gpu_ens_run.py) on the oracle alone
(tests/ens_run_ref.py).  No device anywhere."""
import ctypes as C

import numpy as np
import pytest

from ocean_model_arch_amd import _lib
from ocean_model_arch_amd.ensemble import OceanEnsemble
from tests import ens_forcing_ref as R
from tests import ens_peak_ref as K
from tests import ens_run_ref as A


class _NoDevice(OceanEnsemble):
    """run()'s own checks, which come before any call into the library: an ensemble without a handle."""

    def __init__(self):   # noqa: no context is created
        self.ens = None
        self.members = [None] * 3
        self._recording = False


def test_python_validation():
    e = _NoDevice()
    for bad in (1.0, "2", None, True):
        with pytest.raises(TypeError):
            e.run(bad)
    for kw in (dict(tau="1"), dict(tau=True), dict(tau=[1.0]), dict(t0="0"), dict(t0=False), dict(t0=np.zeros(2)),
               dict(check_every=1.0), dict(check_every=None)):
        with pytest.raises(TypeError):
            e.run(2, **kw)
    with pytest.raises(ValueError):
        e.run(-1)
    for kw in (dict(tau=float("nan")), dict(tau=float("inf")), dict(t0=float("nan")), dict(t0=-float("inf"))):
        with pytest.raises(ValueError):
            e.run(2, **kw)


def test_library_exports_the_entry():
    L = _lib.lib()
    assert "ocn_ens_run" in _lib.ENS_SYMBOLS and hasattr(L, "ocn_ens_run")
    assert L.ocn_ens_run.argtypes == [C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double]
    assert _lib.ENS_OPT_RUN_IN_LAUNCH == 7
    assert L.ocn_abi_version() == 5


def test_refusals_without_a_device():
    L = _lib.lib()
    assert L.ocn_ens_run(None, 1.0, 2, 1, 0, 0.0) == _lib.OCN_ERR_ARG
    assert b"null ensemble" in L.ocn_last_error()
    assert L.ocn_ens_run(None, 1.0, -1, 1, 1, 0.0) == _lib.OCN_ERR_ARG
    assert L.ocn_ens_set_option(None, _lib.ENS_OPT_RUN_IN_LAUNCH, 0) == _lib.OCN_ERR_ARG


# ---------------------------------------------------------------- the premises of the GPU runs
def test_schedule_of_the_calls():
    """Calls (2, 5, 4, 1, 6) behind the first short call, every = 3, through ocn_ens_record_due: records fall inside
    a launch (counted steps 3, 6, 9, 15), at the last step of a multi-step call (18), in the 1-step call (12), and
    the first call has none."""
    L = _lib.lib()
    counted, at, kinds = 0, [], []
    for n in A.CALLS:
        steps, cnt = (C.c_int32 * 8)(), C.c_int32(-1)
        assert L.ocn_ens_record_due(counted, n, 3, steps, 8, C.byref(cnt)) == _lib.OCN_OK
        d = list(steps[:cnt.value])
        at += [counted + s for s in d]
        kinds.append(["one" if n == 1 else "last" if s == n else "inside" for s in d])
        counted += n
    assert at == [3, 6, 9, 12, 15, 18]
    assert kinds == [[], ["inside", "inside"], ["inside"], ["one"], ["inside", "last"]]
    assert A.due(A.CALLS, 3) == (at, [[], [1, 4], [2], [1], [3, 6]])
    # every = 1: each call of two steps or more has records inside and one at its last step
    assert A.due(A.CALLS, 1)[1] == [list(range(1, n + 1)) for n in A.CALLS]


def _rows_move(ser, tag):
    """Every row of every column differs in bits between consecutive records."""
    a, b = ser[:-1].view(np.int64), ser[1:].view(np.int64)
    still = np.argwhere(a == b)
    assert not len(still), (tag, still[:8].tolist())


FORCED = [("one_tile", "one", 1), ("one_tile", "five", 1), ("one_tile", "wrap", 1), ("one_tile", "five", 3),
          ("many_tiles", "one", 1), ("many_tiles", "five", 3), ("one_point", "five", 1)]


@pytest.mark.parametrize("name,kind,every", FORCED)
def test_forced_stations_move_and_feel_the_storm(name, kind, every):
    """Every station row differs in bits between consecutive records in every member, and between the forced and
    the unforced run for every forced member (the 1 x 1 block has no wet face and no interior water to move: its
    forcing is +0.0 whatever the storm, so it is exempt from the second and asserted to be so)."""
    calls = A.CALLS if len(R.RUNS[name][4]) == 5 else R.RUNS[name][4]
    mem = A.all_members(name)
    forced = A.records(name, kind, mem, mem, calls, every)
    free = A.records(name, kind, mem, (), calls, every)
    assert forced.shape == (len(A.due(calls, every)[0]), A.operator(name, kind).nobs, len(mem))
    if name == "one_point":
        assert A.same(forced, free)
        return
    _rows_move(forced, (name, kind, every))
    same = np.argwhere(forced.view(np.int64) == free.view(np.int64))
    assert not len(same), (name, kind, every, same[:8].tolist())


@pytest.mark.parametrize("name,kind", [("one_tile", "five"), ("tau03", "five"), ("tau03", "wrap")])
def test_unforced_stations_move(name, kind):
    calls = A.CALLS if len(R.RUNS[name][4]) == 5 else R.RUNS[name][4]
    mem = A.all_members(name)
    _rows_move(A.records(name, kind, mem, (), calls, 1), (name, kind))


def test_member_sets_of_the_groups_case():
    """Nine members: the recorder on one subset, the peak on another, storms on a third; a forced member's rows
    differ from the same member's unforced ones."""
    name = "groups"
    rec, storms = A.GROUPS_RECORDED, A.GROUPS_FORCED
    got = A.records(name, "five", rec, storms, A.SHORT, 1)
    free = A.records(name, "five", rec, (), A.SHORT, 1)
    _rows_move(got, name)
    for m, i in enumerate(rec):
        col, col0 = got[:, :, m].view(np.int64), free[:, :, m].view(np.int64)
        assert (col != col0).all() if i in storms else (col == col0).all(), i
    assert set(rec) - set(A.GROUPS_TRACKED) and set(A.GROUPS_TRACKED) - set(storms) and set(storms) - set(rec)


@pytest.mark.parametrize("name,forced", [("one_tile", True), ("many_tiles", True), ("one_tile", False), ("tau03", False)])
def test_peak_premises_carry_over(name, forced):
    """What tests/test_ens_peak_cpu.py asserts for these runs: per call of two steps or more some interior point of
    some member has its Smax or Smin at a step of that call that is not its last, and some point at its last."""
    shape, params, classes, _, run_calls = R.RUNS[name]
    calls = K.CALLS if len(run_calls) == 5 else A.SHORT
    refs = [A.peaks(name, i, forced, calls) for i in range(len(classes))]
    box = K.interiors(shape, params)[(1, 1)]
    inner = (slice(box[0], box[1] + 1), slice(box[2], box[3] + 1))
    done = 0
    for c, n in enumerate(calls):
        s_all = np.stack([r[c][(1, 1)][w][1][inner] for r in refs for w in ("max", "min")])
        if n >= 2:
            assert ((s_all > done) & (s_all < done + n)).any(), (name, c, "no peak inside the call")
            assert (s_all == done + n).any(), (name, c, "no peak at the call's last step")
        done += n
