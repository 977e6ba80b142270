"""CPU tests of the station recorder's pure parts (include/ocn_sw.h ocn_ens_record_*): the schedule
ocn_ens_record_due against its Python restatement (ocean_model_arch_amd/ens_record_rule.py), its argument
errors, the entries on a null ensemble, and the exceptions the Python methods raise before any device call.
No device.
"""
import ctypes as C

import numpy as np
import pytest

from ocean_model_arch_amd import _lib, ens_obs_rule, ens_record_rule
from ocean_model_arch_amd.ensemble import OceanEnsemble


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _due(lib, counted, nsteps, every, cap):
    steps = (C.c_int32 * max(cap, 1))(*([-7] * max(cap, 1)))
    n = C.c_int32(-1)
    rc = lib.ocn_ens_record_due(counted, nsteps, every, steps if cap else None, cap, C.byref(n))
    return rc, n.value, list(steps)


def test_due_is_the_rule(lib):
    """counted 0..7, nsteps 0..9, every 1..5, with room for every due step, for two of them and for none:
    the count is always the whole call's, the array holds its first min(cap, count) steps and nothing else is
    written."""
    none = 0
    for counted in range(8):
        for nsteps in range(10):
            for every in range(1, 6):
                want = ens_record_rule.due(counted, nsteps, every)
                assert want == [s for s in range(1, nsteps + 1) if (counted + s) % every == 0]
                none += not want
                for cap in (16, 2, 0):
                    rc, n, steps = _due(lib, counted, nsteps, every, cap)
                    assert rc == _lib.OCN_OK and n == len(want), (counted, nsteps, every, cap)
                    k = min(cap, len(want))
                    assert steps[:k] == want[:k] and all(s == -7 for s in steps[k:]), (counted, nsteps, every, cap)
    assert none > 0   # (calls with no due step are in the sweep)
    assert ens_record_rule.due(2 ** 40 + 1, 5, 3) == [s for s in range(1, 6) if (2 ** 40 + 1 + s) % 3 == 0]
    rc, n, steps = _due(lib, 2 ** 40 + 1, 5, 3, 4)
    assert rc == _lib.OCN_OK and steps[:n] == ens_record_rule.due(2 ** 40 + 1, 5, 3)
    assert lib.ocn_ens_record_due(0, 4, 2, None, 0, None) == _lib.OCN_OK   # (the count is optional)


def test_due_argument_errors(lib):
    n = C.c_int32(0)
    steps = (C.c_int32 * 4)()
    for counted, nsteps, every, arr, cap in [(-1, 3, 1, steps, 4), (0, -1, 1, steps, 4), (0, 3, 0, steps, 4), (0, 3, -2, steps, 4),
                                             (0, 3, 1, steps, -1), (0, 3, 1, None, 4)]:
        assert lib.ocn_ens_record_due(counted, nsteps, every, arr, cap, C.byref(n)) == _lib.OCN_ERR_ARG
        assert b"ens_record_due" in lib.ocn_last_error()
    for bad in [(-1, 3, 1), (0, -1, 1), (0, 3, 0)]:
        with pytest.raises(ValueError):
            ens_record_rule.due(*bad)
    for bad in [(0, 4), (4, 0), (-1, 4)]:
        with pytest.raises(ValueError):
            ens_record_rule.check(*bad)


def test_null_ensemble(lib):
    one = (C.c_int32 * 2)(0, 1)
    w = (C.c_double * 1)(1.0)
    info = _lib.OcnEnsRecordInfo()
    assert lib.ocn_ens_record_begin(None, None, 1, one, one, one, one, w, 1, 1) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_step_record(None, 1.0, 2, 1) == _lib.OCN_ERR_ARG
    assert b"null ensemble" in lib.ocn_last_error()
    assert lib.ocn_ens_record_info(None, C.byref(info)) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_record_download(None, 0, 1, w) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_record_end(None) == _lib.OCN_ERR_ARG
    assert lib.ocn_ens_set_option(None, _lib.ENS_OPT_RECORD_IN_LAUNCH, 0) == _lib.OCN_ERR_ARG


class _NoDevice(OceanEnsemble):
    """The methods' own checks, which come before any call into the library: an ensemble of three members
    without a handle (a call that got through would fail on it)."""

    def __init__(self):   # noqa: no context is created
        self.ens = None
        self.members = [None] * 3
        self._recording = False


def test_python_argument_checks():
    e = _NoDevice()
    op = ens_obs_rule.points("ssh", [[3, 3], [4, 4]])
    for bad in ("ssh", None, [[("ssh", 3, 3, 1.0)]]):
        with pytest.raises(TypeError):
            e.record(bad)
    for kw in (dict(every=1.0), dict(every="2"), dict(every=True), dict(max_records=3.5), dict(max_records=None)):
        with pytest.raises(TypeError):
            e.record(op, **kw)
    for kw in (dict(every=0), dict(every=-3), dict(max_records=0), dict(max_records=2 ** 31 - 1),
               dict(max_records=(1 << 30) // (2 * 3 * 8) + 1)):
        with pytest.raises(ValueError):
            e.record(op, **kw)
    with pytest.raises(IndexError):
        e.record(op, members=[3])
    for bad in (1.0, "2", None, True):
        with pytest.raises(TypeError):
            e.step_record(bad)
    with pytest.raises(ValueError):
        e.step_record(-1)
    for bad in (dict(first=0.0), dict(count=1.5), dict(first="0")):
        with pytest.raises(TypeError):
            e.series(**bad)
    assert ens_record_rule.MAX_SERIES_BYTES == 1 << 30 and np.dtype(np.float64).itemsize == 8
