"""GPU tests of the buffers behind the ensemble's host entries (ocn_ens.h EnsBuf, EnsStage2): one buffer shared by
the three sampling entries, the update's and the filter's tables growing and being reused, the recorder's stage
growing in the middle of a recording, and both pinned copies of the launches' member table in flight.

Nothing new is computed here: every result is compared bit for bit (NaN by position) with the reference the entry's
own test uses -- the gather over the members' downloads (tests/ens_assim_ref.py), ens_obs_rule.apply
(tests/ens_obs_ref.py), ens_record_rule.interp over the series, tests/ens_local_ref.py and tests/ens_assim_ref.py
over the downloads -- and what is new is the ORDER of the calls on one ensemble: small, large, small, and one entry
behind another in the same buffer.  Every ensemble has 9 members of class noise after calls [2, 3]; with 9 members a
y / z row is ens_lu_row(9) = 16 doubles, so 300 observations pass a 64 KiB granule.  Tolerance: none.
"""
import numpy as np
import pytest

from tests import ens_assim_ref as A
from tests import ens_local_ref as R
from tests import ens_obs_ref as O
from tests import shapes as S
from tests.test_gpu_ens_assim import _assim_vs_restatement, _points
from tests.test_gpu_ens_local import _update_vs_downloads
from tests.test_gpu_ens_record import _op
from tests.test_gpu_ens_transform import _run
from tests.test_gpu_ensemble import _start

pytestmark = pytest.mark.gpu

OK = 0
ONE, GRID = S.Shape(61, 9), S.Shape(17, 19, (2, 2))
CLASSES = ["noise"] * 9
STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _points_ij(shape, nobs, seed):
    """nobs points anywhere in the shape's basin (rings included), with a repeat."""
    rng = np.random.default_rng(seed)
    ij = np.stack([rng.integers(1, shape.W + 5, nobs), rng.integers(1, shape.H + 5, nobs)], axis=1)
    if nobs > 4:
        ij[nobs - 1] = ij[0]
    return ij


def _sample_vs_downloads(e, name, ij):
    """sample() at the points ij, then the gather over the members' downloads: True where they agree."""
    got = e.sample(name, _points(e, ij))
    blocks = e.members[0].blocks
    want = A.gather({b.k: [m.download(b.k, name) for m in e.members] for b in blocks}, blocks, e.block_of, ij)
    return got.shape == (len(ij), len(e)) and A.bits_equal(got, want)


# ---------------------------------------------------------------- 1. the shared sampling buffer
def test_sampling_entries_share_one_buffer(amd):
    """ocn_ens_sample, ocn_ens_sample_h and ocn_ens_record_sample lay their tables out in ONE buffer, each its own
    way, and grow it when a call needs more.  In one ensemble: sample at 2 points (240 bytes), sample_h of 40 rows
    over two fields (a few KB: grows), sample at 300 points (25 KB: grows), record + step_record(2),
    sample_recorded of 5 observations and sample at the first 2 points again (both in the buffer the 300 points
    left).  Each result against its own entry's reference."""
    from ocean_model_arch_amd import ens_record_rule
    e = _start(amd, ONE, CLASSES)
    try:
        _run(e, [2, 3])
        few, many = _points_ij(ONE, 2, 1), _points_ij(ONE, 300, 2)
        many[:2] = few
        bad = []
        if not _sample_vs_downloads(e, "ssh", few):
            bad.append("sample at 2 points")
        rng = np.random.default_rng(3)
        names = ("ubrtr", "vbrtrp")
        rows = [[(names[(r + t) % 2], int(rng.integers(1, 66)), int(rng.integers(1, 14)), float(rng.uniform(-1, 1)) or 0.5)
                 for t in range(1 + r % 5)] for r in range(40)]
        op = O.ObsOperator.from_rows(rows, np.full((40, 2), 5))
        got = e.sample_h(op)
        if got.shape != (40, 9) or not O.bits_equal(got, O.apply(op, O.downloads(e, names, range(9)), e.members[0].blocks, e.block_of)):
            bad.append("sample_h of 40 rows")
        if not _sample_vs_downloads(e, "ssh", many):
            bad.append("sample at 300 points")
        rop = _op(ONE, 7, 4)
        e.record(rop, every=1, max_records=4)
        e.step_record(2)
        info = e.record_info()
        assert (info["steps"], info["records"]) == (2, 2), info
        series = e.series()
        at = np.array([1.0, 2.0, 1.5, 1.25, 1.75])
        obs_rows = np.array([0, 6, 3, 3, 5])
        got = e.sample_recorded(obs_rows, at)
        rec, wt = ens_record_rule.at_steps(at, 1, 2)
        if got.shape != (5, 9) or not O.bits_equal(got, ens_record_rule.interp(series, obs_rows, rec, wt, None)):
            bad.append("sample_recorded of 5 observations")
        if not _sample_vs_downloads(e, "ssh", few):
            bad.append("sample at the 2 points again")
        e.complete()
        st = e.synchronize()
    finally:
        e.close()
    assert not bad, bad
    assert st == [OK] * 9, st


# ---------------------------------------------------------------- 2. the update's and the filter's tables
@pytest.mark.parametrize("shape", [ONE, GRID], ids=lambda s: s.id)
def test_update_and_filter_tables_grow_and_are_reused(amd, shape):
    """local_update with 2, 300 and 2 observations, then assimilate(device=True) with 2, 300 and 2, on one block and
    on a 2 x 2 grid (the lists are per block).  Both buffers grow in steps of 65536 bytes; with n = 9 a row is 16
    doubles = 128 bytes:
      ocn_ens_local_update   2 nobs 128 (y, z) + the taper on a 256-byte line + 16 bytes per list entry:
                             2 observations 512 + 256 + a few entries, one granule; 300 observations 76800 + ...,
                             two granules;
      ocn_ens_assimilate     the tables (taper, lists, values, variances, offsets, indices, blocks, the pointer
                             table; a few KB at 300), then hx, y, z: 3 nobs 128, the three vectors 3 nobs 8, the
                             count and the accept flags nobs 8: 2 observations one granule; 300 observations
                             115200 + 7200 + 2400 + ..., two granules.
    So the second call of each grows its buffer (and the filter's forgets the first call's results) and the third
    runs in the larger one.  After each call every field of every member on every block is the restatement's over
    the downloads before it; after each assimilate the four returned arrays and assimilate_results()' y and z are
    that call's."""
    names = ("ssh", "ubrtr")
    e = _start(amd, shape, CLASSES)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 9
        taper = R.ringed_taper(10, 3)   # reach 3
        bad, before = [], None
        for t, nobs in enumerate((2, 300, 2)):
            ij = _points_ij(shape, nobs, 10 + t)
            y, z = R.rows(nobs, 9, 20 + t, scale=0.02)
            b, before = _update_vs_downloads(e, y, z, ij, taper, names, None, before)
            bad += [f"local_update {nobs}: {x}" for x in b]
        shapes = []
        for t, nobs in enumerate((2, 300, 2)):
            ij = _points_ij(shape, nobs, 30 + t)
            b, _, got, _ = _assim_vs_restatement(e, "ssh", ij, A.taper_table(3.0), names, seed=40 + t)
            bad += [f"assimilate {nobs}: {x}" for x in b]
            shapes.append((got["hx"].shape, got["innovations"].shape, e.assimilate_results("z")["z"].shape))
        st = e.synchronize()
    finally:
        e.close()
    assert not bad, bad
    assert shapes == [((k, 9), (k,), (k, 9)) for k in (2, 300, 2)], shapes
    assert st == [OK] * 9, st


# ---------------------------------------------------------------- 3. the recorder's stage
def _recorded_states(amd, op, calls, in_launch_last):
    """An ensemble recording `op` over the chunked calls, then one step_record(4) with the in-launch route on if
    asked: (the series, the recorder's info before and after that last call, the members' state fields)."""
    e = _start(amd, ONE, CLASSES)
    try:
        e.set_record_in_launch(False)
        e.record(op, every=1, max_records=40)
        for i, n in enumerate(calls):
            e.step_record(n)
            if i == 0:
                assert e.synchronize() == [OK] * 9
        mid = e.record_info()
        e.set_record_in_launch(in_launch_last)
        e.step_record(4)
        info = e.record_info()
        series = e.series()
        e.complete()
        assert e.synchronize() == [OK] * 9
        fields = O.downloads(e, STATE, range(9))
    finally:
        e.close()
    return series, mid, info, fields


def test_recorder_stage_grows_mid_recording(amd):
    """Chunked recording (OCN_ENS_OPT_RECORD_IN_LAUNCH 0), every = 1, calls [2, 19, 3]: the second call makes 19
    gathers and the stage has room for 16, so it grows between two calls of one recording.  The series is that of a
    second ensemble with the same states whose calls are at most 4 steps long, which never grows its stage; 24
    records over 24 steps.  Then step_record(4) in the launch on both, in the first ensemble on the grown stage:
    in_launch rises by the three records the launch writes itself, and the series still agree."""
    op = _op(ONE, 23, 5)
    got, mid, info, fields = _recorded_states(amd, op, [2, 19, 3], True)
    want, wmid, winfo, wfields = _recorded_states(amd, op, [2, 4, 4, 4, 4, 3, 3], True)
    assert (mid["steps"], mid["records"], mid["in_launch"]) == (24, 24, 0), mid
    assert (wmid["steps"], wmid["records"], wmid["in_launch"]) == (24, 24, 0), wmid
    assert (info["steps"], info["records"], info["in_launch"]) == (28, 28, 3), info
    assert (winfo["steps"], winfo["records"], winfo["in_launch"]) == (28, 28, 3), winfo
    assert got.shape == want.shape == (28, 23, 9)
    differ = [r for r in range(28) if not O.bits_equal(got[r], want[r])]
    assert not differ, f"records {differ} differ between the ensemble whose stage grew and the one whose did not"
    assert not [(nm, i) for nm in STATE for i in range(9) if not O.bits_equal(fields[nm][0][i], wfields[nm][0][i])]


# ---------------------------------------------------------------- 4. both copies of the member table
def test_member_table_copies_back_to_back(amd):
    """Three step(4) calls with no wait in between -- the first fills one pinned copy of the launches' member table,
    the second the other, the third waits for the first's event and fills the first again -- then complete(): the
    members' fields are those of the same ensemble stepped with a synchronize() after every call."""
    def run(wait):
        e = _start(amd, ONE, CLASSES)
        try:
            _run(e, [2, 3])
            batched = []
            for _ in range(3):
                e.step(4)
                batched.append(e.info()["batched"])
                if wait:
                    assert e.synchronize() == [OK] * 9
            e.complete()
            st = e.synchronize()
            return O.downloads(e, STATE, range(9)), batched, st
        finally:
            e.close()
    got, batched, st = run(False)
    want, wbatched, wst = run(True)
    assert st == wst == [OK] * 9, (st, wst)
    assert batched == wbatched == [9, 9, 9], (batched, wbatched)   # (the premise: every call goes through the table)
    assert not [(nm, i) for nm in STATE for i in range(9) if not O.bits_equal(got[nm][0][i], want[nm][0][i])]
