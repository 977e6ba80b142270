"""GPU tests of the one entry that steps with everything that is active (ocn_ens_run; sw_kernels.hip
k_march_multi_all behind OceanEnsemble.run): the moving-storm forcing, the station recorder and the peak map in one
marching launch, or chunked per step.

The reference is the CPU oracle only, stepped one step(tau) at a time (tests/ens_run_ref.py: the forcing of a
forced member set from the numpy restatement before each step, the operator's numpy restatement applied after
every due step, the numpy peak rule after every step).  After EVERY call the series so far and P / S of every
tracked member are compared bitwise (NaN by position); after complete() every field of every member.  Two routes of
the library are never compared with each other.  tests/test_ens_run_cpu.py asserts the runs' premises without a
device.  Every run attaches its storms (a forced member runs the general bodies from its first step on, which the
forcing launch needs), makes a first short call and a synchronize(), then record() and peak_begin() as the case
needs, then its calls through run().  Tolerance: none.
"""
import pytest

from tests import ens_forcing_ref as R
from tests import ens_run_ref as A
from tests import shapes as S
from tests.test_gpu_ens_forcing import _bad
from tests.test_gpu_ensemble import _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE, ERR_BLOWUP = 0, 1, 4, 5
WHAT = ("max", "min")


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _peaks_bad(e, tracked, refs, tag):
    """The tracked members' (P, S) of every block against refs[i] = {(bm, bn): {which: (P, S)}}."""
    bad = []
    for i in tracked:
        for b in e.members[i].blocks:
            for w in WHAT:
                P, Sx = e.peak(i, b.k, w)
                wp, ws = refs[i][(b.bm, b.bn)][w]
                if not A.same(P, wp):
                    bad.append(f"{tag} member {i} ({b.bm},{b.bn}) P{w}")
                if not A.same(Sx, ws):
                    bad.append(f"{tag} member {i} ({b.bm},{b.bn}) S{w}")
    return bad


def _run(amd, name, kind="five", every=1, storms="all", recorded=None, tracked=None, record=True, peak=True, calls=None,
         cap=None, before=None, check_every=1, complete_first=False):
    """One run: the storms, the first short call, record() and peak_begin(), the calls through run() (the series so
    far and the peaks against the reference after each), complete() and every field of every member against the
    oracle.  storms: "all", a tuple of members, or None (unforced: run(t0=None)).  Returns per call a dict: n, the
    launches issued, the ensemble info, the records / peak steps a launch did itself, the forcing's route, the due
    steps."""
    from ocean_model_arch_amd import _lib
    shape, params, classes, _, run_calls = R.RUNS[name]
    M = len(classes)
    calls = tuple(calls if calls is not None else (A.CALLS if len(run_calls) == 5 else run_calls))
    tau = S.tau_of(params)
    everyone = tuple(range(M))
    forced = () if storms is None else everyone if storms == "all" else tuple(sorted(storms))
    recorded = everyone if recorded is None else tuple(sorted(recorded))
    tracked = everyone if tracked is None else tuple(sorted(tracked))
    at, per_call_due = A.due(calls, every)
    e = _start(amd, shape, list(classes), params)
    try:
        if cap is not None:
            e.set_capacity(cap)
        if forced:
            e.set_storms({i: R.run_storm(name, i) for i in forced}, R.MODEL)
        if before:
            before(e)
        e.step(A.FIRST, tau=tau)
        assert e.synchronize() == [OK] * M
        if complete_first:
            e.complete()
        if record:
            e.record(A.operator(name, kind), every=every, max_records=max(len(at), 1), members=recorded)
            want = A.records(name, kind, recorded, forced, calls, every)
        if peak:
            e.peak_begin("ssh", WHAT, members=tracked)
            refs = {i: A.peaks(name, i, i in forced, calls) for i in tracked}
        out, bad, done, taken = [], [], 0, 0
        for c, n in enumerate(calls):
            l0 = _lib.launch_count()
            r0 = e.record_info()["in_launch"] if record else 0
            k0 = e.peak_info()["in_launch"] if peak else 0
            e.run(n, tau=tau, t0=float(done) * tau if forced else None, check_every=check_every)
            launches = _lib.launch_count() - l0
            out.append(dict(n=n, launches=launches, info=e.info(), due=per_call_due[c],
                            rec=(e.record_info()["in_launch"] - r0) if record else 0,
                            pk=(e.peak_info()["in_launch"] - k0) if peak else 0,
                            frc=e.forcing_info()["in_launch"] if forced else False))
            done += n
            taken += len(per_call_due[c])
            if record:
                ri = e.record_info()
                assert (ri["steps"], ri["records"]) == (done, taken), ri
                got = e.series()
                if not (got.shape == want[:taken].shape and A.same(got, want[:taken])):
                    differ = [r for r in range(min(taken, len(got))) if not A.same(got[r], want[r])]
                    bad.append(f"call {c}: records {differ} of {taken} differ from the oracle")
            if peak:
                assert e.peak_info()["steps"] == done
                bad += _peaks_bad(e, tracked, {i: refs[i][c] for i in tracked}, f"call {c}")
        e.complete()
        st = e.synchronize()
        bad += _bad(e, [A.final_state(name, i, i in forced, calls) for i in range(M)])
    finally:
        e.close()
    assert not bad, bad[:12]
    return out, st


def _frc_writes(n):
    return 1 + (1 if n % 2 == 0 else 0)   # k_ens_forcing ahead of the groups and, after an even count, behind them


def _assert_in_launch(out, members, forced=True, peak=True, groups=None):
    """Every call of two steps or more ran in the launch: the records due before its last step were written there,
    the peak's steps but the last updated there, the forcing formed there, every member batched; the launches are
    the groups', the forcing's writes, one k_ens_peak and one gather exactly when a record is due at the last step."""
    for c in out:
        n, inside = c["n"], [s for s in c["due"] if s < c["n"]]
        if n >= 2:
            assert c["rec"] == len(inside), c
            assert c["pk"] == (n - 1 if peak else 0), c
            assert c["frc"] == bool(forced), c
            assert c["info"]["batched"] == members, c
            tail = 1 if c["due"] and c["due"][-1] == n else 0
            assert c["launches"] == c["info"]["groups"] + (_frc_writes(n) if forced else 0) + (1 if peak else 0) + tail, c
            if groups is not None:
                assert c["info"]["groups"] == groups, c
        else:
            assert c["rec"] == 0 and c["pk"] == 0 and not c["frc"], c


def _assert_chunked(out):
    for c in out:
        assert c["rec"] == 0 and c["pk"] == 0 and not c["frc"], c


# ---------------------------------------------------------------- 1. all three in the launch
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("name,kind", [("one_tile", "one"), ("one_tile", "five"), ("one_tile", "wrap"),
                                       ("many_tiles", "one"), ("many_tiles", "five")])
def test_forced_recorded_peak(amd, name, kind, every):
    """Forced, recorded and tracked, all members, calls (2, 5, 4, 1, 6): one row, a 5-term row over three fields,
    and on 61 x 9 more rows than one tile's 256 threads; every 1 and 3 (records inside launches, at a call's last
    step, in the 1-step call, and a call with none)."""
    out, st = _run(amd, name, kind, every)
    members = A.members_of(name)
    assert st == [OK] * members
    _assert_in_launch(out, members, groups=1)
    if name == "many_tiles":
        assert out[1]["info"]["tiles"] == 51, out[1]


# ---------------------------------------------------------------- 2. two of the three
@pytest.mark.parametrize("name,kind", [("one_tile", "five"), ("tau03", "wrap")])
def test_recorded_peak_unforced(amd, name, kind):
    """The combination that is an error through step_record: known-constant, h_r-read and general members in one
    call (three groups), tau = 1 and tau = 0.3."""
    out, st = _run(amd, name, kind, storms=None)
    members = A.members_of(name)
    assert st == [OK] * members
    _assert_in_launch(out, members, forced=False, groups=3)


@pytest.mark.parametrize("every", [1, 3])
def test_forced_recorded_no_peak(amd, every):
    out, st = _run(amd, "one_tile", "five", every, peak=False)
    assert st == [OK] * 5
    _assert_in_launch(out, 5, peak=False, groups=1)


# ---------------------------------------------------------------- 3. three member sets, several groups
@pytest.mark.parametrize("cap", [2, 7])
def test_three_member_sets(amd, cap):
    """Nine members, the recorder on {1, 2, 3, 4}, the peak on {2, 4, 5, 8}, storms on {0, 1, 2, 6}, under
    capacities 2 and 7: groups that record and force and / or track, and groups with no recorded member, which
    take the kernels they took before.  Only results are asserted (and that the launches did the work)."""
    out, st = _run(amd, "groups", "five", storms=A.GROUPS_FORCED, recorded=A.GROUPS_RECORDED, tracked=A.GROUPS_TRACKED,
                   cap=cap)
    assert st == [OK] * 9
    _assert_in_launch(out, 9)


# ---------------------------------------------------------------- 4. the chunked routes
@pytest.mark.parametrize("off", ["run", "record", "peak", "forcing"])
def test_option_off_is_chunked(amd, off):
    before = {"run": lambda e: e.set_run_in_launch(False), "record": lambda e: e.set_record_in_launch(False),
              "peak": lambda e: e.set_peak_in_launch(False), "forcing": lambda e: e.set_forcing_in_launch(False)}[off]
    out, st = _run(amd, "one_tile", "five", 3, before=before)
    assert st == [OK] * 5
    _assert_chunked(out)


@pytest.mark.parametrize("name", ["grid", "tracer"])
def test_block_grid_and_tracers(amd, name):
    out, st = _run(amd, name, "five")
    assert st == [OK] * A.members_of(name)
    _assert_chunked(out)


def test_check_every_two(amd):
    out, st = _run(amd, "one_tile", "five", 3, check_every=2)
    assert st == [OK] * 5
    _assert_chunked(out)


def test_forced_on_closed_sequences(amd):
    """Behind a complete() the forced members' sequences are closed: a forced call runs in the launch only on open
    ones (ocn_ens_step_forced's own condition), and its chunked route does not open one."""
    out, st = _run(amd, "one_tile", "five", calls=(3, 4), complete_first=True)
    assert st == [OK] * 5
    _assert_chunked(out)


# ---------------------------------------------------------------- 5. delegation
def test_nothing_active_is_step(amd):
    out, st = _run(amd, "one_tile", storms=None, record=False, peak=False)
    assert st == [OK] * 5
    for c in out:   # (tests/test_gpu_ensemble.py: one launch per group, nothing else)
        if c["n"] >= 2:
            assert c["info"]["batched"] == 5 and c["info"]["groups"] == 3 and c["launches"] == 3, c
        else:
            assert c["info"]["batched"] == 0, c


def test_recorder_alone_is_step_record(amd):
    out, st = _run(amd, "one_tile", "wrap", storms=None, peak=False)
    assert st == [OK] * 5
    for c in out:   # (tests/test_gpu_ens_record.py: the groups and one gather behind them)
        if c["n"] >= 2:
            assert c["rec"] == c["n"] - 1 and c["info"]["batched"] == 5 and c["launches"] == c["info"]["groups"] + 1, c
        else:
            assert c["rec"] == 0, c


def test_forced_with_a_peak_alone_is_step_forced(amd):
    out, st = _run(amd, "one_tile", record=False)
    assert st == [OK] * 5
    for c in out:   # (tests/test_gpu_ens_peak.py: the groups, k_ens_peak behind them, the forcing's writes)
        if c["n"] >= 2:
            assert c["pk"] == c["n"] - 1 and c["frc"] and c["info"]["batched"] == 5, c
            assert c["launches"] == c["info"]["groups"] + 1 + _frc_writes(c["n"]), c
        else:
            assert c["pk"] == 0, c


# ---------------------------------------------------------------- 6. single members, the 1 x 1 block
def test_blowup_stays_with_its_member(amd):
    """Member 1 under vmax = 1e9: OCN_ERR_BLOWUP for it alone; the other members' columns, peaks and fields are
    still the oracle's."""
    name, calls = "one_tile", (2, 6)
    shape, params, classes, _, _ = R.RUNS[name]
    others = [0, 2, 3, 4]
    e = _start(amd, shape, list(classes), params)
    try:
        e.set_storms({i: (R.storm_for(shape, 1, vmax=1.0e9) if i == 1 else R.run_storm(name, i)) for i in range(5)}, R.MODEL)
        e.step(A.FIRST)
        assert e.synchronize() == [OK] * 5
        e.record(A.operator(name, "five"), every=1, max_records=sum(calls))
        e.peak_begin("ssh", WHAT)
        done = 0
        for n in calls:
            e.run(n, tau=1.0, t0=float(done))
            done += n
        assert e.peak_info()["in_launch"] == sum(calls) - len(calls) and e.record_info()["in_launch"] == sum(calls) - len(calls)
        got = e.series()
        want = A.records(name, "five", tuple(range(5)), tuple(range(5)), calls, 1)
        bad = [f"column {i}" for i in others if not A.same(got[:, :, i], want[:, :, i])]
        bad += _peaks_bad(e, others, {i: A.peaks(name, i, True, calls)[-1] for i in others}, "others")
        e.complete()
        st = e.synchronize()
        bad += [x for x in _bad(e, [A.final_state(name, i, True, calls) for i in range(5)]) if not x.startswith("member 1 ")]
    finally:
        e.close()
    assert st == [OK, ERR_BLOWUP, OK, OK, OK], st
    assert got.shape == want.shape and not bad, bad[:12]


def test_one_point_block(amd):
    """The 1 x 1 block: all three, calls (2, 3)."""
    out, st = _run(amd, "one_point", "five")
    assert st == [OK, OK]


# ---------------------------------------------------------------- 7. errors
def test_errors(amd):
    from ocean_model_arch_amd import _lib
    name = "one_tile"
    shape, params, classes, _, _ = R.RUNS[name]
    e = _start(amd, shape, list(classes), params)
    try:
        e.step(A.FIRST)
        assert e.synchronize() == [OK] * 5
        e.record(A.operator(name, "five"), every=1, max_records=3)
        e.peak_begin("ssh", "max")

        def untouched(call, code):
            l0, pending = _lib.launch_count(), [m.tail_pending for m in e.members]
            ri, pi = e.record_info(), e.peak_info()
            with pytest.raises(amd.OcnError) as ei:
                call()
            assert ei.value.code == code, ei.value
            assert _lib.launch_count() == l0 and [m.tail_pending for m in e.members] == pending
            assert e.record_info() == ri and e.peak_info() == pi

        untouched(lambda: e.run(2, t0=0.0), ERR_STATE)       # forced without storms
        untouched(lambda: e.run(4), ERR_ARG)                  # four due records, room for three
        untouched(lambda: e.step_record(2), ERR_STATE)        # (still: a peak is active)
        e.run(3)
        assert e.record_info()["records"] == 3 and e.peak_info()["steps"] == 3
        untouched(lambda: e.run(1), ERR_ARG)
        L, l0 = amd.lib(), _lib.launch_count()
        assert L.ocn_ens_run(e.ens, 1.0, -1, 1, 0, 0.0) == ERR_ARG
        assert L.ocn_ens_run(e.ens, float("nan"), 2, 1, 0, 0.0) == ERR_ARG
        assert L.ocn_ens_run(e.ens, 1.0, 2, 1, 1, float("inf")) == ERR_ARG
        assert _lib.launch_count() == l0 and e.peak_info()["steps"] == 3
        e.run(0)
        assert e.synchronize() == [OK] * 5
    finally:
        e.close()
