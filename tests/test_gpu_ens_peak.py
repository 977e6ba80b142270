"""GPU tests of the peak map (ocn_ens_peak_*; ens_peak.hip k_ens_peak / k_ens_exceed and sw_kernels.hip
k_march_multi_pk behind OceanEnsemble.peak_begin / peak / peak_stats / peak_exceed).

The reference is the CPU oracle only, stepped one step(tau) at a time with the numpy rule applied after each step
(tests/ens_peak_ref.py; the forcing of forced members from tests/ens_forcing_ref.py).  P and S of every tracked
member are compared bitwise after EVERY call (NaN by position), and after complete() every field of every member
is still the oracle's.  Two routes of the library are never compared with each other.  The runs are
tests/ens_forcing_ref.py RUNS, forced as there or with no storm; tests/test_ens_peak_cpu.py asserts their premises
without a device.  Every run makes a first short call and a synchronize(), then peak_begin, then its calls.
Tolerance: none.
"""
import numpy as np
import pytest

from tests import ens_forcing_ref as R
from tests import ens_peak_ref as K
from tests import ens_stats_ref
from tests import shapes as S
from tests.test_gpu_ens_forcing import _bad
from tests.test_gpu_ensemble import _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE, ERR_BLOWUP = 0, 1, 4, 5


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _same(got, want):
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


def _peaks_bad(e, tracked, what, refs, tag):
    """The tracked members' (P, S) of every block against refs[i] = {(bm, bn): {which: (P, S)}}."""
    bad = []
    for i in tracked:
        for b in e.members[i].blocks:
            for w in what:
                P, Sx = e.peak(i, b.k, w)
                wp, ws = refs[i][(b.bm, b.bn)][w]
                if not _same(P, wp):
                    bad.append(f"{tag} member {i} ({b.bm},{b.bn}) P{w}")
                if not _same(Sx, ws):
                    bad.append(f"{tag} member {i} ({b.bm},{b.bn}) S{w}")
    return bad


def _run(amd, name, forced, field="ssh", what=("max", "min"), calls=None, cap=None, before=None, check_every=1,
         tracked=None, first=K.FIRST, skip_state=(), complete_first=False):
    """One run: the first short call, peak_begin, the calls (P and S against the reference after each), complete()
    and every field of every member against the oracle.  Returns per call (steps updated in a launch, ensemble
    info, launches issued)."""
    from ocean_model_arch_amd import _lib
    shape, params, classes, _, run_calls = R.RUNS[name]
    calls = tuple(calls if calls is not None else (K.CALLS if len(run_calls) == 5 else run_calls))
    tau = S.tau_of(params)
    what = (what,) if isinstance(what, str) else tuple(what)
    e = _start(amd, shape, list(classes), params)
    try:
        if cap is not None:
            e.set_capacity(cap)
        if forced:
            e.set_storms({i: R.run_storm(name, i) for i in R.run_forced(name)}, R.MODEL)
        if before:
            before(e)
        if first:
            e.step(first, tau=tau)
            assert e.synchronize() == [OK] * len(e)
        if complete_first:
            e.complete()
        e.peak_begin(field, what, members=tracked)
        members = list(range(len(e))) if tracked is None else sorted(tracked)
        info = e.peak_info()
        assert (info["active"], info["field"], info["what"], info["tracked"], info["steps"]) == \
            (True, field, tuple(w for w in ("max", "min") if w in what), len(members), 0), info
        refs = {i: K.reference(name, i, field, forced, calls, first) for i in members}
        per_call, bad, done = [], [], 0
        for c, n in enumerate(calls):
            l0, k0 = _lib.launch_count(), e.peak_info()["in_launch"]
            if forced:
                e.step_forced(n, tau, float(done) * tau, check_every=check_every)
            else:
                e.step(n, tau=tau, check_every=check_every)
            launches = _lib.launch_count() - l0
            per_call.append((e.peak_info()["in_launch"] - k0, e.info(), launches, [m.tail_pending for m in e.members]))
            done += n
            assert e.peak_info()["steps"] == done
            bad += _peaks_bad(e, members, what, {i: refs[i][c] for i in members}, f"call {c}")
        e.complete()
        st = e.synchronize()
        bad += [x for x in _bad(e, [K.final_state(name, i, forced, calls, first) for i in range(len(e))])
                if not any(x.startswith(f"member {i} ") for i in skip_state)]
    finally:
        e.close()
    assert not bad, bad[:12]
    return per_call, st, calls


def _assert_in_launch(per_call, calls, members, groups=None, extra=0):
    """Every call of two steps or more ran in the launch: its steps but the last were updated there, every member
    batched, and the launches are the groups' and one k_ens_peak behind them (+ extra: a forced call's k_ens_forcing
    launches).  The 1-step call is chunked and keeps the sequences open."""
    for n, (upd, info, launches, pending) in zip(calls, per_call):
        if n >= 2:
            assert upd == n - 1 and info["batched"] == members, (n, upd, info)
            x = extra(n) if callable(extra) else extra
            assert launches == info["groups"] + 1 + x, (n, launches, info)
            if groups is not None:
                assert info["groups"] == groups, info
        else:   # (chunked; a forced call of two steps or more behind it runs in the launch only on open sequences)
            assert upd == 0, (n, upd, pending)


# ---------------------------------------------------------------- 1. unforced step()
@pytest.mark.parametrize("name,field,what", [("one_tile", "ssh", ("max", "min")), ("one_tile", "ubrtr", "max"),
                                             ("many_tiles", "ssh", ("max", "min")), ("tau03", "ssh", ("max", "min")),
                                             ("one_point", "ssh", ("max", "min"))])
def test_step_in_launch(amd, name, field, what):
    """Known-constant, h_r-read and general members in one call (three groups on one_tile and many_tiles), tau a
    power of two and 0.3, both extremes and the maximum alone, ssh and ubrtr: every call of two steps or more ran in
    the launch."""
    per_call, st, calls = _run(amd, name, False, field, what)
    members = len(R.RUNS[name][2])
    assert st == [OK] * members
    _assert_in_launch(per_call, calls, members, 3 if name in ("one_tile", "many_tiles") else None)
    if name == "many_tiles":
        assert per_call[1][1]["tiles"] == 51, per_call[1][1]


def test_tracked_subset(amd):
    """Members 1 and 3 tracked: the others march in plain launches of the same call."""
    per_call, st, calls = _run(amd, "one_tile", False, tracked=(1, 3))
    assert st == [OK] * 5
    _assert_in_launch(per_call, calls, 5, 3)


# ---------------------------------------------------------------- 2. forced step_forced()
def _frc_extra(n):
    return 1 + (1 if n % 2 == 0 else 0)   # k_ens_forcing ahead of the groups and, after an even count, behind them


@pytest.mark.parametrize("name,groups", [("one_tile", 1), ("many_tiles", 1), ("subset", 3)])
def test_step_forced_in_launch(amd, name, groups):
    per_call, st, calls = _run(amd, name, True)
    members = len(R.RUNS[name][2])
    assert st == [OK] * members
    _assert_in_launch(per_call, calls, members, groups, _frc_extra)


@pytest.mark.parametrize("cap,groups", [(2, 9), (7, 3)])
@pytest.mark.parametrize("forced", [True, False], ids=["forced", "unforced"])
def test_several_groups(amd, cap, groups, forced):
    per_call, st, calls = _run(amd, "groups", forced, cap=cap)
    assert st == [OK] * 9
    _assert_in_launch(per_call, calls, 9, groups, _frc_extra if forced else 0)


# ---------------------------------------------------------------- 3. peak_begin on a closed sequence
def test_begin_on_a_closed_sequence(amd):
    """peak_begin before any step (P starts as the state init and the uploads left), and behind a complete() that
    closed the sequences: whichever route each call takes -- a call's steps but the last updated in the launch, or
    none -- the bits hold.  An unforced call needs no open sequence for its launch, so the call behind the first
    one runs there.  A forced call runs in the launch only on open sequences of its forced members
    (ocn_ens_step_forced's own condition), and its chunked route, which rewrites the forcing under a closed
    sequence through the upload bookkeeping, does not open one: both forced calls are chunked."""
    per_call, st, calls = _run(amd, "one_tile", False, calls=(3, 4), first=0)
    assert st == [OK] * 5
    assert per_call[0][0] in (0, 2) and per_call[1][0] in (0, 3), per_call
    per_call, st, calls = _run(amd, "one_tile", False, calls=(3, 4), complete_first=True)
    assert st == [OK] * 5
    assert per_call[0][0] in (0, 2) and per_call[1][0] == 3, per_call
    per_call, st, calls = _run(amd, "one_tile", True, calls=(3, 4), complete_first=True)
    assert st == [OK] * 5
    assert [c[0] for c in per_call] == [0, 0], per_call


# ---------------------------------------------------------------- 4. chunked routes
def test_option_off_is_chunked(amd):
    per_call, st, calls = _run(amd, "one_tile", False, before=lambda e: e.set_peak_in_launch(False))
    assert [c[0] for c in per_call] == [0] * len(calls)
    per_call, st, calls = _run(amd, "one_tile", True, before=lambda e: e.set_peak_in_launch(False))
    assert [c[0] for c in per_call] == [0] * len(calls)


@pytest.mark.parametrize("name,forced", [("grid", False), ("grid", True), ("tracer", False)])
def test_block_grid_and_tracers(amd, name, forced):
    per_call, st, calls = _run(amd, name, forced)
    assert [c[0] for c in per_call] == [0] * len(calls)


def test_check_every_two(amd):
    per_call, st, calls = _run(amd, "subset", True, check_every=2)
    assert [c[0] for c in per_call] == [0] * len(calls)


# ---------------------------------------------------------------- 5. single members
def test_blowup_stays_with_its_member(amd):
    """Member 1 under vmax = 1e9: OCN_ERR_BLOWUP for it alone; its P / S follow the rule on the oracle's run (Inf
    and NaN included), the other members' peaks and states are their own runs'."""
    name, calls = "one_tile", (2, 6)
    shape, params, classes, _, _ = R.RUNS[name]
    wild = R.storm_for(shape, 1, vmax=1.0e9)
    times = R.call_times(calls, 1.0)
    ser = K.unchecked_series(shape, classes[1], 1000, wild, R.MODEL, times, params)   # (the oracle's step raises at the blow-up)
    from ocean_model_arch_amd import ens_peak_rule as PR
    box = K.interiors(shape)[(1, 1)]
    e = _start(amd, shape, list(classes), params)
    try:
        e.set_storms({i: (wild if i == 1 else R.run_storm(name, i)) for i in range(5)}, R.MODEL)
        e.step(K.FIRST)
        assert e.synchronize() == [OK] * 5
        e.peak_begin("ssh", ("max", "min"))
        done = 0
        for n in calls:
            e.step_forced(n, 1.0, float(done))
            done += n
        assert e.peak_info()["in_launch"] == sum(calls) - len(calls)
        want = {"max": PR.begin(ser[K.FIRST - 1]["ssh"], box), "min": PR.begin(ser[K.FIRST - 1]["ssh"], box)}
        for k in range(1, done + 1):
            PR.update(*want["max"], ser[K.FIRST + k - 1]["ssh"], k, box)
            PR.update(*want["min"], ser[K.FIRST + k - 1]["ssh"], k, box, minimum=True)
        others = [i for i in range(5) if i != 1]
        bad = _peaks_bad(e, [1], ("max", "min"), {1: {(1, 1): want}}, "wild")
        bad += _peaks_bad(e, others, ("max", "min"), {i: K.reference(name, i, "ssh", True, calls)[-1] for i in others}, "others")
        e.complete()
        st = e.synchronize()
        bad += [x for x in _bad(e, [K.final_state(name, i, True, calls) for i in range(5)]) if not x.startswith("member 1 ")]
    finally:
        e.close()
    assert st == [OK, ERR_BLOWUP, OK, OK, OK], st
    assert not np.isfinite(want["max"][0]).all() or np.abs(want["max"][0]).max() > 1e4
    assert not bad, bad[:12]


def test_still_water_and_second_begin(amd):
    """Member 0's state is +0.0 everywhere: S stays 0.  A second peak_begin starts over: P is the state then, S and
    the step count are 0, and the peaks follow from there."""
    shape = R.RUNS["one_tile"][0]
    steps = sum(K.CALLS)
    want, top = K.still_reference(shape, "ssh", steps)
    e = _start(amd, shape, ["plain", "noise"])
    try:
        zero = np.zeros(e.members[0].blocks[0].shape, order="F")
        for nm in R.STATE:
            e.members[0].upload(0, nm, zero)
        e.step(K.FIRST)
        assert e.synchronize() == [OK, OK]
        e.peak_begin("ssh")
        for n in K.CALLS:
            e.step(n)
        bad = _peaks_bad(e, [0], ("max", "min"), {0: {(1, 1): want}}, "still")
        P, Sx = e.peak(0, 0, "max")
        assert not Sx.any() and not P.any()
        # a second begin: member 1 from where it is now
        before = e.peak(1, 0, "max")
        e.peak_begin("ssh", "max")
        info = e.peak_info()
        assert (info["steps"], info["in_launch"], info["what"]) == (0, 0, ("max",)), info
        P, Sx = e.peak(1, 0, "max")
        now = e.members[1].download(0, "ssh")
        box = K.interiors(shape)[(1, 1)]
        from ocean_model_arch_amd import ens_peak_rule as PR
        wp, ws = PR.begin(now, box)
        assert _same(P, wp) and _same(Sx, ws) and before[1].any()
        with pytest.raises(amd.OcnError) as ei:
            e.peak(1, 0, "min")
        assert ei.value.code == ERR_ARG
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 6. products
@pytest.mark.parametrize("members", [9, 33])
def test_products(amd, members):
    """peak_stats (mean, max, spread) against tests/ens_stats_ref.py on the downloaded peaks' reference, and
    peak_exceed against numpy, with a threshold that some peaks equal exactly and a member whose peak is NaN."""
    from ocean_model_arch_amd import ens_peak_rule as PR
    shape, steps = S.Shape(61, 9), 5
    box = K.interiors(shape)[(1, 1)]
    inner = (slice(box[0], box[1] + 1), slice(box[2], box[3] + 1))

    def ref_p(i):   # the reference's Pmax of member i: the oracle's series under the rule
        ser = R.forced_reference(shape, "noise", 1000 * i, None, None, R.call_times((steps,), 1.0), None, 0, K.FIRST)["series"]
        P, Sx = PR.begin(ser[K.FIRST - 1][(1, 1)]["ssh"], box)
        for k in range(1, steps + 1):
            PR.update(P, Sx, ser[K.FIRST + k - 1][(1, 1)]["ssh"], k, box)
        return P
    want_p = [ref_p(i) for i in range(members)]
    want_p[2] = np.zeros_like(want_p[0])
    want_p[2][inner] = np.nan                        # (member 2: NaN everywhere when the peak begins, and it stays)
    e = _start(amd, shape, ["noise"] * members)
    try:
        e.step(K.FIRST)
        assert e.synchronize() == [OK] * members
        for nm in ("ssh", "sshp"):
            e.members[2].upload(0, nm, np.full(want_p[0].shape, np.nan, order="F"))
        e.peak_begin("ssh", ("max", "min"))
        e.step(steps)
        bad = [i for i in range(members) if not _same(e.peak(i, 0, "max")[0], want_p[i])]
        assert not bad, bad
        use = [i for i in range(members) if i != 2]
        got = e.peak_stats(("mean", "max", "spread"), "max", members=use)
        want = ens_stats_ref.stats([want_p[i] for i in use], ("mean", "max", "spread"))
        for nm in ("mean", "max", "spread"):
            assert _same(got[nm], np.asfortranarray(want[nm])), nm
        thr = float(want_p[0][30, 5])                 # (a peak of member 0 equals it exactly: not counted)
        frac = e.peak_exceed(thr)
        assert _same(frac, PR.exceed(want_p, thr)) and frac.max() > 0.0 and frac[30, 5] < 1.0
        assert _same(e.peak_exceed(thr, members=use), PR.exceed([want_p[i] for i in use], thr))
    finally:
        e.close()


# ---------------------------------------------------------------- 7. errors
def test_errors(amd):
    from ocean_model_arch_amd import _lib, ens_obs_rule
    import ctypes as C
    shape = S.Shape(61, 9)
    e = _start(amd, shape, ["noise"] * 3)
    try:
        L = amd.lib()
        for call in (lambda: e.peak_end(), lambda: e.peak_info(), lambda: e.peak(0), lambda: e.peak_stats(),
                     lambda: e.peak_exceed(0.0)):
            with pytest.raises(amd.OcnError) as ei:
                call()
            assert ei.value.code == ERR_STATE
        assert L.ocn_ens_peak_begin(e.ens, None, _lib.FIELD_ID["hhq"], 1) == ERR_ARG
        assert L.ocn_ens_peak_begin(e.ens, None, _lib.FIELD_ID["ssh"], 4) == ERR_ARG
        assert L.ocn_ens_peak_begin(e.ens, None, _lib.FIELD_ID["ssh"], 0) == ERR_ARG
        assert L.ocn_ens_peak_begin(e.ens, (C.c_uint8 * 3)(), _lib.FIELD_ID["ssh"], 1) == ERR_ARG
        with pytest.raises(amd.OcnError) as ei:
            e.peak_info()                              # (nothing was begun)
        assert ei.value.code == ERR_STATE
        with pytest.raises(ValueError):
            e.peak_begin("hhq")
        with pytest.raises(TypeError):
            e.peak_begin("ssh", what=(1,))
        e.step(2)
        e.peak_begin("ssh", "max", members=(0, 1))
        l0, pending = _lib.launch_count(), [m.tail_pending for m in e.members]
        for call in (lambda: e.peak_stats(members=(1, 2)), lambda: e.peak_exceed(0.0, members=(2,)), lambda: e.peak(2),
                     lambda: e.peak_stats(which="min")):
            with pytest.raises(amd.OcnError) as ei:
                call()
            assert ei.value.code == ERR_ARG
        buf = np.zeros(e.members[0].blocks[0].shape, order="F")
        assert L.ocn_ens_peak_download(e.ens, 0, 1, 1, buf.ctypes.data_as(C.c_void_p), None) == ERR_ARG
        assert L.ocn_ens_peak_download(e.ens, 0, 0, 1, None, None) == ERR_ARG
        assert L.ocn_ens_peak_exceed(e.ens, 0, None, C.c_double(float("nan")), buf.ctypes.data_as(C.c_void_p)) == ERR_ARG
        assert _lib.launch_count() == l0 and [m.tail_pending for m in e.members] == pending
        e.record(ens_obs_rule.points("ssh", [(7, 4)]), every=1, max_records=4)
        with pytest.raises(amd.OcnError) as ei:
            e.step_record(2)
        assert ei.value.code == ERR_STATE
        e.record_end()
        e.peak_end()
        with pytest.raises(amd.OcnError) as ei:
            e.peak_end()
        assert ei.value.code == ERR_STATE
        e.step(3)                                      # (no peak: the plain path)
        assert e.synchronize() == [OK] * 3
    finally:
        e.close()
