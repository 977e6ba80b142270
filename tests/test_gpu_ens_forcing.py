"""GPU tests of the moving-storm forcing (ocn_ens_forcing_*, ocn_ens_step_forced; ens_forcing.hip k_ens_forcing and
sw_kernels.hip k_march_multi_frc behind OceanEnsemble.set_storms / forcing / step_forced).

The reference is the CPU oracle only: tests/shapes.py oracle_model with tests/test_gpu_ensemble.py's member_uploads,
stepped one om.step(tau) at a time with RHSx / RHSy set from the numpy restatement (ens_forcing_rule.rhs; exp
through math.exp) before each step -- tests/ens_forcing_ref.py.  Every field of every member is compared bitwise
after complete() (NaN by position).  Two paths of the library are never compared with each other.  The runs
(shape, classes, forced members, calls) are tests/ens_forcing_ref.py RUNS; tests/test_ens_forcing_cpu.py asserts
their premises -- the forcing is nonzero, changes from step to step, and changes the oracle's run -- without a
device.  Every run makes the usual first short call -- a plain step(FIRST) with the storms attached, which opens the
members' sequences -- and a synchronize() first, as tests/test_gpu_ensemble.py does: a forcing launch goes on with
an open sequence.  The in-launch route and the chunked route are never compared with each other.  Tolerance: none.
"""
import numpy as np
import pytest

from tests import ens_forcing_ref as R
from tests import shapes as S
from tests.test_gpu_ensemble import _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE, ERR_BLOWUP = 0, 1, 4, 5


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _bad(e, refs):
    """Every field of every member against its reference ({(bm, bn): {field: array}}, other keys skipped):
    ["member i (bm,bn):field", ...]."""
    bad = []
    for i, (m, ref) in enumerate(zip(e.members, refs)):
        ref = {k: v for k, v in ref.items() if isinstance(k, tuple)}
        get = S.model_getter([m])
        assert get.blocks == set(ref)
        bad += [f"member {i} {x}" for x in S.mismatches(ref, get)]
    return bad


def _open(amd, name, cap=None):
    """The run's ensemble with its storms attached (not yet stepped)."""
    shape, params, classes, _, _ = R.RUNS[name]
    e = _start(amd, shape, list(classes), params)
    if cap is not None:
        e.set_capacity(cap)
    e.set_storms({i: R.run_storm(name, i) for i in R.run_forced(name)}, R.MODEL)
    return e


def _forced_calls(e, name, calls, check_every=1):
    """The first short call (a plain step(FIRST)) and a synchronize(), then step_forced call by call, the c-th with
    t0 = (forced steps before it) * tau.  Per call: (in_launch, ensemble info, launches issued)."""
    from ocean_model_arch_amd import _lib
    tau = S.tau_of(R.RUNS[name][1])
    e.step(R.FIRST, tau=tau)
    assert e.synchronize() == [OK] * len(e)
    done, out = 0, []
    for n in calls:
        l0 = _lib.launch_count()
        e.step_forced(n, tau, float(done) * tau, check_every=check_every)
        out.append((e.forcing_info()["in_launch"], e.info(), _lib.launch_count() - l0))
        done += n
    return out


def _run(amd, name, cap=None, check_every=1, before=None):
    """One run of RUNS: the calls, complete(), every field of every member against the oracle.  Returns
    (per call: in_launch, ensemble info, launches; the members' pair flags)."""
    calls = R.RUNS[name][4]
    e = _open(amd, name, cap)
    try:
        if before:
            before(e)
        per_call = _forced_calls(e, name, calls, check_every)
        info = e.forcing_info()
        pairs = [m.pair_active for m in e.members]
        e.complete()
        st = e.synchronize()
        bad = _bad(e, [R.run_reference(name, i) for i in range(len(e))])
    finally:
        e.close()
    assert st == [OK] * len(R.RUNS[name][2]) and not bad, (st, bad)
    assert info["attached"] == len(R.run_forced(name)) and info["steps"] == sum(calls), info
    return per_call, pairs


def _assert_in_launch(name, per_call, forcing_groups=None):
    """Every call of at least two steps ran in the launch: every member batched, and the launches are the groups',
    one k_ens_forcing ahead of them (the forcing of t0) and, after an even number of steps, one behind them (the
    last step's forcing home from the second buffers).  A 1-step call is chunked: it keeps the sequences open."""
    calls, members = R.RUNS[name][4], len(R.RUNS[name][2])
    for n, (in_launch, info, launches) in zip(calls, per_call):
        assert in_launch == (n >= 2), (n, in_launch)
        if n >= 2:
            assert info["batched"] == members and launches == info["groups"] + 1 + (1 if n % 2 == 0 else 0), (n, info, launches)
            if forcing_groups is not None:
                assert info["groups"] == forcing_groups, info


# ---------------------------------------------------------------- 1. forcing(t) alone
@pytest.mark.parametrize("grid", [(1, 1), (2, 2)], ids=["b1x1", "b2x2"])
def test_forcing_alone(amd, grid):
    """RHSx / RHSy after forcing(t) against the restatement on 121 x 65 with the rough coast, one block and 2 x 2
    blocks, every member with an uploaded h_r of its own (class hr: hu and hv vary from face to face); a second
    forcing() overwrites the first; the member without a storm keeps its +0.0."""
    shape = S.Shape(121, 65, grid, 0, "rough")
    classes = ["hr", "hr", "hr"]
    e = _start(amd, shape, classes)
    try:
        storms = {i: R.storm_for(shape, i) for i in (0, 2)}
        e.set_storms(storms, R.MODEL)
        assert e.forcing_info()["attached"] == 2
        e.forcing(123.0).forcing(4.5)
        assert e.synchronize() == [OK] * 3 and e.forcing_info()["applies"] == 2
        bad = []
        for i, m in enumerate(e.members):
            om = R.loaded(shape, classes[i], 1000 * i)
            where = {(b.bm, b.bn): k for k, b in enumerate(om.blocks)}
            assert len(m.blocks) == len(om.blocks) == grid[0] * grid[1]
            for b in m.blocks:
                k = where[(b.bm, b.bn)]
                want = R.block_rhs(om, k, storms[i], R.MODEL, 4.5) if i in storms else (om.f[k]["RHSx"], om.f[k]["RHSy"])
                for nm, w in zip(("RHSx", "RHSy"), want):
                    if not R.bits_equal(m.download(b.k, nm), w):
                        bad.append(f"member {i} ({b.bm},{b.bn}):{nm}")
                if i in storms:
                    assert (want[0] != 0.0).any() and (want[1] != 0.0).any()
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 2. step_forced against the oracle
@pytest.mark.parametrize("name,groups", [("one_tile", 1), ("many_tiles", 1), ("subset", 3), ("tau03", 1), ("one_point", 1)])
def test_step_forced_in_launch(amd, name, groups):
    """The run's calls -- odd and even step counts (the last forcing comes home from the second buffers or is there
    already), a 1-step call between them -- then complete(): every field of every member, RHSx / RHSy (the LAST
    step's forcing) included, is the oracle's; the calls of two steps or more ran as forcing launches.  All forced:
    one general group.  subset: the forced members 1 and 3 in the general group, the unforced known-constant and
    h_r-read members in groups of their own, in the same call."""
    per_call, _ = _run(amd, name)
    _assert_in_launch(name, per_call, groups)
    if name == "many_tiles":
        assert per_call[1][1]["tiles"] == 51, per_call[1][1]


@pytest.mark.parametrize("cap,groups,rows", [(2, 9, 16), (7, 3, 16)])
def test_several_groups(amd, cap, groups, rows):
    """Nine forced members under capacities 2 and 7 (tests/test_gpu_ensemble.py test_capacity_cap's plans: nine
    launches of one member, three of three, at 16 rows)."""
    per_call, _ = _run(amd, "groups", cap=cap)
    _assert_in_launch("groups", per_call, groups)
    assert per_call[1][1]["rows"] == rows, per_call[1][1]


def test_option_off_is_chunked(amd):
    """OCN_ENS_OPT_FORCING_IN_LAUNCH 0: every call chunked -- one k_ens_forcing ahead of each step -- bitwise all
    the same."""
    per_call, _ = _run(amd, "one_tile", before=lambda e: e.set_forcing_in_launch(False))
    assert [c[0] for c in per_call] == [False] * len(per_call), per_call


@pytest.mark.parametrize("n", [4, 5])
def test_last_forcing_and_pending_tail(amd, n):
    """One forcing launch of n steps, then complete() with no further step: it re-runs the pending tail -- the last
    step -- and must find that step's forcing in the fields' own arrays.  n = 4: it has come home from the second
    buffers; n = 5: the launch left it there.  Every field is the oracle's, RHSx / RHSy the last step's forcing."""
    name = "one_tile"
    shape, params, classes, _, _ = R.RUNS[name]
    e = _open(amd, name)
    try:
        e.step(R.FIRST)
        assert e.synchronize() == [OK] * len(e)
        e.step_forced(n, 1.0, 0.0)
        assert e.forcing_info()["in_launch"] and all(m.tail_pending for m in e.members)
        e.complete()
        st = e.synchronize()
        refs = [R.run_reference(name, i, (n,)) for i in range(len(e))]
        bad = _bad(e, refs)
        for i, ref in enumerate(refs):   # (what the comparison above holds RHSx to)
            om = R.loaded(shape, classes[i], 1000 * i, params)
            want = R.block_rhs(om, 0, R.run_storm(name, i), R.MODEL, float(n - 1))
            assert R.bits_equal(ref[(1, 1)]["RHSx"], want[0]) and R.bits_equal(ref[(1, 1)]["RHSy"], want[1])
    finally:
        e.close()
    assert st == [OK] * len(classes) and not bad, (st, bad)


# ---------------------------------------------------------------- 3. other configurations, bitwise all the same
@pytest.mark.parametrize("name", ["grid", "tracer"])
def test_block_grid_and_tracers(amd, name):
    """A 2 x 2 block grid and a tracer run: no multi-step launch there, so every call is chunked."""
    per_call, _ = _run(amd, name)
    assert [c[0] for c in per_call] == [False] * len(per_call), per_call


def test_check_every_two(amd):
    """check_every = 2: no multi-step launch checks every second step, so the calls are chunked, the checks at the
    steps of each call that 2 divides; the state is the oracle's."""
    per_call, _ = _run(amd, "subset", check_every=2)
    assert [c[0] for c in per_call] == [False] * len(per_call), per_call


def test_pair_option_runs_no_pair(amd):
    """Members set to OCN_OPT_PAIR 2, the in-launch route off: no pair launch runs for a forced member (a pair
    would defer steps whose forcing belongs to another time), and the state is the oracle's."""
    def before(e):
        e.set_forcing_in_launch(False)
        for m in e.members:
            m.set_pair(2)
    _, pairs = _run(amd, "one_tile", before=before)
    assert pairs == [False] * 5, pairs


# ---------------------------------------------------------------- 4. with the recorder
def test_forcing_then_step_record(amd):
    """forcing(t_s); step_record(1) per step: the series is the oracle's state at the stations after each step."""
    from ocean_model_arch_amd import ens_obs_rule
    name, steps = "one_tile", 5
    shape, params, classes, _, _ = R.RUNS[name]
    pts = [(7, 4), (33, 6), (60, 9), (21, 11)]
    e = _open(amd, name)
    try:
        op = ens_obs_rule.points("ssh", pts)
        e.record(op, every=1, max_records=steps)
        for s in range(steps):
            e.forcing(float(s)).step_record(1, tau=1.0)
        got = e.series()
        e.complete()
        st = e.synchronize()
        refs = [R.run_reference(name, i, (steps,), first=0) for i in range(len(e))]
        bad = _bad(e, refs)
    finally:
        e.close()
    want = np.array([[[ref["series"][s][(1, 1)]["ssh"][i - 1, j - 1] for ref in refs] for i, j in pts] for s in range(steps)])
    assert got.shape == want.shape == (steps, len(pts), len(classes)) and R.bits_equal(got, want)
    assert st == [OK] * len(classes) and not bad, (st, bad)


# ---------------------------------------------------------------- 5. a member that blows up
def test_blowup_stays_with_its_member(amd):
    """Member 1 under an absurd vmax: OCN_ERR_BLOWUP for it alone; the others are their oracle runs."""
    name, calls = "one_tile", (2, 6)
    e = _open(amd, name)
    try:
        e.set_storms({1: R.storm_for(R.RUNS[name][0], 1, vmax=1.0e9)}, R.MODEL)
        assert e.forcing_info()["attached"] == 5            # (the others keep their storms)
        e.step(R.FIRST)
        assert e.synchronize() == [OK] * len(e)
        tau, done = 1.0, 0
        for n in calls:
            e.step_forced(n, tau, float(done) * tau)
            assert e.forcing_info()["in_launch"]
            done += n
        e.complete()
        st = e.synchronize()
        refs = [R.run_reference(name, i, calls) for i in range(len(e))]
        bad = [x for x in _bad(e, refs) if not x.startswith("member 1 ")]
    finally:
        e.close()
    assert st == [OK, ERR_BLOWUP, OK, OK, OK], st
    assert not bad, bad


# ---------------------------------------------------------------- 6. clear_storms
def test_clear_storms_holds_the_last_forcing(amd):
    """clear_storms(), then an unforced call: the oracle with the last forcing held; forcing() and step_forced()
    are then refused (OCN_ERR_STATE) and nothing is launched."""
    name, calls, hold = "one_tile", (2, 5), 4
    e = _open(amd, name)
    try:
        _forced_calls(e, name, calls)
        e.clear_storms()
        assert e.forcing_info()["attached"] == 0
        with pytest.raises(amd.OcnError) as ei:
            e.forcing(1.0)
        assert ei.value.code == ERR_STATE
        with pytest.raises(amd.OcnError) as ei:
            e.step_forced(2, 1.0, 0.0)
        assert ei.value.code == ERR_STATE
        e.step(hold, tau=1.0)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, [R.run_reference(name, i, calls, hold=hold) for i in range(len(e))])
    finally:
        e.close()
    assert st == [OK] * len(R.RUNS[name][2]) and not bad, (st, bad)


def test_refusals_with_an_ensemble(amd):
    """What needs an ensemble to refuse: a storm list of the wrong length, a member outside the ensemble, a bad
    storm among good ones (nothing attached), forcing() with no storm, a time that is not finite."""
    from ocean_model_arch_amd import ens_forcing_rule as FR
    shape = S.Shape(61, 9)
    e = _start(amd, shape, ["noise", "noise"])
    try:
        good = R.storm_for(shape, 0)
        with pytest.raises(ValueError):
            e.set_storms([good])
        with pytest.raises(IndexError):
            e.set_storms({2: good})
        with pytest.raises(ValueError):
            e.set_storms([good, FR.Storm(x0=1.0, y0=1.0, radius=-5.0)])
        with pytest.raises(TypeError):
            e.set_storms([good, "storm"])
        assert e.forcing_info()["attached"] == 0
        with pytest.raises(amd.OcnError) as ei:
            e.forcing(0.0)
        assert ei.value.code == ERR_STATE
        e.set_storms([good, good])
        with pytest.raises(ValueError):
            e.forcing(float("nan"))
        with pytest.raises(TypeError):
            e.step_forced(2.5, 1.0, 0.0)
        with pytest.raises(ValueError):
            e.step_forced(-1, 1.0, 0.0)
        assert e.forcing_info() == {"attached": 2, "in_launch": False, "applies": 0, "steps": 0}
    finally:
        e.close()
