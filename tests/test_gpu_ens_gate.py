"""GPU tests of the gate inside the device filter (ocn_ens_set_gate; ens_assim.hip k_ens_obs_space_g, _hg, _rg in
front of the unchanged ens_local.hip k_ens_local) and of OceanEnsemble.assimilate*(gate=).

The reference is the gated numpy restatement (ens_local_rule.ensrf_obs_space_ordered(gate2=), checked against a
scalar loop by tests/test_ens_gate_cpu.py) on the members' own sample() and downloads, the host route
(device=False) on a twin ensemble, or the ungated call on a twin.  Shapes, inputs and helpers are those of
tests/test_gpu_ens_assim.py.  Every comparison is bitwise on whole arrays (NaN by position).  Tolerance: none.

Planted outliers are a condition, not a measurement: values are the prior mean +- 0.1 with variances >= 0.01
(_obs_values), so d^2 <= 0.01 <= 9 D for them, and a planted value is the prior mean + 1e3.  Before the device is
compared, each test asserts ON THE RESTATEMENT that `accepted` is exactly the planted pattern: no test passes with
the gate inert.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ens_assim_ref as A
from tests import shapes as S
from tests.test_gpu_ens_assim import STAGE_LAUNCHES, THREADS, _obs_values, _points
from tests.test_gpu_ens_local import OBS_61x9
from tests.test_gpu_ens_transform import _downloads, _run
from tests.test_gpu_ensemble import _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, 1
GATE = 3.0
KEYS = set(A.KEYS) | {"nonfinite", "accepted", "rejected"}


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _plant(hx0, seed, planted):
    """_obs_values' values and variances, with the prior mean + 1e3 at the planted indices."""
    values, variances = _obs_values(hx0, seed)
    for k in planted:
        values[k] = hx0[k].mean() + 1e3
    return values, variances


def _gated_vs_restatement(e, name, ij, taper, names, planted, gate=GATE, members=None, seed=0, values=None, expect=None):
    """assimilate(device=True, gate=) against the gated restatement on the members' own sample() and downloads, on
    every block.  `expect`: the accepted pattern the restatement must give (default: all but `planted`).  Returns
    (what differs, the launches of the call, the returned dict, the sample() before)."""
    from ocean_model_arch_amd import _lib
    idx = list(range(len(e))) if members is None else sorted(set(members))
    blocks = e.members[0].blocks
    held = tuple(dict.fromkeys(tuple(names) + (name,)))
    before = {b.k: _downloads(e, held, idx, b.k) for b in blocks}
    hx0 = e.sample(name, _points(e, ij), members=members)
    if values is None:
        values, variances = _plant(hx0, seed, planted)
    else:
        values, variances = values
    Y, Z, ref = A.ensrf_obs_space_ordered(hx0, ij, values, variances, taper, gate2=gate * gate)
    want_acc = [k not in planted for k in range(len(ij))] if expect is None else list(expect)
    assert list(ref["accepted"]) == want_acc, "the restatement does not give the planted pattern"
    acc = ref["accepted"]
    l0 = _lib.launch_count()
    got = e.assimilate(name, ij, values, variances, taper, names=names, members=members, device=True, gate=gate)
    launches = _lib.launch_count() - l0
    yz = e.assimilate_results(("y", "z"))
    bad = []
    if set(got) != KEYS:
        bad.append(f"keys {sorted(got)}")
    bad += A.info_mismatches(got, ref)
    bad += [nm for nm, a, r in (("Y", yz["y"], Y), ("Z", yz["z"], Z)) if not A.bits_equal(a, r)]
    if got["nonfinite"] != ref["nonfinite"] or got["rejected"] != ref["rejected"]:
        bad.append(f"nonfinite {got['nonfinite']} / {ref['nonfinite']}, rejected {got['rejected']} / {ref['rejected']}")
    if got["accepted"].dtype != bool or list(got["accepted"]) != want_acc:
        bad.append("accepted")
    for b in blocks:
        after = _downloads(e, held, idx, b.k)
        for nm in held:
            want = before[b.k][nm]
            if nm in names and acc.any():   # a rejected observation forms nothing: the update of the accepted ones alone
                want = A.block_update(want, b, ij[acc, 0], ij[acc, 1], Y[acc], Z[acc], taper)
            bad += [f"member {i} [{b.k}]:{nm}" for i, g, v in zip(idx, after[nm], want) if not A.bits_equal(g, v)]
    now = e.sample(name, _points(e, ij), members=members)
    if not A.bits_equal(now, got["hx"] if name in names else hx0):
        bad.append("sample() afterwards")
    return bad, launches, got, hx0


# ---------------------------------------------------------------- 1. member counts and tapers; a duplicate point
@pytest.fixture(scope="module")
def ens33(amd):
    e = _start(amd, S.Shape(61, 9), ["noise"] * 33)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 33
        yield e
    finally:
        e.close()


@pytest.mark.parametrize("n", [2, 9, 32, 33])
def test_member_counts(amd, ens33, n):
    """n members in use across the update's register / LDS boundary, a Gaspari-Cohn and a ringed taper.  Outliers
    planted at k = 2 -- OBS_61x9's point (30, 6), whose second copy k = 3 is good -- and at k = 7."""
    e = ens33
    names = ("ssh", "ubrtr")
    members = None if n == 33 else range(n)
    assert (OBS_61x9[2] == OBS_61x9[3]).all()
    for t, (what, taper) in enumerate([("gaspari-cohn", A.taper_table(6.0)), ("ring", A.ringed_taper(50))]):
        bad, launches, got, hx0 = _gated_vs_restatement(e, "ssh", OBS_61x9, taper, names, (2, 7), members=members,
                                                        seed=10 * n + t)
        assert not bad, (what, bad)
        assert launches == len(names) * 1 + STAGE_LAUNCHES, what
        assert got["hx"].shape == (len(OBS_61x9), n) and got["rejected"] == 2 and got["nonfinite"] == 0
        assert not A.bits_equal(got["hx"], hx0), what


# ---------------------------------------------------------------- 2. the strides of row ownership
def test_row_strides(amd):
    """2 THREADS + 3 observations at random points with repeats, outliers planted at k = 0, THREADS - 1, THREADS and
    the last k: the first and the second stride of row ownership, and the list entries a thread rewrites."""
    nobs = 2 * THREADS + 3
    planted = (0, THREADS - 1, THREADS, nobs - 1)
    e = _start(amd, S.Shape(61, 9), ["noise"] * 8)
    try:
        _run(e, [2, 3])
        rng = np.random.default_rng(nobs)
        ij = np.stack([rng.integers(1, 66, nobs), rng.integers(1, 14, nobs)], axis=1)
        ij[nobs - 1] = ij[0]
        ij[THREADS] = ij[3]
        bad, launches, got, _ = _gated_vs_restatement(e, "ssh", ij, A.taper_table(6.0), ("ssh", "ubrtr"), planted, seed=nobs)
    finally:
        e.close()
    assert not bad, bad
    assert launches == 2 + STAGE_LAUNCHES
    assert got["rejected"] == 4 and got["nonfinite"] == 0


# ---------------------------------------------------------------- 3. a duplicate point, both orders
@pytest.mark.parametrize("first_is_outlier", [True, False])
def test_duplicate_point(amd, first_is_outlier):
    e = _start(amd, S.Shape(61, 9), ["noise"] * 5)
    try:
        _run(e, [2, 3])
        ij = np.array([[12, 3], [30, 6], [47, 5], [30, 6], [33, 8]])
        bad, _, got, hx0 = _gated_vs_restatement(e, "ssh", ij, A.taper_table(6.0), ("ssh",), (1,) if first_is_outlier else (3,),
                                                 seed=3)
    finally:
        e.close()
    assert not bad, bad
    assert got["rejected"] == 1 and A.bits_equal(got["hx"][1], got["hx"][3]) and not A.bits_equal(got["hx"][1], hx0[1])


# ---------------------------------------------------------------- 4. gate = inf is the ungated call
def test_inf_is_the_ungated_call(amd):
    """Twin ensembles: assimilate(device=True, gate=inf) on one, assimilate(device=True) on the other -- the fields,
    the results, Y, Z and the launches; everything accepted."""
    from ocean_model_arch_amd import _lib
    names = ("ssh", "ubrtr")
    es = [_start(amd, S.Shape(61, 9), ["noise"] * 9) for _ in range(2)]
    try:
        for e in es:
            _run(e, [2, 3])
            e.complete()                          # (no tail is formed inside the launches counted below)
        hx0 = es[0].sample("ssh", _points(es[0], OBS_61x9))
        values, variances = _obs_values(hx0, 4)
        taper = A.taper_table(6.0)
        got, yz, launches = [], [], []
        for e, gate in zip(es, (np.inf, None)):
            l0 = _lib.launch_count()
            got.append(e.assimilate("ssh", OBS_61x9, values, variances, taper, names=names, device=True, gate=gate))
            launches.append(_lib.launch_count() - l0)
            yz.append(e.assimilate_results(("y", "z")))
        fields = [_downloads(e, names, range(9)) for e in es]
    finally:
        for e in es:
            e.close()
    assert set(got[0]) == KEYS and set(got[1]) == set(A.KEYS) | {"nonfinite"}
    assert got[0]["accepted"].all() and got[0]["rejected"] == 0
    assert not A.info_mismatches(got[0], got[1]) and got[0]["nonfinite"] == got[1]["nonfinite"] == 0
    assert A.bits_equal(yz[0]["y"], yz[1]["y"]) and A.bits_equal(yz[0]["z"], yz[1]["z"])
    assert all(A.bits_equal(a, b) for nm in names for a, b in zip(fields[0][nm], fields[1][nm]))
    assert not A.bits_equal(got[0]["hx"], hx0)
    assert launches[0] == launches[1] == len(names) + STAGE_LAUNCHES


# ---------------------------------------------------------------- 5. all observations rejected
def test_all_rejected(amd):
    """Every value the prior mean + 1e3: no field bit and no hx bit changes, and the launches are the ungated
    call's (the host does not know what was rejected)."""
    names = ("ssh", "ubrtr")
    e = _start(amd, S.Shape(61, 9), ["noise"] * 6)
    try:
        _run(e, [2, 3])
        bad, launches, got, hx0 = _gated_vs_restatement(e, "ssh", OBS_61x9, A.taper_table(6.0), names, range(len(OBS_61x9)),
                                                        seed=5)
    finally:
        e.close()
    assert not bad, bad                        # (the fields against their own downloads before)
    assert not got["accepted"].any() and got["rejected"] == len(OBS_61x9)
    assert A.bits_equal(got["hx"], hx0) and A.bits_equal(got["posterior_spread"], got["prior_spread"])
    assert launches == len(names) + STAGE_LAUNCHES


# ---------------------------------------------------------------- 6. a member that is NaN at an observed point
def test_nan_member(amd):
    """Member 3's ssh is NaN at (30, 6), observed once: that observation is rejected and counted, and no NaN
    appears anywhere else -- in no other member, and in member 3 nowhere but there.  (The observations are
    OBS_61x9's that do not reach (30, 6): the update's rule at a state point reads every member there, so an
    ACCEPTED observation within reach of a NaN point spreads it as ever -- that is the update's contract, not the
    gate's.)"""
    names = ("ssh", "ubrtr")
    taper = A.taper_table(6.0)
    ij = np.array([p for k, p in enumerate(OBS_61x9) if k == 2 or (p[0] - 30) ** 2 + (p[1] - 6) ** 2 >= len(taper)])
    assert [tuple(p) for p in ij].count((30, 6)) == 1 and tuple(ij[2]) == (30, 6) and len(ij) == 8
    e = _start(amd, S.Shape(61, 9), ["noise"] * 6)
    try:
        _run(e, [2, 3])
        e.complete()
        b = e.members[0].blocks[0]
        a = e.members[3].download(0, "ssh")
        a[30 - b.bnd_x1, 6 - b.bnd_y1] = np.nan
        e.members[3].upload(0, "ssh", a)
        clean = e.sample("ssh", _points(e, ij), members=[0, 1, 2, 4, 5])
        bad, launches, got, _ = _gated_vs_restatement(e, "ssh", ij, taper, names, (2,), seed=7, values=_obs_values(clean, 7))
        after = _downloads(e, names, range(6))
    finally:
        e.close()
    assert not bad, bad
    assert got["nonfinite"] == 1 and got["rejected"] == 1 and list(got["accepted"]) == [k != 2 for k in range(len(ij))]
    nans = {nm: [int(np.isnan(x).sum()) for x in after[nm]] for nm in names}
    assert nans == {"ssh": [0, 0, 0, 1, 0, 0], "ubrtr": [0] * 6}, nans
    assert launches == len(names) + STAGE_LAUNCHES


# ---------------------------------------------------------------- 7. the tie
def test_the_tie(amd):
    """2 members with ssh = -1 and +1 everywhere, one observation with r = 2: ybar = 0, D = 4, lim = 9 D = 36.  The
    value 6 is accepted (36 <= 36); the next double above 6 is rejected and changes nothing."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 2)
    try:
        _run(e, [2, 3])
        e.complete()
        shape = e.members[0].blocks[0].shape
        res = []
        for value in (6.0, np.nextafter(6.0, np.inf)):
            for m, v in zip(e.members, (-1.0, 1.0)):
                m.upload(0, "ssh", np.full(shape, v))
            got = e.assimilate("ssh", np.array([[31, 7]]), [value], [2.0], np.array([1.0]), names=("ssh",), device=True, gate=GATE)
            res.append((got, e.sample("ssh", [(0, 31, 7)])[0], e.assimilate_results(("y", "z"))))
        ref = [A.ensrf_obs_space_ordered(np.array([[-1.0, 1.0]]), np.array([[31, 7]]), [v], [2.0], np.array([1.0]), gate2=9.0)
               for v in (6.0, np.nextafter(6.0, np.inf))]
    finally:
        e.close()
    assert list(ref[0][2]["accepted"]) == [True] and list(ref[1][2]["accepted"]) == [False]
    (at, x_at, yz_at), (above, x_above, yz_above) = res
    assert list(at["accepted"]) == [True] and at["rejected"] == 0 and at["innovations"][0] == 6.0
    assert list(above["accepted"]) == [False] and above["rejected"] == 1 and above["innovations"][0] == np.nextafter(6.0, np.inf)
    assert A.bits_equal(x_at, ref[0][2]["hx"][0]) and not A.bits_equal(x_at, np.array([-1.0, 1.0]))
    assert A.bits_equal(x_above, np.array([-1.0, 1.0]))
    assert A.bits_equal(yz_at["z"], ref[0][1]) and A.bits_equal(yz_above["z"], np.zeros((1, 2)))
    assert A.bits_equal(yz_above["y"], np.array([[-1.0, 1.0]]))


# ---------------------------------------------------------------- 8. a block grid
def test_block_grid(amd):
    """A 2 x 2 block grid, 5 members: the rejected observation sits at the seams' corner and its reach meets all four
    blocks' arrays -- every block's list is rewritten; its second copy at the same point is good."""
    names = ("ssh", "ubrtr")
    e = _start(amd, S.Shape(17, 19, (2, 2)), ["noise"] * 5)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 5
        blocks = e.members[0].blocks
        assert len(blocks) == 4
        sx, sy = max(b.nx_start for b in blocks), max(b.ny_start for b in blocks)
        ij = np.array([[3, 3], [19, 21], [sx - 1, sy], [sx, sy - 1], [1, 12], [sx, sy - 1], [21, 23], [sx + 2, 4], [5, sy + 1]])
        taper = A.taper_table(9.0)
        reach = 8
        assert len(taper) > reach * reach
        assert all(sx + reach >= b.bnd_x1 and sx - reach <= b.bnd_x2 and sy - 1 + reach >= b.bnd_y1 and sy - 1 - reach <= b.bnd_y2
                   for b in blocks)
        bad, launches, got, _ = _gated_vs_restatement(e, "ssh", ij, taper, names, (3,), seed=4)
        bad2, launches2, got2, _ = _gated_vs_restatement(e, "ssh", ij, A.ringed_taper(10, 3), names, (0, 3, 5), seed=5)
    finally:
        e.close()
    assert not bad and not bad2, (bad, bad2)
    assert got["rejected"] == 1 and got2["rejected"] == 3
    assert launches == launches2 == len(names) * 4 + STAGE_LAUNCHES


# ---------------------------------------------------------------- 9. the two routes of the Python driver
def _twins_equal(es, names, n):
    fa, fb = (_downloads(e, names, range(n)) for e in es)
    return [(nm, i) for nm in names for i in range(n) if not A.bits_equal(fa[nm][i], fb[nm][i])]


def test_device_against_host_route(amd):
    """Twin ensembles of 5 members (up to 8 members numpy's own reductions run in member order, so the host route's
    loop has the device's bits): assimilate(gate=) with device=True on one, device=False on the other -- fields
    and results; then again with rtps=0.5."""
    n, names = 5, ("ssh", "ubrtr")
    es = [_start(amd, S.Shape(61, 9), ["noise"] * n) for _ in range(2)]
    bad = []
    try:
        for e in es:
            _run(e, [2, 3])
        for t, rtps in enumerate((None, 0.5)):
            hx0 = es[0].sample("ssh", _points(es[0], OBS_61x9))
            values, variances = _plant(hx0, t, (0, 3, 10))
            got = [e.assimilate("ssh", OBS_61x9, values, variances, A.taper_table(6.0), names=names, device=dev, rtps=rtps,
                                gate=GATE) for e, dev in zip(es, (True, False))]
            assert list(got[1]["accepted"]) == [k not in (0, 3, 10) for k in range(len(OBS_61x9))]   # (the host loop)
            if set(got[0]) != KEYS or set(got[1]) != KEYS - {"nonfinite"}:
                bad.append((rtps, "keys"))
            bad += [(rtps, k) for k in A.info_mismatches(got[0], got[1])]
            if list(got[0]["accepted"]) != list(got[1]["accepted"]) or not got[0]["rejected"] == got[1]["rejected"] == 3:
                bad.append((rtps, "accepted"))
            bad += [(rtps,) + x for x in _twins_equal(es, names, n)]
            if A.bits_equal(got[0]["hx"], hx0):
                bad.append((rtps, "nothing happened"))
    finally:
        for e in es:
            e.close()
    assert not bad, bad


def test_h_and_recorded_routes(amd):
    """assimilate_h(gate=) and assimilate_recorded(gate=) against their host routes on twins of 5 members, with
    planted outliers at the first, a middle and the last observation; the launches are the ungated call's."""
    from ocean_model_arch_amd import _lib
    from tests.test_gpu_ens_fgat import SMALL, STATE, _anchored, _recorded
    n = 5
    es = [_recorded(amd, SMALL, ["noise"] * n, 9, [2, 4])[0] for _ in range(2)]
    op = _anchored(SMALL, 9, 0)
    bad = []
    try:
        for e in es:
            e.complete()                          # (no tail is formed inside the launches counted below)
        taper = A.taper_table(5.0)
        # observations at their own times
        rng = np.random.default_rng(1)
        records = es[0].record_info()["records"]
        at = rng.uniform(1.0, float(records), 20)
        at[:3] = [1.0, 2.5, float(records)]
        rows = rng.integers(0, 9, 20)
        planted = (0, 9, 19)
        hx0 = es[0].sample_recorded(rows, at)
        values, variances = _plant(hx0, 1, planted)
        l0 = _lib.launch_count()
        got = [es[0].assimilate_recorded(rows, at, values, variances, taper, device=True, gate=GATE)]
        launches = _lib.launch_count() - l0
        got.append(es[1].assimilate_recorded(rows, at, values, variances, taper, device=False, gate=GATE))
        assert list(got[1]["accepted"]) == [k not in planted for k in range(20)]                     # (the host loop)
        if launches != len(STATE) + STAGE_LAUNCHES:
            bad.append(("recorded", "launches", launches))
        bad += _route_mismatches("recorded", got, hx0, es, STATE, n)
        # a sparse linear H
        planted = (0, 4, 8)
        hx0 = es[0].sample_h(op)
        values, variances = _plant(hx0, 2, planted)
        l0 = _lib.launch_count()
        got = [es[0].assimilate_h(op, values, variances, taper, device=True, gate=GATE)]
        launches = _lib.launch_count() - l0
        got.append(es[1].assimilate_h(op, values, variances, taper, device=False, gate=GATE))
        assert list(got[1]["accepted"]) == [k not in planted for k in range(9)]                      # (the host loop)
        if launches != len(STATE) + STAGE_LAUNCHES:
            bad.append(("h", "launches", launches))
        bad += _route_mismatches("h", got, hx0, es, STATE, n)
    finally:
        for e in es:
            e.close()
    assert not bad, bad


def _route_mismatches(what, got, hx0, es, names, n):
    bad = []
    if set(got[0]) != KEYS or set(got[1]) != KEYS - {"nonfinite"}:
        bad.append((what, "keys"))
    bad += [(what, k) for k in A.info_mismatches(got[0], got[1])]
    if list(got[0]["accepted"]) != list(got[1]["accepted"]) or got[0]["rejected"] != got[1]["rejected"] or got[0]["nonfinite"]:
        bad.append((what, "accepted"))
    bad += [(what,) + x for x in _twins_equal(es, names, n)]
    if A.bits_equal(got[0]["hx"], hx0):
        bad.append((what, "nothing happened"))
    return bad


# ---------------------------------------------------------------- 10. the C entries
def test_set_gate_errors_and_a_gate_that_does_not_leak(amd):
    """ocn_ens_set_gate: every bad value is OCN_ERR_ARG and leaves the setting and the state as they were; 0.0 of
    either sign turns it off.  A gated call followed by an ungated one: ACCEPTED all 1.0, nothing rejected."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    e = _start(amd, S.Shape(61, 9), ["noise"] * 3)
    try:
        _run(e, [2, 3])
        e.complete()
        info = _lib.OcnEnsGateInfo()
        before = _downloads(e, ("ssh",), range(3))["ssh"]
        l0 = _lib.launch_count()
        assert L.ocn_ens_gate_info(e.ens, C.byref(info)) == OK and (info.gate2, info.rejected) == (0.0, 0)
        assert L.ocn_ens_set_gate(e.ens, 9.0) == OK
        for v in (-1.0, -5e-324, float("nan"), -float("inf")):
            assert L.ocn_ens_set_gate(e.ens, v) == ERR_ARG, v
            assert L.ocn_ens_gate_info(e.ens, C.byref(info)) == OK and info.gate2 == 9.0, v
        assert L.ocn_ens_set_gate(None, 9.0) == ERR_ARG and L.ocn_ens_gate_info(e.ens, None) == ERR_ARG
        assert L.ocn_ens_gate_info(None, C.byref(info)) == ERR_ARG
        assert L.ocn_ens_set_gate(e.ens, float("inf")) == OK and e.gate_info() == {"gate2": float("inf"), "rejected": 0}
        assert L.ocn_ens_set_gate(e.ens, -0.0) == OK and e.gate_info() == {"gate2": 0.0, "rejected": 0}
        assert L.ocn_ens_set_gate(e.ens, 9.0) == OK and L.ocn_ens_set_gate(e.ens, 0.0) == OK and e.gate_info()["gate2"] == 0.0
        assert _lib.launch_count() == l0
        assert all(A.bits_equal(a, b) for a, b in zip(before, _downloads(e, ("ssh",), range(3))["ssh"]))
        with pytest.raises(ValueError):
            e.assimilate("ssh", OBS_61x9[:2], [0.1, 0.1], [0.01, 0.01], np.array([1.0]), device=True, gate=-3.0)
        with pytest.raises(TypeError):
            e.assimilate("ssh", OBS_61x9[:2], [0.1, 0.1], [0.01, 0.01], np.array([1.0]), device=True, gate="3")
        assert _lib.launch_count() == l0
        # a gated call, its results through the C entries, then an ungated one
        ij = OBS_61x9
        hx0 = e.sample("ssh", _points(e, ij))
        values, variances = _plant(hx0, 1, (1, 5))
        got = e.assimilate("ssh", ij, values, variances, A.taper_table(6.0), names=("ssh",), device=True, gate=GATE)
        acc = np.full(len(ij), 7.5)
        assert L.ocn_ens_assimilate_result(e.ens, _lib.ENS_ASSIM_ACCEPTED, acc.ctypes.data_as(C.c_void_p)) == OK
        assert list(acc) == [0.0 if k in (1, 5) else 1.0 for k in range(len(ij))] and got["rejected"] == 2
        assert e.gate_info() == {"gate2": 9.0, "rejected": 2}
        values, variances = _obs_values(e.sample("ssh", _points(e, ij)), 2)
        plain = e.assimilate("ssh", ij, values, variances, A.taper_table(6.0), names=("ssh",), device=True)
        acc[:] = 7.5
        assert L.ocn_ens_assimilate_result(e.ens, _lib.ENS_ASSIM_ACCEPTED, acc.ctypes.data_as(C.c_void_p)) == OK
        assert (acc == 1.0).all() and e.gate_info() == {"gate2": 0.0, "rejected": 0}
        assert set(plain) == set(A.KEYS) | {"nonfinite"}
        assert L.ocn_ens_assimilate_result(e.ens, 7, acc.ctypes.data_as(C.c_void_p)) == ERR_ARG
    finally:
        e.close()
