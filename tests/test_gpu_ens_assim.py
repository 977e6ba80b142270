"""GPU tests of the serial filter on the device (ocn_ens_assimilate; ens_assim.hip k_ens_obs_space in front of
ens_local.hip k_ens_local) and of OceanEnsemble.assimilate(device=True).

The reference is the numpy restatement of the contract (tests/ens_assim_ref.py, itself checked against a
scalar loop by tests/test_ens_assim_cpu.py) on the members' own sample() and downloads, or on the CPU
oracle's fields; shapes, inputs and helpers are those of tests/test_gpu_ens_local.py.  Every comparison is
bitwise on whole arrays (NaN by position).  Tolerance: none, but for the scalar Kalman update (ANALYTIC_TOL).
"""
import ctypes as C

import numpy as np
import pytest

from tests import ens_assim_ref as A
from tests import shapes as S
from tests.test_ens_local_cpu import ANALYTIC_TOL, ANALYTIC_VALUE, ANALYTIC_VAR, analytic_check
from tests.test_gpu_ens_local import OBS_61x9, _oracle_update, _ring_mismatches
from tests.test_gpu_ens_transform import _bad_vs, _downloads, _oracles, _pending, _run
from tests.test_gpu_ensemble import _bad, _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, 1
THREADS = 256        # ens_assim.hip kAsThreads: row j belongs to thread j mod THREADS
STAGE_LAUNCHES = 1   # ocn_ens_filter.hip kAsLaunches: the observation-space stage, whatever n and nobs


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _points(e, ij):
    return [(e.block_of(int(i), int(j)), int(i), int(j)) for i, j in ij]


def _obs_values(prior, seed):
    """Values and variances as tests/test_gpu_ens_local.py test_assimilate chooses them: the fields stay O(1)."""
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        values = prior.mean(axis=1) + rng.uniform(-0.1, 0.1, len(prior))
        variances = np.full(len(prior), 0.01) + prior.var(axis=1, ddof=1) * 0.5
    return values, variances


def _assim_vs_restatement(e, name, ij, taper, names, members=None, seed=0, values=None, variances=None):
    """assimilate(device=True) against the restatement on the members' own sample() and downloads, on every
    block.  Returns (what differs, the launches of the call, the returned dict, the sample() before)."""
    from ocean_model_arch_amd import _lib
    idx = list(range(len(e))) if members is None else sorted(set(members))
    blocks = e.members[0].blocks
    held = tuple(dict.fromkeys(tuple(names) + (name,)))
    before = {b.k: _downloads(e, held, idx, b.k) for b in blocks}
    hx0 = e.sample(name, _points(e, ij), members=members)
    bad = []
    if not A.bits_equal(hx0, A.gather({k: before[k][name] for k in before}, blocks, e.block_of, ij)):
        bad.append("sample() before is not the downloads at block_of's block")
    if values is None:
        values, variances = _obs_values(hx0, seed)
    l0 = _lib.launch_count()
    got = e.assimilate(name, ij, values, variances, taper, names=names, members=members, device=True)
    launches = _lib.launch_count() - l0
    yz = e.assimilate_results(("y", "z"))
    Y, Z, ref = A.ensrf_obs_space_ordered(hx0, ij, values, variances, taper)
    if set(got) != set(A.KEYS) | {"nonfinite"}:
        bad.append(f"keys {sorted(got)}")
    bad += A.info_mismatches(got, ref)
    bad += [nm for nm, a, r in (("Y", yz["y"], Y), ("Z", yz["z"], Z)) if not A.bits_equal(a, r)]
    if got["nonfinite"] != ref["nonfinite"]:
        bad.append(f"nonfinite {got['nonfinite']} != {ref['nonfinite']}")
    for b in blocks:
        after = _downloads(e, held, idx, b.k)
        for nm in held:
            want = (A.block_update(before[b.k][nm], b, ij[:, 0], ij[:, 1], Y, Z, taper) if nm in names else before[b.k][nm])
            bad += [f"member {i} [{b.k}]:{nm}" for i, g, v in zip(idx, after[nm], want) if not A.bits_equal(g, v)]
    now = e.sample(name, _points(e, ij), members=members)
    if not A.bits_equal(now, got["hx"] if name in names else hx0):
        bad.append("sample() afterwards")
    return bad, launches, got, hx0


# ---------------------------------------------------------------- 1. member counts and tapers
@pytest.fixture(scope="module")
def ens33(amd):
    """33 members of Shape(61, 9), class noise, after calls [2, 3], complete."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 33)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 33
        yield e
    finally:
        e.close()


@pytest.mark.parametrize("n", [2, 5, 8, 9, 32, 33])
def test_member_counts(amd, ens33, n):
    """n members in use, across the update's register / LDS boundary (32 / 33; the observation-space kernel
    has one path).  Four tapers in turn; all zero: Y and Z are formed, no field bit changes, hx stays.  The
    members not in use keep their bits; the launches are the update's plus STAGE_LAUNCHES."""
    e = ens33
    names = ("ssh", "ubrtr")
    members = None if n == 33 else range(n)
    outside = None if n == 33 else e.members[32].download(0, "ssh")
    tapers = [("gaspari-cohn", A.taper_table(6.0)), ("ring", A.ringed_taper(50)), ("one entry", np.array([0.75])),
              ("all zero", np.array([0.0, -0.0] * 15))]
    for t, (what, taper) in enumerate(tapers):
        bad, launches, got, hx0 = _assim_vs_restatement(e, "ssh", OBS_61x9, taper, names, members, seed=10 * n + t)
        assert not bad, (what, bad)
        assert launches == len(names) * 1 + STAGE_LAUNCHES, what
        assert got["hx"].shape == (len(OBS_61x9), n)
        assert A.bits_equal(got["hx"], hx0) == (what == "all zero"), what
    if outside is not None:
        assert A.bits_equal(e.members[32].download(0, "ssh"), outside)


# ---------------------------------------------------------------- 2. rows per thread
@pytest.mark.parametrize("nobs", [1, THREADS + 1, 2 * THREADS + 3])
def test_rows_per_thread(amd, nobs):
    """1, THREADS + 1 and 2 THREADS + 3 observations at random interior and halo points with repeats: threads
    that own zero, one, two and three rows, and the last partial stride."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 8)
    try:
        _run(e, [2, 3])
        rng = np.random.default_rng(nobs)
        ij = np.stack([rng.integers(1, 66, nobs), rng.integers(1, 14, nobs)], axis=1)
        if nobs > 4:
            ij[nobs - 1] = ij[0]
            ij[THREADS] = ij[3]
        bad, launches, got, _ = _assim_vs_restatement(e, "ssh", ij, A.taper_table(6.0), ("ssh", "ubrtr"), seed=nobs)
    finally:
        e.close()
    assert not bad, bad
    assert launches == 2 + STAGE_LAUNCHES
    assert got["hx"].shape == (nobs, 8) and got["nonfinite"] == 0


# ---------------------------------------------------------------- 3. a block grid
def test_block_grid(amd):
    """A 2 x 2 block grid, 5 members, the observation list of the update's test (both sides of the seams, the
    basin's outer ring, a repeat): hx gathered in block_of's block, every block against the restatement, and
    the halo rings coherent before and after."""
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
        assert len({e.block_of(int(i), int(j)) for i, j in ij}) == 4
        was, _ = _ring_mismatches(e, names, range(5))
        bad, launches, _, _ = _assim_vs_restatement(e, "ssh", ij, A.ringed_taper(10, 3), names, seed=3)
        lost, _ = _ring_mismatches(e, names, range(5))
        bad2, launches2, _, _ = _assim_vs_restatement(e, "ssh", ij, A.taper_table(9.0), names, seed=4)
        lost2, _ = _ring_mismatches(e, names, range(5))
    finally:
        e.close()
    assert not was and not bad and not bad2, (was, bad, bad2)
    assert not lost and not lost2, (lost, lost2)
    assert launches == launches2 == len(names) * 4 + STAGE_LAUNCHES


# ---------------------------------------------------------------- 4. the observed field is not among the updated ones
def test_observed_field_not_updated(amd):
    """ssh observed, ubrtr and vbrtr updated: ssh keeps its bits everywhere, HX is still the restatement's
    (the rows follow the rule, not the field), the listed fields are the restatement's."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 5)
    try:
        _run(e, [2, 3])
        bad, launches, got, hx0 = _assim_vs_restatement(e, "ssh", OBS_61x9, A.taper_table(6.0), ("ubrtr", "vbrtr"), seed=41)
    finally:
        e.close()
    assert not bad, bad                        # (ssh against its own download before; sample() afterwards == before)
    assert launches == 2 + STAGE_LAUNCHES
    assert not A.bits_equal(got["hx"], hx0)


# ---------------------------------------------------------------- 5. pending tails, the upload rule, a subset
def test_continue_as_the_oracle_continues(amd):
    """9 members after calls [2, 5]: the tails pending, the pair roles swapped.  The analysis over all members
    but one, then 4 more steps: every field of every member equals the oracle run 7 steps, updated by the
    restatement from the oracle's own values at the observed points, run 4 steps more; only the tails of the
    members in use were formed."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 9, [2, 5]
    use = [0, 1, 2, 3, 5, 6, 7, 8]
    ij = OBS_61x9
    taper = A.taper_table(6.0)
    oms = _oracles(shape, classes, sum(calls))
    ob = oms[0].blocks[0]
    hx = np.array([[oms[i].f[0]["ssh"][int(a) - ob.bx1, int(b) - ob.by1] for i in use] for a, b in ij])
    values, variances = _obs_values(hx, 5)
    Y, Z, ref = A.ensrf_obs_space_ordered(hx, ij, values, variances, taper)
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 9
        got = e.assimilate("ssh", ij, values, variances, taper, members=use, device=True)
        pending = _pending(e)
        e.step(4)
        e.complete()
        st = e.synchronize()
        _oracle_update(oms, Y, Z, ij, taper, A.STATE, members=use)
        for om in oms:
            om.run(4, 1.0)
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert pending == [i == 4 for i in range(9)], pending
    assert not A.info_mismatches(got, ref) and got["nonfinite"] == 0
    assert st == [OK] * 9 and not bad, (st, bad)


# ---------------------------------------------------------------- 6. the Python driver
def test_python_driver(amd):
    """assimilate(device=True) on the inputs of the update's test_assimilate: the five keys, the spread shrinks
    at every observed point; then one observation with taper [1.0] against the scalar Kalman update in extended
    precision, and nothing changes anywhere else."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 8)
    try:
        _run(e, [2, 3])
        rng = np.random.default_rng(12)
        ij = np.stack([rng.integers(3, 64, 12), rng.integers(3, 12, 12)], axis=1)
        ij[5] = ij[2]
        prior = e.sample("ssh", [(0, int(i), int(j)) for i, j in ij])
        values = prior.mean(axis=1) + rng.uniform(-0.1, 0.1, 12)
        variances = np.full(12, 0.01) + prior.var(axis=1, ddof=1) * 0.5
        info = e.assimilate("ssh", ij, values, variances, amd.ensemble.taper_table(6.0), device=True)
        b = e.members[0].blocks[0]
        xs = np.random.default_rng(5).uniform(0.5, 1.5, (8,) + b.shape)
        for m, a in zip(e.members, xs):
            m.upload(0, "ssh", a)
        p1 = e.sample("ssh", [(0, 31, 7)])[0]
        held = _downloads(e, ("ssh",), range(8))["ssh"]
        one = e.assimilate("ssh", np.array([[31, 7]]), [ANALYTIC_VALUE], [ANALYTIC_VAR], np.array([1.0]), names=("ssh",),
                           device=True)
        q1 = e.sample("ssh", [(0, 31, 7)])[0]
        now = _downloads(e, ("ssh",), range(8))["ssh"]
        with pytest.raises(ValueError):        # a split that would not compose
            e.assimilate("ssh", np.full((8193, 2), 5), np.zeros(8193), np.ones(8193), np.array([1.0]), names=("ubrtr",), device=True)
    finally:
        e.close()
    assert set(info) == {"hx", "innovations", "prior_spread", "posterior_spread", "nonfinite"}
    assert info["hx"].shape == (12, 8) and info["nonfinite"] == 0
    assert (info["posterior_spread"] < info["prior_spread"]).all()
    em, ev = analytic_check(p1, q1, ANALYTIC_VALUE, ANALYTIC_VAR)
    print(f"relative error of the posterior mean {em:.3e}, of the posterior variance {ev:.3e}")
    assert em <= ANALYTIC_TOL and ev <= ANALYTIC_TOL
    assert A.bits_equal(one["hx"][0], q1)
    other = np.ones(held[0].shape, dtype=bool)
    other[31 - b.bnd_x1, 7 - b.bnd_y1] = False
    assert all(A.bits_equal(a[other], c[other]) for a, c in zip(held, now))


# ---------------------------------------------------------------- 7. non-finite values
def test_nonfinite(amd):
    """A NaN in one member's ssh at an observed point: counted.  The same call on a fresh ensemble with that
    member left out by `use`: no count, and bitwise the restatement."""
    shape, classes = S.Shape(61, 9), ["noise"] * 6
    ij = OBS_61x9
    taper = A.taper_table(6.0)
    counts, bads = [], []
    for members in (None, [0, 1, 2, 4, 5]):
        e = _start(amd, shape, classes)
        try:
            _run(e, [2, 3])
            b = e.members[0].blocks[0]
            a = e.members[3].download(0, "ssh")
            a[30 - b.bnd_x1, 6 - b.bnd_y1] = np.nan
            e.members[3].upload(0, "ssh", a)
            clean = e.sample("ssh", _points(e, ij), members=[0, 1, 2, 4, 5])
            values, variances = _obs_values(clean, 7)
            bad, _, got, _ = _assim_vs_restatement(e, "ssh", ij, taper, ("ssh", "ubrtr"), members, values=values,
                                                   variances=variances)
        finally:
            e.close()
        counts.append(got["nonfinite"])
        bads.append(bad)
    assert counts[0] >= 1 and counts[1] == 0, counts
    assert not bads[0] and not bads[1], bads   # (the NaN propagates as the restatement says, too)


# ---------------------------------------------------------------- 8. errors change nothing
def test_errors_change_nothing(amd):
    """Every OCN_ERR_ARG case of the contract: nothing launched, the pending tails still pending, every member
    still its oracle run; the result entries before any successful call."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        ssh, lu, ff1, ub = (_lib.FIELD_ID[nm] for nm in ("ssh", "lu", "ff1_1", "ubrtr"))
        i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        val, var = np.array([0.1, -0.2]), np.array([0.01, 0.02])
        big_i = np.full(8193, 5, dtype=np.int32)
        big = np.ones(8193)
        taper, long_taper = np.array([1.0, 0.5, 0.25]), np.ones(65537)
        keep = [val, var, big_i, big, taper, long_taper]

        def changed(a, at, v):
            a = a.copy()
            a[at] = v
            keep.append(a)
            return ptr(a)
        ok = dict(ens=e.ens, of=ssh, ids=i32(ssh), nf=1, use=None, nobs=2, io=i32(5, 9), jo=i32(4, 6), v=ptr(val), r=ptr(var),
                  t=ptr(taper), nt=3)
        cases = {"null ensemble": dict(ens=None), "null list": dict(ids=None), "null io": dict(io=None), "null jo": dict(jo=None),
                 "null value": dict(v=None), "null variance": dict(r=None), "null taper": dict(t=None), "nfields 0": dict(nf=0),
                 "real(4) id": dict(ids=i32(ssh, lu), nf=2), "absent id": dict(ids=i32(ff1)),
                 "repeated id": dict(ids=i32(ssh, ub, ssh), nf=3), "real(4) obs_field": dict(of=lu), "absent obs_field": dict(of=ff1),
                 "one member": dict(use=(C.c_uint8 * 3)(0, 1, 0)), "no member": dict(use=(C.c_uint8 * 3)(0, 0, 0)),
                 "nobs 0": dict(nobs=0), "nobs 8193": dict(nobs=8193, io=ptr(big_i), jo=ptr(big_i), v=ptr(big), r=ptr(big)),
                 "io 0": dict(io=i32(5, 0)), "io nx + 1": dict(io=i32(66, 9)), "jo 0": dict(jo=i32(0, 6)),
                 "jo ny + 1": dict(jo=i32(4, 14)), "ntaper 0": dict(nt=0), "ntaper 65537": dict(t=ptr(long_taper), nt=65537)}
        for v in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
            cases[f"variance {v}"] = dict(r=changed(var, 1, v))
        for v in (np.nan, np.inf, -np.inf):
            cases[f"value {v}"] = dict(v=changed(val, 1, v))
            cases[f"{v} in taper"] = dict(t=changed(taper, 2, v))
        info = _lib.OcnEnsAssimInfo()
        out = np.zeros(64)
        l0 = _lib.launch_count()
        assert L.ocn_ens_assimilate_info(e.ens, C.byref(info)) == ERR_ARG
        for what in range(7):
            assert L.ocn_ens_assimilate_result(e.ens, what, ptr(out)) == ERR_ARG
        for what, change in cases.items():
            a = {**ok, **change}
            rc = L.ocn_ens_assimilate(a["ens"], a["of"], a["ids"], a["nf"], a["use"], a["nobs"], a["io"], a["jo"], a["v"], a["r"],
                                      a["t"], a["nt"])
            assert rc == ERR_ARG, what
        assert L.ocn_ens_assimilate_result(e.ens, 0, ptr(out)) == ERR_ARG     # still no successful call
        with pytest.raises(amd.OcnError) as ei:
            e.assimilate("ssh", np.array([[5, 4], [66, 6]]), val, var, taper, device=True)
        assert ei.value.code == ERR_ARG
        with pytest.raises(TypeError):
            e.assimilate("ssh", np.array([[5.0, 4.0]]), val[:1], var[:1], taper, device=True)
        with pytest.raises(ValueError):
            e.assimilate("ssh", np.array([[5, 4], [9, 6]]), val[:1], var, taper, device=True)
        assert _lib.launch_count() == l0
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
        # after a successful call: an unknown `what` and a null host array
        e.assimilate("ssh", np.array([[5, 4], [9, 6]]), val, var, taper, names=("ssh",), device=True)
        assert L.ocn_ens_assimilate_result(e.ens, 6, ptr(out)) == ERR_ARG      # (SPANS: the call was not timed)
        assert L.ocn_ens_assimilate_result(e.ens, 7, ptr(out)) == ERR_ARG
        assert L.ocn_ens_assimilate_result(e.ens, -1, ptr(out)) == ERR_ARG
        assert L.ocn_ens_assimilate_result(e.ens, 0, None) == ERR_ARG
        assert L.ocn_ens_assimilate_info(e.ens, C.byref(info)) == OK and (info.nobs, info.n) == (2, 3)
        del keep
    finally:
        e.close()
    assert pending == [True] * 3, pending
    assert st == [OK] * 3 and not bad, (st, bad)


def test_observation_in_a_dropped_block(amd):
    """S.DROPPED's missing middle block: (20, 20) is in the basin and in no local block's array -- OCN_ERR_ARG,
    nothing launched, no bit changed; without it the call goes through."""
    from ocean_model_arch_amd import _lib
    e = _start(amd, S.DROPPED, ["noise"] * 3)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 3
        taper = A.ringed_taper(10, 5)
        before = {b.k: _downloads(e, ("ssh",), range(3), b.k) for b in e.members[0].blocks}
        l0 = _lib.launch_count()
        with pytest.raises(amd.OcnError) as ei:
            e.assimilate("ssh", np.array([[38, 38], [20, 20]]), [0.1, 0.1], [0.01, 0.01], taper, names=("ssh",), device=True)
        none = _lib.launch_count() - l0
        after = {b.k: _downloads(e, ("ssh",), range(3), b.k) for b in e.members[0].blocks}
        bad, launches, _, _ = _assim_vs_restatement(e, "ssh", np.array([[38, 38]]), taper, ("ssh",), seed=9)
    finally:
        e.close()
    assert ei.value.code == ERR_ARG and none == 0
    assert all(A.bits_equal(a, c) for k in before for a, c in zip(before[k]["ssh"], after[k]["ssh"]))
    assert not bad and launches == 1 + STAGE_LAUNCHES, (bad, launches)
