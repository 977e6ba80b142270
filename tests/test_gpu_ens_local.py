"""GPU tests of the localized observation update (ocn_ens_local_update; ens_local.hip k_ens_local) and of
the serial filter built on it (OceanEnsemble.local_update, assimilate).

The reference is the numpy restatement of the contract (tests/ens_local_ref.py, itself checked against a
scalar triple loop by tests/test_ens_local_cpu.py), applied to the members' own downloads or to the CPU
oracle's fields; inputs and per-member oracle runs come from tests/shapes.py as tests/test_gpu_ensemble.py
builds them.  Every comparison is bitwise on whole block arrays (halo and land included; NaN by position).
Tolerance: none, but for the scalar Kalman update of the last test (1e-12, tests/test_ens_local_cpu.py).
"""
import ctypes as C

import numpy as np
import pytest

from tests import ens_local_ref as R
from tests import shapes as S
from tests.test_ens_local_cpu import ANALYTIC_TOL, ANALYTIC_VALUE, ANALYTIC_VAR, analytic_check
from tests.test_gpu_ens_transform import _bad_vs, _downloads, _oracles, _pending, _run
from tests.test_gpu_ensemble import _bad, _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, 1


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _update_vs_downloads(e, y, z, ij, taper, names, members=None, before=None):
    """local_update() against the restatement over the members' own downloads, on every block: the
    (member, block, field) that differ, and the downloads afterwards (the next call's `before`)."""
    idx = list(range(len(e))) if members is None else sorted(set(members))
    blocks = e.members[0].blocks
    if before is None:
        before = {b.k: _downloads(e, names, idx, b.k) for b in blocks}
    e.local_update(y, z, ij, taper, names=names, members=members)
    bad, after = [], {}
    for b in blocks:
        after[b.k] = _downloads(e, names, idx, b.k)
        for nm in names:
            want = R.block_update(before[b.k][nm], b, ij[:, 0], ij[:, 1], y, z, taper)
            bad += [f"member {i} [{b.k}]:{nm}" for i, g, v in zip(idx, after[b.k][nm], want) if not R.bits_equal(g, v)]
    return bad, after


def _changed(before, after):
    return any(not R.bits_equal(a, b) for k in before for nm in before[k] for a, b in zip(before[k][nm], after[k][nm]))


# ---------------------------------------------------------------- 1. the rule, by member count and taper
@pytest.fixture(scope="module")
def ens33(amd):
    """33 members of Shape(61, 9), class noise, after calls [2, 3], complete."""
    shape, classes = S.Shape(61, 9), ["noise"] * 33
    e = _start(amd, shape, classes)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 33
        yield e
    finally:
        e.close()


# Shape(61, 9): the one block's array is the whole 65 x 13 basin, global (1..65, 1..13).  A corner of the
# array, the halo ring, two at one point, the array's last point, and points spread over the interior.
# (An observation in the basin but beyond every array's reach needs a dropped block: test_dropped_block.)
OBS_61x9 = np.array([[1, 1], [2, 7], [30, 6], [30, 6], [65, 13], [12, 3], [33, 11], [47, 5], [58, 9], [35, 7], [64, 2]])


def _tapers(w, h):
    """(what, table): a zero ring inside the support; one entry; more entries than w^2 + h^2, so that every
    observation reaches every point; and all zeros, which must form and store nothing."""
    return [("ring", R.ringed_taper(50, 1)), ("one entry", np.array([0.75])),
            ("all points", R.ringed_taper(w * w + h * h + 7, 2)), ("all zero", np.array([0.0, -0.0] * 15))]


@pytest.mark.parametrize("n", [2, 5, 8, 9, 32, 33])
def test_member_counts(amd, ens33, n):
    """n members in use: below, at and above the groups of 8, the register path's last count (32) and the
    LDS path's first (33), one observation list down both.  Four tapers in turn.  One launch per field and
    block; the members not in use keep their bits."""
    from ocean_model_arch_amd import _lib
    e = ens33
    names = ("ssh", "ubrtr")
    members = None if n == 33 else range(n)
    outside = None if n == 33 else e.members[32].download(0, "ssh")
    ij = OBS_61x9
    before = None
    for t, (what, taper) in enumerate(_tapers(65, 13)):
        y, z = R.rows(len(ij), n, 100 * n + t, scale=0.02 if what == "all points" else 0.25)
        l0 = _lib.launch_count()
        bad, after = _update_vs_downloads(e, y, z, ij, taper, names, members, before)
        assert not bad, (what, bad)
        assert _lib.launch_count() - l0 == len(names), what
        if before is not None:
            assert _changed(before, after) == (what != "all zero"), what
        before = after
    if outside is not None:
        assert R.bits_equal(e.members[32].download(0, "ssh"), outside)


def test_wave_edges(amd):
    """Shape(121, 65), 8 members: with the 30-lane lead the waves change at array columns 34 and 98, and the
    observations sit on both sides of both, on the first and last rows and in the corners, so that a
    taper's reach crosses wave edges in x and workgroup rows in y."""
    shape = S.Shape(121, 65)
    e = _start(amd, shape, ["noise"] * 8)
    try:
        _run(e, [2, 3])
        b = e.members[0].blocks[0]
        assert b.shape == (125, 69)
        x = b.bnd_x1
        ij = np.array([[x + 33, 30], [x + 34, 31], [x + 35, 1], [x + 97, 69], [x + 98, 40], [x + 99, 12], [1, 1], [125, 69],
                       [1, 69], [125, 1], [x + 34, 31], [63, 35], [2, 20]])
        names = ("ssh", "vbrtrp")
        before = None
        for t, (what, taper) in enumerate(_tapers(125, 69)[:3]):
            y, z = R.rows(len(ij), 8, 900 + t, scale=0.01 if what == "all points" else 0.25)
            bad, before = _update_vs_downloads(e, y, z, ij, taper, names, None, before)
            assert not bad, (what, bad)
    finally:
        e.close()


# ---------------------------------------------------------------- 2. a block grid: global indices, halo coherence
def _ring_mismatches(e, names, idx):
    """The (field, member, block, other block) whose halo ring -- the points of the block's array one step
    outside its interior, the ring the exchanges fill; the ring beyond it is not exchanged -- does not hold
    the other block's interior bits where it lies in that interior.  Also the number of points compared."""
    blocks = e.members[0].blocks
    bad, count = [], 0
    for nm in names:
        for i in idx:
            arr = {b.k: e.members[i].download(b.k, nm) for b in blocks}
            for a in blocks:
                for o in blocks:
                    x1, x2 = max(a.nx_start - 1, o.nx_start), min(a.nx_end + 1, o.nx_end)
                    y1, y2 = max(a.ny_start - 1, o.ny_start), min(a.ny_end + 1, o.ny_end)
                    if a.k == o.k or x1 > x2 or y1 > y2:
                        continue
                    mine = arr[a.k][x1 - a.bnd_x1:x2 - a.bnd_x1 + 1, y1 - a.bnd_y1:y2 - a.bnd_y1 + 1]
                    theirs = arr[o.k][x1 - o.bnd_x1:x2 - o.bnd_x1 + 1, y1 - o.bnd_y1:y2 - o.bnd_y1 + 1]
                    count += mine.size
                    if not R.bits_equal(mine, theirs):
                        bad.append((nm, i, a.k, o.k))
    return bad, count


def test_block_grid(amd):
    """A 2 x 2 block grid, 5 members: every block against the restatement with global indices -- the
    observations sit in a corner block only (beyond the other blocks' reach: culled from their lists), on
    both sides of the seams, in the basin's outer ring and twice at one point -- and halo coherence: after
    complete() each block's halo ring holds its neighbours' interior bits (sides and corners), and it
    still does after the updates."""
    shape, classes = S.Shape(17, 19, (2, 2)), ["noise"] * 5
    names = ("ssh", "ubrtr")
    e = _start(amd, shape, classes)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 5
        blocks = e.members[0].blocks
        assert len(blocks) == 4
        sx = max(b.nx_start for b in blocks)   # the first interior column / row beyond the seams
        sy = max(b.ny_start for b in blocks)
        ij = np.array([[3, 3], [19, 21], [sx - 1, sy], [sx, sy - 1], [1, 12], [sx, sy - 1], [21, 23], [sx + 2, 4], [5, sy + 1]])
        was, count = _ring_mismatches(e, names, range(5))
        assert not was and count == 2 * 5 * 2 * (8 + 9 + 9 + 10 + 2), (was, count)   # (the premise)
        taper = R.ringed_taper(10, 3)          # reach 3: (3, 3) and (19, 21) meet one block each
        y, z = R.rows(len(ij), 5, 33)
        bad, _ = _update_vs_downloads(e, y, z, ij, taper, names)
        lost, _ = _ring_mismatches(e, names, range(5))
        wide = R.ringed_taper(21 * 21 + 23 * 23 + 1, 4)
        y2, z2 = R.rows(len(ij), 5, 34, scale=0.02)
        bad2, _ = _update_vs_downloads(e, y2, z2, ij, wide, names)
        lost2, _ = _ring_mismatches(e, names, range(5))
    finally:
        e.close()
    assert not bad and not bad2, (bad, bad2)
    assert not lost and not lost2, (lost, lost2)


def test_dropped_block(amd):
    """A 3 x 3 grid whose middle block is dropped: an observation in the middle of it, with a reach of 3, is
    in the basin but beyond every array's reach -- every list is empty, nothing is launched and no bit
    changes; with one more observation that reaches a block, that block alone is launched on."""
    from ocean_model_arch_amd import _lib
    shape = S.DROPPED
    e = _start(amd, shape, ["noise"] * 3)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 3
        blocks = e.members[0].blocks
        assert len(blocks) == 7
        mid = np.array([[20, 20]])
        assert not any(b.bnd_x1 - 3 <= 20 <= b.bnd_x2 + 3 and b.bnd_y1 - 3 <= 20 <= b.bnd_y2 + 3 for b in blocks)
        taper = R.ringed_taper(10, 5)
        y, z = R.rows(2, 3, 61)
        l0 = _lib.launch_count()
        bad, after = _update_vs_downloads(e, y[:1], z[:1], mid, taper, ("ssh",))
        none = _lib.launch_count() - l0
        both = np.array([[20, 20], [38, 38]])   # the second: the last block's corner
        l0 = _lib.launch_count()
        bad2, after2 = _update_vs_downloads(e, y, z, both, taper, ("ssh",), None, after)
        one = _lib.launch_count() - l0
    finally:
        e.close()
    assert not bad and not bad2, (bad, bad2)
    assert none == 0 and one == 1, (none, one)
    assert _changed(after, after2)


# ---------------------------------------------------------------- 3. pending tails and the upload rule
def _oracle_update(oms, y, z, ij, taper, names, members=None):
    """The restatement applied to fields `names` of every block of the oracle models `members` (None: all)."""
    idx = range(len(oms)) if members is None else sorted(set(members))
    for k, b in enumerate(oms[0].blocks):
        for nm in names:
            new = R.block_update([oms[i].f[k][nm] for i in idx], b, ij[:, 0], ij[:, 1], y, z, taper)
            for i, a in zip(idx, new):
                oms[i].f[k][nm][...] = a


def test_continue_as_the_oracle_continues(amd):
    """9 members after calls [2, 5]: the tails pending, the pair roles swapped (an odd total).
    local_update(STATE), then 4 more steps: every field of every member equals the oracle run 7 steps,
    updated by the restatement, run 4 steps more -- the tail formation, the buffers of a pair after a swap,
    and everything the upload bookkeeping has to drop."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 9, [2, 5]
    ij = OBS_61x9
    y, z = R.rows(len(ij), 9, 71, scale=0.05)
    taper = R.taper_table(6.0)
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 9
        e.local_update(y, z, ij, taper)
        e.step(4)
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        _oracle_update(oms, y, z, ij, taper, R.STATE)
        for om in oms:
            om.run(4, 1.0)
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert st == [OK] * 9 and not bad, (st, bad)


# ---------------------------------------------------------------- 4. a subset of the members
def test_member_not_in_use_is_not_touched(amd):
    """Members 0 and 2 are updated: their pending tails are formed, member 1's stays pending, and member 1
    is still its oracle run once completed; members 0 and 2 are the oracle's, updated."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 5]
    ij = OBS_61x9
    y, z = R.rows(len(ij), 2, 72)
    taper = R.ringed_taper(50, 6)
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 3
        e.local_update(y, z, ij, taper, members=[2, 0])
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        _oracle_update(oms, y, z, ij, taper, R.STATE, members=[0, 2])
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert pending == [False, True, False], pending
    assert st == [OK] * 3 and not bad, (st, bad)


# ---------------------------------------------------------------- 5. composition
def test_composition(amd, ens33):
    """One call with 40 observations against two calls of 17 and 23 from the same state: the same bits."""
    e = ens33
    idx = list(range(8))
    rng = np.random.default_rng(55)
    ij = np.stack([rng.integers(1, 66, 40), rng.integers(1, 14, 40)], axis=1)
    y, z = R.rows(40, 8, 56, scale=0.05)
    taper = R.ringed_taper(37, 7)
    start = [e.members[i].download(0, "ssh") for i in idx]
    e.local_update(y, z, ij, taper, names="ssh", members=idx)
    one = [e.members[i].download(0, "ssh") for i in idx]
    for i, a in zip(idx, start):
        e.members[i].upload(0, "ssh", a)
    e.local_update(y[:17], z[:17], ij[:17], taper, names="ssh", members=idx)
    e.local_update(y[17:], z[17:], ij[17:], taper, names="ssh", members=idx)
    two = [e.members[i].download(0, "ssh") for i in idx]
    assert all(R.bits_equal(a, b) for a, b in zip(one, two))
    assert all(R.bits_equal(a, b) for a, b in zip(one, R.block_update(start, e.members[0].blocks[0], ij[:, 0], ij[:, 1], y, z, taper)))
    assert not all(R.bits_equal(a, b) for a, b in zip(one, start))


# ---------------------------------------------------------------- 6. the serial filter
def test_assimilate(amd):
    """Shape(61, 9), 8 members, 12 ssh observations with a radius of 6: sample() afterwards is the returned
    final HX bit for bit, the fields are the restatement's, the spread at the observed points shrinks; then
    one observation with taper [1.0] against the scalar Kalman update in extended precision."""
    shape = S.Shape(61, 9)
    e = _start(amd, shape, ["noise"] * 8)
    try:
        _run(e, [2, 3])
        rng = np.random.default_rng(12)
        ij = np.stack([rng.integers(3, 64, 12), rng.integers(3, 12, 12)], axis=1)
        ij[5] = ij[2]                                  # two observations of one point
        pts = [(0, int(i), int(j)) for i, j in ij]
        prior = e.sample("ssh", pts)
        values = prior.mean(axis=1) + rng.uniform(-0.1, 0.1, 12)
        variances = np.full(12, 0.01) + prior.var(axis=1, ddof=1) * 0.5
        taper = amd.ensemble.taper_table(6.0)
        before = _downloads(e, R.STATE, range(8))
        info = e.assimilate("ssh", ij, values, variances, taper)
        after = _downloads(e, R.STATE, range(8))
        got = e.sample("ssh", pts)
        Y, Z, ref = R.ensrf_obs_space(prior, ij, values, variances, taper)
        b = e.members[0].blocks[0]
        bad = [f"member {i}:{nm}" for nm in R.STATE
               for i, (g, v) in enumerate(zip(after[nm], R.block_update(before[nm], b, ij[:, 0], ij[:, 1], Y, Z, taper)))
               if not R.bits_equal(g, v)]
        # one observation, taper [1.0], on the O(1), well-spread values of the CPU test, uploaded as ssh: the
        # scalar Kalman update at the observed point, nothing anywhere else
        xs = np.random.default_rng(5).uniform(0.5, 1.5, (8,) + b.shape)
        for m, a in zip(e.members, xs):
            m.upload(0, "ssh", a)
        one = np.array([[31, 7]])
        p1 = e.sample("ssh", [(0, 31, 7)])[0]
        value, r = ANALYTIC_VALUE, ANALYTIC_VAR
        held = _downloads(e, ("ssh",), range(8))["ssh"]
        e.assimilate("ssh", one, [value], [r], np.array([1.0]), names=("ssh",))
        q1 = e.sample("ssh", [(0, 31, 7)])[0]
        now = _downloads(e, ("ssh",), range(8))["ssh"]
    finally:
        e.close()
    assert R.bits_equal(got, info["hx"]) and R.bits_equal(ref["hx"], info["hx"])
    assert not bad, bad
    assert set(info) == {"hx", "innovations", "prior_spread", "posterior_spread"}
    assert info["hx"].shape == (12, 8) and (info["posterior_spread"] < info["prior_spread"]).all()
    em, ev = analytic_check(p1, q1, value, r)
    print(f"relative error of the posterior mean {em:.3e}, of the posterior variance {ev:.3e} "
          f"(prior mean {p1.mean():.3e}, variance {p1.var(ddof=1):.3e})")
    assert em <= ANALYTIC_TOL and ev <= ANALYTIC_TOL
    assert R.bits_equal(p1, xs[:, 31 - b.bnd_x1, 7 - b.bnd_y1])
    other = np.ones(held[0].shape, dtype=bool)
    other[31 - b.bnd_x1, 7 - b.bnd_y1] = False
    assert all(R.bits_equal(a[other], c[other]) for a, c in zip(held, now))


# ---------------------------------------------------------------- 7. errors change nothing
def test_errors_change_nothing(amd):
    """Every OCN_ERR_ARG case of the contract: nothing launched, the pending tails still pending, and every
    member still its oracle run."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        ssh, lu, ff1, ub = (_lib.FIELD_ID[nm] for nm in ("ssh", "lu", "ff1_1", "ubrtr"))
        i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        y, z = R.rows(2, 3, 1)
        big_i, big_j = np.full(8193, 5, dtype=np.int32), np.full(8193, 5, dtype=np.int32)
        big = np.zeros((8193, 3))
        taper, long_taper = np.array([1.0, 0.5, 0.25]), np.ones(65537)
        io, jo = i32(5, 9), i32(4, 6)
        ids = i32(ssh)
        one_only = (C.c_uint8 * 3)(0, 1, 0)

        def bad_value(a, at, v):
            a = a.copy()
            a.flat[at] = v
            return a
        ok = dict(ens=e.ens, ids=ids, nf=1, use=None, nobs=2, io=io, jo=jo, y=ptr(y), z=ptr(z), t=ptr(taper), nt=3)
        keep = [y, z, taper, big, big_i, big_j, long_taper]
        cases = {"null ensemble": dict(ens=None), "null list": dict(ids=None), "null io": dict(io=None),
                 "null jo": dict(jo=None), "null y": dict(y=None), "null z": dict(z=None), "null taper": dict(t=None),
                 "nfields 0": dict(nf=0), "real(4) id": dict(ids=i32(ssh, lu), nf=2), "absent id": dict(ids=i32(ff1)),
                 "repeated id": dict(ids=i32(ssh, ub, ssh), nf=3), "one member": dict(use=one_only),
                 "no member": dict(use=(C.c_uint8 * 3)(0, 0, 0)), "nobs 0": dict(nobs=0),
                 "nobs 8193": dict(nobs=8193, io=ptr(big_i), jo=ptr(big_j), y=ptr(big), z=ptr(big)),
                 "io 0": dict(io=i32(5, 0)), "io nx + 1": dict(io=i32(66, 9)), "jo 0": dict(jo=i32(0, 6)),
                 "jo ny + 1": dict(jo=i32(4, 14)), "ntaper 0": dict(nt=0), "ntaper 65537": dict(t=ptr(long_taper), nt=65537)}
        for what, arr, key in (("y", y, "y"), ("z", z, "z"), ("taper", taper, "t")):
            for v in (np.nan, np.inf, -np.inf):
                a = bad_value(arr, arr.size - 1, v)
                keep.append(a)
                cases[f"{v} in {what}"] = {key: ptr(a)}
        l0 = _lib.launch_count()
        for what, change in cases.items():
            a = {**ok, **change}
            rc = L.ocn_ens_local_update(a["ens"], a["ids"], a["nf"], a["use"], a["nobs"], a["io"], a["jo"], a["y"], a["z"],
                                        a["t"], a["nt"])
            assert rc == ERR_ARG, what
        assert _lib.launch_count() == l0
        # the wrapper checks dtype, shape and finiteness before the call
        ij = np.array([[5, 4], [9, 6]])
        for args, exc in (((y.astype(np.float32), z, ij, taper), TypeError), ((y, z, ij, taper.astype(np.float32)), TypeError),
                          ((y, z, ij.astype(np.float64), taper), TypeError), ((y[:, :2], z, ij, taper), ValueError),
                          ((y, z[:1], ij, taper), ValueError), ((y, z, ij[:, :1], taper), ValueError),
                          ((y, z, ij, taper.reshape(1, 3)), ValueError), ((y, z, ij, np.zeros(0)), ValueError),
                          ((bad_value(y, 0, np.nan), z, ij, taper), ValueError), ((y, z, ij, bad_value(taper, 1, np.inf)), ValueError)):
            with pytest.raises(exc):
                e.local_update(*args)
        with pytest.raises(amd.OcnError) as ei:
            e.local_update(y, z, ij, taper, names=("ssh", "ssh"))
        assert ei.value.code == ERR_ARG
        with pytest.raises(amd.OcnError) as ei:
            e.local_update(y, z, np.array([[5, 4], [66, 6]]), taper)
        assert ei.value.code == ERR_ARG
        assert _lib.launch_count() == l0
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
        del keep
    finally:
        e.close()
    assert pending == [True] * 3, pending
    assert st == [OK] * 3 and not bad, (st, bad)
