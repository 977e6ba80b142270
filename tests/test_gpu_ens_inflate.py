"""GPU tests of the per-point covariance inflation (ocn_ens_spread_save, ocn_ens_inflate,
ocn_ens_inflate_download; ens_inflate.hip k_ens_inflate) and of OceanEnsemble.spread_save, inflate, inflation
and assimilate(rtps=...).

The reference is the numpy restatement of the contract (tests/ens_inflate_ref.py, itself checked against a
scalar loop by tests/test_ens_inflate_cpu.py), applied to the members' own downloads or to the CPU oracle's
fields; shapes, inputs and helpers are those of tests/test_gpu_ens_local.py.  Every comparison is bitwise on
whole block arrays (halo and land included; NaN by position).  Tolerance: none.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ens_inflate_ref as R
from tests import ens_local_ref as LR
from tests import shapes as S
from tests.test_gpu_ens_assim import _obs_values
from tests.test_gpu_ens_local import OBS_61x9, _oracle_update
from tests.test_gpu_ens_transform import _bad_vs, _downloads, _oracles, _pending, _run
from tests.test_gpu_ensemble import _bad, _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE = 0, 1, 4


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _idx(e, members):
    return list(range(len(e))) if members is None else sorted(set(members))


def _save_vs_downloads(e, names, members=None):
    """spread_save() against the restatement's spread over the members' own downloads, on every block: what
    differs, the launches of the call and the saved spreads {block: {field: array}}."""
    from ocean_model_arch_amd import _lib
    idx = _idx(e, members)
    blocks = e.members[0].blocks
    before = {b.k: _downloads(e, names, idx, b.k) for b in blocks}
    l0 = _lib.launch_count()
    e.spread_save(names, members=members)
    launches = _lib.launch_count() - l0
    sb = {b.k: {nm: e.inflation(nm, "prior_spread", b.k) for nm in names} for b in blocks}
    bad = [f"prior spread [{b.k}]:{nm}" for b in blocks for nm in names
           if not R.bits_equal(sb[b.k][nm], R.spread(before[b.k][nm]))]
    return bad, launches, sb


def _inflate_vs_downloads(e, alpha, mode, names, sb, members=None):
    """inflate() against the restatement over the members' own downloads and the saved spreads `sb`, on every
    block: the (member, block, field) and the factors that differ, the launches of the call, and the downloads
    before and after."""
    from ocean_model_arch_amd import _lib
    idx = _idx(e, members)
    blocks = e.members[0].blocks
    before = {b.k: _downloads(e, names, idx, b.k) for b in blocks}
    l0 = _lib.launch_count()
    e.inflate(alpha, mode, names, members=members)
    launches = _lib.launch_count() - l0
    bad, after = [], {}
    for b in blocks:
        after[b.k] = _downloads(e, names, idx, b.k)
        for nm in names:
            want, fac = R.inflate_rule(before[b.k][nm], sb[b.k][nm], mode, alpha)
            bad += [f"member {i} [{b.k}]:{nm}" for i, g, v in zip(idx, after[b.k][nm], want) if not R.bits_equal(g, v)]
            if not R.bits_equal(e.inflation(nm, "factor", b.k), fac):
                bad.append(f"factor [{b.k}]:{nm}")
    return bad, launches, before, after


def _same_state(a, b):
    return all(R.bits_equal(x, y) for k in a for nm in a[k] for x, y in zip(a[k][nm], b[k][nm]))


# ---------------------------------------------------------------- 1. the rule, by member count
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
    """n members in use: below, at and above the groups of 8, the register path's last count (32) and the
    re-reading path's first (33).  spread_save, a local_update that changes the spread, then RTPS with alpha
    0.7, CONST with 1.05 and RTPS with alpha 0, which must change nothing.  One launch per field and block for
    the save and for each inflation; the member not in use keeps its bits."""
    e = ens33
    names = ("ssh", "ubrtr")
    members = None if n == 33 else range(n)
    outside = None if n == 33 else e.members[32].download(0, "ssh")
    bad, launches, sb = _save_vs_downloads(e, names, members)
    assert not bad, bad
    assert launches == len(names)
    y, z = LR.rows(len(OBS_61x9), n, 100 * n)
    e.local_update(y, z, OBS_61x9, LR.ringed_taper(50, 1), names=names, members=members)
    for mode, alpha in (("rtps", 0.7), ("const", 1.05), ("rtps", 0.0)):
        bad, launches, before, after = _inflate_vs_downloads(e, alpha, mode, names, sb, members)
        assert not bad, (mode, alpha, bad)
        assert launches == len(names), (mode, alpha)
        assert _same_state(before, after) == (alpha == 0.0), (mode, alpha)
        fac = e.inflation("ssh", "factor")
        assert (fac == 1.0).all() == (alpha == 0.0), (mode, alpha)
    assert all(R.bits_equal(e.inflation(nm, "prior_spread"), sb[0][nm]) for nm in names)   # valid until the next save
    if outside is not None:
        assert R.bits_equal(e.members[32].download(0, "ssh"), outside)


# ---------------------------------------------------------------- 2. wave and workgroup edges
def test_wave_and_row_edges(amd):
    """Shape(121, 65), 8 members, a 125 x 69 array: with the 30-lane lead the waves change at array columns 34
    and 98, and 69 rows leave a last workgroup with one live row of four.  ssh is uploaded with values that
    differ at every point of the array, halo and outer rings included, so that every point on both sides of
    those edges is written."""
    shape = S.Shape(121, 65)
    e = _start(amd, shape, ["noise"] * 8)
    try:
        _run(e, [2, 3])
        e.complete()
        b = e.members[0].blocks[0]
        assert b.shape == (125, 69)
        rng = np.random.default_rng(125)
        for m in e.members:
            m.upload(0, "ssh", np.asfortranarray(rng.uniform(-1.0, 1.0, b.shape)))
        names = ("ssh", "vbrtrp")
        bad, _, sb = _save_vs_downloads(e, names)
        ij = np.array([[b.bnd_x1 + 33, 30], [b.bnd_x1 + 98, 40], [1, 1], [125, 69], [63, 35]])
        y, z = LR.rows(len(ij), 8, 901, scale=0.01)
        e.local_update(y, z, ij, LR.ringed_taper(125 * 125 + 69 * 69 + 7, 2), names=names)
        for mode, alpha in (("rtps", 0.7), ("const", 0.95)):
            more, launches, _, _ = _inflate_vs_downloads(e, alpha, mode, names, sb)
            bad += [f"{mode}: {x}" for x in more]
            assert launches == len(names)
            fac = e.inflation("ssh", "factor")
            assert (fac != 1.0).all(), mode       # every point of the array was written
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 3. a block grid and the upload rule
def _oracle_spread(oms, names, members=None):
    idx = range(len(oms)) if members is None else sorted(set(members))
    return {k: {nm: R.spread([oms[i].f[k][nm] for i in idx]) for nm in names} for k in range(len(oms[0].blocks))}


def _oracle_inflate(oms, sb, mode, alpha, names, members=None):
    """The restatement applied to fields `names` of every block of the oracle models `members` (None: all)."""
    idx = range(len(oms)) if members is None else sorted(set(members))
    for k in range(len(oms[0].blocks)):
        for nm in names:
            new, _ = R.inflate_rule([oms[i].f[k][nm] for i in idx], sb[k][nm], mode, alpha)
            for i, a in zip(idx, new):
                oms[i].f[k][nm][...] = a


def test_block_grid(amd):
    """A 2 x 2 block grid, 5 members: the save, a local update and the relaxation on every block against the
    restatement per block; then 2 more steps on the device and on the oracle, which took the same three
    operations on its own fields: every field of every member agrees bitwise (the upload rule)."""
    shape, classes, calls = S.Shape(17, 19, (2, 2)), ["noise"] * 5, [2, 3]
    names = R.STATE
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        blocks = e.members[0].blocks
        assert len(blocks) == 4
        sx, sy = max(b.nx_start for b in blocks), max(b.ny_start for b in blocks)
        ij = np.array([[3, 3], [19, 21], [sx - 1, sy], [sx, sy - 1], [1, 12], [21, 23], [sx + 2, 4], [5, sy + 1]])
        taper = LR.ringed_taper(21 * 21 + 23 * 23 + 1, 4)
        y, z = LR.rows(len(ij), 5, 34, scale=0.02)
        bad, launches, sb = _save_vs_downloads(e, names)
        e.local_update(y, z, ij, taper, names=names)
        more, launches2, before, after = _inflate_vs_downloads(e, 0.7, "rtps", names, sb)
        e.step(2)
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        osb = _oracle_spread(oms, names)
        _oracle_update(oms, y, z, ij, taper, names)
        _oracle_inflate(oms, osb, "rtps", 0.7, names)
        for om in oms:
            om.run(2, 1.0)
        late = _bad_vs(e, oms)
    finally:
        e.close()
    assert not bad and not more, (bad, more)
    assert launches == launches2 == len(names) * 4
    assert not _same_state(before, after)
    assert st == [OK] * 5 and not late, (st, late)


# ---------------------------------------------------------------- 4. pending tails, a subset
def test_pending_tails(amd):
    """9 members after calls [2, 5] with no complete(): the tails pending, the pair roles swapped.  spread_save
    and inflate over all members but one form the tails of the members in use only; the saved spread, the
    factor and every field of every member are the oracle's, which ran 7 steps and took the same operations."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 9, [2, 5]
    use = [0, 1, 2, 3, 5, 6, 7, 8]
    names = R.STATE
    y, z = LR.rows(len(OBS_61x9), 8, 71, scale=0.05)
    taper = LR.taper_table(6.0)
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 9
        e.spread_save(names, members=use)
        pending = _pending(e)
        e.local_update(y, z, OBS_61x9, taper, names=names, members=use)
        e.inflate(0.7, "rtps", names, members=use)
        pending2 = _pending(e)
        got_sb = {nm: e.inflation(nm, "prior_spread") for nm in names}
        got_fac = {nm: e.inflation(nm, "factor") for nm in names}
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        osb = _oracle_spread(oms, names, use)
        _oracle_update(oms, y, z, OBS_61x9, taper, names, members=use)
        fac = {nm: R.inflate_rule([oms[i].f[0][nm] for i in use], osb[0][nm], "rtps", 0.7)[1] for nm in names}
        _oracle_inflate(oms, osb, "rtps", 0.7, names, members=use)
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert pending == pending2 == [i == 4 for i in range(9)], (pending, pending2)
    assert all(R.bits_equal(got_sb[nm], osb[0][nm]) for nm in names)
    assert all(R.bits_equal(got_fac[nm], fac[nm]) for nm in names)
    assert st == [OK] * 9 and not bad, (st, bad)


# ---------------------------------------------------------------- 5. special values
def test_special_values(amd):
    """A masked shape, 4 members.  Member 1 holds NaN at a few points (one already when the spread is saved, two
    only afterwards): those points keep every member's bits and get factor 1.0, and no other member gets a
    NaN.  Land points, where every member holds the same value, are not written.  A column that is -0.0 in
    every member keeps its signs; one that is -0.0 in member 0 alone goes through the rule."""
    shape = S.Shape(61, 33, mask="rough")
    e = _start(amd, shape, ["noise"] * 4)
    try:
        _run(e, [2, 3])
        e.complete()
        b = e.members[0].blocks[0]
        mask = S.mask_of(shape)
        land = np.zeros(b.shape, dtype=bool)
        for i in range(b.nx_start, b.nx_end + 1):
            for j in range(b.ny_start, b.ny_end + 1):
                land[i - b.bnd_x1, j - b.bnd_y1] = mask[i - 1, j - 1] != 0
        assert land.any() and not land.all()
        x = [m.download(0, "ssh") for m in e.members]
        for a in x:
            a[land] = x[0][land]                # land: the same bits in every member
            a[20, :] = -0.0
        x[0][30, :] = -0.0
        x[1][3, 2] = np.nan
        for m, a in zip(e.members, x):
            m.upload(0, "ssh", a)
        bad, _, sb = _save_vs_downloads(e, ("ssh",))
        assert np.isnan(sb[0]["ssh"][3, 2])
        with np.errstate(all="ignore"):
            mean = (x[0] + x[2] + x[3]) / 3.0
            held = [np.asfortranarray(np.where(land, a, mean + 0.5 * (a - mean))) for a in x]
        for a in held:
            a[20, :] = -0.0
        held[1][3, 2], held[1][10, 5], held[1][40, 7] = np.nan, np.nan, np.inf
        for m, a in zip(e.members, held):
            m.upload(0, "ssh", a)
        more, _, before, after = _inflate_vs_downloads(e, 1.0, "rtps", ("ssh",), sb)
        fac = e.inflation("ssh", "factor")
        now = after[0]["ssh"]
    finally:
        e.close()
    assert not bad and not more, (bad, more)
    assert all(R.bits_equal(a, h) for a, h in zip(before[0]["ssh"], held))      # (the premise: uploads come back)
    for at in ((3, 2), (10, 5), (40, 7)):
        assert fac[at] == 1.0 and all(R.bits_equal(a[at], h[at]) for a, h in zip(now, held)), at
    assert all(np.isfinite(now[i]).all() for i in (0, 2, 3))
    assert (fac[land] == 1.0).all() and all(R.bits_equal(a[land], h[land]) for a, h in zip(now, held))
    assert (fac[20, :] == 1.0).all() and all(np.signbit(a[20, :]).all() for a in now)
    sea = ~land
    sea[20, :] = False
    interior = np.zeros(b.shape, dtype=bool)
    interior[b.nx_start - b.bnd_x1:b.nx_end - b.bnd_x1 + 1, b.ny_start - b.bnd_y1:b.ny_end - b.bnd_y1 + 1] = True
    wrote = sea & interior & np.isfinite(held[1])
    assert (fac[wrote] > 1.0).mean() > 0.9      # the relaxation undid the halving on the sea
    assert (fac[30, :] != 1.0).any()


# ---------------------------------------------------------------- 6. the cycle
def test_cycle(amd):
    """8 members.  assimilate(device=True, rtps=0.8) on one ensemble equals spread_save, assimilate(device=True),
    inflate(0.8) on its twin, bit for bit, fields and returned arrays; the returned hx describes the analysis
    before the relaxation; and rtps=None is the plain assimilate(device=True)."""
    from ocean_model_arch_amd import _lib
    shape, classes = S.Shape(61, 9), ["noise"] * 8
    ij = OBS_61x9
    taper = LR.taper_table(6.0)
    pts = [(0, int(i), int(j)) for i, j in ij]
    twins = [_start(amd, shape, classes) for _ in range(3)]
    try:
        for e in twins:
            _run(e, [2, 3])
            e.complete()
            assert e.synchronize() == [OK] * 8
        a, b, c = twins
        values, variances = _obs_values(a.sample("ssh", pts), 6)
        l0 = _lib.launch_count()
        info_a = a.assimilate("ssh", ij, values, variances, taper, device=True, rtps=0.8)
        launches = _lib.launch_count() - l0
        b.spread_save()
        info_b = b.assimilate("ssh", ij, values, variances, taper, device=True)
        mid_b = {0: _downloads(b, R.STATE, range(8))}
        b.inflate(0.8, "rtps")
        info_c = c.assimilate("ssh", ij, values, variances, taper, device=True, rtps=None)
        after = [{0: _downloads(e, R.STATE, range(8))} for e in twins]
        relaxed = a.sample("ssh", pts)
        fac = a.inflation("ssh", "factor")
        facs_equal = all(R.bits_equal(a.inflation(nm, w), b.inflation(nm, w)) for nm in R.STATE for w in ("factor", "prior_spread"))
    finally:
        for e in twins:
            e.close()
    assert launches == 6 + (1 + 6) + 6, launches          # the save, the analysis' stage and update, the inflation
    assert _same_state(after[0], after[1]) and facs_equal
    assert _same_state(after[2], mid_b) and not _same_state(after[0], mid_b)
    assert set(info_a) == set(info_b) == set(info_c)
    for key in info_b:
        assert R.bits_equal(info_a[key], info_b[key]) and R.bits_equal(info_c[key], info_b[key]), key
    assert not R.bits_equal(relaxed, info_a["hx"])        # hx: the analysis before the relaxation
    assert (fac != 1.0).any()


# ---------------------------------------------------------------- 7. errors change nothing
def test_errors_change_nothing(amd):
    """Every OCN_ERR_ARG and OCN_ERR_STATE case of the three entries: nothing launched, info() as it was, the
    pending tails still pending, the saved buffers as they were, and every member still its oracle run."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        ssh, lu, ff1, ub = (_lib.FIELD_ID[nm] for nm in ("ssh", "lu", "ff1_1", "ubrtr"))
        i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
        one_only, none, two = (C.c_uint8 * 3)(0, 1, 0), (C.c_uint8 * 3)(0, 0, 0), (C.c_uint8 * 3)(1, 1, 0)
        host = np.full(e.members[0].blocks[0].shape, -7.0, order="F")
        hp = host.ctypes.data_as(C.c_void_p)
        info0 = e.info()
        lists = {"null ensemble": dict(ens=None), "null list": dict(ids=None), "nfields 0": dict(nf=0),
                 "real(4) id": dict(ids=i32(ssh, lu), nf=2), "absent id": dict(ids=i32(ff1)),
                 "repeated id": dict(ids=i32(ssh, ub, ssh), nf=3), "one member": dict(use=one_only), "no member": dict(use=none)}
        ok = dict(ens=e.ens, ids=i32(ssh), nf=1, use=None, mode=0, alpha=1.1)
        inflate = dict(lists)
        inflate.update({"mode 2": dict(mode=2), "mode -1": dict(mode=-1), "alpha NaN": dict(alpha=np.nan),
                        "alpha Inf": dict(alpha=np.inf), "alpha -Inf": dict(mode=1, alpha=-np.inf),
                        "RTPS alpha < 0": dict(mode=1, alpha=-0.1)})
        l0 = _lib.launch_count()
        for what, change in lists.items():
            a = {**ok, **change}
            assert L.ocn_ens_spread_save(a["ens"], a["ids"], a["nf"], a["use"]) == ERR_ARG, what
            assert e.info() == info0, what
        for what, change in inflate.items():
            a = {**ok, **change}
            assert L.ocn_ens_inflate(a["ens"], a["ids"], a["nf"], a["use"], a["mode"], a["alpha"]) == ERR_ARG, what
            assert e.info() == info0, what
        down = {"null ensemble": (None, 0, ssh, 1, hp), "null host": (e.ens, 0, ssh, 1, None), "k -1": (e.ens, -1, ssh, 1, hp),
                "k 1": (e.ens, 1, ssh, 1, hp), "real(4) field": (e.ens, 0, lu, 1, hp), "absent field": (e.ens, 0, ff1, 1, hp),
                "what 2": (e.ens, 0, ssh, 2, hp), "what -1": (e.ens, 0, ssh, -1, hp)}
        for what, args in down.items():
            assert L.ocn_ens_inflate_download(*args) == ERR_ARG, what
        # nothing saved, nothing formed yet
        assert L.ocn_ens_inflate(e.ens, i32(ssh), 1, None, 1, 0.5) == ERR_STATE
        for w in (0, 1):
            assert L.ocn_ens_inflate_download(e.ens, 0, ssh, w, hp) == ERR_STATE, w
        assert (host == -7.0).all()
        # the wrappers check before the call
        for args, exc in ((("0.5",), TypeError), ((np.array([0.5, 0.5]),), TypeError), ((np.nan,), ValueError),
                          ((-0.5, "rtps"), ValueError), ((1.0, "both"), ValueError)):
            with pytest.raises(exc):
                e.inflate(*args)
        with pytest.raises(ValueError):
            e.inflation("ssh", "spread")
        with pytest.raises(ValueError):
            e.assimilate("ssh", OBS_61x9[:2], [0.0, 0.0], [1.0, 1.0], np.array([1.0]), device=True, rtps=-0.5)
        with pytest.raises(amd.OcnError) as ei:
            e.spread_save(("ssh", "ssh"))
        assert ei.value.code == ERR_ARG
        with pytest.raises(amd.OcnError) as ei:
            e.inflate(0.5, "rtps", ("ssh",))
        assert ei.value.code == ERR_STATE
        assert _lib.launch_count() == l0
        pending = _pending(e)
        # a save over members 0 and 1 (it forms their tails): RTPS over any other set, or on another field, is refused
        e.spread_save(("ssh",), members=[0, 1])
        saved = e.inflation("ssh", "prior_spread")
        pending2 = _pending(e)
        l1 = _lib.launch_count()
        for what, (ids, use) in {"all members": (i32(ssh), None), "members 0 and 2": (i32(ssh), (C.c_uint8 * 3)(1, 0, 1)),
                                 "a field not saved": (i32(ub), two), "one of two not saved": (i32(ssh, ub), two)}.items():
            assert L.ocn_ens_inflate(e.ens, ids, len(ids), use, 1, 0.5) == ERR_STATE, what
            assert e.info() == info0, what
        assert L.ocn_ens_inflate_download(e.ens, 0, ssh, 1, hp) == ERR_STATE       # no factor yet
        assert L.ocn_ens_inflate_download(e.ens, 0, ub, 0, hp) == ERR_STATE
        assert L.ocn_ens_spread_save(e.ens, i32(ssh, lu), 2, None) == ERR_ARG      # a refused save keeps the earlier one
        assert _lib.launch_count() == l1 and (host == -7.0).all()
        pending3 = _pending(e)
        assert R.bits_equal(e.inflation("ssh", "prior_spread"), saved)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert pending == [True] * 3, pending
    assert pending2 == pending3 == [False, False, True], (pending2, pending3)
    assert st == [OK] * 3 and not bad, (st, bad)
