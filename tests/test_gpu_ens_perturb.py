"""GPU tests of the correlated random perturbations (ocn_ens_perturb, ocn_ens_perturb_download;
ens_perturb.hip k_ens_noise, k_ens_perturb_apply) and of OceanEnsemble.perturb and perturbation.

The reference is the numpy restatement of the contract (tests/ens_perturb_ref.py, itself checked against
known answers and a scalar loop by tests/test_ens_perturb_cpu.py), applied to the members' own downloads or to
the CPU oracle's fields; shapes, inputs and helpers are those of the other ensemble tests.  Every comparison is
bitwise on whole block arrays (halo and land included; NaN by position).  Tolerance: none.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ens_perturb_ref as R
from tests import ens_stats_ref as SR
from tests import shapes as S
from tests.test_gpu_ens_transform import _bad_vs, _downloads, _oracles, _pending, _run
from tests.test_gpu_ensemble import _bad, _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE = 0, 1, 4


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _index_grids(b):
    return (np.arange(b.bnd_x1, b.bnd_x2 + 1, dtype=np.int64)[:, None],
            np.arange(b.bnd_y1, b.bnd_y2 + 1, dtype=np.int64)[None, :])


def _perturb_vs_downloads(e, idx, groups, **kw):
    """perturb(names=groups, members=idx, **kw) against the restatement over the members' own downloads, on
    every block: the (member, block, field) that differ, the launches of the call, the downloads before and
    after.  Completes the members in use (the downloads)."""
    from ocean_model_arch_amd import _lib
    names = R.flat(groups)
    blocks = e.members[0].blocks
    before = {b.k: _downloads(e, names, idx, b.k) for b in blocks}
    l0 = _lib.launch_count()
    e.perturb(names=groups, members=None if len(idx) == len(e) else idx, **kw)
    launches = _lib.launch_count() - l0
    after = {b.k: _downloads(e, names, idx, b.k) for b in blocks}
    want = R.expected(e, groups, idx, before=before, **kw)
    bad = [f"member {i} [{b.k}]:{nm}" for b in blocks for nm in names
           for i, g, v in zip(idx, after[b.k][nm], want[b.k][nm]) if not R.bits_equal(g, v)]
    return bad, launches, before, after


def _noise_vs_restatement(e, idx, seed, draw, reach, passes):
    """perturbation(a) of every member in use on every block against the restatement's Z."""
    bad = []
    for b in e.members[0].blocks:
        want = R.block_noise(b, idx, seed, draw, reach, passes)
        bad += [f"Z of member {i} [{b.k}]" for a, i in enumerate(idx) if not (e.perturbation(a, b.k) == want[a]).all()]
    return bad


def _same_state(a, b):
    return all(R.bits_equal(x, y) for k in a for nm in a[k] for x, y in zip(a[k][nm], b[k][nm]))


# ---------------------------------------------------------------- 1. the device's Philox
def test_device_philox(amd):
    """Shape(61, 9), 2 members, reach 0: Z is W, so perturbation(a) is the device's Philox at every point of
    the array for two seeds, one with a nonzero high word, and
    two draw ids; passes = 2 with reach = 0 is Z = W as well."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 2)
    bad = []
    try:
        b = e.members[0].blocks[0]
        i, j = _index_grids(b)
        for seed in (7, (0xC0FFEE11 << 32) | 0x80000001):
            for names, last_draw, passes in ((("ssh",), 3, 0), (("ssh", "ubrtr"), 4, 2)):
                e.perturb(1.0e-3, reach=0, passes=passes, names=names, seed=seed, draw=3, centre=False)
                for a in (0, 1):
                    z = e.perturbation(a)
                    assert z.dtype == np.int64 and z.shape == b.shape
                    if not (z == R.white(seed, last_draw, a, i, j)).all():
                        bad.append((hex(seed), last_draw, a))
        assert not (e.perturbation(0) == e.perturbation(1)).all()
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 2. the rule, by member count
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


@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 32, 33])
def test_member_counts(amd, ens33, n):
    """n members in use, members 1 .. n (member 0, whose masks apply, is not in use below 33, and a member's
    index is not its rank): one alone (no centring), below, at and above the groups of 8, and all.  ssh and
    sshp share a draw, ubrtr has the next: 2 noise launches and 3 applications.  Every member in use equals the
    restatement over its own download on every field; the member not in use keeps its bits."""
    e = ens33
    groups = (("ssh", "sshp"), "ubrtr")
    idx = list(range(33)) if n == 33 else list(range(1, n + 1))
    outside = None if n == 33 else {nm: e.members[0].download(0, nm) for nm in R.flat(groups)}
    kw = dict(amplitude=2.0e-3, reach=4, passes=2, seed=1000 + n, draw=n, centre=n >= 2)
    bad, launches, before, after = _perturb_vs_downloads(e, idx, groups, **kw)
    assert not bad, bad
    assert launches == 2 + 3
    assert not _same_state(before, after)
    assert not _noise_vs_restatement(e, idx, kw["seed"], n + 1, 4, 2)      # (the last draw id: ubrtr's)
    d_ssh = [a - b for a, b in zip(after[0]["ssh"], before[0]["ssh"])]
    d_sshp = [a - b for a, b in zip(after[0]["sshp"], before[0]["sshp"])]
    sea = e.members[0].download(0, "lu") > 0.5
    assert all(np.abs(a[sea] - b[sea]).max() < 1.0e-12 for a, b in zip(d_ssh, d_sshp))   # one draw (to rounding)
    if outside is not None:
        assert all(R.bits_equal(e.members[0].download(0, nm), a) for nm, a in outside.items())


# ---------------------------------------------------------------- 3. aprons beyond the array, tile and wave edges
@pytest.fixture(scope="module")
def ens8(amd):
    """8 members of Shape(121, 65) (a 125 x 69 array, lead 30), class noise, after calls [2, 3], complete."""
    e = _start(amd, S.Shape(121, 65), ["noise"] * 8)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 8
        yield e
    finally:
        e.close()


@pytest.mark.parametrize("reach, passes", [(16, 2), (8, 3), (1, 1), (16, 3)])
def test_aprons_and_tile_edges(amd, ens8, reach, passes):
    """A 125 x 69 array with the 30-lane lead: the 64-column tiles change at array columns 34 and 98, and 69
    rows are three 32-row tiles, the last of 5 rows.  Aprons of 32, 24 and 48 reach far beyond the array on
    every side, into negative indices, and across every tile edge; at 48 the apron's rows fill the column
    buffer.  No masks, so every point of the array is written; 8 members are within the exactness bound at
    R = 16, P = 3."""
    e = ens8
    assert e.members[0].blocks[0].shape == (125, 69)
    groups = ("ssh", "vbrtrp")
    masks = {nm: None for nm in groups}
    kw = dict(amplitude=0.5, reach=reach, passes=passes, seed=(reach << 40) | passes, draw=10, centre=True, masks=masks)
    bad, launches, before, after = _perturb_vs_downloads(e, list(range(8)), groups, **kw)
    assert not bad, bad
    assert launches == 2 + 2
    assert not _noise_vs_restatement(e, list(range(8)), kw["seed"], 11, reach, passes)
    assert all((a != b).mean() > 0.99 for nm in groups for a, b in zip(after[0][nm], before[0][nm]))


# ---------------------------------------------------------------- 4. decomposition independence
def _oracle_perturb(oms, idx, groups, seed, draw, reach, passes, centre, amplitude):
    """The restatement applied to the oracle models idx under the default masks (oracle model 0's)."""
    for k, b in enumerate(oms[0].blocks):
        for g, grp in enumerate(groups):
            for nm in ((grp,) if isinstance(grp, str) else grp):
                mname = R.default_mask(nm)
                new = R.perturb_rule([oms[i].f[k][nm] for i in idx], None if mname is None else oms[0].f[k][mname], b.bx1,
                                     b.by1, idx, seed, draw + g, reach, passes, centre, amplitude)
                for i, a in zip(idx, new):
                    oms[i].f[k][nm][...] = a


def test_decomposition_independence(amd):
    """One basin as 1 x 1 and as 2 x 2 blocks, 3 members, one call: Z at every point of every array of the
    2 x 2 ensemble, halo points included, is Z of the 1 x 1 ensemble at the same global indices, so a halo
    point gets what the owning block's interior gets; each block's fields equal the restatement over its own
    downloads.  Then 2 more steps on the 2 x 2 ensemble and on the oracle, which took the restatement on its
    own fields: every field of every member agrees bitwise (the upload rule)."""
    one, four = S.Shape(17, 19), S.Shape(17, 19, (2, 2))
    classes, calls = ["noise"] * 3, [2, 3]
    kw = dict(amplitude=1.0e-3, reach=4, passes=2, seed=(5 << 32) | 17, draw=2, centre=True)
    e1, e4 = _start(amd, one, classes), _start(amd, four, classes)
    try:
        for e in (e1, e4):
            _run(e, calls)
        idx = [0, 1, 2]
        bad1, _, _, _ = _perturb_vs_downloads(e1, idx, R.STATE_GROUPS, **kw)
        bad4, launches, before, after = _perturb_vs_downloads(e4, idx, R.STATE_GROUPS, **kw)
        b1 = e1.members[0].blocks[0]
        z1 = [e1.perturbation(a) for a in idx]
        halo = []
        for b in e4.members[0].blocks:
            assert b1.bnd_x1 <= b.bnd_x1 and b.bnd_x2 <= b1.bnd_x2 and b1.bnd_y1 <= b.bnd_y1 and b.bnd_y2 <= b1.bnd_y2
            for a in idx:
                want = z1[a][b.bnd_x1 - b1.bnd_x1:b.bnd_x2 - b1.bnd_x1 + 1, b.bnd_y1 - b1.bnd_y1:b.bnd_y2 - b1.bnd_y1 + 1]
                if not (e4.perturbation(a, b.k) == want).all():
                    halo.append((b.k, a))
        e4.step(2)
        e4.complete()
        st = e4.synchronize()
        oms = _oracles(four, classes, sum(calls))
        _oracle_perturb(oms, idx, R.STATE_GROUPS, kw["seed"], kw["draw"], 4, 2, True, kw["amplitude"])
        for om in oms:
            om.run(2, 1.0)
        late = _bad_vs(e4, oms)
    finally:
        e1.close()
        e4.close()
    assert len(e4.members[0].blocks) == 4
    assert not bad1 and not bad4 and not halo, (bad1, bad4, halo)
    assert launches == (3 + 6) * 4
    assert not _same_state(before, after)
    assert st == [OK] * 3 and not late, (st, late)


# ---------------------------------------------------------------- 5. masks and special values
def test_masks_and_special_values(amd):
    """A masked shape, 4 members, the default masks (ssh under lu, ubrtr under lcu, vbrtr under lcv).  Land of
    ssh, ubrtr and vbrtr holds -0.0 in every member and keeps its bits; a NaN and an Inf planted at sea points
    of member 1 stay what they are, and the other members are finite there and match the restatement."""
    shape = S.Shape(61, 33, mask="rough")
    e = _start(amd, shape, ["noise"] * 4)
    try:
        _run(e, [2, 3])
        e.complete()
        m0 = e.members[0]
        land = {nm: ~(m0.download(0, R.default_mask(nm)) > 0.5) for nm in ("ssh", "ubrtr", "vbrtr")}
        sea = np.argwhere(~land["ssh"])
        at_nan, at_inf = tuple(sea[len(sea) // 3]), tuple(sea[2 * len(sea) // 3])
        for i, m in enumerate(e.members):
            for nm in land:
                a = m.download(0, nm)
                a[land[nm]] = -0.0
                if i == 1 and nm == "ssh":
                    a[at_nan], a[at_inf] = np.nan, np.inf
                m.upload(0, nm, a)
        idx = [0, 1, 2, 3]
        bad, launches, before, after = _perturb_vs_downloads(e, idx, R.STATE_GROUPS, amplitude=1.0e-3, seed=99, draw=0)
    finally:
        e.close()
    assert not bad, bad
    assert launches == 3 + 6
    assert all(l.any() and not l.all() for l in land.values())
    for nm, l in land.items():
        for a in after[0][nm]:
            assert (a[l] == 0.0).all() and np.signbit(a[l]).all(), nm
    ssh = after[0]["ssh"]
    assert np.isnan(ssh[1][at_nan]) and np.isposinf(ssh[1][at_inf])
    assert all(np.isfinite(ssh[i]).all() for i in (0, 2, 3))
    assert (ssh[0][~land["ssh"]] != before[0]["ssh"][0][~land["ssh"]]).mean() > 0.99


def test_pending_tails_and_a_subset(amd):
    """9 members after calls [2, 5] with no complete(): the tails pending, the pair roles swapped.  perturb over
    all members but one forms the tails of the members in use only; every field of every member is the
    oracle's, which ran 7 steps and took the restatement with the members' indices 0..3, 5..8."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 9, [2, 5]
    use = [0, 1, 2, 3, 5, 6, 7, 8]
    kw = dict(seed=31, draw=5, reach=3, passes=1, centre=True, amplitude=1.0e-3)
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 9
        e.perturb(kw["amplitude"], reach=3, passes=1, seed=31, draw=5, members=use)
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        _oracle_perturb(oms, use, R.STATE_GROUPS, **kw)
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert pending == [i == 4 for i in range(9)], pending
    assert st == [OK] * 9 and not bad, (st, bad)


# ---------------------------------------------------------------- 6. reproducibility
def test_reproducibility_and_the_centred_mean(amd):
    """Twin ensembles given the same call agree bitwise; another draw id gives another field.  With centring the
    ensemble mean moves only by the rounding of the members' updates: stats(mean) afterwards is, bit for bit,
    the restatement's mean over the restatement's members (no tolerance of this test's own)."""
    shape, classes = S.Shape(61, 9), ["noise"] * 5
    idx = list(range(5))
    twins = [_start(amd, shape, classes) for _ in range(3)]
    try:
        for e in twins:
            _run(e, [2, 3])
            e.complete()
        a, b, c = twins
        before = {0: _downloads(a, R.flat(R.STATE_GROUPS), idx)}
        mean0 = a.stats("ssh", "mean")["mean"]
        for e, draw in ((a, 0), (b, 0), (c, 3)):
            e.perturb(1.0e-3, seed=77, draw=draw)
        after = [{0: _downloads(e, R.flat(R.STATE_GROUPS), idx)} for e in twins]
        mean1 = a.stats("ssh", "mean")["mean"]
        want = R.expected(a, R.STATE_GROUPS, idx, seed=77, draw=0, amplitude=1.0e-3, before=before)
    finally:
        for e in twins:
            e.close()
    assert _same_state(after[0], after[1]) and not _same_state(after[0], after[2])
    assert _same_state(after[0], want)
    assert R.bits_equal(mean1, SR.stats(want[0]["ssh"], ("mean",))["mean"])
    assert not R.bits_equal(mean1, mean0)                     # (rounding moves it ...)
    assert np.abs(mean1 - mean0).max() < 1.0e-6 * 1.0e-3      # (... and nothing else does: far below the amplitude)


# ---------------------------------------------------------------- 7. errors change nothing
def test_errors_change_nothing(amd):
    """Every OCN_ERR_ARG case of ocn_ens_perturb and ocn_ens_perturb_download and the OCN_ERR_STATE of a
    download before the first call: nothing launched, info() as it was, the pending tails still pending, and
    every member still its oracle run."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 14, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        ssh, lu, ff1, ub = (_lib.FIELD_ID[nm] for nm in ("ssh", "lu", "ff1_1", "ubrtr"))
        i32 = lambda *v: (C.c_int32 * len(v))(*v)     # noqa: E731
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)    # noqa: E731
        use = lambda *v: (C.c_uint8 * 14)(*v)         # noqa: E731
        host = np.full(e.members[0].blocks[0].shape, -7, dtype=np.int64, order="F")
        hp = host.ctypes.data_as(C.c_void_p)
        info0 = e.info()
        ok = dict(ens=e.ens, ids=i32(ssh), masks=i32(lu), draw=u32(0), nf=1, use=use(1, 1, 1), seed=1, reach=4, passes=2,
                  centre=1, amp=1.0e-3)
        cases = {"null ensemble": dict(ens=None), "null list": dict(ids=None), "null masks": dict(masks=None),
                 "null draws": dict(draw=None), "nfields 0": dict(nf=0),
                 "real(4) id": dict(ids=i32(ssh, lu), masks=i32(lu, lu), draw=u32(0, 1), nf=2), "absent id": dict(ids=i32(ff1)),
                 "repeated id": dict(ids=i32(ssh, ub, ssh), masks=i32(lu, lu, lu), draw=u32(0, 1, 2), nf=3),
                 "real(8) mask": dict(masks=i32(ub)), "mask -2": dict(masks=i32(-2)), "mask 17": dict(masks=i32(17)),
                 "reach -1": dict(reach=-1), "reach 17": dict(reach=17), "passes -1": dict(passes=-1), "passes 4": dict(passes=4),
                 "amplitude 0": dict(amp=0.0), "amplitude < 0": dict(amp=-1.0), "amplitude NaN": dict(amp=np.nan),
                 "amplitude Inf": dict(amp=np.inf), "no member": dict(use=use()), "centring one member": dict(use=use(0, 1)),
                 "14 members at R 16, P 3": dict(use=None, reach=16, passes=3)}
        l0 = _lib.launch_count()
        for what, change in cases.items():
            a = {**ok, **change}
            rc = L.ocn_ens_perturb(a["ens"], a["ids"], a["masks"], a["draw"], a["nf"], a["use"], a["seed"], a["reach"],
                                   a["passes"], a["centre"], a["amp"])
            assert rc == ERR_ARG, what
            assert e.info() == info0, what
        for what, args in {"null ensemble": (None, 0, 0, hp), "null host": (e.ens, 0, 0, None), "k -1": (e.ens, -1, 0, hp),
                           "k 1": (e.ens, 1, 0, hp)}.items():
            assert L.ocn_ens_perturb_download(*args) == ERR_ARG, what
        assert L.ocn_ens_perturb_download(e.ens, 0, 0, hp) == ERR_STATE       # no call yet
        # the wrapper checks before the call
        for args, kw, exc in ((("0.5",), {}, TypeError), ((np.nan,), {}, ValueError), ((0.0,), {}, ValueError),
                              ((1.0,), dict(reach=17), ValueError), ((1.0,), dict(passes=4), ValueError),
                              ((1.0,), dict(reach=1.5), TypeError), ((1.0,), dict(seed=-1), ValueError),
                              ((1.0,), dict(seed=1 << 64), ValueError), ((1.0,), dict(draw=(1 << 32) - 2), ValueError),
                              ((1.0,), dict(names=()), ValueError), ((1.0,), dict(masks={"hhq": None}), ValueError),
                              ((1.0,), dict(members=[3]), ValueError), ((1.0,), dict(reach=16, passes=3), ValueError)):
            with pytest.raises(exc):
                e.perturb(*args, **kw)
        with pytest.raises(KeyError):
            e.perturb(1.0, names=("no_such_field",))
        with pytest.raises(amd.OcnError) as ei:
            e.perturb(1.0, names=("ssh", "ssh"))
        assert ei.value.code == ERR_ARG
        with pytest.raises(amd.OcnError) as ei:
            e.perturbation(0)
        assert ei.value.code == ERR_STATE
        assert _lib.launch_count() == l0 and (host == -7).all()
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
        # 13 members at R = 16, P = 3 are within the bound; afterwards a = 13 is not a member in use of that call
        l1 = _lib.launch_count()
        assert L.ocn_ens_perturb(e.ens, i32(ssh), i32(-1), u32(9), 1, use(*([1] * 13)), 1, 16, 3, 1, 1.0e-9) == OK
        assert _lib.launch_count() == l1 + 2
        assert L.ocn_ens_perturb_download(e.ens, 0, 13, hp) == ERR_ARG and L.ocn_ens_perturb_download(e.ens, 0, -1, hp) == ERR_ARG
        assert (host == -7).all()
        assert L.ocn_ens_perturb_download(e.ens, 0, 12, hp) == OK
        noise_ok = (host == R.block_noise(e.members[0].blocks[0], [12], 1, 9, 16, 3)[0]).all()
    finally:
        e.close()
    assert pending == [True] * 14, pending
    assert st == [OK] * 14 and not bad, (st, bad)
    assert noise_ok
