"""GPU tests of every per-member ensemble kernel from 34 members up to the cap, OCN_ENS_MAX_MEMBERS = 256.

Every such kernel has two bodies, split at kEnsStatsReg = 32 members in use, and the other modules' member counts
stop at 33: the first count of the staged / LDS body, with a member-loop tail of one.  Here the counts are

    40    five full groups of 8, no tail
    128   ens_local.hip's k_ens_local<false> takes n x 512 B of dynamic LDS: exactly 64 KiB, the last count that
          launches without hipFuncAttributeMaxDynamicSharedMemorySize
    odd   members 1, 3, .. 255: 128 in use, member 0 not in use, the highest index (a uint8_t in ens_perturb.hip) in use
    129   the first count that needs the attribute
    255   a tail of 7 at the top; the chunk loads read pointer slot 255, which the launchers fill with member 0
    256   the cap: 128 KiB of dynamic LDS, full xk / yk / zk rows and one member per thread in ens_assim.hip

in ascending order on ONE module-scoped ensemble, so that ocn_ens_transform's staging buffer is reallocated from
call to call, and once more at 40 on the grown buffer.  The members not in use keep their bits: member 255 below
256, members 0 and 254 of the odd subset.

The references and the comparison helpers are the other ensemble modules' own, imported: the numpy restatements
over the members' own downloads, the CPU oracle per member for the stepping.  Every comparison is bitwise on
whole block arrays (NaN by position).  Tolerance: none -- but for the last test, where the device's LDS path at 129
members meets the batch Kalman update of tests/test_ens_kalman_cpu.py (ANALYTIC_TOL, 1e-12).

The 256-member fixture (256 contexts, their uploads, two step calls) is built once; its build time is printed by
test_stepping_at_the_cap (0.6 s on the MI355X; the module's 51 tests take 17 s, the slowest, the batch Kalman
comparison, 2.5 s, nearly all of it the extended-precision reference on the CPU).
"""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest

from tests import ens_assim_ref as A
from tests import ens_inflate_ref as IR
from tests import ens_local_ref as LR
from tests import ens_obs_ref as O
from tests import ens_perturb_ref as PR
from tests import ens_stats_ref as SR
from tests import shapes as S
from tests.test_ens_kalman_cpu import check as kalman_check
from tests.test_ens_local_cpu import ANALYTIC_TOL
from tests.test_gpu_ens_assim import STAGE_LAUNCHES, _assim_vs_restatement, _points
from tests.test_gpu_ens_fgat import SMALL, _assim_rec_vs_restatement, _recorded
from tests.test_gpu_ens_gate import _gated_vs_restatement
from tests.test_gpu_ens_inflate import _inflate_vs_downloads, _save_vs_downloads
from tests.test_gpu_ens_inflate import _same_state as _same_inflated
from tests.test_gpu_ens_local import OBS_61x9, _changed, _ring_mismatches, _tapers, _update_vs_downloads
from tests.test_gpu_ens_obs import _assim_h_vs_restatement, _bilinear_61x9, _sample_h_vs_downloads
from tests.test_gpu_ens_perturb import _noise_vs_restatement, _perturb_vs_downloads
from tests.test_gpu_ens_perturb import _same_state as _same_perturbed
from tests.test_gpu_ens_stats import _counts_diff
from tests.test_gpu_ens_transform import _downloads, _run, _transform_vs_downloads
from tests.test_gpu_ensemble import _bad, _calls, _start

pytestmark = pytest.mark.gpu

OK = 0
CAP = 256
SHAPE = S.Shape(61, 9)
ODD = "odd"
CASES = [40, 128, ODD, 129, 255, 256]      # the counts 40, 128, 129, 255, 256 and the odd subset, ascending in use
NAMES = ("ssh", "ubrtr")


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


@pytest.fixture(scope="module")
def ens256(amd):
    """256 members of Shape(61, 9), class noise, after calls [2, 3], complete: the ensemble, the second call's info
    and launches, and the seconds the whole took."""
    from ocean_model_arch_amd import _lib
    t0 = time.perf_counter()
    e = _start(amd, SHAPE, ["noise"] * CAP)
    try:
        e.step(2)
        assert e.synchronize() == [OK] * CAP
        l0 = _lib.launch_count()
        e.step(3)
        launches = _lib.launch_count() - l0
        info = e.info()
        e.complete()
        assert e.synchronize() == [OK] * CAP
        yield SimpleNamespace(e=e, info=info, launches=launches, build_s=time.perf_counter() - t0)
    finally:
        e.close()


def _case(case):
    """(members as the wrappers take them, their indices, the members not in use that are watched)."""
    if case == ODD:
        return range(1, CAP, 2), list(range(1, CAP, 2)), [0, CAP - 2]
    if case == CAP:
        return None, list(range(CAP)), []
    return range(case), list(range(case)), [CAP - 1]


def _held(e, watched, names):
    return {(i, nm): e.members[i].download(0, nm) for i in watched for nm in names}


def _kept(e, held):
    return [f"member {i}:{nm}" for (i, nm), a in held.items() if not SR.bits_equal(e.members[i].download(0, nm), a)]


def _scale(n):
    """The z rows' scale of the other modules (0.25 at up to 33 members) with the growth of an n-term sum taken out."""
    return 0.25 * (33.0 / n) ** 0.5


# ---------------------------------------------------------------- 5. stepping at the cap
def test_stepping_at_the_cap(amd, ens256):
    """Every field of each of the 256 members is its own oracle run after 5 steps; all 256 went in batched launches,
    and groups, rows, tiles and launches are ocn_ens_plan's for the same capacity."""
    from ocean_model_arch_amd.ensemble import plan
    e, got = ens256.e, ens256.info
    print(f"the 256-member fixture took {ens256.build_s:.2f} s")
    bad = _bad(e, SHAPE, ["noise"] * CAP, 5)
    assert not bad, bad[:8]
    want = plan(e.members[0].blocks[0].c_block(), [0] * CAP, got["capacity"])
    big = max(want, key=lambda g: len(g["members"]))
    assert got["batched"] == CAP and got["members"] == CAP
    assert (got["groups"], got["rows"], got["tiles"], got["max_group"]) == \
        (len(want), big["rows"], big["tiles"], len(big["members"])), (got, [len(g["members"]) for g in want])
    assert ens256.launches == len(want)
    assert sorted(i for g in want for i in g["members"]) == list(range(CAP))


def test_groups_of_100(amd):
    """A second ensemble of 256 with set_max_group(100): the plan's groups of 100, 100 and 56 members, and the same
    bits -- every member is still its oracle run."""
    from ocean_model_arch_amd.ensemble import plan
    classes = ["noise"] * CAP
    e = _start(amd, SHAPE, classes)
    try:
        e.set_max_group(100)
        infos, launches, st = _calls(e, [2, 3])
        bad = _bad(e, SHAPE, classes, 5)
        want = []
        for part in (range(0, 100), range(100, 200), range(200, CAP)):
            want += plan(e.members[0].blocks[0].c_block(), [0 if i in part else -1 for i in range(CAP)], infos[1]["capacity"])
    finally:
        e.close()
    assert st == [OK] * CAP and not bad, (st, bad[:8])
    assert [len(g["members"]) for g in want] == [100, 100, 56]
    assert [g["members"] for g in want] == [list(range(0, 100)), list(range(100, 200)), list(range(200, CAP))]
    got = infos[1]
    assert (got["groups"], got["batched"], got["max_group"], got["rows"], got["tiles"]) == \
        (3, CAP, 100, want[0]["rows"], want[0]["tiles"]), got
    assert launches[1] == 3


# ---------------------------------------------------------------- 1. local_update
@pytest.mark.parametrize("case", CASES)
def test_local_update(amd, ens256, case):
    """tests/test_gpu_ens_local.py test_member_counts at the large counts: four tapers in turn, one launch per field
    and block, the members not in use keep their bits."""
    from ocean_model_arch_amd import _lib
    e = ens256.e
    members, idx, watched = _case(case)
    n = len(idx)
    held = _held(e, watched, NAMES)
    before = None
    for t, (what, taper) in enumerate(_tapers(65, 13)):
        y, z = LR.rows(len(OBS_61x9), n, 100 * n + t + (7 if case == ODD else 0),
                       scale=_scale(n) * (0.08 if what == "all points" else 1.0))
        l0 = _lib.launch_count()
        bad, after = _update_vs_downloads(e, y, z, OBS_61x9, taper, NAMES, members, before)
        assert not bad, (what, bad[:8])
        assert _lib.launch_count() - l0 == len(NAMES), what
        if before is not None:
            assert _changed(before, after) == (what != "all zero"), what
        before = after
    assert not _kept(e, held)


# ---------------------------------------------------------------- 2. the filter on the device
@pytest.mark.parametrize("case", CASES)
def test_assimilate(amd, ens256, case):
    """assimilate(device=True) with a Gaspari-Cohn and a ringed taper; at 129 and 256 members also the gate (outliers
    planted at k = 2 and 7) and the off-grid route, each with the launches its own module asserts."""
    e = ens256.e
    members, idx, watched = _case(case)
    n = len(idx)
    held = _held(e, watched, NAMES)
    seed = 10 * n + (5 if case == ODD else 0)
    tapers = [("gaspari-cohn", A.taper_table(6.0)), ("ring", A.ringed_taper(50))]
    for t, (what, taper) in enumerate(tapers):
        bad, launches, got, hx0 = _assim_vs_restatement(e, "ssh", OBS_61x9, taper, NAMES, members, seed=seed + t)
        assert not bad, (what, bad[:8])
        assert launches == len(NAMES) + STAGE_LAUNCHES, what
        assert got["hx"].shape == (len(OBS_61x9), n) and got["nonfinite"] == 0
        assert not A.bits_equal(got["hx"], hx0), what
    if case in (129, 256):
        for t, (what, taper) in enumerate(tapers):
            bad, launches, got, hx0 = _gated_vs_restatement(e, "ssh", OBS_61x9, taper, NAMES, (2, 7), members=members,
                                                            seed=seed + 2 + t)
            assert not bad, ("gate", what, bad[:8])
            assert launches == len(NAMES) + STAGE_LAUNCHES, what
            assert got["hx"].shape == (len(OBS_61x9), n) and got["rejected"] == 2 and got["nonfinite"] == 0
            assert not A.bits_equal(got["hx"], hx0), what
            op = _bilinear_61x9("ssh", 11, seed + t)
            bad, launches, got, hx0 = _assim_h_vs_restatement(e, op, taper, NAMES, members, seed=seed + 4 + t)
            assert not bad, ("off-grid", what, bad[:8])
            assert launches == len(NAMES) + STAGE_LAUNCHES, what
            assert got["hx"].shape == (11, n) and not O.bits_equal(got["hx"], hx0)
    assert not _kept(e, held)


@pytest.mark.parametrize("n", [129, 256])
def test_assimilate_recorded(amd, n):
    """The recorded route on an ensemble of its own, SMALL shape: 20 observations over a window of 7 records, rows
    named repeatedly, times at and between the records."""
    names = ("ssh", "ubrtr")
    e, op = _recorded(amd, SMALL, ["noise"] * n, 9, [2, 5])
    try:
        e.complete()                              # (no tail is formed inside the launches counted below)
        records = e.record_info()["records"]
        assert records == 7
        rng = np.random.default_rng(n)
        at = rng.uniform(1.0, float(records), 20)
        at[:3] = [1.0, 2.5, float(records)]
        rows = rng.integers(0, 9, 20)
        bad, launches, got, hx0 = _assim_rec_vs_restatement(e, rows, at, op.anchors[rows], O.taper_table(5.0), names, seed=n)
        st = e.synchronize()
    finally:
        e.close()
    assert not bad, bad[:8]
    assert launches == len(names) + STAGE_LAUNCHES
    assert got["hx"].shape == (20, n) and not O.bits_equal(got["hx"], hx0) and got["nonfinite"] == 0
    assert st == [OK] * n


# ---------------------------------------------------------------- 3. transform and sample
def _weights(n, seed, sparse):
    """A well-scaled dense matrix (the identity plus O(1 / n) entries of both signs); `sparse`: with one entry in
    16 zeroed, a zero of each sign among them, and the last member's column a unit column."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, (n, n)) / n + np.eye(n)
    if sparse:
        w[rng.uniform(size=(n, n)) < 1.0 / 16.0] = 0.0
        w[0, 1], w[1, 0] = 0.0, -0.0
        w[:, n - 1] = 0.0
        w[n - 1, n - 1] = 1.0
    return w


@pytest.mark.parametrize("case", CASES + ["40 again"])
def test_transform(amd, ens256, case):
    """The staging path at every count, the buffer growing from case to case and used once more by a smaller count: a
    dense matrix (every group of 8 weights straight through) and one with zero entries and a unit column (the skip
    branch; the member with the unit column keeps its bits).  sample() at the same points is the downloads."""
    e = ens256.e
    members, idx, watched = _case(40 if case == "40 again" else case)
    n = len(idx)
    held = _held(e, watched, NAMES)
    for sparse in (False, True):
        w = _weights(n, 3 * n + sparse + (11 if case == ODD else 0) + (13 if case == "40 again" else 0), sparse)
        full = (w[:, :n // 8 * 8].reshape(n, n // 8, 8) != 0.0).all(axis=2)   # a pass's 8 weights of one input
        assert full.any() and full.all() != sparse and (w == 0.0).any() == sparse   # (the premise: both branches)
        last = e.members[idx[-1]].download(0, "ssh")
        bad = _transform_vs_downloads(e, w, NAMES, members)
        assert not bad, (sparse, bad[:8])
        assert SR.bits_equal(e.members[idx[-1]].download(0, "ssh"), last) == sparse
    now = _downloads(e, ("ssh",), idx)
    assert A.bits_equal(e.sample("ssh", _points(e, OBS_61x9), members=members),
                        A.gather({0: now["ssh"]}, e.members[0].blocks, e.block_of, OBS_61x9))
    assert not _kept(e, held)


# ---------------------------------------------------------------- 4. stats, extrema, inflate, perturb, sample_h
@pytest.mark.parametrize("case", CASES)
def test_stats(amd, ens256, case):
    """All five statistics of ssh against the restatement over the downloads, in one launch."""
    from ocean_model_arch_amd import _lib
    e = ens256.e
    members, idx, _ = _case(case)
    ssh = [m.download(0, "ssh") for m in e.members]
    bad = _counts_diff(e, ssh, len(idx), SR.STATS, members)
    assert not bad, bad
    use = (C.c_uint8 * CAP)(*[1 if i in set(idx) else 0 for i in range(CAP)])
    l0 = _lib.launch_count()
    assert amd.lib().ocn_ens_stats(e.ens, 0, _lib.FIELD_ID["ssh"], use, 31) == OK and _lib.launch_count() - l0 == 1


def test_extrema(amd, ens256):
    """The extrema of each of the 256 members against the restatement over its download; nothing is non-finite after
    everything the tests above did to the state."""
    e = ens256.e
    b = e.members[0].blocks[0]
    lu = e.members[0].download(0, "lu")
    inner = (b.nx_start - b.bnd_x1, b.nx_end - b.bnd_x1 + 1, b.ny_start - b.bnd_y1, b.ny_end - b.bnd_y1 + 1)
    for nm in NAMES:
        ext = e.extrema(nm)
        want = [SR.extrema([m.download(0, nm)], [lu], [inner]) for m in e.members]
        assert ext == want
        assert len(ext) == CAP and all(x["nonfinite"] == 0 and x["count"] > 0 for x in ext)


@pytest.mark.parametrize("case", CASES)
def test_inflate(amd, ens256, case):
    """tests/test_gpu_ens_inflate.py test_member_counts at the large counts: spread_save, a local_update that changes
    the spread, then RTPS with alpha 0.7, CONST with 1.05 and RTPS with alpha 0, which must change nothing."""
    e = ens256.e
    members, idx, watched = _case(case)
    n = len(idx)
    held = _held(e, watched, NAMES)
    bad, launches, sb = _save_vs_downloads(e, NAMES, members)
    assert not bad, bad
    assert launches == len(NAMES)
    y, z = LR.rows(len(OBS_61x9), n, 100 * n + 50, scale=_scale(n))
    e.local_update(y, z, OBS_61x9, LR.ringed_taper(50, 1), names=NAMES, members=members)
    for mode, alpha in (("rtps", 0.7), ("const", 1.05), ("rtps", 0.0)):
        bad, launches, before, after = _inflate_vs_downloads(e, alpha, mode, NAMES, sb, members)
        assert not bad, (mode, alpha, bad[:8])
        assert launches == len(NAMES), (mode, alpha)
        assert _same_inflated(before, after) == (alpha == 0.0), (mode, alpha)
        assert (e.inflation("ssh", "factor") == 1.0).all() == (alpha == 0.0), (mode, alpha)
    assert all(IR.bits_equal(e.inflation(nm, "prior_spread"), sb[0][nm]) for nm in NAMES)
    assert not _kept(e, held)


@pytest.mark.parametrize("case", CASES)
def test_perturb(amd, ens256, case):
    """tests/test_gpu_ens_perturb.py test_member_counts at the large counts with reach, passes = (4, 2) and (16, 2),
    both exact in double at 256 members; (16, 3) is not, and is refused.  ssh and sshp share a draw, ubrtr has the
    next: 2 noise launches and 3 applications."""
    from ocean_model_arch_amd import _lib
    e = ens256.e
    members, idx, watched = _case(case)
    n = len(idx)
    groups = (("ssh", "sshp"), "ubrtr")
    held = _held(e, watched, PR.flat(groups))
    for reach, passes in ((4, 2), (16, 2)):
        assert PR.exact(CAP, reach, passes)
        kw = dict(amplitude=2.0e-3, reach=reach, passes=passes, seed=1000 * reach + n + (7 if case == ODD else 0), draw=n, centre=True)
        bad, launches, before, after = _perturb_vs_downloads(e, idx, groups, **kw)
        assert not bad, (reach, passes, bad[:8])
        assert launches == 2 + 3
        assert not _same_perturbed(before, after)
        assert not _noise_vs_restatement(e, idx, kw["seed"], n + 1, reach, passes)      # (the last draw id: ubrtr's)
    assert not _kept(e, held)
    if n == CAP:
        assert not PR.exact(CAP, 16, 3)
        l0 = _lib.launch_count()
        with pytest.raises(ValueError):
            e.perturb(2.0e-3, reach=16, passes=3, names=groups, seed=1, draw=1)
        assert _lib.launch_count() == l0


@pytest.mark.parametrize("case", CASES)
def test_sample_h(amd, ens256, case):
    """tests/test_gpu_ens_obs.py test_sample_h at the large counts."""
    members, idx, _ = _case(case)
    _sample_h_vs_downloads(ens256.e, len(idx), members)


# ---------------------------------------------------------------- 6. wave edges and a block grid on the LDS path
def test_wave_edges(amd):
    """tests/test_gpu_ens_local.py test_wave_edges with 129 members: Shape(121, 65), the observations on both sides of
    the wave edges at array columns 34 and 98, on the first and last rows and in the corners."""
    n = 129
    e = _start(amd, S.Shape(121, 65), ["noise"] * n)
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
            y, z = LR.rows(len(ij), n, 900 + t, scale=_scale(n) * (0.04 if what == "all points" else 1.0))
            bad, before = _update_vs_downloads(e, y, z, ij, taper, names, None, before)
            assert not bad, (what, bad[:8])
    finally:
        e.close()


def test_block_grid(amd):
    """tests/test_gpu_ens_assim.py test_block_grid with 129 members: a 2 x 2 block grid through
    assimilate(device=True) -- k_ens_sample's per-block table tab[k * n + m] and the per-block lists above 32
    members -- and the halo rings coherent before and after."""
    n = 129
    e = _start(amd, S.Shape(17, 19, (2, 2)), ["noise"] * n)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * n
        blocks = e.members[0].blocks
        assert len(blocks) == 4
        sx, sy = max(b.nx_start for b in blocks), max(b.ny_start for b in blocks)
        ij = np.array([[3, 3], [19, 21], [sx - 1, sy], [sx, sy - 1], [1, 12], [sx, sy - 1], [21, 23], [sx + 2, 4], [5, sy + 1]])
        assert len({e.block_of(int(i), int(j)) for i, j in ij}) == 4
        watch = (0, 64, 128)
        was, _ = _ring_mismatches(e, NAMES, watch)
        bad, launches, _, _ = _assim_vs_restatement(e, "ssh", ij, A.ringed_taper(10, 3), NAMES, seed=3)
        lost, _ = _ring_mismatches(e, NAMES, watch)
        bad2, launches2, _, _ = _assim_vs_restatement(e, "ssh", ij, A.taper_table(9.0), NAMES, seed=4)
        lost2, _ = _ring_mismatches(e, NAMES, watch)
    finally:
        e.close()
    assert not was and not bad and not bad2, (was, bad[:8], bad2[:8])
    assert not lost and not lost2, (lost, lost2)
    assert launches == launches2 == len(NAMES) * 4 + STAGE_LAUNCHES


# ---------------------------------------------------------------- B. the batch Kalman anchor
def test_batch_kalman(amd, ens256):
    """129 members in use, uniform [0.5, 1.5] data uploaded as ssh and ubrtr, 11 observations of ssh (one point
    twice) with a taper that is 1.0 over the whole array: the downloads before and after, the whole 65 x 13 arrays
    of both fields, against the batch Kalman update in extended precision -- the device's LDS path against
    mathematics written independently of the restatements.  The control: off by more than 1e-6 with R * 1.01."""
    e = ens256.e
    n = 129
    members, idx = range(n), list(range(n))
    b = e.members[0].blocks[0]
    assert b.shape == (65, 13)
    rng = np.random.default_rng(129)
    for nm in NAMES:
        for i in idx:
            e.members[i].upload(0, nm, rng.uniform(0.5, 1.5, b.shape))
    before = _downloads(e, NAMES, idx)
    hx0 = e.sample("ssh", _points(e, OBS_61x9), members=members)
    values = hx0.mean(axis=1) + rng.uniform(-0.3, 0.3, len(hx0))
    variances = 0.01 + 0.5 * hx0.var(axis=1, ddof=1)
    taper = np.ones(65 * 65 + 13 * 13)
    got = e.assimilate("ssh", OBS_61x9, values, variances, taper, names=NAMES, members=members, device=True)
    after = _downloads(e, NAMES, idx)
    stack = lambda d: np.concatenate([np.stack([a.ravel() for a in d[nm]], axis=1) for nm in NAMES], axis=0)   # noqa: E731
    H = np.zeros((len(OBS_61x9), 2 * 65 * 13))
    for k, (i, j) in enumerate(OBS_61x9):
        H[k, (int(i) - b.bnd_x1) * 13 + (int(j) - b.bnd_y1)] = 1.0
    assert A.bits_equal(H @ stack(before), hx0)                # (H reads what sample() read)
    em, ev = kalman_check("129 members on the device", stack(before), stack(after), H, values, variances)
    assert em <= ANALYTIC_TOL and ev <= ANALYTIC_TOL
    assert got["nonfinite"] == 0 and (got["posterior_spread"] < got["prior_spread"]).all()
