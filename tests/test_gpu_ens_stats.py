"""GPU tests of the ensemble statistics (ocn_ens_stats, ocn_ens_stats_download, ocn_ens_stats_output_r4,
ocn_ens_extrema; ens_stats.hip k_ens_stats, k_ens_extrema).

The reference is the numpy restatement of the definitions (tests/ens_stats_ref.py, itself checked against
a scalar loop by tests/test_ens_stats_cpu.py) over the CPU oracle's fields or over the members' own
downloads; inputs and per-member oracle runs come from tests/shapes.py as tests/test_gpu_ensemble.py
builds them (classes, seed offset 1000 i).  Every comparison is bitwise on the whole block array (halo
and land included; R.bits_equal), extrema min / max by value.  Tolerance: none.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ens_stats_ref as R
from tests import shapes as S
from tests.test_gpu_ensemble import _bad, _start, member_reference

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE = 0, 1, 4
ALL = R.STATS


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _run(e, calls):
    """The calls (a synchronize() after the first: the known-constant verdicts reach the host); NO complete()."""
    for i, n in enumerate(calls):
        e.step(n)
        if i == 0:
            assert e.synchronize() == [OK] * len(e)


def _downloads(e, name, k=0, members=None):
    idx = range(len(e)) if members is None else sorted(set(members))
    return [e.members[i].download(k, name) for i in idx]


def _diff(got, want):
    """The statistics that differ from the restatement, by name."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    return [nm for nm in want if not (got[nm].dtype == np.float64 and got[nm].flags.f_contiguous
                                      and R.bits_equal(got[nm], want[nm]))]


# ---------------------------------------------------------------- 1. pending tail, swapped roles
def test_pending_tail_and_swapped_roles(amd):
    """9 members after calls [2, 5] with the last call's tail pending and the pair roles swapped (an odd
    total): the statistics equal the restatement over the ORACLE's fields after 7 steps -- hhq exists only
    once the tail is formed, ssh sits in the other buffer of its pair.  Then 4 more steps: every member is
    still its oracle run after 11 steps, so the statistics disturbed nothing."""
    from ocean_model_arch_amd import _lib
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 9, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert all(m.option(_lib.OPT_LAZY_TAIL) == 2 for m in e.members)   # the tails are pending
        bad = []
        for name, what in (("ssh", ALL), ("ubrtr", ALL), ("hhq", ALL)):
            ref = [member_reference(shape, "noise", 1000 * i, sum(calls))[(1, 1)][name] for i in range(9)]
            bad += [f"{name}:{x}" for x in _diff(e.stats(name, what), R.stats(ref, what))]
        e.step(4)
        e.complete()
        st = e.synchronize()
        bad += _bad(e, shape, classes, sum(calls) + 4)
    finally:
        e.close()
    assert st == [OK] * 9 and not bad, (st, bad)


def test_member_not_in_use_is_not_touched(amd):
    """Statistics over members 0 and 2 form their pending tails and leave member 1's pending; member 1
    is still its oracle run once it is completed."""
    from ocean_model_arch_amd import _lib
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        ref = [member_reference(shape, "noise", 1000 * i, sum(calls))[(1, 1)]["ssh"] for i in (0, 2)]
        bad = _diff(e.stats("ssh", ALL, members=[2, 0]), R.stats(ref, ALL))
        pending = [m.option(_lib.OPT_LAZY_TAIL) == 2 for m in e.members]
        e.complete()
        st = e.synchronize()
        bad += _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert pending == [False, True, False], pending
    assert st == [OK] * 3 and not bad, (st, bad)


# ---------------------------------------------------------------- 2. member counts, 7. one launch
@pytest.fixture(scope="module")
def ens33(amd):
    """33 members of Shape(61, 9), class noise, after calls [2, 3], complete; their ssh downloaded once."""
    shape, classes = S.Shape(61, 9), ["noise"] * 33
    e = _start(amd, shape, classes)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 33
        yield e, _downloads(e, "ssh")
    finally:
        e.close()


def _counts_diff(e, ssh, n, what=ALL, members=None):
    """The statistics `what` of ssh over n members -- the first n (all of them: `use` NULL), or the n `members` --
    that differ from the restatement over their entries of `ssh`, every member's download."""
    if members is None:
        members = None if n == len(e) else range(n)
    idx = range(len(e)) if members is None else sorted(set(members))
    assert len(idx) == n
    return _diff(e.stats("ssh", what, members=members), R.stats([ssh[i] for i in idx], what))


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 32, 33])
def test_member_counts(amd, ens33, n):
    """n members in use: below, at and above the groups of 8 loads, the register path's last count (32)
    and the first of the two-pass path (33).  n = 1: mean, min and max are the member's own bits and
    VAR / SPREAD are refused."""
    from ocean_model_arch_amd import _lib
    e, ssh = ens33
    what = ALL if n > 1 else ("mean", "min", "max")
    bad = _counts_diff(e, ssh, n, what)
    assert not bad, bad
    if n == 1:
        got = e.stats("ssh", what, members=[0])
        assert all(R.bits_equal(got[nm], ssh[0]) for nm in what)
        use = (C.c_uint8 * 33)(1)
        for bit in (_lib.ENS_STATS["var"], _lib.ENS_STATS["spread"], _lib.ENS_STATS["mean"] | _lib.ENS_STATS["spread"]):
            assert amd.lib().ocn_ens_stats(e.ens, 0, _lib.FIELD_ID["ssh"], use, bit) == ERR_ARG


@pytest.mark.parametrize("n", [9, 33])
def test_one_launch(amd, ens33, n):
    """With every member complete, all five statistics cost exactly one kernel launch."""
    from ocean_model_arch_amd import _lib
    e, _ = ens33
    use = (C.c_uint8 * 33)(*([1] * n + [0] * (33 - n)))
    l0 = _lib.launch_count()
    rc = amd.lib().ocn_ens_stats(e.ens, 0, _lib.FIELD_ID["ssh"], use, 31)
    assert rc == OK and _lib.launch_count() - l0 == 1


# ---------------------------------------------------------------- 3. shapes
@pytest.mark.parametrize("shape", [S.Shape(1, 1), S.Shape(5, 4), S.Shape(61, 33), S.Shape(121, 65, mask="rough")],
                         ids=lambda s: s.id)
def test_shapes(amd, shape):
    """Arrays narrower than a wave, widths on both sides of 64 and 128 (with the pitch padding) and land
    inside: all five statistics bitwise; the real(4) record is float32 of the statistic with undef
    exactly where member 0's record of the field has it."""
    from ocean_model_arch_amd.output import UNDEF
    e = _start(amd, shape, ["noise"] * 3)
    try:
        _run(e, [2, 3])
        got = e.stats("ssh", ALL)
        bad = _diff(got, R.stats(_downloads(e, "ssh"), ALL))
        m0, b = e.members[0], e.members[0].blocks[0]
        land = m0.output_r4(0, "ssh", float(UNDEF)) == UNDEF
        assert land.any() == (shape.mask is not None)
        for nm in ALL:
            r4 = e.stats_output_r4("ssh", nm)
            want = got[nm][b.nx_start - b.bnd_x1:b.nx_end - b.bnd_x1 + 1,
                           b.ny_start - b.bnd_y1:b.ny_end - b.bnd_y1 + 1].astype(np.float32)
            want[land] = UNDEF
            if not (r4.dtype == np.float32 and r4.shape == want.shape and r4.tobytes(order="F") == want.tobytes(order="F")):
                bad.append(f"r4:{nm}")
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 4. subsets, special values, extrema
def test_subsets_and_special_values(amd):
    """A NaN in member 1, +Inf in member 3, +0.0 / -0.0 in members 0 / 2 under larger values, one point
    NaN in all -- at sea points of ssh; subsets given in any order run in member order; the extrema count
    the non-finite values and skip them, land and the halo."""
    shape = S.Shape(61, 9, mask="rough")
    e = _start(amd, shape, ["noise"] * 5)
    try:
        m0 = e.members[0]
        b = m0.blocks[0]
        lu = m0.download(0, "lu")
        inner = (b.nx_start - b.bnd_x1, b.nx_end - b.bnd_x1 + 1, b.ny_start - b.bnd_y1, b.ny_end - b.bnd_y1 + 1)
        sea = [tuple(p + np.array([inner[0], inner[2]])) for p in
               np.argwhere(np.abs(lu[inner[0]:inner[1], inner[2]:inner[3]]) >= 0.5)]
        p_nan, p_inf, p_zero, p_all = sea[3], sea[40], sea[77], sea[120]
        for i, m in enumerate(e.members):
            a = m.download(0, "ssh")
            a[p_zero] = {0: 0.0, 2: -0.0}.get(i, 1.0 + i)
            a[p_all] = np.nan
            if i == 1:
                a[p_nan] = np.nan
            if i == 3:
                a[p_inf] = np.inf
            m.upload(0, "ssh", a)
        ssh = _downloads(e, "ssh")
        bad = []
        for members in (None, [0, 2, 4], [1], [3, 1]):
            what = ALL if members is None or len(members) > 1 else ("mean", "min", "max")
            idx = range(5) if members is None else sorted(members)
            got = e.stats("ssh", what, members=members)
            bad += [f"{members}:{x}" for x in _diff(got, R.stats([ssh[i] for i in idx], what))]
            if members is None:   # the special values are where the test put them
                assert np.signbit(got["min"][p_zero]) == False and got["min"][p_zero] == 0.0   # noqa: E712
                assert np.isnan(got["mean"][p_nan]) and got["min"][p_nan] == min(ssh[i][p_nan] for i in (0, 2, 3, 4))
                assert got["max"][p_inf] == np.inf and np.isnan(got["var"][p_inf])
                assert all(np.isnan(got[nm][p_all]) for nm in ALL)
        ext = e.extrema("ssh")
        want = [R.extrema([ssh[i]], [lu], [inner]) for i in range(5)]
    finally:
        e.close()
    assert not bad, bad
    assert ext == want, (ext, want)
    assert [x["nonfinite"] for x in ext] == [1, 2, 1, 2, 1] and ext[0]["count"] == len(sea)


# ---------------------------------------------------------------- 5. block grids and tracers
def test_block_grid_with_tracers(amd):
    """A 2 x 2 block grid with a tracer (such members are stepped one by one): the statistics of ssh and
    ff1_1 on every block, the extrema over all blocks."""
    shape = S.Shape(17, 19, (2, 2), 1, "rough")
    e = _start(amd, shape, ["noise"] * 3)
    try:
        _run(e, [2, 3])
        nblk = len(e.members[0].blocks)
        assert nblk == 4
        bad = []
        for name in ("ssh", "ff1_1"):
            for k in range(nblk):
                bad += [f"{name}[{k}]:{x}" for x in _diff(e.stats(name, ALL, k=k), R.stats(_downloads(e, name, k), ALL))]
        blocks = e.members[0].blocks
        inner = [(b.nx_start - b.bnd_x1, b.nx_end - b.bnd_x1 + 1, b.ny_start - b.bnd_y1, b.ny_end - b.bnd_y1 + 1)
                 for b in blocks]
        ext, want = {}, {}
        for name in ("ssh", "ff1_1"):
            ext[name] = e.extrema(name)
            want[name] = [R.extrema([m.download(k, name) for k in range(nblk)], [m.download(k, "lu") for k in range(nblk)],
                                    inner) for m in e.members]
        sea = int((S.mask_of(shape)[2:-2, 2:-2] == 0).sum())
    finally:
        e.close()
    assert not bad, bad
    assert ext == want, (ext, want)
    assert all(x["count"] == sea and x["nonfinite"] == 0 for x in ext["ssh"]), (ext["ssh"], sea)


# ---------------------------------------------------------------- 6. errors
def test_errors_keep_the_earlier_results(amd):
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    e = _start(amd, S.Shape(5, 4), ["noise"] * 2)
    try:
        ssh, mean_bit, spread_bit = _lib.FIELD_ID["ssh"], _lib.ENS_STATS["mean"], _lib.ENS_STATS["spread"]
        mean = e.stats("ssh", ("mean",))["mean"]
        host = np.zeros_like(mean, order="F")
        none = (C.c_uint8 * 2)(0, 0)
        cases = {"real(4) field": (0, _lib.FIELD_ID["lu"], None, mean_bit),
                 "k = -1": (-1, ssh, None, mean_bit), "k = 1": (1, ssh, None, mean_bit),
                 "what = 0": (0, ssh, None, 0), "unknown bit": (0, ssh, None, mean_bit | 32),
                 "no member": (0, ssh, none, mean_bit), "no tracers": (0, _lib.FIELD_ID["ff1_1"], None, mean_bit),
                 "flux_x without tracers": (0, _lib.FIELD_ID["flux_x"], None, mean_bit)}
        for what, (k, fid, use, bits) in cases.items():
            assert L.ocn_ens_stats(e.ens, k, fid, use, bits) == ERR_ARG, what
            assert L.ocn_ens_stats_download(e.ens, 0, spread_bit, host.ctypes.data_as(C.c_void_p)) == ERR_STATE, what
            assert L.ocn_ens_stats_download(e.ens, 0, mean_bit, host.ctypes.data_as(C.c_void_p)) == OK, what
            assert R.bits_equal(host, mean), what
        r4 = np.zeros((5, 4), dtype=np.float32, order="F")
        assert L.ocn_ens_stats_output_r4(e.ens, 0, spread_bit, C.c_float(0.0), r4.ctypes.data_as(C.c_void_p)) == ERR_STATE
        assert L.ocn_ens_stats_download(e.ens, 0, 3, host.ctypes.data_as(C.c_void_p)) == ERR_ARG   # two bits: no statistic
        assert L.ocn_ens_extrema(e.ens, _lib.FIELD_ID["lu"], (_lib.OcnEnsExtrema * 2)()) == ERR_ARG
        with pytest.raises(amd.OcnError) as ei:
            e.stats("ssh", ("spread",), members=[1])
        assert ei.value.code == ERR_ARG
        with pytest.raises(amd.OcnError) as ei:
            e.stats("ssh", ("mean",), members=[])
        assert ei.value.code == ERR_ARG
    finally:
        e.close()


# ---------------------------------------------------------------- 8. the GrADS records
def test_ensemble_output(amd, tmp_path):
    """Record 2 of ssh_mean.dat / ssh_spread.dat holds stats_output_r4's values where write_data puts a
    block's interior; record 1 is the earlier state's; the .ctl names the variable."""
    from ocean_model_arch_amd.output import UNDEF, LocalOutputTime, ensemble_output
    shape = S.Shape(61, 33, mask="rough")
    e = _start(amd, shape, ["noise"] * 3)
    try:
        t = LocalOutputTime.from_period(1.0)
        path = str(tmp_path)
        ensemble_output(e, 1, t, path)
        first = {st: e.stats_output_r4("ssh", st) for st in ("mean", "spread")}
        _run(e, [2, 3])
        ensemble_output(e, 2, t, path)
        want = {st: e.stats_output_r4("ssh", st) for st in ("mean", "spread")}
    finally:
        e.close()
    assert sorted(os.listdir(path)) == ["ssh_mean.ctl", "ssh_mean.dat", "ssh_spread.ctl", "ssh_spread.dat"]
    for st in ("mean", "spread"):
        rec = np.fromfile(os.path.join(path, f"ssh_{st}.dat"), dtype="<f4")
        assert rec.size == 2 * shape.W * shape.H
        for nrec, a in ((1, first[st]), (2, want[st])):
            # one block: its interior is the whole record, row j at ((ny_start + j - 3) * (nx - 4) + nx_start - 3) * 4
            got = rec[(nrec - 1) * shape.W * shape.H:nrec * shape.W * shape.H].reshape((shape.W, shape.H), order="F")
            assert got.tobytes(order="F") == a.tobytes(order="F"), (st, nrec)
        assert (want[st] == UNDEF).any() and not np.array_equal(first[st], want[st])
        ctl = open(os.path.join(path, f"ssh_{st}.ctl")).read()
        assert f"DSET    ^ssh_{st}.dat" in ctl and f"\nssh_{st} " in ctl and "TDEF       2 " in ctl, ctl
