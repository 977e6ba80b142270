"""GPU tests of the ensemble recombination and sampling (ocn_ens_transform, ocn_ens_sample;
ens_transform.hip k_ens_transform, k_ens_unstage, k_ens_sample).

The reference is the numpy restatement of the contract (tests/ens_transform_ref.py, itself checked against
a scalar loop by tests/test_ens_transform_cpu.py), applied to the CPU oracle's fields or to the members'
own downloads; inputs and per-member oracle runs come from tests/shapes.py as tests/test_gpu_ensemble.py
builds them (classes, seed offset 1000 i).  Every comparison is bitwise on whole block arrays (halo and
land included; NaN by position).  Tolerance: none.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ens_transform_ref as T
from tests import shapes as S
from tests.test_gpu_ensemble import _bad, _start, member_uploads

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, 1


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


def _pending(e):
    from ocean_model_arch_amd import _lib
    return [m.option(_lib.OPT_LAZY_TAIL) == 2 for m in e.members]


def _oracles(shape, classes, steps):
    """One oracle model per member (its inputs: class classes[i], seed offset 1000 i) after `steps` steps."""
    oms = []
    for i, cls in enumerate(classes):
        om = S.oracle_model(shape)
        for k, b in enumerate(om.blocks):
            for nm, a in member_uploads(shape, cls, 1000 * i).get((b.bm, b.bn), {}).items():
                om.f[k][nm][...] = a
        om.run(steps, 1.0)
        oms.append(om)
    return oms


def _oracle_transform(oms, w, names, members=None):
    """The restatement applied to fields `names` of every block of the oracle models `members` (None: all)."""
    idx = range(len(oms)) if members is None else sorted(set(members))
    for k in range(len(oms[0].blocks)):
        for nm in names:
            for i, a in zip(idx, T.transform([oms[i].f[k][nm] for i in idx], w)):
                oms[i].f[k][nm][...] = a


def _bad_vs(e, oms):
    """Every field of every member against its oracle model: ["member i (bm,bn):field", ...]."""
    bad = []
    for i, (m, om) in enumerate(zip(e.members, oms)):
        ref = {(b.bm, b.bn): om.f[k] for k, b in enumerate(om.blocks)}
        get = S.model_getter([m])
        assert get.blocks == set(ref)
        bad += [f"member {i} {x}" for x in S.mismatches(ref, get)]
    return bad


def _downloads(e, names, idx, k=0):
    return {nm: [e.members[i].download(k, nm) for i in idx] for nm in names}


def _transform_vs_downloads(e, w, names, members=None, k_all=None):
    """transform() against the restatement over the members' own downloads, on every block: the
    (member, block, field) that differ.  Completes the members in use (the downloads)."""
    idx = list(range(len(e))) if members is None else sorted(set(members))
    blocks = range(len(e.members[0].blocks)) if k_all is None else k_all
    before = {k: _downloads(e, names, idx, k) for k in blocks}
    e.transform(w, names, members=members)
    bad = []
    for k in blocks:
        after = _downloads(e, names, idx, k)
        for nm in names:
            want = T.transform(before[k][nm], w)
            bad += [f"member {i} [{k}]:{nm}" for i, g, v in zip(idx, after[nm], want) if not T.bits_equal(g, v)]
    return bad


# ---------------------------------------------------------------- 1. continue as the oracle continues
def test_continue_as_the_oracle_continues(amd):
    """9 members after calls [2, 5]: the tails pending, the pair roles swapped (an odd total).  transform(STATE)
    with a dense, well-scaled matrix, then 4 more steps: every field of every member equals the oracle run
    7 steps, recombined by the restatement, run 4 steps more -- the tail formation, the buffers of a pair
    after a swap, and everything the upload bookkeeping has to drop."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 9, [2, 5]
    w = np.random.default_rng(41).uniform(-1.0, 1.0, (9, 9)) / 9.0 + np.eye(9) * 0.5
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 9
        e.transform(w)
        e.step(4)
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        _oracle_transform(oms, w, T.STATE)
        for om in oms:
            om.run(4, 1.0)
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert st == [OK] * 9 and not bad, (st, bad)


# ---------------------------------------------------------------- 2. member counts
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


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 32, 33])
def test_member_counts(amd, ens33, n):
    """n members in use: below, at and above the groups of 8 loads, the register path's last count (32) and
    the staging path's first (33), with a matrix that mixes a dense block, a permutation, an identity
    column, a zero column and negative weights.  Up to 32 members: one launch per field and block.  The
    members not in use keep their bits."""
    from ocean_model_arch_amd import _lib
    e = ens33
    names = ("ssh", "ubrtr")
    members = None if n == 33 else range(n)
    w = T.mixed_weights(n)
    outside = None if n == 33 else e.members[32].download(0, "ssh")
    bad = _transform_vs_downloads(e, w, names, members)
    assert not bad, bad
    if outside is not None:
        assert T.bits_equal(e.members[32].download(0, "ssh"), outside)
    if n <= 32:   # every member complete now (the downloads): the launches are the transform's alone
        l0 = _lib.launch_count()
        e.transform(np.eye(n), names, members=members)
        assert _lib.launch_count() - l0 == len(names) * len(e.members[0].blocks)


def test_register_and_staging_paths_agree(amd, ens33):
    """The same 32 x 32 weights as the upper-left block of a 33 x 33 matrix whose last member keeps itself:
    the staging path gives the first 32 members the register path's bits."""
    e = ens33
    w32 = np.random.default_rng(3).uniform(-1.0, 1.0, (32, 32)) / 32.0
    w33 = np.zeros((33, 33))
    w33[:32, :32] = w32
    w33[32, 32] = 1.0
    before = [m.download(0, "ssh") for m in e.members]
    e.transform(w32, ("ssh",), members=range(32))
    reg = [m.download(0, "ssh") for m in e.members]
    for m, a in zip(e.members, before):
        m.upload(0, "ssh", a)
    e.transform(w33, ("ssh",))
    stg = [m.download(0, "ssh") for m in e.members]
    assert all(T.bits_equal(a, b) for a, b in zip(reg, stg))
    assert all(T.bits_equal(a, b) for a, b in zip(reg[:32], T.transform(before[:32], w32)))


# ---------------------------------------------------------------- 3. a member not in use
def test_member_not_in_use_is_not_touched(amd):
    """Members 0 and 2 are transformed: their pending tails are formed, member 1's stays pending, and member
    1 is still its oracle run once completed; members 0 and 2 are the oracle's, recombined."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 5]
    w = np.array([[0.75, -0.5], [0.25, 1.5]])
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 3
        e.transform(w, members=[2, 0])
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        _oracle_transform(oms, w, T.STATE, members=[0, 2])
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert pending == [False, True, False], pending
    assert st == [OK] * 3 and not bad, (st, bad)


# ---------------------------------------------------------------- 4. shapes
@pytest.mark.parametrize("shape", [S.Shape(1, 1), S.Shape(5, 4), S.Shape(61, 33), S.Shape(121, 65, mask="rough")],
                         ids=lambda s: s.id)
def test_shapes(amd, shape):
    """Arrays narrower than a wave, widths on both sides of 64 and 128 (with the pitch padding and the
    shifted first lanes) and land inside: halo, land and sea of the transformed arrays bitwise.

    What is checked beside that: every field of member 1 that is NOT transformed keeps its bits.  The
    fields of a block lie side by side in one slab, so a store before an array's first row or past its
    last would land in a neighbour and show here.  What is NOT checked: the padding between the rows
    inside the transformed arrays themselves.  No entry of the library reads it back (downloads and the
    statistics copy or read only the w points of a row), and a raw pointer would change the members' step
    decisions.  That the kernels cannot store there rests on their code: a lane returns on i >= w and
    addresses j * pitch + i only."""
    names = ("ssh", "ubrtrp")
    w = np.array([[0.5, -0.25, 1.0], [0.25, 1.25, 0.0], [-0.75, 0.5, 0.0]])
    e = _start(amd, shape, ["noise"] * 3)
    try:
        _run(e, [2, 3])
        m1 = e.members[1]
        others = [nm for nm in m1.field_names if nm not in names]
        keep = {nm: m1.download(0, nm) for nm in others}
        bad = _transform_vs_downloads(e, w, names)
        for nm in others:
            got = m1.download(0, nm)
            if got.tobytes(order="F") != keep[nm].tobytes(order="F"):
                bad.append(f"untransformed:{nm}")
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 5. block grid with tracers
def test_block_grid_with_tracers(amd):
    """A 2 x 2 block grid with two tracers (such members are stepped one by one): a tracer field and ssh
    recombined on every block, then stepped -- against the oracle recombined the same way and stepped.
    sample() there reads every block through the per-block table."""
    shape, classes, calls = S.Shape(17, 19, (2, 2), 2, "rough"), ["noise"] * 3, [2, 3]
    names = ("ff1_1", "ssh")
    w = np.array([[0.5, 0.25, 0.0], [0.5, 0.5, 0.0], [0.0, 0.25, 1.0]])
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        blocks = e.members[0].blocks
        assert len(blocks) == 4
        e.transform(w, names)
        pts = [(b.k, i, j) for b in blocks for (i, j) in ((b.bnd_x1, b.bnd_y1), (b.nx_start, b.ny_end), (b.bnd_x2, b.bnd_y2))]
        got = e.sample("ff1_1", pts)
        want = np.array([[m.download(k, "ff1_1")[i - blocks[k].bnd_x1, j - blocks[k].bnd_y1] for m in e.members]
                         for (k, i, j) in pts])
        e.step(3)
        e.complete()
        st = e.synchronize()
        oms = _oracles(shape, classes, sum(calls))
        _oracle_transform(oms, w, names)
        for om in oms:
            om.run(3, 1.0)
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert got.shape == (12, 3) and T.bits_equal(got, want)
    assert st == [OK] * 3 and not bad, (st, bad)


# ---------------------------------------------------------------- 6. special values
def test_special_values(amd):
    """Member 1, uploaded with NaN and +-Inf, gets an all-zero row and a unit column: the others stay finite
    and it keeps its bits.  -0.0 goes through a permutation with its sign.  Denormal weights."""
    shape = S.Shape(61, 9)
    e = _start(amd, shape, ["noise"] * 4)
    try:
        a = e.members[1].download(0, "ssh")
        a[3, 2], a[10, 5], a[40, 7], a[0, 0] = np.nan, np.inf, -np.inf, np.nan
        e.members[1].upload(0, "ssh", a)
        z = e.members[0].download(0, "ssh")
        z[5:9, 3], z[20, 6] = -0.0, 0.0
        e.members[0].upload(0, "ssh", z)
        w = np.random.default_rng(8).uniform(-1.0, 1.0, (4, 4))
        w[1, :] = 0.0
        w[:, 1] = -0.0
        w[1, 1] = 1.0
        bad = _transform_vs_downloads(e, w, ("ssh",))
        now = [m.download(0, "ssh") for m in e.members]
        assert T.bits_equal(now[1], a)
        assert all(np.isfinite(now[i]).all() for i in (0, 2, 3))
        # -0.0 through a permutation: member 0's zeros (uploaded again) arrive in member 3 with their signs
        e.members[0].upload(0, "ssh", z)
        perm = np.zeros((4, 4))
        perm[0, 3] = perm[3, 2] = perm[2, 0] = perm[1, 1] = 1.0
        bad += _transform_vs_downloads(e, perm, ("ssh",))
        got = e.members[3].download(0, "ssh")
        assert T.bits_equal(got, z) and np.signbit(got[5:9, 3]).all() and not np.signbit(got[20, 6])
        tiny = np.array([[5e-324, 1e-310, 0.0, -3e-320], [0.0, 1.0, 0.0, 0.0], [2.5e-308, -5e-324, 1.0, 1e-315],
                         [-1e-309, 0.0, 0.0, 2.0 ** -1040]])
        tiny[1, :] = 0.0
        tiny[1, 1] = 1.0
        bad += _transform_vs_downloads(e, tiny, ("ssh",))
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 7. sample
def test_sample(amd):
    """Interior, halo-corner and land points, 1 and 300 points, a subset given out of order, with tails
    pending before the call and formed afterwards for the members in use only; one launch once formed."""
    from ocean_model_arch_amd import _lib
    shape, classes, calls = S.Shape(61, 33, mask="rough"), ["noise"] * 3, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 3
        b = e.members[0].blocks[0]
        mask = S.mask_of(shape)
        land = [(i, j) for i in range(b.nx_start, b.nx_end + 1) for j in range(b.ny_start, b.ny_end + 1)
                if mask[i - 1, j - 1] != 0]
        assert land
        rng = np.random.default_rng(17)
        pts = [(0, b.nx_start + 7, b.ny_start + 5), (0, b.bnd_x1, b.bnd_y1), (0, b.bnd_x2, b.bnd_y2),
               (0, b.bnd_x1, b.bnd_y2), (0, b.bnd_x2, b.bnd_y1), (0,) + land[0], (0,) + land[-1]]
        pts += [(0, int(rng.integers(b.bnd_x1, b.bnd_x2 + 1)), int(rng.integers(b.bnd_y1, b.bnd_y2 + 1)))
                for _ in range(300 - len(pts))]
        got = e.sample("ssh", pts, members=[2, 0])
        pending = _pending(e)
        l0 = _lib.launch_count()
        again = e.sample("ssh", pts, members=[2, 0])
        launches = _lib.launch_count() - l0
        one = e.sample("ubrtr", pts[2:3])
        full = e.sample("ssh", pts)
        d = {nm: [m.download(0, nm) for m in e.members] for nm in ("ssh", "ubrtr")}

        def want(nm, idx, points):
            return np.array([[d[nm][m][i - b.bnd_x1, j - b.bnd_y1] for m in idx] for (_, i, j) in points])
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert pending == [False, True, False], pending
    assert launches == 1, launches
    assert got.shape == (300, 2) and got.dtype == np.float64
    assert T.bits_equal(got, want("ssh", (0, 2), pts)) and T.bits_equal(again, got)
    assert one.shape == (1, 3) and T.bits_equal(one, want("ubrtr", (0, 1, 2), pts[2:3]))
    assert T.bits_equal(full, want("ssh", (0, 1, 2), pts))
    assert st == [OK] * 3 and not bad, (st, bad)


# ---------------------------------------------------------------- 8. errors change nothing
def test_errors_change_nothing(amd):
    """Every OCN_ERR_ARG case of both entries: nothing written to host, the pending tails still pending,
    and every member still its oracle run."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 2, [2, 5]
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        b = e.members[0].blocks[0]
        ssh, lu, ff1 = _lib.FIELD_ID["ssh"], _lib.FIELD_ID["lu"], _lib.FIELD_ID["ff1_1"]
        i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
        host = np.full(8, -7.0)
        hp = host.ctypes.data_as(C.c_void_p)
        k0, i0, j0 = i32(0, 0), i32(b.nx_start, b.nx_start), i32(b.ny_start, b.ny_start)
        none = (C.c_uint8 * 2)(0, 0)
        sample = {"null ensemble": (None, ssh, None, 2, k0, i0, j0, hp), "null k": (e.ens, ssh, None, 2, None, i0, j0, hp),
                  "null i": (e.ens, ssh, None, 2, k0, None, j0, hp), "null j": (e.ens, ssh, None, 2, k0, i0, None, hp),
                  "null host": (e.ens, ssh, None, 2, k0, i0, j0, None), "npts 0": (e.ens, ssh, None, 0, k0, i0, j0, hp),
                  "npts 65537": (e.ens, ssh, None, 65537, k0, i0, j0, hp),
                  "k -1": (e.ens, ssh, None, 2, i32(0, -1), i0, j0, hp), "k 1": (e.ens, ssh, None, 2, i32(1, 0), i0, j0, hp),
                  "i low": (e.ens, ssh, None, 2, k0, i32(b.nx_start, b.bnd_x1 - 1), j0, hp),
                  "i high": (e.ens, ssh, None, 2, k0, i32(b.bnd_x2 + 1, b.nx_start), j0, hp),
                  "j low": (e.ens, ssh, None, 2, k0, i0, i32(b.bnd_y1 - 1, b.ny_start), hp),
                  "j high": (e.ens, ssh, None, 2, k0, i0, i32(b.ny_start, b.bnd_y2 + 1), hp),
                  "real(4) field": (e.ens, lu, None, 2, k0, i0, j0, hp), "absent field": (e.ens, ff1, None, 2, k0, i0, j0, hp),
                  "no member": (e.ens, ssh, none, 2, k0, i0, j0, hp)}
        for what, args in sample.items():
            assert L.ocn_ens_sample(*args) == ERR_ARG, what
            assert (host == -7.0).all(), what
        w = np.eye(2)
        wp = w.ctypes.data_as(C.c_void_p)
        nan, inf = np.array([[1.0, np.nan], [0.0, 1.0]]), np.array([[1.0, 0.0], [-np.inf, 1.0]])
        transform = {"null ensemble": (None, i32(ssh), 1, None, wp), "null list": (e.ens, None, 1, None, wp),
                     "null w": (e.ens, i32(ssh), 1, None, None), "nfields 0": (e.ens, i32(ssh), 0, None, wp),
                     "real(4) id": (e.ens, i32(ssh, lu), 2, None, wp), "absent id": (e.ens, i32(ff1), 1, None, wp),
                     "repeated id": (e.ens, i32(ssh, _lib.FIELD_ID["ubrtr"], ssh), 3, None, wp),
                     "no member": (e.ens, i32(ssh), 1, none, wp),
                     "NaN weight": (e.ens, i32(ssh), 1, None, nan.ctypes.data_as(C.c_void_p)),
                     "Inf weight": (e.ens, i32(ssh), 1, None, inf.ctypes.data_as(C.c_void_p))}
        l0 = _lib.launch_count()
        for what, args in transform.items():
            assert L.ocn_ens_transform(*args) == ERR_ARG, what
        assert _lib.launch_count() == l0
        # the wrapper checks shape, dtype and finiteness before the call
        for bad_w, exc in ((np.eye(3), ValueError), (np.eye(2, dtype=np.float32), TypeError), (nan, ValueError),
                           (np.ones(4), ValueError)):
            with pytest.raises(exc):
                e.transform(bad_w)
        with pytest.raises(amd.OcnError) as ei:
            e.transform(np.eye(2), names=("ssh", "ssh"))
        assert ei.value.code == ERR_ARG
        with pytest.raises(amd.OcnError) as ei:
            e.sample("ssh", [(0, b.bnd_x2 + 1, b.ny_start)])
        assert ei.value.code == ERR_ARG
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert pending == [True, True], pending
    assert st == [OK] * 2 and not bad, (st, bad)
