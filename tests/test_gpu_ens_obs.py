"""GPU tests of the sparse linear observation operators on the device (ocn_ens_sample_h, ocn_ens_assimilate_h;
ens_assim.hip k_ens_sample_h and k_ens_obs_space_h in front of ens_local.hip k_ens_local) and of
OceanEnsemble.sample_h / assimilate_h.

The reference is the numpy restatement of the contract (tests/ens_obs_ref.py: ens_obs_rule.apply, itself checked
against a scalar loop by tests/test_ens_obs_cpu.py, then the ordered observation-space loop at the anchors and
the update's rule) on the members' own downloads, or on the CPU oracle's fields; shapes, inputs and helpers are
those of tests/test_gpu_ens_assim.py.  Every comparison is bitwise on whole arrays (NaN by position).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import ens_obs_ref as O
from tests import shapes as S
from tests.test_gpu_ens_assim import STAGE_LAUNCHES, THREADS, _obs_values, _points
from tests.test_gpu_ens_local import OBS_61x9, _oracle_update, _ring_mismatches
from tests.test_gpu_ens_transform import _bad_vs, _downloads, _oracles, _pending, _run
from tests.test_gpu_ensemble import _bad, _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, 1
STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")
BASIN_61x9 = (65, 13)   # Shape(61, 9): the array, rings included, is the basin


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


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


def _bilinear_61x9(name, nobs, seed):
    """nobs positions over the whole array of Shape(61, 9), rings and land included; every fourth one on a grid
    line or a grid point."""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(1.0, 64.99, nobs), rng.uniform(1.0, 12.99, nobs)], axis=1)
    xy[3::8, 0] = np.floor(xy[3::8, 0])
    xy[7::8] = np.floor(xy[7::8])
    return O.bilinear(name, xy, shape=BASIN_61x9)


def _assim_h_vs_restatement(e, op, taper, names, members=None, seed=0, values=None, variances=None):
    """assimilate_h(device=True) against the restatement on the members' own downloads, on every block.
    Returns (what differs, the launches of the call, the returned dict, sample_h() before)."""
    from ocean_model_arch_amd import _lib
    idx = list(range(len(e))) if members is None else sorted(set(members))
    blocks = e.members[0].blocks
    held = tuple(dict.fromkeys(tuple(names) + op.names))
    before = O.downloads(e, held, idx)
    hx0 = e.sample_h(op, members=members)
    bad = []
    if not O.bits_equal(hx0, O.apply(op, before, blocks, e.block_of)):
        bad.append("sample_h() before is not the restatement on the downloads")
    if values is None:
        values, variances = _obs_values(hx0, seed)
    l0 = _lib.launch_count()
    got = e.assimilate_h(op, values, variances, taper, names=names, members=members, device=True)
    launches = _lib.launch_count() - l0
    yz = e.assimilate_results(("y", "z"))
    _, Y, Z, ref, want = O.analysis(op, before, blocks, e.block_of, values, variances, taper, names)
    if set(got) != set(O.KEYS) | {"nonfinite"}:
        bad.append(f"keys {sorted(got)}")
    bad += O.info_mismatches(got, ref)
    bad += [nm for nm, a, r in (("Y", yz["y"], Y), ("Z", yz["z"], Z)) if not O.bits_equal(a, r)]
    if got["nonfinite"] != ref["nonfinite"]:
        bad.append(f"nonfinite {got['nonfinite']} != {ref['nonfinite']}")
    after = O.downloads(e, held, idx)
    for nm in held:
        for b in blocks:
            w = want[nm][b.k] if nm in names else before[nm][b.k]
            bad += [f"member {i} [{b.k}]:{nm}" for i, g, v in zip(idx, after[nm][b.k], w) if not O.bits_equal(g, v)]
    return bad, launches, got, hx0


# ---------------------------------------------------------------- 1. the operator alone
def _sample_h_vs_downloads(e, n, members=None):
    """sample_h() over n members of an ensemble of Shape(61, 9) -- the first n (all of them: `use` NULL), or the n
    `members` -- against the restatement on their downloads, and points() rows against sample()."""
    if members is None:
        members = None if n == len(e) else range(n)
    idx = list(range(len(e))) if members is None else sorted(set(members))
    assert len(idx) == n
    rng = np.random.default_rng(n)
    names = ("ssh", "ubrtr", "vbrtr")
    rows = [[("ssh", 30, 6, 1.0)], [("ssh", 1, 1, -0.5)],
            [("ubrtr", 64, 12, 0.25), ("ubrtr", 65, 12, 0.25), ("ubrtr", 64, 13, 0.25), ("ubrtr", 65, 13, 0.25)],
            [(names[t % 3], int(rng.integers(1, 66)), int(rng.integers(1, 14)), float(rng.uniform(-1, 1))) for t in range(16)],
            [("vbrtr", 2, 2, 1e-3), ("ssh", 2, 2, 1e3), ("vbrtr", 2, 2, -7.0)]]
    rows += [[(names[(r + t) % 3], int(rng.integers(1, 66)), int(rng.integers(1, 14)), float(rng.uniform(-1, 1)))
              for t in range(1 + r % 16)] for r in range(300)]          # more than one workgroup of rows
    op = O.ObsOperator.from_rows(rows, np.full((len(rows), 2), 5))
    got = e.sample_h(op, members=members)
    want = O.apply(op, O.downloads(e, names, idx), e.members[0].blocks, e.block_of)
    assert got.shape == (len(rows), n) and O.bits_equal(got, want)
    unit = e.sample_h(O.points("ubrtr", OBS_61x9), members=members)
    assert O.bits_equal(unit, e.sample("ubrtr", _points(e, OBS_61x9), members=members))


@pytest.mark.parametrize("n", [2, 9, 33])
def test_sample_h(amd, ens33, n):
    """Rows of 1, 4 and 16 terms over three fields, terms in the outer rings (halo and land) and repeated:
    sample_h() is the restatement on the members' downloads; points() rows are sample()."""
    _sample_h_vs_downloads(ens33, n)


# ---------------------------------------------------------------- 2. unit rows are the grid-point entry
def test_unit_rows(amd):
    """assimilate_h(points("ssh", OBS)) and assimilate("ssh", OBS) on two identically started ensembles: every
    field of every member, Y, Z, hx, the innovations and the spreads bit for bit, and the same launches."""
    from ocean_model_arch_amd import _lib
    taper = O.taper_table(6.0)
    es = [_start(amd, S.Shape(61, 9), ["noise"] * 5) for _ in range(2)]
    try:
        for e in es:
            _run(e, [2, 3])
        prior = [e.sample("ssh", _points(e, OBS_61x9)) for e in es]      # (the tails formed in both)
        assert O.bits_equal(prior[0], prior[1])
        values, variances = _obs_values(prior[0], 2)
        l0 = _lib.launch_count()
        a = es[0].assimilate("ssh", OBS_61x9, values, variances, taper, device=True)
        l1 = _lib.launch_count()
        ra = es[0].assimilate_results(("y", "z"))
        l2 = _lib.launch_count()
        b = es[1].assimilate_h(O.points("ssh", OBS_61x9), values, variances, taper, device=True)
        l3 = _lib.launch_count()
        rb = es[1].assimilate_results(("y", "z"))
        fa, fb = (_downloads(e, STATE, range(5)) for e in es)
    finally:
        for e in es:
            e.close()
    assert l1 - l0 == l3 - l2 == len(STATE) + STAGE_LAUNCHES
    assert set(a) == set(b) and a["nonfinite"] == b["nonfinite"] == 0
    assert not O.info_mismatches(a, b)
    assert O.bits_equal(ra["y"], rb["y"]) and O.bits_equal(ra["z"], rb["z"])
    assert not [(nm, i) for nm in STATE for i in range(5) if not O.bits_equal(fa[nm][i], fb[nm][i])]


# ---------------------------------------------------------------- 3. bilinear rows: member counts, rows per thread
@pytest.mark.parametrize("n", [2, 5, 8, 9, 32, 33])
def test_bilinear_member_counts(amd, ens33, n):
    """n members in use, across the update's register / LDS boundary (32 / 33), 11 bilinear observations of ssh,
    a Gaspari-Cohn and a ringed taper in turn.  The members not in use keep their bits; the launches are the
    update's plus STAGE_LAUNCHES."""
    e = ens33
    names = ("ssh", "ubrtr")
    members = None if n == 33 else range(n)
    outside = None if n == 33 else e.members[32].download(0, "ssh")
    for t, (what, taper) in enumerate([("gaspari-cohn", O.taper_table(6.0)), ("ring", O.ringed_taper(50))]):
        op = _bilinear_61x9("ssh", 11, 10 * n + t)
        bad, launches, got, hx0 = _assim_h_vs_restatement(e, op, taper, names, members, seed=10 * n + t)
        assert not bad, (what, bad)
        assert launches == len(names) * 1 + STAGE_LAUNCHES, what
        assert got["hx"].shape == (11, n) and not O.bits_equal(got["hx"], hx0)
    if outside is not None:
        assert O.bits_equal(e.members[32].download(0, "ssh"), outside)


@pytest.mark.parametrize("nobs", [1, THREADS + 1])
def test_bilinear_rows_per_thread(amd, nobs):
    """1 and THREADS + 1 bilinear observations: threads that own zero, one and two rows, and in the prologue
    the last partial stride over (observation, member)."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 8)
    try:
        _run(e, [2, 3])
        bad, launches, got, _ = _assim_h_vs_restatement(e, _bilinear_61x9("ssh", nobs, nobs), O.taper_table(6.0),
                                                        ("ssh", "ubrtr"), seed=nobs)
    finally:
        e.close()
    assert not bad, bad
    assert launches == 2 + STAGE_LAUNCHES
    assert got["hx"].shape == (nobs, 8) and got["nonfinite"] == 0


# ---------------------------------------------------------------- 4. two fields in one row
def test_two_fields_in_one_row(amd):
    """Radial velocities cos(theta) u + sin(theta) v of bilinearly interpolated ubrtr and vbrtr, updating ssh,
    ubrtr and vbrtr."""
    e = _start(amd, S.Shape(61, 9), ["noise"] * 5)
    try:
        _run(e, [2, 3])
        rng = np.random.default_rng(4)
        xy = np.stack([rng.uniform(3.0, 62.9, 9), rng.uniform(3.0, 10.9, 9)], axis=1)
        theta = rng.uniform(0.0, 2.0 * np.pi, 9)
        op = O.combine([O.bilinear("ubrtr", xy, shape=BASIN_61x9), O.bilinear("vbrtr", xy, shape=BASIN_61x9)],
                       [np.cos(theta), np.sin(theta)])
        assert op.names == ("ubrtr", "vbrtr") and int(op.start[-1]) == 72
        bad, launches, got, hx0 = _assim_h_vs_restatement(e, op, O.taper_table(6.0), ("ssh", "ubrtr", "vbrtr"), seed=4)
    finally:
        e.close()
    assert not bad, bad
    assert launches == 3 + STAGE_LAUNCHES and not O.bits_equal(got["hx"], hx0)


# ---------------------------------------------------------------- 5. a block grid
def test_block_grid(amd):
    """A 2 x 2 block grid, 5 members: the first observation's four corners lie in four different blocks, others
    sit on the seams and in the basin's outer ring; every block against the restatement, and the halo rings
    coherent before and after."""
    names = ("ssh", "ubrtr")
    e = _start(amd, S.Shape(17, 19, (2, 2)), ["noise"] * 5)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 5
        blocks = e.members[0].blocks
        assert len(blocks) == 4
        sx, sy = max(b.nx_start for b in blocks), max(b.ny_start for b in blocks)
        xy = np.array([[sx - 0.5, sy - 0.25], [3.3, 3.7], [sx - 1.0, sy + 0.5], [1.5, 12.0], [19.2, 21.9], [sx + 2.25, 4.5]])
        op = O.bilinear("ssh", xy, shape=(21, 23))
        assert len({e.block_of(i, j) for _, i, j, _ in op.row(0)}) == 4
        was, _ = _ring_mismatches(e, names, range(5))
        bad, launches, _, _ = _assim_h_vs_restatement(e, op, O.ringed_taper(10, 3), names, seed=3)
        lost, _ = _ring_mismatches(e, names, range(5))
        bad2, launches2, _, _ = _assim_h_vs_restatement(e, op, O.taper_table(9.0), names, seed=4)
        lost2, _ = _ring_mismatches(e, names, range(5))
    finally:
        e.close()
    assert not was and not bad and not bad2, (was, bad, bad2)
    assert not lost and not lost2, (lost, lost2)
    assert launches == launches2 == len(names) * 4 + STAGE_LAUNCHES


# ---------------------------------------------------------------- 6. pending tails, the upload rule, a subset
def test_continue_as_the_oracle_continues(amd):
    """9 members after calls [2, 5]: the tails pending, the pair roles swapped.  The analysis over all members
    but one, then 4 more steps: every field of every member equals the oracle run 7 steps, updated by the
    restatement from H of the oracle's own fields, run 4 steps more; only the tails of the members in use were
    formed."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 9, [2, 5]
    use = [0, 1, 2, 3, 5, 6, 7, 8]
    taper = O.taper_table(6.0)
    op = _bilinear_61x9("ssh", 11, 6)
    oms = _oracles(shape, classes, sum(calls))
    ob = oms[0].blocks[0]
    oblocks = [SimpleNamespace(k=0, bnd_x1=ob.bx1, bnd_y1=ob.by1)]
    hx = O.apply(op, {"ssh": {0: [oms[i].f[0]["ssh"] for i in use]}}, oblocks, lambda i, j: 0)
    values, variances = _obs_values(hx, 5)
    Y, Z, ref = O.ensrf_obs_space_ordered(hx, op.anchors, values, variances, taper)
    e = _start(amd, shape, classes)
    try:
        _run(e, calls)
        assert _pending(e) == [True] * 9
        got = e.assimilate_h(op, values, variances, taper, members=use, device=True)
        pending = _pending(e)
        e.step(4)
        e.complete()
        st = e.synchronize()
        _oracle_update(oms, Y, Z, op.anchors, taper, STATE, members=use)
        for om in oms:
            om.run(4, 1.0)
        bad = _bad_vs(e, oms)
    finally:
        e.close()
    assert pending == [i == 4 for i in range(9)], pending
    assert not O.info_mismatches(got, ref) and got["nonfinite"] == 0
    assert st == [OK] * 9 and not bad, (st, bad)


# ---------------------------------------------------------------- 7. non-finite values
def test_nonfinite(amd):
    """A NaN in one member's ssh at one corner of one observation: counted, and it propagates by position as
    the restatement says.  The same call on a fresh ensemble with that member left out by `use`: no count."""
    shape, classes = S.Shape(61, 9), ["noise"] * 6
    taper = O.taper_table(6.0)
    op = O.bilinear("ssh", [[29.5, 5.5], [12.25, 3.0], [47.0, 5.75], [58.5, 9.5]], shape=BASIN_61x9)
    counts, bads = [], []
    for members in (None, [0, 1, 2, 4, 5]):
        e = _start(amd, shape, classes)
        try:
            _run(e, [2, 3])
            b = e.members[0].blocks[0]
            a = e.members[3].download(0, "ssh")
            a[30 - b.bnd_x1, 6 - b.bnd_y1] = np.nan
            e.members[3].upload(0, "ssh", a)
            clean = e.sample_h(op, members=[0, 1, 2, 4, 5])
            values, variances = _obs_values(clean, 7)
            bad, _, got, hx0 = _assim_h_vs_restatement(e, op, taper, ("ssh", "ubrtr"), members, values=values,
                                                       variances=variances)
        finally:
            e.close()
        counts.append(got["nonfinite"])
        bads.append(bad)
        if members is None:
            assert np.isnan(hx0[0, 3]) and np.isfinite(np.delete(hx0, 3, axis=1)).all()
    assert counts[0] >= 1 and counts[1] == 0, counts
    assert not bads[0] and not bads[1], bads


# ---------------------------------------------------------------- 8. the Python driver
def test_python_driver(amd):
    """device=False is sample_h() + ens_local_rule.ensrf_obs_space at the anchors + local_update() by hand, and
    rtps=0.5 is spread_save() + assimilate_h() + inflate() on both paths: one ensemble, restored by upload
    between the runs.  More than 8192 observations are refused on both paths."""
    from ocean_model_arch_amd import ens_local_rule
    e = _start(amd, S.Shape(61, 9), ["noise"] * 5)
    try:
        _run(e, [2, 3])
        op = _bilinear_61x9("ssh", 11, 8)
        taper = amd.ensemble.taper_table(6.0)
        start = _downloads(e, STATE, range(5))
        values, variances = _obs_values(e.sample_h(op), 8)

        def run(f):
            for nm in STATE:
                for m, a in zip(e.members, start[nm]):
                    m.upload(0, nm, a)
            info = f()
            return info, _downloads(e, STATE, range(5))

        def by_hand():
            Y, Z, info = ens_local_rule.ensrf_obs_space(e.sample_h(op), op.anchors, values, variances, taper)
            e.local_update(Y, Z, op.anchors, taper)
            return info

        def relaxed(device):
            e.spread_save(STATE)
            info = e.assimilate_h(op, values, variances, taper, device=device)
            e.inflate(0.5, "rtps", STATE)
            return info
        pairs = [(run(lambda: e.assimilate_h(op, values, variances, taper)), run(by_hand))]
        for device in (False, True):
            pairs.append((run(lambda: e.assimilate_h(op, values, variances, taper, device=device, rtps=0.5)),
                          run(lambda: relaxed(device))))
        big = O.points("ssh", np.full((8193, 2), 5))
        for device in (False, True):
            with pytest.raises(ValueError):
                e.assimilate_h(big, np.zeros(8193), np.ones(8193), np.array([1.0]), device=device)
        with pytest.raises(TypeError):
            e.assimilate_h(OBS_61x9, values, variances, taper)
    finally:
        e.close()
    for (ia, fa), (ib, fb) in pairs:
        assert set(ia) == set(ib) >= set(O.KEYS) and not O.info_mismatches(ia, ib)
        assert not [(nm, i) for nm in STATE for i in range(5) if not O.bits_equal(fa[nm][i], fb[nm][i])]
    assert not all(O.bits_equal(a, c) for a, c in zip(pairs[0][0][1]["ssh"], start["ssh"]))   # (something happened)
    assert not all(O.bits_equal(a, c) for a, c in zip(pairs[0][0][1]["ssh"], pairs[1][0][1]["ssh"]))   # (and rtps, too)


# ---------------------------------------------------------------- 9. errors change nothing
def _error_cases(e, keep):
    """(the valid arguments, {what: the arguments that change}) of ocn_ens_assimilate_h on Shape(61, 9), 3 members."""
    from ocean_model_arch_amd import _lib
    ssh, sshp, ub, ubp, vb, lu, ff1 = (_lib.FIELD_ID[nm] for nm in ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "lu", "ff1_1"))
    i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    val, var, tw = np.array([0.1, -0.2]), np.array([0.01, 0.02]), np.array([1.0, 0.5, -0.25])
    big_i = np.full(8193, 5, dtype=np.int32)
    big_start = np.arange(8194, dtype=np.int32)
    big = np.ones(8193)
    taper, long_taper = np.array([1.0, 0.5, 0.25]), np.ones(65537)
    five, ones17 = np.full(17, 5, dtype=np.int32), np.ones(17)
    keep += [val, var, tw, big_i, big_start, big, taper, long_taper, five, ones17]

    def changed(a, at, v):
        a = a.copy()
        a[at] = v
        keep.append(a)
        return ptr(a)
    ok = dict(ens=e.ens, ids=i32(ssh), nf=1, use=None, nobs=2, io=i32(5, 9), jo=i32(4, 6), st=i32(0, 1, 3), tf=i32(ssh, ssh, ub),
              ti=i32(5, 9, 10), tj=i32(4, 6, 6), tw=ptr(tw), v=ptr(val), r=ptr(var), t=ptr(taper), nt=3)
    many = dict(nobs=1, st=i32(0, 17), tf=ptr(np.full(17, ssh, dtype=np.int32)), ti=ptr(five), tj=ptr(five), tw=ptr(ones17))
    keep.append(many)
    cases = {"null ensemble": dict(ens=None), "null list": dict(ids=None), "null io": dict(io=None), "null jo": dict(jo=None),
             "null start": dict(st=None), "null tfield": dict(tf=None), "null ti": dict(ti=None), "null tj": dict(tj=None),
             "null tw": dict(tw=None), "null value": dict(v=None), "null variance": dict(r=None), "null taper": dict(t=None),
             "nfields 0": dict(nf=0), "real(4) id": dict(ids=i32(ssh, lu), nf=2), "absent id": dict(ids=i32(ff1)),
             "repeated id": dict(ids=i32(ssh, ub, ssh), nf=3),
             "one member": dict(use=(C.c_uint8 * 3)(0, 1, 0)), "no member": dict(use=(C.c_uint8 * 3)(0, 0, 0)),
             "nobs 0": dict(nobs=0),
             "nobs 8193": dict(nobs=8193, io=ptr(big_i), jo=ptr(big_i), st=ptr(big_start), tf=ptr(np.full(8193, ssh, dtype=np.int32)),
                               ti=ptr(big_i), tj=ptr(big_i), tw=ptr(big), v=ptr(big), r=ptr(big)),
             "anchor io 0": dict(io=i32(5, 0)), "anchor io nx + 1": dict(io=i32(66, 9)), "anchor jo 0": dict(jo=i32(0, 6)),
             "anchor jo ny + 1": dict(jo=i32(4, 14)), "ntaper 0": dict(nt=0), "ntaper 65537": dict(t=ptr(long_taper), nt=65537),
             "start[0] 1": dict(st=i32(1, 2, 3)), "a row of 0 terms": dict(st=i32(0, 0, 3)), "a last row of 0 terms": dict(st=i32(0, 3, 3)),
             "a row of -1 terms": dict(st=i32(0, 2, 1)), "a row of 17 terms": many,
             "real(4) term field": dict(tf=i32(ssh, lu, ub)), "absent term field": dict(tf=i32(ssh, ssh, ff1)),
             "5 distinct fields": dict(st=i32(0, 2, 5), tf=i32(ssh, sshp, ub, ubp, vb), ti=i32(5, 5, 5, 5, 5), tj=i32(4, 4, 4, 4, 4),
                                       tw=ptr(ones17)),
             "term i 0": dict(ti=i32(5, 0, 10)), "term i nx + 1": dict(ti=i32(5, 9, 66)), "term j 0": dict(tj=i32(0, 6, 6)),
             "term j ny + 1": dict(tj=i32(4, 6, 14))}
    keep.append(cases)
    for v in (0.0, -0.0, np.nan, np.inf, -np.inf):
        cases[f"weight {v}"] = dict(tw=changed(tw, 2, v))
    for v in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        cases[f"variance {v}"] = dict(r=changed(var, 1, v))
    for v in (np.nan, np.inf, -np.inf):
        cases[f"value {v}"] = dict(v=changed(val, 1, v))
        cases[f"{v} in taper"] = dict(t=changed(taper, 2, v))
    return ok, cases


def _all_refused(L, ok, cases):
    """Every case through both entries: what was not refused with OCN_ERR_ARG."""
    wrong = []
    out = np.full(64, 7.5)
    sample_only = {"null ensemble", "null start", "null tfield", "null ti", "null tj", "null tw", "no member", "nobs 0"}
    for what, change in cases.items():
        a = {**ok, **change}
        rc = L.ocn_ens_assimilate_h(a["ens"], a["ids"], a["nf"], a["use"], a["nobs"], a["io"], a["jo"], a["st"], a["tf"], a["ti"],
                                    a["tj"], a["tw"], a["v"], a["r"], a["t"], a["nt"])
        if rc != ERR_ARG:
            wrong.append(("assimilate_h", what, rc))
        if what in sample_only or set(change) <= {"st", "tf", "ti", "tj", "tw"} or what == "a row of 17 terms":
            rc = L.ocn_ens_sample_h(a["ens"], a["use"], a["nobs"], a["st"], a["tf"], a["ti"], a["tj"], a["tw"],
                                    out.ctypes.data_as(C.c_void_p))
            if rc != ERR_ARG or not (out == 7.5).all():
                wrong.append(("sample_h", what, rc))
    a = ok
    if L.ocn_ens_sample_h(a["ens"], a["use"], a["nobs"], a["st"], a["tf"], a["ti"], a["tj"], a["tw"], None) != ERR_ARG:
        wrong.append(("sample_h", "null host"))
    if L.ocn_ens_sample_h(a["ens"], a["use"], 65537, a["st"], a["tf"], a["ti"], a["tj"], a["tw"], out.ctypes.data_as(C.c_void_p)) != ERR_ARG:
        wrong.append(("sample_h", "nobs 65537"))
    return wrong


def test_errors_change_nothing(amd):
    """Every OCN_ERR_ARG case of the contract through ctypes.  Before any successful call: return code 1, nothing
    launched, the pending tails still pending, every member still its oracle run, no result to read.  After a
    successful call: return code 1, nothing launched, no field bit changed, and that call's results still there."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 5]
    e = _start(amd, shape, classes)
    keep = []
    try:
        _run(e, calls)
        ok, cases = _error_cases(e, keep)
        out = np.zeros(64)
        l0 = _lib.launch_count()
        wrong = _all_refused(L, ok, cases)
        assert L.ocn_ens_assimilate_result(e.ens, 0, out.ctypes.data_as(C.c_void_p)) == ERR_ARG     # still no successful call
        with pytest.raises(amd.OcnError) as ei:
            e.assimilate_h(O.points("ssh", [[5, 4], [66, 6]]), [0.1, 0.2], [0.01, 0.01], np.array([1.0]), device=True)
        assert ei.value.code == ERR_ARG
        launched = _lib.launch_count() - l0
        pending = _pending(e)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
        # after a successful call
        op = O.ObsOperator.from_rows([[("ssh", 5, 4, 1.0)], [("ssh", 9, 6, 0.5), ("ubrtr", 10, 6, -0.25)]], [[5, 4], [9, 6]])
        e.assimilate_h(op, [0.1, -0.2], [0.01, 0.02], np.array([1.0, 0.5, 0.25]), names=("ssh",), device=True)
        what = ("hx", "y", "z", "innovations", "prior_spread", "posterior_spread")
        res0 = e.assimilate_results(what)
        held = _downloads(e, STATE, range(3))
        l1 = _lib.launch_count()
        wrong2 = _all_refused(L, ok, cases)
        launched2 = _lib.launch_count() - l1
        res1 = e.assimilate_results(what)
        now = _downloads(e, STATE, range(3))
        rc_ok = L.ocn_ens_assimilate_h(*[ok[k] for k in ("ens", "ids", "nf", "use", "nobs", "io", "jo", "st", "tf", "ti", "tj", "tw",
                                                         "v", "r", "t", "nt")])
        res2 = e.assimilate_results(what)
        del keep
    finally:
        e.close()
    assert not wrong and launched == 0, (wrong, launched)
    assert pending == [True] * 3, pending
    assert st == [OK] * 3 and not bad, (st, bad)
    assert not wrong2 and launched2 == 0, (wrong2, launched2)
    assert all(O.bits_equal(res0[k], res1[k]) for k in what)
    assert not [(nm, i) for nm in STATE for i in range(3) if not O.bits_equal(held[nm][i], now[nm][i])]
    assert rc_ok == OK and not O.bits_equal(res2["hx"], res1["hx"])       # (the valid arguments do go through)


def test_term_in_a_dropped_block(amd):
    """S.DROPPED's missing middle block: a term at (20, 20) is in the basin and in no local block's array --
    OCN_ERR_ARG from both entries, nothing launched, no bit changed; an ANCHOR there is allowed."""
    from ocean_model_arch_amd import _lib
    e = _start(amd, S.DROPPED, ["noise"] * 3)
    try:
        _run(e, [2, 3])
        e.complete()
        assert e.synchronize() == [OK] * 3
        taper = O.ringed_taper(10, 5)
        before = {b.k: _downloads(e, ("ssh",), range(3), b.k) for b in e.members[0].blocks}
        l0 = _lib.launch_count()
        lost = O.ObsOperator.from_rows([[("ssh", 38, 38, 1.0)], [("ssh", 37, 37, 0.5), ("ssh", 20, 20, 0.5)]], [[38, 38], [37, 37]])
        with pytest.raises(amd.OcnError) as ei:
            e.assimilate_h(lost, [0.1, 0.1], [0.01, 0.01], taper, names=("ssh",), device=True)
        with pytest.raises(amd.OcnError) as es:
            e.sample_h(lost)
        none = _lib.launch_count() - l0
        after = {b.k: _downloads(e, ("ssh",), range(3), b.k) for b in e.members[0].blocks}
        op = O.ObsOperator.from_rows([[("ssh", 38, 38, 0.5), ("ssh", 39, 38, 0.5)]], [[20, 20]])
        bad, launches, _, _ = _assim_h_vs_restatement(e, op, O.taper_table(30.0), ("ssh",), seed=9)
    finally:
        e.close()
    assert ei.value.code == es.value.code == ERR_ARG and none == 0
    assert all(O.bits_equal(a, c) for k in before for a, c in zip(before[k]["ssh"], after[k]["ssh"]))
    assert not bad and launches >= 1 + STAGE_LAUNCHES, (bad, launches)
