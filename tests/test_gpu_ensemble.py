"""GPU tests of the ensemble launch (ocn_ens_*, sw_kernels.hip k_march_multi_b): the members of an
ensemble that would each run a multi-step launch go as one launch per group, each member with a grid
barrier of its own inside it.

The reference is always the CPU oracle (tests/shapes.py oracle_model and its input classes, with a seed
offset per member so that the members differ in their bits) or, for the Black Sea, the golden digests
of the compiled reference; every field of every member is compared bitwise after complete().  Two
paths of the library are never compared with each other.  A batched launch needs what a multi-step
launch needs: an open sequence and a variant chosen on the host, so every run makes a first short call
and a synchronize() first.  Tolerance: none.
"""
import functools

import pytest

from tests import shapes as S
from tests.golden import cases
from tests.test_gpu_parity import compare_case

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_HIP, ERR_BLOWUP = 0, 1, 2, 5


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


# ---------------------------------------------------------------- inputs and references per member
@functools.lru_cache(maxsize=64)
def member_uploads(shape, cls, off, params=None):
    """The class's uploads (tests/shapes.py uploads) with every field's seed moved by `off`."""
    seeds = S.SEEDS
    S.SEEDS = {nm: s + off for nm, s in seeds.items()}
    try:
        return S.uploads(cls, S.oracle_model(shape, params=params))
    finally:
        S.SEEDS = seeds


@functools.lru_cache(maxsize=64)
def member_reference(shape, cls, off, steps, params=None):
    """{(bm, bn): {field: array}} of the oracle after `steps` steps from the member's inputs (at the
    parameter set's tau, grid and SW keywords; None: the defaults, tau = 1); computed once per key, never
    written by the callers."""
    om = S.oracle_model(shape, params=params)
    for k, b in enumerate(om.blocks):
        for nm, a in member_uploads(shape, cls, off, params).get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    om.run(steps, S.tau_of(params))
    return {(b.bm, b.bn): om.f[k] for k, b in enumerate(om.blocks)}


def _ensemble(amd, shape, members, params=None):
    sw = amd.SWConfig(**S.sw_kwargs(shape, params=params))
    return amd.OceanEnsemble(amd.BasinConfig(mask=S.mask_of(shape), **S.basin_kwargs(shape, params)), sw,
                             amd.ParallelConfig(*shape.grid), members=members)


def _upload(m, ups):
    for b in m.blocks:
        for nm, a in ups.get((b.bm, b.bn), {}).items():
            m.upload(b.k, nm, a)


def _start(amd, shape, classes, params=None):
    """An initialised ensemble with member i's inputs of class classes[i] (seed offset 1000 i); params: a
    parameter set of tests/shapes.py PARAMS."""
    e = _ensemble(amd, shape, len(classes), params)
    e.init()
    for i, (m, cls) in enumerate(zip(e.members, classes)):
        _upload(m, member_uploads(shape, cls, 1000 * i, params))
    return e


def _calls(e, calls, check_every=1, params=None):
    """The calls at the parameter set's tau (a synchronize() after the first: the known-constant verdicts
    reach the host); the info and the launches issued per call; then complete() and the statuses."""
    tau = S.tau_of(params)
    import ocean_model_arch_amd as amd
    infos, launches = [], []
    for i, n in enumerate(calls):
        l0 = amd._lib.launch_count()
        e.step(n, tau=tau, check_every=check_every)
        launches.append(amd._lib.launch_count() - l0)
        infos.append(e.info())
        if i == 0:
            assert e.synchronize() == [OK] * len(e)
    e.complete()
    return infos, launches, e.synchronize()


def _bad(e, shape, classes, steps, params=None):
    """Every field of every member against its own oracle run: ["member i (bm,bn):field", ...]."""
    steps = steps if isinstance(steps, (list, tuple)) else [steps] * len(classes)
    bad = []
    for i, (m, cls) in enumerate(zip(e.members, classes)):
        ref = member_reference(shape, cls, 1000 * i, steps[i], params)
        get = S.model_getter([m])
        assert get.blocks == set(ref)
        bad += [f"member {i} {x}" for x in S.mismatches(ref, get)]
    return bad


# ---------------------------------------------------------------- the cases
def test_mixed_members(amd):
    """Three variants in one ensemble (known-constant: plain and noise; h_r-read; general), an odd step
    count (the role swap) and a 1-step call, which falls back to the members' own steps."""
    shape, classes, calls = S.Shape(121, 65), ["plain", "noise", "noise", "hr", "general", "noise"], [2, 5, 1, 4]
    e = _start(amd, shape, classes)
    try:
        infos, launches, st = _calls(e, calls)
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert st == [OK] * 6 and not bad, (st, bad)
    assert [(i["groups"], i["batched"]) for i in infos] == [(0, 0), (3, 6), (0, 0), (3, 6)], infos
    assert infos[1]["rows"] == 1 and infos[1]["tiles"] == 51 and infos[1]["max_group"] == 4, infos[1]
    assert launches[1] == 3, launches   # one launch per group, nothing else


@pytest.mark.parametrize("W,H,members,cap", [(61, 9, 9, 2), (61, 9, 9, 7), (61, 9, 9, 20), (61, 9, 9, 0), (241, 151, 3, 200)])
def test_capacity_cap(amd, W, H, members, cap):
    """The capacity cap reaches several groups and taller tiles on tiny blocks: the launches are what
    ocn_ens_plan says for the same inputs (cap 2: nine launches of one member; 7: three of three at 16
    rows; 20: one of nine at 3 rows; unset: one of nine at 1 row; 241 x 151 at 200: 3 rows)."""
    from ocean_model_arch_amd.ensemble import plan
    shape, classes, calls = S.Shape(W, H), ["noise"] * members, [2, 6]
    e = _start(amd, shape, classes)
    try:
        e.set_capacity(cap)
        capacity = e.info()["capacity"]
        assert capacity == cap if cap else capacity >= 256, capacity
        want = plan(e.members[0].blocks[0].c_block(), [0] * members, capacity)
        infos, launches, st = _calls(e, calls)
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert st == [OK] * members and not bad, (st, bad)
    big = max(want, key=lambda g: len(g["members"]))
    got = infos[1]
    assert (got["groups"], got["batched"], got["rows"], got["tiles"], got["max_group"]) == \
        (len(want), members, big["rows"], big["tiles"], len(big["members"])), (got, want)
    assert launches[1] == len(want), launches
    expect = {(61, 2): (9, 16), (61, 7): (3, 16), (61, 20): (1, 3), (61, 0): (1, 1), (241, 200): (1, 3)}[(W, cap)]
    assert (len(want), big["rows"]) == expect, want


@pytest.mark.parametrize("W,H", [(1, 1), (1, 241), (241, 1)])
def test_edge_shapes(amd, W, H):
    """The smallest blocks the march accepts; 1 x 1 is a one-tile member: a barrier over one workgroup."""
    shape, classes, calls = S.Shape(W, H), ["noise"] * 3, [2, 3]
    e = _start(amd, shape, classes)
    try:
        infos, _, st = _calls(e, calls)
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert st == [OK] * 3 and not bad, (st, bad)
    assert (infos[1]["groups"], infos[1]["batched"]) == (1, 3), infos


def test_single_member(amd):
    shape, classes, calls = S.Shape(121, 65), ["noise"], [2, 5]
    e = _start(amd, shape, classes)
    try:
        infos, launches, st = _calls(e, calls)
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert st == [OK] and not bad, (st, bad)
    assert (infos[1]["groups"], infos[1]["batched"], infos[1]["max_group"]) == (1, 1, 1) and launches[1] == 1, infos


@pytest.mark.parametrize("check_every", [1, 0])
def test_blowup_isolation(amd, check_every):
    """Member 1's ssh is 2e4 at one sea point when the batched call runs: with the per-step check its
    status is OCN_ERR_BLOWUP and the others' OCN_OK, without it all are OK; members 0 and 2 are bitwise
    their oracle runs either way."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 6]
    e = _start(amd, shape, classes)
    try:
        m = e.members[1]
        ssh, lu = m.download(0, "ssh"), m.download(0, "lu")
        b = m.blocks[0]
        i, j = 30 + 2, 4 + 2   # interior point (30, 4) of the block array (two halo points each side)
        assert lu[i, j] > 0.5 and b.shape == ssh.shape
        ssh[i, j] = 2.0e4
        m.upload(0, "ssh", ssh)
        m.upload(0, "sshn", ssh)
        e.step(calls[0], tau=1.0, check_every=0)
        assert e.synchronize() == [OK] * 3
        e.step(calls[1], tau=1.0, check_every=check_every)
        info = e.info()
        e.complete()
        import ctypes as C
        raw = (C.c_int32 * 3)()
        rc = amd.lib().ocn_ens_synchronize(e.ens, raw)
        st = list(raw)
        bad = [x for x in _bad(e, shape, classes, sum(calls)) if not x.startswith("member 1 ")]
    finally:
        e.close()
    assert (info["groups"], info["batched"]) == (1, 3), info
    assert st == ([OK, ERR_BLOWUP, OK] if check_every else [OK] * 3), st
    assert rc == (ERR_BLOWUP if check_every else OK), rc
    assert not bad, bad


def test_fallback_members(amd):
    """OCN_OPT_MULTI off on member 2 and a raw pointer taken from member 3: they step on their own, the
    other two are batched; member 0 stepped alone between two ensemble calls stays bitwise."""
    shape, classes = S.Shape(121, 65), ["noise"] * 4
    e = _start(amd, shape, classes)
    try:
        e.members[2].set_multi(False)
        assert e.members[3].field_ptr(0, "ssh")
        e.step(2)
        assert e.synchronize() == [OK] * 4
        e.step(4)
        i1 = e.info()
        e.members[0].step(1)
        e.step(3)
        i2 = e.info()
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, [10, 9, 9, 9])
    finally:
        e.close()
    assert st == [OK] * 4 and not bad, (st, bad)
    assert (i1["groups"], i1["batched"]) == (1, 2) and (i2["groups"], i2["batched"]) == (1, 2), (i1, i2)


@pytest.mark.parametrize("shape", [S.Shape(17, 19, (2, 2)), S.Shape(13, 11, (1, 1), 1)], ids=lambda s: s.id)
def test_fallback_configurations(amd, shape):
    """A block grid and a tracer run: nothing is batched, every member steps as a context does."""
    classes, calls = ["noise"] * 2, [2, 3]
    e = _start(amd, shape, classes)
    try:
        infos, _, st = _calls(e, calls)
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert st == [OK] * 2 and not bad, (st, bad)
    assert all(i["batched"] == 0 and i["groups"] == 0 for i in infos), infos


def test_black_sea(amd):
    """The Black Sea as 4 members from the plain initial state: each passes the golden digests of the
    compiled reference."""
    name, calls = "bs_b1x1_s60", [2, 58]
    case = cases.load_e2e(name)
    b = case["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=case["mask"], topography=case.get("topography"))
    e = amd.OceanEnsemble(basin, amd.SWConfig(**case["sw"]), amd.ParallelConfig(*case["bxy"]), members=4)
    try:
        e.init()
        infos, launches, st = _calls(e, calls)
        bad = [f"member {i} {x}" for i, m in enumerate(e.members) for x in compare_case(m, case, name)]
    finally:
        e.close()
    assert st == [OK] * 4 and not bad, (st, bad)
    assert (infos[1]["groups"], infos[1]["batched"]) == (1, 4) and launches[1] == 1, (infos, launches)


def test_borrowed_handles(amd):
    """A member's handle is the ensemble's: ocn_ctx_destroy and the transports refuse it; close() of the
    member's OceanModel leaves it alone; the ensemble still steps."""
    import ctypes as C
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 2, [2, 3]
    e = _start(amd, shape, classes)
    try:
        L = amd.lib()
        ctx = e.members[0].ctx
        assert L.ocn_ctx_destroy(ctx) == ERR_ARG
        assert L.ocn_ctx_attach_comm(ctx, C.create_string_buffer(128), 128) == ERR_ARG
        assert L.ocn_ctx_attach_loopback((C.c_void_p * 1)(ctx.value), 1) == ERR_ARG
        infos, _, st = _calls(e, calls)
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert st == [OK] * 2 and not bad, (st, bad)
    assert infos[1]["batched"] == 2, infos
