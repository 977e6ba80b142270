"""GPU tests of the station recorder (ocn_ens_record_*, ocn_ens_step_record; sw_kernels.hip k_march_multi_rec
behind OceanEnsemble.record / step_record / series).

The reference is the CPU oracle only: tests/shapes.py oracle_model with tests/test_gpu_ensemble.py's
member_uploads, stepped one om.step(tau) at a time; after every due step the numpy restatement of the
operator (ens_obs_rule.apply) is applied to the oracle's arrays.  Every comparison is bitwise (NaN by
position).  The in-launch route and the chunked route are never compared with each other.  A recording
launch needs what a batched launch needs -- an open sequence and a variant chosen on the host -- so every run
makes a first short call and a synchronize() first, as tests/test_gpu_ensemble.py does.  Tolerance: none.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ens_obs_ref as O
from tests import shapes as S
from tests.test_gpu_ensemble import _bad, _start, member_uploads

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE, ERR_BLOWUP = 0, 1, 4, 5
STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")
NAMES4 = ("ssh", "sshp", "ubrtr", "vbrtrp")   # the 16-term rows' fields
OTHER4 = ("vbrtr", "ubrtrp", "sshp", "ssh")   # ... where the other two prognostic fields are read
MIXED = ["plain", "noise", "hr", "general", "noise"]


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


# ---------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=64)
def member_states(shape, cls, off, steps, params=None):
    """[{(bm, bn): {field: array}}, ...]: the six state fields of the oracle after 1 .. steps calls of
    step(tau) from the member's inputs.  Computed once per key; the callers do not write into it."""
    om = S.oracle_model(shape, params=params)
    for k, b in enumerate(om.blocks):
        for nm, a in member_uploads(shape, cls, off, params).get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    out = []
    for _ in range(steps):
        om.step(S.tau_of(params))
        out.append({(b.bm, b.bn): {nm: om.f[k][nm].copy(order="F") for nm in STATE} for k, b in enumerate(om.blocks)})
    return out


def _want(e, shape, classes, idx, op, at, params=None):
    """The records after the oracle steps `at` (1-based, rising) of the members idx: (len(at), nobs, len(idx))."""
    blocks = e.members[0].blocks
    runs = [member_states(shape, classes[i], 1000 * i, max(at), params) for i in idx]
    out = np.zeros((len(at), op.nobs, len(idx)))
    for r, s in enumerate(at):
        fields = {nm: {b.k: [run[s - 1][(b.bm, b.bn)][nm] for run in runs] for b in blocks} for nm in op.names}
        out[r] = O.apply(op, fields, blocks, e.block_of)
    return out


def _op(shape, nobs, seed, names=NAMES4):
    """nobs rows over the whole array of the shape's basin (rings and land included): unit rows, 4-term bilinear
    rows, 16-term rows over the four `names`, and rows that repeat one point; the first unit rows sit in the
    corners of the array, the rest are scattered, so every tile of the block holds some."""
    nx, ny = shape.W + 4, shape.H + 4
    rng = np.random.default_rng(seed)
    pt = lambda: (int(rng.integers(1, nx + 1)), int(rng.integers(1, ny + 1)))   # noqa: E731
    w = lambda: float(rng.uniform(-1.0, 1.0)) or 0.5                             # noqa: E731
    corners = [(1, 1), (nx, 1), (1, ny), (nx, ny), (2, 2), (nx - 1, ny - 1)]
    rows = []
    for r in range(nobs):
        kind = r % 4
        if nobs == 1 or kind == 2:
            rows.append([(names[t % 4],) + pt() + (w(),) for t in range(16)])
        elif kind == 0:
            i, j = corners[r // 4] if r // 4 < len(corners) else pt()
            rows.append([(names[(r // 4) % 4], i, j, 1.0)])
        elif kind == 1:
            x, y = rng.uniform(1.0, nx - 0.01), rng.uniform(1.0, ny - 0.01)
            rows.append(O.bilinear(names[(r // 4 + 1) % 4], [[x, y]], shape=(nx, ny)).row(0))
        else:
            i, j = pt()
            rows.append([(names[2], i, j, w()), (names[0], i, j, w()), (names[2], i, j, w())])
    op = O.ObsOperator.from_rows(rows, np.full((nobs, 2), 3))
    assert len(op.names) <= 4
    return op


def _due(calls, every, counted=0):
    from ocean_model_arch_amd import ens_record_rule
    at, per_call = [], []
    for n in calls:
        d = ens_record_rule.due(counted, n, every)
        per_call.append(d)
        at += [counted + s for s in d]
        counted += n
    return at, per_call


def _record_calls(e, calls, check_every=1, params=None):
    """The step_record calls (a synchronize() after the first: the known-constant verdicts reach the host):
    ensemble info, recorder info and launches per call."""
    from ocean_model_arch_amd import _lib
    tau = S.tau_of(params)
    infos, rinfos, launches = [], [], []
    for i, n in enumerate(calls):
        l0 = _lib.launch_count()
        e.step_record(n, tau=tau, check_every=check_every)
        launches.append(_lib.launch_count() - l0)
        infos.append(e.info())
        rinfos.append(e.record_info())
        if i == 0:
            assert e.synchronize() == [OK] * len(e)
    return infos, rinfos, launches


def _case(amd, shape, classes, nobs, calls, every=1, members=None, check_every=1, in_launch=True, cap=None, seed=0,
          names=NAMES4):
    """One run: the series against the oracle, then complete() and every field of every member against _bad's
    reference.  Returns (infos, rinfos, launches, the in-launch records expected per call)."""
    e = _start(amd, shape, classes)
    try:
        if cap is not None:
            e.set_capacity(cap)
        e.set_record_in_launch(in_launch)
        op = _op(shape, nobs, seed + nobs, names)
        at, per_call = _due(calls, every)
        e.record(op, every=every, max_records=max(len(at), 1), members=members)
        infos, rinfos, launches = _record_calls(e, calls, check_every)
        idx = list(range(len(classes))) if members is None else sorted(set(members))
        got = e.series()
        want = _want(e, shape, classes, idx, op, at) if at else np.zeros((0, nobs, len(idx)))
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert got.shape == want.shape == (len(at), nobs, len(idx))
    differ = [r for r in range(len(at)) if not O.bits_equal(got[r], want[r])]
    assert not differ, f"records {differ} (after steps {[at[r] for r in differ]}) differ from the oracle"
    assert st == [OK] * len(classes) and not bad, (st, bad)
    assert rinfos[-1]["steps"] == sum(calls) and rinfos[-1]["records"] == len(at), rinfos[-1]
    inside = [len([s for s in d if s < n]) for d, n in zip(per_call, calls)]
    return infos, rinfos, launches, inside


# ---------------------------------------------------------------- 1. one tile per member
def test_one_tile_per_member(amd):
    """Shape(61, 9), five members of four variants, 300 rows (more than the member's 256 threads), every = 1,
    calls [2, 5, 4]: the first call is chunked, the odd count exercises the role swap, the third call starts
    from swapped roles.  Four and three records come from the launches themselves, each call's last from the
    gather behind its launches: groups + 1 launches."""
    infos, rinfos, launches, inside = _case(amd, S.Shape(61, 9), MIXED, 300, [2, 5, 4])
    assert inside == [1, 4, 3]
    assert [r["in_launch"] for r in rinfos] == [0, 4, 4 + 3], rinfos
    assert infos[1]["batched"] == 5 and launches[1] == infos[1]["groups"] + 1, (infos, launches)
    assert infos[2]["batched"] == 5 and launches[2] == infos[2]["groups"] + 1, (infos, launches)


# ---------------------------------------------------------------- 2. many tiles per member
@pytest.mark.parametrize("nobs", [64, 1])
def test_many_tiles_per_member(amd, nobs):
    """Shape(121, 65): 51 tiles a member, so the rows are read by workgroups that did not write them; with 64
    rows most workgroups own none, with one row all but one."""
    infos, rinfos, launches, inside = _case(amd, S.Shape(121, 65), ["plain", "noise", "hr", "general"], nobs, [2, 6],
                                            names=OTHER4 if nobs == 64 else NAMES4)
    assert infos[1]["tiles"] == 51 and infos[1]["batched"] == 4, infos[1]
    assert rinfos[-1]["in_launch"] == 5 and launches[1] == infos[1]["groups"] + 1, (rinfos, launches)


# ---------------------------------------------------------------- 3. the schedule across calls
def test_schedule_across_calls(amd):
    """every = 3, calls [2, 5, 4, 1, 6]: records after steps 3 (mid-launch), 6, 9 (mid-launch), 12 (a chunked
    1-step call's only step), 15 (mid-launch) and 18 (a call's last step); steps, records and slices of the
    series."""
    shape, classes, calls, every = S.Shape(61, 9), MIXED, [2, 5, 4, 1, 6], 3
    e = _start(amd, shape, classes)
    try:
        op = _op(shape, 37, 3)
        at, per_call = _due(calls, every)
        assert at == [3, 6, 9, 12, 15, 18] and per_call == [[], [1, 4], [2], [1], [3, 6]]
        e.record(op, every=every, max_records=6)
        infos, rinfos, launches = _record_calls(e, calls)
        want = _want(e, shape, classes, range(5), op, at)
        whole = e.series()
        parts = [e.series(0, 0), e.series(1, 2), e.series(5), e.series(first=4, count=1)]
        with pytest.raises(ValueError):
            e.series(5, 2)
        with pytest.raises(ValueError):
            e.series(-1, 1)
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert whole.shape == (6, 37, 5) and O.bits_equal(whole, want)
    assert parts[0].shape == (0, 37, 5) and O.bits_equal(parts[1], want[1:3]) and O.bits_equal(parts[2], want[5:])
    assert O.bits_equal(parts[3], want[4:5])
    assert [(r["steps"], r["records"]) for r in rinfos] == [(2, 0), (7, 2), (11, 3), (12, 4), (18, 6)], rinfos
    assert [r["in_launch"] for r in rinfos] == [0, 2, 3, 3, 4], rinfos
    assert rinfos[0]["every"] == 3 and rinfos[0]["nobs"] == 37 and rinfos[0]["n"] == 5 and rinfos[0]["max_records"] == 6
    assert st == [OK] * 5 and not bad, (st, bad)


# ---------------------------------------------------------------- 4. a subset, several groups, tall tiles
@pytest.mark.parametrize("cap", [7, 2])
def test_subset_groups_tall_tiles(amd, cap):
    """Nine members, four in use (named out of order: the columns are in member order), a capacity of 7 (three
    groups of three at 16 rows) and of 2 (nine launches of one member): members not in use step as ever."""
    infos, rinfos, launches, inside = _case(amd, S.Shape(61, 9), ["noise"] * 9, 21, [2, 6], members=[8, 3, 1, 4], cap=cap)
    assert (infos[1]["groups"], infos[1]["rows"], infos[1]["batched"]) == ({7: 3, 2: 9}[cap], 16, 9), infos[1]
    assert rinfos[-1]["n"] == 4 and rinfos[-1]["in_launch"] == 5, rinfos
    assert launches[1] == infos[1]["groups"] + 1, launches


# ---------------------------------------------------------------- 5. forced and natural fallback
def test_forced_fallback(amd):
    """Case 1 with OCN_ENS_OPT_RECORD_IN_LAUNCH 0: the same series from the chunked route."""
    infos, rinfos, launches, inside = _case(amd, S.Shape(61, 9), MIXED, 300, [2, 5, 4], in_launch=False)
    assert [r["in_launch"] for r in rinfos] == [0, 0, 0], rinfos


@pytest.mark.parametrize("shape", [S.Shape(17, 19, (2, 2)), S.Shape(13, 11, (1, 1), 1)], ids=lambda s: s.id)
def test_natural_fallback_configurations(amd, shape):
    """A block grid (the terms of one row lie in different blocks) and a tracer run: nothing is batched, the
    whole call is chunked."""
    infos, rinfos, launches, inside = _case(amd, shape, ["noise", "general"], 23, [2, 3], seed=7)
    assert rinfos[-1]["in_launch"] == 0 and all(i["batched"] == 0 for i in infos), (rinfos, infos)


def test_natural_fallback_check_every(amd):
    """check_every = 2 is no multi-step launch: chunked, with every = 3 across stretches that begin off the
    checks' phase."""
    infos, rinfos, launches, inside = _case(amd, S.Shape(61, 9), MIXED, 23, [2, 5, 4], every=3, check_every=2)
    assert rinfos[-1]["in_launch"] == 0, rinfos


# ---------------------------------------------------------------- 6. the smallest block
def test_edge_shape(amd):
    """Shape(1, 1), three members: a barrier over one workgroup, whose first lanes take all the rows."""
    infos, rinfos, launches, inside = _case(amd, S.Shape(1, 1), ["noise"] * 3, 9, [2, 3])
    assert (infos[1]["groups"], infos[1]["batched"]) == (1, 3) and rinfos[-1]["in_launch"] == 2, (infos, rinfos)


# ---------------------------------------------------------------- 7. isolation
@pytest.mark.parametrize("check_every", [1, 0])
def test_blowup_isolation(amd, check_every):
    """Member 1 made to blow up exactly as tests/test_gpu_ensemble.py test_blowup_isolation does: the other
    members' columns and fields are the oracle's, the statuses as that test expects."""
    shape, classes, calls = S.Shape(61, 9), ["noise"] * 3, [2, 6]
    e = _start(amd, shape, classes)
    try:
        m = e.members[1]
        ssh, lu = m.download(0, "ssh"), m.download(0, "lu")
        i, j = 30 + 2, 4 + 2
        assert lu[i, j] > 0.5
        ssh[i, j] = 2.0e4
        m.upload(0, "ssh", ssh)
        m.upload(0, "sshn", ssh)
        op = _op(shape, 40, 11)
        e.record(op, every=1, max_records=8)
        e.step_record(calls[0], tau=1.0, check_every=0)
        assert e.synchronize() == [OK] * 3
        e.step_record(calls[1], tau=1.0, check_every=check_every)
        info, rinfo = e.info(), e.record_info()
        got = e.series()
        want = _want(e, shape, classes, [0, 2], op, list(range(1, 9)))
        e.complete()
        raw = (C.c_int32 * 3)()
        rc = amd.lib().ocn_ens_synchronize(e.ens, raw)
        st = list(raw)
        bad = [x for x in _bad(e, shape, classes, sum(calls)) if not x.startswith("member 1 ")]
    finally:
        e.close()
    assert (info["groups"], info["batched"]) == (1, 3) and rinfo["in_launch"] == 5, (info, rinfo)
    assert st == ([OK, ERR_BLOWUP, OK] if check_every else [OK] * 3), st
    assert rc == (ERR_BLOWUP if check_every else OK), rc
    assert got.shape == (8, 40, 3) and O.bits_equal(got[:, :, [0, 2]], want)
    assert not bad, bad


# ---------------------------------------------------------------- 8. interleaving
def test_interleaving(amd):
    """step_record, plain step(3), step_record: the plain steps are neither counted nor recorded; a second
    record() replaces the first; record_end() and then step_record raises."""
    from ocean_model_arch_amd import _lib
    shape, classes = S.Shape(61, 9), ["noise", "hr", "noise"]
    e = _start(amd, shape, classes)
    try:
        op = _op(shape, 19, 5)
        e.record(op, every=1, max_records=16)
        e.step_record(2)
        assert e.synchronize() == [OK] * 3
        e.step_record(4)
        e.step(3)
        e.step_record(3)
        first, info1 = e.series(), e.record_info()
        want1 = _want(e, shape, classes, range(3), op, [1, 2, 3, 4, 5, 6, 10, 11, 12])
        op2 = _op(shape, 5, 6, OTHER4)
        e.record(op2, every=2, max_records=4, members=[0, 2])
        info2 = e.record_info()
        e.step_record(4)
        second, info3 = e.series(), e.record_info()
        want2 = _want(e, shape, classes, [0, 2], op2, [14, 16])
        e.record_end()
        assert not e.record_info()["active"]
        with pytest.raises(_lib.OcnError) as err:
            e.step_record(2)
        assert err.value.code == ERR_STATE
        e.complete()
        st = e.synchronize()
        bad = _bad(e, shape, classes, 16)
    finally:
        e.close()
    assert (info1["steps"], info1["records"]) == (9, 9) and O.bits_equal(first, want1)
    assert (info2["steps"], info2["records"], info2["in_launch"], info2["n"], info2["nobs"]) == (0, 0, 0, 2, 5), info2
    assert (info3["steps"], info3["records"]) == (4, 2) and O.bits_equal(second, want2)
    assert st == [OK] * 3 and not bad, (st, bad)


# ---------------------------------------------------------------- 9. errors change nothing
def test_errors_change_nothing(amd):
    """Every OCN_ERR_ARG and OCN_ERR_STATE case of the contract: no launch, the earlier series still there bit
    for bit, the members' fields unchanged, and a step_record past max_records steps nothing."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    shape, classes = S.Shape(61, 9), ["noise"] * 3
    e = _start(amd, shape, classes)
    try:
        op = _op(shape, 12, 9)
        e.record(op, every=2, max_records=3)
        e.step_record(2)
        assert e.synchronize() == [OK] * 3
        e.step_record(3)
        e.complete()
        kept, info = e.series(), e.record_info()
        before = O.downloads(e, STATE, range(3))
        assert (info["steps"], info["records"]) == (5, 2)

        def arr(a, dt):
            return np.ascontiguousarray(a, dtype=dt)

        def begin(ens=e.ens, use=None, nobs=2, start=(0, 1, 2), tfield=("ssh", "ubrtr"), ti=(5, 6), tj=(5, 6), tw=(1.0, 0.5),
                  every=1, max_records=4, null=None):
            a = {"start": arr(start, np.int32), "tfield": arr([_lib.FIELD_ID[nm] if isinstance(nm, str) else nm for nm in tfield], np.int32),
                 "ti": arr(ti, np.int32), "tj": arr(tj, np.int32), "tw": arr(tw, np.float64)}
            p = {k: (None if k == null else v.ctypes.data_as(C.c_void_p)) for k, v in a.items()}
            u = None if use is None else (C.c_uint8 * 3)(*use)
            return L.ocn_ens_record_begin(ens, u, nobs, p["start"], p["tfield"], p["ti"], p["tj"], p["tw"], every, max_records)

        l0 = _lib.launch_count()
        args = {"null ensemble": dict(ens=None), "nobs 0": dict(nobs=0), "nobs 65537": dict(nobs=65537),
                "no member in use": dict(use=(0, 0, 0)), "start[0] 1": dict(start=(1, 1, 2)),
                "an empty row": dict(start=(0, 0, 2)),
                "17 terms": dict(nobs=1, start=(0, 17), tfield=("ssh",) * 17, ti=(5,) * 17, tj=(5,) * 17, tw=(0.5,) * 17),
                "a zero weight": dict(tw=(1.0, 0.0)), "a nan weight": dict(tw=(1.0, np.nan)),
                "a real(4) field": dict(tfield=("ssh", "lu")), "an absent field": dict(tfield=("ssh", 10 ** 6)),
                "five fields": dict(nobs=1, start=(0, 5), tfield=STATE[:5], ti=(5,) * 5, tj=(5,) * 5, tw=(0.5,) * 5),
                "a term outside the array": dict(ti=(5, 66)), "a non-state field": dict(tfield=("ssh", "hhu")),
                "every 0": dict(every=0), "max_records 0": dict(max_records=0),
                "a series above 1 GiB": dict(max_records=2 ** 31 - 1)}
        args.update({f"null {k}": dict(null=k) for k in ("start", "tfield", "ti", "tj", "tw")})
        wrong = {k: rc for k, rc in ((k, begin(**kw)) for k, kw in args.items()) if rc != ERR_ARG}
        assert not wrong, wrong
        host = np.zeros(3 * 12 * 3)
        hp = host.ctypes.data_as(C.c_void_p)
        wrong = {k: rc for k, rc in {"past max_records": L.ocn_ens_step_record(e.ens, 1.0, 3, 1),
                                     "nsteps -1": L.ocn_ens_step_record(e.ens, 1.0, -1, 1),
                                     "null ensemble": L.ocn_ens_step_record(None, 1.0, 1, 1),
                                     "download past the records": L.ocn_ens_record_download(e.ens, 1, 2, hp),
                                     "download first -1": L.ocn_ens_record_download(e.ens, -1, 1, hp),
                                     "download count -1": L.ocn_ens_record_download(e.ens, 0, -1, hp),
                                     "download null host": L.ocn_ens_record_download(e.ens, 0, 1, None),
                                     "info null": L.ocn_ens_record_info(e.ens, None),
                                     "end null": L.ocn_ens_record_end(None),
                                     "option 2": L.ocn_ens_set_option(e.ens, _lib.ENS_OPT_RECORD_IN_LAUNCH, 2)}.items() if rc != ERR_ARG}
        assert not wrong, wrong
        with pytest.raises(ValueError):
            e.record(op, every=0)
        with pytest.raises(TypeError):
            e.record(op, every=1.5)
        with pytest.raises(TypeError):
            e.record("ssh")
        with pytest.raises(ValueError):
            e.record(op, max_records=2 ** 31 - 1)
        with pytest.raises(TypeError):
            e.step_record(2.0)
        assert _lib.launch_count() == l0
        after_info = e.record_info()
        assert after_info == info and O.bits_equal(e.series(), kept)
        after = O.downloads(e, STATE, range(3))
        assert not [(nm, i) for nm in STATE for i in range(3) if not O.bits_equal(after[nm][0][i], before[nm][0][i])]
        assert _lib.launch_count() == l0            # (the members were complete: the downloads launched nothing)
        e.record_end()
        wrong = {k: rc for k, rc in {"step_record": L.ocn_ens_step_record(e.ens, 1.0, 2, 1),
                                     "download": L.ocn_ens_record_download(e.ens, 0, 1, hp),
                                     "end": L.ocn_ens_record_end(e.ens)}.items() if rc != ERR_STATE}
        assert not wrong, wrong
        assert _lib.launch_count() == l0
        st = e.synchronize()
        bad = _bad(e, shape, classes, 5)
    finally:
        e.close()
    assert st == [OK] * 3 and not bad, (st, bad)
