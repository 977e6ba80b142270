"""GPU tests of observations at their own times (ocn_ens_record_sample, ocn_ens_assimilate_rec; ens_assim.hip
rec_interp, k_ens_record_sample and k_ens_obs_space_r in front of ens_local.hip k_ens_local) and of
OceanEnsemble.sample_recorded / assimilate_recorded.

The references: ens_record_rule.interp (checked against a scalar loop by tests/test_ens_fgat_cpu.py) on the
recorder's own series(); assimilate_h() on a twin ensemble for observations at the last record; the ordered
observation-space loop and the update's rule (tests/ens_obs_ref.py) on the members' own downloads.  Helpers are
those of tests/test_gpu_ens_record.py.  Every comparison is bitwise on whole arrays (NaN by position).
Tolerance: none.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ens_obs_ref as O
from tests import shapes as S
from tests.test_gpu_ens_assim import STAGE_LAUNCHES, _obs_values
from tests.test_gpu_ens_record import _op, _record_calls
from tests.test_gpu_ensemble import _start

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE = 0, 1, 4
STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")
SMALL = S.Shape(13, 11)      # one block, the basin 17 x 15 with its rings
LAST = np.nextafter(1.0, 0.0)
WEIGHTS = (0.0, 0.5, 0.3, LAST)


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _anchored(shape, nobs, seed):
    """tests/test_gpu_ens_record.py's operator with the anchors scattered over the basin."""
    op = _op(shape, nobs, seed)
    rng = np.random.default_rng(seed + 77)
    anchors = np.stack([rng.integers(1, shape.W + 5, nobs), rng.integers(1, shape.H + 5, nobs)], axis=1)
    return O.ObsOperator.from_rows([op.row(j) for j in range(nobs)], anchors)


def _recorded(amd, shape, classes, nobs, calls, every=1, members=None, seed=0, max_records=32):
    e = _start(amd, shape, classes)
    try:
        op = _anchored(shape, nobs, seed)
        e.record(op, every=every, max_records=max_records, members=members)
        _record_calls(e, calls)
    except BaseException:
        e.close()
        raise
    return e, op


def _sample_c(e, use, rows, rec, wt, n):
    """ocn_ens_record_sample through ctypes: the weights exactly as given."""
    import ocean_model_arch_amd as amd
    r, c, w = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(rec, np.int32), np.ascontiguousarray(wt, np.float64)
    out = np.full((len(r), n), 7.5)
    u = None if use is None else (C.c_uint8 * len(e))(*use)
    rc = amd.lib().ocn_ens_record_sample(e.ens, u, len(r), _ptr(r), _ptr(c), _ptr(w), _ptr(out))
    return rc, out


def _mixed_obs(count, nobs_r, records, seed):
    """`count` observations: rows named repeatedly, records over the whole series, the weights of WEIGHTS in turn (0
    at the last record)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, nobs_r, count)
    rec = rng.integers(0, records, count)
    wt = np.array(WEIGHTS)[np.arange(count) % len(WEIGHTS)]
    rows[-1], rec[-1] = nobs_r - 1, records - 1          # the series' last element
    return rows, rec, np.where(rec == records - 1, 0.0, wt)


# ---------------------------------------------------------------- 1. the gather alone
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("n", [2, 9, 33])
def test_sample_recorded_is_interp(amd, n, every):
    """n + 1 members of which the recorder holds all but member 1: one observation and 257 (more than one workgroup
    of (observation, member) pairs at every n), rows named repeatedly, the four weights; `use` NULL, the recorder's
    members named, and a proper subset of them.  Then sample_recorded() over times at and between the records."""
    from ocean_model_arch_amd import ens_record_rule as R
    held = [0] + list(range(2, n + 1))
    calls = [2, 5] if every == 1 else [2, 7, 6]
    e, op = _recorded(amd, SMALL, ["noise"] * (n + 1), 7, calls, every=every, members=held)
    try:
        info = e.record_info()
        records = info["records"]
        assert records == (7 if every == 1 else 5) and info["n"] == n
        series = e.series()
        bad = []
        subsets = [(None, list(range(n))), (held, list(range(n)))]
        if n > 2:
            sub = [i for k, i in enumerate(held) if k % 3 != 0]
            subsets.append((sub, [held.index(i) for i in sub]))
        for count in (1, 257):
            rows, rec, wt = _mixed_obs(count, 7, records, 10 * n + count)
            for members, cols in subsets:
                use = None if members is None else [1 if i in members else 0 for i in range(n + 1)]
                rc, got = _sample_c(e, use, rows, rec, wt, len(cols))
                if rc != OK or not O.bits_equal(got, R.interp(series, rows, rec, wt, cols)):
                    bad.append((count, members, rc))
        rng = np.random.default_rng(n)
        first, last = every, records * every
        at = np.concatenate([[first, last, first + 0.5 * every], rng.uniform(first, last, 60)])
        rows = rng.integers(0, 7, len(at))
        for members, cols in subsets:
            got = e.sample_recorded(rows, at, members=members)
            rec, wt = R.at_steps(at, every, records)
            assert got.shape == (len(at), len(cols))
            if not O.bits_equal(got, R.interp(series, rows, rec, wt, cols)):
                bad.append(("sample_recorded", members))
        assert e.record_info() == info and O.bits_equal(e.series(), series)
    finally:
        e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 2. at the last record it is assimilate_h
@pytest.mark.parametrize("n", [2, 9, 33])
def test_twin_at_the_last_record(amd, n):
    """A: step_record, then assimilate_recorded(device=True) with every observation at the last record; B: the same
    steps, then assimilate_h(device=True) of the same rows.  The record of a call's last step is sample_h() at that
    time, so everything is equal bit for bit, the launches too.  A Gaspari-Cohn taper, four steps more, a ringed
    one."""
    from ocean_model_arch_amd import _lib
    a, op = _recorded(amd, SMALL, ["noise"] * n, 11, [2, 5])
    b = _start(amd, SMALL, ["noise"] * n)
    bad = []
    try:
        for i, k in enumerate([2, 5]):
            b.step(k)
            if i == 0:
                assert b.synchronize() == [OK] * n
        rows = np.array([3, 0, 10, 7, 3, 5, 1, 9, 2, 8, 6, 4])             # (row 3 twice)
        op_rows = O.ObsOperator.from_rows([op.row(int(r)) for r in rows], op.anchors[rows])
        for t, (what, taper) in enumerate([("gaspari-cohn", O.taper_table(6.0)), ("ring", O.ringed_taper(50))]):
            steps = a.record_info()["steps"]
            at = np.full(len(rows), float(steps))
            hx0 = a.sample_recorded(rows, at)
            if not O.bits_equal(hx0, b.sample_h(op_rows)):
                bad.append((what, "the last record is not sample_h()"))
            values, variances = _obs_values(hx0, 10 * n + t)
            a.complete()                                                   # (sample_h() formed B's tails)
            l0 = _lib.launch_count()
            ga = a.assimilate_recorded(rows, at, values, variances, taper, device=True)
            l1 = _lib.launch_count()
            ya = a.assimilate_results(("y", "z"))
            l2 = _lib.launch_count()
            gb = b.assimilate_h(op_rows, values, variances, taper, device=True)
            l3 = _lib.launch_count()
            yb = b.assimilate_results(("y", "z"))
            if not (l1 - l0 == l3 - l2 == len(STATE) + STAGE_LAUNCHES):
                bad.append((what, "launches", l1 - l0, l3 - l2))
            if set(ga) != set(gb) or ga["nonfinite"] != gb["nonfinite"] or ga["nonfinite"] != 0:
                bad.append((what, "keys or nonfinite"))
            bad += [(what, k) for k in O.info_mismatches(ga, gb)]
            bad += [(what, k) for k in ("y", "z") if not O.bits_equal(ya[k], yb[k])]
            if O.bits_equal(ga["hx"], hx0):
                bad.append((what, "nothing happened"))
            fa, fb = O.downloads(a, STATE, range(n)), O.downloads(b, STATE, range(n))
            bad += [(what, nm, i) for nm in STATE for i in range(n) if not O.bits_equal(fa[nm][0][i], fb[nm][0][i])]
            a.step_record(4)
            b.step(4)
    finally:
        a.close()
        b.close()
    assert not bad, bad


# ---------------------------------------------------------------- 3. the two routes of the Python driver
def test_device_against_host_route(amd):
    """Twin ensembles of 5 members (up to 8 members numpy's own reductions run in member order, so the host route's
    loop has the device's bits), 40 observations over a window of 6 records with mixed weights: device=True on
    one, device=False on the other -- fields and results.  Three steps more, so that the recorder spans the first
    analysis, and again with rtps=0.5 over the window as it is."""
    n = 5
    es = [_recorded(amd, SMALL, ["noise"] * n, 9, [2, 4])[0] for _ in range(2)]
    op = _anchored(SMALL, 9, 0)
    bad = []
    try:
        for t, rtps in enumerate((None, 0.5)):
            rng = np.random.default_rng(t)
            records = es[0].record_info()["records"]
            assert records == 6 + 3 * t
            at = rng.uniform(1.0, float(records), 40)
            at[:4] = [1.0, 2.5, float(records), 3.0]
            rows = rng.integers(0, 9, 40)
            hx0 = es[0].sample_recorded(rows, at)
            values, variances = _obs_values(hx0, t)
            taper = O.taper_table(5.0)
            got = [e.assimilate_recorded(rows, at, values, variances, taper, device=dev, rtps=rtps)
                   for e, dev in zip(es, (True, False))]
            if set(got[0]) != set(O.KEYS) | {"nonfinite"} or not set(got[1]) >= set(O.KEYS):
                bad.append((rtps, "keys"))
            bad += [(rtps, k) for k in O.info_mismatches(got[0], got[1])]
            if O.bits_equal(got[0]["hx"], hx0):
                bad.append((rtps, "nothing happened"))
            fa, fb = (O.downloads(e, STATE, range(n)) for e in es)
            bad += [(rtps, nm, i) for nm in STATE for i in range(n) if not O.bits_equal(fa[nm][0][i], fb[nm][0][i])]
            infos = [e.record_info() for e in es]
            assert infos[0] == infos[1] and infos[0]["records"] == records
            for e in es:
                e.step_record(3)
        # the default anchors are the recorded operator's
        for e, dev, ij in zip(es, (True, False), (None, op.anchors[[0, 4]])):
            e.assimilate_recorded([0, 4], [2.0, 3.5], [0.1, 0.2], [0.01, 0.01], np.array([1.0, 0.5]), anchors=ij, names=("ssh",),
                                  device=dev)
        fa, fb = (O.downloads(e, ("ssh",), range(n)) for e in es)
        bad += [("default anchors", i) for i in range(n) if not O.bits_equal(fa["ssh"][0][i], fb["ssh"][0][i])]
    finally:
        for e in es:
            e.close()
    assert not bad, bad


# ---------------------------------------------------------------- 4. against the restatement; other configurations
def _assim_rec_vs_restatement(e, rows, at, anchors, taper, names, members=None, cols=None, seed=0, values=None,
                              variances=None):
    """assimilate_recorded(device=True) against the restatement -- interp on series(), the ordered loop at the
    anchors, the update's rule on the members' own downloads of every block.  The recorder must not change.
    Returns (what differs, the launches of the call, the returned dict, hx before)."""
    from ocean_model_arch_amd import _lib
    from ocean_model_arch_amd import ens_record_rule as R
    info = e.record_info()
    held = list(range(len(e))) if e._rec_members is None else e._rec_members
    idx = held if members is None else sorted(set(members))
    blocks = e.members[0].blocks
    series = e.series()
    rec, wt = R.at_steps(np.asarray(at, dtype=np.float64), info["every"], info["records"])
    hx0 = R.interp(series, rows, rec, wt, [held.index(i) for i in idx])
    bad = []
    if not O.bits_equal(e.sample_recorded(rows, at, members=members), hx0):
        bad.append("sample_recorded() is not interp(series())")
    if values is None:
        values, variances = _obs_values(hx0, seed)
    before = O.downloads(e, names, idx)
    l0 = _lib.launch_count()
    got = e.assimilate_recorded(rows, at, values, variances, taper, anchors=anchors, names=names, members=members, device=True)
    launches = _lib.launch_count() - l0
    yz = e.assimilate_results(("y", "z"))
    Y, Z, ref = O.ensrf_obs_space_ordered(hx0, anchors, values, variances, taper)
    if set(got) != set(O.KEYS) | {"nonfinite"}:
        bad.append(f"keys {sorted(got)}")
    bad += O.info_mismatches(got, ref)
    bad += [nm for nm, a, r in (("Y", yz["y"], Y), ("Z", yz["z"], Z)) if not O.bits_equal(a, r)]
    if got["nonfinite"] != ref["nonfinite"]:
        bad.append(f"nonfinite {got['nonfinite']} != {ref['nonfinite']}")
    after = O.downloads(e, names, idx)
    anchors = np.asarray(anchors)
    for nm in names:
        for b in blocks:
            want = O.block_update(before[nm][b.k], b, anchors[:, 0], anchors[:, 1], Y, Z, taper)
            bad += [f"member {i} [{b.k}]:{nm}" for i, g, v in zip(idx, after[nm][b.k], want) if not O.bits_equal(g, v)]
    if e.record_info() != info or not O.bits_equal(e.series(), series):
        bad.append("the recorder changed")
    return bad, launches, got, hx0


@pytest.mark.parametrize("shape", [S.Shape(17, 19, (2, 2)), S.Shape(13, 11, (1, 1), 1), S.Shape(1, 1)], ids=lambda s: s.id)
def test_other_configurations(amd, shape):
    """A 2 x 2 block grid and a tracer run (their records come from the recorder's chunked route) and the 1 x 1
    block: 4 members of which the analysis takes three, every = 2, 21 observations over the window."""
    names = ("ssh", "ubrtr")
    e, op = _recorded(amd, shape, ["noise", "general", "noise", "noise"], 6, [2, 5, 3], every=2, seed=3)
    try:
        info = e.record_info()
        assert info["records"] == 5
        rng = np.random.default_rng(5)
        at = rng.uniform(2.0, 10.0, 21)
        at[:3] = [2.0, 10.0, 5.0]
        rows = rng.integers(0, 6, 21)
        anchors = np.stack([rng.integers(1, shape.W + 5, 21), rng.integers(1, shape.H + 5, 21)], axis=1)
        nblk = len(e.members[0].blocks)
        outside = e.members[1].download(0, "ssh")
        bad, launches, got, hx0 = _assim_rec_vs_restatement(e, rows, at, anchors, O.taper_table(7.0), names,
                                                            members=[3, 0, 2], seed=1)
        untouched = O.bits_equal(e.members[1].download(0, "ssh"), outside)
        e.step_record(1)
        st = e.synchronize()
    finally:
        e.close()
    assert not bad, bad
    assert STAGE_LAUNCHES + 1 <= launches <= STAGE_LAUNCHES + len(names) * nblk
    assert got["hx"].shape == (21, 3) and not O.bits_equal(got["hx"], hx0) and got["nonfinite"] == 0
    assert st == [OK] * 4 and untouched


# ---------------------------------------------------------------- 5. errors change nothing
def _error_cases(e, keep):
    """(the valid arguments, {what: the arguments that change}) of ocn_ens_assimilate_rec on SMALL with 4 members of
    which the recorder holds 0, 1 and 3, 5 rows and 3 records."""
    from ocean_model_arch_amd import _lib
    ssh, ub, lu, ff1 = (_lib.FIELD_ID[nm] for nm in ("ssh", "ubrtr", "lu", "ff1_1"))
    i32 = lambda *v: (C.c_int32 * len(v))(*v)          # noqa: E731
    u8 = lambda *v: (C.c_uint8 * len(v))(*v)           # noqa: E731
    f64 = lambda *v: (C.c_double * len(v))(*v)         # noqa: E731
    big_i, big_0, big = np.full(8193, 5, dtype=np.int32), np.zeros(8193, dtype=np.int32), np.ones(8193)
    long_taper, big_w = np.ones(65537), np.zeros(8193)
    keep += [big_i, big_0, big, long_taper, big_w]
    ok = dict(ens=e.ens, ids=i32(ssh), nf=1, use=None, nobs=2, io=i32(5, 9), jo=i32(4, 6), row=i32(1, 2), rec=i32(2, 1),
              wt=f64(0.0, 0.5), v=f64(0.1, -0.2), r=f64(0.01, 0.02), t=f64(*([1.0, 0.5, 0.25] + [0.125] * 33)), nt=36)
    cases = {"null ensemble": dict(ens=None), "null list": dict(ids=None), "null io": dict(io=None), "null jo": dict(jo=None),
             "null row": dict(row=None), "null rec": dict(rec=None), "null wt": dict(wt=None), "null value": dict(v=None),
             "null variance": dict(r=None), "null taper": dict(t=None),
             "nfields 0": dict(nf=0), "real(4) id": dict(ids=i32(ssh, lu), nf=2), "absent id": dict(ids=i32(ff1)),
             "repeated id": dict(ids=i32(ssh, ub, ssh), nf=3),
             "one member": dict(use=u8(0, 1, 0, 0)), "no member": dict(use=u8(0, 0, 0, 0)),
             "a member the recorder does not hold": dict(use=u8(1, 1, 1, 0)),
             "nobs 0": dict(nobs=0),
             "nobs 8193": dict(nobs=8193, io=_ptr(big_i), jo=_ptr(big_i), row=_ptr(big_0), rec=_ptr(big_0), wt=_ptr(big_w),
                               v=_ptr(big), r=_ptr(big)),
             "anchor io 0": dict(io=i32(5, 0)), "anchor io nx + 1": dict(io=i32(18, 9)), "anchor jo 0": dict(jo=i32(0, 6)),
             "anchor jo ny + 1": dict(jo=i32(4, 16)), "ntaper 0": dict(nt=0), "ntaper 65537": dict(t=_ptr(long_taper), nt=65537),
             "row -1": dict(row=i32(1, -1)), "row nobs_r": dict(row=i32(5, 2)), "rec -1": dict(rec=i32(-1, 1)),
             "rec R": dict(rec=i32(2, 3)), "wt != 0 at the last record": dict(wt=f64(0.5, 0.5)),
             "wt tiny at the last record": dict(wt=f64(5e-324, 0.5))}
    keep.append(cases)
    for v in (-5e-324, -0.5, 1.0, 1.5, np.nan, np.inf, -np.inf):
        cases[f"wt {v}"] = dict(wt=f64(0.0, v))
    for v in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        cases[f"variance {v}"] = dict(r=f64(0.01, v))
    for v in (np.nan, np.inf, -np.inf):
        cases[f"value {v}"] = dict(v=f64(0.1, v))
        cases[f"{v} in taper"] = dict(t=f64(1.0, 0.5, v), nt=3)
    return ok, cases


_AS_KEYS = ("ens", "ids", "nf", "use", "nobs", "io", "jo", "row", "rec", "wt", "v", "r", "t", "nt")
_SAMPLE_CASES = ("null ensemble", "null row", "null rec", "null wt", "one member", "no member", "a member the recorder does not hold",
                 "nobs 0", "row -1", "row nobs_r", "rec -1", "rec R", "wt != 0 at the last record", "wt tiny at the last record")


def _all_refused(L, ok, cases, want=ERR_ARG):
    """Every case through ocn_ens_assimilate_rec and, where it has the argument, ocn_ens_record_sample: what was not
    refused with `want` (a null argument: OCN_ERR_ARG always), or wrote to host."""
    wrong = []
    out = np.full(64, 7.5)
    for what, change in cases.items():
        a = {**ok, **change}
        expect = ERR_ARG if what.startswith("null") else want
        rc = L.ocn_ens_assimilate_rec(*[a[k] for k in _AS_KEYS])
        if rc != expect:
            wrong.append(("assimilate_rec", what, rc))
        if what in _SAMPLE_CASES or what.startswith("wt "):
            rc = L.ocn_ens_record_sample(a["ens"], a["use"], a["nobs"], a["row"], a["rec"], a["wt"], _ptr(out))
            if rc != expect or not (out == 7.5).all():
                wrong.append(("record_sample", what, rc))
    a = ok
    if L.ocn_ens_record_sample(a["ens"], a["use"], a["nobs"], a["row"], a["rec"], a["wt"], None) != ERR_ARG:
        wrong.append(("record_sample", "null host"))
    big_0, big = np.zeros(65537, dtype=np.int32), np.zeros(65537)
    if want == ERR_ARG and L.ocn_ens_record_sample(a["ens"], a["use"], 65537, _ptr(big_0), _ptr(big_0), _ptr(big), _ptr(out)) != ERR_ARG:
        wrong.append(("record_sample", "nobs 65537"))
    return wrong


def test_errors_change_nothing(amd):
    """Every refusal of the contract through ctypes.  Without a recorder: OCN_ERR_STATE.  With a recorder that has
    no record yet: OCN_ERR_ARG for the valid arguments too.  Then every case before any successful call and after
    one: the return code, nothing launched, the members' bits, the recorder's info and series and the earlier
    results unchanged.  And the Python methods' TypeError / ValueError."""
    from ocean_model_arch_amd import _lib
    L = amd.lib()
    e = _start(amd, SMALL, ["noise"] * 4)
    keep = []
    try:
        ok, cases = _error_cases(e, keep)
        l0 = _lib.launch_count()
        no_recorder = _all_refused(L, ok, cases, want=ERR_STATE)
        with pytest.raises(_lib.OcnError) as err:
            e.sample_recorded([0], [1.0])
        assert err.value.code == ERR_STATE
        op = _anchored(SMALL, 5, 1)
        e.record(op, every=1, max_records=3, members=[0, 1, 3])
        no_record = [L.ocn_ens_assimilate_rec(*[ok[k] for k in _AS_KEYS]),
                     L.ocn_ens_record_sample(e.ens, None, 2, ok["row"], ok["rec"], ok["wt"], _ptr(np.zeros(6)))]
        with pytest.raises(ValueError):
            e.sample_recorded([0], [1.0])
        assert _lib.launch_count() == l0
        _record_calls(e, [2, 1])
        e.complete()
        assert e.synchronize() == [OK] * 4
        info, series = e.record_info(), e.series()
        assert info["records"] == 3
        held = O.downloads(e, STATE, range(4))
        out = np.zeros(64)
        l1 = _lib.launch_count()
        wrong = _all_refused(L, ok, cases)
        assert L.ocn_ens_assimilate_result(e.ens, 0, _ptr(out)) == ERR_ARG          # still no successful call
        launched = _lib.launch_count() - l1
        # a successful call, then all of it again
        rc_ok = L.ocn_ens_assimilate_rec(*[ok[k] for k in _AS_KEYS])
        what = ("hx", "y", "z", "innovations", "prior_spread", "posterior_spread")
        res0 = e.assimilate_results(what)
        now0 = O.downloads(e, STATE, range(4))
        l2 = _lib.launch_count()
        wrong2 = _all_refused(L, ok, cases)
        py = []
        for exc, f in [(TypeError, lambda: e.sample_recorded([0.0], [1.0])), (TypeError, lambda: e.sample_recorded([0], ["a"])),
                       (ValueError, lambda: e.sample_recorded([0, 1], [1.0])), (ValueError, lambda: e.sample_recorded([5], [1.0])),
                       (ValueError, lambda: e.sample_recorded([0], [0.5])), (ValueError, lambda: e.sample_recorded([0], [3.5])),
                       (ValueError, lambda: e.sample_recorded([0], [np.nan])),
                       (ValueError, lambda: e.sample_recorded([0], [1.0], members=[0, 2])),
                       (ValueError, lambda: e.sample_recorded([0], [1.0], members=[1])),
                       (ValueError, lambda: e.sample_recorded(np.zeros(65537, dtype=np.int32), np.ones(65537))),
                       (ValueError, lambda: e.assimilate_recorded(np.zeros(8193, dtype=np.int32), np.ones(8193), np.zeros(8193),
                                                                  np.ones(8193), np.array([1.0]), device=True)),
                       (ValueError, lambda: e.assimilate_recorded(np.zeros(8193, dtype=np.int32), np.ones(8193), np.zeros(8193),
                                                                  np.ones(8193), np.array([1.0]))),
                       (TypeError, lambda: e.assimilate_recorded([0], [1.0], [0.1], [0.01], np.array([1.0]), anchors=[[2.5, 3.0]])),
                       (ValueError, lambda: e.assimilate_recorded([0], [1.0], [0.1], [0.01], np.array([1.0]), anchors=[[2, 3], [4, 5]])),
                       (ValueError, lambda: e.assimilate_recorded([0], [1.0], [0.1, 0.2], [0.01], np.array([1.0]))),
                       (ValueError, lambda: e.assimilate_recorded([0], [1.0], [0.1], [0.01], np.array([1.0]), rtps=-1.0))]:
            try:
                f()
                py.append((exc.__name__, "not raised"))
            except exc:
                pass
        launched2 = _lib.launch_count() - l2
        res1 = e.assimilate_results(what)
        now1 = O.downloads(e, STATE, range(4))
        info1, series1 = e.record_info(), e.series()
        del keep
    finally:
        e.close()
    assert not no_recorder, no_recorder
    assert no_record == [ERR_ARG, ERR_ARG], no_record
    assert not wrong and launched == 0, (wrong, launched)
    assert rc_ok == OK
    assert not wrong2 and not py and launched2 == 0, (wrong2, py, launched2)
    assert all(O.bits_equal(res0[k], res1[k]) for k in what)
    changed = [(nm, i) for nm in STATE for i in range(4) if not O.bits_equal(now0[nm][0][i], now1[nm][0][i])]
    assert not changed, changed
    assert not all(O.bits_equal(now0["ssh"][0][i], held["ssh"][0][i]) for i in (0, 1, 3))   # (the valid arguments do go through)
    assert O.bits_equal(now0["ssh"][0][2], held["ssh"][0][2])                               # (... and leave member 2 alone)
    assert info1 == info and O.bits_equal(series1, series)


# ---------------------------------------------------------------- 6. non-finite values
def test_nonfinite(amd):
    """Member 3's state holds a NaN at a station before the recorded steps (unchecked steps: its status stays
    OCN_OK), so its column of the records holds NaN there: the analysis counts it, and it propagates by position as
    the restatement says.  On a fresh ensemble with that member left out by `members`: no count."""
    classes = ["noise"] * 6
    counts, bads = [], []
    for members in (None, [0, 1, 2, 4, 5]):
        e = _start(amd, SMALL, classes)
        try:
            e.step(2)
            assert e.synchronize() == [OK] * 6
            b = e.members[0].blocks[0]
            lu = e.members[3].download(0, "lu")
            sea = np.argwhere(lu[3:-3, 3:-3] > 0.5) + 3
            p, q = sea[np.argmin(((sea - np.array(lu.shape) / 2.0) ** 2).sum(axis=1))]     # the sea point nearest the centre
            i, j = int(p) + b.bnd_x1, int(q) + b.bnd_y1
            for nm in ("ssh", "sshp"):
                a = e.members[3].download(0, nm)
                a[p, q] = np.nan
                e.members[3].upload(0, nm, a)
            op = O.ObsOperator.from_rows([[("ssh", i, j, 1.0)], [("ssh", 3, 3, 1.0)], [("ubrtr", 12, 10, 0.5), ("ssh", 14, 4, 0.5)],
                                          [("ssh", i, j + 1, 0.25), ("ssh", i + 1, j + 1, 0.75)]],
                                         [[i, j], [3, 3], [12, 10], [i, j + 1]])
            e.record(op, every=1, max_records=4)
            e.step_record(3, check_every=0)
            assert e.synchronize() == [OK] * 6
            series = e.series()
            assert np.isnan(series[0, 0, 3]) and np.isfinite(np.delete(series, 3, axis=2)).all()
            rows, at = [0, 1, 2, 3, 0], [1.0, 2.5, 3.0, 1.25, 2.0]
            clean = e.sample_recorded(rows, at, members=[0, 1, 2, 4, 5])
            values, variances = _obs_values(clean, 7)
            bad, _, got, hx0 = _assim_rec_vs_restatement(e, rows, at, op.anchors[rows], O.taper_table(6.0), ("ssh", "ubrtr"),
                                                         members=members, values=values, variances=variances)
        finally:
            e.close()
        counts.append(got["nonfinite"])
        bads.append(bad)
        if members is None:
            assert np.isnan(hx0[0, 3]) and np.isfinite(np.delete(hx0, 3, axis=1)).all()
    assert counts[0] >= 1 and counts[1] == 0, counts
    assert not bads[0] and not bads[1], bads
