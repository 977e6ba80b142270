"""GPU parity of the pair launches' inviscid bodies (OCN_OPT_INVISCID, sw_kernels.hip MarchStepT NV): with mu = +0.0
everywhere and r_diss = +0.0f in every row they form none of the viscous and friction terms, and must leave every
bit what the full bodies leave -- signed zeros, tiny dividends, non-finite and huge state included.  Bitwise against
the CPU oracle (tests/shapes.py, tests/test_gpu_parity.py OracleTwin); tolerance: none.

Blocks: widths 117 and 233 (a second and a third 116-column strip of ONE column) and 58 (half a strip), heights 19
and 40 (the pair tiles here are 8 rows: three and five tiles, the last of 3 / 8 rows), set_pair(2) so that such small
blocks run pairs, the multi-step launch off; one rough coast.  Calls [2, 5, 1, 6] -- the verdict after the first,
pairs over odd and even pending counts, a call of one step -- then complete().

The shape, coast, parameter and fixture sweeps run the default path (inviscid bodies wherever mu and r_diss are
zero) against the oracle as well; these cases add the on / off comparison, the conditions under which the bodies
must not run, and the inputs their guard exists for.
"""
import numpy as np
import pytest

from tests import shapes as S
from tests.test_gpu_parity import bits_equal
from tests.test_gpu_shapes import _model

pytestmark = pytest.mark.gpu

CALLS = [2, 5, 1, 6]
SHAPES = [S.Shape(w, h) for w in (117, 233, 58) for h in (19, 40)] + [S.Shape(117, 40, mask="rough")]


FIELDS = [nm for nm in S.oracle_model(S.Shape(5, 4)).f[0] if nm not in S.SKIP]   # every field the oracle has


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _drive(amd, shape, ups, inviscid, calls=CALLS, check_every=1, between=None, grid_opts=None):
    """A model on the shape with pairs on any block, `ups` ({field: array}, one block) uploaded after init, the calls
    (synchronize() after the first: the verdict reaches the host); between = (index, {field: array}): uploaded
    before that call.  Returns the path flags after each call and, after complete(), {(bm, bn): {field: array}}
    of every field the oracle has."""
    m = _model(amd, shape, multi=False, pair=2, **(grid_opts or {}))
    try:
        m.set_inviscid(inviscid)
        m.init()
        for b in m.blocks:
            for nm, a in ups.get((b.bm, b.bn), {}).items():
                m.upload(b.k, nm, a)
        flags = []
        for i, n in enumerate(calls):
            if between and between[0] == i:
                for b in m.blocks:
                    for nm, a in between[1].items():
                        m.upload(b.k, nm, a)
            m.step(n, check_every=check_every)
            if i == 0:
                m.synchronize()
            flags.append({"nv": m.onepass_inviscid, "pair": m.pair_active, "zero": m.onepass_zero, "x4": m.x4_active,
                          "hr": m.onepass_hr})
        m.complete()
        m.synchronize()
        get = S.model_getter([m])
        out = {(b.bm, b.bn): {nm: get(b.bm, b.bn, nm) for nm in FIELDS} for b in m.blocks}
    finally:
        m.close()
    return flags, out


def _oracle(shape, ups, calls=CALLS, between=None, check=True):
    """check = False: check_every = 0's run -- the oracle's step raises after its last SW stage where
    check_ssh_err counts a point (no tracers here: nothing of the step follows), and the run goes on."""
    om = S.oracle_model(shape)
    for k, b in enumerate(om.blocks):
        for nm, a in ups.get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    for i, n in enumerate(calls):
        if between and between[0] == i:
            for k in range(len(om.blocks)):
                for nm, a in between[1].items():
                    om.f[k][nm][...] = a
        for _ in range(n):
            try:
                om.step(1.0)
            except FloatingPointError:
                if check:
                    raise
    return {(b.bm, b.bn): om.f[k] for k, b in enumerate(om.blocks)}


def _bad(ref, got):
    return [f"({bm},{bn}):{nm}" for (bm, bn), f in ref.items() for nm, a in f.items()
            if nm not in S.SKIP and not bits_equal(got[(bm, bn)][nm], a)]


def _check_flags(flags, on, what):
    """The inviscid bodies only with the option on, only after the verdict, and then in every call that ran pairs."""
    assert not flags[0]["nv"], (what, flags)
    assert any(f["pair"] for f in flags[1:]), (what, flags)
    for f in flags[1:]:
        assert f["nv"] == (on and f["pair"]), (what, on, flags)


# ---------------------------------------------------------------- the default state, on and off
@pytest.mark.parametrize("cls", ["plain", "noise"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
def test_default_state_on_and_off_match_oracle(amd, shape, cls):
    ups = S.uploads_for(shape, cls)
    ref = S.reference(shape, cls, sum(CALLS))
    for on in (True, False):
        flags, got = _drive(amd, shape, ups, on)
        bad = _bad(ref, got)
        assert not bad, f"{shape.id} {cls} inviscid {on}: fields differ from the oracle: {bad}"
        _check_flags(flags, on, f"{shape.id} {cls}")
        assert all(f["zero"] for f in flags), flags


# ---------------------------------------------------------------- signed zeros
def _signed_zero_uploads(shape):
    """Still water under a level surface (every ssh difference cancels exactly: the pressure terms are +-0) with
    -0.0 in parts of the four velocity arrays: every momentum sum is a sum of signed zeros."""
    om = S.oracle_model(shape)
    f = om.f[0]
    ssh = np.full_like(f["ssh"], 0.25, order="F")
    ups = {nm: ssh.copy(order="F") for nm in ("ssh", "sshn", "sshp")}
    i, j = np.meshgrid(np.arange(ssh.shape[0]), np.arange(ssh.shape[1]), indexing="ij")
    for nm, sel in (("ubrtr", (i + j) % 2 == 0), ("vbrtr", j % 3 == 0), ("ubrtrp", i % 3 == 1), ("vbrtrp", (i // 2 + j) % 2 == 1)):
        a = np.zeros_like(ssh, order="F")
        a[sel] = -0.0
        assert np.signbit(a).any() and not np.signbit(a).all()
        ups[nm] = a
    ups["ubrtrn"] = ups["ubrtr"].copy(order="F")
    ups["vbrtrn"] = ups["vbrtr"].copy(order="F")
    return {(1, 1): ups}


@pytest.mark.parametrize("shape", [S.Shape(117, 19), S.Shape(233, 40), S.Shape(117, 40, mask="rough")], ids=lambda s: s.id)
def test_signed_zeros_match_oracle(amd, shape):
    """The case that fails if a zero's sign is lost: the velocities stay signed zeros, and which sign each new one
    has is decided by the sums the inviscid bodies shorten."""
    ups = _signed_zero_uploads(shape)
    ref = _oracle(shape, ups)
    for on in (True, False):
        flags, got = _drive(amd, shape, ups, on)
        bad = _bad(ref, got)
        assert not bad, f"{shape.id} inviscid {on}: fields differ from the oracle: {bad}"
        _check_flags(flags, on, shape.id)


# ---------------------------------------------------------------- where the bodies must not run
@pytest.mark.parametrize("mu", [50.0, -0.0], ids=["mu50", "mu-0"])
def test_uniform_nonzero_mu_keeps_the_full_bodies(amd, mu):
    """A uniform mu whose bits are not zero (50.0; -0.0: 0 * x has the other sign) is still a known constant, but
    no inviscid body runs."""
    shape = S.Shape(233, 40)
    ups = {(1, 1): dict(S.uploads_for(shape, "noise")[(1, 1)])}
    ups[(1, 1)]["mu"] = np.full_like(ups[(1, 1)]["ssh"], mu, order="F")
    ref = _oracle(shape, ups)
    flags, got = _drive(amd, shape, ups, True)
    bad = _bad(ref, got)
    assert not bad, f"mu {mu}: fields differ from the oracle: {bad}"
    assert not any(f["nv"] for f in flags) and all(f["zero"] for f in flags) and any(f["pair"] for f in flags), flags


def test_r_diss_row_keeps_the_full_bodies(amd):
    """ocn_ctx_upload accepts r_diss (a real(4) field: the compact tables are rebuilt): one row of 1e-6 -- the
    friction is then a real term there -- and no inviscid body runs; the oracle is matched."""
    shape = S.Shape(117, 40)
    om = S.oracle_model(shape)
    rd = om.f[0]["r_diss"].copy(order="F")
    assert not rd.any()
    rd[:, 17] = np.float32(1.0e-6)
    ups = {(1, 1): dict(S.uploads_for(shape, "noise")[(1, 1)])}
    ups[(1, 1)]["r_diss"] = rd
    ref = _oracle(shape, ups)
    flags, got = _drive(amd, shape, ups, True)
    bad = _bad(ref, got)
    assert not bad, f"fields differ from the oracle: {bad}"
    assert not any(f["nv"] for f in flags) and any(f["pair"] for f in flags), flags


def test_mu_uploaded_between_calls_drops_the_variant_at_once(amd):
    shape = S.Shape(233, 40)
    ups = S.uploads_for(shape, "noise")
    mu = np.full_like(ups[(1, 1)]["ssh"], 50.0, order="F")
    between = (2, {"mu": mu})
    calls = [2, 5, 6, 5]
    ref = _oracle(shape, ups, calls, between)
    flags, got = _drive(amd, shape, ups, True, calls, between=between)
    bad = _bad(ref, got)
    assert not bad, f"fields differ from the oracle: {bad}"
    assert [f["nv"] for f in flags] == [False, True, False, False], flags
    assert flags[3]["zero"] and flags[3]["pair"], flags


# ---------------------------------------------------------------- tiny dividends: the re-run
@pytest.mark.parametrize("mu0", [False, True], ids=["abyss", "abyss_mu0"])
@pytest.mark.parametrize("shape", [S.Shape(117, 19), S.Shape(117, 40, mask="rough")], ids=lambda s: s.id)
def test_abyss_matches_oracle(amd, shape, mu0):
    """tests/shapes.py abyss: velocities of 2e-305, so every wet row takes the IEEE re-runs in producers and
    consumers.  The class uploads mu = 5e3, with which the full bodies run (asserted); abyss_mu0 is the same state
    with mu left +0.0, where the inviscid bodies run and their re-run (step<true>, entered through a1's dividend)
    forms the full terms from the state ring."""
    ups = {(1, 1): dict(S.uploads(("abyss"), S.oracle_model(shape))[(1, 1)])}
    if mu0:
        del ups[(1, 1)]["mu"]
    ref = _oracle(shape, ups)
    for on in (True, False):
        flags, got = _drive(amd, shape, ups, on)
        bad = _bad(ref, got)
        assert not bad, f"{shape.id} inviscid {on}: fields differ from the oracle: {bad}"
        if mu0:
            _check_flags(flags, on, shape.id)
        else:
            assert not any(f["nv"] for f in flags) and any(f["pair"] for f in flags), flags


# ---------------------------------------------------------------- non-finite and huge state
@pytest.mark.parametrize("value", [np.inf, np.nan, 1.0e305], ids=["inf", "nan", "1e305"])
def test_nonfinite_state_on_equals_off(amd, value):
    """inf, nan or 1e305 at two sea points of ubrtr: column 116 of the interior, the last of the first 116-column
    strip (its neighbour belongs to the next workgroup), and a tile's first row (row 16 of the interior: the tiles
    are 8 rows).  Ordinary IEEE arithmetic, no check (check_every = 0), two calls.  The inviscid run equals the full
    run byte for byte -- 0 * inf and 0 * nan are NaN in both -- and the non-finite values lie where the oracle's do."""
    shape = S.Shape(233, 40)
    om = S.oracle_model(shape)
    u = om.f[0]["ubrtr"].copy(order="F")
    for (i, j) in ((2 + 115, 2 + 21), (2 + 60, 2 + 16)):
        assert om.f[0]["lcu"][i, j] > 0.5
        u[i, j] = value
    ups = {(1, 1): {"ubrtr": u, "ubrtrn": u.copy(order="F")}}
    calls = [2, 4]
    ref = _oracle(shape, ups, calls, check=False)
    runs = {}
    for on in (True, False):
        flags, got = _drive(amd, shape, ups, on, calls, check_every=0)
        assert flags[1]["pair"] and flags[1]["nv"] == on, flags
        runs[on] = got[(1, 1)]
    import bench
    assert set(bench.DUMP_FIELDS) <= set(FIELDS) and {"str_t", "str_s", "RHSx_dif", "RHSy_dif"} <= set(bench.DUMP_FIELDS)
    for nm in bench.DUMP_FIELDS:   # every one: the stresses and the RHS terms are what the dropped terms feed
        assert bits_equal(runs[True][nm], runs[False][nm]), f"{nm}: the inviscid run differs from the full run"
        assert np.array_equal(np.isfinite(runs[True][nm]), np.isfinite(ref[(1, 1)][nm])), f"{nm}: non-finite values elsewhere"
    assert not np.isfinite(runs[True]["ubrtr"]).all()


# ---------------------------------------------------------------- a block grid: x4 pairs
@pytest.mark.parametrize("cls", ["noise", "hr"])
def test_block_grid_x4_pairs_match_oracle(amd, cls):
    """A 3 x 2 block grid in one process, overlap level 1: pairs of x2 steps (one_step_x4), the plain body and, with
    a non-uniform rest depth (hr: what a topography file gives), the body that reads h_r.  x4_active is what it is
    without the inviscid bodies."""
    shape = S.Shape(70, 54, (3, 2))
    ups = S.uploads_for(shape, cls)
    ref = S.reference(shape, cls, 7)
    x4 = {}
    for on in (True, False):
        flags, got = _drive(amd, shape, ups, on, [2, 5], grid_opts={"x4": 1, "overlap": 1})
        bad = _bad(ref, got)
        assert not bad, f"{cls} inviscid {on}: fields differ from the oracle: {bad}"
        assert flags[1]["nv"] == on and not flags[0]["nv"], flags
        assert flags[1]["hr"] == (cls == "hr"), flags
        x4[on] = [f["x4"] for f in flags]
    assert x4[True] == x4[False] and x4[True][1] == S.expect_x4(shape, cls, 1), x4


# ---------------------------------------------------------------- the blow-up report
def test_blowup_message_is_the_same(amd):
    """tests/test_gpu_pair.py test_pair_counts_blowup_points_once's scenario: check_ssh_err's report from pair
    launches of the inviscid bodies is the full bodies' report."""
    msgs = []
    for on in (True, False):
        m = amd.OceanModel(amd.box_config(200)).set_pair(2).set_inviscid(on).init()
        try:
            m.step(2, check_every=1).synchronize()
            s = m.download(0, "ssh")
            s[60:140, 60:140] = 2.0e4
            for nm in ("ssh", "sshn", "sshp"):
                m.upload(0, nm, s)
            m.step(3, check_every=0).synchronize()
            with pytest.raises(amd.OcnError) as e:
                m.step(4, check_every=1).synchronize()
            assert m.pair_active and m.onepass_inviscid == on
            msgs.append(str(e.value))
        finally:
            m.close()
    assert msgs[0] == msgs[1], msgs
