"""GPU parity of the inviscid pair bodies with the guard folded into the range-check accumulator (sw_kernels.hip
MarchStepT NV, StepRegs::mark), on the tallest tiles the pair launch has.  Bitwise against the CPU oracle;
tolerance: none.

Blocks of 300 rows (widths 117: a second strip of one column; 58: half a strip; one rough coast) with the tile
height fixed by ocn_set_pair_rows: 293 rows are asked for (the height a 4096^2 box would take in one round) and
every body clips that to the cap of 150 -- two tiles of 150 rows, 160 rows of row constants in LDS -- where the
automatic plan of such a block is 8 rows.  The helpers are tests/test_gpu_inviscid.py's.
"""
import numpy as np
import pytest

from tests import shapes as S
from tests.test_gpu_inviscid import FIELDS, _bad, _check_flags, _drive, _oracle
from tests.test_gpu_parity import bits_equal

pytestmark = pytest.mark.gpu

CALLS = [2, 5, 1, 6]
SHAPES = [S.Shape(117, 300), S.Shape(58, 300), S.Shape(117, 300, mask="rough")]
ASKED, CAP = 293, 150      # the fixed height asked for; what every two-step body clips it to


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _size(shape):
    """The interior the pair launch covers (one block: the shape's box)."""
    assert shape.grid == (1, 1)
    return shape.W, shape.H


# ---------------------------------------------------------------- tall tiles, on and off
@pytest.mark.parametrize("cls", ["plain", "noise"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
def test_tall_tiles_on_and_off_match_oracle(amd, shape, cls):
    ups = S.uploads_for(shape, cls)
    ref = S.reference(shape, cls, sum(CALLS))
    w, h = _size(shape)
    assert h == 300
    try:
        amd._lib.set_pair_rows(ASKED)
        assert amd._lib.pair_plan(w, h, 1, True)[0] == CAP       # clipped, for the inviscid bodies
        assert amd._lib.pair_plan(w, h, 1, False)[0] == CAP      # and for the full ones
        for on in (True, False):
            flags, got = _drive(amd, shape, ups, on)
            bad = _bad(ref, got)
            assert not bad, f"{shape.id} {cls} inviscid {on}: fields differ from the oracle: {bad}"
            _check_flags(flags, on, f"{shape.id} {cls}")
            assert all(f["zero"] for f in flags), flags
    finally:
        amd._lib.set_pair_rows(0)


# ---------------------------------------------------------------- the guard deep in a tall tile
def _on_equals_off(amd, shape, ups, calls, what):
    """check_every = 0 runs with the inviscid bodies on and off: equal byte for byte over bench.DUMP_FIELDS, the
    non-finite values where the oracle's are."""
    import bench
    ref = _oracle(shape, ups, calls, check=False)
    runs = {}
    for on in (True, False):
        flags, got = _drive(amd, shape, ups, on, calls, check_every=0)
        assert flags[1]["pair"] and flags[1]["nv"] == on, (what, flags)
        runs[on] = got[(1, 1)]
    assert set(bench.DUMP_FIELDS) <= set(FIELDS)
    for nm in bench.DUMP_FIELDS:
        assert bits_equal(runs[True][nm], runs[False][nm]), f"{what} {nm}: the inviscid run differs from the full run"
        assert np.array_equal(np.isfinite(runs[True][nm]), np.isfinite(ref[(1, 1)][nm])), \
            f"{what} {nm}: non-finite values elsewhere"
    return runs[True]


@pytest.mark.parametrize("value", [np.inf, np.nan, 1.0e305], ids=["inf", "nan", "1e305"])
def test_guard_on_a_tall_tile_on_equals_off(amd, value):
    """inf, nan or 1e305 at a sea point of ubrtr in interior row 280, column 116: row 130 of the second 150-row tile,
    the last column of the first strip -- a lane that is clean for most of its tile and marked from there on."""
    shape = S.Shape(117, 300)
    om = S.oracle_model(shape)
    u = om.f[0]["ubrtr"].copy(order="F")
    i, j = 2 + 115, 2 + 279
    assert om.f[0]["lcu"][i, j] > 0.5
    u[i, j] = value
    ups = {(1, 1): {"ubrtr": u, "ubrtrn": u.copy(order="F")}}
    try:
        amd._lib.set_pair_rows(ASKED)
        got = _on_equals_off(amd, shape, ups, [2, 4], f"{value}")
    finally:
        amd._lib.set_pair_rows(0)
    assert not np.isfinite(got["ubrtr"]).all()


# ---------------------------------------------------------------- a marked wave that meets tiny dividends
def _abyss_mu0(shape):
    ups = {(1, 1): dict(S.uploads("abyss", S.oracle_model(shape))[(1, 1)])}
    del ups[(1, 1)]["mu"]      # mu stays +0.0: the inviscid bodies run
    return ups


@pytest.mark.parametrize("rows", [0, ASKED], ids=["auto8", "cap150"])
def test_marked_wave_with_tiny_dividends_on_equals_off(amd, rows):
    """tests/shapes.py abyss with mu left +0.0 (velocities of 2e-305: every wet row's own range checks ask for the
    IEEE re-run) and 1e305 at one sea point of ubrtr: the marked waves' rows take the marked path -- the full
    body's udiv pass with all its checks -- and then the IEEE re-run those checks ask for."""
    shape = S.Shape(117, 300)
    ups = _abyss_mu0(shape)
    om = S.oracle_model(shape)
    i, j = 2 + 60, 2 + 150
    assert om.f[0]["lcu"][i, j] > 0.5
    for nm in ("ubrtr", "ubrtrn"):
        ups[(1, 1)][nm] = ups[(1, 1)][nm].copy(order="F")
        ups[(1, 1)][nm][i, j] = 1.0e305
    w, h = _size(shape)
    try:
        amd._lib.set_pair_rows(rows)
        assert amd._lib.pair_plan(w, h, 1, True)[0] == (CAP if rows else 8)
        got = _on_equals_off(amd, shape, ups, [2, 4], f"rows {rows}")
    finally:
        amd._lib.set_pair_rows(0)
    assert not np.isfinite(got["ubrtr"]).all()


def test_tiny_dividends_on_a_tall_tile_match_oracle(amd):
    """abyss with mu left +0.0, no plant, 150-row tiles: the unmarked waves' IEEE re-runs, against the oracle."""
    shape = S.Shape(117, 300)
    ups = _abyss_mu0(shape)
    ref = _oracle(shape, ups)
    try:
        amd._lib.set_pair_rows(ASKED)
        for on in (True, False):
            flags, got = _drive(amd, shape, ups, on)
            bad = _bad(ref, got)
            assert not bad, f"inviscid {on}: fields differ from the oracle: {bad}"
            _check_flags(flags, on, shape.id)
    finally:
        amd._lib.set_pair_rows(0)
