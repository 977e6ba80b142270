"""CPU checks of the two-step launch's tile plan (include/ocn_sw.h ocn_pair_plan, ocn_set_pair_rows): pure host
code, no device.  The plan is the rule the launches had before it became a function of its own (restated here),
up to 150 rows; the inviscid bodies (nv) share the cap -- a cap of 300 rows for them (4096^2 in one round of
293-row tiles, 301 iterations) was measured and not kept, so nv changes no plan."""
import ctypes as C
import os

import pytest

CAP = {0: 150, 1: 150}        # OCN_PAIR_MAX_ROWS, for the full and the inviscid bodies alike
COLS = 116                    # a workgroup's output columns (MarchStep::kPairCols)
SLOTS = 256 * 4 * 2           # wave slots of the chip for the two-step launch (two waves per SIMD)


@pytest.fixture(scope="module")
def lib():
    import ocean_model_arch_amd as amd
    if not os.path.exists(amd._lib.LIB_PATH):
        amd.build()
    return amd.lib()


@pytest.fixture(autouse=True)
def _automatic(lib):
    """Every test starts and ends with the automatic height (the process may have OCN_PAIR_ROWS set)."""
    assert lib.ocn_set_pair_rows(0) == 0
    yield
    assert lib.ocn_set_pair_rows(0) == 0


def _plan(lib, w, h, mult, nv):
    rows, rounds, its = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.ocn_pair_plan(w, h, mult, nv, C.byref(rows), C.byref(rounds), C.byref(its)) == 0
    return rows.value, rounds.value, its.value


def _formula(w, h, mult, cap):
    """pair_rows as the launches had it (cap 150): the fewest rounds x (rows + 8), the smallest such height."""
    wx = (w - 1 + COLS) // COLS
    best, cost, rnd = 8, -1, 0
    for rows in range(8, cap + 1):
        tiles = (h + rows - 1) // rows
        waves = 4 * tiles * wx * mult
        rounds = (waves + SLOTS - 1) // SLOTS
        c = rounds * (rows + 8)
        if cost < 0 or c < cost:
            best, cost, rnd = rows, c, rounds
    return best, rnd, cost


def test_bench_box(lib):
    assert _plan(lib, 4096, 4096, 1, 0) == (147, 2, 310)      # what the launches chose before
    assert _plan(lib, 4096, 4096, 1, 1) == (147, 2, 310)      # the inviscid bodies: the same cap, the same plan


@pytest.mark.parametrize("nv", [0, 1])
@pytest.mark.parametrize("wh", [(200, 200), (117, 40)])
def test_small_blocks_keep_8_rows(lib, wh, nv):
    assert _plan(lib, wh[0], wh[1], 1, nv) == (8, 1, 16)


def test_batch_of_blocks_equals_the_earlier_rule(lib):
    assert _plan(lib, 1024, 2048, 8, 0) == _formula(1024, 2048, 8, 150)


@pytest.mark.parametrize("nv", [0, 1])
def test_plans_follow_the_rule_within_the_cap(lib, nv):
    for w, h, mult in [(1, 1, 1), (58, 300, 1), (117, 300, 1), (1024, 2048, 1), (1024, 2048, 8), (2048, 1024, 4),
                       (4096, 4096, 1), (4096, 4096, 3), (8192, 8192, 1), (16384, 16384, 2), (71, 79, 8), (5000, 301, 1)]:
        got = _plan(lib, w, h, mult, nv)
        assert got == _formula(w, h, mult, CAP[nv]), (w, h, mult, nv)
        assert 8 <= got[0] <= CAP[nv] and got[1] >= 1 and got[2] == got[1] * (got[0] + 8)


def test_fixed_height_is_clipped_to_the_cap(lib):
    for fixed in (8, 147, 150, 151, 246, 247, 293, 300, 301, 100000):
        assert lib.ocn_set_pair_rows(fixed) == 0
        for nv in (0, 1):
            rows, rounds, its = _plan(lib, 4096, 4096, 1, nv)
            assert rows == min(fixed, CAP[nv]), (fixed, nv)
            tiles = -(-4096 // rows)
            assert rounds == -(-4 * tiles * 36 // SLOTS) and its == rounds * (rows + 8)
    assert lib.ocn_set_pair_rows(0) == 0
    assert _plan(lib, 4096, 4096, 1, 1) == (147, 2, 310)


def test_bad_arguments(lib):
    from ocean_model_arch_amd import _lib
    r, q, i = C.c_int(), C.c_int(), C.c_int()
    ok = (C.byref(r), C.byref(q), C.byref(i))
    for k in range(3):
        a = list(ok)
        a[k] = None
        assert lib.ocn_pair_plan(100, 100, 1, 1, *a) == _lib.OCN_ERR_ARG
    for w, h, mult in [(0, 100, 1), (100, 0, 1), (-5, 100, 1), (100, -1, 1), (100, 100, 0), (100, 100, -2)]:
        assert lib.ocn_pair_plan(w, h, mult, 0, *ok) == _lib.OCN_ERR_ARG
    for rows in (-1, 1, 7):
        assert lib.ocn_set_pair_rows(rows) == _lib.OCN_ERR_ARG
    assert _plan(lib, 4096, 4096, 1, 1) == (147, 2, 310)      # a refused value changes nothing


def test_wrappers(lib):
    from ocean_model_arch_amd import _lib
    assert _lib.pair_plan(4096, 4096) == (147, 2, 310)
    assert _lib.pair_plan(4096, 4096, nv=False) == (147, 2, 310)
    _lib.set_pair_rows(200)
    try:
        assert _lib.pair_plan(4096, 4096)[0] == 150 and _lib.pair_plan(4096, 4096, nv=False)[0] == 150
        _lib.set_pair_rows(64)
        assert _lib.pair_plan(4096, 4096)[0] == 64
    finally:
        _lib.set_pair_rows(0)
    with pytest.raises(_lib.OcnError):
        _lib.set_pair_rows(3)
