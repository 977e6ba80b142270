"""GPU coastline sweep: the march paths of tests/test_gpu_shapes.py (one-pass, pair, multi-step, x2,
x4, the ensemble launch, loopback ranks, tracer steps) on basins with a coast INSIDE every tile, bitwise
against the CPU oracle -- the same drive, comparison and path-flag assertions as the shape sweep, whose
boxes have no land but the frame and whole dropped blocks.

Masks (tests/shapes.py MASK_KINDS; tests/test_shapes_cpu.py asserts what each promises): rough (one-point
seas and islands, diagonal touches), checker (no velocity point wet), diag (walls across every tile edge,
h-points with 1, 2, 3 and 4 sea corners), comb (channels one point wide), rough_drop (rough plus two
dropped blocks).  What they pin in sw_kernels.hip: the mask bytes unpacked per lane and shifted to the
m +- 1 lanes, the mask formed as a double from a bit, the sea counts at the h-points (three sea corners:
udiv by 3; else rcp_sea), the Fallback loads where the reference stores nothing, the predicated stores,
the count of checked points, the own bits of the x2 / x4 producers and k_bits_x4's mask bytes on the
widened halo, which a rectangular box cannot tell from the block's own.

Input classes: the sweep's, and `still` and `abyss` (tests/shapes.py): velocities of 1e-290 / 2e-305 on
still water, so that every row with a wet velocity point takes both IEEE re-runs of MarchStep::iteration
(derive<true> and step<true>) in every step of every call -- in the pair launch's producer and consumer
waves, the multi-step launch, the ensemble launch, the x2 steps and the x4 pairs, not only in the first
single one-pass steps.  still shows that the re-runs do no harm; only abyss lies where udiv without them
gives other bits (about one quotient in a thousand), so it is the class that fails when a re-run is lost.

The flag cases run all 8 settings of (full_free_surface, trans_terms, ksw_lat): one-pass steps exactly
when all three are on (ocn_ctx.hip ocn_ctx_step, decide), the role-flip or stage path otherwise.

Tolerance: none.  A coast must not push a run onto another path: every case asserts the path flags the
shape sweep asserts.
"""
import pytest

from tests import shapes as S
from tests.test_gpu_ensemble import OK, _bad, _calls, _start
from tests.test_gpu_shapes import OVERLAP2, SINGLE_MODES, _drive, _grid_failures, _model, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _base_id(shape):
    return shape._replace(mask=None, tracers=0).id


# ---------------------------------------------------------------- one block
SINGLE_CASES = [(s, md) for s in S.COAST_SINGLE for md in SINGLE_MODES]


@pytest.mark.parametrize("shape,mode", SINGLE_CASES, ids=[f"{s.id}-{md}" for s, md in SINGLE_CASES])
def test_single_block_coasts_match_oracle(amd, shape, mode):
    opts, calls, _, want = SINGLE_MODES[mode]
    failures = []
    for cls in S.coast_classes(shape):
        # the general class in the pair mode: known constants off, so the general-variant pair runs
        kc = False if (cls == "general" and mode.startswith("pair")) else None
        bad, flags = _run(amd, shape, cls, calls, kc=kc, **opts)
        if bad:
            failures.append(f"{cls}: fields differ from the oracle: {bad}")
        got = {k: flags[-1][k] for k in want}
        if got != want or not flags[0]["one"]:
            failures.append(f"{cls}: path flags {flags}, wanted {want} after the verdict and one-pass steps throughout")
    assert not failures, f"{shape.id} ({mode}): " + "; ".join(failures)


# ---------------------------------------------------------------- several blocks in one process
GRID_CASES = [(s, x4, ov) for s in S.COAST_GRIDS for ov in (1, 2) if ov == 1 or _base_id(s) in OVERLAP2
              for x4 in (0, 1)]


@pytest.mark.parametrize("shape,x4,overlap", GRID_CASES, ids=[f"{s.id}-x4_{x}-ov{o}" for s, x, o in GRID_CASES])
def test_block_grid_coasts_match_oracle(amd, shape, x4, overlap):
    """x2 steps and x4 pairs wherever the block sizes allow them (tests/shapes.py expect_x2 / expect_x4,
    with the dropped blocks read from the mask): the neighbours' mask bytes on the widened halo differ
    from the block's own edge there."""
    failures = _grid_failures(amd, shape, x4, overlap, classes=S.coast_classes(shape))
    assert not failures, f"{shape.id} (x4 {x4}, overlap {overlap}): " + "; ".join(failures)


TRACER_CASES = [(s, x4) for s in S.COAST_TRACER_GRIDS for x4 in (1, 3)]


@pytest.mark.parametrize("shape,x4", TRACER_CASES, ids=[f"{s.id}-x4_{x}" for s, x in TRACER_CASES])
def test_tracer_block_grid_coasts_match_oracle(amd, shape, x4):
    failures = _grid_failures(amd, shape, x4, 1, classes=S.coast_classes(shape))
    assert not failures, f"{shape.id} (x4 {x4}): " + "; ".join(failures)


# ---------------------------------------------------------------- loopback ranks, one block each
@pytest.mark.parametrize("cls", ["noise", "still", "abyss"])
@pytest.mark.parametrize("shape", S.COAST_RANK_GRIDS, ids=[s.id for s in S.COAST_RANK_GRIDS])
def test_rank_grid_coasts_match_oracle(amd, shape, cls):
    """One block per loopback rank, calls [2, 2, 3] with a synchronize() after the first two (see
    tests/test_gpu_shapes.py test_rank_grids_match_oracle): the third call votes with the verdict known
    and runs the x4 pair where the rules allow it."""
    nranks = shape.grid[0] * shape.grid[1]
    models = [_model(amd, shape, rank=r, nranks=nranks) for r in range(nranks)]
    try:
        amd.OceanModel.attach_loopback(models)
        flags = amd.run_ranks(models, lambda m: _drive(m, shape, cls, [2, 2, 3], nsync=2))
        get = S.model_getter(models)
        ref = S.reference(shape, cls, 7)
        assert get.blocks == set(ref) and all(len(m.blocks) == 1 for m in models)
        bad = S.mismatches(ref, get)
    finally:
        for m in models:
            m.close()
    assert not bad, f"{shape.id} over {nranks} ranks ({cls}): fields differ from the oracle: {bad}"
    want = {"x2": S.expect_x2(shape), "x4": S.expect_x4(shape, cls, 1, peers=True)}
    got = [{k: f[-1][k] for k in want} for f in flags]
    assert got == [want] * nranks, (flags, want)


# ---------------------------------------------------------------- ensembles
@pytest.mark.parametrize("members", ["mixed", "deep"])
@pytest.mark.parametrize("shape", S.COAST_ENSEMBLES, ids=[s.id for s in S.COAST_ENSEMBLES])
def test_ensemble_coasts_match_oracle(amd, shape, members):
    """mixed: six members of three variants (known-constant: plain, noise and still; h_r-read; general)
    in one launch per group, as tests/test_gpu_ensemble.py test_mixed_members has them on the box.
    deep: abyss, noise, abyss -- one known-constant group whose members differ in mu, two of them where
    the IEEE re-runs change the bits (tests/shapes.py abyss)."""
    classes, calls = (S.COAST_ENSEMBLE_CLASSES if members == "mixed" else S.COAST_ENSEMBLE_DEEP), [2, 5]
    groups, biggest = (3, 4) if members == "mixed" else (1, 3)
    e = _start(amd, shape, classes)
    try:
        infos, launches, st = _calls(e, calls)
        bad = _bad(e, shape, classes, sum(calls))
    finally:
        e.close()
    assert st == [OK] * len(classes) and not bad, (st, bad)
    assert [(i["groups"], i["batched"]) for i in infos] == [(0, 0), (groups, len(classes))], infos
    assert infos[1]["max_group"] == biggest, infos[1]
    assert launches[1] == groups, launches   # one launch per group, nothing else


# ---------------------------------------------------------------- the SWConfig flags
def _flag_model(amd, shape, flags, **kw):
    return amd.OceanModel(amd.BasinConfig(nx=shape.W + 4, ny=shape.H + 4, mask=S.mask_of(shape)),
                          amd.SWConfig(**S.sw_kwargs(shape, flags)), amd.ParallelConfig(*shape.grid), **kw)


@pytest.mark.parametrize("flags", S.FLAG_SETTINGS, ids=["ffs%d_trans%d_ksw%d" % f for f in S.FLAG_SETTINGS])
@pytest.mark.parametrize("shape", S.COAST_FLAG_SHAPES, ids=[s.id for s in S.COAST_FLAG_SHAPES])
def test_flag_settings_match_oracle(amd, shape, flags):
    """All 8 settings of (full_free_surface, trans_terms, ksw_lat) on a rough coast, noise inputs: one-pass
    steps exactly when all three are on (ocn_ctx.hip decide: one_call needs ca, i.e. full_free_surface 1,
    and trans_terms and ksw_lat on).  The block grid at both overlap levels.

    trans_terms = 0 with full_free_surface = 1 on several blocks once left the p-level depths wrong on
    the halo ring: the reuse steps do not exchange hh_update's n levels, a9 forms the p levels on the ring
    from them, and without uv_trans's exchange nothing rewrites those (ocn_ctx.hip reuse_allowed)."""
    cls, calls = "noise", [2, 5]
    ref = S.reference(shape, cls, sum(calls), flags)
    for overlap in ((1, 2) if shape.grid != (1, 1) else (None,)):
        m = _flag_model(amd, shape, flags)
        try:
            if overlap is not None:
                m.set_overlap(overlap)
            path = _drive(m, shape, cls, calls)
            get = S.model_getter([m])
            assert get.blocks == set(ref), (get.blocks, set(ref))
            bad = S.mismatches(ref, get)
        finally:
            m.close()
        assert not bad, f"{shape.id} flags {flags} overlap {overlap}: fields differ from the oracle: {bad}"
        # (the first call follows an ssh upload: with tracers its steps wait for hh_init's depths, so only the
        # call after the verdict is pinned to one-pass steps; without all three flags no call has any)
        assert path[-1]["one"] == (flags == (1, 1, 1)), (flags, path)
        assert flags == (1, 1, 1) or not any(p["one"] for p in path), (flags, path)


@pytest.mark.parametrize("flags", [(1, 0, 1), (1, 0, 0), (0, 1, 1)], ids=["ffs%d_trans%d_ksw%d" % f for f in
                                                                           [(1, 0, 1), (1, 0, 0), (0, 1, 1)]])
def test_rank_flag_settings_match_oracle(amd, flags):
    """The same over loopback ranks (one block each, no tracer): the decision is the same on every rank."""
    shape, cls = S.COAST_RANK_GRIDS[1], "noise"
    nranks = shape.grid[0] * shape.grid[1]
    models = [_flag_model(amd, shape, flags, rank=r, nranks=nranks) for r in range(nranks)]
    try:
        amd.OceanModel.attach_loopback(models)
        paths = amd.run_ranks(models, lambda m: _drive(m, shape, cls, [2, 2, 3], nsync=2))
        get = S.model_getter(models)
        ref = S.reference(shape, cls, 7, flags)
        assert get.blocks == set(ref)
        bad = S.mismatches(ref, get)
    finally:
        for m in models:
            m.close()
    assert not bad, f"{shape.id} over {nranks} ranks, flags {flags}: fields differ from the oracle: {bad}"
    assert not any(p["one"] for path in paths for p in path), paths
