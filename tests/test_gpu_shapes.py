"""GPU shape sweep: the one-pass, pair (two steps per launch), multi-step, x2 and x4 marches at the
block shapes where their launch geometry changes, bitwise against the CPU oracle on rough,
non-symmetric, halo-consistent state (tests/shapes.py: the shapes, the four input classes, the
reference and the comparison; tests/test_shapes_cpu.py: those inputs are sound).

Boundaries probed: a one-pass / x2 wave's 60 output columns and a pair / x4 workgroup's 116 (interior
widths 59 / 60 / 61, 116 / 117, 120 / 121: a last column tile one point wide), tile heights from the
cost models with a last tile of one row, blocks lower than the shortest pair tile, x2's 2 x 2 and x4's
4 x 4 block minimum, inner parts (overlap level 2) that are empty or one point wide, the E / W band
widths' switch at blocks 180 / 348 wide, neighbour tables with holes (dropped all-land blocks: a
diagonal neighbour with neither side neighbour at its corner, where the hybrid last step once left
the corner halo of the depths' p and n levels stale -- ocn_ctx.hip side_fed), and h_r's copy
exchanged 4 rings deep between blocks 2-3 points wide (ocn_ctx.hip refresh_hrx).

Every run: uploads, a first call of 2 steps, synchronize() (the known-constant verdict reaches the
host), the rest; then every field of every block against the oracle.  Tolerance: none.  A test loops
over its input classes and reports every failing class.
"""
import pytest

from tests import shapes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _model(amd, shape, rank=0, nranks=1, multi=None, pair=None, x4=None, overlap=None, kc=None, params=None,
           flags=(1, 1, 1)):
    """params: a parameter set of tests/shapes.py PARAMS (its grid and SW keywords; None: the defaults)."""
    sw = amd.SWConfig(**S.sw_kwargs(shape, flags, params))
    m = amd.OceanModel(amd.BasinConfig(mask=S.mask_of(shape), **S.basin_kwargs(shape, params)), sw,
                       amd.ParallelConfig(*shape.grid), rank=rank, nranks=nranks)
    if multi is not None:
        m.set_multi(multi)
    if pair is not None:
        m.set_pair(pair)
    if x4 is not None:
        m.set_x4(x4)
    if overlap is not None:
        m.set_overlap(overlap)
    if kc is not None:
        m.set_known_constants(kc)
    return m


def _drive(m, shape, cls, calls, nsync=1, params=None):
    """init, the class's uploads to m's blocks, the calls at the parameter set's tau (1.0 without one;
    synchronize() after each of the first nsync); returns the path flags after each call."""
    m.init()
    ups = S.uploads_for(shape, cls, params)
    tau = S.tau_of(params)
    for b in m.blocks:
        for nm, a in ups.get((b.bm, b.bn), {}).items():
            m.upload(b.k, nm, a)
    flags = []
    for i, n in enumerate(calls):
        m.step(n, tau=tau, check_every=1)
        if i < nsync:
            m.synchronize()   # the known-constant verdict reaches the host
        flags.append({"one": m.onepass_active, "multi": m.multi_active, "pair": m.pair_active,
                      "x2": m.x2_active, "x4": m.x4_active})
    m.synchronize()
    return flags


def _run(amd, shape, cls, calls, params=None, **opts):
    m = _model(amd, shape, params=params, **opts)
    try:
        flags = _drive(m, shape, cls, calls, params=params)
        get = S.model_getter([m])
        ref = S.reference(shape, cls, sum(calls), params=params)
        assert get.blocks == set(ref), (get.blocks, set(ref))
        bad = S.mismatches(ref, get)
    finally:
        m.close()
    return bad, flags


# ---------------------------------------------------------------- one block
# mode -> (options, calls, input classes, flags expected on the call after the verdict)
SINGLE_MODES = {
    # the rest of the call as ONE multi-step launch with a grid barrier (ocn_ctx.hip multi_ok holds on
    # every shape here: one block, no ring work, a variant chosen on the host, a grid of at most 190
    # workgroups -- sw_kernels.hip multi_rows, kMultiMaxTiles 256)
    "default": ({}, [2, 5], ("plain", "general"), {"one": True, "multi": True, "pair": False}),
    "nomulti": ({"multi": False}, [2, 5], ("plain", "general"), {"one": True, "multi": False, "pair": False}),
    # two steps per launch forced below the 512^2 default: [2, 6] ends in a pair, [2, 5] in a single step
    "pair26": ({"multi": False, "pair": 2}, [2, 6], S.CLASSES, {"one": True, "multi": False, "pair": True}),
    "pair25": ({"multi": False, "pair": 2}, [2, 5], S.CLASSES, {"one": True, "multi": False, "pair": True}),
}


@pytest.mark.parametrize("shape,mode", [(s, md) for s in S.SINGLE for md in SINGLE_MODES],
                         ids=[f"{s.id}-{md}" for s in S.SINGLE for md in SINGLE_MODES])
def test_single_block_shapes_match_oracle(amd, shape, mode):
    opts, calls, classes, want = SINGLE_MODES[mode]
    failures = []
    for cls in classes:
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
# overlap level 2 (the inner part beside the exchange, then the bands): the grids whose x2 / x4 inner
# part is empty or one point wide, and the band-width switch
OVERLAP2 = ["7x9_b3x2", "10x6_b5x3", "13x11_b3x3", "9x8_b2x2", "16x16_b2x2", "17x19_b2x2", "27x27_b3x3",
            "361x12_b2x1", "358x12_b2x1", "700x9_b2x1", "12x700_b1x2"]
GRID_CASES = [(s, x4, ov) for s in S.GRIDS for ov in (1, 2) if ov == 1 or s.id in OVERLAP2 for x4 in (0, 1)]


def _grid_failures(amd, shape, x4, overlap, classes=S.CLASSES, params=None):
    failures = []
    for cls in classes:
        bad, flags = _run(amd, shape, cls, [2, 5], x4=x4, overlap=overlap, params=params)
        if bad:
            failures.append(f"{cls}: fields differ from the oracle: {bad}")
        want = {"x2": S.expect_x2(shape), "x4": S.expect_x4(shape, cls, x4)}
        got = {k: flags[-1][k] for k in want}
        if got != want:
            failures.append(f"{cls}: path flags {flags}, wanted {want} after the verdict")
    return failures


@pytest.mark.parametrize("shape,x4,overlap", GRID_CASES, ids=[f"{s.id}-x4_{x}-ov{o}" for s, x, o in GRID_CASES])
def test_block_grids_match_oracle(amd, shape, x4, overlap):
    """x2 steps wherever every block is at least 2 x 2, pairs of them (x4) wherever every block is at
    least 4 x 4 and the variant is a known-constant one (tests/shapes.py expect_x2 / expect_x4)."""
    failures = _grid_failures(amd, shape, x4, overlap)
    assert not failures, f"{shape.id} (x4 {x4}, overlap {overlap}): " + "; ".join(failures)


# tracer runs: x2 steps carry the tracers; x4 pairs in one process only with OCN_OPT_X4 3
TRACER_CASES = [(s, 1, 1) for s in S.TRACER_GRIDS] + \
               [(s, 3, ov) for s in (S.Shape(17, 19, (2, 2), 1), S.DROPPED._replace(tracers=2)) for ov in (1, 2)]


@pytest.mark.parametrize("shape,x4,overlap", TRACER_CASES, ids=[f"{s.id}-x4_{x}-ov{o}" for s, x, o in TRACER_CASES])
def test_tracer_block_grids_match_oracle(amd, shape, x4, overlap):
    failures = _grid_failures(amd, shape, x4, overlap)
    assert not failures, f"{shape.id} (x4 {x4}, overlap {overlap}): " + "; ".join(failures)


# ---------------------------------------------------------------- loopback ranks, one block each
@pytest.mark.parametrize("overlap", [1, 2])
@pytest.mark.parametrize("cls", ["noise", "general"])
@pytest.mark.parametrize("shape", S.RANK_GRIDS, ids=[s.id for s in S.RANK_GRIDS])
def test_rank_grids_match_oracle(amd, shape, cls, overlap):
    """One block per loopback rank (the RCCL path's plans, packs and votes; threads of one process):
    h_r's copy refreshed every call, 4 rings deep, between ranks whose blocks are 2-3 points wide.
    Calls [2, 2, 3] with a synchronize() after the first two: with a communicator there is no lazy
    tail, so the 2-step call after an ssh upload (hh_init's depths stale) runs standard steps and
    issues no known-constant check; the second call runs one-pass steps and the check, the third
    votes with the verdict known and runs the x4 pair where the rules allow it."""
    nranks = shape.grid[0] * shape.grid[1]
    assert nranks <= 8
    models = [_model(amd, shape, rank=r, nranks=nranks, overlap=overlap) for r in range(nranks)]
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
    assert not bad, f"{shape.id} over {nranks} ranks ({cls}, overlap {overlap}): fields differ from the oracle: {bad}"
    want = {"x2": S.expect_x2(shape), "x4": S.expect_x4(shape, cls, 1, peers=True)}
    got = [{k: f[-1][k] for k in want} for f in flags]
    assert got == [want] * nranks, (flags, want)
