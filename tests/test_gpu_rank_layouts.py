"""GPU sweep over rank layouts in which a rank holds SEVERAL blocks and ranks differ (tests/shapes.py
RANK_LAYOUTS; tests/test_shapes_cpu.py asserts what each layout reaches, tests/test_halo_plan_cpu.py its
halo plans point by point): loopback ranks (threads of one process, at most 4), every field of every
block bitwise against the CPU oracle.  Tolerance: none.

Every other multi-rank test gives each rank exactly one block.  Here a halo plan mixes local device
copies with messages at depths 1, 2 and 4 (the tracers at their own depth), block batching and the
march + tracer co-launch run over a rank's several blocks under a communicator, the x2 steps and x4 pairs
overlap an inner launch per block with an exchange that is partly a copy, h_r's copy is refreshed every
call, and ranks hold different numbers and sizes of blocks -- so whatever a rank would decide from its own
blocks alone differs between ranks: every rank must still report the same paths.

Calls [2, 2, 3] with a synchronize() after the first two, as tests/test_gpu_shapes.py
test_rank_grids_match_oracle (the third call votes with the known-constant verdict read and runs the x4
pair where the rules allow it).  The one-tracer layout's last call has 5 steps: a co-launch needs a tracer
step pending when a march is launched, and a 3-step call is an opening pair or step (none pending yet)
and the last step.  Only the known-constant variant's march co-launches (sw_kernels.hip
MarchStep::kCoTracer), so the class `general` must report none.  A test loops over its input classes and
reports every failing class.
"""
import pytest

from tests import shapes as S
from tests.test_gpu_shapes import _drive, _model

pytestmark = pytest.mark.gpu

CALLS = [2, 2, 3]
CALLS_CO = [2, 2, 5]   # the one-tracer layout (see above)


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _classes(shape):
    return ("noise", "general") if shape.tracers else ("noise", "hr", "general")


def _run_layout(amd, shape, nranks, cls, overlap=None, x4=None, co=None, params=None, want=None, watchdog=None):
    """The layout over loopback ranks through CALLS; returns the list of what went wrong.  want: the path
    flags expected on every rank (default: tests/shapes.py expect_x2 / expect_x4 with peers)."""
    assert nranks <= 4
    want_blocks = S.rank_blocks(shape, nranks)
    calls = CALLS_CO if shape.tracers == 1 else CALLS
    models = [_model(amd, shape, rank=r, nranks=nranks, overlap=overlap, x4=x4, params=params) for r in range(nranks)]
    try:
        for m in models:
            if co is not None:
                m.set_co_launch(co)
            if watchdog:
                m.set_watchdog(watchdog)
        amd.OceanModel.attach_loopback(models)

        def body(m):
            flags = _drive(m, shape, cls, calls, nsync=2, params=params)
            return flags, m.co_launched

        res = amd.run_ranks(models, body)
        get = S.model_getter(models)
        ref = S.reference(shape, cls, sum(calls), params=params)
        assert get.blocks == set(ref), (get.blocks, set(ref))
        have_blocks = [sorted((b.bm, b.bn) for b in m.blocks) for m in models]
        bad = S.mismatches(ref, get)
    finally:
        for m in models:
            m.close()
    out = []
    if bad:
        out.append(f"fields differ from the oracle: {bad}")
    if have_blocks != want_blocks:
        out.append(f"blocks per rank {have_blocks}, wanted {want_blocks}")
    want = want or {"x2": S.expect_x2(shape), "x4": S.expect_x4(shape, cls, 1 if x4 is None else x4, peers=True)}
    got = [{k: f[-1][k] for k in want} for f, _ in res]
    if got != [want] * nranks:   # every rank the same paths, and the expected ones
        out.append(f"path flags per rank {got}, wanted {want} on every rank")
    if shape.tracers == 1:   # the march and the tracer step of a rank's blocks as one launch
        want_co = co is not False and cls == "noise"
        if [c for _, c in res] != [want_co] * nranks:
            out.append(f"co_launched per rank {[c for _, c in res]}, wanted {want_co}")
    return out


def _sweep(amd, shape, nranks, classes, **opts):
    failures = [f"{cls}: {msg}" for cls in classes for msg in _run_layout(amd, shape, nranks, cls, **opts)]
    assert not failures, f"{S.layout_id(shape, nranks)} {opts}: " + "; ".join(failures)


@pytest.mark.parametrize("overlap", [1, 2, -1], ids=["ov1", "ov2", "auto"])
@pytest.mark.parametrize("shape,nranks", S.RANK_LAYOUTS, ids=[S.layout_id(s, n) for s, n in S.RANK_LAYOUTS])
def test_rank_layouts_match_oracle(amd, shape, nranks, overlap):
    _sweep(amd, shape, nranks, _classes(shape), overlap=overlap)


def test_rank_layout_tracers_x4_always(amd):
    """OCN_OPT_X4 3 on the one-tracer layout: the same pairs as auto takes with peers."""
    _sweep(amd, S.Shape(17, 19, (2, 2), 1), 2, ("noise", "general"), x4=3)


def test_rank_layout_tracers_without_co_launch(amd):
    """OCN_OPT_CO_LAUNCH off: the march batch and the tracer-step batch of a rank's blocks as two launches."""
    _sweep(amd, S.Shape(17, 19, (2, 2), 1), 2, ("noise", "general"), co=False)


def test_rank_layout_coast_still_water(amd):
    """The coastline sweep's still and abyss classes (every wet row takes both IEEE re-runs) on the rough
    mask with dropped blocks, ranks of 2, 2 and 3 blocks."""
    shape = S.Shape(36, 36, (3, 3), 0, "rough_drop")
    assert (shape.W, shape.H) in S.STILL_SHAPES
    _sweep(amd, shape, 3, ("still", "abyss"))


def test_rank_without_blocks(amd):
    """Blocks (3, 1) and (4, 1) of a 4 x 1 grid all land, over 2 ranks: rank 1 owns nothing (the reference
    allows it).  Its context takes part in every vote and in synchronize's reduction with an empty block
    list; rank 0's exchanges are all local copies.  The empty rank has no exchange of its own, so it
    votes against the x2 steps (ocn_ctx.hip x2_local) and every rank runs the hybrid one-pass steps -- the
    path flags pin that; the results are the oracle's bit for bit.  A watchdog of 5 s ends the run should
    a rank ever wait for the other."""
    shape, nranks = S.EMPTY_RANK
    failures = [f"{cls}: {msg}" for cls in ("noise", "general")
                for msg in _run_layout(amd, shape, nranks, cls, want={"x2": False, "x4": False}, watchdog=5.0)]
    assert not failures, f"{S.layout_id(shape, nranks)}: " + "; ".join(failures)


def test_rank_layout_coarse_grid(amd):
    """The parameter sweep's `coarse` set (adjacent rows' metrics differ by percents, tau 30): a band launch
    that took its row table from the wrong local block would show in the high bits."""
    _sweep(amd, S.Shape(17, 19, (2, 2)), 2, ("noise", "hr", "general"), params="coarse")


@pytest.mark.parametrize("tracers,seed", [(0, 610), (1, 611)])
def test_random_sequences_two_blocks_per_rank(amd, tracers, seed):
    """tests/test_gpu_multirank.py's seeded random entry sequences on 2 x 2 blocks over 2 ranks (1 x 2
    blocks per rank): every field of every block, and every read, bitwise against the oracle's replay."""
    from tests.test_gpu_multirank import _ranks_sequence
    _ranks_sequence(amd, seed, 20, tracers=tracers, grid=(2, 2), nranks=2)
