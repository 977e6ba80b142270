"""The shape sweep's inputs are sound and its comparison has teeth (no GPU: the oracle alone).

For every shape x input class of tests/test_gpu_shapes.py the oracle must run the sweep's longest
call sequence without a FloatingPointError (check_ssh_err), keep every field finite and |ssh| < 1,
and end with a nonzero ubrtr at every interior lcu point of every block -- rough data that moved
everywhere, so a wrong column or row in a kernel cannot reproduce the reference's bits by symmetry
or by leaving zeros.  The comparison helper must name exactly the block and field of a one-ulp change.

The same for the coastline sweep (tests/test_gpu_coast.py): every (shape, mask, class) it runs is finite
and trips no check_ssh_err; the still class stays below udiv's range after every step; every mask kind
has what it promises (tests/shapes.py MASK_KINDS) and a land / sea change across the tiles' column edges.

The rank layouts (tests/shapes.py RANK_LAYOUTS) hold what their table promises: the per-rank block lists
of rank_blocks are the library's own (domain.decompose, every rank), blocks with local and remote
neighbours at once, and the blocks whose x4 inner part is empty.
"""
import numpy as np
import pytest

from tests import shapes as S

ALL = [(s, S.SINGLE_STEPS) for s in S.SINGLE] + [(s, S.GRID_STEPS) for s in S.GRIDS + S.TRACER_GRIDS]


@pytest.mark.parametrize("cls", S.CLASSES)
@pytest.mark.parametrize("shape,steps", ALL, ids=[s.id for s, _ in ALL])
def test_sweep_inputs_are_sound(shape, steps, cls):
    ref = S.reference(shape, cls, steps)   # raises FloatingPointError on a blow-up
    xs, ys = S.block_sizes(shape)
    assert len(ref) == shape.grid[0] * shape.grid[1] - len(S.dropped_blocks(shape))
    for (bm, bn), f in ref.items():
        assert f["ssh"].shape == (xs[bm - 1] + 4, ys[bn - 1] + 4), (bm, bn)
        for nm, a in f.items():
            assert np.isfinite(a).all(), f"({bm},{bn}):{nm} not finite"
        assert np.abs(f["ssh"]).max() < 1.0, (bm, bn, np.abs(f["ssh"]).max())
        inner = (slice(2, -2), slice(2, -2))
        u, lcu = f["ubrtr"][inner], f["lcu"][inner]
        assert (u[lcu > 0.5] != 0.0).all(), f"({bm},{bn}): ubrtr still zero on {(u[lcu > 0.5] == 0.0).sum()} lcu points"


def test_uploads_keep_neighbour_halos_in_agreement():
    """A block's halo columns / rows hold what the neighbour's interior holds (the cut from one global
    array), and each role-flip pair is uploaded equal."""
    shape = S.Shape(13, 11, (3, 3))
    om = S.oracle_model(shape)
    ups = S.uploads("general", om)
    by = {(b.bm, b.bn): b for b in om.blocks}
    for (bm, bn), u in ups.items():
        assert sorted(u) == sorted(["ssh", "sshn", "ubrtr", "ubrtrn", "vbrtr", "vbrtrn", "hhq_rest", "mu", "RHSx", "RHSy"])
        for a, b in (("ssh", "sshn"), ("ubrtr", "ubrtrn"), ("vbrtr", "vbrtrn")):
            assert S.bits_equal(u[a], u[b])
        # the first halo ring is what the library compares with the neighbours (check_coherence); the
        # second ring of the masked state fields follows the block's own masks and initial ssh there
        # (exchanged one ring deep), so only the unmasked fields agree two rings deep
        e = ups.get((bm + 1, bn))
        if e is not None:   # my east halo columns = the east neighbour's first interior columns
            for nm in ("hhq_rest", "mu"):
                assert S.bits_equal(np.asfortranarray(u[nm][-2:, :]), np.asfortranarray(e[nm][2:4, :])), (bm, bn, nm)
            for nm in ("ssh", "ubrtr", "vbrtr"):
                assert S.bits_equal(np.asfortranarray(u[nm][-2, 1:-1]), np.asfortranarray(e[nm][2, 1:-1])), (bm, bn, nm)
        n = ups.get((bm, bn + 1))
        if n is not None:
            for nm in ("hhq_rest", "mu"):
                assert S.bits_equal(np.asfortranarray(u[nm][:, -2:]), np.asfortranarray(n[nm][:, 2:4])), (bm, bn, nm)
            for nm in ("ssh", "ubrtr", "vbrtr"):
                assert S.bits_equal(np.asfortranarray(u[nm][1:-1, -2]), np.asfortranarray(n[nm][1:-1, 2])), (bm, bn, nm)
        assert u["ssh"].shape == by[(bm, bn)].shape
    # rough and not symmetric: the noise differs from its mirror images
    a = ups[(2, 2)]["mu"]
    assert not np.array_equal(a, a[::-1, :]) and not np.array_equal(a, a[:, ::-1]) and not np.array_equal(a, a[::-1, ::-1])


def test_dropped_block_mask_drops_two_blocks():
    om = S.oracle_model(S.DROPPED)
    have = {(b.bm, b.bn) for b in om.blocks}
    assert len(have) == 7 and (2, 2) not in have and (1, 1) not in have
    holes = {(b.bm, b.bn): sorted(set(range(1, 9)) - set(b.nbr)) for b in om.blocks}
    # oracle.DIRS: 1 E, 2 W, 3 N, 4 S, 8 SW -- holes inside the grid on sides and on a diagonal
    assert 1 in holes[(1, 2)] and 4 in holes[(1, 2)] and 3 not in holes[(1, 2)]
    assert 8 in holes[(3, 3)] and 2 not in holes[(3, 3)] and 4 not in holes[(3, 3)]
    assert S.min_block(S.DROPPED) == (12, 12)


def test_expected_paths_follow_the_block_size_rules():
    g = {s.id: s for s in S.GRIDS}
    assert [S.expect_x2(g[k]) for k in ("7x9_b3x2", "10x6_b5x3", "5x3_b5x3", "13x11_b3x3")] == [True, True, False, True]
    assert [S.expect_x4(g[k], "plain", 1) for k in ("7x9_b3x2", "13x11_b3x3", "9x8_b2x2", "16x16_b2x2")] == \
        [False, False, True, True]
    assert not S.expect_x4(g["9x8_b2x2"], "general", 1) and not S.expect_x4(g["9x8_b2x2"], "plain", 0)
    tr = S.Shape(17, 19, (2, 2), 1)
    assert not S.expect_x4(tr, "plain", 1) and S.expect_x4(tr, "plain", 3) and S.expect_x4(tr, "plain", 1, peers=True)
    assert S.min_block(S.Shape(361, 12, (2, 1))) == (180, 12) and S.min_block(S.Shape(358, 12, (2, 1))) == (179, 12)
    assert S.min_block(S.Shape(700, 9, (2, 1))) == (350, 9)


def test_comparison_names_the_block_and_field_of_a_one_ulp_change():
    shape = S.Shape(13, 11, (3, 3))
    ref = S.reference(shape, "general", 3)
    copy = {key: {nm: a.copy(order="F") for nm, a in f.items()} for key, f in ref.items()}
    get = lambda bm, bn, nm: copy[(bm, bn)][nm]   # noqa: E731
    assert S.mismatches(ref, get) == []
    a = copy[(2, 3)]["hhu_n"]
    word = a.view(np.uint64)
    word[-1, 0] ^= np.uint64(1)   # the lowest mantissa bit of a corner halo point
    assert S.mismatches(ref, get) == ["(2,3):hhu_n"]
    word[-1, 0] ^= np.uint64(1)
    b = copy[(1, 1)]["lcu"].view(np.uint32)   # a real(4) field too
    b[0, -1] ^= np.uint32(1)
    assert S.mismatches(ref, get) == ["(1,1):lcu"]
    # the scratch arrays the model does not hold are not compared
    copy[(1, 1)]["lcu"].view(np.uint32)[0, -1] ^= np.uint32(1)
    copy[(1, 1)]["lu1"][0, 0] += 1.0
    assert S.mismatches(ref, get) == []
    # +0.0 against -0.0 is a difference (bitwise, not ==)
    r0 = ref[(3, 1)]["RHSx_dif"][0, 0]   # a bnd corner no kernel writes: +0.0
    assert r0 == 0.0 and not np.signbit(r0)
    copy[(3, 1)]["RHSx_dif"][0, 0] = -0.0
    assert S.mismatches(ref, get) == ["(3,1):RHSx_dif"]


# ---------------------------------------------------------------- the coastline sweep's inputs
COAST = [(s, S.SINGLE_STEPS) for s in S.COAST_SINGLE] + \
        [(s, S.GRID_STEPS) for s in S.COAST_GRIDS + S.COAST_TRACER_GRIDS + S.COAST_RANK_GRIDS]
COAST_ALL = [(s, n, c) for s, n in COAST for c in S.coast_classes(s)] + \
            [(s, S.GRID_STEPS, c) for s in S.COAST_ENSEMBLES for c in ("plain", "noise", "still", "hr", "general", "abyss")]
UDIV_MIN = 2.0 ** -900   # sw_kernels.hip kUdivMinExp: a nonzero dividend below it sends its row to the IEEE re-run


def _sea_corners(mask):
    """The number of sea corners (0 .. 4) of every h-point of a global mask (1 = land)."""
    sea = 1 - mask
    return sea[:-1, :-1] + sea[1:, :-1] + sea[:-1, 1:] + sea[1:, 1:]


@pytest.mark.parametrize("shape,steps,cls", COAST_ALL, ids=[f"{s.id}-{c}" for s, _, c in COAST_ALL])
def test_coast_inputs_are_sound(shape, steps, cls):
    if cls not in ("still", "abyss"):
        ref = S.reference(shape, cls, steps)   # raises FloatingPointError on a blow-up (check_ssh_err)
        assert len(ref) == shape.grid[0] * shape.grid[1] - len(S.dropped_blocks(shape))
        for (bm, bn), f in ref.items():
            for nm, a in f.items():
                assert np.isfinite(a).all(), f"({bm},{bn}):{nm} not finite"
        return
    # still, abyss: after EVERY step 0 < max |u|, |v| < 2^-900 on the wet points (no wet point: all zero), the
    # number of nonzero velocity points unchanged, ssh below the range too
    om = S.oracle_model(shape)
    for k, b in enumerate(om.blocks):
        for nm, a in S.uploads_for(shape, cls).get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    count0 = None
    for step in range(steps + 1):
        if step:
            om.step(1.0)
        count = 0
        for f in om.f:
            for nm, msk in (("ubrtr", "lcu"), ("vbrtr", "lcv")):
                a, wet = np.abs(f[nm]), f[msk] > 0.5
                assert np.isfinite(f[nm]).all() and (a[~wet] == 0.0).all(), (step, nm)
                if wet.any():
                    assert 0.0 < a[wet].max() < UDIV_MIN, (step, nm, a[wet].max())
                count += int((a != 0.0).sum())
            assert np.abs(f["ssh"]).max() < UDIV_MIN, (step, np.abs(f["ssh"]).max())
        count0 = count if count0 is None else count0
        assert count == count0, (step, count, count0)
    wet_any = any((f[m] > 0.5).any() for f in om.f for m in ("lcu", "lcv"))
    assert wet_any == (shape.mask != "checker")


COAST_MASKS = sorted({s._replace(tracers=0) for s, _ in COAST} | set(S.COAST_ENSEMBLES) | set(S.COAST_FLAG_SHAPES),
                     key=lambda s: s.id)


@pytest.mark.parametrize("shape", COAST_MASKS, ids=[s.id for s in COAST_MASKS])
def test_coast_masks_have_what_their_kind_promises(shape):
    shape = shape._replace(tracers=0)
    m = S.mask_of(shape)
    assert m.shape == (shape.W + 4, shape.H + 4) and m.dtype == np.int32
    assert m[:2].all() and m[-2:].all() and m[:, :2].all() and m[:, -2:].all()   # the 2-point land frame
    assert not m[2:-2, 2:-2].all()
    corners = _sea_corners(m)
    sea = 1 - m
    if shape.mask in ("rough", "diag", "rough_drop"):
        assert all((corners == k).any() for k in (1, 2, 3, 4)), [(k, int((corners == k).sum())) for k in range(5)]
    if shape.mask == "checker":   # no u, v or vorticity point wet; every sea point isolated
        assert not (sea[:-1] * sea[1:]).any() and not (sea[:, :-1] * sea[:, 1:]).any() and not (corners == 4).any()
        om = S.oracle_model(shape)
        assert all(f[nm].sum() == 0.0 for f in om.f for nm in ("lcu", "lcv", "luu")) and om.f[0]["lu"].sum() > 0
    if shape.mask == "comb":   # channels one point wide: a sea point with land on both sides in x
        inner = sea[1:-1] * (1 - sea[:-2]) * (1 - sea[2:])
        assert inner.any() and not (corners == 4).any()
        if shape.H >= 6:   # ... joined by a full row every fifth row
            assert sea[2:-2, 2].all() and sea[2:-2, 7].all()
    want = [(1, 1), (2, 2)] if shape.mask == "rough_drop" else []
    assert sorted(S.dropped_blocks(shape)) == want
    # a land / sea change across the output-column edges of the one-pass / x2 and the pair / x4 tiles
    # (interior columns, 1-based: array index + 1), tests/test_gpu_shapes.py's docstring
    if shape.W > 61:
        for a in (59, 60, 63, 116):
            assert (m[a + 1, 2:-2] != m[a + 2, 2:-2]).any(), f"no land / sea change across columns {a} / {a + 1}"


def test_coast_dropped_blocks_come_from_the_mask():
    """dropped_blocks reads the mask, not the kind's name: the paths expected of rough_drop are those of
    drop, and a kind without all-land blocks drops none."""
    assert sorted(S.dropped_blocks(S.DROPPED)) == sorted(S.dropped_blocks(S.COAST_DROPPED)) == [(1, 1), (2, 2)]
    assert S.min_block(S.COAST_DROPPED) == (12, 12) and S.expect_x2(S.COAST_DROPPED)
    assert S.expect_x4(S.COAST_DROPPED, "still", 1) and not S.expect_x4(S.COAST_DROPPED, "general", 1)
    om = S.oracle_model(S.COAST_DROPPED)
    assert {(b.bm, b.bn) for b in om.blocks} == {(bm, bn) for bm in (1, 2, 3) for bn in (1, 2, 3)} - {(1, 1), (2, 2)}
    assert S.dropped_blocks(S.Shape(13, 11, (3, 3), 0, "diag")) == []
    # the masks are functions of (W, H): the same array again, and a caller's copy
    a, b = S.mask_of(S.COAST_DROPPED), S.mask_of(S.COAST_DROPPED)
    assert a is not b and np.array_equal(a, b)


# ---------------------------------------------------------------- the rank layouts (several blocks per rank)
LAYOUTS = S.RANK_LAYOUTS + [S.EMPTY_RANK]
LAYOUT_IDS = [S.layout_id(s, n) for s, n in LAYOUTS]
# blocks per rank, in rank order
LAYOUT_COUNTS = {"17x19_b2x2-r2": [2, 2], "27x27_b3x3-r3": [3, 3, 3], "36x36_b3x3_drop-r3": [2, 2, 3],
                 "36x36_b3x3_rough_drop-r3": [2, 2, 3], "13x11_b4x2-r2": [4, 4], "13x11_b4x2-r4": [2, 2, 2, 2],
                 "23x12_b4x1-r2": [2, 2], "17x12_b3x1-r3": [1, 1, 1], "17x19_b2x2_tr1-r2": [2, 2],
                 "36x36_b3x3_tr2_rough_drop-r3": [2, 2, 3], "40x12_b4x1_east_land-r2": [2, 0]}
# the kept blocks whose x4 inner part is empty, on the layouts where x4 pairs can run at all
EMPTY_X4_INNER = {"23x12_b4x1-r2": [(2, 1), (3, 1)], "17x12_b3x1-r3": [(2, 1)]}
SIDES = {1: (5, 6), 2: (7, 8), 3: (5, 7), 4: (6, 8)}   # side -> its two diagonals (ocn_ctx.hip side_fed)


def _decomposed(shape, nranks):
    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import domain
    basin = amd.BasinConfig(mask=S.mask_of(shape), **S.basin_kwargs(shape))
    return [domain.decompose(basin, amd.ParallelConfig(*shape.grid), r, nranks) for r in range(nranks)]


def _x4_inner_empty(b):
    """ocn_ctx.hip x4_inner restated for blocks narrower than 3 x 116: the interior less 4 on each side
    fed by a neighbour (the side's own or one of its two diagonal ones)."""
    fed = {s: any(b.nbr_rank[d - 1] >= 0 for d in (s,) + SIDES[s]) for s in SIDES}
    w, h = b.nx_end - b.nx_start + 1, b.ny_end - b.ny_start + 1
    assert w < 3 * 116
    return w - 4 * (fed[1] + fed[2]) < 1 or h - 4 * (fed[3] + fed[4]) < 1


@pytest.mark.parametrize("shape,nranks", LAYOUTS, ids=LAYOUT_IDS)
def test_rank_layouts_have_what_they_promise(shape, nranks):
    lid = S.layout_id(shape, nranks)
    want = S.rank_blocks(shape, nranks)
    ranks = _decomposed(shape, nranks)
    assert [sorted((b.bm, b.bn) for b in blocks) for blocks in ranks] == want
    assert [len(w) for w in want] == LAYOUT_COUNTS[lid]
    assert sorted(sum(want, [])) == sorted(S.kept_blocks(shape))
    if (shape, nranks) != S.EMPTY_RANK and lid != "17x12_b3x1-r3":
        assert nranks < len(S.kept_blocks(shape))
    # a block with a local AND a remote neighbour: every layout with several blocks on a rank
    mixed = [(b.bm, b.bn) for r, blocks in enumerate(ranks) for b in blocks
             if any(q == r for q in b.nbr_rank) and any(q >= 0 and q != r for q in b.nbr_rank)]
    assert bool(mixed) == (max(LAYOUT_COUNTS[lid]) > 1 and (shape, nranks) != S.EMPTY_RANK), mixed
    empty = sorted((b.bm, b.bn) for blocks in ranks for b in blocks if _x4_inner_empty(b))
    if S.expect_x4(shape, "noise", 1, peers=True):
        assert empty == EMPTY_X4_INNER.get(lid, []), empty
    else:
        assert shape.W == 13 and empty   # (blocks 3 wide: no pairs at all)


def test_rank_layout_details():
    by = {S.layout_id(s, n): _decomposed(s, n) for s, n in S.RANK_LAYOUTS}
    # 17x19 over 2: N / S local, E / W and the diagonals remote (oracle.DIRS: 1 E, 2 W, 3 N, 4 S, 5 .. 8 diagonals)
    for r, blocks in enumerate(by["17x19_b2x2-r2"]):
        for b in blocks:
            have = {d: q for d, q in enumerate(b.nbr_rank, 1) if q >= 0}
            assert len(have) == 3 and all((q == r) == (d in (3, 4)) for d, q in have.items()), (b.bm, b.bn, have)
    # 27x27 over 3: the middle block has all 8 neighbours, 2 local and 6 remote
    mid = [b for b in by["27x27_b3x3-r3"][1] if (b.bm, b.bn) == (2, 2)][0]
    assert sorted(mid.nbr_rank) == [0, 0, 0, 1, 1, 2, 2, 2]
    # the dropped layouts: a hole across a rank boundary (block (1, 2) on rank 0 misses (2, 2) of rank 1)
    for lid in ("36x36_b3x3_drop-r3", "36x36_b3x3_rough_drop-r3"):
        b12 = [b for b in by[lid][0] if (b.bm, b.bn) == (1, 2)][0]
        assert b12.nbr_rank[0] == -1 and b12.nbr_rank[5 - 1] == 1 and b12.nbr_rank[6 - 1] == 1, b12.nbr_rank
    # 13x11 b4x2: x2 only, blocks 3 wide exist
    s = S.Shape(13, 11, (4, 2))
    assert S.block_sizes(s) == ([3, 3, 3, 4], [5, 6]) and S.expect_x2(s) and not S.expect_x4(s, "noise", 1, peers=True)
    assert S.block_sizes(S.Shape(23, 12, (4, 1)))[0] == [5, 6, 6, 6] and S.block_sizes(S.Shape(17, 12, (3, 1)))[0] == [5, 6, 6]
    assert S.dims_create(2) == (2, 1) and S.dims_create(3) == (3, 1) and S.dims_create(4) == (2, 2) and S.dims_create(8) == (4, 2)
    # the rank without blocks
    assert S.rank_blocks(*S.EMPTY_RANK) == [[(1, 1), (2, 1)], []]
    assert sorted(S.dropped_blocks(S.EMPTY_RANK[0])) == [(3, 1), (4, 1)]


@pytest.mark.parametrize("shape,nranks", S.RANK_LAYOUTS, ids=LAYOUT_IDS[:-1])
def test_rank_layout_inputs_are_sound(shape, nranks):
    """The classes tests/test_gpu_rank_layouts.py runs on the layouts not in the sweeps above."""
    for cls in ("noise", "general") if shape.tracers else ("noise", "hr", "general"):
        ref = S.reference(shape, cls, S.GRID_STEPS)   # raises FloatingPointError on a blow-up
        for (bm, bn), f in ref.items():
            for nm, a in f.items():
                assert np.isfinite(a).all(), f"{cls} ({bm},{bn}):{nm} not finite"
