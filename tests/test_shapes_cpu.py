"""The shape sweep's inputs are sound and its comparison has teeth (no GPU: the oracle alone).

For every shape x input class of tests/test_gpu_shapes.py the oracle must run the sweep's longest
call sequence without a FloatingPointError (check_ssh_err), keep every field finite and |ssh| < 1,
and end with a nonzero ubrtr at every interior lcu point of every block -- rough data that moved
everywhere, so a wrong column or row in a kernel cannot reproduce the reference's bits by symmetry
or by leaving zeros.  The comparison helper must name exactly the block and field of a one-ulp change.

The same for the coastline sweep (tests/test_gpu_coast.py): every (shape, mask, class) it runs is finite
and trips no check_ssh_err; the still class stays below udiv's range after every step; every mask kind
has what it promises (tests/shapes.py MASK_KINDS) and a land / sea change across the tiles' column edges.
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
