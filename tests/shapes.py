"""Shape sweep helpers: rectangular boxes, rough halo-consistent inputs, the oracle reference and the
bitwise comparison -- shared by tests/test_shapes_cpu.py (oracle only) and tests/test_gpu_shapes.py.

A Shape is an interior W x H (BasinConfig(nx=W+4, ny=H+4)), a block grid, a tracer count and a
mask kind (None: the closed box; "drop": the centre and the (1, 1) corner block of the grid all land,
which the decomposition drops; the coast kinds of MASK_KINDS below).  The CPU oracle (oracle/oracle.py,
pinned bit for bit to the compiled reference by tests/test_oracle_pinned.py) is the reference.

A parameter set (PARAMS below: a name -> basin keywords, SW keywords, tau) moves a run off tau = 1,
time_smooth = 0.5 and the default grid; oracle_model, sw_kwargs, basin_kwargs, uploads_for and reference take
its name, and None (the default) is the run every sweep before tests/test_gpu_params.py makes.

Inputs are cut from GLOBAL (nx, ny) arrays of numpy.random.default_rng(seed).uniform(-1, 1), one
seed per field: block (bm, bn) gets [bnd_x1-1:bnd_x2, bnd_y1-1:bnd_y2], so the halos of neighbouring
blocks agree (the library's own checks keep the x2 / x4 steps off for uploads whose halos do not).
Rough, non-symmetric data: a mirrored or shifted index does not reproduce the same bits.

Classes:
  plain    nothing uploaded (the known-constant variant)
  noise    ssh += 1e-3 r on lu, ubrtr += 1e-4 r on lcu, vbrtr += 1e-4 r on lcv -- each also into the
           other buffer of its role-flip pair (sshn, ubrtrn, vbrtrn), as every state the reference
           reaches has them (init and a8 leave each pair equal); a pair that differs on a halo sea point
           is a state the library runs with standard steps (sw_stencils.h Coherence), which the older
           tests cover
  hr       hhq_rest += 5 (1 + r) where hhq_rest > 0 (the h_r-read variant)
  general  noise + hr + mu = 50 (1 + r), RHSx = 2e-7 r on lcu, RHSy = 2e-7 r on lcv
  still    still water with velocities below udiv's range (tests/test_gpu_coast.py only): ssh = sshn =
           sshp = 0, ubrtr = ubrtrn = ubrtrp = 1e-290 (1 + 0.5 r) on lcu, vbrtr likewise on lcv.  The
           state stays below 2^-900 over the sweep's runs (tests/test_shapes_cpu.py asserts it after
           every step), so every row with a wet velocity point takes BOTH IEEE re-runs of
           sw_kernels.hip MarchStep::iteration in every step of every call -- established by reading
           derive<E> and step<E>, not by a counter:
             derive<true>: its dividends up(n+1), vp(n+1), up(n+2) are the velocities themselves, nonzero
               and below 2^-900; the depth averages sh, a_u0 .. a_v1 stay normal (h_r = 100);
             step<true>: a_ssh = u hu dyh - (its left lane's) + v hv dxh - (the row before's), about
               1e-290 x 100 x 250 = 2.5e-286 < 2^-900 wherever the fluxes do not cancel exactly; uv_diff2's
               a1 .. a4 are +-0 (mu = 0: every term is mu x ...), which exp_check passes.
           The general variant cannot be kept tiny with a forcing of 2e-7, and still + hr was not needed:
           the h_r-read variant runs the same derive / step code (its template flag changes where h_r
           comes from, not a dividend), so neither combination is a class of its own.
  abyss    still, deeper: velocities of 2e-305 (1 + 0.5 r) and a uniform mu = 5e3 (still a known-constant
           variant: sw_kernels.hip FallbackCheck only asks that mu be one value, so pairs, x4 and the
           ensemble launch stay available).  Why it exists: udiv's residual fma(q, d, -x) is exact down
           to about |x| = 2^-969, far below the 2^-900 the range check uses, so at still's 1e-290 the
           fast path and the IEEE re-run give the same bits and a re-run that does nothing goes
           unnoticed (measured: a library whose derive<true> re-run never runs passed every still
           case).  At 2e-305 the quotients are still normal but the residual is a subnormal of a few
           bits: about 1 quotient in 1000 differs from IEEE division without the re-run (checked on the
           host over these magnitudes and the metrics' divisors).  mu = 5e3 (mu dt / dx^2 about 0.08:
           stable, the state stays between 1e-305 and 4e-305 over the runs) makes a5's quotients feed
           back into the velocities in EVERY step -- with mu = 0 they reach only str_t / str_s of a
           call's last step -- and puts uv_diff2's dividends a1 .. a4 (step<true>) out of range too.

Coast mask kinds (MASK_KINDS; each keeps the 2-point land frame; i, j are the 0-based interior indices):
  rough       land with probability 0.15 per interior point (default_rng, a fixed seed per W x H):
              one-point seas, one-point islands, diagonal touches
  checker     land where i + j is odd: every sea point isolated, no u, v or vorticity point wet
  diag        land where (i - j) % 7 == 0: diagonal walls across every tile edge, every h-point corner
              configuration
  comb        land where i is odd and j % 5 != 0: channels one point wide, joined every fifth row
  rough_drop  rough plus the two all-land blocks of "drop"
  east_land   the closed box with the eastern half of the block grid (bm > bnx / 2) all land (not a coast
              kind: only EMPTY_RANK below uses it)

Rank layouts (RANK_LAYOUTS: a shape over FEWER ranks than it keeps blocks, so a rank holds several
blocks and a halo plan mixes local copies with messages; rank_blocks restates the library's
block-to-rank map): tests/test_halo_plan_cpu.py (the plans, on the CPU) and tests/test_gpu_rank_layouts.py.
"""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

from tests.test_gpu_parity import bits_equal

CLASSES = ("plain", "noise", "hr", "general")
COAST_CLASSES = CLASSES + ("still", "abyss")   # still, abyss: the coastline sweep only
MASK_KINDS = ("rough", "checker", "diag", "comb", "rough_drop")
# rough's seed is 1000 W + H + ROUGH_SEED_BUMP.get((W, H), 0): bumped where the plain seed leaves a tile
# edge of tests/test_shapes_cpu.py without a land / sea change or an h-point class empty
ROUGH_SEED_BUMP = {(361, 12): 1}   # (seed 361012 has no land / sea change across columns 116 / 117)
SEEDS = {"ssh": 101, "ubrtr": 102, "vbrtr": 103, "hhq_rest": 104, "mu": 105, "RHSx": 106, "RHSy": 107}
SKIP = ("lu1", "rlh_c")   # oracle scratch, not fields of the model


class Shape(NamedTuple):
    W: int
    H: int
    grid: Tuple[int, int] = (1, 1)
    tracers: int = 0
    mask: Optional[str] = None

    @property
    def id(self):
        s = f"{self.W}x{self.H}_b{self.grid[0]}x{self.grid[1]}"
        return s + (f"_tr{self.tracers}" if self.tracers else "") + (f"_{self.mask}" if self.mask else "")


# ---------------------------------------------------------------- the sweep's shapes
SINGLE = [Shape(w, h) for w, h in [(1, 1), (2, 1), (1, 2), (3, 3), (4, 5), (5, 4), (59, 7), (60, 8), (61, 9), (61, 32),
                                   (116, 33), (117, 31), (120, 2), (121, 65), (233, 129), (241, 151), (64, 150),
                                   (120, 150), (7, 241), (1, 241), (241, 1), (180, 7)]]
DROPPED = Shape(36, 36, (3, 3), 0, "drop")
GRIDS = [Shape(7, 9, (3, 2)), Shape(10, 6, (5, 3)), Shape(5, 3, (5, 3)), Shape(13, 11, (3, 3)), Shape(9, 8, (2, 2)),
         Shape(16, 16, (2, 2)), Shape(17, 19, (2, 2)), Shape(27, 27, (3, 3)), Shape(122, 10, (2, 1)),
         Shape(361, 12, (2, 1)), Shape(358, 12, (2, 1)), Shape(700, 9, (2, 1)), Shape(12, 700, (1, 2)), DROPPED]
TRACER_GRIDS = [s._replace(tracers=t) for s in (Shape(13, 11, (3, 3)), Shape(17, 19, (2, 2)), DROPPED) for t in (1, 2)]
RANK_GRIDS = [Shape(7, 9, (3, 2)), Shape(9, 8, (2, 2)), Shape(17, 19, (2, 2))]
SINGLE_STEPS, GRID_STEPS = 8, 7   # the longest run of the sweep on a shape (calls [2, 6] / [2, 5])

# ---------------------------------------------------------------- several blocks per rank, uneven ranks
# (shape, nranks); what each reaches (tests/test_shapes_cpu.py asserts it):
#   17x19 b2x2 / 2   1 x 2 blocks per rank: N / S a local copy, E / W and the diagonals remote; blocks
#                    8-9 x 9-10, so x4 pairs run
#   27x27 b3x3 / 3   1 x 3 per rank, the middle rank with peers on both sides; block (2, 2) has all 8
#                    neighbours, 2 local and 6 remote
#   36x36 b3x3 drop, rough_drop / 3   ranks hold 2, 2 and 3 blocks: neighbour tables with holes across a
#                    rank boundary
#   13x11 b4x2 / 2, 4   2 x 2 and 2 x 1 blocks per rank; blocks 3-4 x 5-6: x2 only, and h_r's copy goes 4
#                    deep between blocks 3 wide
#   23x12 b4x1 / 2   widths 5, 6, 6, 6: blocks (2, 1) and (3, 1) are fed from both sides and 6 wide, so
#                    their x4 inner part is empty -- on BOTH ranks
#   17x12 b3x1 / 3   one block per rank (the one layout here with as many ranks as blocks), widths 5, 6,
#                    6: the x4 inner part is empty on rank 1 only -- ranks that differ in what their own
#                    blocks allow
#   17x19 b2x2 tr1 / 2, 36x36 b3x3 tr2 rough_drop / 3   tracer runs: with peers, x4 auto runs pairs with
#                    tracer steps; the co-launch covers a rank's several blocks
RANK_LAYOUTS = [(Shape(17, 19, (2, 2)), 2), (Shape(27, 27, (3, 3)), 3), (DROPPED, 3),
                (Shape(36, 36, (3, 3), 0, "rough_drop"), 3), (Shape(13, 11, (4, 2)), 2), (Shape(13, 11, (4, 2)), 4),
                (Shape(23, 12, (4, 1)), 2), (Shape(17, 12, (3, 1)), 3), (Shape(17, 19, (2, 2), 1), 2),
                (Shape(36, 36, (3, 3), 2, "rough_drop"), 3)]
# blocks (3, 1) and (4, 1) all land: over 2 ranks rank 1 owns no block (the reference allows it)
EMPTY_RANK = (Shape(40, 12, (4, 1), 0, "east_land"), 2)


def layout_id(shape, nranks):
    return f"{shape.id}-r{nranks}"

# ---------------------------------------------------------------- the coastline sweep's shapes
# (tests/test_gpu_coast.py; the smallest shapes of the sweep above at which each tile edge exists)
COAST_SINGLE = [Shape(w, h, mask=k) for w, h in [(5, 4), (61, 9), (61, 33), (117, 31), (121, 65), (233, 129)]
                for k in ("rough", "checker", "diag", "comb")]
COAST_DROPPED = Shape(36, 36, (3, 3), 0, "rough_drop")
COAST_GRIDS = [Shape(w, h, g, 0, k) for w, h, g in [(13, 11, (3, 3)), (17, 19, (2, 2)), (27, 27, (3, 3)),
                                                    (122, 10, (2, 1)), (361, 12, (2, 1))]
               for k in ("rough", "diag")] + [COAST_DROPPED]
COAST_TRACER_GRIDS = [s._replace(tracers=t) for s in (Shape(17, 19, (2, 2), 0, "rough"), COAST_DROPPED) for t in (1, 2)]
COAST_RANK_GRIDS = [Shape(9, 8, (2, 2), 0, "rough"), Shape(17, 19, (2, 2), 0, "rough")]
COAST_ENSEMBLES = [Shape(w, h, mask=k) for w, h in [(61, 9), (121, 65)] for k in ("rough", "comb")]
COAST_ENSEMBLE_CLASSES = ["plain", "noise", "still", "hr", "general", "noise"]
COAST_FLAG_SHAPES = [Shape(61, 33, mask="rough"), Shape(17, 19, (2, 2), 1, "rough")]
FLAG_SETTINGS = [(a, b, c) for a in (1, 0) for b in (1, 0) for c in (1, 0)]   # (full_free_surface, trans_terms, ksw_lat)
STILL_SHAPES = [(61, 33), (121, 65), (17, 19), (36, 36)]   # W x H of the shapes that also run still and abyss
COAST_ENSEMBLE_DEEP = ["abyss", "noise", "abyss"]   # a second ensemble: one known-constant group


# ---------------------------------------------------------------- the parameter sweep
# (tests/test_gpu_params.py; tests/test_params_cpu.py asserts what each set promises)
# name -> (BasinConfig keywords, SWConfig keywords, tau).  What each reaches in sw_kernels.hip:
#   tau03, tau075_ts03  tau is no power of two: MarchStep<P2 = false>, qtau = a / tau, an IEEE division;
#                       time_smooth 0.3: filter weights whose products round
#   tau2, tau025_ts0    a power of two other than 1: P2 = true with inv_tau != 1 (at tau = 1, a * inv_tau,
#                       a * tau and a are the same bits); the filter off
#   tau3_ts1            the filter at full weight
#   cart                curve_grid 0: no cos(lat) scaling, one Coriolis value
#   south, equator      rlh_s negative / of both signs in one block and across a block boundary
#   coarse              half-degree steps from 30 N: adjacent rows' dx, dxh, dxt, dxb differ by percents,
#                       so a lane that takes row n +- 1's metric or reciprocal changes high bits -- on the
#                       ext rows x2 / x4 steps form for their halo as well; tau 30 keeps the Courant number
#   polar               80 N: dx about 43 m, large reciprocals
#   rot                 a rotated sphere: rlh_s varies along a row, the compact tables must be refused
EQUATOR = object()   # basin_kwargs: the rlat that puts the interior's middle row at latitude 0
PARAMS = {
    "tau03": ({}, {}, 0.3),
    "tau075_ts03": ({}, dict(time_smooth=0.3), 0.75),
    "tau2": ({}, {}, 2.0),
    "tau025_ts0": ({}, dict(time_smooth=0.0), 0.25),
    "tau3_ts1": ({}, dict(time_smooth=1.0), 3.0),
    "cart": (dict(curve_grid=0), {}, 0.75),
    "south": (dict(rlat=-44.8), {}, 0.75),
    "equator": (dict(rlat=EQUATOR), {}, 0.75),
    "coarse": (dict(dxst=0.5, dyst=0.4, rlat=30.0), {}, 30.0),
    "polar": (dict(rlat=80.0), {}, 0.3),
    "rot": (dict(rotation_on_lon=10.0, rotation_on_lat=20.0), {}, 0.75),
}
CORE_PARAMS = ["tau03", "tau075_ts03", "tau2", "coarse", "equator"]
OTHER_PARAMS = ["tau025_ts0", "tau3_ts1", "cart", "south", "polar"]
PARAM_SINGLE = [Shape(121, 65, mask="rough"), Shape(61, 9, mask="comb")]
PARAM_GRIDS = [Shape(17, 19, (2, 2), 0, "rough"), Shape(27, 27, (3, 3), 0, "rough"), Shape(361, 12, (2, 1), 0, "diag")]
PARAM_TRACER_GRIDS = [Shape(17, 19, (2, 2), 1, "rough"), Shape(36, 36, (3, 3), 2, "rough_drop")]
PARAM_RANK_GRIDS = [Shape(9, 8, (2, 2), 0, "rough"), Shape(17, 19, (2, 2), 0, "rough")]
PARAM_ENSEMBLE = Shape(61, 9, mask="rough")
PARAM_ROT = [Shape(61, 33, mask="rough"), Shape(17, 19, (2, 2), 1, "rough")]
PARAM_DEEP = ["tau03", "tau075_ts03"]   # abyss: the IEEE re-runs and a / tau in one row
# tau changes across the P2 / non-P2 variant boundary: (steps, tau) per call
TAU_CALLS = ((3, 1.0), (2, 0.3), (1, 0.3), (3, 2.0), (2, 0.75))


def coast_classes(shape):
    """The input classes the coastline sweep runs on a shape: noise and general on one block, noise, hr
    and general on a grid, and still and abyss on STILL_SHAPES."""
    base = ("noise", "general") if shape.grid == (1, 1) else ("noise", "hr", "general")
    return base + (("still", "abyss") if (shape.W, shape.H) in STILL_SHAPES else ())


def block_sizes(shape):
    """(widths, heights) of the grid's blocks (decomposition.f90:448-482)."""
    from oracle.oracle import uniform_sizes
    return uniform_sizes(shape.W, shape.grid[0]), uniform_sizes(shape.H, shape.grid[1])


def _frame(shape):
    m = np.zeros((shape.W + 4, shape.H + 4), dtype=np.int32, order="F")
    m[:2, :] = 1; m[-2:, :] = 1; m[:, :2] = 1; m[:, -2:] = 1
    return m


def _block_origin(shape, bm, bn):
    xs, ys = block_sizes(shape)
    return 2 + sum(xs[:bm - 1]), 2 + sum(ys[:bn - 1]), xs[bm - 1], ys[bn - 1]


@functools.lru_cache(maxsize=None)
def _mask(shape):
    W, H = shape.W, shape.H
    m = _frame(shape)
    i, j = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    kind = shape.mask
    if kind in ("rough", "rough_drop"):
        seed = 1000 * W + H + ROUGH_SEED_BUMP.get((W, H), 0)
        land = np.random.default_rng(seed).random((W, H)) < 0.15
    elif kind == "checker":
        land = (i + j) % 2 == 1
    elif kind == "diag":
        land = (i - j) % 7 == 0
    elif kind == "comb":
        land = (i % 2 == 1) & (j % 5 != 0)
    else:
        assert kind in ("drop", "east_land"), kind
        land = np.zeros((W, H), dtype=bool)
    m[2:-2, 2:-2] = land
    if kind == "east_land":
        for bm in range(shape.grid[0] // 2 + 1, shape.grid[0] + 1):
            for bn in range(1, shape.grid[1] + 1):
                x0, y0, w, h = _block_origin(shape, bm, bn)
                m[x0:x0 + w, y0:y0 + h] = 1
    if kind in ("drop", "rough_drop"):
        for bm, bn in [((shape.grid[0] + 1) // 2, (shape.grid[1] + 1) // 2), (1, 1)]:
            x0, y0, w, h = _block_origin(shape, bm, bn)
            m[x0:x0 + w, y0:y0 + h] = 1
    m.setflags(write=False)
    return m


def mask_of(shape):
    """None (the box), or the int32 (W + 4, H + 4) mask of the shape's kind (1 = land)."""
    return None if shape.mask is None else _mask(shape).copy(order="F")


def dropped_blocks(shape):
    """The blocks the decomposition drops: those whose interior is all land in the mask itself."""
    if shape.mask is None:
        return []
    m, out = _mask(shape), []
    for bm in range(1, shape.grid[0] + 1):
        for bn in range(1, shape.grid[1] + 1):
            x0, y0, w, h = _block_origin(shape, bm, bn)
            if m[x0:x0 + w, y0:y0 + h].all():
                out.append((bm, bn))
    return out


def kept_blocks(shape):
    """(bm, bn) of the blocks the decomposition keeps, in global (column-major) order."""
    drop = set(dropped_blocks(shape))
    return [(bm, bn) for bn in range(1, shape.grid[1] + 1) for bm in range(1, shape.grid[0] + 1) if (bm, bn) not in drop]


def dims_create(n):
    """MPI_Dims_create(n, 2) as ctx_setup.hip dims_create restates it: balanced, non-increasing factors."""
    f = int(np.floor(np.sqrt(n)))
    while n % f:
        f -= 1
    return n // f, f


def rank_blocks(shape, nranks):
    """The library's block-to-rank map (ctx_setup.hip decompose after the reference's
    create_uniform_decomposition): per rank the sorted (bm, bn) of its blocks -- the process grid
    p1 x p2 = MPI_Dims_create(nranks), a rank's patch bnx / p1 x bny / p2 blocks, rank = c1 p2 + c2 of the
    patch coordinates, dropped blocks left out (a rank may be left with none)."""
    p1, p2 = dims_create(nranks)
    bnx, bny = shape.grid
    assert bnx % p1 == 0 and bny % p2 == 0, (shape.grid, nranks)
    lbx, lby = bnx // p1, bny // p2
    out = [[] for _ in range(nranks)]
    for bm, bn in kept_blocks(shape):
        out[((bm - 1) // lbx) * p2 + (bn - 1) // lby].append((bm, bn))
    return [sorted(b) for b in out]


def min_block(shape):
    """Smallest block width and height over the blocks the decomposition keeps."""
    xs, ys = block_sizes(shape)
    drop = set(dropped_blocks(shape))
    kept = [(bm, bn) for bm in range(1, shape.grid[0] + 1) for bn in range(1, shape.grid[1] + 1) if (bm, bn) not in drop]
    return min(xs[bm - 1] for bm, _ in kept), min(ys[bn - 1] for _, bn in kept)


def expect_x2(shape):
    """ocn_ctx.hip x2_local: halo exchanges, every block at least 2 x 2."""
    return shape.grid != (1, 1) and min(min_block(shape)) >= 2


def expect_x4(shape, cls, x4, peers=False):
    """ocn_ctx.hip x4_local / x4_now: the option, every block at least 4 x 4, tracer runs only with
    OCN_OPT_X4 3 or peers on other ranks, and a known-constant variant (the x4 pairs have no general
    one: mu and the forcing uploaded -> single x2 steps of the general variant)."""
    return bool(x4) and expect_x2(shape) and min(min_block(shape)) >= 4 and cls != "general" and \
        (shape.tracers == 0 or x4 == 3 or peers)


# ---------------------------------------------------------------- oracle twin, inputs, reference
def sw_kwargs(shape, flags=(1, 1, 1), params=None):
    """SWConfig's keywords (the oracle's and the library's alike) for the shape's tracers, the
    (full_free_surface, trans_terms, ksw_lat) setting and the parameter set (a name of PARAMS)."""
    kw = dict(use_tracers=1, tracer_num=shape.tracers) if shape.tracers else {}
    if tuple(flags) != (1, 1, 1):
        kw.update(full_free_surface=flags[0], trans_terms=flags[1], ksw_lat=flags[2])
    if params is not None:
        kw.update(PARAMS[params][1])
    return kw


def basin_kwargs(shape, params=None):
    """BasinConfig's keywords (the oracle's and the library's alike) but the mask: the shape's nx, ny and
    the parameter set's grid.  EQUATOR stands for the rlat at which the interior's middle row (0-based
    interior row (H - 1) // 2) lies at latitude 0: yt = rlat + j dyst is then -(j dyst) + j dyst = 0."""
    kw = dict(nx=shape.W + 4, ny=shape.H + 4)
    if params is not None:
        kw.update(PARAMS[params][0])
        if kw.get("rlat") is EQUATOR:
            from oracle import oracle as O
            kw["rlat"] = -(((shape.H - 1) // 2) * kw.get("dyst", O.BasinConfig(nx=5, ny=5).dyst))
    return kw


def tau_of(params=None):
    return 1.0 if params is None else PARAMS[params][2]


def oracle_model(shape, flags=(1, 1, 1), params=None):
    """An initialised oracle.OracleModel on the shape's box, block grid and tracer count, with the
    parameter set's grid and SW keywords."""
    from oracle import oracle as O
    sw = O.SWConfig(**sw_kwargs(shape, flags, params))
    return O.OracleModel(O.BasinConfig(mask=mask_of(shape), **basin_kwargs(shape, params)), sw, *shape.grid).init()


def uploads(cls, om):
    """{(bm, bn): {field: array}} for input class cls, from the initial state of oracle model om."""
    assert cls in COAST_CLASSES, cls
    if cls == "plain":
        return {}
    nx, ny = om.basin.nx, om.basin.ny
    g = {nm: np.random.default_rng(seed).uniform(-1.0, 1.0, (nx, ny)) for nm, seed in SEEDS.items()}
    out = {}
    for k, b in enumerate(om.blocks):
        f = om.f[k]

        def cut(nm):
            return g[nm][b.bx1 - 1:b.bx2, b.by1 - 1:b.by2]

        u = {}
        if cls in ("noise", "general"):
            for nm, other, amp, msk in (("ssh", "sshn", 1.0e-3, "lu"), ("ubrtr", "ubrtrn", 1.0e-4, "lcu"),
                                        ("vbrtr", "vbrtrn", 1.0e-4, "lcv")):
                a = f[nm].copy(order="F")
                sel = f[msk] > 0.5
                a[sel] += amp * cut(nm)[sel]
                u[nm] = a
                u[other] = a.copy(order="F")
        if cls in ("still", "abyss"):
            for nm in ("ssh", "sshn", "sshp"):
                u[nm] = np.zeros_like(f[nm], order="F")
            for nm, msk in (("ubrtr", "lcu"), ("vbrtr", "lcv")):
                a = np.zeros_like(f[nm], order="F")
                sel = f[msk] > 0.5
                a[sel] = (1.0e-290 if cls == "still" else 2.0e-305) * (1.0 + 0.5 * cut(nm)[sel])
                for role in (nm, nm + "n", nm + "p"):
                    u[role] = a.copy(order="F")
        if cls == "abyss":
            u["mu"] = np.full_like(f["mu"], 5.0e3, order="F")
        if cls in ("hr", "general"):
            a = f["hhq_rest"].copy(order="F")
            sel = a > 0.0
            a[sel] += 5.0 * (1.0 + cut("hhq_rest"))[sel]
            u["hhq_rest"] = a
        if cls == "general":
            u["mu"] = np.asfortranarray(50.0 * (1.0 + cut("mu")))
            for nm, msk in (("RHSx", "lcu"), ("RHSy", "lcv")):
                a = f[nm].copy(order="F")
                sel = f[msk] > 0.5
                a[sel] = 2.0e-7 * cut(nm)[sel]
                u[nm] = a
        out[(b.bm, b.bn)] = u
    return out


@functools.lru_cache(maxsize=16)
def uploads_for(shape, cls, params=None):
    return uploads(cls, oracle_model(shape, params=params))


def loaded_oracle(shape, cls, flags=(1, 1, 1), params=None):
    """oracle_model with the class's uploads written into its fields."""
    om = oracle_model(shape, flags, params)
    for k, b in enumerate(om.blocks):
        for nm, a in uploads_for(shape, cls, params).get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    return om


@functools.lru_cache(maxsize=16)
def reference(shape, cls, steps, flags=(1, 1, 1), params=None):
    """{(bm, bn): {field: array}} of the oracle after `steps` steps from the class's inputs, at tau = 1
    or, with a parameter set, at its tau, grid and SW keywords.  Computed once per (shape, class, steps,
    flags, params) and shared; callers must not write into it."""
    om = loaded_oracle(shape, cls, flags, params)
    om.run(steps, tau_of(params))
    return {(b.bm, b.bn): om.f[k] for k, b in enumerate(om.blocks)}


@functools.lru_cache(maxsize=8)
def reference_calls(shape, cls, calls):
    """The oracle driven through calls = ((steps, tau), ...) from the class's inputs: a list, per call, of
    {(bm, bn): {field: array}} -- ssh alone after every call but the last, every field after the last.
    Shared; callers must not write into it."""
    om = loaded_oracle(shape, cls)
    out = []
    for i, (n, tau) in enumerate(calls):
        om.run(n, tau)
        last = i == len(calls) - 1
        out.append({(b.bm, b.bn): (om.f[k] if last else {"ssh": om.f[k]["ssh"].copy(order="F")})
                    for k, b in enumerate(om.blocks)})
    return out


# ---------------------------------------------------------------- comparison
def mismatches(ref, get):
    """Every field of every block of `ref` ({(bm, bn): {field: array}}) against get(bm, bn, field),
    bitwise (no tolerance; lu1 and rlh_c skipped): the list of "(bm,bn):field" that differ."""
    bad = []
    for (bm, bn), f in ref.items():
        for nm, a in f.items():
            if nm in SKIP:
                continue
            if not bits_equal(get(bm, bn, nm), a):
                bad.append(f"({bm},{bn}):{nm}")
    return bad


def model_getter(models):
    """get(bm, bn, field) over the blocks of one GPU model or of several (loopback ranks)."""
    where = {(b.bm, b.bn): (m, b.k) for m in models for b in m.blocks}

    def get(bm, bn, nm):
        m, k = where[(bm, bn)]
        return m.download(k, nm)

    get.blocks = set(where)
    return get
