"""Shape sweep helpers: rectangular boxes, rough halo-consistent inputs, the oracle reference and the
bitwise comparison -- shared by tests/test_shapes_cpu.py (oracle only) and tests/test_gpu_shapes.py.

A Shape is an interior W x H (BasinConfig(nx=W+4, ny=H+4)), a block grid, a tracer count and a
mask kind (None: the closed box; "drop": the centre and the (1, 1) corner block of the grid all land,
which the decomposition drops).  The CPU oracle (oracle/oracle.py, pinned bit for bit to the compiled
reference by tests/test_oracle_pinned.py) is the reference.

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
"""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

from tests.test_gpu_parity import bits_equal

CLASSES = ("plain", "noise", "hr", "general")
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


def block_sizes(shape):
    """(widths, heights) of the grid's blocks (decomposition.f90:448-482)."""
    from oracle.oracle import uniform_sizes
    return uniform_sizes(shape.W, shape.grid[0]), uniform_sizes(shape.H, shape.grid[1])


def dropped_blocks(shape):
    return [] if shape.mask != "drop" else [((shape.grid[0] + 1) // 2, (shape.grid[1] + 1) // 2), (1, 1)]


def mask_of(shape):
    """None (the box), or the box with the dropped blocks' interiors all land."""
    if shape.mask is None:
        return None
    assert shape.mask == "drop", shape.mask
    m = np.zeros((shape.W + 4, shape.H + 4), dtype=np.int32, order="F")
    m[:2, :] = 1; m[-2:, :] = 1; m[:, :2] = 1; m[:, -2:] = 1
    xs, ys = block_sizes(shape)
    for bm, bn in dropped_blocks(shape):
        x0, y0 = 2 + sum(xs[:bm - 1]), 2 + sum(ys[:bn - 1])
        m[x0:x0 + xs[bm - 1], y0:y0 + ys[bn - 1]] = 1
    return m


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
def oracle_model(shape):
    """An initialised oracle.OracleModel on the shape's box, block grid and tracer count."""
    from oracle import oracle as O
    sw = O.SWConfig(use_tracers=1, tracer_num=shape.tracers) if shape.tracers else O.SWConfig()
    return O.OracleModel(O.BasinConfig(nx=shape.W + 4, ny=shape.H + 4, mask=mask_of(shape)), sw, *shape.grid).init()


def uploads(cls, om):
    """{(bm, bn): {field: array}} for input class cls, from the initial state of oracle model om."""
    assert cls in CLASSES, cls
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


@functools.lru_cache(maxsize=8)
def uploads_for(shape, cls):
    return uploads(cls, oracle_model(shape))


@functools.lru_cache(maxsize=8)
def reference(shape, cls, steps):
    """{(bm, bn): {field: array}} of the oracle after `steps` steps (tau = 1) from the class's inputs.
    Computed once per (shape, class, steps) and shared; callers must not write into it."""
    om = oracle_model(shape)
    for k, b in enumerate(om.blocks):
        for nm, a in uploads_for(shape, cls).get((b.bm, b.bn), {}).items():
            om.f[k][nm][...] = a
    om.run(steps)
    return {(b.bm, b.bn): om.f[k] for k, b in enumerate(om.blocks)}


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
