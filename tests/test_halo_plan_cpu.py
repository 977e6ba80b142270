"""The halo plans of the x2 steps (2 deep) and the x4 pairs (4 deep) on the CPU, every rank simulated in
numpy (no gloo, no GPU): ctx_comm.hip plan_entries / halo_layer / field_depth through the host-only
ocn_halo_schedule_deep, on layouts where a rank holds several blocks (tests/shapes.py RANK_LAYOUTS: a
plan mixes local copies with messages), on the same shapes with one block per rank, and on the layout
that leaves a rank without blocks.

The reference's known-answer test (shared/mpp/syncborder_block2D_gen_test.fi, as
tests/test_distributed_cpu.py runs it one point deep over gloo): every block's interior holds
kat(field, m, n) of the global (m, n), everything else NaN -- the arrays carry a margin of 4 around the
interior, so the rings beyond bnd_* exist, as they do on the device (ocn_ctx.h kXRing).  After every
rank's schedule has run (SEND packs into a per-peer buffer, RECV unpacks from the sender's buffer at the
same offset, LOCAL copies) a halo point holds kat of its own global coordinates exactly when it lies
within the field's depth of the interior and the block of its direction class (a side, or a corner) is
kept; every other point is still NaN.  A state field and a tracer field share one schedule: the tracer
goes 1 deep, 2 deep in a 4-deep exchange (field_depth).

Left out: (13, 11, (4, 2)) at depth 4.  Its blocks are 3 points wide, so a 4-deep strip reads the
source block's own halo, which this simulation leaves NaN (on the device only h_r's copy is exchanged
so, ocn_ctx.hip refresh_hrx; the x4 pairs need blocks of 4 x 4).  NARROW below is computed from the block
sizes and asserted to be exactly that.
"""
import numpy as np
import pytest

import ocean_model_arch_amd as amd
from ocean_model_arch_amd import domain
from tests import shapes as S
from tests.test_distributed_cpu import DIRS, kat

FIELDS = ["ssh", "ff1_1"]   # a state field and a tracer field in one schedule
MARGIN = 4
DEPTHS = (1, 2, 4)


def _one_block_per_rank(shape):
    n = shape.grid[0] * shape.grid[1]
    p1, p2 = S.dims_create(n)
    return n if shape.grid[0] % p1 == 0 and shape.grid[1] % p2 == 0 else None


_SHAPES = list(dict.fromkeys(s._replace(tracers=0) for s, _ in S.RANK_LAYOUTS + [S.EMPTY_RANK]))
LAYOUTS = list(dict.fromkeys([(s._replace(tracers=0), n) for s, n in S.RANK_LAYOUTS + [S.EMPTY_RANK]] +
                             [(s, _one_block_per_rank(s)) for s in _SHAPES if _one_block_per_rank(s)]))
NARROW = [(S.layout_id(s, n), d) for s, n in LAYOUTS for d in DEPTHS if min(S.min_block(s)) < d]
CASES = [(s, n, d) for s, n in LAYOUTS for d in DEPTHS if (S.layout_id(s, n), d) not in NARROW]


def field_depth(name, depth):
    """ctx_comm.hip field_depth: what the step machine exchanges of each field."""
    return depth if name == "ssh" else (2 if depth >= 4 else 1)


def test_cases_cover_the_layouts():
    assert sorted(NARROW) == [("13x11_b4x2-r2", 4), ("13x11_b4x2-r4", 4), ("13x11_b4x2-r8", 4)]
    ids = {S.layout_id(s, n) for s, n in LAYOUTS}
    assert {"17x19_b2x2-r2", "17x19_b2x2-r4", "27x27_b3x3-r3", "27x27_b3x3-r9", "36x36_b3x3_drop-r3",
            "36x36_b3x3_rough_drop-r9", "13x11_b4x2-r4", "23x12_b4x1-r2", "17x12_b3x1-r3",
            "40x12_b4x1_east_land-r2"} <= ids, ids
    assert len(CASES) == 3 * len(LAYOUTS) - 3


class Arr:
    """One field of one block with a margin of MARGIN points around the interior, addressed by global (m, n)."""

    def __init__(self, b, fi):
        self.x0, self.y0 = b.nx_start - MARGIN, b.ny_start - MARGIN
        self.a = np.full((b.nx_end - b.nx_start + 1 + 2 * MARGIN, b.ny_end - b.ny_start + 1 + 2 * MARGIN), np.nan)
        for m in range(b.nx_start, b.nx_end + 1):
            for n in range(b.ny_start, b.ny_end + 1):
                self.a[m - self.x0, n - self.y0] = kat(fi, m, n)

    def index(self, rect):
        x0, x1, y0, y1 = rect
        assert x0 <= x1 and y0 <= y1, rect
        assert x0 >= self.x0 and y0 >= self.y0 and x1 - self.x0 < self.a.shape[0] and y1 - self.y0 < self.a.shape[1], rect
        mm, nn = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), indexing="ij")
        return (mm.T.ravel() - self.x0, nn.T.ravel() - self.y0)   # column-major walk (m fastest)


def _exchange(shape, nranks, depth):
    basin = amd.BasinConfig(mask=S.mask_of(shape), **S.basin_kwargs(shape))
    par = amd.ParallelConfig(*shape.grid)
    blocks = [domain.decompose(basin, par, r, nranks) for r in range(nranks)]
    sched = [domain.halo_schedule(basin, par, FIELDS, r, nranks, depth=depth) for r in range(nranks)]
    arrs = [[{f: Arr(b, fi) for fi, f in enumerate(FIELDS)} for b in blocks[r]] for r in range(nranks)]
    size = {}
    for r in range(nranks):
        for e in sched[r]:
            if e["kind"] == amd._lib.HALO_SEND:
                size[(r, e["peer"])] = max(size.get((r, e["peer"]), 0), e["offset"] + e["count"])
    buf = {key: np.full(n, np.nan) for key, n in size.items()}
    for r in range(nranks):
        for e in sched[r]:
            if e["kind"] == amd._lib.HALO_SEND:
                a = arrs[r][e["k_src"]][e["field"]]
                ii = a.index(e["src"])
                assert len(ii[0]) == e["count"], e
                buf[(r, e["peer"])][e["offset"]:e["offset"] + e["count"]] = a.a[ii]
    for r in range(nranks):
        # (the local copies read boundary strips inside the source's interior, which nothing writes: any order)
        for e in sched[r]:
            if e["kind"] == amd._lib.HALO_SEND:
                continue
            d = arrs[r][e["k"]][e["field"]]
            ii = d.index(e["dst"])
            assert len(ii[0]) == e["count"], e
            if e["kind"] == amd._lib.HALO_RECV:
                d.a[ii] = buf[(e["peer"], r)][e["offset"]:e["offset"] + e["count"]]
            else:
                s = arrs[r][e["k_src"]][e["field"]]
                jj = s.index(e["src"])
                assert len(jj[0]) == e["count"], e
                d.a[ii] = s.a[jj]
    return blocks, sched, arrs


@pytest.mark.parametrize("shape,nranks,depth", CASES, ids=[f"{S.layout_id(s, n)}-d{d}" for s, n, d in CASES])
def test_deep_halo_plans_deliver_the_known_answer(shape, nranks, depth):
    blocks, sched, arrs = _exchange(shape, nranks, depth)
    assert [sorted((b.bm, b.bn) for b in bl) for bl in blocks] == S.rank_blocks(shape, nranks)
    # every message has its other end, at the same offset with the same length and field
    sends = sorted((r, e["peer"], e["offset"], e["count"], e["field"]) for r in range(nranks) for e in sched[r]
                   if e["kind"] == amd._lib.HALO_SEND)
    recvs = sorted((e["peer"], r, e["offset"], e["count"], e["field"]) for r in range(nranks) for e in sched[r]
                   if e["kind"] == amd._lib.HALO_RECV)
    assert sends == recvs
    assert len({(s[0], s[1], s[2]) for s in sends}) == len(sends)   # no two strips at one offset of a message
    for r in range(nranks):
        for e in sched[r]:
            assert e["peer"] != r or e["kind"] == amd._lib.HALO_LOCAL, e
            if e["kind"] == amd._lib.HALO_LOCAL:   # only this rank's blocks
                assert e["peer"] == r and 0 <= e["k"] < len(blocks[r]) and 0 <= e["k_src"] < len(blocks[r]), e
            if e["kind"] == amd._lib.HALO_RECV:
                assert 0 <= e["k"] < len(blocks[r]) and e["k_src"] == -1, e
            if e["kind"] == amd._lib.HALO_SEND:
                assert 0 <= e["k_src"] < len(blocks[r]) and e["k"] == -1, e
        if not blocks[r]:
            assert sched[r] == []   # a rank without blocks neither sends nor receives
    if nranks < len(S.kept_blocks(shape)) and (shape, nranks) != S.EMPTY_RANK:
        kinds = {e["kind"] for r in range(nranks) for e in sched[r]}
        assert kinds == {amd._lib.HALO_LOCAL, amd._lib.HALO_SEND, amd._lib.HALO_RECV}
    # the known answer, point by point over the margin
    cls_dir = {v: k for k, v in DIRS.items()}
    bad = []
    for r in range(nranks):
        for b, d in zip(blocks[r], arrs[r]):
            for fi, f in enumerate(FIELDS):
                fd = field_depth(f, depth)
                a = d[f]
                for m in range(b.nx_start - MARGIN, b.nx_end + MARGIN + 1):
                    for n in range(b.ny_start - MARGIN, b.ny_end + MARGIN + 1):
                        dm = 1 if m > b.nx_end else -1 if m < b.nx_start else 0
                        dn = 1 if n > b.ny_end else -1 if n < b.ny_start else 0
                        v = a.a[m - a.x0, n - a.y0]
                        if not dm and not dn:
                            want = kat(fi, m, n)   # the interior: untouched
                        else:
                            out_x = m - b.nx_end if dm > 0 else b.nx_start - m if dm < 0 else 0
                            out_y = n - b.ny_end if dn > 0 else b.ny_start - n if dn < 0 else 0
                            fed = b.nbr_rank[cls_dir[(dm, dn)] - 1] >= 0
                            want = kat(fi, m, n) if fed and max(out_x, out_y) <= fd else None
                        if (want is None and not np.isnan(v)) or (want is not None and v != want):
                            bad.append((r, (b.bm, b.bn), f, m, n, v, want))
    assert not bad, f"{len(bad)} points, the first: {bad[:5]}"


def test_deep_schedule_arguments():
    basin, par = amd.box_config(16), amd.ParallelConfig(2, 2)
    one = domain.halo_schedule(basin, par, FIELDS, 0, 2)
    assert one == domain.halo_schedule(basin, par, FIELDS, 0, 2, depth=1)
    for depth in (0, 3, 5, -1):
        with pytest.raises(amd.OcnError):
            domain.halo_schedule(basin, par, FIELDS, 0, 2, depth=depth)
    # deeper plans carry more: 2 / 4 layers of the state, 1 / 2 of the tracer
    n = {d: sum(e["count"] for e in domain.halo_schedule(basin, par, ["ssh"], 0, 2, depth=d)) for d in DEPTHS}
    t = {d: sum(e["count"] for e in domain.halo_schedule(basin, par, ["ff1_1"], 0, 2, depth=d)) for d in DEPTHS}
    assert n[1] < n[2] < n[4] and t[1] == t[2] < t[4] and t[4] == n[2]
