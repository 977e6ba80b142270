"""Sparse linear observation operators in numpy (include/ocn_sw.h ocn_ens_sample_h, ocn_ens_assimilate_h):
the CSR table the library takes, the contract's validation, the ordered sum the device forms restated on
downloaded arrays, and the builders a user starts from -- grid points, bilinear interpolation, linear
combinations of operators (a radial velocity cos(theta) u + sin(theta) v).

    H_j(u) = s:   s = x_0 * w_0;   then, in the caller's term order,   p = x_t * w_t;  s = s + p

numpy's elementwise multiply and add are single IEEE double operations per element and nothing here is fused,
so `apply` gives the device's bits; tests/ens_obs_ref.py hands it to the tests, which check it against a
scalar loop.  Pure numpy: no device, no library.
"""
from __future__ import annotations

import numpy as np

MAX_TERMS = 16        # OCN_ENS_OBS_MAX_TERMS: terms of one observation
MAX_FIELDS = 4        # OCN_ENS_OBS_MAX_FIELDS: distinct fields among the terms of one operator


def _integers(what, a, shape_tail=()):
    a = np.asarray(a)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError(f"ObsOperator: {what} of dtype {a.dtype}, not integers")
    a = a.astype(np.int64).reshape((-1,) + shape_tail)
    if a.size and (np.abs(a) >= 2 ** 31).any():
        raise ValueError(f"ObsOperator: {what} beyond 32 bits")
    return a


class ObsOperator:
    """A sparse linear observation operator over nobs observations: observation j owns the terms
    start[j] .. start[j+1]-1 (1 .. MAX_TERMS of them), term t is the value of real(8) field tname[t] at the
    library's 1-based global indices (ti[t], tj[t]) times the weight tw[t] (float64, finite, not +-0.0); at
    most MAX_FIELDS distinct fields.  anchors[j] = (io, jo) is observation j's localization centre in index
    space, an integer point of the basin that is not tied to the terms.

    The constructor does the contract's validation that needs no basin (TypeError for a wrong dtype,
    ValueError otherwise); whether a field is real(8), a point lies in a local block's array and an anchor
    within the basin is the library's to say.  `names`: the distinct fields in the order of their first term."""

    def __init__(self, start, tname, ti, tj, tw, anchors):
        self.start = _integers("start", start)
        self.tname = tuple(tname)
        self.ti, self.tj = _integers("ti", ti), _integers("tj", tj)
        w = np.asarray(tw)
        if w.dtype != np.float64:
            raise TypeError(f"ObsOperator: weights of dtype {w.dtype}, not float64")
        self.tw = np.array(w, dtype=np.float64).ravel()
        self.anchors = _integers("anchors", anchors, (2,))
        if any(not isinstance(nm, str) for nm in self.tname):
            raise TypeError("ObsOperator: field names are strings")
        if len(self.start) < 2 or self.start[0] != 0:
            raise ValueError("ObsOperator: start has nobs + 1 >= 2 entries and start[0] is 0")
        counts = np.diff(self.start)
        if (counts < 1).any() or (counts > MAX_TERMS).any():
            raise ValueError(f"ObsOperator: an observation with 0 or more than {MAX_TERMS} terms")
        nt = int(self.start[-1])
        if not len(self.tname) == len(self.ti) == len(self.tj) == len(self.tw) == nt:
            raise ValueError(f"ObsOperator: {nt} terms by start, {len(self.tname)} names, {len(self.ti)} ti, {len(self.tj)} tj, "
                             f"{len(self.tw)} weights")
        if len(self.anchors) != self.nobs:
            raise ValueError(f"ObsOperator: {len(self.anchors)} anchors for {self.nobs} observations")
        if not np.isfinite(self.tw).all() or (self.tw == 0.0).any():
            raise ValueError("ObsOperator: a weight that is zero or not finite")
        self.names = tuple(dict.fromkeys(self.tname))
        if len(self.names) > MAX_FIELDS:
            raise ValueError(f"ObsOperator: {len(self.names)} distinct fields, more than {MAX_FIELDS}")

    @property
    def nobs(self) -> int:
        return len(self.start) - 1

    def row(self, j: int):
        """Observation j's terms, in order: [(name, i, j, w), ...]."""
        return [(self.tname[t], int(self.ti[t]), int(self.tj[t]), self.tw[t]) for t in range(int(self.start[j]), int(self.start[j + 1]))]

    @classmethod
    def from_rows(cls, rows, anchors):
        """From one list of (name, i, j, w) terms per observation."""
        start = np.cumsum([0] + [len(r) for r in rows])
        terms = [t for r in rows for t in r]
        return cls(start, [t[0] for t in terms], np.array([t[1] for t in terms], dtype=np.int64),
                   np.array([t[2] for t in terms], dtype=np.int64), np.array([t[3] for t in terms], dtype=np.float64), anchors)


def apply(op: ObsOperator, fields, blocks, block_of) -> np.ndarray:
    """H applied to downloaded arrays, with the device's operations in the device's order: the (nobs, n)
    array whose column m belongs to the m-th member.  fields[name][k]: the members' arrays of field `name` on
    local block k, in member order (shape and global indices the block's: A(bnd_x1:bnd_x2, bnd_y1:bnd_y2));
    blocks[k]: the block (bnd_x1, bnd_y1); block_of(i, j): the block a point is read in
    (OceanEnsemble.block_of).  The inputs are not written."""
    out = None
    with np.errstate(all="ignore"):
        for j in range(op.nobs):
            s = None
            for name, i, jj, w in op.row(j):
                b = blocks[block_of(i, jj)]
                x = np.array([a[i - b.bnd_x1, jj - b.bnd_y1] for a in fields[name][b.k]], dtype=np.float64)
                p = x * w
                s = p if s is None else s + p
            if out is None:
                out = np.zeros((op.nobs, len(s)))
            out[j] = s
    return out


def points(name: str, ij) -> ObsOperator:
    """One-term rows of weight 1.0 -- field `name` at the 1-based global points ij (nobs, 2) -- each anchored
    at its point: what ocn_ens_sample and ocn_ens_assimilate observe, bit for bit."""
    ij = _integers("points", ij, (2,))
    n = len(ij)
    return ObsOperator(np.arange(n + 1), [name] * n, ij[:, 0], ij[:, 1], np.ones(n), ij)


def bilinear(name: str, xy, mask=None, *, shape) -> ObsOperator:
    """Bilinear interpolation of field `name` to the positions xy (nobs, 2): fractional 1-based global index
    coordinates IN THE NAMED FIELD'S OWN ARRAY, within the basin of shape = (nx, ny) points.  As in
    ocn_ens_local_update, indices are those of the field's array: the half-cell stagger of u and v points
    against h points is the caller's to subtract before calling.

    With i0 = floor(x), fx = x - i0 and the same along y, the corners are taken in the order (i0, j0),
    (i0+1, j0), (i0, j0+1), (i0+1, j0+1) with the weights (1-fx)(1-fy), fx (1-fy), (1-fx) fy, fx fy.  A corner
    whose weight is exactly 0.0 is dropped, so an integer position is the one-term row of weight 1.0.  `mask`,
    an (nx, ny) array, drops the corners where it is 0 (land); if it dropped any, the remaining weights are
    divided by their sum in corner order.  ValueError if no corner is left or a remaining corner lies
    outside the basin.  The anchor is the nearest point, (floor(x + 0.5), floor(y + 0.5)) clipped to the
    basin: at most 0.71 cells from the position."""
    nx, ny = (int(v) for v in shape)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if not np.isfinite(xy).all():
        raise ValueError("bilinear: a position that is not finite")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (nx, ny):
            raise ValueError(f"bilinear: a mask of shape {mask.shape}, not {(nx, ny)}")
    rows, anchors = [], []
    for x, y in xy:
        i0, j0 = int(np.floor(x)), int(np.floor(y))
        fx, fy = x - np.float64(i0), y - np.float64(j0)
        one = np.float64(1.0)
        corners = [(i0, j0, (one - fx) * (one - fy)), (i0 + 1, j0, fx * (one - fy)), (i0, j0 + 1, (one - fx) * fy),
                   (i0 + 1, j0 + 1, fx * fy)]
        corners = [c for c in corners if c[2] != 0.0]
        for i, j, _ in corners:
            if not (1 <= i <= nx and 1 <= j <= ny):
                raise ValueError(f"bilinear: corner ({i}, {j}) of position ({x}, {y}) lies outside the basin {(nx, ny)}")
        if mask is not None:
            sea = [c for c in corners if mask[c[0] - 1, c[1] - 1] != 0]
            if len(sea) < len(corners) and sea:
                s = sea[0][2]
                for c in sea[1:]:
                    s = s + c[2]
                sea = [(i, j, w / s) for i, j, w in sea]
            corners = sea
        if not corners:
            raise ValueError(f"bilinear: no corner left at position ({x}, {y})")
        rows.append([(name, i, j, w) for i, j, w in corners])
        anchors.append((min(max(int(np.floor(x + 0.5)), 1), nx), min(max(int(np.floor(y + 0.5)), 1), ny)))
    return ObsOperator.from_rows(rows, np.array(anchors, dtype=np.int64).reshape(-1, 2))


def combine(ops, coeffs) -> ObsOperator:
    """The row-wise linear combination sum_a coeffs[a] * ops[a] of operators over the same observations --
    a radial velocity is combine([bilinear("ubrtr", ...), bilinear("vbrtr", ...)], [cos(theta), sin(theta)]);
    a coefficient is a float or one float per observation.  Row j is the terms of ops[0]'s row j, each weight
    times coeffs[0], then those of ops[1], ... in their order; a term at a (field, i, j) the row already holds
    is merged into that term (the weights added), and a term whose weight comes out as exactly 0.0 is dropped.
    The limits hold after merging: 1 .. MAX_TERMS terms a row, MAX_FIELDS fields.  The anchors are ops[0]'s."""
    ops = list(ops)
    if not ops or len(coeffs) != len(ops):
        raise ValueError("combine: one coefficient per operator, at least one operator")
    nobs = ops[0].nobs
    if any(o.nobs != nobs for o in ops):
        raise ValueError("combine: operators over different numbers of observations")
    cs = [np.broadcast_to(np.asarray(c, dtype=np.float64), (nobs,)) for c in coeffs]
    rows = []
    for j in range(nobs):
        row = {}
        for o, c in zip(ops, cs):
            for name, i, jj, w in o.row(j):
                key = (name, i, jj)
                row[key] = row[key] + w * c[j] if key in row else w * c[j]
        rows.append([(name, i, jj, w) for (name, i, jj), w in row.items() if w != 0.0])
    return ObsOperator.from_rows(rows, ops[0].anchors)
