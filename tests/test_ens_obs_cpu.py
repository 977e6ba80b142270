"""CPU tests of the sparse linear observation operators (ocean_model_arch_amd/ens_obs_rule.py): the numpy
restatement of the contract's ordered sum against a scalar loop over Python floats, the builders' weights and
errors, and how the filter's followed rows relate to H of the updated fields.  No device, no library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import ens_obs_ref as O
from tests.test_ens_local_cpu import ANALYTIC_TOL


def _two_blocks():
    """Two blocks side by side, one ring of halo each: interiors 1..6 and 7..12 along x, 1..7 along y."""
    def blk(k, x0, x1):
        return SimpleNamespace(k=k, nx_start=x0, nx_end=x1, ny_start=1, ny_end=7, bnd_x1=x0 - 1, bnd_x2=x1 + 1, bnd_y1=0,
                               bnd_y2=8)
    return [blk(0, 1, 6), blk(1, 7, 12)]


def _fields(blocks, names, n, seed):
    rng = np.random.default_rng(seed)
    return {nm: {b.k: [rng.uniform(-1.5, 1.5, (b.bnd_x2 - b.bnd_x1 + 1, b.bnd_y2 - b.bnd_y1 + 1)) for _ in range(n)]
                 for b in blocks} for nm in names}


def test_restatement_is_the_scalar_loop():
    """Rows of 1, 2, 4 and 16 terms over three fields and two blocks, points in the halo and terms of one
    row in different blocks, a -0.0 and a NaN among the values: `apply` bit for bit the loop over Python
    floats."""
    blocks = _two_blocks()
    find = O.block_of(blocks)
    names = ("ssh", "ubrtr", "vbrtr")
    rng = np.random.default_rng(3)
    for n in (1, 2, 5):
        fields = _fields(blocks, names, n, n)
        fields["ssh"][0][0][3, 3] = -0.0
        fields["ubrtr"][1][n - 1][2, 2] = np.nan
        rows = [[("ssh", 3, 3, 1.0)], [("ssh", 3, 3, -2.5), ("ubrtr", 8, 2, 0.3)],
                [("ssh", 6, 4, 0.1), ("ssh", 7, 4, 0.2), ("ssh", 6, 5, 0.3), ("ssh", 7, 5, 0.4)],
                [(names[t % 3], int(rng.integers(0, 14)), int(rng.integers(0, 9)), float(rng.uniform(-1, 1))) for t in range(16)],
                [("vbrtr", 0, 0, 1e-3), ("vbrtr", 13, 8, 1e3)]]
        op = O.ObsOperator.from_rows(rows, np.array([[3, 3], [5, 2], [6, 4], [1, 1], [12, 7]]))
        got, want = O.apply(op, fields, blocks, find), O.scalar_apply(op, fields, blocks, find)
        assert got.shape == (5, n) and O.bits_equal(got, want)
        assert O.bits_equal(got[0], np.array([a[3, 3] for a in fields["ssh"][0]]))   # the unit row: a copy, -0.0 kept


def test_bilinear_weights():
    """An integer position is the one-term row of weight exactly 1.0; a cell centre four weights of 0.25 in
    the corner order; one masked corner leaves three of 0.25 / 0.75; the anchors are the nearest points."""
    op = O.bilinear("ssh", [[4.0, 6.0], [13.0, 9.0], [4.5, 6.5], [4.25, 6.0]], shape=(13, 9))
    assert op.row(0) == [("ssh", 4, 6, 1.0)] and op.row(1) == [("ssh", 13, 9, 1.0)]
    assert op.row(2) == [("ssh", 4, 6, 0.25), ("ssh", 5, 6, 0.25), ("ssh", 4, 7, 0.25), ("ssh", 5, 7, 0.25)]
    assert op.row(3) == [("ssh", 4, 6, 0.75), ("ssh", 5, 6, 0.25)]
    assert op.anchors.tolist() == [[4, 6], [13, 9], [5, 7], [4, 6]]
    mask = np.ones((13, 9), dtype=np.int32)
    mask[4, 5] = 0                                        # the point (5, 6)
    third = np.float64(0.25) / np.float64(0.75)
    op = O.bilinear("ssh", [[4.5, 6.5], [4.0, 6.0]], mask, shape=(13, 9))
    assert op.row(0) == [("ssh", 4, 6, third), ("ssh", 4, 7, third), ("ssh", 5, 7, third)]
    assert op.row(1) == [("ssh", 4, 6, 1.0)]
    unit = O.points("ubrtr", [[4, 6], [13, 9]])
    assert unit.row(1) == [("ubrtr", 13, 9, 1.0)] and unit.anchors.tolist() == [[4, 6], [13, 9]]


def test_builders_refuse():
    """All corners masked, a corner outside the basin, zero and non-finite weights, 17 terms, 5 fields, and the
    table's own shape."""
    with pytest.raises(ValueError):
        O.bilinear("ssh", [[4.5, 6.5]], np.zeros((13, 9)), shape=(13, 9))
    for xy in ([13.5, 4.0], [0.5, 4.0], [4.0, 9.25], [4.0, 0.0]):
        with pytest.raises(ValueError):
            O.bilinear("ssh", [xy], shape=(13, 9))
    for w in (0.0, -0.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            O.ObsOperator.from_rows([[("ssh", 2, 2, 1.0), ("ssh", 3, 2, w)]], [[2, 2]])
    with pytest.raises(ValueError):
        O.ObsOperator.from_rows([[("ssh", 1 + t % 13, 1 + t // 13, 0.1) for t in range(O.MAX_TERMS + 1)]], [[2, 2]])
    O.ObsOperator.from_rows([[("ssh", 1 + t % 13, 1 + t // 13, 0.1) for t in range(O.MAX_TERMS)]], [[2, 2]])
    five = ("ssh", "sshp", "ubrtr", "vbrtr", "ubrtrp")
    with pytest.raises(ValueError):
        O.ObsOperator.from_rows([[(nm, 2, 2, 0.5)] for nm in five], [[2, 2]] * 5)
    O.ObsOperator.from_rows([[(nm, 2, 2, 0.5)] for nm in five[:O.MAX_FIELDS]], [[2, 2]] * 4)
    with pytest.raises(ValueError):                        # an observation without terms
        O.ObsOperator([0, 1, 1], ["ssh"], [2], [2], np.array([1.0]), [[2, 2], [3, 3]])
    with pytest.raises(ValueError):                        # start[0] != 0
        O.ObsOperator([1, 2], ["ssh", "ssh"], [2, 2], [2, 2], np.array([1.0, 1.0]), [[2, 2]])
    with pytest.raises(ValueError):                        # one anchor short
        O.ObsOperator([0, 1, 2], ["ssh", "ssh"], [2, 2], [2, 2], np.array([1.0, 1.0]), [[2, 2]])
    with pytest.raises(TypeError):
        O.ObsOperator([0, 1], ["ssh"], [2.0], [2], np.array([1.0]), [[2, 2]])
    with pytest.raises(TypeError):
        O.ObsOperator([0, 1], ["ssh"], [2], [2], np.array([1.0], dtype=np.float32), [[2, 2]])
    with pytest.raises(ValueError):                        # 9 + 9 distinct terms after merging
        O.combine([O.ObsOperator.from_rows([[("ssh", 1 + t, 1, 0.1) for t in range(9)]], [[2, 2]]),
                   O.ObsOperator.from_rows([[("ssh", 1 + t, 2, 0.1) for t in range(9)]], [[2, 2]])], [1.0, 1.0])


def test_combine_keeps_order_and_anchors():
    """cos(theta) u + sin(theta) v: u's terms in their order, then v's, each weight one product; the anchors
    are the first operator's; a term both operators hold is merged where it first stood."""
    u = O.bilinear("ubrtr", [[4.5, 6.5], [7.0, 3.25]], shape=(13, 9))
    v = O.bilinear("vbrtr", [[4.75, 6.0], [7.0, 3.0]], shape=(13, 9))
    c, s = np.cos(np.array([0.3, 2.0])), np.sin(np.array([0.3, 2.0]))
    r = O.combine([u, v], [c, s])
    assert r.row(0) == [(nm, i, j, w * c[0]) for nm, i, j, w in u.row(0)] + [(nm, i, j, w * s[0]) for nm, i, j, w in v.row(0)]
    assert r.row(1) == [("ubrtr", 7, 3, 0.75 * c[1]), ("ubrtr", 7, 4, 0.25 * c[1]), ("vbrtr", 7, 3, s[1])]
    assert r.anchors.tolist() == u.anchors.tolist() == [[5, 7], [7, 3]] and r.names == ("ubrtr", "vbrtr")
    twice = O.combine([u, u], [0.5, 0.25])
    assert twice.row(0) == [(nm, i, j, w * 0.5 + w * 0.25) for nm, i, j, w in u.row(0)]


def _followed_and_applied(n, taper):
    """A 13 x 9 array, three bilinear observations, n members: the rows the ordered loop follows at the anchors,
    and H applied to the fields that local_rule leaves with the loop's Y and Z."""
    rng = np.random.default_rng(100 + n)
    blocks = [SimpleNamespace(k=0, nx_start=1, nx_end=13, ny_start=1, ny_end=9, bnd_x1=1, bnd_x2=13, bnd_y1=1, bnd_y2=9)]
    find = O.block_of(blocks)
    fields = {"ssh": {0: [rng.uniform(0.5, 1.5, (13, 9)) for _ in range(n)]}}
    op = O.bilinear("ssh", [[3.3, 4.6], [7.5, 2.25], [11.8, 7.1]], shape=(13, 9))
    hx0 = O.apply(op, fields, blocks, find)
    values = hx0.mean(axis=1) + np.array([0.05, -0.08, 0.02])
    variances = np.full(3, 0.01) + hx0.var(axis=1, ddof=1) * 0.5
    _, _, _, info, after = O.analysis(op, fields, blocks, find, values, variances, taper, ("ssh",))
    return info["hx"], O.apply(op, after, blocks, find)


@pytest.mark.parametrize("n", [2, 5, 9, 33])
def test_flat_taper_rows_are_h_of_the_fields(n):
    """With a taper that is 1.0 over the whole array the update is linear in the state with ONE coefficient per
    observation, so H of the updated fields is the followed row up to rounding: a few dozen rounded
    operations on O(1) data, ~1e-15 relative, against ANALYTIC_TOL."""
    followed, applied = _followed_and_applied(n, np.ones(13 * 13 + 9 * 9))
    err = float(np.max(np.abs(applied - followed) / np.abs(followed)))
    print(f"n = {n}: worst relative difference {err:.3e}")
    assert err <= ANALYTIC_TOL


def test_tapered_rows_are_not_h_of_the_fields():
    """With a Gaspari-Cohn taper the two differ: the followed row takes observation k with the taper at its
    ANCHOR's distance from k's anchor, while H of the updated fields weighs each term's point by that point's
    own distance -- the rows are an augmented state, not H of the fields, and calls do not compose."""
    followed, applied = _followed_and_applied(5, O.taper_table(6.0))
    print(f"worst relative difference {float(np.max(np.abs(applied - followed) / np.abs(followed))):.3e}")
    doc = test_tapered_rows_are_not_h_of_the_fields.__doc__
    assert "anchor" in doc.lower() and "augmented state" in doc
