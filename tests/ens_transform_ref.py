"""The reference of the ensemble recombination (include/ocn_sw.h ocn_ens_transform): the numpy restatement
of the contract, a per-column loop over the kept terms on whole arrays.  numpy's elementwise multiply and
add are the same two IEEE double operations per element, so results are compared bitwise
(tests/ens_stats_ref.py bits_equal: the int64 views, NaN by position).

    new_b = +0.0                      if column b has no weight other than +0.0 / -0.0
    otherwise, over a ascending, skipping every a whose w[a][b] is +0.0 or -0.0:
        first kept term:  s = x_a * w[a][b]
        later kept terms: p = x_a * w[a][b];  s = s + p
    new_b = s
"""
import numpy as np

from tests.ens_stats_ref import bits_equal  # noqa: F401  (the comparison of every user of this module)

STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")


def transform(fields, w):
    """The new members' arrays from `fields`, the old members' arrays in member order, and the (n, n)
    weights w[a, b] of old member a in new member b.  Fresh arrays: the inputs are not written."""
    x = [np.asarray(a, dtype=np.float64) for a in fields]
    n = len(x)
    w = np.asarray(w, dtype=np.float64)
    assert n >= 1 and w.shape == (n, n) and np.isfinite(w).all()
    out = []
    with np.errstate(all="ignore"):
        for b in range(n):
            s = None
            for a in range(n):
                if w[a, b] == 0.0:   # +0.0 and -0.0 (the weights are finite): the term is not formed
                    continue
                p = x[a] * w[a, b]
                s = p if s is None else s + p
            out.append(np.asfortranarray(np.zeros_like(x[0]) if s is None else s))
    return out


def mixed_weights(n, seed=0):
    """An (n, n) matrix that mixes what the kernels treat differently: a dense block with negative weights
    over the first members, a permutation, an identity column and a zero column over the rest."""
    if n == 1:
        return np.array([[-0.75]])
    if n == 2:
        return np.array([[0.5, 0.0], [-1.5, 0.0]])
    rng = np.random.default_rng(7000 + 10 * n + seed)
    w = np.zeros((n, n))
    d = max(2, n // 2)
    w[:d, :d] = rng.uniform(-1.0, 1.0, (d, d)) / d
    rest = list(range(d, n))
    rest.pop()                      # the last column stays zero
    if rest:
        i = rest.pop()
        w[i, i] = 1.0               # an identity column
    for a, b in zip(rest, rest[1:] + rest[:1]):
        w[a, b] = 1.0               # a cyclic permutation of the others
    return w
