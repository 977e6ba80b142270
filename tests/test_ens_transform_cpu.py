"""CPU checks of the ensemble recombination (ocn_ens_transform, ocn_ens_sample): the numpy restatement the
GPU tests compare against (tests/ens_transform_ref.py) is itself checked against an independent scalar
loop over Python floats, and the properties the contract promises are checked on it; the entries'
null-ensemble errors need no device."""
import os

import numpy as np
import pytest

from tests import ens_transform_ref as T

ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    import ocean_model_arch_amd as amd
    if not os.path.exists(amd._lib.LIB_PATH):
        amd.build()
    return amd.lib()


def _members(n=7):
    """n members of a 5 x 4 array; member 1 holds a NaN and both infinities, member 0 a -0.0, member 2 a +0.0."""
    x = np.random.default_rng(91).uniform(-1.0, 1.0, (n, 5, 4))
    if n > 1:
        x[1, 0, 0], x[1, 2, 1], x[1, 4, 3] = np.nan, np.inf, -np.inf
    x[0, 3, 2] = -0.0
    if n > 2:
        x[2, 3, 2] = 0.0
    return x


def _scalar(x, w):
    """The contract with Python floats (IEEE doubles), one point and one column at a time."""
    n = len(x)
    out = np.zeros_like(x)
    for idx in np.ndindex(x.shape[1:]):
        for b in range(n):
            s, first = 0.0, True
            for a in range(n):
                wab = float(w[a, b])
                if wab == 0.0:
                    continue
                p = float(x[(a,) + idx]) * wab
                s, first = (p, False) if first else (s + p, False)
            out[(b,) + idx] = s
    return out


def _same(got, want):
    return all(T.bits_equal(g, v) for g, v in zip(got, want)) and len(got) == len(want)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 9])
def test_restatement_matches_scalar_loop(n):
    x = _members(n)
    rng = np.random.default_rng(n)
    dense = rng.uniform(-2.0, 2.0, (n, n))
    sparse = np.where(rng.uniform(0, 1, (n, n)) < 0.5, 0.0, dense)
    signed_zero = np.where(sparse == 0.0, -0.0, sparse)
    tiny = dense * 5e-324 / 2.0 + np.where(dense > 0, 1e-310, -3e-320)   # denormal weights
    for w in (dense, sparse, signed_zero, tiny, T.mixed_weights(n)):
        assert _same(T.transform(list(x), w), _scalar(x, w))


def test_identity_and_permutations_copy_bits():
    """-0.0, NaN and the infinities included: NaN by position, everything else the same 64 bits."""
    x = _members()
    n = len(x)
    assert _same(T.transform(list(x), np.eye(n)), x)
    for seed in range(4):
        perm = np.random.default_rng(seed).permutation(n)
        w = np.zeros((n, n))
        w[perm, np.arange(n)] = 1.0          # new member b = old member perm[b]
        got = T.transform(list(x), w)
        assert _same(got, x[perm])
        assert np.signbit(got[list(perm).index(0)][3, 2])
    dup = np.zeros((n, n))
    dup[3, :] = 1.0                          # resampling: every member becomes member 3
    assert _same(T.transform(list(x), dup), [x[3]] * n)


def test_zero_column_gives_positive_zero():
    x = _members()
    w = T.mixed_weights(len(x))
    w[:, 2] = -0.0
    got = T.transform(list(x), w)
    assert not got[2].any() and not np.signbit(got[2]).any()
    assert not got[-1].any() and not np.signbit(got[-1]).any()   # mixed_weights' own zero column


def test_nan_member_with_zero_row_reaches_no_other_column():
    x = _members()
    n = len(x)
    w = np.random.default_rng(5).uniform(-1.0, 1.0, (n, n))
    w[1, :] = 0.0
    w[:, 1] = 0.0
    w[1, 1] = 1.0                            # member 1 keeps itself: a unit column
    got = T.transform(list(x), w)
    assert T.bits_equal(got[1], x[1])
    assert all(np.isfinite(got[b]).all() for b in range(n) if b != 1)
    clean = x.copy()
    clean[1] = 0.0                           # the same columns whatever member 1 holds
    want = T.transform(list(clean), w)
    assert all(T.bits_equal(got[b], want[b]) for b in range(n) if b != 1)


def test_use_ordering():
    """The members in use run in member order: a subset's transform is the transform of that sub-list,
    and the order of summation is the list's -- reversing it changes the bits of a dense column."""
    x = _members(9)
    idx = [0, 2, 5, 7]
    w = np.random.default_rng(11).uniform(-1.0, 1.0, (4, 4))
    got = T.transform([x[i] for i in idx], w)
    assert _same(got, _scalar(x[idx], w))
    rev = T.transform([x[i] for i in idx[::-1]], w[::-1, :])
    assert all(np.allclose(g, r, rtol=1e-12, atol=0) for g, r in zip(got, rev))
    assert not _same(got, rev)               # same sums mathematically, another order: other roundings


def test_inputs_are_not_written():
    x = _members()
    keep = x.copy()
    T.transform(list(x), T.mixed_weights(len(x)))
    assert T.bits_equal(x, keep)


def test_null_ensemble_is_an_argument_error(lib):
    assert lib.ocn_ens_sample(None, 0, None, 1, None, None, None, None) == ERR_ARG
    assert lib.ocn_ens_transform(None, None, 1, None, None) == ERR_ARG


def test_wrapper_names_the_state():
    from ocean_model_arch_amd import ensemble
    assert ensemble.STATE == T.STATE
