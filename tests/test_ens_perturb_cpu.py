"""CPU checks of the correlated perturbations' restatement (ocean_model_arch_amd/ens_perturb_rule.py), the
reference of tests/test_gpu_ens_perturb.py: Philox4x32-10 against known answers, the smoothing against the
1-D kernel, the vectorised rule bit for bit against a scalar loop over Python ints and floats, the exact
centring, the exactness bound, and the statistics the coefficient promises.  No device.
"""
import math

import numpy as np
import pytest

from tests import ens_perturb_ref as R

M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- a scalar restatement, Python ints only
def philox_scalar(c, k):
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def white_scalar(seed, draw, member, i, j):
    o = philox_scalar((i & M32, j & M32, member, draw), (seed & M32, seed >> 32))
    return sum((w & 0xFFFF) + (w >> 16) for w in o) - 262140


def z_scalar(seed, draw, member, i, j, reach, passes):
    """Z at one point: the box sums written out as nested sums over the offsets of every pass."""
    if reach == 0 or passes == 0:
        return white_scalar(seed, draw, member, i, j)
    k = R.kernel_1d(reach, passes)          # the offsets' multiplicities
    a = reach * passes
    return sum(k[dx + a] * k[dy + a] * white_scalar(seed, draw, member, i + dx, j + dy)
               for dx in range(-a, a + 1) for dy in range(-a, a + 1))


# ---------------------------------------------------------------- Philox
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((M32,) * 4, (M32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("counter, key, want", KAT)
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(counter, key)
    assert tuple(int(x) for x in got) == want
    assert tuple(philox_scalar(counter, key)) == want
    # vectorised: the same answer at every element, whatever else is in the array
    arr = R.philox4x32_10([np.array([c, 1, c]) for c in counter], key)
    assert all(int(a[0]) == w and int(a[2]) == w for a, w in zip(arr, want))


def test_white_is_the_sum_of_halves():
    i = np.array([[-3, 0, 7], [2 ** 31 - 1, -2 ** 31, 12345]])
    j = np.array([[5, -1, 0], [9, 9, -77]])
    seed = 0xDEADBEEF12345678
    w = R.white(seed, 3, 17, i, j)
    assert w.dtype == np.int64 and np.abs(w).max() < 2 ** 18
    for at in np.ndindex(i.shape):
        assert int(w[at]) == white_scalar(seed, 3, 17, int(i[at]), int(j[at])), at


# ---------------------------------------------------------------- the smoothing
@pytest.mark.parametrize("reach, passes", [(0, 0), (0, 2), (3, 0), (1, 1), (2, 2), (4, 2), (3, 3), (16, 3)])
def test_smooth_of_a_delta_is_the_kernel(reach, passes):
    k = R.kernel_1d(reach, passes)
    a = reach * passes if reach and passes else 0
    assert len(k) == 2 * reach * passes + 1 and sum(k) == (2 * reach + 1) ** passes and k == k[::-1]
    k = k if a else [1]
    q = sum(t * t for t in k)
    w = np.zeros((4 * a + 1, 4 * a + 1), dtype=np.int64)
    w[2 * a, 2 * a] = 1
    z = R.smooth(w, reach if a else 0, passes if a else 0)
    assert z.shape == (2 * a + 1, 2 * a + 1)
    assert (z == np.outer(np.array(k, dtype=np.int64), np.array(k, dtype=np.int64))).all()
    assert int((z.astype(object) ** 2).sum()) == q * q


# ---------------------------------------------------------------- the rule against a scalar loop
@pytest.mark.parametrize("reach, passes, centre", [(2, 2, True), (1, 3, True), (0, 2, False), (3, 1, False), (2, 0, True)])
def test_rule_against_a_scalar_loop(reach, passes, centre):
    nx, ny, i0, j0 = 7, 5, -2, 11
    members, seed, draw, amp = [0, 2, 5], (7 << 32) | 99, 4, 0.03
    rng = np.random.default_rng(75)
    x = [np.asfortranarray(rng.uniform(-1.0, 1.0, (nx, ny))) for _ in members]
    mask = np.asfortranarray((rng.uniform(0.0, 1.0, (nx, ny)) > 0.3).astype(np.float32))
    x[1][2, 2], x[2][3, 3], x[0][4, 1] = np.nan, np.inf, -0.0
    got = R.perturb_rule(x, mask, i0, j0, members, seed, draw, reach, passes, centre, amp)
    n = len(members)
    q = sum(t * t for t in R.kernel_1d(reach, passes))
    den = R.K_SIGMA * float(q)
    if centre:
        den = den * float(n)
    c = amp / den
    for i in range(nx):
        for j in range(ny):
            z = [z_scalar(seed, draw, m, i0 + i, j0 + j, reach, passes) for m in members]
            d = [n * v - sum(z) for v in z] if centre else z
            assert sum(d) == 0 or not centre
            for a in range(n):
                want = x[a][i, j] + c * float(d[a]) if mask[i, j] > 0.5 else x[a][i, j]
                assert R.bits_equal(np.float64(got[a][i, j]), np.float64(want)), (a, i, j)
    assert np.isnan(got[1][2, 2]) and np.isinf(got[2][3, 3])
    assert np.isfinite(got[0]).all()          # a NaN or Inf reaches no other member


def test_centred_perturbations_sum_to_zero():
    members = [1, 3, 4, 8, 9]
    z = R.noise((20, 9), -4, 3, members, 5, 0, 4, 2)
    t = sum(z)
    d = [len(members) * v - t for v in z]
    assert (sum(d) == 0).all() and any((v != 0).any() for v in d)
    # and a window's noise does not depend on where the window starts
    z2 = R.noise((9, 4), 2, 5, members, 5, 0, 4, 2)
    assert all((a[6:15, 2:6] == b).all() for a, b in zip(z, z2))


# ---------------------------------------------------------------- the exactness bound
def test_exactness_bound():
    assert R.exact(256, 16, 2) and R.exact(13, 16, 3) and not R.exact(14, 16, 3)
    assert R.exact(256, 0, 3) and R.exact(256, 16, 0)
    assert 13 * 33 ** 6 * 2 ** 19 <= 2 ** 53 < 14 * 33 ** 6 * 2 ** 19
    x13 = [np.zeros((2, 2), order="F") for _ in range(14)]
    R.perturb_rule(x13[:13], None, 1, 1, range(13), 0, 0, 16, 3, True, 1.0)            # accepted
    with pytest.raises(AssertionError):
        R.perturb_rule(x13, None, 1, 1, range(14), 0, 0, 16, 3, True, 1.0)             # refused
    # the bound does what it is for: the largest |D| the rule can form is exact in double
    for n, r, p in ((13, 16, 3), (256, 16, 2)):
        worst = 2 * n * (2 ** 18) * (2 * r + 1) ** (2 * p)
        assert worst <= 2 ** 53 and int(float(worst)) == worst


# ---------------------------------------------------------------- the statistics the coefficient promises
def _window(reach, passes, size=512, seed=2024, member=0):
    return R.noise((size, size), 1, 1, [member], seed, 0, reach, passes)[0]


def test_variance_and_autocorrelation():
    """reach = 0, no centring, 512 x 512 points of one member: the sample variance of c D is amplitude^2 within
    2 % (262 144 independent samples; the sum of eight uniforms has kurtosis about 2.85, so the relative
    standard error is sqrt(1.85 / N) = 0.27 %, and 2 % is above seven of those).  Measured: -0.004 %.

    reach = 3, passes = 2: the lag-t autocorrelation along x is (k * k)_t / q.  The bound is five standard
    errors by Bartlett's formula for a linear filter of independent noise, summed over the two-dimensional
    lags of the separable correlation rho(a) rho(b):
        N var(r_t) = sum_b rho(b)^2  x  sum_a [rho(a)^2 + rho(a+t) rho(a-t) - 4 rho(t) rho(a) rho(a-t) + 2 rho(t)^2 rho(a)^2]
    with N the products in the lag-t mean; N over that sum is the window's effective sample count (3.7 million
    at lag 1, where numerator and denominator nearly cancel, down to 5 600 at lag 8, of 262 144 points).
    Measured deviations, lags 1..8, in standard errors: +1.10 +1.35 +1.47 +1.56 +1.62 +1.65 +1.66 +1.65 (one
    sign: the lags share the window and its variance estimate, which is +2.2 % against (q kSigma)^2, about one
    of its own standard errors)."""
    amp = 0.25
    d = _window(0, 0).astype(np.float64)
    v = R.coefficient(amp, 0, 0, 1, False) * d
    rel = v.var(ddof=1) / amp ** 2 - 1.0
    print(f"variance: relative deviation {rel:+.4%}")
    assert abs(rel) < 0.02

    reach, passes = 3, 2
    z = _window(reach, passes).astype(np.float64)
    k = R.kernel_1d(reach, passes)
    q = sum(t * t for t in k)
    L = len(k)
    rho = lambda t: sum(k[s] * k[s + abs(t)] for s in range(L - abs(t))) / q if abs(t) < L else 0.0   # noqa: E731
    c0 = (z * z).mean()
    print(f"lag 0: variance over (q kSigma)^2 - 1 = {c0 / (q * R.K_SIGMA) ** 2 - 1.0:+.4%}")
    sum_b = sum(rho(b) ** 2 for b in range(-L, L + 1))
    devs = []
    for t in range(1, 9):
        r_t = (z[t:, :] * z[:-t, :]).mean() / c0
        bart = sum_b * sum(rho(a) ** 2 + rho(a + t) * rho(a - t) - 4.0 * rho(t) * rho(a) * rho(a - t) + 2.0 * rho(t) ** 2 * rho(a) ** 2
                           for a in range(-2 * L, 2 * L + 1))
        n_prod = z[t:, :].size
        se = math.sqrt(bart / n_prod)
        devs.append((r_t - rho(t)) / se)
        print(f"lag {t}: r = {r_t:.5f}, rho = {rho(t):.5f}, effective samples {n_prod / bart:.0f}, deviation {devs[-1]:+.2f} se")
    assert max(abs(x) for x in devs) < 5.0, devs
    assert rho(2 * reach * passes + 1) == 0.0 and rho(1) > 0.8


def test_binding_lists_the_symbols():
    from ocean_model_arch_amd import _lib
    assert {"ocn_ens_perturb", "ocn_ens_perturb_download"} <= set(_lib.ENS_SYMBOLS)
