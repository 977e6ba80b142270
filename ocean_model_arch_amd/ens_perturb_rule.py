"""Correlated random perturbations of the members in numpy (include/ocn_sw.h ocn_ens_perturb): the rule the
device applies, restated on whole arrays.

    W_m(i, j) = S - 262140, S the sum of the eight 16-bit halves of
                Philox4x32-10((uint32)i, (uint32)j, u_m, draw; seed & 0xffffffff, seed >> 32)
    Z_m = B_y^P B_x^P W_m, (B_x Z)(i, j) = sum over d = -R .. R of Z(i + d, j)       (int64, exact)
    D_m = n Z_m - sum over the members in use of Z          (centre)       D_m = Z_m   (not)
    q = the sum of the squares of the 1-D box of width 2R+1 convolved P times
    den = kSigma * (double)q;  with centre: den = den * (double)n;  c = amplitude / den
    where the mask applies (no mask, or mask > 0.5f):  d = (double)D_m;  p = c * d;  x_m = x_m + p

Everything up to D is integer arithmetic, so any evaluation order gives the same bits; numpy's elementwise
multiply and add are single IEEE double operations and nothing here is fused, so `perturb_rule` gives the
device's bits.  tests/ens_perturb_ref.py hands it to the tests, which check it against a scalar loop.  Pure
numpy: no device, no library.
"""
from __future__ import annotations

import numpy as np

MAX_REACH, MAX_PASSES = 16, 3
K_SIGMA = float.fromhex("0x1.a20bd6fff1bdfp+15")   # sqrt(2 (2^32 - 1) / 3): the standard deviation of S
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LOW, _32, _16 = np.uint64(0xFFFFFFFF), np.uint64(32), np.uint64(16)
_HALF = np.uint64(0xFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 of the four counter words and the two key words (arrays or scalars of values below
    2^32, broadcast against each other): the four output words as uint64 arrays below 2^32."""
    c = [np.asarray(x, dtype=np.uint64) & _LOW for x in counter]
    c = [np.array(x, dtype=np.uint64) for x in np.broadcast_arrays(*c)]
    k0, k1 = (np.uint64(int(x) & 0xFFFFFFFF) for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]              # 32 x 32 bits: below 2^64
        c = [(p1 >> _32) ^ c[1] ^ k0, p1 & _LOW, (p0 >> _32) ^ c[3] ^ k1, p0 & _LOW]
        k0, k1 = (k0 + _W0) & _LOW, (k1 + _W1) & _LOW
    return c


def white(seed, draw, member, i, j):
    """W of member `member` (its index in the ensemble) at the global indices i, j (integer arrays, broadcast
    against each other; any values, negative ones included): int64, |W| < 2^18."""
    seed = int(seed)
    assert 0 <= seed < 1 << 64 and 0 <= int(draw) < 1 << 32 and 0 <= int(member) < 1 << 32
    i = np.asarray(i, dtype=np.int64).astype(np.int32).astype(np.int64).astype(np.uint64)   # (uint32)(int32)i
    j = np.asarray(j, dtype=np.int64).astype(np.int32).astype(np.int64).astype(np.uint64)
    out = philox4x32_10((i, j, int(member), int(draw)), (seed & 0xFFFFFFFF, seed >> 32))
    s = np.zeros(out[0].shape, dtype=np.uint64)
    for o in out:
        s = s + (o & _HALF) + (o >> _16)
    return s.astype(np.int64) - np.int64(262140)


def apron(reach, passes):
    """How far Z looks: R P points (0 where R = 0 or P = 0: Z = W)."""
    assert 0 <= reach <= MAX_REACH and 0 <= passes <= MAX_PASSES
    return int(reach) * int(passes)


def smooth(w, reach, passes):
    """Z over (nx, ny) from W over the window widened by the apron, (nx + 2 R P, ny + 2 R P): P box sums of
    width 2R+1 along x, then P along y, each taking R points off either end."""
    z = np.asarray(w, dtype=np.int64)
    r = int(reach)
    a = apron(reach, passes)
    assert z.ndim == 2 and z.shape[0] >= 2 * a and z.shape[1] >= 2 * a
    if r == 0:
        return z.copy()
    for axis in (0, 1):
        for _ in range(int(passes)):
            n = z.shape[axis] - 2 * r
            z = sum(np.take(z, range(d, d + n), axis=axis) for d in range(2 * r + 1))
    return z


def kernel_1d(reach, passes):
    """k: the box of width 2R+1 convolved with itself P times (the delta for P = 0), as Python ints."""
    apron(reach, passes)
    k = [1]
    for _ in range(int(passes)):
        k = [sum(k[t - d] for d in range(2 * int(reach) + 1) if 0 <= t - d < len(k)) for t in range(len(k) + 2 * int(reach))]
    return k


def exact(n, reach, passes):
    """The exactness bound: n (2R+1)^(2P) 2^19 <= 2^53 keeps every integer-to-double conversion exact."""
    return int(n) * (2 * int(reach) + 1) ** (2 * int(passes)) * (1 << 19) <= 1 << 53


def coefficient(amplitude, reach, passes, n, centre):
    """c: amplitude over the standard deviation of D."""
    q = sum(t * t for t in kernel_1d(reach, passes))
    den = np.float64(K_SIGMA) * np.float64(q)
    if centre:
        den = den * np.float64(n)
    return np.float64(amplitude) / den


def noise(shape, i0, j0, members, seed, draw, reach, passes):
    """Z_m over an array of `shape` whose element [0, 0] has the global indices (i0, j0), for each member
    index of `members`: a list of int64 arrays."""
    a = apron(reach, passes) if reach and passes else 0
    i = np.arange(i0 - a, i0 + shape[0] + a, dtype=np.int64)[:, None]
    j = np.arange(j0 - a, j0 + shape[1] + a, dtype=np.int64)[None, :]
    return [smooth(white(seed, draw, m, i, j), reach if a else 0, passes if a else 0) for m in members]


def perturb_rule(x, mask, i0, j0, members, seed, draw, reach, passes, centre, amplitude):
    """new_x: the members' arrays x (the members in use, member order, one shape; element [0, 0] at the global
    indices (i0, j0)) after the rule, as fresh arrays.  members: their indices in the ensemble; mask: member
    0's real(4) mask array of that shape, or None."""
    x = [np.array(a, dtype=np.float64, order="F", copy=True) for a in x]
    n = len(x)
    members = [int(m) for m in members]
    assert n >= 1 and len(members) == n and sorted(set(members)) == members
    assert (n >= 2 or not centre) and exact(n, reach, passes)
    assert np.isfinite(amplitude) and amplitude > 0.0
    z = noise(x[0].shape, i0, j0, members, seed, draw, reach, passes)
    c = coefficient(amplitude, reach, passes, n, centre)
    t = sum(z) if centre else None
    write = np.ones(x[0].shape, dtype=bool) if mask is None else np.asarray(mask, dtype=np.float32) > np.float32(0.5)
    assert write.shape == x[0].shape
    with np.errstate(all="ignore"):
        for m in range(n):
            dm = np.int64(n) * z[m] - t if centre else z[m]
            d = dm.astype(np.float64)
            p = c * d
            new = x[m] + p
            x[m][write] = new[write]
    return x
