"""The reference of the localized observation update (include/ocn_sw.h ocn_ens_local_update): the numpy
restatement of the rule, vectorised over the points and loop-ordered over the members and the
observations, and the observation-space loop of the serial square-root filter.

Both live in ocean_model_arch_amd/ens_local_rule.py, because OceanEnsemble.assimilate follows the ensemble
at the observed points with the very same function; this module hands them to the tests, so that the
driver and the tests share ONE function.  Its independence comes from tests/test_ens_local_cpu.py, which
checks it bit for bit against a plain scalar triple loop over Python floats.  numpy's elementwise
operations are single IEEE double operations, so results are compared bitwise (bits_equal: the int64
views, NaN by position).

    d2 = (i-io[k])^2 + (j-jo[k])^2;  d2 >= ntaper: skip k;  rho = taper[d2];  rho +-0.0: skip k
    s = x_0;  s = s + x_m (m = 1 .. n-1);  mean = s / n
    a = (x_0 - mean) y[k][0];  p = (x_m - mean) y[k][m], a = a + p (m = 1 .. n-1);  g = rho a
    x_m = x_m + g z[k][m]
"""
import numpy as np

from ocean_model_arch_amd.ens_local_rule import ensrf_obs_space, local_rule, reach_of, taper_table  # noqa: F401
from tests.ens_stats_ref import bits_equal  # noqa: F401  (the comparison of every user of this module)

STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")


def block_update(fields, block, io, jo, y, z, taper):
    """`local_rule` on the members' whole arrays of one block (the library's BlockInfo, bnd_x1 .. bnd_y2, or
    the oracle's Block, bx1 .. by2): the array's points by their global indices."""
    x1, x2, y1, y2 = ((block.bnd_x1, block.bnd_x2, block.bnd_y1, block.bnd_y2) if hasattr(block, "bnd_x1") else
                      (block.bx1, block.bx2, block.by1, block.by2))
    gi, gj = np.arange(x1, x2 + 1), np.arange(y1, y2 + 1)
    return local_rule(fields, gi, gj, io, jo, y, z, taper)


def rows(nobs, n, seed, scale=0.25):
    """Well-scaled y and z rows: O(scale) entries of both signs, so that a few dozen observations keep O(1)
    fields O(1)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (nobs, n)), rng.uniform(-scale, scale, (nobs, n))


def ringed_taper(ntaper, seed=0):
    """A taper with a zero ring inside its support: positive entries falling from 1.0, and +0.0 / -0.0
    over the middle fifth of the table."""
    t = np.linspace(1.0, 0.05, ntaper) * np.random.default_rng(seed).uniform(0.9, 1.0, ntaper)
    t[0] = 1.0
    a, b = 2 * ntaper // 5, 3 * ntaper // 5
    t[a:b:2] = 0.0
    t[a + 1:b:2] = -0.0
    return t
