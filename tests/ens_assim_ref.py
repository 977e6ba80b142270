"""The reference of the serial filter on the device (include/ocn_sw.h ocn_ens_assimilate): the contract's
observation-space loop in numpy with explicit member loops, ordered sums and ordered spreads.

It lives in ocean_model_arch_amd/ens_local_rule.py next to `ensrf_obs_space`, the host path's loop it
restates (whose np.sum calls leave the order of the sums to numpy); this module hands it to the tests.
Its independence comes from tests/test_ens_assim_cpu.py, which checks it bit for bit against a plain scalar
loop over Python floats.  Comparisons are bitwise (bits_equal: the int64 views, NaN by position).

    s1 = x_0; s1 = s1 + x_m;  ybar = s1 / n;  y'_m = x_m - ybar;  q = y'_0 y'_0; p = y'_m y'_m, q = q + p
    s = q / (n-1);  D = s + r_k;  d = value_k - ybar;  t = r_k / D;  alpha = 1 / (1 + sqrt(t));  c = (n-1) D
    Y[k][m] = y'_m;  Z[k][m] = (d - alpha y'_m) / c;  every row then takes observation k by the update's rule
"""
import numpy as np

from ocean_model_arch_amd.ens_local_rule import ensrf_obs_space_ordered  # noqa: F401
from tests.ens_local_ref import STATE, bits_equal, block_update, local_rule, ringed_taper, taper_table  # noqa: F401

KEYS = ("hx", "innovations", "prior_spread", "posterior_spread")


def info_mismatches(got, want):
    """The keys of KEYS whose arrays differ in any bit."""
    return [k for k in KEYS if not bits_equal(got[k], want[k])]


def gather(fields_by_block, blocks, block_of, ij):
    """hx from downloads: fields_by_block[k] the members' arrays of block k, block_of(i, j) the block an
    observation is read in."""
    rows = []
    for i, j in np.asarray(ij):
        b = blocks[block_of(int(i), int(j))]
        rows.append([a[int(i) - b.bnd_x1, int(j) - b.bnd_y1] for a in fields_by_block[b.k]])
    return np.array(rows, dtype=np.float64)
