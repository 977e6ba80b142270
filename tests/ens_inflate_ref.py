"""The reference of the per-point covariance inflation (include/ocn_sw.h ocn_ens_inflate, ocn_ens_spread_save):
the numpy restatement of the rule, vectorised over the points and loop-ordered over the members.

It lives in ocean_model_arch_amd/ens_inflate_rule.py; this module hands it to the tests.  Its independence
comes from tests/test_ens_inflate_cpu.py, which checks it bit for bit against a plain scalar loop over
Python floats.  numpy's elementwise operations are single IEEE double operations, so results are compared
bitwise (bits_equal: the int64 views, NaN by position).

    s = x_0;  s = s + x_m;  mean = s / n;  d_m = x_m - mean
    q = d_0 d_0;  p = d_m d_m, q = q + p;  var = q / (n-1);  sa = sqrt(var)
    CONST: f = alpha (where sa > 0, finite)    RTPS: t = sb - sa; r = t / sa; g = alpha r; f = 1.0 + g
                                                     (where sa > 0, sa and sb finite)
    where the rule applies and f != 1.0:  p = f d_m;  x_m = mean + p
"""
from ocean_model_arch_amd.ens_inflate_rule import CONST, RTPS, inflate_rule, spread  # noqa: F401
from tests.ens_stats_ref import bits_equal  # noqa: F401  (the comparison of every user of this module)

STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")


def same(got, want):
    """Two lists of arrays, bit for bit."""
    return len(got) == len(want) and all(bits_equal(g, v) for g, v in zip(got, want))
