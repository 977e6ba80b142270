"""The reference of the sparse linear observation operators (include/ocn_sw.h ocn_ens_sample_h,
ocn_ens_assimilate_h): the contract's ordered sum in numpy, and the chain the device entry is compared with.

The restatement lives in ocean_model_arch_amd/ens_obs_rule.py (`apply`), next to the builders a user starts
from; this module hands it to the tests.  Its independence comes from tests/test_ens_obs_cpu.py, which checks
it bit for bit against `scalar_apply`, a plain loop over Python floats.  Comparisons are bitwise (bits_equal:
the int64 views, NaN by position).

    H_j(u) = s:   s = x_0 * w_0;   then   p = x_t * w_t;  s = s + p   in the caller's term order
"""
import numpy as np

from ocean_model_arch_amd.ens_obs_rule import (MAX_FIELDS, MAX_TERMS, ObsOperator, apply, bilinear, combine,  # noqa: F401
                                               points)
from tests.ens_assim_ref import (KEYS, bits_equal, block_update, ensrf_obs_space_ordered, info_mismatches,  # noqa: F401
                                 local_rule, ringed_taper, taper_table)


def block_of(blocks):
    """OceanEnsemble.block_of over a list of blocks: the one whose interior holds the point, else the first
    whose array does."""
    def find(i, j):
        for b in blocks:
            if b.nx_start <= i <= b.nx_end and b.ny_start <= j <= b.ny_end:
                return b.k
        for b in blocks:
            if b.bnd_x1 <= i <= b.bnd_x2 and b.bnd_y1 <= j <= b.bnd_y2:
                return b.k
        raise ValueError(f"point ({i}, {j}) lies in no block's array")
    return find


def scalar_apply(op, fields, blocks, find):
    """`apply` as a loop over Python floats, one observation, one member and one term at a time."""
    n = len(next(iter(next(iter(fields.values())).values())))
    out = np.zeros((op.nobs, n))
    for j in range(op.nobs):
        for m in range(n):
            s = None
            for t in range(int(op.start[j]), int(op.start[j + 1])):
                i, jj = int(op.ti[t]), int(op.tj[t])
                b = blocks[find(i, jj)]
                x = float(fields[op.tname[t]][b.k][m][i - b.bnd_x1, jj - b.bnd_y1])
                p = x * float(op.tw[t])
                s = p if s is None else s + p
            out[j, m] = s
    return out


def downloads(e, names, idx):
    """fields[name][k]: the arrays of members idx of field `name` on local block k, as `apply` takes them."""
    return {nm: {b.k: [e.members[i].download(b.k, nm) for i in idx] for b in e.members[0].blocks} for nm in names}


def analysis(op, fields, blocks, find, values, variances, taper, names):
    """What ocn_ens_assimilate_h leaves, from downloads: hx0 = apply, the ordered observation-space loop at the
    anchors, the update's rule on every block of the fields `names`.  Returns (hx0, Y, Z, info, after) with
    after[name][k] the members' arrays afterwards."""
    hx0 = apply(op, fields, blocks, find)
    Y, Z, info = ensrf_obs_space_ordered(hx0, op.anchors, values, variances, taper)
    after = {nm: {b.k: block_update(fields[nm][b.k], b, op.anchors[:, 0], op.anchors[:, 1], Y, Z, taper) for b in blocks}
             for nm in names}
    return hx0, Y, Z, info, after
