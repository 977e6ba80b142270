"""The reference of the correlated perturbations (include/ocn_sw.h ocn_ens_perturb): the numpy restatement of
the rule, applied to whole block arrays with their global origin.

It lives in ocean_model_arch_amd/ens_perturb_rule.py; this module hands it to the tests.  Its independence
comes from tests/test_ens_perturb_cpu.py, which checks Philox against published known answers and the
vectorised rule bit for bit against a plain scalar loop over Python ints and floats.  The random part is
integer arithmetic and the update two IEEE double operations, so results are compared bitwise (bits_equal:
the int64 views, NaN by position).

    W = S - 262140, S the eight 16-bit halves of Philox4x32-10((uint32)i, (uint32)j, member, draw; seed)
    Z = B_y^P B_x^P W (box sums of width 2R+1);  D_m = n Z_m - sum Z (centre), Z_m (not)
    c = amplitude / (kSigma q [n]);  where the mask applies:  p = c (double)D_m;  x_m = x_m + p
"""
import numpy as np

from ocean_model_arch_amd.ens_perturb_rule import (K_SIGMA, coefficient, exact, kernel_1d, noise, perturb_rule,  # noqa: F401
                                                   philox4x32_10, smooth, white)
from ocean_model_arch_amd.ensemble import STATE_GROUPS, default_mask  # noqa: F401
from tests.ens_stats_ref import bits_equal  # noqa: F401  (the comparison of every user of this module)


def block_noise(b, members, seed, draw, reach, passes):
    """Z of the members with the ensemble indices `members` over block b's whole array (b: a BlockInfo)."""
    return noise(b.shape, b.bnd_x1, b.bnd_y1, members, seed, draw, reach, passes)


def block_rule(b, x, mask, members, seed, draw, reach, passes, centre, amplitude):
    """perturb_rule over block b's whole arrays x (the members in use, member order) under the mask array."""
    return perturb_rule(x, mask, b.bnd_x1, b.bnd_y1, members, seed, draw, reach, passes, centre, amplitude)


def expected(e, groups, idx, seed=0, draw=0, reach=4, passes=2, centre=True, amplitude=1.0, masks=None, before=None):
    """What OceanEnsemble.perturb(amplitude, reach, passes, groups, masks, seed, draw, centre, idx) makes of the
    members' own downloads (`before`: {block: {field: [arrays of the members idx]}}; None: downloaded here), on
    every block: {block: {field: [new arrays]}}."""
    out = {}
    for b in e.members[0].blocks:
        out[b.k] = {}
        for g, grp in enumerate(groups):
            for nm in ((grp,) if isinstance(grp, str) else grp):
                mname = masks[nm] if masks is not None and nm in masks else default_mask(nm)
                mask = None if mname is None else e.members[0].download(b.k, mname)
                x = before[b.k][nm] if before is not None else [e.members[i].download(b.k, nm) for i in idx]
                out[b.k][nm] = block_rule(b, x, mask, idx, seed, draw + g, reach, passes, centre, amplitude)
    return out


def flat(groups):
    return tuple(nm for grp in groups for nm in ((grp,) if isinstance(grp, str) else grp))


def assemble(e, arrays, fill=np.nan):
    """One global (nx, ny) array from per-block arrays {k: array}: each block's interior."""
    out = np.full((e.basin.nx, e.basin.ny), fill, dtype=arrays[0].dtype)
    for b in e.members[0].blocks:
        a = arrays[b.k]
        out[b.nx_start - 1:b.nx_end, b.ny_start - 1:b.ny_end] = a[b.nx_start - b.bnd_x1:b.nx_end - b.bnd_x1 + 1,
                                                                   b.ny_start - b.bnd_y1:b.ny_end - b.bnd_y1 + 1]
    return out
