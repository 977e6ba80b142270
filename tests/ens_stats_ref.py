"""The reference of the ensemble statistics (include/ocn_sw.h ocn_ens_stats, ocn_ens_extrema): plain
numpy restatements of the five definitions, array operations member by member in member order -- no
np.mean, np.var, np.min or np.max, whose summation order and NaN rules are their own.  Every operation
is one IEEE double operation per element, so the results are compared bitwise (bits_equal: the int64
views, and NaN at the same positions).

    MEAN    s = x0; s = s + x_i; mean = s / n
    VAR     d_i = x_i - mean; q = d0 d0; q = q + d_i d_i; var = q / (n - 1)
    SPREAD  sqrt(var)
    MIN     c = x0; c = x_i where (x_i < c or c != c)        MAX: the same with >
"""
import numpy as np

STATS = ("mean", "var", "spread", "min", "max")


def stats(fields, what=STATS):
    """{statistic: array} over `fields`, the members' arrays in member order (at least one; var and
    spread need two)."""
    x = [np.asarray(a, dtype=np.float64) for a in fields]
    n = len(x)
    assert n >= 1
    out = {}
    with np.errstate(all="ignore"):
        s = x[0].copy()
        for a in x[1:]:
            s = s + a
        mean = s / np.float64(n)
        if "mean" in what:
            out["mean"] = mean
        if "var" in what or "spread" in what:
            assert n >= 2
            d = x[0] - mean
            q = d * d
            for a in x[1:]:
                d = a - mean
                q = q + d * d
            var = q / np.float64(n - 1)
            if "var" in what:
                out["var"] = var
            if "spread" in what:
                out["spread"] = np.sqrt(var)
        for nm, less in (("min", True), ("max", False)):
            if nm not in what:
                continue
            c = x[0].copy()
            for a in x[1:]:
                take = ((a < c) if less else (a > c)) | (c != c)
                c = np.where(take, a, c)
            out[nm] = c
    return {k: np.asfortranarray(v) for k, v in out.items()}


def extrema(field_blocks, lu_blocks, interiors):
    """One member's {min, max, nonfinite, count} over the interior sea points of its blocks: field_blocks
    / lu_blocks the block arrays, interiors the (x0, x1, y0, y1) 0-based half-open interior of each."""
    mn, mx, nonfinite, count = np.inf, -np.inf, 0, 0
    for a, lu, (x0, x1, y0, y1) in zip(field_blocks, lu_blocks, interiors):
        v = np.asarray(a)[x0:x1, y0:y1][np.abs(np.asarray(lu)[x0:x1, y0:y1]) >= 0.5]
        count += int(v.size)
        fin = np.isfinite(v)
        nonfinite += int((~fin).sum())
        for t in v[fin]:
            if t < mn:
                mn = float(t)
            if t > mx:
                mx = float(t)
    return {"min": mn, "max": mx, "nonfinite": nonfinite, "count": count}


def bits_equal(a, b):
    """Same shape, NaN at the same positions, and the same 64 bits (the int64 views) everywhere else.
    A NaN's sign and payload are not compared: IEEE 754 leaves those of a generated NaN (Inf - Inf in
    the variance of a column with an Inf) to the implementation -- x86 makes 0xFFF8..., the GPU
    0x7FF8... -- so they are no property of the definitions."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~na]))
