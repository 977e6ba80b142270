#!/usr/bin/env python
"""ocn_ens_assimilate at the sizes its few-seconds tests leave out, each once against the restatement: one JSON
line.

    python scripts/ens_assim_large.py [--obs 8192] [--members 96,128]

On tests/shapes.py Shape(61, 9) with class-noise members after calls [2, 3]: `obs` observations (the entry's
limit) with 8 members, and 64 observations with each of the large member counts (beyond 64 members the update
runs its LDS path, the observation-space kernel its one path).  Every comparison is bitwise: the rows, the
vectors and the updated fields against tests/ens_assim_ref.py on the members' own sample() and downloads.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=8192)
    ap.add_argument("--members", default="96,128")
    a = ap.parse_args()

    import numpy as np

    import ocean_model_arch_amd as amd
    from tests import ens_assim_ref as A
    from tests import shapes as S
    from tests.test_gpu_ensemble import _start

    shape, names = S.Shape(61, 9), ("ssh", "ubrtr")
    taper = A.taper_table(6.0)
    out = {"bench": "ens_assim_large", "shape": "Shape(61, 9)", "fields": list(names), "radius": 6.0,
           "ocn_build_id": amd.build_id(), "results": []}
    for M, nobs in [(8, a.obs)] + [(int(m), 64) for m in a.members.split(",") if m]:
        e = _start(amd, shape, ["noise"] * M)
        try:
            e.step(2)
            st = e.synchronize()
            e.step(3)
            e.complete()
            st += e.synchronize()
            blk = e.members[0].blocks[0]
            rng = np.random.default_rng(M + nobs)
            ij = np.stack([rng.integers(1, 66, nobs), rng.integers(1, 14, nobs)], axis=1)
            before = {nm: [m.download(0, nm) for m in e.members] for nm in names}
            hx = e.sample("ssh", [(0, int(i), int(j)) for i, j in ij])
            values = hx.mean(axis=1) + rng.uniform(-0.1, 0.1, nobs)
            variances = np.full(nobs, 0.01) + hx.var(axis=1, ddof=1) * 0.5
            t0 = time.perf_counter()
            got = e.assimilate("ssh", ij, values, variances, taper, names=names, device=True)
            ms = 1e3 * (time.perf_counter() - t0)
            yz = e.assimilate_results(("y", "z"))
            after = {nm: [m.download(0, nm) for m in e.members] for nm in names}
            st += e.synchronize()
            Y, Z, ref = A.ensrf_obs_space_ordered(hx, ij, values, variances, taper)
            rows = not A.info_mismatches(got, ref) and A.bits_equal(yz["y"], Y) and A.bits_equal(yz["z"], Z)
            fields = all(A.bits_equal(g, v) for nm in names
                         for g, v in zip(after[nm], A.block_update(before[nm], blk, ij[:, 0], ij[:, 1], Y, Z, taper)))
            out["results"].append({"members": M, "observations": nobs, "rows_bitwise_equal": bool(rows),
                                   "fields_bitwise_equal": bool(fields), "nonfinite": int(got["nonfinite"]),
                                   "statuses_ok": not any(st), "assimilate_ms": round(ms, 3)})
        finally:
            e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
