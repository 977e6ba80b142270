#!/usr/bin/env python
"""The device analysis with a sparse linear observation operator against the grid-point analysis and against
the host route a user had for off-grid observations: one JSON line.

    python scripts/ens_obs_bench.py [--members 8,32,64] [--obs 256,1024] [--radius 10] [--steps 20] [--repeats 7]
                                    [--legs a,b,c,d] [--baseline parent.json]

The case is scripts/ens_assim_bench.py's: the Black Sea fixture's basin (tests/golden, one block), per member
count M in ONE process an OceanEnsemble of M members perturbed by per-member ssh patterns, after a 2-step and
a `steps`-step call, completed; per observation count that many ssh observations at random interior positions,
a Gaspari-Cohn taper of `radius` points, STATE updated.  Alternating per repeat after one untimed repeat of
each, every leg timed from the call to the end of synchronize(), its results read back:

  a  assimilate("ssh", ij, device=True): the positions rounded to grid points (ocn_ens_assimilate).  With
     --legs a the script needs nothing of the operator's, so it also runs in a checkout of the parent commit;
     --baseline embeds that run's JSON line under "baseline"
  b  assimilate_h(points("ssh", ij), device=True): the same observations as one-term unit rows
  c  assimilate_h(bilinear("ssh", xy), device=True): 4-term rows at the fractional positions
  d  the host route for c: every member's ssh downloaded, bilinear interpolation in numpy,
     ens_local_rule.ensrf_obs_space at the anchors, one local_update(STATE)

Before anything is timed, c is compared bitwise with the restatement (tests/ens_obs_ref.py) on the members'
downloads.  Reported: median (min - max) in ms over the repeats.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="8,32,64")
    ap.add_argument("--obs", default="256,1024")
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()
    legs_on = a.legs.split(",")

    import numpy as np

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import ens_local_rule
    from ocean_model_arch_amd.ensemble import STATE, taper_table
    from tests.golden import cases
    if set(legs_on) - {"a"}:
        from ocean_model_arch_amd import ens_obs_rule
        from tests import ens_obs_ref as O

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])

    def summary(ms, nd=4):
        return {"median_ms": round(statistics.median(ms), nd), "min_ms": round(min(ms), nd), "max_ms": round(max(ms), nd)}

    taper = taper_table(a.radius)
    out = {"bench": "ens_obs", "case": a.case, "steps": a.steps, "repeats": a.repeats, "fields": list(STATE), "legs": legs_on,
           "radius": a.radius, "ntaper": len(taper), "ocn_build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        blk = e.members[0].blocks[0]
        shape = blk.shape
        gi, gj = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        for i, m in enumerate(e.members):   # smooth ssh patterns of a few centimetres, one per member
            ph = 0.7 * i
            bump = 0.02 * np.sin(gi / 17.0 + ph) * np.cos(gj / 11.0 - 0.5 * ph) + 0.01 * np.sin((gi + gj) / 29.0 + 2.0 * ph)
            m.upload(0, "ssh", np.asfortranarray(m.download(0, "ssh") + bump))
        e.step(2, 1.0, 1)
        st = e.synchronize()
        e.step(a.steps, 1.0, 1)
        e.complete()
        st += e.synchronize()
        if any(st):
            raise RuntimeError(f"member statuses {st}")

        for nobs in [int(x) for x in a.obs.split(",")]:
            rng = np.random.default_rng(1000 * M + nobs)
            xy = np.stack([rng.uniform(blk.nx_start, blk.nx_end, nobs), rng.uniform(blk.ny_start, blk.ny_end, nobs)], axis=1)
            ij = np.floor(xy + 0.5).astype(np.int64)
            pts = [(0, int(i), int(j)) for i, j in ij]
            variances = np.full(nobs, 1e-4)   # (1 cm)^2
            res = {"members": M, "observations": nobs, "array": list(shape), "update_path": "register" if M <= 32 else "lds"}

            def noisy(hx):
                return hx.mean(axis=1) + rng.normal(0.0, 0.01, nobs)

            if set(legs_on) - {"a"}:
                unit = ens_obs_rule.points("ssh", ij)
                bil = ens_obs_rule.bilinear("ssh", xy, shape=(b["nx"], b["ny"]))
                res["terms"] = int(bil.start[-1])
                # the device against the restatement, bitwise, before anything is timed
                before = O.downloads(e, STATE, range(M))
                values = noisy(e.sample_h(bil))
                got = e.assimilate_h(bil, values, variances, taper, device=True)
                yz = e.assimilate_results(("y", "z"))
                after = O.downloads(e, STATE, range(M))
                _, Y, Z, ref, want = O.analysis(bil, before, e.members[0].blocks, e.block_of, values, variances, taper, STATE)
                res["bitwise_equal_to_restatement"] = bool(
                    not O.info_mismatches(got, ref) and O.bits_equal(yz["y"], Y) and O.bits_equal(yz["z"], Z)
                    and all(O.bits_equal(g, v) for nm in STATE for g, v in zip(after[nm][0], want[nm][0])))
                res["nonfinite"] = int(got["nonfinite"])
                # d's interpolation: the four corners and weights of every row as arrays (rows of fewer terms padded
                # with weight 0 at the first corner)
                ci, cj, cw = (np.zeros((nobs, 4), dtype=t) for t in (np.int64, np.int64, np.float64))
                for j in range(nobs):
                    row = bil.row(j)
                    for t in range(4):
                        _, i_, j_, w_ = row[t] if t < len(row) else (None, row[0][1], row[0][2], 0.0)
                        ci[j, t], cj[j, t], cw[j, t] = i_ - blk.bnd_x1, j_ - blk.bnd_y1, w_

            def leg_a():
                v = noisy(e.sample("ssh", pts))
                t0 = time.perf_counter()
                e.assimilate("ssh", ij, v, variances, taper, device=True)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def leg_b():
                v = noisy(e.sample_h(unit))
                t0 = time.perf_counter()
                e.assimilate_h(unit, v, variances, taper, device=True)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def leg_c():
                v = noisy(e.sample_h(bil))
                t0 = time.perf_counter()
                e.assimilate_h(bil, v, variances, taper, device=True)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def leg_d():
                v = noisy(e.sample_h(bil))
                t0 = time.perf_counter()
                hx = np.stack([(m.download(0, "ssh")[ci, cj] * cw).sum(axis=1) for m in e.members], axis=1)
                Y, Z, _ = ens_local_rule.ensrf_obs_space(hx, bil.anchors, v, variances, taper)
                e.local_update(Y, Z, bil.anchors, taper)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            legs = {k: f for k, f in (("a", leg_a), ("b", leg_b), ("c", leg_c), ("d", leg_d)) if k in legs_on}
            times = {k: [] for k in legs}
            for r in range(a.repeats + 1):   # (repeat 0 untimed)
                for k, leg in legs.items():
                    dt = leg()
                    if r:
                        times[k].append(dt)
            res["statuses_ok"] = not any(e.synchronize())
            for k, ts in times.items():
                res[k] = summary(ts)
            out["results"].append(res)
        e.close()
    if a.baseline:
        with open(a.baseline) as f:
            out["baseline"] = json.loads(f.read().strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
