#!/usr/bin/env python
"""The analysis of observations at their own times from the recorder's series on the device, against the host
route a user had for it and against the analysis-time entry it should cost the same as: one JSON line.

    python scripts/ens_fgat_bench.py [--members 8,32,64] [--obs 256:16,1024:256] [--window 12] [--radius 10]
                                     [--repeats 7] [--legs a,b,c]

The case is scripts/ens_obs_bench.py's: the Black Sea fixture's basin (tests/golden, one block), per member count M
in ONE process an OceanEnsemble of M members perturbed by per-member ssh patterns, after a 2-step call.  Per
"observations:stations" pair: that many stations at random interior positions (bilinear rows of ssh) recorded over
`window` steps (every = 1), the members completed; the observations name random stations at random times within
the window; a Gaspari-Cohn taper of `radius` points at the stations' anchors, STATE updated.  Alternating per repeat
after one untimed repeat of each, every leg timed from the call to the end of synchronize(), its results read back:

  a  assimilate_recorded(device=True): ocn_ens_assimilate_rec
  b  assimilate_recorded(device=False): series() down, ens_record_rule.interp, ens_local_rule.ensrf_obs_space,
     one local_update(STATE)
  c  assimilate_h(device=True) of the same rows (ocn_ens_assimilate_h: the members' equivalents at analysis time):
     the cost a should match, since only the prologue differs

Before anything is timed, from one saved state restored by upload in between:
  * sample_recorded() against ens_record_rule.interp(series()), bitwise: the rows routes a and b start from;
  * with every observation at the last record, a against c: hx, Y, Z, the vectors and every field of every member,
    bitwise;
  * a against b at the observations' own times: hx, the vectors and the fields, bitwise -- reported with the
    largest field difference, not required: beyond 5 members the host loop's np.sum leaves the order of its sums
    to numpy (OceanEnsemble.assimilate's docstring), so its last bits are its own;
  * a against b with that loop's sums in member order (ens_local_rule.ensrf_obs_space_ordered in b's place),
    bitwise.
Reported: median (min - max) in ms over the repeats, and a / b, a / c from the medians.
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
    ap.add_argument("--obs", default="256:16,1024:256")
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()
    legs_on = a.legs.split(",")

    import numpy as np

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import ens_obs_rule, ens_record_rule
    from ocean_model_arch_amd.ensemble import STATE, taper_table
    from tests import ens_obs_ref as O
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])

    def summary(ms, nd=4):
        return {"median_ms": round(statistics.median(ms), nd), "min_ms": round(min(ms), nd), "max_ms": round(max(ms), nd)}

    taper = taper_table(a.radius)
    out = {"bench": "ens_fgat", "case": a.case, "window": a.window, "repeats": a.repeats, "fields": list(STATE), "legs": legs_on,
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

        for pair in a.obs.split(","):
            nobs, nsta = (int(x) for x in pair.split(":"))
            rng = np.random.default_rng(1000 * M + nobs)
            xy = np.stack([rng.uniform(blk.nx_start, blk.nx_end, nsta), rng.uniform(blk.ny_start, blk.ny_end, nsta)], axis=1)
            stations = ens_obs_rule.bilinear("ssh", xy, shape=(b["nx"], b["ny"]))
            e.record(stations, every=1, max_records=a.window)
            e.step_record(a.window, 1.0, 1)
            e.complete()
            st += e.synchronize()
            if any(st):
                raise RuntimeError(f"member statuses {st}")
            info = e.record_info()
            rows = rng.integers(0, nsta, nobs)
            at = rng.uniform(1.0, float(a.window), nobs)
            at[0], at[-1] = 1.0, float(a.window)
            at_last = np.full(nobs, float(a.window))
            rows_op = ens_obs_rule.ObsOperator.from_rows([stations.row(int(r)) for r in rows], stations.anchors[rows])
            variances = np.full(nobs, 1e-4)   # (1 cm)^2
            res = {"members": M, "observations": nobs, "stations": nsta, "records": info["records"], "in_launch": info["in_launch"],
                   "array": list(shape), "update_path": "register" if M <= 32 else "lds"}

            def noisy(hx):
                return hx.mean(axis=1) + rng.normal(0.0, 0.01, nobs)

            # the routes against each other, bitwise, before anything is timed
            start = O.downloads(e, STATE, range(M))

            def restore():
                for nm in STATE:
                    for m, arr in zip(e.members, start[nm][0]):
                        m.upload(0, nm, arr)

            def fields_equal(x, y):
                return all(O.bits_equal(g, v) for nm in STATE for g, v in zip(x[nm][0], y[nm][0]))

            series = e.series()
            rec, wt = ens_record_rule.at_steps(at, 1, info["records"])
            hx_own = e.sample_recorded(rows, at)
            res["sample_bitwise_equal_to_interp"] = bool(O.bits_equal(hx_own, ens_record_rule.interp(series, rows, rec, wt)))
            values = noisy(e.sample_recorded(rows, at_last))
            ga = e.assimilate_recorded(rows, at_last, values, variances, taper, device=True)
            ya, fa = e.assimilate_results(("y", "z")), O.downloads(e, STATE, range(M))
            restore()
            gc = e.assimilate_h(rows_op, values, variances, taper, device=True)
            yc, fc = e.assimilate_results(("y", "z")), O.downloads(e, STATE, range(M))
            res["a_bitwise_equal_to_c_at_last_record"] = bool(
                not O.info_mismatches(ga, gc) and O.bits_equal(ya["y"], yc["y"]) and O.bits_equal(ya["z"], yc["z"])
                and ga["nonfinite"] == gc["nonfinite"] and fields_equal(fa, fc))
            values = noisy(hx_own)
            restore()
            ga = e.assimilate_recorded(rows, at, values, variances, taper, device=True)
            fa = O.downloads(e, STATE, range(M))
            restore()
            gb = e.assimilate_recorded(rows, at, values, variances, taper, device=False)
            fb = O.downloads(e, STATE, range(M))
            res["a_bitwise_equal_to_b"] = bool(not O.info_mismatches(ga, gb) and fields_equal(fa, fb))
            with np.errstate(all="ignore"):
                res["a_b_max_abs_field_difference"] = float(max(np.nanmax(np.abs(g - v)) for nm in STATE
                                                                for g, v in zip(fa[nm][0], fb[nm][0])))
            res["nonfinite"] = int(ga["nonfinite"])
            restore()
            Y, Z, go = O.ensrf_obs_space_ordered(ens_record_rule.interp(series, rows, rec, wt), stations.anchors[rows], values,
                                                 variances, taper)
            e.local_update(Y, Z, stations.anchors[rows], taper)
            res["a_bitwise_equal_to_b_with_ordered_sums"] = bool(not O.info_mismatches(ga, go)
                                                                 and fields_equal(fa, O.downloads(e, STATE, range(M))))
            restore()

            def leg_a():
                v = noisy(e.sample_recorded(rows, at))
                t0 = time.perf_counter()
                e.assimilate_recorded(rows, at, v, variances, taper, device=True)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def leg_b():
                v = noisy(e.sample_recorded(rows, at))
                t0 = time.perf_counter()
                e.assimilate_recorded(rows, at, v, variances, taper, device=False)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def leg_c():
                v = noisy(e.sample_h(rows_op))
                t0 = time.perf_counter()
                e.assimilate_h(rows_op, v, variances, taper, device=True)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            legs = {k: f for k, f in (("a", leg_a), ("b", leg_b), ("c", leg_c)) if k in legs_on}
            times = {k: [] for k in legs}
            for r in range(a.repeats + 1):   # (repeat 0 untimed)
                for k, leg in legs.items():
                    dt = leg()
                    if r:
                        times[k].append(dt)
            res["statuses_ok"] = not any(e.synchronize())
            for k, ts in times.items():
                res[k] = summary(ts)
            for k in ("b", "c"):
                if "a" in times and k in times:
                    res[f"a_over_{k}"] = round(statistics.median(times["a"]) / statistics.median(times[k]), 4)
            out["results"].append(res)
            restore()
            st = e.synchronize()
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
