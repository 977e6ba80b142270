#!/usr/bin/env python
"""Forcing, station records and the peak map in one launch against the routes around it: one JSON line.

    python scripts/ens_run_bench.py [--members 8,32,64] [--steps 98] [--d-steps 14] [--every 2] [--stations 64]
                                    [--repeats 5] [--legs a,b,c,d]

The case is the Black Sea fixture's basin (tests/golden, one block); per member count M in ONE process an
OceanEnsemble of M members with a storm per member (scripts/ens_forcing_bench.py's storms), `stations` unit rows of
ssh on sea points spread over the basin, recorded every `every` steps, and the peaks (max and min) of ssh.  Every
timed call follows an untimed 2-step call and a synchronize() (an open sequence) and is timed from the call to the
end of synchronize(); alternating per repeat after one untimed repeat of each:

  a  step_forced(steps) with a peak active and no recorder: the best there was for two of the three products
  b  run(steps) in the launch with all three (the three infos are asserted to show the in-launch route)
  c  run(steps) with set_run_in_launch(False): the chunked route
  d  the only composition of all three without run(): per step step_forced(1) with the peak active, then on a due
     step sample_h -- over --d-steps steps, scaled to `steps`

Before anything is timed, per member count, the series and P and S after 2 + 6 steps by b, c and d from identically
started ensembles are compared bitwise, every member.
Reported: median (min - max) in ms per member-step over the repeats, and b/a, c/b, d/b of the medians.
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
    ap.add_argument("--steps", type=int, default=98)
    ap.add_argument("--d-steps", type=int, default=14)
    ap.add_argument("--every", type=int, default=2)
    ap.add_argument("--stations", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()
    legs_on = a.legs.split(",")

    import numpy as np

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import ens_forcing_rule as FR
    from ocean_model_arch_amd import ens_obs_rule
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])
    tau = 1.0
    # the stations: sea points of the interior, spread evenly over their list (1-based global indices)
    sea = np.argwhere(np.asarray(c["mask"])[2:-2, 2:-2] == 0) + 3
    op = ens_obs_rule.points("ssh", sea[(np.arange(a.stations) * len(sea)) // a.stations])

    def storm(i):
        cs, sn = FR.inflow(20.0)
        return FR.Storm(x0=0.2 * b["nx"] + 3.1 * (i % 16), y0=0.5 * b["ny"] + 1.7 * (i % 11) - 8.0, cx=0.0025, cy=0.0007 * (i % 5 - 2),
                        radius=1.0e5 + 2.0e3 * (i % 9), vmax=30.0 + (i % 7), dp=3000.0 + 50.0 * (i % 13), cos_in=cs, sin_in=sn)

    def fresh(M):
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        e.set_storms([storm(i) for i in range(M)], FR.ForcingModel())
        e.step(2, tau, 1)
        if any(e.synchronize()):
            raise RuntimeError("member statuses after the first call")
        return e

    def composed(e, t0, steps, counted=0):
        """leg d: step_forced(1) with the peak active, then sample_h on a due step; the records."""
        recs = []
        for s in range(steps):
            e.step_forced(1, tau, t0 + s * tau)
            if (counted + s + 1) % a.every == 0:
                recs.append(e.sample_h(op))
        return recs

    def peaks_of(e, M):
        return [[x.tobytes(order="F") for w in ("max", "min") for x in e.peak(i, 0, w)] for i in range(M)]

    def routes(e, n):
        """(records, peak steps, forcing) a call of n steps from a fresh recorder and peak shows in the launch."""
        return e.record_info()["in_launch"], e.peak_info()["in_launch"], e.forcing_info()["in_launch"]

    def summary(ms, per):
        return {"median_ms": round(statistics.median(ms) / per, 6), "min_ms": round(min(ms) / per, 6),
                "max_ms": round(max(ms) / per, 6)}

    out = {"bench": "ens_run", "case": a.case, "steps": a.steps, "d_steps": a.d_steps, "every": a.every,
           "stations": a.stations, "repeats": a.repeats, "legs": legs_on, "unit": "ms per member-step",
           "ocn_build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        k, got = 6, {}
        for leg in "bcd":
            f = fresh(M)
            f.peak_begin("ssh", ("max", "min"))
            if leg == "d":
                ser = np.array(composed(f, 0.0, k))
            else:
                f.set_run_in_launch(leg == "b")
                f.record(op, every=a.every, max_records=k // a.every + 1)
                f.run(k, tau, 0.0)
                want = ((k - 1) // a.every, k - 1, True) if leg == "b" else (0, 0, False)
                if routes(f, k) != want:
                    raise RuntimeError(f"leg {leg}: routes {routes(f, k)}, not {want}")
                ser = f.series()
            got[leg] = (ser.tobytes(), peaks_of(f, M))
            f.close()
        if not (got["b"] == got["c"] == got["d"]):
            raise RuntimeError(f"{M} members: the series or the peaks of legs b, c and d differ")

        e = fresh(M)
        clock = [0.0]
        res = {"members": M, "array": list(e.members[0].blocks[0].shape), "products_bitwise_equal_b_c_d": True}

        def opened():   # (a plain call: a forced call runs in the launch only on sequences one has opened)
            e.step(2, tau, 1)
            e.synchronize()

        def timed(f):
            t0 = time.perf_counter()
            f()
            e.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        def stepped(leg):
            opened()
            e.set_run_in_launch(leg != "c")
            e.peak_begin("ssh", ("max", "min"))
            if leg != "a":
                e.record(op, every=a.every, max_records=a.steps // a.every + 1)
            call = (lambda: e.step_forced(a.steps, tau, clock[0])) if leg == "a" else (lambda: e.run(a.steps, tau, clock[0]))
            dt = timed(call)
            clock[0] += a.steps * tau
            want = {"a": a.steps - 1, "b": a.steps - 1, "c": 0}[leg]
            if e.peak_info()["in_launch"] != want or bool(e.forcing_info()["in_launch"]) != (leg != "c"):
                raise RuntimeError(f"leg {leg}: peak in_launch {e.peak_info()['in_launch']}, forcing {e.forcing_info()}")
            if leg != "a":
                if e.record_info()["in_launch"] != ((a.steps - 1) // a.every if leg == "b" else 0):
                    raise RuntimeError(f"leg {leg}: records in_launch {e.record_info()['in_launch']}")
                e.record_end()
            e.peak_end()
            return dt

        def leg_d():
            opened()
            e.peak_begin("ssh", ("max", "min"))
            dt = timed(lambda: composed(e, clock[0], a.d_steps))
            clock[0] += a.d_steps * tau
            e.peak_end()
            return dt * a.steps / a.d_steps

        legs = {k_: f for k_, f in (("a", lambda: stepped("a")), ("b", lambda: stepped("b")), ("c", lambda: stepped("c")),
                                    ("d", leg_d)) if k_ in legs_on}
        times = {k_: [] for k_ in legs}
        for r in range(a.repeats + 1):   # (repeat 0 untimed)
            for k_, leg in legs.items():
                dt = leg()
                if r:
                    times[k_].append(dt)
        res["statuses_ok"] = not any(e.synchronize())
        for k_, ts in times.items():
            res[k_] = summary(ts, M * a.steps)
        for num, den in (("b", "a"), ("c", "b"), ("d", "b")):
            if num in res and den in res:
                res[f"{num}/{den}"] = round(res[num]["median_ms"] / res[den]["median_ms"], 3)
        out["results"].append(res)
        print(f"ens_run_bench: {M} members done", file=sys.stderr, flush=True)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
