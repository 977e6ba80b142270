#!/usr/bin/env python
"""Station time series recorded inside the multi-step launch against the routes around it: one JSON line.

    python scripts/ens_record_bench.py [--members 8,32,64] [--stations 16,256] [--steps 100] [--repeats 7]
                                       [--legs a,b,c,d,e] [--baseline parent.json]

The case is the Black Sea fixture's basin (tests/golden, one block); per member count M in ONE process an
OceanEnsemble of M members perturbed by per-member ssh patterns; per station count that many bilinear ssh
rows at random interior positions.  Every timed call is `steps` steps after an untimed 2-step call and a
synchronize() (an open sequence, the variant chosen on the host), timed from the call to the end of
synchronize(); alternating per repeat after one untimed repeat of each:

  a  step(steps): no recording.  With --legs a the script needs nothing of the recorder's, so it also runs in a
     checkout of the parent commit; --baseline embeds that run's JSON line under "baseline"
  b  step_record(steps), every = 1, in the launch (record_info()["in_launch"] is asserted)
  c  the same with every = 10
  d  the parent's only route: step(1) + sample_h(op), steps times
  e  step_record(steps), every = 1, with set_record_in_launch(False): the chunked route, no host wait

Before anything is timed, per member count, the series of b, d and e over 11 steps from identically started
ensembles are compared bitwise.  Reported: median (min - max) in ms per member-step over the repeats.
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
    ap.add_argument("--stations", default="16,256")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()
    legs_on = a.legs.split(",")
    recording = bool(set(legs_on) - {"a"})

    import numpy as np

    import ocean_model_arch_amd as amd
    from tests.golden import cases
    if recording:
        from ocean_model_arch_amd import ens_obs_rule

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])

    def fresh(M):
        """M members with smooth ssh patterns of a few centimetres, one per member, after a 2-step call."""
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        shape = e.members[0].blocks[0].shape
        gi, gj = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        for i, m in enumerate(e.members):
            ph = 0.7 * i
            bump = 0.02 * np.sin(gi / 17.0 + ph) * np.cos(gj / 11.0 - 0.5 * ph) + 0.01 * np.sin((gi + gj) / 29.0 + 2.0 * ph)
            ssh = np.asfortranarray(m.download(0, "ssh") + bump)
            m.upload(0, "ssh", ssh)
            m.upload(0, "sshn", ssh)   # (the pair stays equal: the calls flip roles and open their sequences)
        e.step(2, 1.0, 1)
        if any(e.synchronize()):
            raise RuntimeError("member statuses after the first call")
        return e

    def summary(ms, per):
        return {"median_ms": round(statistics.median(ms) / per, 6), "min_ms": round(min(ms) / per, 6),
                "max_ms": round(max(ms) / per, 6)}

    def bits(x):
        return np.ascontiguousarray(x).view(np.int64)

    out = {"bench": "ens_record", "case": a.case, "steps": a.steps, "repeats": a.repeats, "legs": legs_on,
           "unit": "ms per member-step", "ocn_build_id": amd.build_id(), "results": []}
    station_counts = [int(x) for x in a.stations.split(",")]
    for M in [int(x) for x in a.members.split(",")]:
        e = fresh(M)
        blk = e.members[0].blocks[0]
        ops = {}
        for nobs in station_counts if recording else []:
            rng = np.random.default_rng(1000 * M + nobs)
            xy = np.stack([rng.uniform(blk.nx_start, blk.nx_end, nobs), rng.uniform(blk.ny_start, blk.ny_end, nobs)], axis=1)
            ops[nobs] = ens_obs_rule.bilinear("ssh", xy, shape=(b["nx"], b["ny"]))
        equal = None
        if {"b", "d", "e"} <= set(legs_on):   # the three routes' series from identical starts, bitwise
            op, k = ops[max(ops)], 11
            runs = {}
            for leg in "bde":
                f = fresh(M)
                if leg == "d":
                    rows = []
                    for _ in range(k):
                        f.step(1, 1.0, 1)
                        rows.append(f.sample_h(op))
                    runs[leg] = np.stack(rows)
                else:
                    f.set_record_in_launch(leg == "b")
                    f.record(op, every=1, max_records=k).step_record(k, 1.0, 1)
                    runs[leg] = f.series()
                    want = k - 1 if leg == "b" else 0
                    if f.record_info()["in_launch"] != want:
                        raise RuntimeError(f"leg {leg}: in_launch {f.record_info()['in_launch']}, not {want}")
                if any(f.synchronize()):
                    raise RuntimeError(f"member statuses in leg {leg}'s comparison run")
                f.close()
            equal = bool((bits(runs["b"]) == bits(runs["d"])).all() and (bits(runs["b"]) == bits(runs["e"])).all())
            if not equal:
                raise RuntimeError("the series of legs b, d and e differ")

        for nobs in station_counts if recording else [0]:
            op = ops.get(nobs)
            res = {"members": M, "stations": nobs, "array": list(blk.shape)}
            if op is not None:
                res["terms"] = int(op.start[-1])
                res["series_bitwise_equal_b_d_e"] = equal

            def opened():
                e.step(2, 1.0, 1)
                e.synchronize()

            def timed(f):
                t0 = time.perf_counter()
                f()
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def leg_a():
                opened()
                return timed(lambda: e.step(a.steps, 1.0, 1))

            def recorded(every, in_launch):
                e.set_record_in_launch(in_launch)
                e.record(op, every=every, max_records=a.steps // every + 1)
                opened()
                dt = timed(lambda: e.step_record(a.steps, 1.0, 1))
                got, want = e.record_info()["in_launch"], (a.steps // every - (a.steps % every == 0)) if in_launch else 0
                if got != want:
                    raise RuntimeError(f"in_launch {got}, not {want} (every {every}, in the launch: {in_launch})")
                e.record_end()
                return dt

            def leg_d():
                opened()

                def run():
                    for _ in range(a.steps):
                        e.step(1, 1.0, 1)
                        e.sample_h(op)
                return timed(run)

            legs = {k: f for k, f in (("a", leg_a), ("b", lambda: recorded(1, True)), ("c", lambda: recorded(10, True)),
                                      ("d", leg_d), ("e", lambda: recorded(1, False))) if k in legs_on}
            times = {k: [] for k in legs}
            for r in range(a.repeats + 1):   # (repeat 0 untimed)
                for k, leg in legs.items():
                    dt = leg()
                    if r:
                        times[k].append(dt)
            res["statuses_ok"] = not any(e.synchronize())
            for k, ts in times.items():
                res[k] = summary(ts, M * a.steps)
            out["results"].append(res)
            print(f"ens_record_bench: {M} members, {nobs} stations done", file=sys.stderr, flush=True)
        e.close()
    if a.baseline:
        with open(a.baseline) as f:
            out["baseline"] = json.loads(f.read().strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
