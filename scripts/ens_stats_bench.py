#!/usr/bin/env python
"""Ensemble statistics on the device against downloads of every member: one JSON line.

    python scripts/ens_stats_bench.py [--members 8,32,64] [--steps 100] [--repeats 5] [--box N]

The basin is the Black Sea fixture's (tests/golden, one block) or, with --box N, the N x N closed box.
Per member count M, in ONE process: an OceanEnsemble of M members after a 2-step and a `steps`-step call,
completed.  Then, alternating per repeat after one untimed repeat of each:

  device  stats("ssh", mean + spread + min + max) -- one launch and one download per statistic
  extrema extrema("ssh") -- two launches, 32 bytes per member back (extrema_back_to_back: the same call
          repeated with no other leg between, extrema_kernels: its span between two events on the stream)
  host    what a host can do without them: download("ssh") of every member, then the numpy restatement
          of the same definitions (tests/ens_stats_ref.py) -- host_download is the downloads alone

and the k_ens_stats launch alone between two HIP events on the ensemble's stream (members complete, so
nothing else is enqueued), as bytes moved per second: (M reads + 4 writes) x 8 B per point of the array.
The device results are compared bitwise with the host route's before anything is timed.
Reported: median (min - max) in ms over the repeats.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WHAT = ("mean", "spread", "min", "max")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="8,32,64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--box", type=int, default=0)
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()

    import torch

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import _lib
    from tests import ens_stats_ref as R

    if a.box:
        basin, sw, par, case = amd.box_config(a.box), amd.SWConfig(), amd.ParallelConfig(1, 1), f"box{a.box}"
    else:
        from tests.golden import cases
        c = cases.load_e2e(a.case)
        b = c["basin"]
        basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                                curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
        sw, par, case = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"]), a.case

    def summary(ts):
        ms = [1e3 * t for t in ts]
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    out = {"bench": "ens_stats", "case": case, "steps": a.steps, "repeats": a.repeats, "statistics": list(WHAT),
           "build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        e.step(2, 1.0, 1)
        st = e.synchronize()
        e.step(a.steps, 1.0, 1)
        e.complete()
        st += e.synchronize()
        if any(st):
            raise RuntimeError(f"member statuses {st}")
        shape = e.members[0].blocks[0].shape
        points = shape[0] * shape[1]

        def device():
            t0 = time.perf_counter()
            got = e.stats("ssh", WHAT)
            return time.perf_counter() - t0, got

        def extrema():
            t0 = time.perf_counter()
            got = e.extrema("ssh")
            return time.perf_counter() - t0, got

        def host():
            t0 = time.perf_counter()
            fields = [m.download(0, "ssh") for m in e.members]
            t1 = time.perf_counter()
            got = R.stats(fields, WHAT)
            return time.perf_counter() - t0, (t1 - t0, got)

        same = all(R.bits_equal(device()[1][nm], host()[1][1][nm]) for nm in WHAT)
        legs = {"device": device, "extrema": extrema, "host": host}
        times = {k: [] for k in legs}
        times["host_download"] = []
        for r in range(a.repeats + 1):   # (repeat 0 untimed)
            for k, leg in legs.items():
                dt, x = leg()
                if r:
                    times[k].append(dt)
                    if k == "host":
                        times["host_download"].append(x[0])
        # the launch alone, between events on the ensemble's stream
        s = torch.cuda.ExternalStream(lib_stream(e))
        bits = sum(_lib.ENS_STATS[n] for n in WHAT)
        kms = []
        for r in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            _lib.check(amd.lib().ocn_ens_stats(e.ens, 0, _lib.FIELD_ID["ssh"], None, bits), "ocn_ens_stats")
            e1.record(s)
            e1.synchronize()
            if r:
                kms.append(e0.elapsed_time(e1))
        kmed = statistics.median(kms)
        xhost = []   # (the host's time for the same calls: extrema back to back, no other leg between)
        xms = []   # ocn_ens_extrema's two launches likewise (the entry's own copies and wait lie outside the events' span)
        for r in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            t0 = time.perf_counter()
            e.extrema("ssh")
            dt = time.perf_counter() - t0
            e1.record(s)
            e1.synchronize()
            if r:
                xms.append(e0.elapsed_time(e1))
                xhost.append(dt)
        nbytes = (M * (2 if M > 32 else 1) + len(WHAT)) * 8 * points   # (beyond 32 members the variance reads them again)
        res = {"members": M, "array": list(shape), "bitwise_equal_to_host_route": bool(same)}
        for k, ts in times.items():
            res[k] = summary(ts)
        res["host_over_device"] = round(res["host"]["median_ms"] / res["device"]["median_ms"], 2)
        res["kernel"] = {"median_ms": round(kmed, 5), "min_ms": round(min(kms), 5), "max_ms": round(max(kms), 5),
                         "bytes": nbytes, "tb_per_s": round(nbytes / (kmed * 1e-3) / 1e12, 3)}
        res["extrema_kernels"] = {"median_ms": round(statistics.median(xms), 5), "min_ms": round(min(xms), 5),
                                  "max_ms": round(max(xms), 5)}
        res["extrema_back_to_back"] = summary(xhost)
        out["results"].append(res)
        e.close()
    print(json.dumps(out))


def lib_stream(e):
    """The ensemble's shared stream (every member's ocn_ctx_stream) as an integer handle."""
    import ocean_model_arch_amd as amd
    return int(amd.lib().ocn_ctx_stream(e.members[0].ctx))


if __name__ == "__main__":
    main()
