#!/usr/bin/env python
"""Correlated perturbations on the device against numpy draws applied by download / upload: one JSON line.

    python scripts/ens_perturb_bench.py [--members 8,32,64] [--repeats 3] [--calls 20] [--rounds 3]

The basin is the Black Sea fixture's (tests/golden, one block).  The measurement runs in fresh child processes,
`rounds` of them one after another (--child: one such process); the parent opens no device and reports every
round's medians.  Per member count M, in one child: an OceanEnsemble of M members after init() alone -- the
members identical, which is the state perturb() is for -- and OceanEnsemble.perturb with its default arguments
(reach 4, passes 2, the six state fields in three draws under their masks, centred).  First the result is
compared bitwise, field by field, with the restatement (tests/ens_perturb_ref.py) over the members' downloads.
Then

  kernel   per call, between two HIP events on the ensemble's stream, after warm-up calls: perturb() as above
           (three launches of k_ens_noise, six of k_ens_perturb_apply) and perturb() of the same six fields in ONE
           draw (one noise launch, six applications); median (min - max) over `calls` calls.  noise_share: the
           noise launches' part of the default call, estimated from the difference of the two -- two noise
           launches -- as 3/2 of it over the default call's time
  device   perturb(), then synchronize, by the host clock
  host     the route it replaces: the numpy restatement's draw for every member and field, applied by
           download and upload of the same fields; host_copies: its downloads and uploads alone

device and host alternate per repeat after one untimed repeat of each; median (min - max) in ms.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def child(a):
    import torch

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd.ensemble import STATE, STATE_GROUPS
    from tests import ens_perturb_ref as R
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])
    amp = 0.01

    def summary(ts, nd=3):
        ms = [1e3 * t for t in ts]
        return {"median_ms": round(statistics.median(ms), nd), "min_ms": round(min(ms), nd), "max_ms": round(max(ms), nd)}

    out = {"bench": "ens_perturb", "case": a.case, "repeats": a.repeats, "calls": a.calls, "groups": [list(g) for g in STATE_GROUPS],
           "reach": 4, "passes": 2, "lib": os.path.relpath(amd._lib.LIB_PATH, REPO), "build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        idx = list(range(M))
        shape = e.members[0].blocks[0].shape

        def downloads():
            return {0: {nm: [m.download(0, nm) for m in e.members] for nm in STATE}}

        # the device against the restatement, bitwise, before anything is timed
        before = downloads()
        e.perturb(amp, seed=1)
        after = downloads()
        want = R.expected(e, STATE_GROUPS, idx, seed=1, amplitude=amp, before=before)
        same = all(R.bits_equal(g, v) for nm in STATE for g, v in zip(after[0][nm], want[0][nm]))
        res = {"members": M, "array": list(shape), "bitwise_equal_to_restatement": bool(same),
               "points_changed_of_ssh": int((after[0]["ssh"][0] != before[0]["ssh"][0]).sum())}

        # the launches alone, between events on the ensemble's stream
        s = torch.cuda.ExternalStream(int(amd.lib().ocn_ctx_stream(e.members[0].ctx)))

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            e1.synchronize()
            return 1e-3 * e0.elapsed_time(e1)

        k3, k1 = [], []
        for r in range(a.calls + 3):   # (three warm-up calls of each)
            t3 = timed(lambda: e.perturb(amp, seed=2 + r))
            t1 = timed(lambda: e.perturb(amp, names=(STATE,), seed=2 + r))
            if r >= 3:
                k3.append(t3)
                k1.append(t1)
        res["kernel_default"] = dict(summary(k3, 5), launches=9)
        res["kernel_one_draw"] = dict(summary(k1, 5), launches=7)
        res["noise_share"] = round(1.5 * (statistics.median(k3) - statistics.median(k1)) / statistics.median(k3), 3)

        def device(r):
            e.synchronize()
            t0 = time.perf_counter()
            e.perturb(amp, seed=100 + r)
            e.synchronize()
            return time.perf_counter() - t0, None

        def host(r):
            e.synchronize()
            t0 = time.perf_counter()
            x = downloads()
            t1 = time.perf_counter()
            new = R.expected(e, STATE_GROUPS, idx, seed=100 + r, amplitude=amp, before=x)
            t2 = time.perf_counter()
            for nm in STATE:
                for m, f in zip(e.members, new[0][nm]):
                    m.upload(0, nm, f)
            t3 = time.perf_counter()
            return t3 - t0, (t1 - t0) + (t3 - t2)

        times = {"device": [], "host": [], "host_copies": []}
        for r in range(a.repeats + 1):   # (repeat 0 untimed)
            for k, leg in (("device", device), ("host", host)):
                dt, x = leg(r)
                if r:
                    times[k].append(dt)
                    if k == "host":
                        times["host_copies"].append(x)
        for k, ts in times.items():
            res[k] = summary(ts)
        res["host_over_device"] = round(res["host"]["median_ms"] / res["device"]["median_ms"], 1)
        res["statuses_ok"] = not any(e.synchronize())
        out["results"].append(res)
        print(f"[ens_perturb_bench] {M} members done", file=sys.stderr, flush=True)
        e.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="8,32,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--case", default="bs_b1x1_s60")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for r in range(a.rounds):
        txt = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", "--members", a.members, "--repeats",
                                       str(a.repeats), "--calls", str(a.calls), "--case", a.case], text=True, timeout=900)
        runs.append(json.loads(txt.strip().splitlines()[-1]))
        print(f"[ens_perturb_bench] round {r} done", file=sys.stderr, flush=True)
    out = {k: v for k, v in runs[0].items() if k != "results"}
    out["rounds"] = a.rounds
    out["results"] = []
    for i, first in enumerate(runs[0]["results"]):
        rows = [run["results"][i] for run in runs]
        res = {"members": first["members"], "array": first["array"],
               "bitwise_equal_to_restatement": all(x["bitwise_equal_to_restatement"] for x in rows),
               "statuses_ok": all(x["statuses_ok"] for x in rows), "points_changed_of_ssh": first["points_changed_of_ssh"]}
        for key in ("kernel_default", "kernel_one_draw", "device", "host", "host_copies"):
            res[key + "_median_ms"] = [x[key]["median_ms"] for x in rows]
        res["noise_share"] = [x["noise_share"] for x in rows]
        res["host_over_device"] = [x["host_over_device"] for x in rows]
        out["results"].append(res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
