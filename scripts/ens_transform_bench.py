#!/usr/bin/env python
"""Recombining an ensemble on the device against download / numpy / upload of every member: one JSON line.

    python scripts/ens_transform_bench.py [--members 8,32,64] [--steps 20] [--repeats 5] [--box N]

The basin is the Black Sea fixture's (tests/golden, one block) or, with --box N, the N x N closed box.
Per member count M, in ONE process: an OceanEnsemble of M members after a 2-step and a `steps`-step call,
completed.  The weights are a random orthogonal M x M matrix (dense; the state keeps its size however
often it is applied).  First the device's transform(STATE) is compared bitwise, field by field, with the
ordered restatement (tests/ens_transform_ref.py) over the members' downloads.  Then, alternating per repeat
after one untimed repeat of each:

  device  transform(STATE), then synchronize
  host    the only route without it: download the six fields of every member, recombine them as X @ W in
          numpy (the fastest host arithmetic, not the ordered restatement), upload them -- host_copies is
          the downloads and uploads alone
  sample  sample("ssh") at 16 stations against the same 16 points read out of download("ssh") of every member

(device_back_to_back, sample_back_to_back: the same calls repeated with no other leg between),
and the transform's launches alone between two HIP events on the ensemble's stream (members complete; the
copy of the weights lies inside the span), with
  bytes  (M read + M written) x 8 B per point and field; beyond 32 members (M ceil(M / 8) + 3 M) x 8 B:
         every pass of 8 columns reads the M inputs again, the results are written to the staging arrays,
         read from them and written to the members
  flops  2 M^2 per point and field (a multiply and an add per term, not fused)
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

STATIONS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="8,32,64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--box", type=int, default=0)
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()

    import numpy as np
    import torch

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd.ensemble import STATE
    from tests import ens_transform_ref as T

    if a.box:
        basin, sw, par, case = amd.box_config(a.box), amd.SWConfig(), amd.ParallelConfig(1, 1), f"box{a.box}"
    else:
        from tests.golden import cases
        c = cases.load_e2e(a.case)
        b = c["basin"]
        basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                                curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
        sw, par, case = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"]), a.case

    def summary(ts, nd=4):
        ms = [1e3 * t for t in ts]
        return {"median_ms": round(statistics.median(ms), nd), "min_ms": round(min(ms), nd), "max_ms": round(max(ms), nd)}

    out = {"bench": "ens_transform", "case": case, "steps": a.steps, "repeats": a.repeats, "fields": list(STATE),
           "stations": STATIONS, "build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        e.step(2, 1.0, 1)
        st = e.synchronize()
        e.step(a.steps, 1.0, 1)
        e.complete()
        st += e.synchronize()
        if any(st):
            raise RuntimeError(f"member statuses {st}")
        blk = e.members[0].blocks[0]
        shape = blk.shape
        points = shape[0] * shape[1]
        w = np.ascontiguousarray(np.linalg.qr(np.random.default_rng(M).standard_normal((M, M)))[0])
        rng = np.random.default_rng(1)
        pts = [(0, int(rng.integers(blk.nx_start, blk.nx_end + 1)), int(rng.integers(blk.ny_start, blk.ny_end + 1)))
               for _ in range(STATIONS)]

        def downloads():
            return {nm: [m.download(0, nm) for m in e.members] for nm in STATE}

        # the device against the ordered restatement, bitwise, before anything is timed
        before = downloads()
        e.transform(w)
        after = downloads()
        same = all(T.bits_equal(g, v) for nm in STATE for g, v in zip(after[nm], T.transform(before[nm], w)))

        def device():
            t0 = time.perf_counter()
            e.transform(w)
            e.synchronize()
            return time.perf_counter() - t0, None

        def host():
            t0 = time.perf_counter()
            x = downloads()
            t1 = time.perf_counter()
            new = {nm: np.stack([f.ravel(order="F") for f in x[nm]], axis=1) @ w for nm in STATE}
            t2 = time.perf_counter()
            for nm in STATE:
                for i, m in enumerate(e.members):
                    m.upload(0, nm, np.asfortranarray(new[nm][:, i].reshape(shape, order="F")))
            t3 = time.perf_counter()
            return t3 - t0, (t1 - t0) + (t3 - t2)

        def sample():
            t0 = time.perf_counter()
            got = e.sample("ssh", pts)
            return time.perf_counter() - t0, got

        def sample_host():
            t0 = time.perf_counter()
            d = [m.download(0, "ssh") for m in e.members]
            got = np.array([[f[i - blk.bnd_x1, j - blk.bnd_y1] for f in d] for (_, i, j) in pts])
            return time.perf_counter() - t0, got

        sample_same = T.bits_equal(sample()[1], sample_host()[1])
        legs = {"device": device, "host": host, "sample": sample, "sample_host": sample_host}
        times = {k: [] for k in legs}
        times["host_copies"] = []
        for r in range(a.repeats + 1):   # (repeat 0 untimed)
            for k, leg in legs.items():
                dt, x = leg()
                if r:
                    times[k].append(dt)
                    if k == "host":
                        times["host_copies"].append(x)
        # the two device legs again with no other leg between (the first library call after another leg's
        # pageable copies pays for them on the host, as DESIGN section 7 found for the extrema)
        for k in ("device", "sample"):
            times[k + "_back_to_back"] = [legs[k]()[0] for r in range(a.repeats + 1)][1:]
        # the launches alone, between events on the ensemble's stream
        s = torch.cuda.ExternalStream(int(amd.lib().ocn_ctx_stream(e.members[0].ctx)))
        kms = []
        for r in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            e.transform(w)
            e1.record(s)
            e1.synchronize()
            if r:
                kms.append(e0.elapsed_time(e1))
        kmed = statistics.median(kms)
        per_point = (2 * M if M <= 32 else M * ((M + 7) // 8) + 3 * M) * 8
        nbytes, flops = per_point * points * len(STATE), 2 * M * M * points * len(STATE)
        res = {"members": M, "array": list(shape), "path": "register" if M <= 32 else "staging",
               "bitwise_equal_to_restatement": bool(same), "sample_bitwise_equal_to_downloads": bool(sample_same)}
        for k, ts in times.items():
            res[k] = summary(ts)
        res["host_over_device"] = round(res["host"]["median_ms"] / res["device"]["median_ms"], 2)
        res["host_copies_over_device"] = round(res["host_copies"]["median_ms"] / res["device"]["median_ms"], 2)
        res["sample_host_over_sample"] = round(res["sample_host"]["median_ms"] / res["sample"]["median_ms"], 2)
        res["kernel"] = {"median_ms": round(kmed, 5), "min_ms": round(min(kms), 5), "max_ms": round(max(kms), 5),
                         "launches": len(STATE) * (1 if M <= 32 else 2), "bytes": nbytes, "flops": flops,
                         "tb_per_s": round(nbytes / (kmed * 1e-3) / 1e12, 3),
                         "tflop_per_s": round(flops / (kmed * 1e-3) / 1e12, 3)}
        out["results"].append(res)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
