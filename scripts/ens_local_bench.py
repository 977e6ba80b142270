#!/usr/bin/env python
"""A localized serial filter's analysis on the device against download / numpy / upload of every member: one
JSON line.

    python scripts/ens_local_bench.py [--members 8,32,64] [--obs 64,1024] [--radius 10] [--steps 20] [--repeats 3]

The basin is the Black Sea fixture's (tests/golden, one block).  Per member count M, in ONE process: an
OceanEnsemble of M members, perturbed by a per-member ssh offset pattern so that they differ, after a 2-step
and a `steps`-step call, completed.  Per observation count: that many ssh observations at random interior
points, a Gaspari-Cohn taper of `radius` points.  First the device's local_update(STATE) is compared
bitwise, field by field, with the restatement (tests/ens_local_ref.py) over the members' downloads.  Then,
alternating per repeat after one untimed repeat of each:

  device         assimilate("ssh", ...) -- sample(), the observation-space loop on the host, one
                 local_update(STATE) -- then synchronize
  device_update  local_update(STATE) with rows formed before, then synchronize: the part that replaces the
                 host's loop over the fields
  host           the only other route: download the six fields of every member, the observation-space loop,
                 the restatement's arithmetic in vectorised numpy on every field, upload them
  host_fields    host without the observation-space loop (both routes run the same one); host_copies: its
                 downloads and uploads alone

and the update's launches alone between two HIP events on the ensemble's stream (members complete; the copy
of the tables lies inside the span).  Reported: median (min - max) in ms over the repeats.
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
    ap.add_argument("--obs", default="64,1024")
    ap.add_argument("--radius", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()

    import numpy as np
    import torch

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd.ensemble import STATE, taper_table
    from tests import ens_local_ref as R
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])

    def summary(ts, nd=3):
        ms = [1e3 * t for t in ts]
        return {"median_ms": round(statistics.median(ms), nd), "min_ms": round(min(ms), nd), "max_ms": round(max(ms), nd)}

    taper = taper_table(a.radius)
    out = {"bench": "ens_local", "case": a.case, "steps": a.steps, "repeats": a.repeats, "fields": list(STATE),
           "radius": a.radius, "ntaper": len(taper), "build_id": amd.build_id(), "results": []}
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

        def downloads():
            return {nm: [m.download(0, nm) for m in e.members] for nm in STATE}

        for nobs in [int(x) for x in a.obs.split(",")]:
            rng = np.random.default_rng(1000 * M + nobs)
            ij = np.stack([rng.integers(blk.nx_start, blk.nx_end + 1, nobs), rng.integers(blk.ny_start, blk.ny_end + 1, nobs)], axis=1)
            pts = [(0, int(i), int(j)) for i, j in ij]
            variances = np.full(nobs, 1e-4)   # (1 cm)^2

            def truth():
                hx = e.sample("ssh", pts)
                return hx, hx.mean(axis=1) + rng.normal(0.0, 0.01, nobs)

            # the device against the restatement, bitwise, before anything is timed
            hx, values = truth()
            Y, Z, _ = R.ensrf_obs_space(hx, ij, values, variances, taper)
            before = downloads()
            e.local_update(Y, Z, ij, taper)
            after = downloads()
            same = all(R.bits_equal(g, v) for nm in STATE
                       for g, v in zip(after[nm], R.block_update(before[nm], blk, ij[:, 0], ij[:, 1], Y, Z, taper)))

            def device():
                _, v = truth()
                t0 = time.perf_counter()
                e.assimilate("ssh", ij, v, variances, taper)
                e.synchronize()
                return time.perf_counter() - t0, None

            def device_update():
                h, v = truth()
                y, z, _ = R.ensrf_obs_space(h, ij, v, variances, taper)
                t0 = time.perf_counter()
                e.local_update(y, z, ij, taper)
                e.synchronize()
                return time.perf_counter() - t0, None

            def host():
                _, v = truth()
                t0 = time.perf_counter()
                x = downloads()
                t1 = time.perf_counter()
                h = np.array([[f[i - blk.bnd_x1, j - blk.bnd_y1] for f in x["ssh"]] for i, j in ij])
                y, z, _ = R.ensrf_obs_space(h, ij, v, variances, taper)
                t2 = time.perf_counter()
                new = {nm: R.block_update(x[nm], blk, ij[:, 0], ij[:, 1], y, z, taper) for nm in STATE}
                t3 = time.perf_counter()
                for nm in STATE:
                    for m, f in zip(e.members, new[nm]):
                        m.upload(0, nm, f)
                t4 = time.perf_counter()
                return t4 - t0, ((t1 - t0) + (t4 - t2), (t1 - t0) + (t4 - t3))

            legs = {"device": device, "device_update": device_update, "host": host}
            times = {k: [] for k in legs}
            times["host_fields"], times["host_copies"] = [], []
            for r in range(a.repeats + 1):   # (repeat 0 untimed)
                for k, leg in legs.items():
                    dt, x = leg()
                    if r:
                        times[k].append(dt)
                        if k == "host":
                            times["host_fields"].append(x[0])
                            times["host_copies"].append(x[1])
            # the launches alone, between events on the ensemble's stream
            s = torch.cuda.ExternalStream(int(amd.lib().ocn_ctx_stream(e.members[0].ctx)))
            h, v = truth()
            y, z, _ = R.ensrf_obs_space(h, ij, v, variances, taper)
            kms = []
            for r in range(a.repeats + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                e.local_update(y, z, ij, taper)
                e1.record(s)
                e1.synchronize()
                if r:
                    kms.append(e0.elapsed_time(e1))
            res = {"members": M, "observations": nobs, "array": list(shape), "path": "register" if M <= 32 else "lds",
                   "bitwise_equal_to_restatement": bool(same), "statuses_ok": not any(e.synchronize())}
            for k, ts in times.items():
                res[k] = summary(ts)
            res["host_over_device"] = round(res["host"]["median_ms"] / res["device"]["median_ms"], 2)
            res["host_fields_over_device_update"] = round(res["host_fields"]["median_ms"] / res["device_update"]["median_ms"], 2)
            res["kernel"] = {"median_ms": round(statistics.median(kms), 5), "min_ms": round(min(kms), 5),
                             "max_ms": round(max(kms), 5), "launches": len(STATE)}
            out["results"].append(res)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
