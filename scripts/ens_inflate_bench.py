#!/usr/bin/env python
"""Relaxation to prior spread on the device against download / numpy / upload of every member: one JSON line.

    python scripts/ens_inflate_bench.py [--members 8,32,64] [--steps 20] [--repeats 3] [--calls 20]
                                        [--variant-lib build_variants/libocn_sw_inf256x1.so] [--rounds 3]

The basin is the Black Sea fixture's (tests/golden, one block).  Per member count M, in ONE process: an
OceanEnsemble of M members, perturbed by a per-member ssh offset pattern so that they differ, after a 2-step
and a `steps`-step call, completed.  First spread_save(STATE) and inflate(STATE) are compared bitwise, field by
field, with the restatement (tests/ens_inflate_ref.py) over the members' downloads.  Then

  kernel   per call, between two HIP events on the ensemble's stream, members complete, after warm-up calls:
           spread_save(STATE) (six launches of k_ens_stats, the spread alone) and inflate(STATE) in RTPS with
           alpha 1 right after a CONST inflation by 0.5, so that every sea point is written each time (six
           launches of k_ens_inflate); median (min - max) over `calls` calls, and the achieved bytes/s by the
           model of (n + 1) reads + (n + 1) writes of 8 B per point and field for inflate, n reads + 1 write
           for spread_save (the model counts every point of the array; land points are read, not written)
  device   spread_save + inflate, then synchronize, by the host clock
  host     the only other route: download the six fields of every member, the restatement in numpy on every
           field, upload them; host_copies: its downloads and uploads alone

device and host alternate per repeat after one untimed repeat of each; median (min - max) in ms.

--variant-lib: the workgroup geometry.  The library builds k_ens_inflate with 64 x 4 workgroups; a library
built with EXTRA=-DOCN_ENS_INFLATE_ROWS=1 has 256 x 1.  The `kernel` measurement alone is then repeated in
fresh child processes, `rounds` times the pair (default library, variant library) in alternation, and both
series are reported under "geometry".
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="8,32,64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--case", default="bs_b1x1_s60")
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd.ensemble import STATE
    from tests import ens_inflate_ref as R
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])

    def summary(ts, nd=3):
        ms = [1e3 * t for t in ts]
        return {"median_ms": round(statistics.median(ms), nd), "min_ms": round(min(ms), nd), "max_ms": round(max(ms), nd)}

    out = {"bench": "ens_inflate", "case": a.case, "steps": a.steps, "repeats": a.repeats, "calls": a.calls,
           "fields": list(STATE), "lib": os.path.relpath(amd._lib.LIB_PATH, REPO), "build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        blk = e.members[0].blocks[0]
        shape = blk.shape
        points = shape[0] * shape[1]
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

        res = {"members": M, "array": list(shape), "path": "register" if M <= 32 else "re-read"}
        if not a.kernel_only:
            # the device against the restatement, bitwise, before anything is timed
            before = downloads()
            e.spread_save()
            sb = {nm: e.inflation(nm, "prior_spread") for nm in STATE}
            same = all(R.bits_equal(sb[nm], R.spread(before[nm])) for nm in STATE)
            e.inflate(0.5, "const")
            mid = downloads()
            e.inflate(1.0, "rtps")
            after = downloads()
            for nm in STATE:
                want, fac = R.inflate_rule(mid[nm], sb[nm], "rtps", 1.0)
                same = same and all(R.bits_equal(g, v) for g, v in zip(after[nm], want))
                same = same and R.bits_equal(e.inflation(nm, "factor"), fac)
            res["bitwise_equal_to_restatement"] = bool(same)
            res["points_written_of_ssh"] = int((e.inflation("ssh", "factor") != 1.0).sum())

        # the launches alone, between events on the ensemble's stream
        s = torch.cuda.ExternalStream(int(amd.lib().ocn_ctx_stream(e.members[0].ctx)))

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            e1.synchronize()
            return 1e-3 * e0.elapsed_time(e1)

        e.spread_save()
        ks, ki = [], []
        for r in range(a.calls + 3):   # (three warm-up calls of each)
            t_s = timed(lambda: e.spread_save())
            e.inflate(0.5, "const")
            t_i = timed(lambda: e.inflate(1.0, "rtps"))
            if r >= 3:
                ks.append(t_s)
                ki.append(t_i)
        model_i, model_s = 2 * (M + 1) * 8 * points * len(STATE), (M + 1) * 8 * points * len(STATE)
        res["kernel_inflate"] = dict(summary(ki, 5), launches=len(STATE), model_bytes=model_i,
                                     model_GBps=round(model_i / statistics.median(ki) / 1e9, 1))
        res["kernel_spread_save"] = dict(summary(ks, 5), launches=len(STATE), model_bytes=model_s,
                                         model_GBps=round(model_s / statistics.median(ks) / 1e9, 1))

        if not a.kernel_only:
            def device():
                e.inflate(0.5, "const")
                e.synchronize()
                t0 = time.perf_counter()
                e.spread_save()
                e.inflate(1.0, "rtps")
                e.synchronize()
                return time.perf_counter() - t0, None

            def host():
                e.inflate(0.5, "const")
                e.synchronize()
                t0 = time.perf_counter()
                x = downloads()
                t1 = time.perf_counter()
                new = {nm: R.inflate_rule(x[nm], R.spread(x[nm]), "rtps", 1.0)[0] for nm in STATE}
                t2 = time.perf_counter()
                for nm in STATE:
                    for m, f in zip(e.members, new[nm]):
                        m.upload(0, nm, f)
                t3 = time.perf_counter()
                return t3 - t0, (t1 - t0) + (t3 - t2)

            times = {"device": [], "host": [], "host_copies": []}
            for r in range(a.repeats + 1):   # (repeat 0 untimed)
                for k, leg in (("device", device), ("host", host)):
                    dt, x = leg()
                    if r:
                        times[k].append(dt)
                        if k == "host":
                            times["host_copies"].append(x)
            for k, ts in times.items():
                res[k] = summary(ts)
            res["host_over_device"] = round(res["host"]["median_ms"] / res["device"]["median_ms"], 1)
        res["statuses_ok"] = not any(e.synchronize())
        out["results"].append(res)
        print(f"[ens_inflate_bench] {M} members done", file=sys.stderr, flush=True)
        e.close()

    if a.variant_lib and not a.kernel_only:
        variant = os.path.abspath(a.variant_lib)
        series = {"64x4": [], "256x1": []}
        for r in range(a.rounds):
            for label, path in (("64x4", None), ("256x1", variant)):
                env = dict(os.environ)
                env.pop("OCN_LIB_PATH", None)
                if path:
                    env["OCN_LIB_PATH"] = path
                txt = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--kernel-only", "--members", a.members,
                                               "--steps", str(a.steps), "--calls", str(a.calls), "--case", a.case],
                                              env=env, text=True, timeout=600)
                series[label].append(json.loads(txt.strip().splitlines()[-1]))
                print(f"[ens_inflate_bench] geometry round {r}: {label} done", file=sys.stderr, flush=True)
        geo = {"rounds": a.rounds, "variant_lib": os.path.relpath(variant, REPO), "inflate_median_ms": {}}
        for label, runs in series.items():
            geo["build_id_" + label] = runs[0]["build_id"]
            for i, M in enumerate(int(x) for x in a.members.split(",")):
                geo["inflate_median_ms"].setdefault(str(M), {})[label] = [run["results"][i]["kernel_inflate"]["median_ms"] for run in runs]
        out["geometry"] = geo
    print(json.dumps(out))


if __name__ == "__main__":
    main()
