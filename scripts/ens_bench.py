#!/usr/bin/env python
"""Ensemble launch against a loop over contexts on the Black Sea basin (one block): one JSON line.

    python scripts/ens_bench.py [--members 1,2,4,8,16,32,64] [--calls 10] [--steps 100] [--repeats 5]
                                [--rows-sweep 8,16]

The basin and mask are the Black Sea fixture's (tests/golden, as the bs_b1x1_* cases load them).  Per
member count M, in ONE process, alternating per repeat so that both legs see the same clock state:

  ens   OceanEnsemble of M members: an untimed 2-step call + synchronize (opens the sequences, the
        known-constant verdicts reach the host), then the timed region: `calls` calls of `steps` steps
        with check_every 1, ocn_ens_complete, ocn_ens_synchronize.
  loop  the same M members as M independent OceanModel contexts stepped one after the other (what a
        host can do without ensembles): the same calls, then complete + synchronize of each.  Every
        context has its own stream, and a multi-step launch needs all its workgroups resident: where
        the members' launches together exceed the device's capacity (M x tiles > capacity) the host
        synchronizes each member's call before it steps the next member -- unsynchronised, the launches
        can each be partly resident and wait for each other until the barriers give up (measured:
        OCN_ERR_HIP from M = 8 on, profiles/ensemble/ens_bench_loop_unsynchronised.json).
  loop_per_step  the same contexts with OCN_OPT_MULTI off: one launch per step on M streams, which
        needs no such care.

One untimed repeat of both legs first (code objects, allocations).  Reported per M and leg: the median
and the spread over the repeats of ms per member-step, the aggregate cell-updates/s, and ocn_ens_info
of the last timed call.  --rows-sweep: for those M, the ensemble again with OCN_ENS_OPT_MAX_GROUP M/2
and M/4 -- two or four launches of shorter tiles against one of taller tiles (the planner's policy
question).  A leg that fails (a barrier that gave up) is reported with its error, not retried.
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
    ap.add_argument("--members", default="1,2,4,8,16,32,64")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows-sweep", default="8,16")
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()

    import ocean_model_arch_amd as amd
    from tests.golden import cases

    case = cases.load_e2e(a.case)
    b = case["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=case["mask"], topography=case.get("topography"))
    sw, par = amd.SWConfig(**case["sw"]), amd.ParallelConfig(*case["bxy"])
    cells = (b["nx"] - 4) * (b["ny"] - 4)

    def ens_leg(e):
        e.init().step(2, 1.0, 1)
        st = e.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            e.step(a.steps, 1.0, 1)
        info = e.info()
        e.complete()
        st += e.synchronize()
        dt = time.perf_counter() - t0
        if any(st):
            raise RuntimeError(f"member statuses {st}")
        return dt, info

    def single_tiles():   # sw_kernels.hip multi_rows: the shortest tiles with at most 256 workgroups
        w, h = b["nx"] - 4, b["ny"] - 4
        return next(t for t in (-(-w // 60) * -(-h // (4 * r)) for r in range(1, 17)) if t <= 256)

    def loop_leg(ms, multi, capacity):
        serial = multi and len(ms) * single_tiles() > capacity
        for m in ms:
            m.set_multi(multi)
            m.init().step(2, 1.0, 1)
        for m in ms:
            m.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            for m in ms:
                m.step(a.steps, 1.0, 1)
                if serial:
                    m.synchronize()
        for m in ms:
            m.complete()
        for m in ms:
            m.synchronize()
        return time.perf_counter() - t0, {"multi_step_launches": all(m.multi_active for m in ms), "serialised": serial}

    def stats(ts, M):
        per = [1e3 * t / (M * a.calls * a.steps) for t in ts]
        med = statistics.median(per)
        return {"ms_per_member_step": round(med, 6), "min": round(min(per), 6), "max": round(max(per), 6),
                "cell_updates_per_s": round(cells / (med * 1e-3), 1)}

    rows_sweep = [int(x) for x in a.rows_sweep.split(",") if x]
    out = {"bench": "ensemble", "case": a.case, "cells_per_member": cells, "calls": a.calls, "steps_per_call": a.steps,
           "repeats": a.repeats, "build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        e = amd.OceanEnsemble(basin, sw, par, members=M)
        ms = [amd.OceanModel(basin, sw, par) for _ in range(M)]
        capacity = e.info()["capacity"]
        legs = {"ens": lambda: ens_leg(e), "loop": lambda: loop_leg(ms, True, capacity),
                "loop_per_step": lambda: loop_leg(ms, False, capacity)}
        splits = [g for g in (M // 2, M // 4) if M in rows_sweep and g >= 1]
        for g in splits:
            legs[f"ens_max_group_{g}"] = (lambda g=g: (e.set_max_group(g), ens_leg(e), e.set_max_group(0))[1])
        times, extra, errors = {k: [] for k in legs}, {}, {}
        for r in range(a.repeats + 1):   # (repeat 0 untimed)
            for k, leg in legs.items():
                if k in errors:
                    continue
                try:
                    dt, x = leg()
                except Exception as ex:   # noqa: BLE001 -- reported in the result line
                    errors[k] = str(ex)
                    continue
                if r:
                    times[k].append(dt)
                    extra[k] = x
        res = {"members": M}
        for k in legs:
            if k in errors:
                res[k] = {"error": errors[k]}
                continue
            res[k] = stats(times[k], M)
            res[k]["info"] = extra[k]
        loops = [res[k]["ms_per_member_step"] for k in ("loop", "loop_per_step") if k not in errors]
        if "ens" not in errors and loops:   # the better of the two loops against the ensemble
            res["loop_over_ens"] = round(min(loops) / res["ens"]["ms_per_member_step"], 3)
        out["results"].append(res)
        e.close()
        for m in ms:
            m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
