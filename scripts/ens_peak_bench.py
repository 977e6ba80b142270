#!/usr/bin/env python
"""The peak map kept on the device against the routes around it: one JSON line.

    python scripts/ens_peak_bench.py [--members 8,32,64] [--steps 98] [--host-steps 4] [--repeats 5] [--legs a,b,c,d]

The case is the Black Sea fixture's basin (tests/golden, one block); per member count M in ONE process an
OceanEnsemble of M members, unforced and then with a storm per member (scripts/ens_forcing_bench.py's storms).
Every timed call follows an untimed 2-step call and a synchronize() (an open sequence) and is timed from the call
to the end of synchronize(); alternating per repeat after one untimed repeat of each:

  a  step(steps) / step_forced(steps) with no peak active: the baseline
  b  the same call with a peak active, in the launch (peak_info()["in_launch"] is asserted to grow by steps - 1)
  c  the same with set_peak_in_launch(False): the chunked route, one k_ens_peak launch per step
  d  the only route without the entries: step(1), a download of ssh from every member and the numpy rule, per
     step -- over --host-steps steps (it is slow), scaled to `steps`

Before anything is timed, per member count and forcing, P and S (max and min of ssh) after 2 + 6 steps by b, c and
d from identically started ensembles are compared bitwise, every member.
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
    ap.add_argument("--host-steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--case", default="bs_b1x1_s60")
    a = ap.parse_args()
    legs_on = a.legs.split(",")

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import ens_forcing_rule as FR
    from ocean_model_arch_amd import ens_peak_rule as PR
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])
    tau = 1.0

    def storm(i):
        cs, sn = FR.inflow(20.0)
        return FR.Storm(x0=0.2 * b["nx"] + 3.1 * (i % 16), y0=0.5 * b["ny"] + 1.7 * (i % 11) - 8.0, cx=0.0025, cy=0.0007 * (i % 5 - 2),
                        radius=1.0e5 + 2.0e3 * (i % 9), vmax=30.0 + (i % 7), dp=3000.0 + 50.0 * (i % 13), cos_in=cs, sin_in=sn)

    def fresh(M, forced):
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        if forced:
            e.set_storms([storm(i) for i in range(M)], FR.ForcingModel())
        e.step(2, tau, 1)
        if any(e.synchronize()):
            raise RuntimeError("member statuses after the first call")
        return e

    def go(e, forced, n, t0):
        if forced:
            e.step_forced(n, tau, t0)
        else:
            e.step(n, tau, 1)

    def box(e):
        g = e.members[0].blocks[0]
        return (g.nx_start - g.bnd_x1, g.nx_end - g.bnd_x1, g.ny_start - g.bnd_y1, g.ny_end - g.bnd_y1)

    def host_begin(e):
        return [{w: PR.begin(m.download(0, "ssh"), box(e)) for w in ("max", "min")} for m in e.members]

    def host_route(e, forced, peaks, k0, t0, steps):
        """leg d: step(1), every member's ssh down, the numpy rule."""
        for s in range(steps):
            go(e, forced, 1, t0 + s * tau)
            for m, pk in zip(e.members, peaks):
                x = m.download(0, "ssh")
                PR.update(*pk["max"], x, k0 + s + 1, box(e))
                PR.update(*pk["min"], x, k0 + s + 1, box(e), minimum=True)

    def summary(ms, per):
        return {"median_ms": round(statistics.median(ms) / per, 6), "min_ms": round(min(ms) / per, 6),
                "max_ms": round(max(ms) / per, 6)}

    out = {"bench": "ens_peak", "case": a.case, "steps": a.steps, "host_steps": a.host_steps, "repeats": a.repeats,
           "legs": legs_on, "unit": "ms per member-step", "ocn_build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        for forced in (False, True):
            k, got = 6, {}
            for leg in "bcd":
                f = fresh(M, forced)
                if leg == "d":
                    peaks = host_begin(f)
                    host_route(f, forced, peaks, 0, 0.0, k)
                    got[leg] = [[pk[w][x].tobytes(order="F") for w in ("max", "min") for x in (0, 1)] for pk in peaks]
                else:
                    f.set_peak_in_launch(leg == "b")
                    f.peak_begin("ssh", ("max", "min"))
                    go(f, forced, k, 0.0)
                    if f.peak_info()["in_launch"] != (k - 1 if leg == "b" else 0):
                        raise RuntimeError(f"leg {leg}: in_launch {f.peak_info()['in_launch']}")
                    got[leg] = [[a_.tobytes(order="F") for w in ("max", "min") for a_ in f.peak(i, 0, w)] for i in range(M)]
                f.close()
            if not (got["b"] == got["c"] == got["d"]):
                raise RuntimeError(f"{M} members, forced {forced}: the peaks of legs b, c and d differ")

            e = fresh(M, forced)
            clock = [0.0]
            res = {"members": M, "forced": forced, "array": list(e.members[0].blocks[0].shape), "peaks_bitwise_equal_b_c_d": True}

            def opened():   # (a plain call: a forced call runs in the launch only on sequences one has opened)
                e.step(2, tau, 1)
                e.synchronize()

            def timed(f):
                t0 = time.perf_counter()
                f()
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def stepped(peak, in_launch):
                opened()
                if peak:
                    e.set_peak_in_launch(in_launch)
                    e.peak_begin("ssh", ("max", "min"))
                k0 = 0
                dt = timed(lambda: go(e, forced, a.steps, clock[0]))
                clock[0] += a.steps * tau
                if peak:
                    if e.peak_info()["in_launch"] - k0 != (a.steps - 1 if in_launch else 0):
                        raise RuntimeError(f"in_launch grew by {e.peak_info()['in_launch'] - k0}")
                    e.peak_end()
                return dt

            def leg_d():
                opened()
                peaks = host_begin(e)
                dt = timed(lambda: host_route(e, forced, peaks, 0, clock[0], a.host_steps))
                clock[0] += a.host_steps * tau
                return dt * a.steps / a.host_steps

            legs = {k_: f for k_, f in (("a", lambda: stepped(False, False)), ("b", lambda: stepped(True, True)),
                                        ("c", lambda: stepped(True, False)), ("d", leg_d)) if k_ in legs_on}
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
            print(f"ens_peak_bench: {M} members, forced {forced} done", file=sys.stderr, flush=True)
            e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
