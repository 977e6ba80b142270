#!/usr/bin/env python
"""The moving-storm forcing formed on the device against the route around it: one JSON line.

    python scripts/ens_forcing_bench.py [--members 8,32,64] [--steps 98] [--host-steps 4] [--repeats 5]
                                        [--legs a,b,c,d]

The case is the Black Sea fixture's basin (tests/golden, one block); per member count M in ONE process an
OceanEnsemble of M members, each with a storm of its own track, size and strength (100 km radius, 30 m/s, 30 hPa,
moving 10 m/s).  Every timed call follows an untimed 2-step call and a synchronize() (an open sequence), and is
timed from the call to the end of synchronize(); alternating per repeat after one untimed repeat of each:

  a  the only route without the entries: per step and member the forcing in numpy on the host, two uploads,
     then step(1) -- over --host-steps steps (it is slow), with np.exp in the place of the per-element math.exp
     of the bitwise restatement (a faster host than the one the comparison below uses)
  b  step_forced(steps) with set_forcing_in_launch(False): the chunked route, one forcing launch per step
  c  step_forced(steps) in the launch (forcing_info()["in_launch"] is asserted)
  d  step(steps) of the same forced members, the forcing held: the general variant's multi-step launch, the floor

Before anything is timed, per member count, the states after 2 + 4 steps by a (with the bitwise restatement), b and
c from identically started ensembles are compared bitwise, every member, the six state fields and RHSx / RHSy.
Reported: median (min - max) in ms per member-step over the repeats.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIELDS = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp", "RHSx", "RHSy")
NAMES = ("lcu", "lcv", "dx", "dy", "dxt", "dyt", "dxh", "dyh", "hhq_rest")


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

    import numpy as np

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import ens_forcing_rule as FR
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])
    model = FR.ForcingModel()
    tau = 1.0

    def storm(i):
        cs, sn = FR.inflow(20.0)
        return FR.Storm(x0=0.2 * b["nx"] + 3.1 * (i % 16), y0=0.5 * b["ny"] + 1.7 * (i % 11) - 8.0, cx=0.0025, cy=0.0007 * (i % 5 - 2),
                        radius=1.0e5 + 2.0e3 * (i % 9), vmax=30.0 + (i % 7), dp=3000.0 + 50.0 * (i % 13), cos_in=cs, sin_in=sn)

    def fresh(M):
        e = amd.OceanEnsemble(basin, sw, par, members=M).init()
        e.set_storms([storm(i) for i in range(M)], model)
        e.step(2, tau, 1)
        if any(e.synchronize()):
            raise RuntimeError("member statuses after the first call")
        return e

    def host_route(e, statics, t0, steps):
        """leg a: per step and member the forcing on the host, two uploads, step(1)."""
        for s in range(steps):
            t = FR.step_time(t0, s, tau)
            for i, m in enumerate(e.members):
                blk = m.blocks[0]
                rx, ry = FR.rhs(storm(i), model, t, statics[i], (blk.bnd_x1, blk.bnd_y1),
                                (blk.nx_start, blk.nx_end, blk.ny_start, blk.ny_end))
                m.upload(0, "RHSx", rx)
                m.upload(0, "RHSy", ry)
            e.step(1, tau, 1)

    def summary(ms, per):
        return {"median_ms": round(statistics.median(ms) / per, 6), "min_ms": round(min(ms) / per, 6),
                "max_ms": round(max(ms) / per, 6)}

    out = {"bench": "ens_forcing", "case": a.case, "steps": a.steps, "host_steps": a.host_steps, "repeats": a.repeats,
           "legs": legs_on, "unit": "ms per member-step", "ocn_build_id": amd.build_id(), "results": []}
    for M in [int(x) for x in a.members.split(",")]:
        # the three routes' states from identical starts, bitwise
        k, states = 4, {}
        for leg in "abc":
            f = fresh(M)
            if leg == "a":
                statics = [{nm: m.download(0, nm) for nm in NAMES} for m in f.members]
                host_route(f, statics, 0.0, k)
            else:
                f.set_forcing_in_launch(leg == "c")
                f.step_forced(k, tau, 0.0)
                if f.forcing_info()["in_launch"] != (leg == "c"):
                    raise RuntimeError(f"leg {leg}: in_launch {f.forcing_info()['in_launch']}")
            f.complete()
            if any(f.synchronize()):
                raise RuntimeError(f"member statuses in leg {leg}'s comparison run")
            states[leg] = [[m.download(0, nm).tobytes(order="F") for nm in FIELDS] for m in f.members]
            f.close()
        equal = states["a"] == states["b"] == states["c"]
        if not equal:
            raise RuntimeError(f"{M} members: the states of legs a, b and c differ")

        e = fresh(M)
        blk = e.members[0].blocks[0]
        statics = [{nm: m.download(0, nm) for nm in NAMES} for m in e.members]
        clock = [0.0]
        res = {"members": M, "array": list(blk.shape), "states_bitwise_equal_a_b_c": equal}

        def opened():
            e.step(2, tau, 1)
            e.synchronize()

        def timed(f):
            t0 = time.perf_counter()
            f()
            e.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        def leg_a():
            opened()
            keep, FR._exp_libm = FR._exp_libm, np.exp   # (timing only: a faster host than the bitwise restatement)
            try:
                dt = timed(lambda: host_route(e, statics, clock[0], a.host_steps))
            finally:
                FR._exp_libm = keep
            clock[0] += a.host_steps * tau
            return dt * a.steps / a.host_steps             # (as if over `steps` steps: the same divisor as the others)

        def forced(in_launch):
            e.set_forcing_in_launch(in_launch)
            opened()
            dt = timed(lambda: e.step_forced(a.steps, tau, clock[0]))
            clock[0] += a.steps * tau
            if e.forcing_info()["in_launch"] != in_launch:
                raise RuntimeError(f"in_launch {e.forcing_info()['in_launch']}, not {in_launch}")
            return dt

        def leg_d():
            opened()
            return timed(lambda: e.step(a.steps, tau, 1))

        legs = {k_: f for k_, f in (("a", leg_a), ("b", lambda: forced(False)), ("c", lambda: forced(True)), ("d", leg_d))
                if k_ in legs_on}
        times = {k_: [] for k_ in legs}
        for r in range(a.repeats + 1):   # (repeat 0 untimed)
            for k_, leg in legs.items():
                dt = leg()
                if r:
                    times[k_].append(dt)
        res["statuses_ok"] = not any(e.synchronize())
        res["groups"] = e.info()["groups"]
        for k_, ts in times.items():
            res[k_] = summary(ts, M * a.steps)
        out["results"].append(res)
        print(f"ens_forcing_bench: {M} members done", file=sys.stderr, flush=True)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
