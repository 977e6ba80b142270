#!/usr/bin/env python
"""The serial filter's analysis with its observation-space loop on the host against the same on the device:
one JSON line.

    python scripts/ens_assim_bench.py [--members 8,32,64] [--obs 64,1024] [--radius 10] [--steps 20] [--repeats 5]
                                      [--gate off|inf|SIGMA] [--outliers FRACTION]

The case is scripts/ens_local_bench.py's: the Black Sea fixture's basin (tests/golden, one block), per member
count M in ONE process an OceanEnsemble of M members perturbed by per-member ssh patterns, after a 2-step and
a `steps`-step call, completed; per observation count that many ssh observations at random interior points,
a Gaspari-Cohn taper of `radius` points, STATE updated.  First assimilate(device=True) is compared bitwise
with the restatement (tests/ens_assim_ref.py) on the members' sample() and downloads: rows, vectors and
every field.  Then, alternating per repeat after one untimed repeat of each:

  host    assimilate(device=False) + synchronize: sample(), the observation-space loop in numpy, one
          local_update(STATE) -- the path before ocn_ens_assimilate, unchanged by it: the yardstick
  device  assimilate(device=True) + synchronize: one ocn_ens_assimilate, then its results read back
  call    ocn_ens_assimilate alone + synchronize: what a host that does not read the rows back pays

and, from timed calls (OCN_ENS_OPT_ASSIM_TIMING), the spans of k_ens_obs_space and of the update's launches
between HIP events on the ensemble's stream.  Reported: median (min - max) in ms over the repeats.

--gate (default off: the ungated kernels, every leg as before): the gate in sigma of every leg (ocn_ens_set_gate;
assimilate(gate=)), `inf` for the gated kernel that rejects nothing.  --outliers F (with a gate only): every
round(1 / F)-th observation's value is the members' mean + 1e3, which a finite gate rejects; the result then counts
the rejected observations of the checked call.
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--case", default="bs_b1x1_s60")
    ap.add_argument("--gate", default="off")
    ap.add_argument("--outliers", type=float, default=0.0)
    a = ap.parse_args()
    gate = None if a.gate == "off" else float(a.gate)
    if a.outliers and (gate is None or not 0.0 < a.outliers <= 1.0):
        ap.error("--outliers: a fraction in (0, 1], with a --gate")
    every = int(round(1.0 / a.outliers)) if a.outliers else 0

    import ctypes as C

    import numpy as np

    import ocean_model_arch_amd as amd
    from ocean_model_arch_amd import _lib
    from ocean_model_arch_amd.ensemble import STATE, taper_table
    from tests import ens_assim_ref as A
    from tests.golden import cases

    c = cases.load_e2e(a.case)
    b = c["basin"]
    basin = amd.BasinConfig(nx=b["nx"], ny=b["ny"], dxst=b["dxst"], dyst=b["dyst"], rlon=b["rlon"], rlat=b["rlat"],
                            curve_grid=b["curve_grid"], mask=c["mask"], topography=c.get("topography"))
    sw, par = amd.SWConfig(**c["sw"]), amd.ParallelConfig(*c["bxy"])

    def summary(ms, nd=4):
        return {"median_ms": round(statistics.median(ms), nd), "min_ms": round(min(ms), nd), "max_ms": round(max(ms), nd)}

    taper = taper_table(a.radius)
    out = {"bench": "ens_assim", "case": a.case, "steps": a.steps, "repeats": a.repeats, "fields": list(STATE),
           "radius": a.radius, "ntaper": len(taper), "ocn_build_id": amd.build_id(), "gate": a.gate, "outliers": a.outliers,
           "results": []}
    L = amd.lib()
    kw = {} if gate is None else {"gate": gate}
    gate2 = None if gate is None else gate * gate
    ids = (C.c_int32 * len(STATE))(*[_lib.FIELD_ID[nm] for nm in STATE])
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
            io, jo = np.ascontiguousarray(ij[:, 0], dtype=np.int32), np.ascontiguousarray(ij[:, 1], dtype=np.int32)
            variances = np.full(nobs, 1e-4)   # (1 cm)^2
            ptr = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731

            def truth():
                hx = e.sample("ssh", pts)
                values = hx.mean(axis=1) + rng.normal(0.0, 0.01, nobs)
                if every:
                    values[::every] = hx.mean(axis=1)[::every] + 1e3
                return hx, values

            # the device against the restatement, bitwise, before anything is timed
            hx, values = truth()
            before = downloads()
            got = e.assimilate("ssh", ij, values, variances, taper, device=True, **kw)
            yz = e.assimilate_results(("y", "z"))
            after = downloads()
            Y, Z, ref = A.ensrf_obs_space_ordered(hx, ij, values, variances, taper, gate2=gate2)
            acc = ref["accepted"] if gate is not None else np.ones(nobs, dtype=bool)   # (the update takes the accepted alone)
            same = (not A.info_mismatches(got, ref) and A.bits_equal(yz["y"], Y) and A.bits_equal(yz["z"], Z)
                    and (gate is None or list(got["accepted"]) == list(acc))
                    and all(A.bits_equal(g, v) for nm in STATE
                            for g, v in zip(after[nm], A.block_update(before[nm], blk, ij[acc, 0], ij[acc, 1], Y[acc], Z[acc], taper))))

            def host():
                _, v = truth()
                t0 = time.perf_counter()
                e.assimilate("ssh", ij, v, variances, taper, **kw)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def device():
                _, v = truth()
                t0 = time.perf_counter()
                e.assimilate("ssh", ij, v, variances, taper, device=True, **kw)
                e.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def call():
                _, v = truth()
                v = np.ascontiguousarray(v)
                if gate is not None:   # (the Python driver's legs leave it set; an ungated run never names the entry)
                    amd._lib.check(L.ocn_ens_set_gate(e.ens, gate2), "ocn_ens_set_gate")
                t0 = time.perf_counter()
                rc = L.ocn_ens_assimilate(e.ens, _lib.FIELD_ID["ssh"], ids, len(STATE), None, nobs, ptr(io), ptr(jo), ptr(v),
                                          ptr(variances), ptr(taper), len(taper))
                e.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                amd._lib.check(rc, "ocn_ens_assimilate")
                return dt

            legs = {"host": host, "device": device, "call": call}
            times = {k: [] for k in legs}
            for r in range(a.repeats + 1):   # (repeat 0 untimed)
                for k, leg in legs.items():
                    dt = leg()
                    if r:
                        times[k].append(dt)
            e.set_assim_timing(True)
            spans = {"obs_space_ms": [], "update_ms": []}
            for r in range(a.repeats + 1):
                _, v = truth()
                e.assimilate("ssh", ij, v, variances, taper, device=True, **kw)
                sp = e.assimilate_spans()
                if r:
                    for k in spans:
                        spans[k].append(sp[k])
            e.set_assim_timing(False)
            res = {"members": M, "observations": nobs, "array": list(shape), "update_path": "register" if M <= 32 else "lds",
                   "bitwise_equal_to_restatement": bool(same), "nonfinite": int(got["nonfinite"]),
                   "statuses_ok": not any(e.synchronize())}
            if gate is not None:
                res["rejected"] = int(got["rejected"])
            for k, ts in times.items():
                res[k] = summary(ts)
            res["k_ens_obs_space"] = summary(spans["obs_space_ms"], 5)
            res["update_launches"] = dict(summary(spans["update_ms"], 5), launches=len(STATE))
            res["host_over_device"] = round(res["host"]["median_ms"] / res["device"]["median_ms"], 2)
            res["us_per_observation"] = round(1e3 * res["k_ens_obs_space"]["median_ms"] / nobs, 3)
            out["results"].append(res)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
