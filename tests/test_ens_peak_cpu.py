"""CPU checks of the peak map (include/ocn_sw.h ocn_ens_peak_*): the rule's header (csrc/ens_peak_point.h, the
text the device compiles) built with g++ against the numpy restatement (ens_peak_rule.update) and a scalar loop,
bit for bit; the premises of the GPU runs (tests/test_gpu_ens_peak.py) on the reference alone; and the validation
errors from Python.  No device anywhere."""
import os
import subprocess

import numpy as np
import pytest

from ocean_model_arch_amd import ens_peak_rule as PR
from tests import ens_forcing_ref as R
from tests import ens_peak_ref as K

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ocean_model_arch_amd", "csrc")

HARNESS = r"""
#define __host__
#define __device__
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ens_peak_point.h"
// in.bin: n, steps as doubles, then P0[n], then steps x x[n];  out.bin: Pmax[n], Pmin[n] doubles, Smax[n], Smin[n] int32
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    double hd[2];
    if (fread(hd, 8, 2, f) != 2) return 4;
    const size_t n = (size_t)hd[0];
    const int steps = (int)hd[1];
    std::vector<double> pmax(n), pmin(n), x(n);
    std::vector<int32_t> smax(n, 0), smin(n, 0);
    if (fread(pmax.data(), 8, n, f) != n) return 5;
    pmin = pmax;
    for (int k = 1; k <= steps; ++k) {
        if (fread(x.data(), 8, n, f) != n) return 6;
        for (size_t q = 0; q < n; ++q) {
            ocn::peak_point<false>(x[q], k, pmax[q], smax[q]);
            ocn::peak_point<true>(x[q], k, pmin[q], smin[q]);
        }
    }
    fclose(f);
    f = fopen(argv[2], "wb");
    fwrite(pmax.data(), 8, n, f); fwrite(pmin.data(), 8, n, f);
    fwrite(smax.data(), 4, n, f); fwrite(smin.data(), 4, n, f);
    fclose(f);
    printf("%zu points %d steps\n", n, steps);
    return 0;
}
"""


def _scalar(p0, xs, minimum):
    """The rule as a loop over Python floats."""
    P, S = [float(v) for v in p0], [0] * len(p0)
    for k, x in enumerate(xs, 1):
        for q, v in enumerate(x):
            v = float(v)
            if ((v < P[q]) if minimum else (v > P[q])) or P[q] != P[q]:
                P[q], S[q] = v, k
    return np.array(P), np.array(S, dtype=np.int32)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_rule_header_matches_numpy_and_a_scalar_loop_bitwise(tmp_path):
    inf, nan, den = float("inf"), float("nan"), 5e-324
    special = [0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -52, inf, -inf, nan, den, -den, 2.0 ** -1022, 1e308, -1e308]
    rng = np.random.default_rng(7)
    # every ordered pair of special values as (P0, x1), then more steps of special and random values
    p0 = np.array([a for a in special for _ in special] + list(rng.standard_normal(64)))
    n, steps = len(p0), 7
    xs = [np.array([b for _ in special for b in special] + list(rng.standard_normal(64)))]
    for _ in range(steps - 1):
        x = rng.choice(np.array(special + [0.5, -0.5, 2.0]), size=n)
        xs.append(np.where(rng.random(n) < 0.3, xs[-1], x))          # equal values from step to step among them
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    np.concatenate([[float(n), float(steps)], p0] + xs).tofile(tmp_path / "in.bin")
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith(f"{n} points {steps} steps"), r.stdout + r.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    got_p = np.frombuffer(raw[:16 * n], dtype=np.float64).reshape(2, n)
    got_s = np.frombuffer(raw[16 * n:], dtype=np.int32).reshape(2, n)
    box = (0, n - 1, 0, 0)
    for m, minimum in enumerate((False, True)):
        P, S = PR.begin(p0.reshape(n, 1), box)
        for k, x in enumerate(xs, 1):
            PR.update(P, S, x.reshape(n, 1), k, box, minimum=minimum)
        sp, ss = _scalar(p0, xs, minimum)
        # (NaN by position, every other value by its bits, -0.0 included)
        for want_p, want_s in ((P[:, 0], S[:, 0]), (sp, ss)):
            assert np.array_equal(np.isnan(got_p[m]), np.isnan(want_p))
            ok = ~np.isnan(want_p)
            assert _bits(got_p[m][ok], np.ascontiguousarray(want_p[ok]))
            assert _bits(got_s[m], np.ascontiguousarray(want_s))
    # the properties the contract names, on the first step's pairs
    P, S = PR.begin(p0.reshape(n, 1), box)
    PR.update(P, S, xs[0].reshape(n, 1), 1, box)
    a, b = p0, xs[0]
    tie = (a == b)
    assert tie.any() and (S[tie, 0] == 0).all() and _bits(P[tie, 0], a[tie])            # +-0 and equal values: the earlier bits
    assert (S[np.isnan(a), 0] == 1).all() and _bits(P[np.isnan(a) & ~np.isnan(b), 0], b[np.isnan(a) & ~np.isnan(b)])
    assert (S[np.isnan(b) & ~np.isnan(a), 0] == 0).all()                                # a NaN x replaces no number


# ---------------------------------------------------------------- the premises of the GPU runs
RUNS = [("one_tile", False, "ssh"), ("one_tile", False, "ubrtr"), ("many_tiles", False, "ssh"), ("one_tile", True, "ssh"),
        ("many_tiles", True, "ssh"), ("subset", True, "ssh"), ("groups", True, "ssh"), ("groups", False, "ssh"), ("tau03", False, "ssh")]


@pytest.mark.parametrize("name,forced,field", RUNS)
def test_premises_of_the_gpu_runs(name, forced, field):
    """Per call of two steps or more: some interior point of some member has its Smax or Smin, as it stands after
    the call, at a step of that call that is not its last (only the update inside the launch can have written it)
    and some point at the call's last step (the launch behind it).  Land keeps S = 0; two members differ in P."""
    shape, params, classes, _, run_calls = R.RUNS[name]
    calls = K.CALLS if len(run_calls) == 5 else (2, 5, 4)
    refs = [K.reference(name, i, field, forced, calls) for i in range(len(classes))]
    box = K.interiors(shape, params)[(1, 1)]
    inner = (slice(box[0], box[1] + 1), slice(box[2], box[3] + 1))
    done = 0
    for c, n in enumerate(calls):
        s_all = np.stack([r[c][(1, 1)][w][1][inner] for r in refs for w in ("max", "min")])
        if n >= 2:
            assert ((s_all > done) & (s_all < done + n)).any(), (name, c, "no peak inside the call")
            assert (s_all == done + n).any(), (name, c, "no peak at the call's last step")
        done += n
    if field == "ssh":
        land = K.land(shape, params)[(1, 1)]
        if land[inner].any():
            for r in refs:
                for w in ("max", "min"):
                    assert (r[-1][(1, 1)][w][1][land] == 0).all()
    last = [r[-1][(1, 1)]["max"][0] for r in refs]
    assert any(not _bits(last[0], p) for p in last[1:])
    # outside the interior: +0.0 / 0
    outside = np.ones(last[0].shape, dtype=bool)
    outside[inner] = False
    for r in refs:
        assert _bits(r[-1][(1, 1)]["max"][0][outside], np.zeros(int(outside.sum()))) and (r[-1][(1, 1)]["max"][1][outside] == 0).all()


def test_still_water_keeps_s_zero():
    """A member whose state is +0.0 everywhere and that nothing forces does not move in the oracle: S stays 0."""
    last, top = K.still_reference(R.RUNS["one_tile"][0], "ssh", sum(K.CALLS))
    assert top == 0.0
    assert (last["max"][1] == 0).all() and (last["min"][1] == 0).all()


# ---------------------------------------------------------------- validation from Python
def test_python_validation():
    with pytest.raises(TypeError):
        PR.what_bits(("max", 1))
    with pytest.raises(ValueError):
        PR.what_bits(("max", "mean"))
    with pytest.raises(ValueError):
        PR.what_bits(())
    assert PR.what_bits("max") == 1 and PR.what_bits(("min", "max")) == 3 and PR.which_bit("min") == 2
    with pytest.raises(TypeError):
        PR.which_bit(1)
    with pytest.raises(ValueError):
        PR.which_bit("both")
    with pytest.raises(ValueError):
        PR.check_field("hhq")
    with pytest.raises(TypeError):
        PR.check_field(32)
    with pytest.raises(TypeError):
        PR.check_threshold("1.0")
    with pytest.raises(ValueError):
        PR.check_threshold(float("nan"))
    assert PR.check_threshold(float("inf")) == float("inf")
    with pytest.raises(ValueError):
        PR.update(*PR.begin(np.zeros((2, 2)), (0, 1, 0, 1)), np.zeros((2, 2)), 0, (0, 1, 0, 1))
    e = PR.exceed(np.array([[[1.0]], [[float("nan")]], [[2.0]], [[1.0]]]), 1.0)
    assert e.shape == (1, 1) and e[0, 0] == 0.25
