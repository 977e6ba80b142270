"""GPU parameter sweep: the march paths of tests/test_gpu_shapes.py and tests/test_gpu_coast.py (one-pass,
pair, multi-step, x2, x4, the ensemble launch, loopback ranks, tracer steps, the role-flip / stage paths)
at run parameters other than tau = 1, time_smooth = 0.5 on the default grid -- bitwise against the CPU
oracle, which tests/test_oracle_pinned.py pins to the compiled reference at each of these parameter sets
(tests/golden/cases.py PARAM_CASES).  The same drive, comparison and path-flag assertions as those sweeps,
on the coastline sweep's smallest shapes.

The sets (tests/shapes.py PARAMS; tests/test_params_cpu.py asserts what each promises and that every
run here stays bounded):
  tau 0.3, 0.75, 3, 30   no power of two: sw_kernels.hip MarchStep<P2 = false>, whose qtau is the IEEE
                         division a / tau -- the variant each of the five launch sites (launch_onepass,
                         the multi-step, pair and x4 launches, onepass_multi_variant for ensembles) picks
                         by std::frexp, in the known-constant, h_r-read and general flavours
  tau 2, 0.25            P2 = true with inv_tau != 1 (at tau = 1, a * inv_tau, a * tau and a are one value)
  time_smooth 0, 0.3, 1  the filter off, at weights whose products round, and at full weight
  cart, south, equator,  per-row metric tables and reciprocals that differ from row to row (coarse: in the
  coarse, polar          second digit, so row n +- 1 for row n changes high bits -- on the ext rows that
                         x2 / x4 steps form for their halo too), Coriolis terms of either and both signs
  rot                    rlh_s varies along a row: the compact tables are refused, the 2-D-array path runs

The tau-change cases cross the P2 / non-P2 boundary between calls with no synchronize() or read in
between: a deferred last step must run with the tau -- and the variant -- of the call that owns it.

Tolerance: none.
"""
import pytest

from tests import shapes as S
from tests.test_gpu_ensemble import OK, _bad, _calls, _start
from tests.test_gpu_shapes import SINGLE_MODES, _drive, _grid_failures, _model, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


# ---------------------------------------------------------------- the cases (tests/test_params_cpu.py reads them)
SINGLE_CLASSES = ("noise", "general")
GRID_CLASSES = ("noise", "hr", "general")
SINGLE_CASES = [(p, s, md) for p in S.CORE_PARAMS for s in S.PARAM_SINGLE for md in SINGLE_MODES]
DEEP_SHAPE, DEEP_MODE = S.PARAM_SINGLE[0], "pair26"
GRID_CASES = [(p, s, x4, ov) for p in S.CORE_PARAMS for s in S.PARAM_GRIDS for x4 in (0, 1) for ov in (1, 2)]
TRACER_CASES = [(p, s, x4) for p in S.CORE_PARAMS for s in S.PARAM_TRACER_GRIDS for x4 in (1, 3)]
RANK_CASES = [(p, s) for p in S.CORE_PARAMS for s in S.PARAM_RANK_GRIDS]
RANK_CALLS = [2, 2, 3]
OTHER_SINGLE, OTHER_MODES, OTHER_GRID = S.PARAM_SINGLE[0], ("default", "pair26"), S.PARAM_GRIDS[0]
FLAG_PARAMS, FLAG_SHAPE, FLAG_SETTINGS = "tau03", S.PARAM_TRACER_GRIDS[0], [(0, 1, 1), (1, 0, 1)]
# layout -> (shape, model options, {call: the path flags wanted after it}).  A tau change ends the open
# sequence (ocn_ctx.hip step_impl: complete_open with the old tau, then a new call), and a new call pairs
# two steps only where the second is not its last, so of these calls only the 3-step one at tau = 2 runs a pair
TAU_LAYOUTS = {
    "default": (S.PARAM_SINGLE[0], {}, {4: {"one": True}}),
    "nomulti": (S.PARAM_SINGLE[0], {"multi": False}, {4: {"one": True, "multi": False}}),
    "pair26": (S.PARAM_SINGLE[0], {"multi": False, "pair": 2}, {3: {"one": True, "pair": True}, 4: {"one": True}}),
    "grid_x4": (S.PARAM_GRIDS[0], {"x4": 1}, {4: {"x2": True}}),
}
TAU_CLASS = "noise"


def _single_failures(amd, shape, mode, classes, params):
    opts, calls, _, want = SINGLE_MODES[mode]
    failures = []
    for cls in classes:
        # the general class in the pair mode: known constants off, so the general-variant pair runs
        kc = False if (cls == "general" and mode.startswith("pair")) else None
        bad, flags = _run(amd, shape, cls, calls, kc=kc, params=params, **opts)
        if bad:
            failures.append(f"{cls}: fields differ from the oracle: {bad}")
        got = {k: flags[-1][k] for k in want}
        if got != want or not flags[0]["one"]:
            failures.append(f"{cls}: path flags {flags}, wanted {want} after the verdict and one-pass steps throughout")
    return failures


# ---------------------------------------------------------------- the core sets on every path
@pytest.mark.parametrize("params,shape,mode", SINGLE_CASES, ids=[f"{p}-{s.id}-{md}" for p, s, md in SINGLE_CASES])
def test_single_block_params_match_oracle(amd, params, shape, mode):
    failures = _single_failures(amd, shape, mode, SINGLE_CLASSES, params)
    assert not failures, f"{params} {shape.id} ({mode}): " + "; ".join(failures)


@pytest.mark.parametrize("params", S.PARAM_DEEP)
def test_single_block_deep_params_match_oracle(amd, params):
    """abyss (tests/shapes.py): every row with a wet velocity point takes both IEEE re-runs, and a / tau is
    a division in the same rows -- in the pair launch's producer and consumer waves."""
    failures = _single_failures(amd, DEEP_SHAPE, DEEP_MODE, ("abyss",), params)
    assert not failures, f"{params} {DEEP_SHAPE.id} ({DEEP_MODE}): " + "; ".join(failures)


@pytest.mark.parametrize("params,shape,x4,overlap", GRID_CASES,
                         ids=[f"{p}-{s.id}-x4_{x}-ov{o}" for p, s, x, o in GRID_CASES])
def test_block_grid_params_match_oracle(amd, params, shape, x4, overlap):
    """x2 steps and x4 pairs: 27 x 27 on 3 x 3 has a block with ext rows above and below."""
    failures = _grid_failures(amd, shape, x4, overlap, classes=GRID_CLASSES, params=params)
    assert not failures, f"{params} {shape.id} (x4 {x4}, overlap {overlap}): " + "; ".join(failures)


@pytest.mark.parametrize("params,shape,x4", TRACER_CASES, ids=[f"{p}-{s.id}-x4_{x}" for p, s, x in TRACER_CASES])
def test_tracer_block_grid_params_match_oracle(amd, params, shape, x4):
    failures = _grid_failures(amd, shape, x4, 1, classes=GRID_CLASSES, params=params)
    assert not failures, f"{params} {shape.id} (x4 {x4}): " + "; ".join(failures)


def _ranks(amd, shape, cls, params, flags=(1, 1, 1)):
    """One block per loopback rank, calls [2, 2, 3] with a synchronize() after the first two (see
    tests/test_gpu_shapes.py test_rank_grids_match_oracle): (fields that differ, the ranks' path flags)."""
    nranks = shape.grid[0] * shape.grid[1]
    models = [_model(amd, shape, rank=r, nranks=nranks, params=params, flags=flags) for r in range(nranks)]
    try:
        amd.OceanModel.attach_loopback(models)
        paths = amd.run_ranks(models, lambda m: _drive(m, shape, cls, RANK_CALLS, nsync=2, params=params))
        get = S.model_getter(models)
        ref = S.reference(shape, cls, sum(RANK_CALLS), flags, params)
        assert get.blocks == set(ref) and all(len(m.blocks) == 1 for m in models)
        bad = S.mismatches(ref, get)
    finally:
        for m in models:
            m.close()
    return bad, paths


@pytest.mark.parametrize("params,shape", RANK_CASES, ids=[f"{p}-{s.id}" for p, s in RANK_CASES])
def test_rank_grid_params_match_oracle(amd, params, shape):
    cls = "noise"
    bad, paths = _ranks(amd, shape, cls, params)
    assert not bad, f"{params} {shape.id} over ranks ({cls}): fields differ from the oracle: {bad}"
    want = {"x2": S.expect_x2(shape), "x4": S.expect_x4(shape, cls, 1, peers=True)}
    got = [{k: f[-1][k] for k in want} for f in paths]
    assert got == [want] * len(paths), (paths, want)


@pytest.mark.parametrize("params", S.CORE_PARAMS)
def test_ensemble_params_match_oracle(amd, params):
    """Six members of three variants (tests/shapes.py COAST_ENSEMBLE_CLASSES) in one launch per group, as
    tests/test_gpu_coast.py test_ensemble_coasts_match_oracle asserts them."""
    shape, classes, calls = S.PARAM_ENSEMBLE, S.COAST_ENSEMBLE_CLASSES, [2, 5]
    e = _start(amd, shape, classes, params)
    try:
        infos, launches, st = _calls(e, calls, params=params)
        bad = _bad(e, shape, classes, sum(calls), params)
    finally:
        e.close()
    assert st == [OK] * len(classes) and not bad, (st, bad)
    assert [(i["groups"], i["batched"]) for i in infos] == [(0, 0), (3, len(classes))], infos
    assert infos[1]["max_group"] == 4, infos[1]
    assert launches[1] == 3, launches   # one launch per group, nothing else


# ---------------------------------------------------------------- the other sets: one pass each
@pytest.mark.parametrize("mode", OTHER_MODES)
@pytest.mark.parametrize("params", S.OTHER_PARAMS)
def test_single_block_other_params_match_oracle(amd, params, mode):
    failures = _single_failures(amd, OTHER_SINGLE, mode, SINGLE_CLASSES, params)
    assert not failures, f"{params} {OTHER_SINGLE.id} ({mode}): " + "; ".join(failures)


@pytest.mark.parametrize("params", S.OTHER_PARAMS)
def test_block_grid_other_params_match_oracle(amd, params):
    failures = _grid_failures(amd, OTHER_GRID, 1, 1, classes=GRID_CLASSES, params=params)
    assert not failures, f"{params} {OTHER_GRID.id}: " + "; ".join(failures)


# ---------------------------------------------------------------- the rotated sphere
@pytest.mark.parametrize("shape", S.PARAM_ROT, ids=[s.id for s in S.PARAM_ROT])
def test_rotated_grid_runs_the_array_path(amd, shape):
    """rlh_s varies along a row, so the compact tables cannot hold it: no compact static fields, no
    one-pass steps in any call, and the 2-D-array path's results bitwise the oracle's."""
    params, calls = "rot", [2, 5]
    failures = []
    for cls in (SINGLE_CLASSES if shape.grid == (1, 1) else GRID_CLASSES):
        m = _model(amd, shape, params=params)
        try:
            path = _drive(m, shape, cls, calls, params=params)
            compact = m.compact_active
            get = S.model_getter([m])
            ref = S.reference(shape, cls, sum(calls), params=params)
            assert get.blocks == set(ref), (get.blocks, set(ref))
            bad = S.mismatches(ref, get)
        finally:
            m.close()
        if bad:
            failures.append(f"{cls}: fields differ from the oracle: {bad}")
        if compact or any(p["one"] for p in path):
            failures.append(f"{cls}: compact_active {compact}, path flags {path}: wanted neither compact tables "
                            "nor one-pass steps")
    assert not failures, f"rot {shape.id}: " + "; ".join(failures)


# ---------------------------------------------------------------- flags off at a tau that is no power of two
@pytest.mark.parametrize("flags", FLAG_SETTINGS, ids=["ffs%d_trans%d_ksw%d" % f for f in FLAG_SETTINGS])
def test_flag_settings_match_oracle_at_tau03(amd, flags):
    """The role-flip / stage paths' a / tau (sw_stencils.h qtau): no one-pass steps in any call, as
    tests/test_gpu_coast.py test_flag_settings_match_oracle asserts; both overlap levels."""
    params, shape, cls, calls = FLAG_PARAMS, FLAG_SHAPE, "noise", [2, 5]
    ref = S.reference(shape, cls, sum(calls), flags, params)
    for overlap in (1, 2):
        m = _model(amd, shape, overlap=overlap, params=params, flags=flags)
        try:
            path = _drive(m, shape, cls, calls, params=params)
            get = S.model_getter([m])
            assert get.blocks == set(ref), (get.blocks, set(ref))
            bad = S.mismatches(ref, get)
        finally:
            m.close()
        assert not bad, f"{shape.id} flags {flags} overlap {overlap}: fields differ from the oracle: {bad}"
        assert not any(p["one"] for p in path), (flags, path)


# ---------------------------------------------------------------- tau changes across the variant boundary
@pytest.mark.parametrize("reads", [False, True], ids=["unread", "read_each_call"])
@pytest.mark.parametrize("layout", list(TAU_LAYOUTS))
def test_tau_changes_between_calls_match_oracle(amd, layout, reads):
    """step(3, 1.0), step(2, 0.3), step(1, 0.3), step(3, 2.0), step(2, 0.75): P2 with inv_tau = 1, not P2,
    P2 with inv_tau = 0.5, not P2.  unread: after the first call's synchronize() (the known-constant
    verdict) nothing synchronizes or reads until the end, so a call's tail stays pending into the next
    call wherever the library defers it, and must be formed with its own call's tau and variant.
    read_each_call: ssh is read and compared after every call."""
    shape, opts, want = TAU_LAYOUTS[layout]
    cls, calls = TAU_CLASS, S.TAU_CALLS
    refs = S.reference_calls(shape, cls, calls)
    failures, paths = [], []
    m = _model(amd, shape, **opts)
    try:
        m.init()
        for b in m.blocks:
            for nm, a in S.uploads_for(shape, cls).get((b.bm, b.bn), {}).items():
                m.upload(b.k, nm, a)
        get = S.model_getter([m])
        assert get.blocks == set(refs[-1]), (get.blocks, set(refs[-1]))
        for i, (n, tau) in enumerate(calls):
            m.step(n, tau=tau, check_every=1)
            if i == 0:
                m.synchronize()   # the known-constant verdict reaches the host
            paths.append({"one": m.onepass_active, "multi": m.multi_active, "pair": m.pair_active, "x2": m.x2_active})
            if reads and i < len(calls) - 1:
                bad = S.mismatches(refs[i], get)
                if bad:
                    failures.append(f"after call {i} {(n, tau)}: {bad}")
        m.synchronize()
        bad = S.mismatches(refs[-1], get)
    finally:
        m.close()
    if bad:
        failures.append(f"at the end: fields differ from the oracle: {bad}")
    got = {i: {k: paths[i][k] for k in w} for i, w in want.items()}
    if got != want:
        failures.append(f"path flags per call {paths}, wanted {want}")
    assert not failures, f"{shape.id} ({layout}): " + "; ".join(failures)
