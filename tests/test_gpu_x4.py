"""GPU parity of the pairs of x2 steps (OCN_OPT_X4, ocn_ctx.hip one_step_x4): blocks with halo
exchanges run two one-pass steps per launch with ONE exchange of the state four points deep per two
steps -- the launch's first step also updates the two halo rings neighbour blocks own, as they do --
bitwise against the reference fixtures (its step exchanges 15 fields at 7 sync points per step:
shared/mpp/syncborder_block2D_gen_all.fi:100-129 after every stage, core/kernel_interface.f90:105-117).

The pairs run the known-constant variant the host has chosen, so every run makes a first short call
and a synchronize() (the check's verdict reaches the host), then the rest.  One process with several
blocks (local copies, the lazy call tail: pairs across calls) and loopback ranks (the RCCL path's
plans, exchanges and vote; one call per run after the first).  Tolerance: none.
"""
import pytest

from tests.golden import cases
from tests.test_gpu_parity import build_model, compare_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import ocean_model_arch_amd as amd
    amd.lib()
    return amd


def _run_blocks(amd, name, calls, x4=True, overlap=None):
    case = cases.load_e2e(name)
    m = build_model(amd, case, overlap=overlap).set_x4(x4).init()
    used = []
    try:
        m.step(calls[0], tau=1.0, check_every=1)
        m.synchronize()   # the known-constant verdict reaches the host
        for n in calls[1:]:
            m.step(n, tau=1.0, check_every=1)
            used.append(m.x4_active)
        m.synchronize()
        bad = compare_case(m, case, name)
    finally:
        m.close()
    return bad, used


@pytest.mark.parametrize("name,calls", [("box70x54_b3x2_s20", [2, 18]), ("box70x54_b3x2_s20", [2, 5, 1, 1, 3, 8]),
                                        ("box70x54_b3x2_s20", [1] * 20), ("bs_b4x2_s60", [2, 58]),
                                        ("bs_b4x2_s60", [3, 1, 1, 1, 54]), ("box40x32_b2x2_s5", [2, 3]),
                                        ("box2048_b2x2_s4", [1, 3]), ("box4096_b4x2_s4", [1, 3]),
                                        ("box2048_b2x2_s10", [2, 8]), ("box4096_b4x2_s12", [2, 10])])
def test_x4_blocks_match_reference(amd, name, calls):
    """Several blocks in one process (local halo copies): pairs of x2 steps inside calls and across
    calls (the reference's 1-step cadence: a pair every second call), every field bitwise."""
    bad, used = _run_blocks(amd, name, calls)
    assert not bad, f"{name} {calls}: fields differ from the reference: {bad}"
    assert any(used), used


@pytest.mark.parametrize("name,calls", [("box70x54_b3x2_s20", [2, 18]), ("bs_b4x2_s60", [2, 5, 1, 52]),
                                        ("box4096_b4x2_s4", [1, 3])])
def test_x4_overlapped_blocks_match_reference(amd, name, calls):
    """OCN_OPT_OVERLAP 2 (the default with remote peers): each block's inner pair on the compute stream
    beside the 4-deep exchange, then the bands around it on the comm stream -- bitwise."""
    bad, used = _run_blocks(amd, name, calls, overlap=2)
    assert not bad, f"{name} {calls}: fields differ from the reference: {bad}"
    assert any(used), used


@pytest.mark.parametrize("name,calls", [("box70x54_b3x2_tr_s20", [2, 18]), ("box70x54_b3x2_tr_s20", [2, 5, 1, 1, 3, 8]),
                                        ("box70x54_b3x2_tr_s20", [1] * 20), ("bs_b4x2_tr_s60", [2, 58]),
                                        ("bs_b4x2_tr_s60", [3, 1, 1, 1, 54]), ("bs_b4x2_tr_s604", [2, 602])])
@pytest.mark.parametrize("overlap", [None, 2])
def test_x4_tracer_blocks_match_reference(amd, name, calls, overlap):
    """Tracer runs with x4 pairs (one_step_x4 with tracer steps): the exchange carries the tracers 2
    deep, the pending tracer step runs over the interior and the halo ring neighbours own (co-launched
    with the pair), the pair's producers write the first step's state for the second tracer step --
    two SW steps and two tracer steps per exchange, every field bitwise (control/tracer.f90:33-62 after
    each step, leapfrog_tracer.f90:13-170)."""
    bad, used = _run_blocks(amd, name, calls, x4=3, overlap=overlap)
    assert not bad, f"{name} {calls}: fields differ from the reference: {bad}"
    assert any(used), used


def test_x4_tracer_runs_in_one_process_default_to_x2(amd):
    """OCN_OPT_X4 auto (1): a tracer run whose exchanges are all local copies keeps the x2 steps (the
    pair's second tracer step costs a launch more than the exchange it saves), bitwise."""
    bad, used = _run_blocks(amd, "box70x54_b3x2_tr_s20", [2, 18])
    assert not bad and not any(used), (bad, used)


@pytest.mark.parametrize("name,calls", [("box70x54_topo_b3x2_s20", [2, 18]), ("box70x54_topo_b3x2_s20", [2, 5, 1, 1, 3, 8]),
                                        ("bs_topo_b4x2_s60", [2, 58])])
@pytest.mark.parametrize("overlap", [None, 2])
def test_x4_topography_blocks_match_reference(amd, name, calls, overlap):
    """A rest depth read from a topography file (control/init_data.f90:115-120): the pairs run the
    h_r-read variant (OCN_KC_KNOWN_HR) with h_r's copy exchanged four rings deep (refresh_hrx) -- every
    field bitwise."""
    bad, used = _run_blocks(amd, name, calls, overlap=overlap)
    assert not bad, f"{name} {calls}: fields differ from the reference: {bad}"
    assert any(used), used


def test_x4_off_is_the_x2_path(amd):
    bad, used = _run_blocks(amd, "box70x54_b3x2_s20", [2, 18], x4=False)
    assert not bad and not any(used), (bad, used)


def _run_ranks(amd, name, nranks, calls, overlap=None, co=None):
    """One block per loopback rank, the bench's cadence (a first call, a synchronize: the
    known-constant verdict reaches every host, so the next call's vote can choose the pairs), then
    the remaining calls, complete() and a synchronize.  Returns (differing fields, per rank the
    x4_active of each later call, per rank whether a later call co-launched a march and a tracer step)."""
    case = cases.load_e2e(name)
    models = [build_model(amd, case, rank=r, nranks=nranks, overlap=overlap) for r in range(nranks)]
    if co is not None:
        for m in models:
            m.set_co_launch(co)
    amd.OceanModel.attach_loopback(models)

    def body(m):
        m.init()
        m.step(calls[0], tau=1.0, check_every=1)
        m.synchronize()
        used, co_used = [], False
        for n in calls[1:]:
            m.step(n, tau=1.0, check_every=1)
            used.append(m.x4_active)
            co_used = co_used or m.co_launched
        m.complete()
        m.synchronize()
        return used, co_used

    try:
        res = amd.run_ranks(models, body)
        bad = []
        for m in models:
            bad += compare_case(m, case, name, whole=False)
    finally:
        for m in models:
            m.close()
    return bad, [r[0] for r in res], [r[1] for r in res]


@pytest.mark.parametrize("name,nranks,calls", [("box70x54_b3x2_s20", 6, [2, 18]), ("bs_b4x2_s60", 8, [2, 58]),
                                               ("box40x32_b2x2_s5", 4, [2, 3]), ("box70x54_b3x2_s20", 6, [2, 7, 3, 8]),
                                               ("bs_b4x2_tr_s60", 8, [2, 58]), ("box70x54_b3x2_tr_s20", 6, [2, 7, 3, 8]),
                                               ("box70x54_topo_b3x2_s20", 6, [2, 18]), ("bs_topo_b4x2_s60", 8, [2, 58])])
def test_x4_ranks_match_reference(amd, name, nranks, calls):
    """One block per loopback rank: the exchange is the RCCL path's (device pack / unpack, per-peer
    messages 4 deep), the decision every rank's (the vote's x4 word), every field bitwise.  (With a
    communicator a call runs pairs after a call of 2 or more steps has voted with the verdict known.)"""
    bad, used, _ = _run_ranks(amd, name, nranks, calls)
    assert not bad, f"{name} over {nranks} ranks {calls}: fields differ from the reference: {bad}"
    assert all(any(u) for u in used) and all(u == used[0] for u in used), used


@pytest.mark.parametrize("overlap", [1, 2])
@pytest.mark.parametrize("name,nranks,calls", [("box2048_b2x2_s10", 4, [2, 8]), ("box4096_b4x2_s12", 8, [2, 10])])
def test_x4_fullsize_ranks_match_reference(amd, name, nranks, calls, overlap):
    """BASELINE configs 3 and 4 at full size, one block per loopback rank, exactly as a multi-GPU bench
    run executes them: the warm-up call, then one long call of x4 pairs (every rank asserts it ran
    them), complete(); overlap 2 = the inner pair beside the 4-deep exchange then the bands (the
    default with peers), overlap 1 = exchange then the whole pair.  Every field of every block
    bitwise against the reference's 4 / 8-block run (shared/mpp/syncborder_block2D_gen_all.fi:100-129,
    core/kernel_interface.f90:105-117)."""
    bad, used, _ = _run_ranks(amd, name, nranks, calls, overlap=overlap)
    assert not bad, f"{name} over {nranks} ranks, overlap {overlap}: fields differ from the reference: {bad}"
    assert all(all(u) for u in used), used


@pytest.mark.parametrize("overlap", [1, 2])
@pytest.mark.parametrize("name,calls", [("bs_b4x2_tr_s60", [2, 58]), ("bs_b4x2_tr_s604", [2, 602])])
def test_x4_tracer_ranks_co_launch_match_reference(amd, name, calls, overlap):
    """Config 5 (Black Sea + tracer, 8 blocks) over 8 loopback ranks with x4 pairs and the tracer steps:
    the tracers exchanged 2 deep with the state, the pending tracer step co-launched with the pair
    (overlap 2: in the bands' launch after the exchange; overlap 1: with the whole pair) -- every rank
    ran the pairs and the co-launch, every field bitwise (control/tracer.f90:33-62,
    interface/tracer/tracer_interface.f90:52-98)."""
    bad, used, co = _run_ranks(amd, name, 8, calls, overlap=overlap, co=True)
    assert not bad, f"{name} over 8 ranks, overlap {overlap}: fields differ from the reference: {bad}"
    assert all(all(u) for u in used), used
    assert all(co), co


def test_x4_counts_blowup_like_single_launches(amd):
    """check_ssh_err (vel_ssh.f90:40-67) in the pairs: each point counted once per step -- a producer
    counts its workgroup's interior points, never the halo points it updates for a neighbour: the same
    count as the x2 single launches."""
    import numpy as np
    msgs = []
    for x4 in (True, False):
        m = amd.OceanModel(amd.box_config(120), par=amd.ParallelConfig(3, 2)).set_x4(x4).init()
        m.step(2, check_every=1).synchronize()
        for b in m.blocks:   # a hot patch straddling the block boundaries
            s = m.download(b.k, "ssh")
            i = np.arange(b.bnd_x1, b.bnd_x2 + 1)[:, None]
            j = np.arange(b.bnd_y1, b.bnd_y2 + 1)[None, :]
            s[(abs(i - 42) < 9) & (abs(j - 62) < 9)] = 2.0e4
            for nm in ("ssh", "sshn", "sshp"):
                m.upload(b.k, nm, s)
        m.step(2, check_every=0).synchronize()   # the re-check's verdict reaches the host
        with pytest.raises(amd.OcnError) as e:
            m.step(5, check_every=1)
            used = m.x4_active
            m.synchronize()
        msgs.append(str(e.value))
        m.close()
        assert used == x4
    assert msgs[0] == msgs[1], msgs


@pytest.mark.parametrize("delay_us", [0, 600])
def test_overlap_choice_is_measured_and_voted(amd, delay_us):
    """OCN_OPT_OVERLAP auto with peers on other ranks (ocn_ctx.hip ov_begin): one x2 step in sequence
    and the next overlapped, each timed; the next call's vote max-reduces both times and every rank
    keeps the faster form -- every rank decides, all the same, the level is the one the compared
    times pick, and an injected 600 us wait before each exchange (a slow link) is in the measured
    sequential step.  (Which form wins is not asserted: four loopback ranks share one GPU, and their
    step times carry the other ranks' work and the transport's cross-rank waits.)  Either way every
    field bitwise against the reference's 4-block run (core/kernel_interface.f90:105-117 is the
    reference's own overlap mode)."""
    name, calls = "box2048_b2x2_s10", [4, 2, 4]
    case = cases.load_e2e(name)
    models = [build_model(amd, case, rank=r, nranks=4) for r in range(4)]
    for m in models:
        m.set_exchange_delay(delay_us)
    amd.OceanModel.attach_loopback(models)

    def body(m):
        m.init()
        infos = []
        for n in calls:
            m.step(n, tau=1.0, check_every=1)
            infos.append(m.overlap_info())
        m.complete()
        m.synchronize()
        return infos

    try:
        infos = amd.run_ranks(models, body)
        bad = []
        for m in models:
            bad += compare_case(m, case, name, whole=False)
    finally:
        for m in models:
            m.close()
    assert not bad, f"{name} delay {delay_us}: fields differ from the reference: {bad}"
    last = [i[-1] for i in infos]
    print("overlap", delay_us, last)
    assert all(i["state"] == 3 for i in last), last
    assert len({i["level"] for i in last}) == 1 and len({(i["seq_ms"], i["overlapped_ms"]) for i in last}) == 1, last
    i0 = last[0]
    assert i0["level"] == (2 if i0["overlapped_ms"] < i0["seq_ms"] else 1), last
    if delay_us:
        assert i0["seq_ms"] > delay_us * 1e-3 and i0["overlapped_ms"] > 0.0, last


# ---------------------------------------------------------------- the overlap choice settles
def _overlap_settles(amd, shape, nranks, first, n):
    """OCN_OPT_OVERLAP auto over loopback ranks on the `noise` class: first calls of `first` steps, a
    synchronize() after each, then calls of n steps -- OVERLAP_MAX_VOTES voting calls in all
    (ocn_overlap_info: the bound after which the choice is final one way or the other), then two more.
    Returns per rank the overlap_info after every call; every field of every block is compared bitwise
    with the oracle."""
    from ocean_model_arch_amd._lib import OVERLAP_MAX_VOTES
    from tests import shapes as S
    from tests.test_gpu_shapes import _model
    calls = list(first) + [n] * (OVERLAP_MAX_VOTES - len(first) + 2)
    models = [_model(amd, shape, rank=r, nranks=nranks) for r in range(nranks)]
    ups = S.uploads_for(shape, "noise")

    def body(m):
        m.init()
        for b in m.blocks:
            for nm, a in ups.get((b.bm, b.bn), {}).items():
                m.upload(b.k, nm, a)
        infos = []
        for i, k in enumerate(calls):
            m.step(k, tau=1.0, check_every=1)
            if i < len(first):
                m.synchronize()
            infos.append(m.overlap_info())
        m.synchronize()
        return infos

    try:
        amd.OceanModel.attach_loopback(models)
        infos = amd.run_ranks(models, body)
        bad = S.mismatches(S.reference(shape, "noise", sum(calls)), S.model_getter(models))
    finally:
        for m in models:
            m.close()
    print("overlap", shape.id, nranks, calls, [[(i["state"], i["level"], i["kind"], i["probes"]) for i in r] for r in infos])
    assert not bad, f"{shape.id} over {nranks} ranks {calls}: fields differ from the oracle: {bad}"
    at = OVERLAP_MAX_VOTES - 1   # the info after the last of the bounded voting calls
    for r in infos:
        assert r[at]["state"] in (3, 4), (r[at], "not final after OVERLAP_MAX_VOTES voting calls")
        assert r[at]["state"] == 3 or r[at]["level"] == 2, r[at]   # (gave up: level 2)
        for later in r[at + 1:]:   # final: neither the state nor the level moves, and no step is a probe
            assert (later["state"], later["level"], later["kind"], later["probes"]) == \
                (r[at]["state"], r[at]["level"], r[at]["kind"], r[at]["probes"]), (r[at], later)
    assert len({(r[at]["state"], r[at]["level"], r[at]["probes"]) for r in infos}) == 1, [r[at] for r in infos]
    return infos


@pytest.mark.parametrize("first", [(2,), (2, 2)], ids=["first2", "first2_2"])
@pytest.mark.parametrize("w,h,grid,nranks", [(17, 12, (3, 1), 3), (23, 12, (4, 1), 2), (17, 19, (2, 2), 4)])
def test_overlap_choice_settles_on_uneven_ranks(amd, w, h, grid, nranks, first):
    """Ranks whose blocks differ in what they allow (tests/shapes.py RANK_LAYOUTS: the x4 inner part is
    empty on rank 1 only / on a block of each rank; 2 x 2 equal blocks beside them) and calls of 6 steps,
    which mix x4 pairs with a single x2 step: the measured choice (ocn_ctx.hip ov_begin, check_coherence)
    must become final on every rank, the same level everywhere, and no step be a probe after that.
    first2: one 2-step call, then the 6-step calls -- the first of those runs x2 steps only (the known-
    constant verdict reaches the vote a call later), which is enough to measure both forms of the x2 kind
    before any pair runs.  first2_2: two 2-step calls, each followed by synchronize() -- the pairs run from
    the first 6-step call on, so every measuring call mixes the two kinds (and on 17 x 12 the ranks
    differ in whether their own blocks could overlap a pair): the case the choice once never left."""
    from tests import shapes as S
    _overlap_settles(amd, S.Shape(w, h, grid), nranks, first, 6)


@pytest.mark.parametrize("first", [(2,), (2, 2)], ids=["first2", "first2_2"])
@pytest.mark.parametrize("n", [5, 3])
def test_overlap_choice_settles_with_short_calls(amd, n, first):
    """Calls [2, 5, 5, ...] and [2, 3, 3, ...] on 2 x 2 blocks over 4 ranks (first2_2: [2, 2, 5, ...] and
    [2, 2, 3, ...] with the pairs from the first longer call on): a call of 3 steps with pairs is an opening
    pair and the last step -- no step that may be timed -- so the choice has to give up (state 4, level 2)
    unless the x2 steps before the first pairs were enough to decide."""
    from tests import shapes as S
    _overlap_settles(amd, S.Shape(17, 19, (2, 2)), 4, first, n)


def test_x4_option_reads_back_as_set(amd):
    """ocn_ctx_get_option(OCN_OPT_X4): 0, 1 or 3 as set while the last call ran no pairs, 2 after one that
    did (x4_active)."""
    from ocean_model_arch_amd import _lib
    m = amd.OceanModel(amd.box_config(40), par=amd.ParallelConfig(2, 2))
    try:
        assert m.option(_lib.OPT_X4) == 1 and not m.x4_active
        for on, want in ((3, 3), (False, 0), (True, 1), (0, 0), (3, 3)):
            m.set_x4(on)
            assert m.option(_lib.OPT_X4) == want and not m.x4_active, (on, want)
        m.init()
        m.step(2, check_every=1).synchronize()
        m.step(6, check_every=1)
        assert m.x4_active and m.option(_lib.OPT_X4) == 2
        m.set_x4(False)
        m.step(3, check_every=1)
        assert not m.x4_active and m.option(_lib.OPT_X4) == 0
        m.synchronize()
    finally:
        m.close()
