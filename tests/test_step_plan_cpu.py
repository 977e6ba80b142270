"""CPU checks of the step planner (ocean_model_arch_amd/csrc/ocn_step_plan.h through
tests/native/step_plan_host.cpp): which launches an ocn_ctx_step call makes.  Pure host code, no device.

* the walk over the planner's input grid with what holds for any correct plan (the native program's, run
  through the library);
* the planner against a restatement of the rule as it stood before it became functions of its own --
  step_impl, complete_open, probe_multi and their predicates, transcribed below with the context as a
  namespace of the facts -- on a seeded sample of fact vectors and on the shipped situations: every field
  of every kind, and the sequence state behind the call;
* the probe's answers against what the open plan then does; purity."""
import ctypes as C
import os
import random
import subprocess
from types import SimpleNamespace

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "tests", "native", "libstep_plan_host.so")

# StepFacts' members in their order (step_plan_host.cpp facts_of)
FACTS = ["onepass", "lazy", "multi", "x2", "flip", "recompute", "known_const", "last_hybrid", "use_graph",
         "stage_timing", "tr_step", "compact", "march", "fused", "forced", "pair", "x4", "full_free_surface",
         "trans_terms", "ksw_lat", "use_tracers", "nblocks", "has_exchange", "has_comm", "remote_peers", "ring_sea",
         "edge_ring_sea", "rows_x_ok", "x4_tab_ok", "min_extent", "x4_pitch_ok", "cells0", "multi_fits", "r8_handed",
         "reuse_allowed", "hh_consistent", "udiv_ok", "ring2_saved"]
# a kind's integers (step_plan_host.cpp put_kind): StepKind's members, then whether a graph may replay it
KIND = ["check", "first", "last", "flip", "a_done", "next_a", "next_reuse", "rc", "rc_next", "one", "next_one",
        "one_last", "x2", "x2_save", "x2_end", "pair", "check2", "multi", "graph"]
GENERAL, KNOWN, DEVICE, KNOWN_HR = 0, 1, 2, 3
PAIRS, MULTI, SINGLES = 0, 1, 2
PAIR_MIN_CELLS = 512 * 512
CAP = 128


@pytest.fixture(scope="module")
def sp():
    subprocess.check_call(["make", "-s", "-f", os.path.join(REPO, "tests", "native", "Makefile")], cwd=REPO)
    L = C.CDLL(LIB)
    ip = C.POINTER(C.c_int32)
    L.sp_fresh.argtypes = [ip, ip, ip, C.c_int, ip, C.c_int, C.c_int, ip, C.c_int, ip]
    L.sp_open.argtypes = [ip, ip] + [C.c_int] * 7 + [ip, C.c_int, ip]
    L.sp_probe.argtypes = [ip, ip] + [C.c_int] * 7
    L.sp_tail.argtypes = [ip] + [C.c_int] * 6 + [ip, ip]
    L.sp_await.argtypes = [ip, ip, C.c_int, C.c_int]
    L.sp_walk.restype = C.c_long
    L.sp_walk.argtypes = [C.POINTER(C.c_long)]
    return L


def ints(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def kinds_of(buf, n):
    return [tuple(buf[i * len(KIND):(i + 1) * len(KIND)]) for i in range(n)]


# ---- the planner through the library

def new_fresh(L, c, own, voted, coherent_known, kc, nsteps, ce):
    fv, buf, st = ints([getattr(c, n) for n in FACTS]), (C.c_int32 * (CAP * len(KIND)))(), (C.c_int32 * 10)()
    before = list(fv)
    n = L.sp_fresh(fv, ints(own), ints(voted), int(coherent_known), ints(kc), nsteps, ce, buf, CAP, st)
    assert n >= 0 and list(fv) == before
    keys = ["voted", "N", "flip_call", "one_call", "x2_call", "lazy_end", "rc_call", "x4_call", "pairs", "ring2_saved"]
    return kinds_of(buf, n), dict(zip(keys, st))


def new_open(L, c, kc, same_tau, open_x2, d, dc, nsteps, ce):
    fv, buf, st = ints([getattr(c, n) for n in FACTS]), (C.c_int32 * (CAP * len(KIND)))(), (C.c_int32 * 6)()
    before = list(fv)
    n = L.sp_open(fv, ints(kc), int(same_tau), int(open_x2), d, int(dc[0]), int(dc[1]), nsteps, ce, buf, CAP, st)
    assert n >= 0 and list(fv) == before
    if not st[0]:
        return None
    return kinds_of(buf, n), dict(mode=st[1], deferred=st[2], deferred_check=[st[3], st[4]][:st[2]], go=st[5])


def new_probe(L, c, kc, same_tau, open_x2, d, dc, nsteps, ce):
    r = L.sp_probe(ints([getattr(c, n) for n in FACTS]), ints(kc), int(same_tau), int(open_x2), d, int(dc[0]), int(dc[1]),
                   nsteps, ce)
    return bool(r & 1), bool(r & 2)


def new_tail(L, c, kc_mode, d, dc, open_pair, open_x2):
    buf, st = (C.c_int32 * (3 * len(KIND)))(), (C.c_int32 * 2)()
    n = L.sp_tail(ints([getattr(c, n) for n in FACTS]), kc_mode, d, int(dc[0]), int(dc[1]), int(open_pair), int(open_x2), buf, st)
    return kinds_of(buf, n), dict(swap_back=st[0], ring2_saved=st[1])


# ---- the rule as it stood: ocn_ctx.hip before the planner, c = the context (the facts, kc_mode, x4_dev_ok,
# fb_x2, coherent, x2_dev_ok, coherent_known, open_x2, open_pair, deferred, deferred_check)

def kind(**kw):
    k = dict.fromkeys(KIND, 0)
    k.update({n: int(v) for n, v in kw.items()})
    return k


def tup(k, graph):
    return tuple(k[n] for n in KIND[:-1]) + (int(graph),)


def old_pair_ok(c):
    if c.forced:
        return False
    if (not c.pair or c.nblocks != 1 or c.has_exchange or c.has_comm or c.ring_sea or not c.compact or not c.march or
            c.use_tracers > 0):
        return False
    if c.kc_mode == DEVICE:
        return False
    if c.pair >= 2:
        return True
    if c.kc_mode == GENERAL:
        return False
    return c.cells0 >= PAIR_MIN_CELLS


def old_multi_ok(c, check_every):
    return bool(c.multi and c.use_tracers <= 0 and c.nblocks == 1 and not c.has_exchange and not c.has_comm and
                not c.ring_sea and c.compact and c.march and c.kc_mode != DEVICE and check_every in (0, 1) and c.multi_fits)


def old_lazy_allowed(c, x2):
    return bool(c.lazy and not c.has_comm and not c.r8_handed and (c.use_tracers <= 0 or c.tr_step) and
                (x2 or (not c.ring_sea and not c.has_exchange)))


def old_x2_local(c):
    if not c.x2 or not c.compact or not c.rows_x_ok or c.edge_ring_sea or not c.has_exchange:
        return False
    return not c.min_extent < 1   # (no block of the grid with an extent below 1)


def old_x4_local(c):
    if (not c.x4 or not c.x4_tab_ok or not c.known_const or c.r8_handed or (c.use_tracers > 0 and not c.tr_step) or
            not c.march):
        return False
    if c.use_tracers > 0 and c.x4 < 3 and not c.remote_peers:   # (has_comm(c) && c->dec.nranks > 1)
        return False
    if c.min_extent < 3:
        return False
    return bool(c.x4_pitch_ok)


def old_x4_now(c):
    return c.kc_mode in (KNOWN, KNOWN_HR) and bool(c.x4_dev_ok if c.has_comm else old_x4_local(c) and c.fb_x2)


def old_graph_ok(c):
    return bool(c.use_graph and not c.has_comm and not c.stage_timing and not (c.use_tracers > 0 and c.tr_step))


def old_await_waits(c, x2, nsteps):
    """await_kc up to its host wait (fb_copy and capturing are the context's own)"""
    if c.kc_mode != DEVICE or c.has_comm or nsteps < 4:
        return False
    c.kc_mode = KNOWN
    pairs = old_x4_now(c) if x2 else old_pair_ok(c)
    c.kc_mode = DEVICE
    return pairs


def continuing_step(check, x2):
    return kind(check=check, flip=1, one=1, next_one=1, a_done=1, x2=x2)


def continuing_pair(check, check2, x2):
    return dict(continuing_step(check, x2), pair=1, check2=int(check2))


def multi_step(check, nsteps):
    return dict(continuing_step(check, False), multi=nsteps)


def last_step(c, check):
    k = kind(last=1, one_last=1, check=check, x2_end=c.ring2_saved)
    c.ring2_saved = 0
    return k


def last_pair(check, check2):
    return kind(last=1, one_last=1, pair=1, check=check, check2=check2)


def old_complete_open(c):
    """the kinds complete_open runs, whether the roles swap back first (c.open holds)"""
    if c.deferred:
        d = c.deferred
        c.deferred = 0
        c.open_pair = False
        if d == 2 and old_pair_ok(c):
            return [last_pair(c.deferred_check[0], c.deferred_check[1])], False
        ks = []
        if d == 2:
            ks.append(continuing_step(c.deferred_check[0], c.open_x2))
        return ks + [last_step(c, c.deferred_check[d - 1])], False
    ks = []
    if c.open_pair:
        c.open_pair = False
        if old_pair_ok(c):
            return [last_pair(False, False)], True
        ks.append(continuing_step(False, c.open_x2))
    return ks + [last_step(c, False)], True


def set_kc(c, kc):
    c.kc_mode, c.x4_dev_ok, c.fb_x2 = kc   # (what prepare_kc leaves)


def old_probe_multi(c, same_tau, nsteps, check_every, kc):
    if not same_tau or not c.onepass or not old_lazy_allowed(c, c.open_x2):
        return False, False
    go = c.deferred == 0
    set_kc(c, kc)
    pairs = old_x4_now(c) if c.open_x2 else old_pair_ok(c)
    return bool(not pairs and not c.open_x2 and not old_graph_ok(c) and nsteps >= 2 and old_multi_ok(c, check_every)), go


def old_step_open(c, same_tau, nsteps, check_every, kc):
    """step_impl's open branch: None if the sequence ends, else the kinds (with their graph flag) and the mode"""
    graph_ok = old_graph_ok(c)
    if not (same_tau and c.onepass and old_lazy_allowed(c, c.open_x2)):
        return None
    set_kc(c, kc)
    pairs = old_x4_now(c) if c.open_x2 else old_pair_ok(c)
    out = []
    if pairs:
        mode = PAIRS
        chk = list(c.deferred_check[:c.deferred])
        for s in range(1, nsteps + 1):
            chk.append(int(check_every > 0 and s % check_every == 0))
        c.deferred = 0
        i = 0
        while i + 2 < len(chk):
            out.append(tup(continuing_pair(chk[i], chk[i + 1], c.open_x2), graph_ok))
            c.open_pair = True
            i += 2
        c.deferred = len(chk) - i
        c.deferred_check = chk[i:]
    else:
        for j in range(c.deferred):
            out.append(tup(continuing_step(c.deferred_check[j], c.open_x2), False))
        c.deferred = 0
        c.deferred_check = []
        if not c.open_x2 and not graph_ok and nsteps >= 2 and old_multi_ok(c, check_every):
            mode = MULTI
            out.append(tup(multi_step(check_every == 1, nsteps), False))
            c.open_pair = False
        else:
            mode = SINGLES
            for s in range(1, nsteps + 1):
                out.append(tup(continuing_step(check_every > 0 and s % check_every == 0, c.open_x2), graph_ok))
                c.open_pair = False
    return out, mode


def old_step_fresh(c, voted, nsteps, check_every, kc):
    """step_impl behind prepare_static: voted = the verdicts a vote brings (coherent, udiv_ok, hh_consistent, x2_ok)"""
    graph_ok = old_graph_ok(c)
    eligible = bool(c.flip and c.fused and c.compact and c.march)
    x2_here = old_x2_local(c)
    lazy_cand = eligible and c.onepass and old_lazy_allowed(c, x2_here)
    udiv_ok, first_one, x2_ok = c.udiv_ok, c.hh_consistent, x2_here and c.x2_dev_ok
    N = nsteps + 1 if lazy_cand else nsteps
    votes = bool(N >= 2 and (eligible or (c.has_comm and c.flip)) and not c.coherent_known)
    if votes:
        c.coherent, udiv_ok, first_one = voted[0], voted[1], voted[2]
        x2_ok = x2_here and voted[3]
    tr_ok = c.use_tracers <= 0 or (c.tr_step and first_one and
                                   (x2_ok and c.last_hybrid if c.has_exchange else
                                    not c.ring_sea and (c.last_hybrid or (c.nblocks == 1 and not c.has_comm))))

    def decide(n):
        flip_call = n >= 2 and eligible and c.coherent and (c.full_free_surface != 1 or c.reuse_allowed)
        ca = flip_call and c.full_free_surface == 1
        one_call = (ca and c.onepass and (n >= 3 or (n >= 2 and first_one)) and c.trans_terms > 0 and c.ksw_lat > 0 and
                    tr_ok and udiv_ok)
        return bool(flip_call), bool(ca), bool(one_call)
    flip_call, ca, one_call = decide(N)
    x2_call = bool(one_call and x2_ok and c.last_hybrid)
    lazy_end = bool(lazy_cand and one_call and (nsteps >= 2 or first_one) and
                    (x2_call or (not c.ring_sea and not c.has_exchange)))
    if not lazy_end and N != nsteps:
        N = nsteps
        flip_call, ca, one_call = decide(N)
    last_one = bool(one_call and ((c.nblocks == 1 and not c.has_exchange and not c.has_comm and not c.ring_sea) or
                                  c.last_hybrid))
    if one_call:
        set_kc(c, kc)
    rc_call = bool(ca and c.recompute and not one_call)
    x4_call = bool(one_call and x2_call and old_x4_now(c))
    pairs = bool(one_call and (x4_call if x2_call else old_pair_ok(c)))

    def plain_one(s):
        one = one_call and (s >= 2 or first_one) and s <= N - 1
        next_one = one_call and s + 1 <= N - 1
        next_a = ca and flip_call and s != N and not next_one and not (last_one and s + 1 == N)
        return one and not next_a and not (last_one and s == N)
    out = []
    s = 1
    while s <= nsteps:
        k = kind()
        k["check"] = int(check_every > 0 and s % check_every == 0)
        k["first"] = int(s == 1)
        k["last"] = int(s == N)
        k["flip"] = int(flip_call and not k["last"])
        k["one"] = int(one_call and (s >= 2 or first_one) and s <= N - 1)
        k["next_one"] = int(one_call and s + 1 <= N - 1)
        k["one_last"] = int(last_one and k["last"])
        k["a_done"] = int(ca and not k["first"])
        k["next_a"] = int(ca and k["flip"] and not k["next_one"] and not (last_one and s + 1 == N))
        k["next_reuse"] = int(k["next_a"] and s + 1 < N)
        k["rc"] = int(rc_call and k["flip"] and not k["first"])
        k["rc_next"] = int(rc_call and s + 1 < N)
        k["x2"] = int(x2_call and k["one"])
        k["x2_save"] = int(k["x2"] and not c.ring2_saved)
        k["x2_end"] = int(k["one_last"] and c.ring2_saved)
        if k["x2_save"]:
            c.ring2_saved = 1
        if k["x2_end"]:
            c.ring2_saved = 0
        if pairs and k["one"] and s + 1 < nsteps and plain_one(s + 1):
            k["pair"] = 1
            k["check2"] = int(check_every > 0 and (s + 1) % check_every == 0)
            k["next_one"] = int(one_call and s + 2 <= N - 1)
            k["next_a"] = k["next_reuse"] = 0
            s += 1
        out.append(tup(k, graph_ok))
        s += 1
    st = dict(voted=int(votes), N=N, flip_call=int(flip_call), one_call=int(one_call), x2_call=int(x2_call and one_call),
              lazy_end=int(lazy_end), rc_call=int(rc_call), x4_call=int(x4_call), pairs=int(pairs),
              ring2_saved=int(c.ring2_saved))
    return out, st


# ---- the cases

def shipped():
    """the facts of the shipped situations, by name"""
    box = dict(onepass=1, lazy=1, multi=1, x2=1, flip=1, recompute=1, known_const=1, last_hybrid=1, use_graph=0,
               stage_timing=0, tr_step=1, compact=1, march=1, fused=1, forced=0, pair=1, x4=1, full_free_surface=1,
               trans_terms=1, ksw_lat=1, use_tracers=0, nblocks=1, has_exchange=0, has_comm=0, remote_peers=0, ring_sea=0,
               edge_ring_sea=0, rows_x_ok=0, x4_tab_ok=0, min_extent=4095, x4_pitch_ok=1, cells0=4096 * 4096, multi_fits=0,
               r8_handed=0, reuse_allowed=1, hh_consistent=1, udiv_ok=1, ring2_saved=0)
    bs = dict(box, min_extent=131, cells0=286 * 132, multi_fits=1)
    blocks = dict(box, nblocks=8, has_exchange=1, rows_x_ok=1, x4_tab_ok=1, min_extent=1023, cells0=1024 * 2048)
    return {"box4096": box, "black sea": bs, "black sea, a tracer": dict(bs, use_tracers=1),
            "4x2 blocks": blocks, "ranks": dict(blocks, nblocks=2, has_comm=1, remote_peers=1),
            "forced member": dict(bs, forced=1), "r8 handed": dict(box, r8_handed=1, hh_consistent=0),
            "graph": dict(box, use_graph=1), "graph, black sea": dict(bs, use_graph=1)}


def sample(rng):
    """a fact vector: a shipped situation with some facts redrawn, and what the phases leave"""
    f = dict(rng.choice(list(shipped().values())))
    for n in FACTS:
        if rng.random() < 0.07:
            f[n] = {"pair": rng.choice([0, 1, 2]), "x4": rng.choice([0, 1, 3]), "nblocks": rng.choice([1, 2]),
                    "min_extent": rng.choice([0, 2, 5]), "cells0": rng.choice([100 * 100, 4096 * 4096])}.get(n, 1 - min(f[n], 1))
    f["ring2_saved"] = 0   # (no sequence is under way at a fresh call; the open calls and tails set it below)
    c = SimpleNamespace(**f)
    c.kc = (rng.choice([KNOWN, KNOWN, KNOWN, GENERAL, DEVICE, KNOWN_HR]), int(rng.random() < 0.8), int(rng.random() < 0.8))
    c.own = [int(rng.random() < 0.85) for _ in range(2)]   # (the context's coherent and x2_dev_ok)
    c.voted = [int(rng.random() < 0.85) for _ in range(4)]
    c.coherent_known = int(rng.random() < 0.5)
    c.nsteps = rng.choice([1, 1, 2, 3, 4, 5, 7, 100])
    c.check_every = rng.choice([0, 0, 1, 2, 3])
    c.same_tau = int(rng.random() < 0.9)
    c.open_x2 = int(f["has_exchange"] and rng.random() < 0.8)
    c.deferred = rng.choice([0, 0, 1, 2])
    c.deferred_check = [rng.randrange(2) for _ in range(c.deferred)]
    c.open_pair = rng.randrange(2)
    return c


def ctx_of(c, **kw):
    """the context the old rule runs on: the sample's facts and state (a copy; the old rule writes to it)"""
    o = SimpleNamespace(**vars(c))
    o.deferred_check = list(c.deferred_check)
    o.kc_mode, o.x4_dev_ok, o.fb_x2 = c.kc
    o.coherent, o.x2_dev_ok = c.own
    for n, v in kw.items():
        setattr(o, n, v)
    return o


def check_case(L, c, seen):
    dc2 = (c.deferred_check + [0, 0])[:2]
    # a fresh call
    want, wst = old_step_fresh(ctx_of(c), c.voted, c.nsteps, c.check_every, c.kc)
    got, gst = new_fresh(L, c, c.own, c.voted, c.coherent_known, c.kc, c.nsteps, c.check_every)
    assert (got, gst) == (want, wst), vars(c)
    assert new_fresh(L, c, c.own, c.voted, c.coherent_known, c.kc, c.nsteps, c.check_every) == (got, gst)
    seen["x2 call"] += wst["x2_call"]
    seen["x4 call"] += wst["x4_call"]
    seen["lazy end"] += wst["lazy_end"]
    seen["non-lazy last step"] += int(not wst["lazy_end"] and want[-1][KIND.index("last")])
    seen["recompute call"] += wst["rc_call"]
    seen["standard call"] += int(not wst["flip_call"])
    seen["fresh pairs"] += wst["pairs"]
    # the await question, with the variant still on the device
    for x2 in (0, 1):
        a = ctx_of(c, kc_mode=DEVICE)
        assert bool(L.sp_await(ints([getattr(c, n) for n in FACTS]), ints((DEVICE,) + c.kc[1:]), x2, c.nsteps)) == \
            old_await_waits(a, x2, c.nsteps), vars(c)
        assert a.kc_mode == DEVICE
    # a call while a sequence is open (an x2 sequence has its ring saved)
    o = ctx_of(c, ring2_saved=c.open_x2)
    f = ctx_of(c, ring2_saved=c.open_x2)
    want = old_step_open(o, c.same_tau, c.nsteps, c.check_every, c.kc)
    got = new_open(L, f, c.kc, c.same_tau, c.open_x2, c.deferred, dc2, c.nsteps, c.check_every)
    probe = new_probe(L, f, c.kc, c.same_tau, c.open_x2, c.deferred, dc2, c.nsteps, c.check_every)
    assert probe == old_probe_multi(ctx_of(c), c.same_tau, c.nsteps, c.check_every, c.kc), vars(c)
    if want is None:
        assert got is None and probe == (False, False), vars(c)
    else:
        kinds, mode = want
        assert got[0] == kinds, vars(c)
        assert got[1] == dict(mode=mode, deferred=o.deferred, deferred_check=list(o.deferred_check), go=int(c.deferred == 0))
        assert got == new_open(L, f, c.kc, c.same_tau, c.open_x2, c.deferred, dc2, c.nsteps, c.check_every)
        # the probe against what the plan then does: one multi-step kind behind the deferred steps; the first kind
        # the call's own
        multi_kinds = [k for k in kinds if k[KIND.index("multi")]]
        assert probe[0] == (mode == MULTI) == (len(multi_kinds) == 1) and len(multi_kinds) <= 1, vars(c)
        assert probe[1] == (c.deferred == 0), vars(c)
        seen[("pairs", "multi", "singles")[mode] + " mode"] += 1
    # the tail
    o = ctx_of(c, ring2_saved=c.open_x2)
    shape = "deferred" if c.deferred else "pair" if c.open_pair else "plain"
    kinds, swap = old_complete_open(o)
    got = new_tail(L, f, c.kc[0], c.deferred, dc2, c.open_pair, c.open_x2)
    assert got == ([tup(k, False) for k in kinds], dict(swap_back=int(swap), ring2_saved=int(o.ring2_saved))), vars(c)
    assert len(kinds) <= 3
    seen["tail: " + shape] += 1


NEEDED = ["pairs mode", "multi mode", "singles mode", "x2 call", "x4 call", "lazy end", "non-lazy last step",
          "recompute call", "standard call", "tail: deferred", "tail: pair", "tail: plain"]


def test_walk(sp):
    checked = C.c_long(0)
    assert sp.sp_walk(C.byref(checked)) == 0
    assert checked.value > 10 ** 9


def test_sample_matches_the_old_rule(sp):
    rng = random.Random(20261021)
    seen = dict.fromkeys(NEEDED + ["fresh pairs"], 0)
    for _ in range(10000):
        check_case(sp, sample(rng), seen)
    assert all(seen[n] >= 20 for n in NEEDED), seen


@pytest.mark.parametrize("name", list(shipped()))
def test_shipped_situations_match_the_old_rule(sp, name):
    f = shipped()[name]
    seen = dict.fromkeys(NEEDED + ["fresh pairs"], 0)
    topo = [KNOWN_HR, GENERAL]   # a topography: the rest depth varies (the h_r-read variant), or nothing known
    for kc_mode in [KNOWN, DEVICE] + topo:
        for nsteps in (1, 2, 3, 4, 7, 100):
            for ce in (0, 1, 3):
                for d, dc in ((0, []), (1, [1]), (2, [0, 1])):
                    for open_pair in ((0, 1) if d == 0 else (0,)):
                        c = SimpleNamespace(**f)
                        c.kc = (kc_mode, int(f["has_comm"]), int(f["has_exchange"]))
                        c.own = [1, f["has_exchange"]]
                        c.voted = [1, f["udiv_ok"], f["hh_consistent"], f["has_exchange"]]
                        c.coherent_known = int(not f["has_comm"])
                        c.nsteps, c.check_every, c.same_tau = nsteps, ce, 1
                        c.open_x2, c.deferred, c.deferred_check, c.open_pair = f["has_exchange"], d, dc, open_pair
                        check_case(sp, c, seen)
    # what each situation ships as
    want = {"box4096": ["pairs mode", "lazy end"], "black sea": ["multi mode", "lazy end"],
            "black sea, a tracer": ["singles mode", "lazy end"], "4x2 blocks": ["x2 call", "x4 call", "pairs mode"],
            "ranks": ["x2 call", "x4 call", "non-lazy last step"], "forced member": ["multi mode"],
            "r8 handed": ["non-lazy last step"], "graph": ["pairs mode"], "graph, black sea": ["singles mode"]}[name]
    assert all(seen[n] for n in want), seen
    if name == "forced member":
        assert not seen["pairs mode"] and not seen["fresh pairs"]
    if name in ("ranks", "r8 handed"):
        assert not seen["lazy end"]
