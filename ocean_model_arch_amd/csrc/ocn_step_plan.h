// ocn_step_plan.h -- which launches an ocn_ctx_step call makes: pure host code, no HIP, so that it also
// builds into a stand-alone program and a test library (tests/native/step_plan_host.cpp).
//
// A call has phases, each with device work in ocn_ctx.hip: prepare_static (the compact tables), the vote
// (check_coherence), prepare_kc (the one-pass variant) and await_kc (its verdict).  StepFacts is the
// snapshot step_facts() takes of the context: options, the sw switches, shape and state that no phase of
// the call changes once it is taken.  What the vote and prepare_kc leave -- Vote, Kc -- is an argument of
// the function that needs it, never a member of the snapshot.  No function here writes anything but its
// result, and none allocates.
#pragma once
#include <cstdint>

namespace ocn {

#ifndef OCN_KC_DEFINED   // also in ocn_internal.h (the launchers' variant)
#define OCN_KC_DEFINED
enum { OCN_KC_GENERAL = 0, OCN_KC_KNOWN = 1, OCN_KC_DEVICE = 2, OCN_KC_KNOWN_HR = 3 };
#endif

// What one step of an ocn_ctx_step call runs: check = check_ssh_err; first / last step of the
// call; flip = role-flip step; a_done = its fused A already ran (fused into the previous step's
// hh_init launch); next_a = fuse the next step's fused A into this step's hh_init (MarchCA),
// next_reuse = the next step is a reuse step; rc = recompute steps (fused B forms hhq, hhu_p,
// hhv_p itself and writes sshp's filter into the second sshp buffer), rc_next = the next step is
// one (this step's hh_init + A launch then does not store hhq on the interior, hhu_p, hhv_p).
// one = one-pass step (sw_kernels.hip MarchStep), next_one = the next step is one (this step
// then runs no hh_init: the one-pass step forms hh_init's values itself).
// x2 = the one-pass step as one_step_x2 (2-deep state exchange, whole-interior march); x2_save = the
// first of a sequence (the reference's second halo ring of the state is saved first); x2_end = a
// last step after such a sequence (that ring restored and the state's first ring exchanged first).
// pair = this one-pass step and the next as one launch (one_step_pair), check2 = the next one's check.
// multi = this many one-pass steps in one launch (one_step_multi), each checked if check.
struct StepKind {
    bool check, first, last, flip, a_done, next_a, next_reuse, rc, rc_next, one, next_one, one_last;
    bool x2, x2_save, x2_end;
    bool pair = false, check2 = false;
    int multi = 0;
    bool operator==(const StepKind &o) const
    {
        return check == o.check && first == o.first && last == o.last && flip == o.flip && a_done == o.a_done &&
               next_a == o.next_a && next_reuse == o.next_reuse && rc == o.rc && rc_next == o.rc_next &&
               one == o.one && next_one == o.next_one && one_last == o.one_last && x2 == o.x2 &&
               x2_save == o.x2_save && x2_end == o.x2_end && pair == o.pair && check2 == o.check2 && multi == o.multi;
    }
};

struct StepFacts {
    // the options (OCN_OPT_*); forced: the ensemble writes this member's forcing for each step's own time
    bool onepass, lazy, multi, x2, flip, recompute, known_const, last_hybrid, use_graph, stage_timing, tr_step;
    bool compact, march, fused, forced;
    int pair, x4;
    // the sw switches
    int full_free_surface, trans_terms, ksw_lat, use_tracers;
    // shape: the rank's blocks; exchanges between blocks; a communicator, with peers on other ranks; a8 / a9
    // work on the halo ring, on a ring no neighbour fills; the x2 rows' and the x4 tables' divisors in range;
    // the smallest nx_end - nx_start or ny_end - ny_start over the grid's blocks; every block's rows padded
    // for the x4 rings; block 0's interior points; block 0's grid resident at once (onepass_multi_fits)
    int nblocks;
    bool has_exchange, has_comm, remote_peers, ring_sea, edge_ring_sea, rows_x_ok, x4_tab_ok;
    int min_extent;
    bool x4_pitch_ok;
    long cells0;
    bool multi_fits;
    // state: a raw r8 pointer handed out; reuse steps allowed; hh_init's stored depths match the state; the
    // one-pass row divisors in udiv's range; an x2 sequence's second halo ring is saved
    bool r8_handed, reuse_allowed, hh_consistent, udiv_ok, ring2_saved;
};

// what the last vote (check_coherence) left, or the context's own answers where none was taken
struct Vote { bool coherent, udiv_ok, first_one, x2_ok; };
// what prepare_kc left: the call's one-pass variant, and whether pairs of x2 steps may run (every rank's
// vote; the known-constant check covered the x2 range)
struct Kc { int mode; bool x4_dev_ok, fb_x2; };

// a captured graph replays the step (RCCL / events stay outside graphs; so do the tracer steps' calls:
// their launches follow pending state)
inline bool graph_ok(const StepFacts &f)
{
    return f.use_graph && !f.has_comm && !f.stage_timing && !(f.use_tracers > 0 && f.tr_step);
}

// Role-flip steps possible on this rank (ocn_ctx.hip flip_eligible)
inline bool flip_eligible(const StepFacts &f) { return f.flip && f.fused && f.compact && f.march; }

// one_step_pair possible in this call: one block without exchanges or ring work, the compact tables
// and the march, the one-pass variant chosen by the host (kc_mode not OCN_KC_DEVICE; OCN_OPT_PAIR 1:
// a known-constant one on blocks of 512^2 or more, 2: any)
#ifndef OCN_PAIR_MIN_CELLS
#define OCN_PAIR_MIN_CELLS (512L * 512L)
#endif
inline bool pair_ok(const StepFacts &f, int kc_mode)
{
    if (f.forced) return false;   // (a pair would defer steps whose forcing belongs to another time)
    if (!f.pair || f.nblocks != 1 || f.has_exchange || f.has_comm || f.ring_sea || !f.compact || !f.march ||
        f.use_tracers > 0)
        return false;
    if (kc_mode == OCN_KC_DEVICE) return false;   // (the variant the launches run is chosen on the device)
    if (f.pair >= 2) return true;
    // the default: the known-constant variants only -- the general variant's pair is VALU bound at
    // twice its single launch (4096^2: 1.09 vs 0.54 ms), no faster
    if (kc_mode == OCN_KC_GENERAL) return false;
    return f.cells0 >= OCN_PAIR_MIN_CELLS;
}

// one_step_multi possible in this call (an open sequence, pairs not used): one block without exchanges or
// ring work, the compact tables and the march, the variant chosen on the host, every step checked or
// none, and a block small enough that its grid is resident at once -- the launch-latency-bound case
inline bool multi_ok(const StepFacts &f, int kc_mode, int32_t check_every)
{
    return f.multi && f.use_tracers <= 0 && f.nblocks == 1 && !f.has_exchange && !f.has_comm && !f.ring_sea &&
           f.compact && f.march && kc_mode != OCN_KC_DEVICE && (check_every == 0 || check_every == 1) && f.multi_fits;
}

// Lazy call tail possible: single process (a tail formed on one rank only would unbalance the
// exchanges), no raw r8 pointers handed out, no tracers (expl_tracer reads hh_init's arrays after
// every step), and the one-pass step as one launch per block (no exchange, no a8 / a9 work on the
// halo ring: the redone step must find the previous state intact).
inline bool lazy_allowed(const StepFacts &f, bool x2)
{
    return f.lazy && !f.has_comm && !f.r8_handed && (f.use_tracers <= 0 || f.tr_step) &&
           (x2 || (!f.ring_sea && !f.has_exchange));
}

// one_step_x2's static conditions on this rank (the device checks come from check_coherence):
// halo exchanges to do, the compact tables with the ext rows, no a8 / a9 work on a ring no neighbour
// fills, every block of the grid at least 2 x 2 (its 2-deep strips lie in its interior)
inline bool x2_local(const StepFacts &f)
{
    return f.x2 && f.compact && f.rows_x_ok && !f.edge_ring_sea && f.has_exchange && f.min_extent >= 1;
}

// one_step_x4's static conditions on this rank (with x2_local's): its tables, no tracers (expl_tracer
// after every step), the known-constant variant allowed, every block of the grid at least 4 x 4 (its
// 4-deep strips lie in its interior) and row padding for the extra rings
inline bool x4_local(const StepFacts &f)
{
    // (tracer runs: with the tracer steps, one_step_x4 runs them -- by default only where exchanges go to
    // other ranks: a pair's second tracer step is one more launch after it, which with only local copies
    // costs more than the exchange it saves -- C5 layout on one GPU 0.0281 (x2) vs 0.0338 ms per step,
    // profiles/r06a; over RCCL each exchange is a group's latency)
    if (!f.x4 || !f.x4_tab_ok || !f.known_const || f.r8_handed || (f.use_tracers > 0 && !f.tr_step) || !f.march)
        return false;
    if (f.use_tracers > 0 && f.x4 < 3 && !f.remote_peers) return false;
    return f.min_extent >= 3 && f.x4_pitch_ok;
}
// pairs of x2 steps in this call (after prepare_kc): x4_local on every rank (the vote) or this one
// (one process), the known-constant variant chosen on the host
inline bool x4_now(const StepFacts &f, const Kc &kc)
{
    return (kc.mode == OCN_KC_KNOWN || kc.mode == OCN_KC_KNOWN_HR) &&
           (f.has_comm ? kc.x4_dev_ok : x4_local(f) && kc.fb_x2);
}
// two steps per launch in a call of one-pass steps: pairs of x2 steps (one_step_x4), or one_step_pair
inline bool pairs_now(const StepFacts &f, const Kc &kc, bool x2) { return x2 ? x4_now(f, kc) : pair_ok(f, kc.mode); }

// The first call of a sequence long enough for pairs, right after prepare_kc issued the known-
// constant check: wait for the check's verdict (one host wait per check -- the check's pass over
// the fields and a 4-byte copy, behind whatever the stream holds) so that the call's steps run as
// pairs of the host-chosen variant instead of single launches of both variants with the device
// picking (4096^2: 0.39 ms per single step against 0.28-0.30 ms per step in pairs; the single
// steps' HBM traffic also pulls the shader clock down, 2.25 -> 1.55 GHz over 5 ms, and the pairs'
// clock climbs back over ~30 ms: profiles/r06/clock_*.txt).  Not with a communicator (the ranks' votes
// carry the verdicts), not for calls of 1-3 steps (no pair before their deferred last steps); the
// question is put with the variant the wait could bring.  (ocn_ctx.hip await_kc adds: the verdict's copy
// is under way, no graph is being captured.)
inline bool await_kc_pays(const StepFacts &f, Kc kc, bool x2, int nsteps)
{
    if (kc.mode != OCN_KC_DEVICE || f.has_comm || nsteps < 4) return false;
    kc.mode = OCN_KC_KNOWN;
    return pairs_now(f, kc, x2);
}

// The step kinds of an open sequence and of the tail that ends one.
// A continuing one-pass step: nothing around its launch, the next step is one too
inline StepKind continuing_step(bool check, bool x2)
{
    StepKind k{};
    k.check = check;
    k.flip = k.one = k.next_one = k.a_done = true;
    k.x2 = x2;   // (an x2 sequence: one_step_x2, as a pair one_step_x4)
    return k;
}
// two of them as one launch (one_step_pair, one_step_x4)
inline StepKind continuing_pair(bool check, bool check2, bool x2)
{
    StepKind k = continuing_step(check, x2);
    k.pair = true;
    k.check2 = check2;
    return k;
}
// nsteps of them as one launch (one_step_multi), each checked if check
inline StepKind multi_step(bool check, int nsteps)
{
    StepKind k = continuing_step(check, false);
    k.multi = nsteps;
    return k;
}
// The call's last step after one-pass steps.  It ends a sequence of x2 steps: the saved second ring is
// restored and the first exchanged before it (x2_end), here and nowhere else -- the caller stores
// ring2_saved = false
inline StepKind last_step(bool check, bool ring2_saved)
{
    StepKind k{};
    k.last = k.one_last = true;
    k.check = check;
    k.x2_end = ring2_saved;
    return k;
}
// a one-pass step and the last step as one launch (one_step_pair with LAST: one block, no exchange)
inline StepKind last_pair(bool check, bool check2)
{
    StepKind k{};
    k.last = k.one_last = k.pair = true;
    k.check = check;
    k.check2 = check2;
    return k;
}
// step s of a call is checked
inline bool check_at(int s, int32_t check_every) { return check_every > 0 && s % check_every == 0; }

// ---- a fresh call: no open sequence goes on

// with RCCL every rank takes part in the decisions: the vote is taken before the plan (coherent_known: the
// pairs' coherence was checked after the state last changed outside ocn_ctx_step)
inline bool fresh_votes(const StepFacts &f, int nsteps, bool coherent_known)
{
    const bool eligible = flip_eligible(f);
    // a lazy call is planned as the first nsteps steps of a call of nsteps + 1 (the last deferred)
    const int N = eligible && f.onepass && lazy_allowed(f, x2_local(f)) ? nsteps + 1 : nsteps;
    return N >= 2 && (eligible || (f.has_comm && f.flip)) && !coherent_known;
}

// the call's constants: the steps run are 1..nsteps of a call of N steps (N = nsteps + 1: a lazy call, the
// tail stays pending); pairs / x4_call are known only after prepare_kc (fresh_pairs)
struct FreshPlan {
    int nsteps, N;
    bool first_one, flip_call, ca, one_call, x2_call, lazy_end, last_one, rc_call, pairs, x4_call, graph;
};
inline FreshPlan plan_fresh(const StepFacts &f, const Vote &v, int nsteps)
{
    FreshPlan p{};
    const bool eligible = flip_eligible(f);
    const bool lazy_cand = eligible && f.onepass && lazy_allowed(f, x2_local(f));
    // tracer runs with one-pass steps (tracer steps): the call's first step a one-pass step too, and
    // with exchanges the x2 steps (their exchange carries the tracers); one block: no ring work
    // and the last step a one-pass step (last_one below: it runs the pending tracer step)
    const bool tr_ok = f.use_tracers <= 0 ||
                       (f.tr_step && v.first_one &&
                        (f.has_exchange ? v.x2_ok && f.last_hybrid
                                        : !f.ring_sea && (f.last_hybrid || (f.nblocks == 1 && !f.has_comm))));
    auto decide = [&](int n) {
        p.N = n;
        p.flip_call = n >= 2 && eligible && v.coherent && (f.full_free_surface != 1 || f.reuse_allowed);
        // role-flip calls with full_free_surface = 1 fuse each step's hh_init with the next step's A;
        // their reuse steps recompute hhq / hhu_p / hhv_p in fused B, which then filters sshp into
        // the second buffer (the ring launch completes it on the halo ring)
        p.ca = p.flip_call && f.full_free_surface == 1;
        // one-pass steps 2..K-1 (all SW terms on, no tracers: expl_tracer reads hh_init's hhu / hhv /
        // hhq_p, which a one-pass step keeps in registers; row divisors in udiv's range) -- the first
        // step too when hh_init's stored depths match the state (hh_consistent)
        p.one_call = p.ca && f.onepass && (n >= 3 || (n >= 2 && v.first_one)) && f.trans_terms > 0 &&
                     f.ksw_lat > 0 && tr_ok && v.udiv_ok;
        // one-pass steps with one 2-deep exchange each (one_step_x2) where there are exchanges
        p.x2_call = p.one_call && v.x2_ok && f.last_hybrid;   // (its sequences end in the hybrid last step)
        // the last step run is a one-pass step (one launch per block, or an x2 step): the tail may wait
        p.lazy_end = lazy_cand && p.one_call && (nsteps >= 2 || v.first_one) &&
                     (p.x2_call || (!f.ring_sea && !f.has_exchange));
    };
    decide(lazy_cand ? nsteps + 1 : nsteps);
    if (!p.lazy_end && p.N != nsteps) decide(nsteps);
    p.nsteps = nsteps;
    p.first_one = v.first_one;
    // the last step as one march + hh_init too (single block, no exchange, no ring work)
    // (with exchanges or ring work: the hybrid last step, OCN_OPT_ONEPASS_LAST)
    p.last_one = p.one_call && ((f.nblocks == 1 && !f.has_exchange && !f.has_comm && !f.ring_sea) || f.last_hybrid);
    p.rc_call = p.ca && f.recompute && !p.one_call;
    p.graph = graph_ok(f);
    return p;
}
// two one-pass steps per launch where both are plain one-pass steps and the second is not the
// last one run (a lazy tail redoes that one from the state before it, which a pair never writes)
// (with exchanges: pairs of x2 steps with one 4-deep exchange each, one_step_x4)
inline FreshPlan fresh_pairs(const StepFacts &f, FreshPlan p, const Kc &kc)
{
    p.x4_call = p.one_call && p.x2_call && x4_now(f, kc);
    p.pairs = p.one_call && (p.x2_call ? p.x4_call : pair_ok(f, kc.mode));
    return p;
}

// step s (1-based) of the plan's call: its kind, the steps it runs (2: step s + 1 folded into a pair) and the
// x2 sequence's ring state behind it
struct FreshStep { StepKind k; int steps; bool ring2_saved; };
inline FreshStep fresh_step(const FreshPlan &p, int s, int32_t check_every, bool ring2_saved)
{
    const int N = p.N;
    auto plain_one = [&](int t) {   // step t is a one-pass step that needs nothing around its launch
        const bool one = p.one_call && (t >= 2 || p.first_one) && t <= N - 1, next_one = p.one_call && t + 1 <= N - 1;
        const bool next_a = p.ca && p.flip_call && t != N && !next_one && !(p.last_one && t + 1 == N);
        return one && !next_a && !(p.last_one && t == N);
    };
    StepKind k{};
    k.check = check_at(s, check_every);
    k.first = s == 1;
    k.last = s == N;
    k.flip = p.flip_call && !k.last;
    k.one = p.one_call && (s >= 2 || p.first_one) && s <= N - 1;
    k.next_one = p.one_call && s + 1 <= N - 1;
    k.one_last = p.last_one && k.last;
    k.a_done = p.ca && !k.first;
    k.next_a = p.ca && k.flip && !k.next_one && !(p.last_one && s + 1 == N);
    k.next_reuse = k.next_a && s + 1 < N;
    k.rc = p.rc_call && k.flip && !k.first;
    k.rc_next = p.rc_call && s + 1 < N;
    k.x2 = p.x2_call && k.one;
    k.x2_save = k.x2 && !ring2_saved;
    k.x2_end = k.one_last && ring2_saved;
    if (k.x2_save) ring2_saved = true;
    if (k.x2_end) ring2_saved = false;
    int steps = 1;
    if (p.pairs && k.one && s + 1 < p.nsteps && plain_one(s + 1)) {
        k.pair = true;
        k.check2 = check_at(s + 1, check_every);
        k.next_one = p.one_call && s + 2 <= N - 1;
        k.next_a = k.next_reuse = false;
        steps = 2;
    }
    return FreshStep{k, steps, ring2_saved};
}

// ---- a call while a sequence is open

// the open sequence goes on: every step of this call is a one-pass step (the state and the constants
// are what its last step left), and the tail stays pending; else the tail is formed and the call is fresh
inline bool open_goes_on(const StepFacts &f, bool same_tau, bool open_x2)
{
    return same_tau && f.onepass && lazy_allowed(f, open_x2);
}

// The call's launches (after prepare_kc): pairs -- two steps per launch, the steps deferred by the last
// call first, while 3 or more are pending; the last 1 or 2 deferred (next call, complete_open) --, or
// the deferred steps and then all the call's steps in one launch (multi), or one by one (singles).
// emit(kind, graph) takes the kinds in order; graph: a captured graph may replay it (never a deferred
// step run alone); it returns false to stop (a launch failed: the caller drops the sequence).
// go: no deferred step runs ahead of the call's first one.
enum { kOpenPairs = 0, kOpenMulti = 1, kOpenSingles = 2 };
struct OpenPlan { int mode, deferred; bool deferred_check[2], go; };
template <class Emit>
inline OpenPlan plan_open(const StepFacts &f, const Kc &kc, bool open_x2, int deferred, const bool deferred_check[2],
                          int32_t nsteps, int32_t check_every, Emit &&emit)
{
    OpenPlan p{kOpenSingles, 0, {false, false}, deferred == 0};
    const bool graph = graph_ok(f);
    // pending step i: a deferred one, or the call's step i - deferred + 1
    auto chk = [&](int i) { return i < deferred ? deferred_check[i] : check_at(i - deferred + 1, check_every); };
    if (pairs_now(f, kc, open_x2)) {
        p.mode = kOpenPairs;
        const int64_t total = (int64_t)deferred + nsteps;
        int i = 0;
        for (; (int64_t)i + 2 < total; i += 2)
            if (!emit(continuing_pair(chk(i), chk(i + 1), open_x2), graph)) return p;
        p.deferred = (int)(total - i);   // 1 or 2
        for (int j = 0; j < p.deferred; ++j) p.deferred_check[j] = chk(i + j);
        return p;
    }
    for (int j = 0; j < deferred; ++j)   // (no pairs now: deferred steps first)
        if (!emit(continuing_step(deferred_check[j], open_x2), false)) return p;
    if (!open_x2 && !graph && nsteps >= 2 && multi_ok(f, kc.mode, check_every)) {
        p.mode = kOpenMulti;
        emit(multi_step(check_every == 1, nsteps), false);
        return p;
    }
    for (int s = 1; s <= nsteps; ++s)
        if (!emit(continuing_step(check_at(s, check_every), open_x2), graph)) return p;
    return p;
}

// ---- the pending tail of an open sequence (complete_open)

// Deferred steps are run as the last ones, from the current state: both in one launch (pair + LAST), or
// (x2 sequences with pairs of x2 steps: one_step_x4 deferred them) a single and the last step.  Else
// the last launch is run again from the state before it (swap_back: the roles return first) as the
// call's last step; a pair: both again, the second as the last step (counted the first time: no
// checks), or (a pair of x2 steps) its first step again, then the last step.
// ring2_saved: the x2 sequence's ring state behind the tail.
struct TailPlan { bool swap_back; int n; StepKind k[2]; bool ring2_saved; };
inline TailPlan plan_tail(int deferred, const bool deferred_check[2], bool open_pair, bool open_x2, bool pair_ok,
                          bool ring2_saved)
{
    TailPlan t{deferred == 0, 0, {}, ring2_saved};
    const bool c0 = deferred ? deferred_check[0] : false, c1 = deferred == 2 ? deferred_check[1] : false;
    if ((deferred == 2 || (!deferred && open_pair)) && pair_ok) {
        t.k[t.n++] = last_pair(c0, c1);
        return t;
    }
    if (deferred == 2 || (!deferred && open_pair)) t.k[t.n++] = continuing_step(c0, open_x2);
    t.k[t.n++] = last_step(deferred ? deferred_check[deferred - 1] : false, ring2_saved);
    t.ring2_saved = false;
    return t;
}

}  // namespace ocn
