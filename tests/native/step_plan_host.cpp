// Host harness of the step planner (ocean_model_arch_amd/csrc/ocn_step_plan.h): flat-integer entry points
// for tests/test_step_plan_cpu.py and, with -DSTEP_PLAN_MAIN, a stand-alone program that walks the
// planner's input grid and checks what holds for any correct plan (a sanitizer build of it runs on the CPU).
//
// The walk.  The literal product of every boolean fact with every other axis has more than 2^40 points, so
// it is taken per planner function over the facts that function reads, which loses nothing because the
// functions are pure and take their inputs by value or const reference:
//   * plan_fresh over every combination of the facts and verdicts it reads, nsteps 1..7 -- its constants'
//     invariants, and the set of distinct FreshPlans it can return;
//   * fresh_step over every distinct FreshPlan x pairs x check_every 0..3 x the ring state;
//   * the predicates pair_ok, multi_ok, x4_now and await_kc_pays over all the facts they read, block counts 1
//     and 2, pair 0 / 1 / 2, x4 0 / 1 / 3, every kc_mode (graph_ok through use_graph alone);
//   * plan_open over those facts x open_x2 x deferred 0..2 with every deferred_check x nsteps x check_every;
//   * plan_tail over deferred x checks x open_pair x open_x2 x pair_ok x the ring state;
//   * the chains fresh call -> up to two open calls -> tail, for the x2 ring's saves and ends.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ocean_model_arch_amd/csrc/ocn_step_plan.h"

using namespace ocn;

namespace {

// the facts as the tests pass them, in StepFacts' order (tests/test_step_plan_cpu.py FACTS)
enum { kNumFacts = 38, kKindInts = 19 };
StepFacts facts_of(const int32_t *v)
{
    StepFacts f{};
    int i = 0;
    f.onepass = v[i++]; f.lazy = v[i++]; f.multi = v[i++]; f.x2 = v[i++]; f.flip = v[i++]; f.recompute = v[i++];
    f.known_const = v[i++]; f.last_hybrid = v[i++]; f.use_graph = v[i++]; f.stage_timing = v[i++]; f.tr_step = v[i++];
    f.compact = v[i++]; f.march = v[i++]; f.fused = v[i++]; f.forced = v[i++];
    f.pair = v[i++]; f.x4 = v[i++];
    f.full_free_surface = v[i++]; f.trans_terms = v[i++]; f.ksw_lat = v[i++]; f.use_tracers = v[i++];
    f.nblocks = v[i++];
    f.has_exchange = v[i++]; f.has_comm = v[i++]; f.remote_peers = v[i++]; f.ring_sea = v[i++];
    f.edge_ring_sea = v[i++]; f.rows_x_ok = v[i++]; f.x4_tab_ok = v[i++];
    f.min_extent = v[i++]; f.x4_pitch_ok = v[i++]; f.cells0 = v[i++]; f.multi_fits = v[i++];
    f.r8_handed = v[i++]; f.reuse_allowed = v[i++]; f.hh_consistent = v[i++]; f.udiv_ok = v[i++]; f.ring2_saved = v[i++];
    static_assert(kNumFacts == 38, "facts");
    return f;
}

// a kind as kKindInts integers: StepKind's members in their order, then whether a graph may replay it
void put_kind(const StepKind &k, bool graph, int32_t *o)
{
    const int32_t v[kKindInts] = {k.check, k.first, k.last, k.flip, k.a_done, k.next_a, k.next_reuse, k.rc, k.rc_next, k.one,
                                  k.next_one, k.one_last, k.x2, k.x2_save, k.x2_end, k.pair, k.check2, k.multi, graph};
    memcpy(o, v, sizeof(v));
}

// a fresh call as step_impl makes it: own = the context's coherent and x2_dev_ok, voted = the four verdicts a vote
// would bring
struct Fresh { FreshPlan p; bool voted; };
Fresh fresh_of(const StepFacts &f, const int32_t *own, const int32_t *voted, bool coherent_known, const Kc &kc, int nsteps)
{
    const bool x2_here = x2_local(f), votes = fresh_votes(f, nsteps, coherent_known);
    const Vote v = votes ? Vote{voted[0] != 0, voted[1] != 0, voted[2] != 0, x2_here && voted[3]}
                         : Vote{own[0] != 0, f.udiv_ok, f.hh_consistent, x2_here && own[1]};
    return Fresh{fresh_pairs(f, plan_fresh(f, v, nsteps), kc), votes};
}

}  // namespace

extern "C" {

// kinds: room for cap kinds of kKindInts integers; state: votes, N, flip_call, one_call, x2_call, lazy_end, rc_call,
// x4_call, pairs, ring2_saved behind the call.  Returns the number of kinds (-1: more than cap).
int sp_fresh(const int32_t *facts, const int32_t *own, const int32_t *voted, int coherent_known, const int32_t *kc,
             int nsteps, int check_every, int32_t *kinds, int cap, int32_t *state)
{
    const StepFacts f = facts_of(facts);
    const Fresh fr = fresh_of(f, own, voted, coherent_known != 0, Kc{kc[0], kc[1] != 0, kc[2] != 0}, nsteps);
    bool ring2 = f.ring2_saved;
    int n = 0;
    for (int s = 1; s <= nsteps;) {
        const FreshStep st = fresh_step(fr.p, s, check_every, ring2);
        if (n >= cap) return -1;
        put_kind(st.k, fr.p.graph, kinds + (size_t)kKindInts * n++);
        ring2 = st.ring2_saved;
        s += st.steps;
    }
    const int32_t out[10] = {fr.voted, fr.p.N, fr.p.flip_call, fr.p.one_call, fr.p.x2_call, fr.p.lazy_end, fr.p.rc_call,
                             fr.p.x4_call, fr.p.pairs, ring2};
    memcpy(state, out, sizeof(out));
    return n;
}

// state: goes_on, mode, deferred, deferred_check[2], go (the probe's answers: mode == kOpenMulti, go)
int sp_open(const int32_t *facts, const int32_t *kc, int same_tau, int open_x2, int deferred, int dc0, int dc1, int nsteps,
            int check_every, int32_t *kinds, int cap, int32_t *state)
{
    const StepFacts f = facts_of(facts);
    const bool dc[2] = {dc0 != 0, dc1 != 0};
    memset(state, 0, 6 * sizeof(int32_t));
    if (!open_goes_on(f, same_tau != 0, open_x2 != 0)) return 0;
    int n = 0;
    bool over = false;
    const OpenPlan p = plan_open(f, Kc{kc[0], kc[1] != 0, kc[2] != 0}, open_x2 != 0, deferred, dc, nsteps, check_every,
                                 [&](const StepKind &k, bool graph) {
                                     if (n >= cap) { over = true; return false; }
                                     put_kind(k, graph, kinds + (size_t)kKindInts * n++);
                                     return true;
                                 });
    const int32_t out[6] = {1, p.mode, p.deferred, p.deferred_check[0], p.deferred_check[1], p.go};
    memcpy(state, out, sizeof(out));
    return over ? -1 : n;
}

// the probe's two answers (ocn_ctx.hip step_probe: the open plan with nothing run), multi + 2 * go
int sp_probe(const int32_t *facts, const int32_t *kc, int same_tau, int open_x2, int deferred, int dc0, int dc1, int nsteps,
             int check_every)
{
    const StepFacts f = facts_of(facts);
    const bool dc[2] = {dc0 != 0, dc1 != 0};
    if (!open_goes_on(f, same_tau != 0, open_x2 != 0)) return 0;
    const OpenPlan p = plan_open(f, Kc{kc[0], kc[1] != 0, kc[2] != 0}, open_x2 != 0, deferred, dc, nsteps, check_every,
                                 [](const StepKind &, bool) { return true; });
    return (p.mode == kOpenMulti) + 2 * p.go;
}

// state: swap_back, ring2_saved behind the tail; kinds: room for 3
int sp_tail(const int32_t *facts, int kc_mode, int deferred, int dc0, int dc1, int open_pair, int open_x2, int32_t *kinds,
            int32_t *state)
{
    const StepFacts f = facts_of(facts);
    const bool dc[2] = {dc0 != 0, dc1 != 0};
    const TailPlan t = plan_tail(deferred, dc, open_pair != 0, open_x2 != 0, pair_ok(f, kc_mode), f.ring2_saved);
    for (int i = 0; i < t.n; ++i) put_kind(t.k[i], false, kinds + (size_t)kKindInts * i);
    state[0] = t.swap_back;
    state[1] = t.ring2_saved;
    return t.n;
}

int sp_await(const int32_t *facts, const int32_t *kc, int x2, int nsteps)
{
    return await_kc_pays(facts_of(facts), Kc{kc[0], kc[1] != 0, kc[2] != 0}, x2 != 0, nsteps);
}

}  // extern "C"

// ---- the walk

namespace {

long g_bad = 0, g_checked = 0;
void expect(bool ok, const char *what)
{
    ++g_checked;
    if (ok) return;
    if (g_bad++ < 20) fprintf(stderr, "step plan walk: %s\n", what);
}

// facts of a plain run: one 4096^2 block, nothing attached, the defaults
StepFacts base_facts()
{
    StepFacts f{};
    f.onepass = f.lazy = f.multi = f.x2 = f.flip = f.recompute = f.known_const = f.last_hybrid = f.tr_step = true;
    f.compact = f.march = f.fused = true;
    f.pair = 1; f.x4 = 1;
    f.full_free_surface = 1; f.trans_terms = 1; f.ksw_lat = 1;
    f.nblocks = 1;
    f.rows_x_ok = f.x4_tab_ok = f.x4_pitch_ok = true;
    f.edge_ring_sea = false;
    f.min_extent = 4095; f.cells0 = 4096L * 4096L;
    f.reuse_allowed = f.hh_consistent = f.udiv_ok = true;
    return f;
}

int steps_of(const StepKind &k) { return k.multi ? k.multi : k.pair ? 2 : 1; }
void kind_rules(const StepKind &k)
{
    expect(!k.last || (!k.flip && !k.one), "a last step with flip or one");
    expect(!k.one_last || k.last, "one_last without last");
    expect(!k.pair || !k.multi, "a pair that is a multi-step kind");
}

// a FreshPlan as an integer: its members, N as N - nsteps
unsigned plan_key(const FreshPlan &p)
{
    const bool b[12] = {p.N != p.nsteps, p.first_one, p.flip_call, p.ca, p.one_call, p.x2_call, p.lazy_end, p.last_one,
                        p.rc_call, p.pairs, p.x4_call, p.graph};
    unsigned k = (unsigned)p.nsteps;
    for (bool v : b) k = k * 2u + v;
    return k;
}

void walk_fresh()
{
    std::vector<char> seen(8u << 12, 0);
    std::vector<FreshPlan> plans;
    // eligible: all of flip / fused / compact / march, or one of them missing (they enter through flip_eligible alone
    // wherever a one-pass call is planned)
    for (int el = 0; el < 5; ++el)
        for (unsigned m = 0; m < (1u << 21); ++m) {   // (17 facts, 4 verdicts)
            StepFacts f = base_facts();
            f.flip = el != 1; f.fused = el != 2; f.compact = el != 3; f.march = el != 4;
            unsigned b = m;
            auto bit = [&] { const bool v = b & 1u; b >>= 1; return v; };
            f.onepass = bit(); f.lazy = bit(); f.has_comm = bit(); f.r8_handed = bit(); f.use_tracers = bit();
            f.tr_step = bit(); f.ring_sea = bit(); f.has_exchange = bit(); f.x2 = bit(); f.full_free_surface = bit();
            f.reuse_allowed = bit(); f.trans_terms = bit(); f.ksw_lat = bit(); f.last_hybrid = bit();
            f.nblocks = bit() ? 2 : 1; f.recompute = bit(); f.use_graph = bit();
            const bool vc = bit(), vu = bit(), vf = bit(), vx = bit();
            const Vote v{vc, vu, vf, vx && x2_local(f)};   // (x2_ok as step_impl forms it)
            for (int nsteps = 1; nsteps <= 7; ++nsteps) {
                FreshPlan p = plan_fresh(f, v, nsteps);
                expect(p.nsteps == nsteps && (p.N == nsteps || p.N == nsteps + 1), "fresh: N");
                expect(p.lazy_end == (p.N == nsteps + 1), "fresh: a lazy end plans nsteps + 1, nothing else does");
                expect(!p.lazy_end || (p.one_call && lazy_allowed(f, p.x2_call)), "fresh: a lazy end without one-pass steps");
                expect(!p.one_call || (p.ca && p.flip_call && flip_eligible(f)), "fresh: one-pass steps outside a role-flip call");
                expect(!p.x2_call || (p.one_call && f.has_exchange && v.x2_ok), "fresh: x2 steps");
                expect(!p.last_one || p.one_call, "fresh: last_one");
                expect(!p.rc_call || (!p.one_call && p.ca), "fresh: recompute steps");
                expect(p.graph == graph_ok(f) && !p.pairs && !p.x4_call, "fresh: graph / pairs before prepare_kc");
                expect(!p.lazy_end || !(f.has_comm || f.r8_handed), "fresh: a lazy end with ranks or raw pointers");
                if (!seen[plan_key(p)]) { seen[plan_key(p)] = 1; plans.push_back(p); }
            }
        }
    printf("fresh: %zu distinct plans\n", plans.size());
    for (const FreshPlan &plan : plans)
        for (int pairs = 0; pairs <= (plan.one_call ? 1 : 0); ++pairs)
            for (int ce = 0; ce <= 3; ++ce)
                for (int r2 = 0; r2 <= 1; ++r2) {
                    FreshPlan p = plan;
                    p.pairs = pairs;
                    p.x4_call = pairs && p.x2_call;
                    bool ring2 = r2, any_x2 = false;
                    int run = 0;
                    for (int s = 1; s <= p.nsteps;) {
                        const FreshStep st = fresh_step(p, s, ce, ring2);
                        const StepKind &k = st.k;
                        kind_rules(k);
                        expect(st.steps == steps_of(k) && !k.multi, "fresh: steps of a kind");
                        expect(k.check == check_at(s, ce) && (!k.pair || k.check2 == check_at(s + 1, ce)), "fresh: checks");
                        expect(!k.pair || (pairs && k.one && s + 1 <= p.nsteps), "fresh: a pair");
                        expect(!k.pair || !p.lazy_end || s + 1 != p.nsteps, "fresh: a pair's second step is the last run of a lazy call");
                        expect(!k.pair || !(k.last || k.one_last || k.next_a), "fresh: a pair with work around it");
                        expect(!k.x2_save || !ring2, "fresh: x2_save with the ring saved");
                        expect(!k.x2_end || ring2, "fresh: x2_end with the ring unsaved");
                        expect(k.x2 == (p.x2_call && k.one), "fresh: x2");
                        any_x2 |= k.x2;
                        ring2 = st.ring2_saved;
                        run += st.steps;
                        s += st.steps;
                    }
                    expect(run == p.nsteps, "fresh: the kinds cover nsteps steps");
                    if (!r2) expect(ring2 == (p.lazy_end && any_x2), "fresh: the ring behind the call");
                }
}

void walk_predicates_and_open()
{
    long calls = 0;
    for (int x2 = 0; x2 <= 1; ++x2)
        for (unsigned m = 0; m < (1u << 12); ++m)
            for (int a = 0; a < 3; ++a)         // pair 0 / 1 / 2, or x4 0 / 1 / 3
                for (int bsel = 0; bsel < (x2 ? 3 : 2); ++bsel)   // block count 1 / 2, or the smallest extent 0 / 2 / 5
                    for (int mode = 0; mode < 4; ++mode) {
                        StepFacts f = base_facts();
                        unsigned b = m;
                        auto bit = [&] { const bool v = b & 1u; b >>= 1; return v; };
                        f.use_graph = bit(); f.tr_step = bit(); f.use_tracers = bit(); f.has_comm = bit(); f.march = bit();
                        Kc kc{mode, false, false};
                        if (x2) {   // the facts x4_now reads
                            f.has_exchange = true;
                            kc.x4_dev_ok = bit(); kc.fb_x2 = bit();
                            f.x4_tab_ok = bit(); f.known_const = bit(); f.r8_handed = bit(); f.remote_peers = bit();
                            f.x4_pitch_ok = bit();
                            f.x4 = a == 2 ? 3 : a;
                            f.min_extent = bsel == 0 ? 0 : bsel == 1 ? 2 : 5;
                        } else {    // the facts pair_ok and multi_ok read
                            f.forced = bit(); f.has_exchange = bit(); f.ring_sea = bit(); f.compact = bit();
                            f.multi = bit(); f.multi_fits = bit();
                            f.cells0 = bit() ? 4096L * 4096L : 100L * 100L;
                            f.pair = a;
                            f.nblocks = bsel + 1;
                        }
                        f.lazy = true;   // (open_goes_on is the caller's; the plan does not read it)
                        const bool pairs = pairs_now(f, kc, x2 != 0), known = mode == OCN_KC_KNOWN || mode == OCN_KC_KNOWN_HR;
                        expect(!pairs || mode != OCN_KC_DEVICE, "pairs with the variant chosen on the device");
                        expect(!pairs || x2 || (!f.forced && f.pair && f.nblocks == 1 && !f.has_exchange && !f.has_comm &&
                                                !f.ring_sea && !f.use_tracers),
                               "pair_ok outside one plain block");
                        expect(!pairs || !x2 || (known && (f.has_comm || f.min_extent >= 3)), "x4_now without a known-constant variant or on tiny blocks");
                        for (int ce = 0; ce <= 3; ++ce)
                            expect(!multi_ok(f, mode, ce) || (mode != OCN_KC_DEVICE && ce <= 1 && f.nblocks == 1 && f.multi_fits),
                                   "multi_ok");
                        expect(!await_kc_pays(f, kc, x2 != 0, 3) && (mode == OCN_KC_DEVICE || !await_kc_pays(f, kc, x2 != 0, 7)),
                               "await_kc_pays for a short call or a variant already chosen");
                        for (int d = 0; d <= 2; ++d)
                            for (int dcs = 0; dcs < (1 << d); ++dcs)
                                for (int nsteps = 1; nsteps <= 7; ++nsteps)
                                    for (int ce = 0; ce <= 3; ++ce) {
                                        const bool dc[2] = {(dcs & 1) != 0, (dcs & 2) != 0};
                                        bool want[16], got[16];
                                        int nwant = 0, ngot = 0, run = 0;
                                        for (int j = 0; j < d; ++j) want[nwant++] = dc[j];
                                        for (int s = 1; s <= nsteps; ++s) want[nwant++] = check_at(s, ce);
                                        bool first = true;
                                        const OpenPlan p = plan_open(f, kc, x2 != 0, d, dc, nsteps, ce, [&](const StepKind &k, bool graph) {
                                            kind_rules(k);
                                            expect(!k.last && !k.first && k.one && k.flip && k.next_one && !k.x2_save && !k.x2_end,
                                                   "open: a kind that is no continuing one-pass step");
                                            expect(k.x2 == (x2 != 0), "open: x2");
                                            expect(!k.multi || (!x2 && mode != OCN_KC_DEVICE && !graph && k.multi == nsteps),
                                                   "open: a multi-step kind in an x2 sequence, with a device-chosen variant or in a graph");
                                            expect(!k.pair || pairs, "open: a pair without pairs");
                                            expect(!graph || graph_ok(f), "open: a graph where none may replay");
                                            expect(!(first && d && !pairs) || !graph, "open: a deferred single step in a graph");
                                            first = false;
                                            for (int j = 0; j < steps_of(k) && ngot < 16; ++j) got[ngot++] = j == 1 && k.pair ? k.check2 : k.check;
                                            run += steps_of(k);
                                            return true;
                                        });
                                        ++calls;
                                        expect(run + p.deferred == d + nsteps, "open: steps run + newly deferred = deferred + nsteps");
                                        expect(p.mode == kOpenPairs ? p.deferred == 1 || p.deferred == 2 : p.deferred == 0, "open: newly deferred");
                                        expect((p.mode == kOpenPairs) == pairs && p.go == (d == 0), "open: mode / go");
                                        for (int j = 0; j < p.deferred && ngot < 16; ++j) got[ngot++] = p.deferred_check[j];
                                        expect(ngot == nwant && !memcmp(got, want, (size_t)nwant * sizeof(bool)), "open: the checks in step order");
                                    }
                    }
    printf("open: %ld calls planned\n", calls);
}

void walk_tail()
{
    for (int d = 0; d <= 2; ++d)
        for (int dcs = 0; dcs < 4; ++dcs)
            for (int m = 0; m < 16; ++m) {
                const bool dc[2] = {(dcs & 1) != 0, (dcs & 2) != 0}, open_pair = m & 1, x2 = m & 2, pok = m & 4, r2 = m & 8;
                const TailPlan t = plan_tail(d, dc, open_pair, x2, pok, r2);
                expect(t.n >= 1 && t.n <= 3, "tail: at most three kinds");
                int run = 0;
                for (int i = 0; i < t.n; ++i) { kind_rules(t.k[i]); run += steps_of(t.k[i]); expect(!t.k[i].multi && !t.k[i].x2_save, "tail: kinds"); }
                const StepKind &l = t.k[t.n - 1];
                expect(l.last && l.one_last && !l.flip, "tail: the final kind is a last step");
                expect(t.n == 1 || (t.k[0].one && !t.k[0].last && !t.k[0].pair && t.k[0].x2 == x2), "tail: the step ahead of the last one");
                expect(run == (d ? d : open_pair ? 2 : 1) && t.swap_back == (d == 0), "tail: the steps it runs");
                expect(l.pair ? pok && !l.x2_end && t.ring2_saved == r2 : l.x2_end == r2 && !t.ring2_saved, "tail: the x2 ring");
                expect(l.pair ? l.check == (d && dc[0]) && l.check2 == (d && dc[1]) : l.check == (d && dc[d - 1]), "tail: checks");
            }
}

// fresh call -> up to two open calls -> tail: every x2_save is met by one x2_end, the tail's final kind has last
void walk_chains()
{
    long chains = 0;
    for (int x2 = 0; x2 <= 1; ++x2)
        for (int pairs = 0; pairs <= 1; ++pairs)
            for (int n0 = 1; n0 <= 7; ++n0)
                for (int n1 = 0; n1 <= 7; ++n1)
                    for (int n2 = 0; n2 <= (n1 ? 7 : 0); ++n2)
                        for (int ce = 0; ce <= 3; ++ce) {
                            StepFacts f = base_facts();
                            f.multi = false;
                            if (x2) { f.has_exchange = true; f.nblocks = 2; }
                            const Kc kc{pairs ? OCN_KC_KNOWN : OCN_KC_GENERAL, false, true};
                            const FreshPlan p = fresh_pairs(f, plan_fresh(f, Vote{true, true, true, x2 != 0}, n0), kc);
                            if (!p.lazy_end) { expect(false, "chain: the fresh call leaves no tail"); continue; }
                            expect(p.x2_call == (x2 != 0) && p.pairs == (pairs != 0), "chain: the fresh call's form");
                            int saves = 0, ends = 0, d = 0;
                            bool ring2 = false, open_pair = false, dc[2] = {false, false};
                            auto count = [&](const StepKind &k) { saves += k.x2_save; ends += k.x2_end; };
                            for (int s = 1; s <= n0;) {
                                const FreshStep st = fresh_step(p, s, ce, ring2);
                                count(st.k);
                                ring2 = st.ring2_saved;
                                s += st.steps;
                            }
                            for (int n : {n1, n2}) {
                                if (!n) continue;
                                const OpenPlan o = plan_open(f, kc, p.x2_call, d, dc, n, ce, [&](const StepKind &k, bool) {
                                    count(k);
                                    open_pair = k.pair;
                                    return true;
                                });
                                d = o.deferred; dc[0] = o.deferred_check[0]; dc[1] = o.deferred_check[1];
                            }
                            const TailPlan t = plan_tail(d, dc, open_pair, p.x2_call, pair_ok(f, kc.mode), ring2);
                            for (int i = 0; i < t.n; ++i) count(t.k[i]);
                            expect(saves == ends && saves == (x2 ? 1 : 0) && !t.ring2_saved, "chain: the x2 ring's saves and ends balance");
                            expect(t.k[t.n - 1].last, "chain: the tail's final kind has last");
                            ++chains;
                        }
    printf("chains: %ld\n", chains);
}

}  // namespace

// the whole walk; returns the number of violated checks (the first 20 named on stderr)
extern "C" long sp_walk(long *checked)
{
    g_bad = g_checked = 0;
    walk_fresh();
    walk_predicates_and_open();
    walk_tail();
    walk_chains();
    if (checked) *checked = g_checked;
    return g_bad;
}

#ifdef STEP_PLAN_MAIN
int main()
{
    long checked = 0;
    const long bad = sp_walk(&checked);
    printf("step plan walk: %ld checks, %ld violated\n", checked, bad);
    return bad ? 1 : 0;
}
#endif
